"""DTU / Tanks&Temples depth-map fusion driver (counterpart of the reference's tools/gipuma/main.py).

The reference filters the depth maps by probability (-f), converts cameras, images and depth maps for fusibile (-m, -g), runs
the CUDA-only fusibile binary (-d) and copies its PLY to the collection folder (-r).  Here -f happens in memory, -d is ONE call of
ops.consensus_fuse per scan (mdf_consensus_fuse_fwd: every view of the scan as the reference once, against every other view),
and the PLY is written straight to the output folder under the name the reference's -r step gives it: ours{scan:03d}_l3.ply
(DTU) or {scene}.ply.  Images are cropped top-left to the depth maps' size in memory (the reference's -c step).  There is no
.dmb / .P round trip, so -m and -g are accepted and do nothing.

  python mdf-net_amd/tools/gipuma/main.py -f -d -e OUTPUTS -r DATA_ROOT -o PLY_DIR [--dataset dtu --scans 1,4,9]
"""
import argparse
import logging
import os
import sys
import time

_TOP = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # mdf-net_amd/
if _TOP not in sys.path:
    sys.path.insert(0, _TOP)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.data_io import read_pfm, read_cam_file, write_ply  # noqa: E402
from tools.gipuma import conf  # noqa: E402

logging.basicConfig(level=logging.INFO, format="%(asctime)s-%(levelname)s: %(message)s")


def probability_filter(depth, prob, prob_threshold):
    """The reference's probability_filter: depth[prob < prob_threshold] = 0 (on a copy)."""
    depth = np.array(depth, dtype=np.float32, copy=True)
    depth[np.asarray(prob) < prob_threshold] = 0
    return depth


def read_crop_img(filename, h, w):
    """RGB uint8 [h, w, 3]: the image cropped top-left to the depth map's size."""
    from PIL import Image
    img = np.asarray(Image.open(filename).convert("RGB"))
    if img.shape[0] < h or img.shape[1] < w:
        raise ValueError(f"{filename}: image {img.shape[1]}x{img.shape[0]} is smaller than the depth map {w}x{h}")
    return np.ascontiguousarray(img[:h, :w])


def load_scan(scan_folder, eval_scan_folder, nviews, prob_threshold, prob_filter=True, img_folder="images", cam_folder="cams"):
    """-> (views, depths [N,H,W] f32, images [N,H,W,3] u8, K [N,3,3], E [N,4,4]) for every view with a depth map."""
    views, depths, images, Ks, Es = [], [], [], [], []
    for v in range(nviews):
        dpath = os.path.join(eval_scan_folder, "depth_est", "{:08d}.pfm".format(v))
        if not os.path.exists(dpath):
            continue
        depth = np.ascontiguousarray(read_pfm(dpath)[0], dtype=np.float32)
        if prob_filter:
            prob = read_pfm(os.path.join(eval_scan_folder, "confidence", "{:08d}.pfm".format(v)))[0]
            depth = probability_filter(depth, prob, prob_threshold)
        h, w = depth.shape
        k, e = read_cam_file(os.path.join(scan_folder, cam_folder, "{:08d}_cam.txt".format(v)))
        views.append(v)
        depths.append(depth)
        images.append(read_crop_img(os.path.join(scan_folder, img_folder, "{:08d}.jpg".format(v)), h, w))
        Ks.append(k)
        Es.append(e)
    if not views:
        raise FileNotFoundError(f"no depth maps under {eval_scan_folder}/depth_est")
    return views, np.stack(depths), np.stack(images), np.stack(Ks), np.stack(Es)


def fuse_scan(scan_folder, eval_scan_folder, out_ply, args, prob_filter=True, img_folder="images", cam_folder="cams",
              device=None):
    from mdfnet_hip import ops
    device = device or torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    t0 = time.time()
    views, depths, images, K, E = load_scan(scan_folder, eval_scan_folder, args["nviewss"], args["prob_threshold"], prob_filter,
                                            img_folder, cam_folder)
    t1 = time.time()
    xyz, rgb, counts = ops.consensus_fuse(torch.from_numpy(depths).to(device), torch.from_numpy(images).to(device), K, E,
                                          args["disp_threshold"], args["check_views"])
    xyz, rgb = xyz.cpu().numpy(), rgb.cpu().numpy()
    t2 = time.time()
    os.makedirs(os.path.dirname(os.path.abspath(out_ply)), exist_ok=True)
    write_ply(out_ply, xyz, rgb)
    logging.info("%s: %d views, %d points (load %.2fs, fuse %.2fs) -> %s", eval_scan_folder, len(views), len(xyz), t1 - t0,
                 t2 - t1, out_ply)
    return out_ply, len(xyz)


def main(argv=None):
    parser = argparse.ArgumentParser(description="dtu fusion parameter setting")
    parser.add_argument("-c", "--cut", action="store_true", help="(always done in memory: images are cropped to the depth maps)")
    parser.add_argument("-f", "--filter", action="store_true", help="filter depth_map with prob_map")
    parser.add_argument("-m", "--move", action="store_true", help="(not needed: no projection-matrix files)")
    parser.add_argument("-g", "--gipuma", action="store_true", help="(not needed: no .dmb depth / normal files)")
    parser.add_argument("-d", "--depth_fusion", action="store_true", help="depth map fusion on the GPU")
    parser.add_argument("--dataset", default="dtu", choices=["dtu", "tanks_intermediate", "tanks_advanced"])
    parser.add_argument("--scans", default="11", help="DTU scan numbers (comma separated) or Tanks scene names")
    import config                       # the project's roots (MDF_DATA_ROOT, MDF_OUTPUT_ROOT), as eval.py writes them
    parser.add_argument("-e", "--eval_folder", default=config.OUTPUT_ROOT,
                        help="eval outputs: <eval>/<scan>/depth_est/*.pfm, <eval>/<scan>/confidence/*.pfm")
    parser.add_argument("-r", "--root_dir", default=config.DATA_ROOT, help="dataset root")
    parser.add_argument("-o", "--out_folder", default=None, help="where the PLYs go (default: <eval>/oursply)")
    args = parser.parse_args(argv)
    if args.move or args.gipuma:
        print("-m / -g: not needed here (cameras and depth maps go to the GPU directly; no .P / .dmb files)")
    if args.dataset == "dtu":
        root = os.path.join(args.root_dir, "dtu1600x1200")
        scans = ["scan" + s.strip() for s in args.scans.split(",")]
        cam_folder = "cams"
    else:
        root = os.path.join(args.root_dir, "TankandTemples", args.dataset.split("_")[1])
        scans = [s.strip() for s in args.scans.split(",")]
        cam_folder = "cams_1"
    out_folder = args.out_folder or os.path.join(args.eval_folder, "oursply")
    written = []
    if not args.depth_fusion:
        print("nothing to do without -d (the probability filter runs in memory as part of the fusion)")
        return written
    for scan in scans:
        fa = conf.fusion_args(args.dataset, scan)
        logging.info("######current scan:%s nviews:%d check_view:%d prob_threshold:%s disp_threshold:%s", scan, fa["nviewss"],
                     fa["check_views"], fa["prob_threshold"], fa["disp_threshold"])
        name = "ours{:03d}_l3.ply".format(int(scan[4:])) if args.dataset == "dtu" else scan + ".ply"
        written.append(fuse_scan(os.path.join(root, scan), os.path.join(args.eval_folder, scan), os.path.join(out_folder, name), fa,
                                 prob_filter=args.filter, cam_folder=cam_folder)[0])
    return written


if __name__ == "__main__":
    main()
