"""Point-cloud fusion with visibility and small-segment filters (counterpart of the reference's tools/pcd/fusion.py).

Per scan: the probability filter (prob > 0.8), the visibility filter, visibility fusion, the visibility filter, average fusion,
the visibility filter and the small-segment filter run as ONE ops.pcd_fuse call with every view resident on the GPU
(mdf_pcd_fuse_fwd), then the mask-true pixels are lifted to world points and written to {out}/{scan}.ply (or
{eval}/{scan}/{filter}/{scan}.ply without -o).  Images are read with PIL and cropped top-left to the depth maps' size.
Scans shard over ranks (one process per GPU, no collective).

This entry point runs stages 1-6 only: main() refuses a call without --no_normal or with --downsample.  Normal estimation
and voxel downsampling (stages 7 and 8, ops.pcd_fuse(normals=, downsample=)) run from tools/pcd/cloud.py, which takes the same
arguments with the reference's defaults and shares build_parser(), run() and get_cloud() with this file.

  python mdf-net_amd/tools/pcd/fusion.py -r DATA_ROOT -e OUTPUTS -o PLY_DIR -d tanks -s intermediate --no_normal
"""
import argparse
import os
import sys
import time

_TOP = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # mdf-net_amd/
if _TOP not in sys.path:
    sys.path.insert(0, _TOP)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.data_io import read_pfm, read_cam_file, write_ply  # noqa: E402

TANKS_SCANS = {"intermediate": ["Family", "Francis", "Horse", "Lighthouse", "M60", "Panther", "Playground", "Train"],
               "advanced": ["Auditorium", "Ballroom", "Courtroom", "Museum", "Palace", "Temple"]}
DTU_SCANS = [11]


def load_pair(path):
    """pair.txt -> (ids [str], {id: [source ids, best first]}) (utils.load_pair)."""
    with open(path) as f:
        lines = f.readlines()
    n = int(lines[0])
    ids, pairs = [], {}
    for i in range(1, 1 + 2 * n, 2):
        vid = lines[i].strip()
        tok = lines[i + 1].strip().split(" ")
        pairs[vid] = [tok[j] for j in range(1, 1 + 2 * int(tok[0]), 2)]
        ids.append(vid)
    return ids, pairs


def read_crop_rgb(path, h, w):
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"))
    return np.ascontiguousarray(img[:h, :w])


def load_scan(scan_location, eval_location, img_folder, cam_folder):
    """-> dict(ids, depths [N,H,W] f32, probs [N,H,W] f32, images [N,H,W,3] u8, K [N,3,3], E [N,4,4], srcs [[index] ...]):
    every view of pair.txt, its sources restricted to views of the scan (as get_cloud does)."""
    ids, pairs = load_pair(os.path.join(scan_location, "pair.txt"))
    depths, probs, images, Ks, Es = [], [], [], [], []
    for vid in ids:
        name = "{:0>8}".format(vid)
        depth = np.ascontiguousarray(read_pfm(os.path.join(eval_location, "depth_est", name + ".pfm"))[0], dtype=np.float32)
        prob = np.ascontiguousarray(read_pfm(os.path.join(eval_location, "confidence", name + ".pfm"))[0], dtype=np.float32)
        h, w = depth.shape
        k, e = read_cam_file(os.path.join(scan_location, cam_folder, name + "_cam.txt"))
        depths.append(depth)
        probs.append(prob)
        images.append(read_crop_rgb(os.path.join(scan_location, img_folder, name + ".jpg"), h, w))
        Ks.append(k)
        Es.append(e)
    index = {vid: i for i, vid in enumerate(ids)}
    srcs = [[index[s] for s in pairs[vid] if s in index] for vid in ids]
    return {"ids": ids, "depths": np.stack(depths), "probs": np.stack(probs), "images": np.stack(images), "K": np.stack(Ks),
            "E": np.stack(Es), "srcs": srcs}


def save_mask(path, mask):
    from PIL import Image
    Image.fromarray(mask.astype(np.uint8) * 255).save(path)


def get_cloud(dataset_root, scan, img_folder, cam_folder, eval_folder, args, device=None):
    from mdfnet_hip import ops
    device = device or torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    scan_location = os.path.join(dataset_root, scan)
    eval_location = os.path.join(eval_folder, scan)
    t0 = time.time()
    sc = load_scan(scan_location, eval_location, img_folder, cam_folder)
    t1 = time.time()
    g = lambda a: torch.from_numpy(a).to(device)
    out = ops.pcd_fuse(g(sc["depths"]), g(sc["probs"]), g(sc["images"]), sc["K"], sc["E"], sc["srcs"], view=args.view,
                       vthresh=args.vthresh, normals=not args.no_normal, downsample=args.downsample)
    xyz, rgb = out["xyz"].cpu().numpy(), out["rgb"].cpu().numpy()
    nrm = out["normals"].cpu().numpy() if "normals" in out else None
    t2 = time.time()
    if args.write_mask:
        os.makedirs(os.path.join(eval_location, args.filter_folder), exist_ok=True)
        masks = out["masks"].cpu().numpy()
        for i, vid in enumerate(sc["ids"]):
            save_mask(os.path.join(eval_location, args.filter_folder, "{:0>8}_mask.png".format(vid)), masks[i])
    if args.outply_folder is None:
        ply_path = os.path.join(eval_location, args.filter_folder, scan + ".ply")
    else:
        ply_path = os.path.join(args.outply_folder, scan + ".ply")
    os.makedirs(os.path.dirname(os.path.abspath(ply_path)), exist_ok=True)
    if nrm is not None:
        write_ply(ply_path, xyz, rgb, normals=nrm)
    else:
        write_ply(ply_path, xyz, rgb)
    if "voxel" in out:
        fused = int(out["counts"].sum().item())
        print(f"{scan}: downsampled {fused} -> {len(xyz)} points at voxel size {out['voxel']:.9g}")
    print(f"{scan}: {len(sc['ids'])} views, {len(xyz)} points (load {t1 - t0:.2f}s, fuse {t2 - t1:.2f}s) -> {ply_path}")
    return ply_path


def build_parser():
    parser = argparse.ArgumentParser(description="point-cloud fusion with visibility and small-segment filters")
    parser.add_argument("--view", type=int, default=10)
    parser.add_argument("--vthresh", type=int, default=4)
    parser.add_argument("--cam_scale", type=float, default=1)
    parser.add_argument("--downsample", type=float, default=None, help="voxel size, or -1 for the 90th percentile of the "
                        "nearest-neighbour spacing (cloud.py only)")
    parser.add_argument("--no_normal", action="store_true", default=False, help="skip normal estimation (required by fusion.py)")
    parser.add_argument("--write_mask", action="store_true", default=False)
    import config                       # the project's roots (MDF_DATA_ROOT, MDF_OUTPUT_ROOT), as eval.py writes them
    parser.add_argument("-r", "--root_folder", default=config.DATA_ROOT, type=str, help="dataset root location")
    parser.add_argument("-e", "--eval_folder", default=config.OUTPUT_ROOT, type=str, help="eval output location")
    parser.add_argument("-o", "--outply_folder", default=None, type=str, help="PLY folder (default: <eval>/<scan>/<filter>)")
    parser.add_argument("-d", "--dataset", default="tanks", type=str, help="dtu or tanks")
    parser.add_argument("-s", "--set", default="intermediate", type=str, help="tanks set: intermediate or advanced")
    parser.add_argument("-f", "--filter_folder", default="filter", type=str, help="filter output location")
    parser.add_argument("--scans", default=None, type=str, help="comma-separated scans (DTU numbers or Tanks names)")
    return parser


def run(args):
    """Fuse every scan the arguments name (this rank's share) -> the PLY paths written."""
    if args.dataset == "dtu":
        dataset_root = os.path.join(args.root_folder, "dtu1600x1200")
        labels = [s.strip() for s in args.scans.split(",")] if args.scans else [str(x) for x in DTU_SCANS]
        scans = ["scan" + s for s in labels]
        img_folder, cam_folder = "images", "cams"
    elif args.dataset == "tanks":
        if args.set not in TANKS_SCANS:
            raise SystemExit("tanks set: intermediate or advanced")
        dataset_root = os.path.join(args.root_folder, "TankandTemples", args.set)
        scans = [s.strip() for s in args.scans.split(",")] if args.scans else TANKS_SCANS[args.set]
        img_folder, cam_folder = "images", "cams_1"
    else:
        raise SystemExit("please use dtu or tanks dataset")
    from mdfnet_hip import shard
    rank, world, _ = shard.init()
    written = []
    for i in shard.shard_items(len(scans), rank, world):     # scans are independent: shard them, no collective
        t0 = time.time()
        written.append(get_cloud(dataset_root, scans[i], img_folder, cam_folder, args.eval_folder, args))
        print("scan:", scans[i], "all time:", (time.time() - t0) / 60, "min")
    shard.barrier()
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.no_normal or args.downsample is not None:
        raise SystemExit("normal estimation and voxel downsampling are not implemented in fusion.py: run it with --no_normal "
                         "and without --downsample, or run tools/pcd/cloud.py, which has both")
    return run(args)


if __name__ == "__main__":
    main()
