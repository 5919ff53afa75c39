"""Scene import: a folder of images plus a COLMAP sparse model -> the scene layout eval.py -d scene reads.

  python mdf-net_amd/tools/colmap/main.py --model SPARSE_DIR --images IMAGE_DIR --out ROOT/SCENE [--nsrc 10]
         [--theta0 5 --sigma1 1 --sigma2 10] [--quantiles 0.01,0.99] [--max_dim 0] [--undistort [--undistort_fit inside|same]]

The model (text or binary) gives the cameras, the sparse points and their tracks.  Its cameras are PINHOLE / SIMPLE_PINHOLE; with
--undistort also SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV and OPENCV_FISHEYE, whose images are resampled to a pinhole camera on
the GPU (ops.undistort_images, tools/colmap/undistort.py) and whose cam files carry that camera: zoomed until no border pixel falls
outside the photograph (--undistort_fit inside, the default) or at the photograph's own focal length, black where it has nothing
(same).  Without the flag such a model is refused with the advice to undistort first.  On the GPU (ops.view_scores, ops.view_depth_ranges) every image pair is scored by the triangulation
angles of the points it shares and every image gets the depth range its own observations span; the host picks the --nsrc best
sources per image.  Written under --out:
  images/%08d.jpg    ids dense 0..N-1 in ascending COLMAP image id.  --max_dim D scales an image whose longer side exceeds D down
                     to it (the first two rows of K scale by the same factor); then the image is cropped at the bottom and right to
                     multiples of 32, which leaves K unchanged.  A JPEG that needs neither is copied byte for byte.
  cams/%08d_cam.txt  extrinsic, intrinsic, `depth_min depth_max` on line 11 (floats written with repr)
  pair.txt           per image its sources and their scores
  index.txt          id, COLMAP image id, file name
Images without observations are left out."""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != _HERE]     # select.py here must not stand in for the stdlib's select
_TOP = os.path.dirname(os.path.dirname(_HERE))     # mdf-net_amd/
if _TOP not in sys.path:
    sys.path.insert(0, _TOP)

import argparse  # noqa: E402
import shutil  # noqa: E402

import numpy as np  # noqa: E402

from tools.colmap import model_io, undistort as undist  # noqa: E402
from tools.colmap.select import select_views  # noqa: E402

MULTIPLE = 32


def write_cam(path, rot, trans, K, depth_min, depth_max):
    e = np.eye(4, dtype=np.float64)
    e[:3, :3], e[:3, 3] = rot, trans
    rows = lambda m: "".join(" ".join(repr(float(x)) for x in r) + "\n" for r in m)
    with open(path, "w") as f:
        f.write("extrinsic\n" + rows(e) + "\nintrinsic\n" + rows(np.asarray(K, dtype=np.float64)) + "\n"
                + repr(float(depth_min)) + " " + repr(float(depth_max)) + "\n")


def write_pairs(path, score, sources):
    with open(path, "w") as f:
        f.write(f"{len(sources)}\n")
        for i, srcs in enumerate(sources):
            f.write(f"{i}\n{len(srcs)} " + " ".join(f"{int(j)} {float(score[i, j])!r}" for j in srcs) + "\n")


def export_image(src, dst, K, max_dim=0):
    """Write src as the JPEG dst, scaled down to max_dim (if > 0 and the longer side exceeds it) and cropped at the bottom and right
    to multiples of 32.  -> (K of the written image, (width, height))."""
    from PIL import Image
    K = np.array(K, dtype=np.float64)
    with Image.open(src) as im:
        w, h = im.size
        s = float(max_dim) / max(w, h) if max_dim > 0 and max(w, h) > max_dim else 1.0
        sw, sh = (max(int(round(w * s)), 1), max(int(round(h * s)), 1)) if s != 1.0 else (w, h)
        cw, ch = sw // MULTIPLE * MULTIPLE, sh // MULTIPLE * MULTIPLE
        if cw == 0 or ch == 0:
            raise SystemExit(f"{src}: {sw} x {sh} pixels leave nothing after the crop to multiples of {MULTIPLE}")
        if s == 1.0 and (cw, ch) == (w, h) and im.format == "JPEG":
            shutil.copyfile(src, dst)
        else:
            out = im.convert("RGB")
            if s != 1.0:
                out = out.resize((sw, sh), Image.BILINEAR)
            out.crop((0, 0, cw, ch)).save(dst, format="JPEG", quality=95)
    K[:2] *= s
    return K, (cw, ch)


def import_scene(model_dir, image_dir, out_dir, nsrc=10, theta0=5.0, sigma1=1.0, sigma2=10.0, quantiles=(0.01, 0.99), max_dim=0,
                 device=None, log=print, undistort=False, undistort_fit="inside"):
    """-> dict with score [N,N], shared [N,N], range [N,2], count [N], sources [N,k] (numpy) and the scene arrays.  undistort: read
    the distorted camera models too and resample their images (tools/colmap/undistort.py); a pinhole camera's images are exported
    as without it."""
    import torch
    from mdfnet_hip import ops
    if undistort_fit not in undist.FITS:
        raise SystemExit(f"--undistort_fit {undistort_fit!r}: one of {', '.join(undist.FITS)}")
    scene = model_io.scene_arrays(model_io.read_model(model_dir, distorted=undistort), log=log)
    n = len(scene["names"])
    if n == 0:
        raise SystemExit(f"{model_dir}: no image with observations")
    device = device or torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    g = {k: torch.from_numpy(np.ascontiguousarray(scene[k])).to(device) for k in ("rot", "trans", "pts", "track_off", "track_img")}
    score, shared = ops.view_scores(g["rot"], g["trans"], g["pts"], g["track_off"], g["track_img"], theta0, sigma1, sigma2)
    rng, count = ops.view_depth_ranges(g["rot"], g["trans"], g["pts"], g["track_off"], g["track_img"], quantiles)
    score, shared, rng, count = score.cpu().numpy(), shared.cpu().numpy(), rng.cpu().numpy(), count.cpu().numpy()
    sources = select_views(score, nsrc)
    for sub in ("images", "cams"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    paths = [os.path.join(image_dir, name) for name in scene["names"]]
    for i, src in enumerate(paths):
        if not os.path.exists(src):
            raise SystemExit(f"{src}: the image of COLMAP image {int(scene['colmap_ids'][i])} is missing")
    written_K = {}                                          # image -> K_out, for the images of distorted cameras
    for cam_id in sorted(set(int(c) for c in scene["camera_ids"])):          # one plan (and one zoom fit) per camera
        members = [i for i in range(n) if int(scene["camera_ids"][i]) == cam_id]
        camera = scene["cameras"][members[0]]
        if camera[0] in model_io.SUPPORTED_MODELS:
            continue
        what = f"camera {cam_id} ({camera[0]})"
        p = undist.plan(camera, max_dim, undistort_fit, what)
        undist.export_images([(paths[i], os.path.join(out_dir, "images", "%08d.jpg" % i)) for i in members], p, device, what, log)
        written_K.update((i, p["K_out"]) for i in members)
    with open(os.path.join(out_dir, "index.txt"), "w") as index:
        for i in range(n):
            K = written_K[i] if i in written_K else export_image(paths[i], os.path.join(out_dir, "images", "%08d.jpg" % i), scene["K"][i], max_dim)[0]
            if not rng[i, 0] > 0:
                log(f"image {i}: depth range starts at {rng[i, 0]!r}; points behind the camera?")
            write_cam(os.path.join(out_dir, "cams", "%08d_cam.txt" % i), scene["rot"][i], scene["trans"][i], K, rng[i, 0], rng[i, 1])
            index.write(f"{i} {int(scene['colmap_ids'][i])} {scene['names'][i]}\n")
    write_pairs(os.path.join(out_dir, "pair.txt"), score, sources)
    log(f"{out_dir}: {n} images, {len(scene['pts'])} points, {len(scene['track_img'])} observations, {sources.shape[1]} sources per image")
    return dict(scene, score=score, shared=shared, range=rng, count=count, sources=sources)


def build_parser():
    parser = argparse.ArgumentParser(description="import a scene from a COLMAP sparse model")
    parser.add_argument("--model", required=True, type=str, help="folder with cameras/images/points3D .txt or .bin")
    parser.add_argument("--images", required=True, type=str, help="folder the model's image names are relative to")
    parser.add_argument("--out", required=True, type=str, help="ROOT/SCENE to write")
    parser.add_argument("--nsrc", default=10, type=int)
    parser.add_argument("--theta0", default=5.0, type=float)
    parser.add_argument("--sigma1", default=1.0, type=float)
    parser.add_argument("--sigma2", default=10.0, type=float)
    parser.add_argument("--quantiles", default="0.01,0.99", type=str)
    parser.add_argument("--max_dim", default=0, type=int)
    parser.add_argument("--undistort", action="store_true", help="read SIMPLE_RADIAL / RADIAL / OPENCV / FULL_OPENCV / OPENCV_FISHEYE "
                        "cameras too and resample their images to a pinhole camera on the GPU")
    parser.add_argument("--undistort_fit", default="inside", choices=undist.FITS, help="inside: zoom until no border pixel falls outside "
                        "the photograph; same: keep the focal length, pixels the photograph does not cover stay black")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    q = tuple(float(x) for x in args.quantiles.split(","))
    if len(q) != 2:
        raise SystemExit(f"--quantiles {args.quantiles!r}: two comma-separated values")
    import_scene(args.model, args.images, args.out, args.nsrc, args.theta0, args.sigma1, args.sigma2, q, args.max_dim,
                 undistort=args.undistort, undistort_fit=args.undistort_fit)


if __name__ == "__main__":
    main()
