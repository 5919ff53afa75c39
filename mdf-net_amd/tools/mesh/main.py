"""Mesh driver: the filter's depth maps of a scan -> a coloured triangle mesh <out>/<scan>_mesh.ply (no counterpart in the
reference, which stops at the point cloud; DESIGN section 7 "TSDF meshing").

Takes the flags of tools/filter/dynamic_filter_gpu.py (-f/-d/-s/-e/-r/-o/--scans; -d dtu|tanks|scene) and reads what it wrote:
<eval>/<scan>/<filter>/<ref>_depth_est.pfm (0 where the filter rejected a pixel) and <scan>.ply, plus the scan's cameras and
images.  The volume is the per-axis 1 %-99 % quantile box of the point cloud, grown by 5 % and by the truncation distance;
the depth maps are integrated into a truncated signed distance volume (ops.tsdf_integrate), its zero level set is extracted by
marching tetrahedra (ops.tsdf_mesh) and the vertices are coloured from the images (ops.mesh_colour): three groups of HIP kernels,
every view resident on the GPU.  Scans shard over ranks (one process per GPU, no collective)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

_TOP = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # mdf-net_amd/
if _TOP not in sys.path:
    sys.path.insert(0, _TOP)

from mdfnet_hip import ops, shard  # noqa: E402
from tools.data_io import read_pfm, read_pairfile, read_cam_file, read_ply, write_ply_mesh  # noqa: E402


class MissingFilterOutput(SystemExit):
    pass


def build_parser():
    parser = argparse.ArgumentParser(description="TSDF fusion of the filtered depth maps and marching tetrahedra: <scan>_mesh.ply")
    parser.add_argument("-f", "--filter_folder", default="filter", type=str)
    parser.add_argument("-d", "--dataset", default="tanks", type=str, help="dtu, tanks or scene")
    parser.add_argument("-s", "--set", default="intermediate", type=str)
    parser.add_argument("-e", "--eval_folder", default=os.environ.get("MDF_OUTPUT_ROOT", "/hy-tmp/outputs"), type=str)
    parser.add_argument("-r", "--root_folder", default=os.environ.get("MDF_DATA_ROOT", "/hy-nas"), type=str)
    parser.add_argument("-o", "--outply_folder", default=None, type=str)
    parser.add_argument("--scans", default="", type=str, help="-d scene: comma-separated scene folders under -r (tools/colmap/main.py)")
    parser.add_argument("--resolution", default=512, type=int, help="lattice points along the longest side of the volume")
    parser.add_argument("--voxel", default=None, type=float, help="voxel edge in world units (overrides --resolution)")
    parser.add_argument("--trunc", default=3.0, type=float, help="truncation distance in voxels")
    parser.add_argument("--min_weight", default=1, type=int, help="views that must have seen a lattice point for it to count")
    return parser


def scans_of(args):
    """-> (root, scans, img_folder, cam_folder), as tools/filter/dynamic_filter_gpu.py resolves them."""
    if args.dataset == "dtu":
        return (os.path.join(args.root_folder, "dtu1600x1200"), ["scan" + s for s in os.environ.get("MDF_DTU_SCANS", "11").split(",")],
                "images", "cams")
    if args.dataset == "tanks":
        scans = {"intermediate": ["Family", "Francis", "Horse", "Lighthouse", "M60", "Panther", "Playground", "Train"],
                 "advanced": ["Auditorium", "Ballroom", "Courtroom", "Museum", "Palace", "Temple"]}[args.set]
        return os.path.join(args.root_folder, "TankandTemples", args.set), scans, "images", "cams_1"
    if args.dataset == "scene":
        scans = [s for s in args.scans.split(",") if s]
        if not scans:
            raise SystemExit("-d scene needs --scans a,b (folders under -r)")
        return args.root_folder, scans, "images", "cams"
    raise SystemExit("please use dtu, tanks or scene dataset")


def check_args(args):
    if args.voxel is not None and not (args.voxel > 0 and np.isfinite(args.voxel)):
        raise SystemExit(f"--voxel {args.voxel}: a finite positive edge length is needed")
    if not (args.trunc > 0 and np.isfinite(args.trunc)):
        raise SystemExit(f"--trunc {args.trunc}: a positive number of voxels is needed")
    if args.voxel is None and args.resolution - 1 - 2 * args.trunc < 1:
        raise SystemExit(f"--resolution {args.resolution} leaves no room between two truncation bands of {args.trunc} voxels")
    if args.min_weight < 1:
        raise SystemExit(f"--min_weight {args.min_weight}: at least 1")


def mesh_box(points, resolution=512, voxel=None, trunc=3.0):
    """HOST: the volume of a point cloud [M,3] -> (origin float32 [3], voxel float32, dims (nx,ny,nz), trunc float32 in world units).
    The per-axis 1 %-99 % quantile box, grown by 5 % of its extent on every side and then by the truncation distance; without
    `voxel` the longest side holds exactly `resolution` lattice points."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    if len(pts) == 0:
        raise ValueError("the point cloud is empty")
    lo, hi = np.quantile(pts, 0.01, axis=0), np.quantile(pts, 0.99, axis=0)
    grow = 0.05 * (hi - lo)
    lo, hi = lo - grow, hi + grow
    longest = float((hi - lo).max())
    if voxel is None:
        voxel = longest / (resolution - 1 - 2 * trunc) if longest > 0 else 1.0
    voxel = np.float32(voxel)
    tau = np.float32(np.float32(trunc) * voxel)
    lo, hi = lo - float(tau), hi + float(tau)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / float(voxel) - 1e-4)) + 1 for a in range(3))     # (1e-4: the fp32 rounding of voxel)
    return lo.astype(np.float32), voxel, dims, tau


def filter_command(args, scan):
    extra = f" --scans {scan}" if args.dataset == "scene" else (f" -s {args.set}" if args.dataset == "tanks" else "")
    out = f" -o {args.outply_folder}" if args.outply_folder else ""
    return (f"python mdf-net_amd/tools/filter/dynamic_filter_gpu.py -d {args.dataset} -r {args.root_folder} -e {args.eval_folder} "
            f"-f {args.filter_folder}{out}{extra}")


def load_scan(args, root, scan, img_folder, cam_folder):
    """-> dict(depths [V,h,w] f32, images [V,h,w,3] u8, K [V,3,3], E [V,4,4], points [M,3]) on the host; raises MissingFilterOutput
    naming the command that writes what is missing."""
    from PIL import Image
    scan_location = os.path.join(root, scan)
    eval_location = os.path.join(args.eval_folder, scan)
    workspace = os.path.join(eval_location, args.filter_folder)
    ply = os.path.join(args.outply_folder or eval_location, scan + ".ply")
    pair = os.path.join(scan_location, "pair.txt")
    if not os.path.exists(pair):
        raise SystemExit(f"{pair} not found: -r / --scans do not point at an imported scan")
    views = [ref for ref, srcs in read_pairfile(pair)[1] if len(srcs)]
    maps = {v: os.path.join(workspace, f"{v}_depth_est.pfm") for v in views}
    missing = [p for p in list(maps.values()) + [ply] if not os.path.exists(p)]
    if missing or not views:
        raise MissingFilterOutput(f"{scan}: the filter's outputs are missing ({len(missing)} files, first: {(missing or [workspace])[0]}).\n"
                                  f"They are written by:  {filter_command(args, scan)}")
    depths, images, Ks, Es = [], [], [], []
    for v in views:
        d = np.ascontiguousarray(read_pfm(maps[v])[0], dtype=np.float32)
        k, e = read_cam_file(os.path.join(scan_location, cam_folder, "{:0>8}_cam.txt".format(v)))
        img = np.array(Image.open(os.path.join(scan_location, img_folder, "{:0>8}.jpg".format(v))).convert("RGB"), dtype=np.uint8)
        h, w = d.shape
        if img.shape[0] < h or img.shape[1] < w:
            raise SystemExit(f"{scan}: image {v} is {img.shape[1]}x{img.shape[0]}, smaller than its {w}x{h} depth map")
        if depths and depths[0].shape != d.shape:
            raise SystemExit(f"{scan}: depth map {v} is {w}x{h}, the first is {depths[0].shape[1]}x{depths[0].shape[0]}; one size is needed")
        depths.append(d)
        images.append(np.ascontiguousarray(img[:h, :w]))
        Ks.append(k)
        Es.append(e)
    return {"depths": np.stack(depths), "images": np.stack(images), "K": np.stack(Ks), "E": np.stack(Es), "points": read_ply(ply)[0]}


def mesh_scan(args, root, scan, img_folder, cam_folder, device=None, log=print):
    device = device or torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    sc = load_scan(args, root, scan, img_folder, cam_folder)
    origin, voxel, dims, tau = mesh_box(sc["points"], args.resolution, args.voxel, args.trunc)
    depths = torch.from_numpy(sc["depths"]).to(device)
    images = torch.from_numpy(sc["images"]).to(device)
    D, W = ops.tsdf_integrate(depths, sc["K"], sc["E"], origin, voxel, dims, tau)
    vertices, triangles = ops.tsdf_mesh(D, W, origin, voxel, args.min_weight)
    del D, W
    rgb = ops.mesh_colour(vertices, depths, images, sc["K"], sc["E"], tau)
    out_dir = args.outply_folder or os.path.join(args.eval_folder, scan)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, scan + "_mesh.ply")
    write_ply_mesh(path, vertices.cpu().numpy(), rgb.cpu().numpy(), triangles.cpu().numpy())
    log(f"{scan}: {len(sc['depths'])} views, volume {dims[0]}x{dims[1]}x{dims[2]} at voxel {float(voxel):.6g}, "
        f"{vertices.shape[0]} vertices, {triangles.shape[0]} triangles -> {path}")
    return path


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    root, scans, img_folder, cam_folder = scans_of(args)
    rank, world, _ = shard.init()
    for i in shard.shard_items(len(scans), rank, world):     # scans are independent: shard them, no collective
        t0 = time.time()
        mesh_scan(args, root, scans[i], img_folder, cam_folder)
        print("scan:", scans[i], "all time:", time.time() - t0)
    shard.barrier()


if __name__ == "__main__":
    main()
