"""Generate tests/golden/pcd_fusion.npz from the REAL reference's tools/pcd/fusion.py:get_cloud (build container only).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_pcd_golden.py

Imports the reference's tools/pcd/fusion.py and utils/utils.py from MDF_REFERENCE (read-only; never copied) and runs get_cloud
on a seeded 8-view 64x80 scene (oracle.gen_golden.filter_scene, written to a temporary dataset / eval tree), with
  - cv2: imread returns the scene's images (BGR), imwrite does nothing;
  - open3d: a point-cloud stand-in that records the points and colours get_cloud hands it (run with --no_normal);
  - tqdm: the iterable itself;
  - torch.utils.cpp_extension.load: tests/pcd_oracle.py's restatements of fusion.cpp's two cores (nothing is compiled);
  - Tensor.cuda: identity (this box has no GPU).
vis_fusion_core's violation counts (every candidate's) are recorded too.  The state after every stage is recorded by wrapping the module's stage functions: batch_vis_filter's entry and exit, the
per-view small-segment masks, and the depth handed to the back projection.  Camera 7 is moved 650 along its optical axis, so
part of the scene lies behind it."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MDF_REFERENCE", "/root/reference")
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcd_oracle as O  # noqa: E402
from tools.data_io import save_pfm  # noqa: E402

N, H, W, SEED, BEHIND = 8, 64, 80, 17, 7


def scene():
    from oracle.gen_golden import filter_scene
    depths, _, K, E = filter_scene(h=H, w=W, nsrc=N - 1, seed=SEED)
    rng = np.random.RandomState(SEED)
    E = E.copy()
    E[BEHIND, 2, 3] -= 650.0                 # camera z' = z - 650: points nearer than 650 are behind it
    probs = rng.uniform(0.7, 1.0, depths.shape).astype(np.float32)
    v, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    images = (np.stack([3 * x + 7 * v, 5 * y + 11 * v, x + y + 13 * v], -1) % 256).astype(np.uint8)   # compressible colours
    srcs = [sorted((j for j in range(N) if j != i), key=lambda j: (abs(i - j), j)) for i in range(N)]
    return depths, probs, images, K, E, srcs


def write_tree(tmp, depths, probs, images, K, E, srcs):
    scan = "scan1"
    sd, ev = os.path.join(tmp, "data", scan), os.path.join(tmp, "eval", scan)
    for d in (os.path.join(sd, "images"), os.path.join(sd, "cams"), os.path.join(ev, "depth_est"), os.path.join(ev, "confidence"),
              os.path.join(ev, "filter")):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(sd, "pair.txt"), "w") as f:
        f.write(f"{N}\n")
        for i in range(N):
            s = srcs[i] + [N + 5]            # a view outside the scan: get_cloud skips it
            f.write(f"{i}\n{len(s)} " + " ".join(f"{j} {50 - k}.0" for k, j in enumerate(s)) + "\n")
    imgs = {}
    for i in range(N):
        name = f"{i:08d}"
        save_pfm(os.path.join(ev, "depth_est", name + ".pfm"), depths[i])
        save_pfm(os.path.join(ev, "confidence", name + ".pfm"), probs[i])
        imgs[os.path.join(sd, "images", name + ".jpg")] = np.ascontiguousarray(images[i][:, :, ::-1])   # cv2 reads BGR
        with open(os.path.join(sd, "cams", name + "_cam.txt"), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in E[i]) + "\n\n")
            f.write("intrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in K[i]) + "\n\n425.0 2.5\n")
    return os.path.join(tmp, "data"), scan, os.path.join(tmp, "eval"), imgs


def stub_modules(imgs, cloud, cands=None):
    def vis_fusion_core(all_d, xy, violation, valid):
        if cands is not None:                        # the reference's candidates of this reference view, in its order
            cands.append((all_d.numpy().copy(), violation.numpy().copy()))
        out = O.vis_fusion_core(all_d.numpy(), xy[:, 0].numpy(), xy[:, 1].numpy(), violation.numpy(), valid.numpy())
        return torch.from_numpy(out)

    def small_seg_core(depth, window_size, diff_thresh, size_thresh):
        return torch.from_numpy(O.small_seg_core(depth.numpy(), window_size, diff_thresh, size_thresh))

    cpp = types.ModuleType("torch.utils.cpp_extension")
    cpp.load = lambda *a, **k: types.SimpleNamespace(vis_fusion_core=vis_fusion_core, small_seg_core=small_seg_core)
    sys.modules["torch.utils.cpp_extension"] = cpp
    sys.modules["cv2"] = types.SimpleNamespace(imread=lambda p: imgs[p], imwrite=lambda *a: True)
    sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, *a, **k: it)

    class PointCloud:
        def __init__(self):
            cloud.append(self)

        def estimate_normals(self):
            raise RuntimeError("run with --no_normal")
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a))
    o3d.io = types.SimpleNamespace(write_point_cloud=lambda *a, **k: True)
    sys.modules["open3d"] = o3d
    torch.Tensor.cuda = lambda self, *a, **k: self


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pcd_fusion.npz"))
    a = ap.parse_args()
    depths, probs, images, K, E, srcs = scene()
    cloud, rec = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        data, scan, ev, imgs = write_tree(tmp, depths, probs, images, K, E, srcs)
        cands = []
        stub_modules(imgs, cloud, cands)
        pdir = os.path.join(REF, "tools", "pcd")
        sys.path.insert(0, pdir)
        cwd = os.getcwd()
        os.chdir(pdir)
        import fusion as R                               # the reference's tools/pcd/fusion.py
        os.chdir(cwd)
        sys.path.remove(pdir)

        def state(views):
            ids = sorted((k for k in views if k != "id_list"), key=int)
            return (np.stack([views[i]["depth"][0, 0].numpy() for i in ids]), np.stack([views[i]["mask"][0, 0].numpy() for i in ids]))
        names = iter([("prob", "vis1"), ("vis_fusion", "vis2"), ("ave", "vis3")])
        orig_bvf = R.batch_vis_filter

        def batch_vis_filter(views, pair, args):
            before, after = next(names)
            rec[before] = state(views)
            orig_bvf(views, pair, args)
            rec[after] = state(views)
        R.batch_vis_filter = batch_vis_filter
        segs = []
        orig_seg = R.small_seg_filter
        R.small_seg_filter = lambda *x: segs.append(orig_seg(*x)) or segs[-1]
        final_depths = []
        orig_i2c = R.idx_img2cam
        R.idx_img2cam = lambda idx, depth, cam: final_depths.append(depth[0, 0].numpy().copy()) or orig_i2c(idx, depth, cam)
        args = argparse.Namespace(view=10, vthresh=4, cam_scale=1, downsample=None, no_normal=True, write_mask=False,
                                  outply_folder=tmp, filter_folder="filter")
        R.get_cloud(data, scan, "images", "cams", ev, 0.8, args)
    seg_mask = rec["vis3"][1] & np.stack([s.numpy() for s in segs])
    rec["seg"] = (np.stack(final_depths), seg_mask)
    pc = cloud[-1]
    out = {"depths": depths, "probs": probs, "images": images, "K": K, "E": E,
           "srcs": O.src_table(srcs, N, 10)[:, :N - 1], "vthresh": np.int32(4), "behind_view": np.int32(BEHIND),
           "points": np.asarray(pc.points, dtype=np.float32), "colors": np.asarray(pc.colors, dtype=np.float32)}
    # visibility fusion's candidates per reference view (reference view order): their count and violation counts
    out["cand_counts"] = np.array([len(d) for d, _ in cands], dtype=np.int32)
    out["cand_violations"] = np.concatenate([v for _, v in cands]).astype(np.int8)
    for k, (d, m) in rec.items():
        out["depth_" + k], out["mask_" + k] = d.astype(np.float32), m.astype(bool)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", {k: int(m.sum()) for k, (_, m) in rec.items()}, len(out["points"]), "points")


if __name__ == "__main__":
    main()
