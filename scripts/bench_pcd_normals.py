"""Point-cloud post-processing (stages 7 and 8 of ops.pcd_fuse: mdf_pts_index_build, mdf_pts_normals, mdf_pts_knn,
mdf_pts_voxel_downsample) on a synthetic Tanks-size scan: mdfnet_hip.synth.pcd_scan at 1920 x 1056 with --views views (default 64).

Two child processes, each under its own `timeout`, the second only if the first ended well:
  gpu   one pcd_fuse(normals=True, downsample=-1) over the scan (wall time), then on its fused points the median of --repeats
        timings (HIP events) of each stage: the index build, the normals, the spacing (the k = 2 self-query, the sort, the two
        values read back), the voxel grid.  Leaves visited per query of the 30-neighbour search come from mdf_pts_knn over a
        --sample subsample of the points as queries against the whole index.
  cpu   for context, the float64 host oracle on the same subsample alone: scipy.spatial.cKDTree(sub).query(sub, k=30, workers=16).
Nothing was measured before these kernels existed, so there is no pass bar.
  python scripts/bench_pcd_normals.py [--views 64] [--repeats 3] [--sample 1000000] [--out profiles/pcd_normals_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return r, e0.elapsed_time(e1)


def gpu_step(a):
    import numpy as np
    import torch
    from mdfnet_hip import ops, synth
    dev = torch.device("cuda", 0)
    t0 = time.time()
    s = synth.pcd_scan(a.views, a.height, a.width, seed=3, nsrc=a.view)
    print(f"scene {a.views}x{a.height}x{a.width}: {time.time() - t0:.1f}s to build", flush=True)
    args = [torch.from_numpy(s[k]).to(dev) for k in ("depths", "probs", "images")] + [s["K"], s["E"], s["srcs"]]
    base = ops.pcd_fuse(*args, view=a.view, vthresh=a.vthresh)                 # warm-up, and the points the stages are timed on
    xyz, rgb, dirs = base["xyz"], base["rgb"], base["dirs"]
    m = int(xyz.shape[0])
    print(f"{m} fused points", flush=True)
    torch.cuda.synchronize()
    t0 = time.time()
    full = ops.pcd_fuse(*args, view=a.view, vthresh=a.vthresh, normals=True, downsample=-1)
    torch.cuda.synchronize()
    wall = time.time() - t0
    voxel, m_out = full["voxel"], int(full["xyz"].shape[0])
    del full, base
    xyz64 = xyz.double()
    times = {"index_build": [], "normals": [], "spacing": [], "voxel_grid": []}
    for _ in range(a.repeats):
        index, t = timed(lambda: ops.point_index(xyz64))
        times["index_build"].append(t)
        nrm, t = timed(lambda: ops.estimate_normals(index, dirs=dirs, k=ops.PCD_NORMAL_KNN))
        times["normals"].append(t)
        v, t = timed(lambda: ops.pcd_voxel_size(index))
        times["spacing"].append(t)
        assert v == voxel, "the voxel size changed between runs"
        attrs = torch.cat([(rgb.float() / 255.0).double(), nrm], 1)
        out, t = timed(lambda: ops.voxel_downsample(xyz64, voxel, attrs=attrs))
        times["voxel_grid"].append(t)
        assert out[0].shape[0] == m_out, "the downsampled point count changed between runs"
        del out, attrs
    nsub = min(a.sample, m)
    sel = torch.from_numpy(np.sort(np.random.RandomState(0).choice(m, nsub, replace=False))).to(dev)
    sub = xyz64[sel].contiguous()
    (_, visits), t_knn = timed(lambda: ops.knn_search(index, ops.point_index(sub), ops.PCD_NORMAL_KNN, return_visits=True))
    (_, visits2), _ = timed(lambda: ops.knn_search(index, ops.point_index(sub), 2, return_visits=True))
    np.save(os.path.join(a.tmp, "sub.npy"), sub.cpu().numpy())
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"scene": f"{a.views}x{a.height}x{a.width}", "sources": a.view, "vthresh": a.vthresh, "repeats": a.repeats, "points": m,
           "points_after_downsample": m_out, "voxel": voxel, "k": ops.PCD_NORMAL_KNN,
           "pcd_fuse_normals_downsample_wall_s": round(wall, 3),
           "stage_ms_median": {k: round(v, 3) for k, v in med.items()},
           "stage_ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "normals_points_per_s": m / (med["normals"] * 1e-3),
           "index_build_points_per_s": m / (med["index_build"] * 1e-3),
           "spacing_points_per_s": m / (med["spacing"] * 1e-3),
           "voxel_grid_points_per_s": m / (med["voxel_grid"] * 1e-3),
           "knn30_subsample": {"queries": nsub, "ms": round(t_knn, 3), "leaves_visited_per_query_mean": float(visits.double().mean()),
                               "leaves_visited_per_query_max": int(visits.max())},
           "knn2_subsample": {"leaves_visited_per_query_mean": float(visits2.double().mean())}}
    for k, v in med.items():
        print(f"  {k:12s} {v:10.3f} ms")
    with open(os.path.join(a.tmp, "gpu.json"), "w") as f:
        json.dump(res, f)


def cpu_step(a):
    import numpy as np
    from scipy.spatial import cKDTree
    sub = np.load(os.path.join(a.tmp, "sub.npy"))
    t0 = time.time()
    tree = cKDTree(sub)
    t1 = time.time()
    tree.query(sub, k=30, workers=16)
    t2 = time.time()
    res = {"points": len(sub), "build_s": round(t1 - t0, 3), "query_k30_workers16_s": round(t2 - t1, 3),
           "query_points_per_s": len(sub) / (t2 - t1)}
    with open(os.path.join(a.tmp, "cpu.json"), "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--view", type=int, default=10)
    ap.add_argument("--vthresh", type=int, default=4)
    ap.add_argument("--height", type=int, default=1056)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=1000000)
    ap.add_argument("--gpu_timeout", type=int, default=900)
    ap.add_argument("--cpu_timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_normals_bench.json"))
    ap.add_argument("--step", default=None, help="(internal) gpu or cpu: run that step in this process")
    ap.add_argument("--tmp", default=None, help="(internal) the folder the steps exchange files in")
    a = ap.parse_args()
    if a.step == "gpu":
        return gpu_step(a)
    if a.step == "cpu":
        return cpu_step(a)
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in (("gpu", a.gpu_timeout), ("cpu", a.cpu_timeout)):
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--tmp", tmp]
            for k in ("views", "view", "vthresh", "height", "width", "repeats", "sample"):
                cmd += [f"--{k}", str(getattr(a, k))]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit(f"the {step} step ended with status {rc}: nothing more is started")
        res = json.load(open(os.path.join(tmp, "gpu.json")))
        res["cpu_oracle_ckdtree"] = json.load(open(os.path.join(tmp, "cpu.json")))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
