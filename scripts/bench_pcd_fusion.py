"""Point-cloud fusion (mdf_pcd_fuse_fwd / mdf_pcd_compact, ops.pcd_fuse) on a synthetic Tanks-size scan: mdfnet_hip.synth.pcd_scan
at 1920 x 1056 with --views views (default 64) and 10 sources each.

Times every stage with HIP events around its own mdf_pcd_fuse_fwd call (one step per call, the state carried between calls):
the probability filter (torch), the three visibility filters, visibility fusion, average fusion, the small-segment filter,
and the compaction.  Reports candidates/s of visibility fusion (N (V+1) H W candidate slots: every reference and source pixel,
valid or not) and points/s of the compaction.  Stages 7 and 8 (normals, voxel downsampling) are timed by scripts/bench_pcd_normals.py.
  python scripts/bench_pcd_fusion.py [--views 64] [--repeats 3] [--out profiles/pcd_fusion_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return r, e0.elapsed_time(e1)


def run_once(s, view, vthresh, dev):
    from mdfnet_hip import ops
    n, h, w = s["depths"].shape
    depths = torch.from_numpy(s["depths"]).to(dev)
    probs = torch.from_numpy(s["probs"]).to(dev)
    images = torch.from_numpy(s["images"]).to(dev)
    cams = torch.from_numpy(ops.pcd_cameras(s["K"], s["E"])).to(dev)
    srcs = torch.from_numpy(ops.pcd_sources(s["srcs"], n, view)).to(dev)
    need = int(np.ceil(np.float32(vthresh - 1.1)))
    torch.cuda.synchronize()
    times = {}

    def prob():
        m = (probs > ops.PCD_PROB_THRESHOLD).to(torch.uint8)
        return (depths * m).contiguous(), m.contiguous()
    (dep, mask), times["prob"] = timed(prob)
    ws = total = None
    for k, name in enumerate(ops.PCD_STEPS[1:], 1):
        (ws, counts, total), times[name] = timed(lambda: ops.pcd_steps(dep, mask, cams, srcs, need, k, k))
    xyz = torch.empty((total, 3), device=dev)
    rgb = torch.empty((total, 3), device=dev, dtype=torch.uint8)
    dirs = torch.empty((total, 3), device=dev)
    from mdfnet_hip import check, lib
    _, times["compact"] = timed(lambda: check(lib().mdf_pcd_compact(dep.data_ptr(), mask.data_ptr(), images.data_ptr(), cams.data_ptr(), n,
                                                              h, w, view, ws.data_ptr(), xyz.data_ptr(), rgb.data_ptr(),
                                                              dirs.data_ptr(), total, None), "mdf_pcd_compact"))
    return times, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--view", type=int, default=10)
    ap.add_argument("--vthresh", type=int, default=4)
    ap.add_argument("--height", type=int, default=1056)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_fusion_bench.json"))
    a = ap.parse_args()
    from mdfnet_hip import synth
    dev = torch.device("cuda", 0)
    t0 = time.time()
    s = synth.pcd_scan(a.views, a.height, a.width, seed=3, nsrc=a.view)
    print(f"scene {a.views}x{a.height}x{a.width}: {time.time() - t0:.1f}s to build")
    run_once(s, a.view, a.vthresh, dev)                           # warm-up (code objects, allocator)
    runs = [run_once(s, a.view, a.vthresh, dev) for _ in range(a.repeats)]
    points = runs[0][1]
    assert all(r[1] == points for r in runs), "point count changed between runs"
    med = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
    n, h, w = a.views, a.height, a.width
    cand = float(n) * (a.view + 1) * h * w
    res = {"scene": f"{n}x{h}x{w}", "sources": a.view, "vthresh": a.vthresh, "repeats": a.repeats, "points": points,
           "stage_ms_median": {k: round(v, 3) for k, v in med.items()},
           "stage_ms_min": {k: round(min(r[0][k] for r in runs), 3) for k in med},
           "total_ms_median": round(sum(med.values()), 3),
           "vis_fusion_candidates_per_s": cand / (med["vis_fusion"] * 1e-3),
           "compact_points_per_s": points / (med["compact"] * 1e-3),
           "vis_filter_pixel_views_per_s": float(n) * a.view * h * w / (med["vis1"] * 1e-3)}
    for k, v in med.items():
        print(f"  {k:11s} {v:9.3f} ms")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
