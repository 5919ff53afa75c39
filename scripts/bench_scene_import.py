"""Scene import (ops.view_scores, ops.view_depth_ranges: mdf_view_scores / mdf_view_depth_ranges) on a generated sparse model:
--images cameras on a partial ring (default 300), --points points (default 500 000), every point seen in a window of neighbouring
cameras with random drop-outs.

Prints the record count (one record per point and image pair that sees it), the bytes the radix sorts move (8 passes, each
reading and writing a 64-bit key and a 32-bit value per element, plus the histogram read), the median of --repeats timings (HIP
events) of both ops, and for context the numpy oracle (tests/view_select_oracle.py, float64, one host thread) on every
--subset-th point, scaled by the record count.  Nothing was measured before these kernels existed, so there is no pass bar.
  python scripts/bench_scene_import.py [--images 300] [--points 500000] [--window 8] [--repeats 5] [--out profiles/scene_import_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_scene(n_img, n_pts, window, drop, seed):
    """The oracle's generator (tests/view_select_oracle.py:make_scene), vectorised over the points."""
    import numpy as np
    import view_select_oracle as O
    rot, trans, _, _, _ = O.make_scene(n_img, 0, seed, arc_deg=300.0)
    rng = np.random.RandomState(seed + 1)
    pts = rng.normal(0.0, 0.6, (n_pts, 3))
    k = rng.randint(0, n_img, n_pts)
    cand = k[:, None] + np.arange(-window, window + 1)[None, :]
    seen = (cand >= 0) & (cand < n_img) & (rng.uniform(size=cand.shape) >= drop)
    off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(seen.sum(1))]).astype(np.int64)
    return rot, trans, pts, off, cand[seen].astype(np.int32)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return r, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--drop", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subset", type=int, default=100, help="the oracle runs on every subset-th point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_import_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import view_select_oracle as O
    from mdfnet_hip import ops
    t0 = time.time()
    s = make_scene(a.images, a.points, a.window, a.drop, 11)
    n_obs, n_rec = len(s[4]), O.n_records(s[3])
    print(f"scene: {a.images} images, {a.points} points, {n_obs} observations, {n_rec} records ({time.time() - t0:.1f}s to build)", flush=True)
    dev = torch.device("cuda", 0)
    g = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in s]
    ops.view_scores(*g)
    ops.view_depth_ranges(*g)                                    # warm-up
    times = {"view_scores": [], "view_depth_ranges": []}
    for _ in range(a.repeats):
        (score, shared), t = timed(lambda: ops.view_scores(*g))
        times["view_scores"].append(t)
        _, t = timed(lambda: ops.view_depth_ranges(*g))
        times["view_depth_ranges"].append(t)
    tile = 4096

    def sort_bytes(n):                                           # 8 passes: histogram read (8 B), scatter read + write (12 B each)
        return 8 * (n * (8 + 12 + 12) + 2 * 256 * ((n + tile - 1) // tile) * 12)

    sub = slice(0, a.points, a.subset)
    lens = np.diff(s[3])[sub]
    sub_off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens)])
    sub_img = np.concatenate([s[4][s[3][p]:s[3][p + 1]] for p in range(0, a.points, a.subset)]) if a.points else s[4]
    t0 = time.time()
    want, _ = O.scores(s[0], s[1], s[2][sub], sub_off, sub_img)
    t_oracle = time.time() - t0
    sub_rec = O.n_records(sub_off)
    res = {"images": a.images, "points": a.points, "observations": n_obs, "records": n_rec, "repeats": a.repeats,
           "ms_median": {k: round(statistics.median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "records_per_s": n_rec / (statistics.median(times["view_scores"]) * 1e-3),
           "sort_bytes": {"view_scores": sort_bytes(n_rec), "view_depth_ranges": 2 * sort_bytes(n_obs)},
           "pairs_with_shared_points": int((shared.cpu().numpy() > 0).sum() // 2),
           "oracle_numpy": {"records": sub_rec, "seconds": round(t_oracle, 3),
                            "scaled_to_all_records_s": round(t_oracle * n_rec / max(sub_rec, 1), 1)}}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
