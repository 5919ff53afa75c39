"""DTU point-cloud evaluation (mdf_pts_*, mdf_dtu_masks; ops.dtu_eval_scan's phases) on a synthetic DTU-size scan:
mdfnet_hip.synth.dtu_eval_scene with --stl STL points on a 300 x 300 mm surface, --data points (every surface sample four times
within 0.05 mm: overlapping fused views, 0.3 mm noise, 2 % outliers up to 90 mm off) and an ObsMask at 0.5 mm.

Times every phase with HIP events around its own op call: the three index builds (all data, STL, reduced data), the reduction
(neighbour count + CSR + rounds; its round and pair counts), data -> stl and stl -> data distances (queries/s and leaves visited
per query: mean, p99, max) and the masks.  Median over --repeats.
  python scripts/bench_dtu_eval.py [--stl 2500000] [--data 10000000] [--repeats 3] [--out profiles/dtu_eval_bench.json]"""
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


def visit_stats(v):
    v = v.double()
    return {"mean": float(v.mean()), "p99": float(torch.quantile(v[torch.randperm(len(v), device=v.device)[:1 << 24]], 0.99)),
            "max": int(v.max())}


def run_once(sc, order, dev):
    from mdfnet_hip import ops
    q = torch.from_numpy(sc["qdata"].astype(np.float64)).to(dev)
    s = torch.from_numpy(sc["qstl"]).to(dev)
    obs = torch.from_numpy(sc["obs_mask"]).to(dev)
    torch.cuda.synchronize()
    t, out = {}, {}
    idx_all, t["index_data"] = timed(lambda: ops.point_index(q))
    stats = {}
    (keep, rounds), t["reduce"] = timed(lambda: ops.reduce_points(q, 0.2, order, index=idx_all, stats=stats))
    qr = q[keep].contiguous()
    idx_stl, t["index_stl"] = timed(lambda: ops.point_index(s))
    idx_red, t["index_reduced"] = timed(lambda: ops.point_index(qr))
    (dd, vd), t["data_to_stl"] = timed(lambda: ops.nn_distance(idx_stl, idx_red, bb=sc["bb"], return_visits=True))
    (ds, vs), t["stl_to_data"] = timed(lambda: ops.nn_distance(idx_red, idx_stl, bb=sc["bb"], return_visits=True))
    _, t["masks"] = timed(lambda: ops.dtu_masks(qr, obs, sc["bb"], sc["res"], s, sc["plane"]))
    out.update(reduced=int(qr.shape[0]), rounds=rounds, edges=stats["edges"], visits_data_to_stl=visit_stats(vd),
               visits_stl_to_data=visit_stats(vs), capped_data=int((dd == 60.0).sum()), checksum=float(dd.sum() + ds.sum()))
    return t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stl", type=int, default=2_500_000)
    ap.add_argument("--data", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtu_eval_bench.json"))
    args = ap.parse_args()
    from mdfnet_hip import synth
    dev = torch.device("cuda", 0)
    t0 = time.time()
    sc = synth.dtu_eval_scene(args.stl, args.data, seed=0)
    order = np.random.RandomState(0).permutation(args.data)
    print(f"scene: {args.stl} stl, {args.data} data points, ObsMask {sc['obs_mask'].shape} ({time.time() - t0:.1f}s on the host)")
    run_once(sc, order, dev)                                           # warm-up (code objects, allocator)
    runs = [run_once(sc, order, dev) for _ in range(args.repeats)]
    names = list(runs[0][0])
    med = {k: round(statistics.median(r[0][k] for r in runs), 3) for k in names}
    mn = {k: round(min(r[0][k] for r in runs), 3) for k in names}
    info = runs[0][1]
    assert all(r[1]["checksum"] == info["checksum"] and r[1]["rounds"] == info["rounds"] for r in runs), "runs differ"
    res = {"scene": {"stl": args.stl, "data": args.data, "obs_mask": list(sc["obs_mask"].shape), "res_mm": sc["res"]},
           "repeats": args.repeats, "phase_ms_median": med, "phase_ms_min": mn, "total_ms_median": round(sum(med.values()), 3),
           "reduced_points": info["reduced"], "reduce_rounds": info["rounds"], "reduce_edges": info["edges"],
           "data_to_stl_queries_per_s": info["reduced"] / (med["data_to_stl"] * 1e-3),
           "stl_to_data_queries_per_s": args.stl / (med["stl_to_data"] * 1e-3),
           "leaves_visited_data_to_stl": info["visits_data_to_stl"], "leaves_visited_stl_to_data": info["visits_stl_to_data"],
           "capped_data_points": info["capped_data"]}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
