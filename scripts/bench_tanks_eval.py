"""Tanks and Temples F-score evaluation (ops.tanks_eval_scene: mdf_pts_transform / _crop / _voxel_downsample / _index_build / _nn /
_icp_sums) on a synthetic scene of realistic size: a curved surface of --gt ground-truth points spaced about tau / 2 apart, --est
estimated points covering most of it (noise 0.7 tau, 4 % outliers, a rigid offset of a few tau), a polygon crop.

Reports the GPU time of every step of the protocol (HIP events around each C-ABI call, summed per entry), the wall time of the
whole evaluation, the point counts, the scores, and the leaves visited per nearest-neighbour query (mean, p99, max) at each ICP
stage's threshold and in the final comparison.  With --oracle_scale S it then times tests/tanks_eval_oracle.py (numpy + scipy
cKDTree) on an S times smaller scene on the same host, as context only.
  python scripts/bench_tanks_eval.py [--est 20000000] [--gt 10000000] [--oracle_scale 10] [--out profiles/tanks_eval_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def scene(n_est, n_gt, tau, seed=0):
    """Like tests/tanks_eval_oracle.py:fixture_scene, sized so that the ground truth's spacing is about tau / 2."""
    rng = np.random.RandomState(seed)
    side = np.sqrt(n_gt) * tau / 4                       # half the square's side: (2 side)^2 / n_gt = (tau / 2)^2
    k = 3.0 / side

    def surface(u, v):
        return np.stack([u, 0.12 * side * np.sin(k * u) * np.cos(0.7 * k * v) + 0.04 * u * v / side, v], 1)

    gt = surface(rng.uniform(-side, side, n_gt), rng.uniform(-side, side, n_gt))
    n_out = n_est // 25
    est = surface(rng.uniform(-side, 0.6 * side, n_est - n_out), rng.uniform(-0.8 * side, side, n_est - n_out))
    est += rng.normal(0, 0.7 * tau / np.sqrt(3.0), est.shape)
    est = np.concatenate([est, rng.uniform(-side, side, (n_out, 3)) * [1, 0.3, 1]])
    ang = 0.0005
    off = np.eye(4)
    off[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    off[:3, 3] = [2.5 * tau, -1.5 * tau, 2.0 * tau]
    inv = np.linalg.inv(off)
    est = est @ inv[:3, :3].T + inv[:3, 3]
    poly = side * np.array([[-0.9, -0.85], [0.2, -0.95], [0.85, -0.4], [0.7, 0.8], [-0.1, 0.6], [-0.9, 0.9]])
    crop = {"axis": 1, "axis_min": -0.1 * side, "axis_max": 0.25 * side, "polygon": poly}
    return est, gt, crop


def visit_stats(v):
    v = v.double()
    return {"mean": float(v.mean()), "p99": float(torch.quantile(v[torch.randperm(len(v), device=v.device)[:1 << 24]], 0.99)),
            "max": int(v.max())}


def gpu_run(est, gt, crop, tau, dev):
    from mdfnet_hip import ops
    e, g = torch.from_numpy(est).to(dev), torch.from_numpy(gt).to(dev)
    torch.cuda.synchronize()
    ops.profile_begin()
    t0 = time.time()
    res = ops.tanks_eval_scene(e, g, crop, tau, np.eye(4), device=dev)
    wall = time.time() - t0
    per = {}
    for name, _, ms, _ in ops.profile_end():
        per.setdefault(name, [0, 0.0])
        per[name][0] += 1
        per[name][1] += ms
    # leaves visited per query: the stages' sources under the final T against the ground truth, and the final comparison
    visits = {}
    gidx = ops.point_index(g)
    cur = ops.transform_points(e, res["T"])
    cur = cur[ops.crop_volume(cur, crop["axis"], crop["axis_min"], crop["axis_max"], crop["polygon"])].contiguous()
    for name, vox, thr in (("icp_A", tau, 80 * tau), ("icp_B", tau / 2, 20 * tau), ("icp_C", None, 2 * tau)):
        s = ops.voxel_downsample(cur, vox) if vox else cur[::max(int(round(cur.shape[0] / ops.TANKS_STAGE_C_POINTS)), 1)].contiguous()
        visits[name] = visit_stats(ops.nn_search(gidx, s, thr, return_visits=True)[2])
    del gidx
    ed = ops.voxel_downsample(cur, tau / 2)
    gc = g[ops.crop_volume(g, crop["axis"], crop["axis_min"], crop["axis_max"], crop["polygon"])].contiguous()
    gd = ops.voxel_downsample(gc, tau / 2)
    visits["score_est_to_gt"] = visit_stats(ops.nn_search(ops.point_index(gd), ops.point_index(ed), 10 * tau, return_visits=True)[2])
    visits["score_gt_to_est"] = visit_stats(ops.nn_search(ops.point_index(ed), ops.point_index(gd), 10 * tau, return_visits=True)[2])
    out = {"wall_s": round(wall, 3), "gpu_ms_per_entry": {k: {"calls": c, "ms": round(ms, 3)} for k, (c, ms) in sorted(per.items())},
           "gpu_ms_total": round(sum(ms for _, ms in per.values()), 3), "leaves_visited": visits,
           "counts": {k: int(v) for k, v in res.items() if k.startswith("n_")},
           "precision": res["precision"], "recall": res["recall"], "fscore": res["fscore"],
           "stage_iterations": res["stage_iterations"].tolist(), "stage_fitness": res["stage_fitness"].tolist(),
           "stage_rmse": res["stage_rmse"].tolist()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--est", type=int, default=20_000_000)
    ap.add_argument("--gt", type=int, default=10_000_000)
    ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--oracle_scale", type=int, default=10, help="time the CPU oracle on a scene this many times smaller (0: skip)")
    ap.add_argument("--oracle_only", action="store_true", help="skip the GPU part and add the oracle's time to the file at --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tanks_eval_bench.json"))
    args = ap.parse_args()
    if args.oracle_only:
        with open(args.out) as f:
            res = json.load(f)
    else:
        dev = torch.device("cuda", 0)
        gpu_run(*scene(args.est // 100, args.gt // 100, args.tau, seed=1), args.tau, dev)      # warm-up (code objects, allocator)
        t0 = time.time()
        est, gt, crop = scene(args.est, args.gt, args.tau)
        print(f"scene: {args.est} estimated, {args.gt} ground-truth points, tau {args.tau} ({time.time() - t0:.1f}s on the host)", flush=True)
        res = {"scene": {"est": args.est, "gt": args.gt, "tau": args.tau}, "gpu": gpu_run(est, gt, crop, args.tau, dev)}
        print(json.dumps(res, indent=1), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    if args.oracle_scale:
        import tanks_eval_oracle as O
        s = args.oracle_scale
        est, gt, crop = scene(args.est // s, args.gt // s, args.tau)
        t0 = time.time()
        want = O.eval_scene(est, gt, crop, args.tau, np.eye(4))
        res["cpu_oracle"] = {"est": args.est // s, "gt": args.gt // s, "wall_s": round(time.time() - t0, 1), "fscore": want["fscore"],
                             "note": "numpy + scipy cKDTree, one thread; context only"}
        print(json.dumps(res["cpu_oracle"], indent=1), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
