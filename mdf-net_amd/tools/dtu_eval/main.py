"""DTU point-cloud evaluation: accuracy, completeness and overall in mm (counterpart of the reference's MATLAB scorer,
tools/matlab_linux/matlab2015/BaseEvalMain_web.m with PointCompareMain.m, and ComputeStat_web.m).

Per scan cSet it reads {ply_path}/{method}{cSet:03d}_{light}.ply (what tools/gipuma/main.py writes), the STL points
{data_path}/Points/stl/stl{cSet:03d}_total.ply, {data_path}/ObsMask/ObsMask{cSet}_10.mat (ObsMask, BB, Res) and
{data_path}/ObsMask/Plane{cSet}.mat (P), runs ops.dtu_eval_scan on the GPU (reduction to 0.2 mm, data -> stl and stl -> data
distances capped at 60 mm, the observation mask and the ground plane) and writes {results_path}/{method}_Eval_{cSet}.npz with
BaseEval's fields.  Like the reference it reuses a result file that already exists.  Scans shard over ranks (no collective);
after a barrier rank 0 prints the per-scan mean / median accuracy and completeness and the final line.
Divergence from MATLAB: the reduction's visiting order is numpy.random.RandomState(seed).permutation(N), not randperm.

  python mdf-net_amd/tools/dtu_eval/main.py --data_path "DATA/MVS Data" --ply_path PLY_DIR --scans 1,4
"""
import argparse
import os
import sys
import time

_TOP = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # mdf-net_amd/
if _TOP not in sys.path:
    sys.path.insert(0, _TOP)

import numpy as np  # noqa: E402

USED_SETS = [1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118]
BASE_EVAL_FIELDS = ("Qdata", "Ddata", "Qstl", "Dstl", "DataInMask", "StlAbovePlane", "GroundPlane", "dst", "Margin")


def scan_paths(args, cset):
    return {"data": os.path.join(args.ply_path, f"{args.method.lower()}{cset:03d}_{args.light}.ply"),
            "stl": os.path.join(args.data_path, "Points", "stl", f"stl{cset:03d}_total.ply"),
            "mask": os.path.join(args.data_path, "ObsMask", f"ObsMask{cset}_10.mat"),
            "plane": os.path.join(args.data_path, "ObsMask", f"Plane{cset}.mat"),
            "result": os.path.join(args.results_path, f"{args.method}_Eval_{cset}.npz")}


def eval_scan(args, cset, device=None):
    """PointCompareMain.m for one scan -> the result file (computed unless it exists)."""
    from mdfnet_hip import ops
    from tools.data_io import read_mat, read_ply_vertices
    p = scan_paths(args, cset)
    if os.path.exists(p["result"]):
        print(f"scan {cset}: reusing {p['result']}")
        return p["result"]
    t0 = time.time()
    qdata = read_ply_vertices(p["data"])
    qstl = read_ply_vertices(p["stl"])
    mask = read_mat(p["mask"])
    plane = read_mat(p["plane"])["P"]
    t1 = time.time()
    ev = ops.dtu_eval_scan(qdata, qstl, mask["ObsMask"], mask["BB"], float(np.asarray(mask["Res"]).reshape(-1)[0]), plane,
                           dst=args.dst, seed=args.seed, max_dist=args.max_dist, device=device)
    t2 = time.time()
    os.makedirs(os.path.dirname(os.path.abspath(p["result"])), exist_ok=True)
    tmp = p["result"] + ".tmp.npz"
    np.savez(tmp, cSet=cset, **{k: ev[k] for k in BASE_EVAL_FIELDS})
    os.replace(tmp, p["result"])
    print(f"scan {cset}: {len(qdata)} points -> {ev['Qdata'].shape[1]} after reduction ({ev['Rounds']} rounds, {ev['Edges']} "
          f"pairs), {len(qstl)} stl points (read {t1 - t0:.2f}s, evaluate {t2 - t1:.2f}s) -> {p['result']}")
    return p["result"]


def scan_stats(path, max_dist):
    from mdfnet_hip import ops
    with np.load(path) as z:
        return ops.dtu_scan_stats({k: z[k] for k in ("Ddata", "DataInMask", "Dstl", "StlAbovePlane")}, max_dist)


def summary(args, scans):
    """BaseEvalMain_web.m's table and final line (and ComputeStat_web.m's counts / variances) from the result files.
    -> (per-scan stats list, (acc, comp, overall))."""
    rows = []
    for cset in scans:
        st = scan_stats(scan_paths(args, cset)["result"], args.max_dist)
        st["cSet"] = cset
        rows.append(st)
        print(f"scan {cset}: mean/median Data (acc.) {st['MeanData']:f}/{st['MedData']:f}   "
              f"mean/median Stl (comp.) {st['MeanStl']:f}/{st['MedStl']:f}   (n {st['nData']}/{st['nStl']})")
    acc = float(np.mean([r["MeanData"] for r in rows]))
    comp = float(np.mean([r["MeanStl"] for r in rows]))
    overall = (acc + comp) / 2
    print(f"final evaluation result on all scans: acc.: {acc:f}, comp.: {comp:f}, overall: {overall:f}")
    return rows, (acc, comp, overall)


def parse(argv=None):
    import config                       # the project's data root (MDF_DATA_ROOT)
    parser = argparse.ArgumentParser(description="DTU point-cloud evaluation (accuracy / completeness) on the GPU")
    parser.add_argument("--data_path", default=os.path.join(config.DATA_ROOT, "MVS Data"),
                        help="the DTU 'MVS Data' root (Points/stl, ObsMask)")
    parser.add_argument("--ply_path", default=None, help="the method's PLYs (default: <data_path>/Points/<method>)")
    parser.add_argument("--results_path", default=None, help="where the result files go (default: the ply path)")
    parser.add_argument("--method", default="ours")
    parser.add_argument("--light", default="l3")
    parser.add_argument("--scans", default=None, help="comma-separated scan numbers (default: the 22 evaluation scans)")
    parser.add_argument("--dst", type=float, default=0.2, help="minimum distance between points after the reduction (mm)")
    parser.add_argument("--max_dist", type=float, default=20.0, help="outlier threshold of the statistics (mm)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the reduction's visiting order")
    args = parser.parse_args(argv)
    args.ply_path = args.ply_path or os.path.join(args.data_path, "Points", args.method)
    args.results_path = args.results_path or args.ply_path
    args.scans = [int(s) for s in args.scans.split(",")] if args.scans else list(USED_SETS)
    return args


def main(argv=None):
    import torch
    from mdfnet_hip import shard
    args = parse(argv)
    rank, world, local = shard.init()
    device = torch.device("cuda", local)
    for i in shard.shard_items(len(args.scans), rank, world):      # scans are independent: shard them, no collective
        eval_scan(args, args.scans[i], device)
    shard.barrier()
    if rank == 0:
        return summary(args, args.scans)
    return None


if __name__ == "__main__":
    main()
