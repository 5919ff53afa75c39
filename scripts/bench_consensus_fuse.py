"""DTU fusion kernel (mdf_consensus_fuse_fwd) on a synthetic 49-view 1184x1600 scan (oracle/gen_golden.py:filter_scene at that
size, 5 % of the depths zeroed as by the probability filter, random colours; DTU parameters disp_thresh 0.25, num_consistent 3).

Reports
* the kernel time per scan: HIP events around the two entries (fusion + count scan, then compaction), --repeats runs,
  median / min / max;
* (pixel, view) pairs per second, N (N-1) H W pairs per scan;
* vector instructions per pair MEASURED: SQ_INSTS_VALU of consensus_fuse_kernel (wave instructions, from a separate
  `rocprofv3 --pmc` child run on the same scene) x 64 lanes / pairs -- what a pair costs on average, out-of-bounds and
  disagreeing pairs included (profiles/r05_filter_pmc.md measures the N1 filter the same way);
* the fraction of the vector-issue roof that implies: lane instructions / fusion time over 1024 SIMD-32 x 32 lanes x 2.4 GHz,
  the clock bench.py's cfg5_scan.filter uses;
* for reference, scripts/isa_stats.py's static `loopv` of the per-pair loop (every branch counted once, not an average).
  python scripts/bench_consensus_fuse.py [--repeats 10] [--out profiles/consensus_fuse_bench.json] [--no-counters]"""
import argparse
import json
import os
import re
import glob
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

VECTOR_ISSUE_LANE_OPS = 1024 * 32 * 2.4e9


def loop_valu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_stats.py"),
                          os.path.join(ROOT, "mdf-net_amd", "csrc", "consensus_fuse.hip")], capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        if line.startswith("consensus_fuse_kernel"):
            return int(line.split()[-1])
    raise RuntimeError("consensus_fuse_kernel not in isa_stats output:\n" + out)


def count_valu(scene, repeats):
    """SQ_INSTS_VALU per consensus_fuse_kernel launch, from a fresh child process under rocprofv3 (counters only + kernel trace)."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_WAVES", "--kernel-trace", "--output-format", "csv",
               "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--scene", scene, "--repeats", str(repeats), "--no-counters"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        acc = {}
        for f in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
            import csv
            for row in csv.DictReader(open(f)):
                if "consensus_fuse_kernel" in row["Kernel_Name"]:
                    acc.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        if "SQ_INSTS_VALU" not in acc:
            raise RuntimeError("no SQ_INSTS_VALU rows for consensus_fuse_kernel in the rocprofv3 output")
        # one row per dispatch (rocprofv3 sums the counter over the device): the mean over the dispatches
        return {k: statistics.mean(v) for k, v in acc.items()}, len(acc["SQ_INSTS_VALU"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1184)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-counters", action="store_true", help="skip the rocprofv3 SQ_INSTS_VALU child run")
    ap.add_argument("--scene", default=None, help="(internal) .npz written by the parent: skips the scene generation")
    a = ap.parse_args()
    from oracle.gen_golden import filter_scene
    from mdfnet_hip import ops
    t0 = time.time()
    if a.scene:
        z = np.load(a.scene)
        depths, images, K, E = z["depths"], z["images"], z["K"], z["E"]
    else:
        depths, _, K, E = filter_scene(h=a.height, w=a.width, nsrc=a.views - 1, seed=7)
        rng = np.random.RandomState(7)
        depths = depths.copy()
        depths[rng.rand(*depths.shape) < 0.05] = 0.0
        images = rng.randint(0, 256, depths.shape + (3,)).astype(np.uint8)
    t_gen = time.time() - t0
    counters, dispatches = None, 0
    if not a.no_counters:                    # before this process opens the GPU: the child has the device to itself
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "scene.npz")
            np.savez(path, depths=depths, images=images, K=K, E=E)
            counters, dispatches = count_valu(path, 1)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    d, im = torch.from_numpy(depths).to(dev), torch.from_numpy(images).to(dev)
    xyz, _, counts = ops.consensus_fuse(d, im, K, E, 0.25, 3)           # warm-up (code object load, allocator)
    ms, ms_fuse = [], []
    for _ in range(a.repeats):
        ops.profile_begin()
        xyz, _, counts = ops.consensus_fuse(d, im, K, E, 0.25, 3)
        recs = ops.profile_end()
        ms.append(sum(x[2] for x in recs if x[0] in ("mdf_consensus_fuse_fwd", "mdf_consensus_compact")))
        ms_fuse.append(sum(x[2] for x in recs if x[0] == "mdf_consensus_fuse_fwd"))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ops.consensus_fuse(d, im, K, E, 0.25, 3)
    torch.cuda.synchronize()
    wall_ms = 1e3 * (time.perf_counter() - t1)
    n, h, w = depths.shape
    pairs = float(n) * (n - 1) * h * w
    med, med_fuse = statistics.median(ms), statistics.median(ms_fuse)
    rec = {"workload": f"consensus fusion of one synthetic DTU-shaped scan: {n} views x {w}x{h}, disp_thresh 0.25, num_consistent 3",
           "kernel_ms_per_scan": {"median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "repeats": len(ms),
                                  "fusion_and_scan_median": round(med_fuse, 3)},
           "wall_ms_per_scan": round(wall_ms, 3),
           "pairs_per_scan": pairs, "pairs_per_s": round(pairs / (med * 1e-3), 1),
           "static_loop_valu_every_branch": loop_valu(),
           "points": int(xyz.shape[0]), "points_per_view_min_max": [int(counts.min()), int(counts.max())],
           "scene_generation_s": round(t_gen, 1), "device": torch.cuda.get_device_name(0)}
    if counters is not None:
        valu = counters["SQ_INSTS_VALU"]
        per_pair = valu * 64.0 / pairs
        rec["measured"] = {"SQ_INSTS_VALU_per_scan": valu, "SQ_WAVES_per_scan": counters.get("SQ_WAVES"), "dispatches": dispatches,
                           "vector_instructions_per_pair": round(per_pair, 2),
                           "frac_of_vector_issue_roof": round(valu * 64.0 / (med_fuse * 1e-3) / VECTOR_ISSUE_LANE_OPS, 4)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
