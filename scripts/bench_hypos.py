"""hypos_fit modes 2 (laplace), 3 (gauss0) and 4 (gauss1) on the same inputs at cfg2's two inter-stage shapes: us per launch and the
share of HBM bandwidth.  dev tool; needs an MI355X.

    python scripts/bench_hypos.py [--launches 200] [--rounds 9] [--modes 2,3,4]

Each mode reads D planes of prob, the hypotheses (D planes when they are per pixel, D floats otherwise), the depth (modes 2, 3) and
writes s: the bytes below.  The three modes differ in register arithmetic only, so mode 2 (the default composition's stage 2 fit)
is the yardstick: the new modes are expected within 1.5x of its time.

Timing: HIP events around a window of `launches` back-to-back launches of one mode through the C ABI with prebuilt arguments (no
allocation, no Python wrapper in the window); the three modes take turns, `rounds` windows each, after a warm-up window of every
mode; median and minimum over the windows.  The host time of enqueueing the window is printed beside it: where it is not clearly
below the event time, the window measured the launch path and not the kernel, and the line says so.  These kernels are shorter than
the launch path, so their own time comes from a kernel trace, one run per mode (modes 3 and 4 are one kernel name):
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_hypos.py --modes 3 --launches 100 --rounds 2"""
import argparse
import ctypes
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "mdf-net_amd"), os.path.join(R, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import heads_mirror as M  # noqa: E402
from mdfnet_hip import check, lib, ops  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X
DEV = "cuda:0"
SHAPES = [(148, 200, 48, False), (296, 400, 24, True)]      # h, w, D, per-pixel hypotheses: cfg2's stage 0 -> 1 and 1 -> 2


def traffic(mode, D, hw, per_pixel):
    planes = D + (D if per_pixel else 0) + (1 if mode in (2, 3) else 0) + 1
    return 4 * hw * planes + (0 if per_pixel else 4 * D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--modes", default="2,3,4")
    a = ap.parse_args()
    modes = tuple(int(m) for m in a.modes.split(","))
    assert torch.cuda.is_available(), "bench_hypos.py measures on an MI355X; there is no CPU path"
    fn = lib().mdf_hypos_fit_fwd
    for h, w, D, pp in SHAPES:
        prob, _, _ = M.make_probs(1, D, h, w, 7)
        hyp = M.make_hypos(1, D, h, w, pp, 7)
        if pp:      # hypotheses as the pipeline makes them: a few millimetres around the regressed depth
            centre = np.random.RandomState(3).uniform(450, 900, (1, 1, h, w))
            hyp = (centre + np.linspace(-30, 30, D).reshape(1, D, 1, 1)).astype(np.float32)
        pg, hg = torch.from_numpy(prob).to(DEV), torch.from_numpy(hyp).to(DEV)
        dg = ops.depth_regress(pg, hg)
        out = torch.empty((1, h, w), device=DEV)
        stream = ops._stream(out)
        args = {m: (m, pg.data_ptr(), dg.data_ptr(), hg.data_ptr(), int(pp), None, out.data_ptr(), 1, D, h, w, stream) for m in modes}

        def window(m):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.launches):
                rc = fn(*args[m])
            e1.record()
            host_us = (time.perf_counter() - t0) * 1e6 / a.launches
            torch.cuda.synchronize()
            check(rc, "mdf_hypos_fit_fwd")
            return e0.elapsed_time(e1) * 1e3 / a.launches, host_us
        for m in modes:
            window(m)
        res = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                res[m].append(window(m))
        base = statistics.median(t for t, _ in res[modes[0]])
        for m in modes:
            ts, hs = [t for t, _ in res[m]], [x for _, x in res[m]]
            med, host = statistics.median(ts), statistics.median(hs)
            by = traffic(m, D, h * w, pp)
            note = "" if host < 0.8 * med else "   [window bound by the launch path, not the kernel]"
            print(f"{h}x{w} D={D} {'per-pixel' if pp else 'shared'} mode {m}: median {med:6.2f} us  min {min(ts):6.2f} us  max {max(ts):6.2f} us  "
                  f"(host enqueue {host:5.2f} us)  {by / 1e6:6.2f} MB  {by / (med * 1e-6) / HBM_PEAK * 100:5.1f} % of HBM peak  "
                  f"x{med / base:4.2f} of mode {modes[0]}{note}")


if __name__ == "__main__":
    main()
