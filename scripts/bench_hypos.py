"""hypos_fit modes 2 (laplace), 3 (gauss0) and 4 (gauss1) and the atv spread kernel on the same inputs at cfg2's two inter-stage
shapes, then the two step-2 kernels (hypos_from_fit, atv_hypos) on the same maps: us per launch and the share of HBM bandwidth.
dev tool; needs an MI355X.

    python scripts/bench_hypos.py [--launches 200] [--rounds 9] [--modes 2,3,4,atv] [--no-step2]

Each step-1 kernel reads D planes of prob, the hypotheses (D planes when they are per pixel, D floats otherwise), the depth (modes 2, 3
and atv) and writes one plane: the bytes below.  They differ in register arithmetic only, so mode 2 (the default composition's stage
2 fit) is the yardstick: modes 3 and 4 are expected within 1.5x of its time, and atv, which reads the same planes as mode 3 and
writes one, at parity with mode 3.  The step-2 kernels read two planes and write D_out planes of four times the size.

Timing: HIP events around a window of `launches` back-to-back launches of one kernel through the C ABI with prebuilt arguments (no
allocation, no Python wrapper in the window); the kernels take turns, `rounds` windows each, after a warm-up window of every
one; median and minimum over the windows.  The host time of enqueueing the window is printed beside it: where it is not clearly
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
SHAPES = [(148, 200, 48, False, 24), (296, 400, 24, True, 8)]      # h, w, D, per-pixel hypotheses, D of the next stage: cfg2's stage 0 -> 1 and 1 -> 2


def traffic(mode, D, hw, per_pixel):
    planes = D + (D if per_pixel else 0) + (1 if mode in ("2", "3", "atv") else 0) + 1
    return 4 * hw * planes + (0 if per_pixel else 4 * D)


def measure(calls, launches, rounds):
    """calls: {name: (fn, args)} -> {name: [(event us per launch, host us per launch)]}, the kernels taking turns."""
    def window(name):
        fn, args = calls[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(launches):
            rc = fn(*args)
        e1.record()
        host_us = (time.perf_counter() - t0) * 1e6 / launches
        torch.cuda.synchronize()
        check(rc, name)
        return e0.elapsed_time(e1) * 1e3 / launches, host_us
    for name in calls:
        window(name)
    res = {name: [] for name in calls}
    for _ in range(rounds):
        for name in calls:
            res[name].append(window(name))
    return res


def report(title, res, nbytes):
    names = list(res)
    base = statistics.median(t for t, _ in res[names[0]])
    for name in names:
        ts, hs = [t for t, _ in res[name]], [x for _, x in res[name]]
        med, host = statistics.median(ts), statistics.median(hs)
        by = nbytes[name]
        note = "" if host < 0.8 * med else "   [window bound by the launch path, not the kernel]"
        print(f"{title} {name}: median {med:6.2f} us  min {min(ts):6.2f} us  max {max(ts):6.2f} us  "
              f"(host enqueue {host:5.2f} us)  {by / 1e6:6.2f} MB  {by / (med * 1e-6) / HBM_PEAK * 100:5.1f} % of HBM peak  "
              f"x{med / base:4.2f} of {names[0]}{note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--modes", default="2,3,4,atv")
    ap.add_argument("--no-step2", action="store_true", help="skip hypos_from_fit / atv_hypos")
    a = ap.parse_args()
    modes = tuple(m.strip() for m in a.modes.split(","))
    assert torch.cuda.is_available(), "bench_hypos.py measures on an MI355X; there is no CPU path"
    fit, spread = lib().mdf_hypos_fit_fwd, lib().mdf_atv_spread_fwd
    for h, w, D, pp, d_next in SHAPES:
        prob, _, _ = M.make_probs(1, D, h, w, 7)
        hyp = M.make_hypos(1, D, h, w, pp, 7)
        if pp:      # hypotheses as the pipeline makes them: a few millimetres around the regressed depth
            centre = np.random.RandomState(3).uniform(450, 900, (1, 1, h, w))
            hyp = (centre + np.linspace(-30, 30, D).reshape(1, D, 1, 1)).astype(np.float32)
        pg, hg = torch.from_numpy(prob).to(DEV), torch.from_numpy(hyp).to(DEV)
        dg = ops.depth_regress(pg, hg)
        out = torch.empty((1, h, w), device=DEV)
        stream = ops._stream(out)
        calls = {}
        for m in modes:
            if m == "atv":
                calls["atv spread"] = (spread, (pg.data_ptr(), dg.data_ptr(), hg.data_ptr(), int(pp), ctypes.c_float(1.5), out.data_ptr(), 1, D, h, w, stream))
            else:
                calls["mode " + m] = (fit, (int(m), pg.data_ptr(), dg.data_ptr(), hg.data_ptr(), int(pp), None, out.data_ptr(), 1, D, h, w, stream))
        nbytes = {name: traffic(name.split()[0] if name.startswith("atv") else name.split()[1], D, h * w, pp) for name in calls}
        report(f"{h}x{w} D={D} {'per-pixel' if pp else 'shared'}", measure(calls, a.launches, a.rounds), nbytes)
        if a.no_step2:
            continue
        # step 2 on one map of each kind: the laplace fit's s, the atv spread
        sg, eg = ops.hypos_fit(2, pg, dg, hg), ops.atv_spread(pg, dg, hg, 1.5)
        rng = torch.tensor([[425.0, 935.0]], device=DEV)
        hout = torch.empty((1, d_next, 2 * h, 2 * w), device=DEV)
        log_thr = float(torch.log(torch.tensor(1e-5)))
        calls = {"hypos_from_fit": (lib().mdf_hypos_from_fit_fwd, (2, sg.data_ptr(), dg.data_ptr(), rng.data_ptr(), ctypes.c_float(log_thr), hout.data_ptr(),
                                                                   1, d_next, h, w, 1, stream)),
                 "atv_hypos": (lib().mdf_atv_hypos_fwd, (eg.data_ptr(), dg.data_ptr(), hout.data_ptr(), 1, d_next, h, w, 1, stream))}
        by = 4 * h * w * (2 + 4 * d_next)
        report(f"{h}x{w} -> {2 * h}x{2 * w} D_out={d_next}", measure(calls, a.launches, a.rounds), {k: by for k in calls})


if __name__ == "__main__":
    main()
