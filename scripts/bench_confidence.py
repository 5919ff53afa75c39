"""The three launches of the cascade confidence (eval.py --confidence cascade) at the DTU stage shapes, against the one launch of the
default path (confidence_up2_kernel at 8x592x800) in the same process, alternating.  dev tool; needs an MI355X.

    python scripts/bench_confidence.py [--launches 200] [--rounds 9] [--only NAME] [--out profiles/confidence_cascade_bench.json]

    stage0   confidence_cascade_kernel<0>   48 x 148 x 200, no last                  -> 148 x 200
    stage1   confidence_cascade_kernel<0>   24 x 296 x 400, last 148 x 200           -> 296 x 400
    stage2   confidence_cascade_kernel<8>    8 x 592 x 800, last 296 x 400, up2      -> 1184 x 1600
    up2      confidence_up2_kernel<8>        8 x 592 x 800                           -> 1184 x 1600     (the default path's launch)

Bytes per launch are the algorithmic ones: the volume and `last` read once, the map written once.  Timing: HIP events around a window
of `launches` back-to-back launches of one configuration through the C ABI with prebuilt arguments (no allocation, no Python wrapper
in the window); the configurations take turns, `rounds` windows each, after a warm-up window of each; median, minimum and maximum
over the windows.  Every launch of a window works on the next of a ring of input / output sets that together exceed the 256 MiB
Infinity Cache twice, so the bytes come from HBM as they do in a forward (one set only: --ring 1).  The host time of enqueueing a
window is recorded beside it: where it is not clearly below the event time, the window measured the launch path and not the kernel
("launch_bound": true) and the bytes/s is a lower bound.  The kernels' own times come from a kernel trace, one run per configuration:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_confidence.py --only stage2 --launches 100 --rounds 2"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "mdf-net_amd"), os.path.join(R, "tests")]
import torch  # noqa: E402

from mdfnet_hip import check, lib, ops  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X (6.3e12 achievable by a float4 copy)
DEV = "cuda:0"
# name -> (kernel, D, H, W, has last, up2)
CONFIGS = {"stage0": ("confidence_cascade_kernel", 48, 148, 200, False, False), "stage1": ("confidence_cascade_kernel", 24, 296, 400, True, False),
           "stage2": ("confidence_cascade_kernel", 8, 592, 800, True, True), "up2": ("confidence_up2_kernel", 8, 592, 800, False, True)}


def traffic(D, H, W, last, up2):
    return 4 * (D * H * W + (H // 2) * (W // 2) * int(last) + H * W * (4 if up2 else 1))


def softmax_volume(D, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.softmax(torch.randn(1, D, H, W, device=DEV, generator=g) * 3.0, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--only", default=None, choices=list(CONFIGS))
    ap.add_argument("--ring", type=int, default=0, help="input / output sets per configuration (0: enough for 2 x 256 MiB)")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "confidence_cascade_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_confidence.py measures on an MI355X; there is no CPU path"
    names = [a.only] if a.only else list(CONFIGS)
    l = lib()
    calls, keep = {}, []
    for name in names:
        kernel, D, H, W, has_last, up2 = CONFIGS[name]
        by = traffic(D, H, W, has_last, up2)
        ring = a.ring or min(128, -(-2 * 256 * 1024 * 1024 // by))
        sets = []
        for r in range(ring):
            prob = softmax_volume(D, H, W, 100 + r)
            last = torch.rand(1, H // 2, W // 2, device=DEV) if has_last else None
            out = torch.empty((1, 2 * H, 2 * W) if up2 else (1, H, W), device=DEV)
            keep.append((prob, last, out))
            st = ops._stream(out)
            if kernel == "confidence_up2_kernel":
                sets.append((l.mdf_confidence_up2_fwd, (prob.data_ptr(), out.data_ptr(), 1, D, H, W, st)))
            else:
                sets.append((l.mdf_confidence_cascade_fwd, (prob.data_ptr(), last.data_ptr() if has_last else None, ctypes.c_float(0.8),
                                                            ctypes.c_float(0.2), 4, 1, int(up2), out.data_ptr(), 1, D, H, W, st)))
        calls[name] = sets
    torch.cuda.synchronize()

    def window(name):
        sets = calls[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        rc = 0
        for i in range(a.launches):
            fn, args = sets[i % len(sets)]
            rc |= fn(*args)
        e1.record()
        host_us = (time.perf_counter() - t0) * 1e6 / a.launches
        torch.cuda.synchronize()
        check(rc, name)
        return e0.elapsed_time(e1) * 1e3 / a.launches, host_us
    for name in names:
        window(name)
    res = {name: [] for name in names}
    for _ in range(a.rounds):
        for name in names:
            res[name].append(window(name))
    report = {"device": torch.cuda.get_device_name(0), "launches_per_window": a.launches, "rounds": a.rounds, "hbm_peak_bytes_per_s": HBM_PEAK,
              "method": "HIP events around windows of back-to-back launches over a ring of buffer sets, configurations alternating", "configs": {}}
    for name in names:
        kernel, D, H, W, has_last, up2 = CONFIGS[name]
        ts, hs = [t for t, _ in res[name]], [h for _, h in res[name]]
        med, host = statistics.median(ts), statistics.median(hs)
        by = traffic(D, H, W, has_last, up2)
        bound = host >= 0.8 * med
        report["configs"][name] = {"kernel": kernel, "D": D, "H": H, "W": W, "last": has_last, "up2": up2, "bytes": by, "ring": len(calls[name]),
                                   "us_median": round(med, 3), "us_min": round(min(ts), 3), "us_max": round(max(ts), 3),
                                   "host_enqueue_us_median": round(host, 3), "launch_bound": bool(bound),
                                   "bytes_per_s_at_median": by / (med * 1e-6), "share_of_hbm_peak": by / (med * 1e-6) / HBM_PEAK}
        print(f"{name:7s} {kernel:26s} {D:2d}x{H}x{W}: median {med:6.2f} us  min {min(ts):6.2f}  max {max(ts):6.2f}  (host enqueue {host:5.2f} us)  "
              f"{by / 1e6:6.2f} MB  {by / (med * 1e-6) / 1e12:5.2f} TB/s = {by / (med * 1e-6) / HBM_PEAK * 100:5.1f} % of HBM peak"
              + ("   [window bound by the launch path, not the kernel]" if bound else ""))
    if not a.only:
        c = report["configs"]
        total = sum(c[n]["us_median"] for n in ("stage0", "stage1", "stage2"))
        report["cascade_three_launches_us"] = round(total, 3)
        report["default_one_launch_us"] = c["up2"]["us_median"]
        report["stage2_over_up2"] = round(c["stage2"]["us_median"] / c["up2"]["us_median"], 4)
        print(f"cascade: {total:.2f} us in three launches against {c['up2']['us_median']:.2f} us for the default path's one; "
              f"stage2 / up2 = {report['stage2_over_up2']:.3f}")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
