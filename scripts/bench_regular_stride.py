"""The depth-preserving (1,2,2) sampling layers of RegularNet_4Scales at the volumes the stage-1 and stage-2 regularisers of BASELINE
config 2 give them, beside the (2,2,2) launch of the same channel pair at ITS cfg2 volume, and the whole regulariser forward for both
strides (dev tool; a record of cost, not a gate).
usage: python scripts/bench_regular_stride.py [--out profiles/regular_stride_122.md] [--rounds 5] [--iters 20] [--label TEXT] [--routes]
--routes adds a table of every (1,2,2) layer under MDF_CONV3D_HW_ROUTE = 0 (the rule) / 1 / 2 / 3, alternating (what the launch rule
of conv3d_hw.hip is read from).

Timing: device events around `iters` back-to-back launches, after a warm-up of every shape; `rounds` rounds that alternate the two
strides inside one process; the table reports the median round and the spread (min .. max) of the rounds."""
import argparse
import contextlib
import io
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R + "/mdf-net_amd"]
import torch  # noqa: E402
from mdfnet_hip import ops  # noqa: E402

DEV = "cuda:0"
# cfg2 cost volumes of the two RegularNet_4Scales slots: (stage, in_chs, D, H, W)
STAGES = [(1, 16, 24, 296, 400), (2, 8, 8, 592, 800)]
# (layer, cin, cout, transposed, level of its INPUT): level l has H, W >> l (and, for (2,2,2), D >> l)
LAYERS = [("conv12.0", 8, 16, False, 0), ("conv23.0", 16, 32, False, 1), ("conv343.0", 32, 64, False, 2),
          ("conv343.2T", 64, 32, True, 3), ("trconv32T", 32, 16, True, 2), ("trconv21T", 16, 8, True, 1)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def alternate(fns, rounds, iters):
    """-> per fn (median us, min us, max us) over `rounds` rounds that alternate the fns."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ts[i].append(timed(fn, iters))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def layer_call(cin, cout, tr, d, h, w, stride):
    """One sampling layer with its fused epilogue (folded BN, ReLU; the skip tensor for the transposed layers, as in the U-Net)."""
    x = torch.randn(1, d, h, w, cin, device=DEV)
    wt = torch.randn(*((cin, cout) if tr else (cout, cin)), 3, 3, 3, device=DEV) / (27 * cin) ** 0.5
    wp = ops.pack_conv3d_weight(wt, tr)
    al, be = torch.rand(cout, device=DEV) + 0.5, torch.randn(cout, device=DEV) * 0.1
    y = ops.conv3d_ndhwc(x, wp, cin, cout, stride, tr, al, be, True)
    skip = torch.randn_like(y) if tr else None
    vox = d * h * w if tr else y.shape[1] * y.shape[2] * y.shape[3]
    return (lambda: ops.conv3d_ndhwc(x, wp, cin, cout, stride, tr, al, be, True, skip)), 2.0 * 27 * cin * cout * vox


def regulariser(in_chs, stride, pad):
    from net.unit.regular import RegularNet_4Scales
    torch.manual_seed(in_chs)
    return RegularNet_4Scales(in_chs, 8, stride, pad).eval().to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "regular_stride_122.md"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--routes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regular_stride.py measures on a GPU; there is none (not measured)")
    lines = ["# RegularNet_4Scales, sample_stride (1,2,2) against (2,2,2): cfg2 volumes", "",
             f"`scripts/bench_regular_stride.py --rounds {args.rounds} --iters {args.iters}{' --routes' if args.routes else ''}` on {torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?').split(':')[0]})"
             + (f", {args.label}" if args.label else "") + ".",
             "Device events around back-to-back launches after a warm-up, the two strides alternating inside one process; median round",
             "(min .. max of the rounds).  TFLOP/s: 2 x 27 x Cin x Cout x voxels of the M index space over the median.  The (1,2,2) net does",
             "2x / 4x / 8x the work of (2,2,2) at the three lower levels by construction: a record of cost, not a verdict.  The launch rule",
             "(conv3d_hw.hip: launch_hw_mt) is read from the route table of `--routes`; volumes other than these twelve are not measured.", "",
             "## Sampling layers (fused BN + ReLU; the transposed layers with their skip tensor)", "",
             "| stage | layer | Cin->Cout | (1,2,2) input DxHxW | us (min .. max) | TFLOP/s | (2,2,2) input DxHxW | us (min .. max) | TFLOP/s |",
             "|---|---|---|---|---|---|---|---|---|"]
    for stage, _, D, H, W in STAGES:
        for name, cin, cout, tr, lvl in LAYERS:
            h, w = H >> lvl, W >> lvl
            d2 = max(D >> lvl, 1)
            f_new, fl_new = layer_call(cin, cout, tr, D, h, w, (1, 2, 2))
            f_old, fl_old = layer_call(cin, cout, tr, d2, h, w, 2)
            (m1, lo1, hi1), (m2, lo2, hi2) = alternate([f_new, f_old], args.rounds, args.iters)
            row = (f"| {stage} | {name} | {cin}->{cout}{' T' if tr else ''} | {D}x{h}x{w} | {m1:.1f} ({lo1:.1f} .. {hi1:.1f}) | {fl_new / m1 / 1e6:.2f} | "
                   f"{d2}x{h}x{w} | {m2:.1f} ({lo2:.1f} .. {hi2:.1f}) | {fl_old / m2 / 1e6:.2f} |")
            print(row, flush=True)
            lines.append(row)
            del f_new, f_old
            torch.cuda.empty_cache()
    if args.routes:
        lines += ["", "## (1,2,2) layers by route (MDF_CONV3D_HW_ROUTE: 0 the rule, 1 one tile per wave, 2 the largest wave tile, 3 split-K where built)", "",
                  "| stage | layer | Cin->Cout | input DxHxW | rule us | route 1 us | route 2 us | route 3 us |", "|---|---|---|---|---|---|---|---|"]
        for stage, _, D, H, W in STAGES:
            for name, cin, cout, tr, lvl in LAYERS:
                h, w = H >> lvl, W >> lvl
                f_new, _ = layer_call(cin, cout, tr, D, h, w, (1, 2, 2))

                def routed(r, f=f_new):
                    def call():
                        os.environ["MDF_CONV3D_HW_ROUTE"] = r      # (read per call by the library)
                        f()
                    return call
                split_built = (cin >= 64) if tr else (cin >= 32)
                res = alternate([routed(r) for r in ("0", "1", "2", "3")], args.rounds, args.iters)
                os.environ.pop("MDF_CONV3D_HW_ROUTE", None)
                cells = [f"{m:.1f} ({lo:.1f} .. {hi:.1f})" for m, lo, hi in res]
                if not split_built:
                    cells[3] = "= route 1"
                row = f"| {stage} | {name} | {cin}->{cout}{' T' if tr else ''} | {D}x{h}x{w} | " + " | ".join(cells) + " |"
                print(row, flush=True)
                lines.append(row)
                del f_new
                torch.cuda.empty_cache()
    lines += ["", "## Whole regulariser forward (cost volume -> prob, soft-argmin depth), random weights, eval", "",
              "| stage | cost volume CxDxHxW | (1,2,2) us (min .. max) | (2,2,2) us (min .. max) | ratio |", "|---|---|---|---|---|"]
    for stage, C, D, H, W in STAGES:
        cost = torch.randn(1, C, D, H, W, device=DEV)
        hyp = torch.sort(torch.rand(1, D, H, W, device=DEV) * 500 + 400, dim=1)[0]
        with contextlib.redirect_stdout(io.StringIO()):
            m_new, m_old = regulariser(C, (1, 2, 2), (0, 1, 1)), regulariser(C, (2, 2, 2), (1, 1, 1))
        with torch.no_grad():
            (a, alo, ahi), (b, blo, bhi) = alternate([lambda: m_new(cost, hyp), lambda: m_old(cost, hyp)], args.rounds, max(args.iters // 4, 3))
        row = f"| {stage} | {C}x{D}x{H}x{W} | {a:.0f} ({alo:.0f} .. {ahi:.0f}) | {b:.0f} ({blo:.0f} .. {bhi:.0f}) | {a / b:.2f} |"
        print(row, flush=True)
        lines.append(row)
        del cost, hyp, m_new, m_old
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
