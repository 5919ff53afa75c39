"""The validation metrics' two launches (depth_metrics_reduce_multi_kernel + depth_metrics_finalize_kernel) over the four maps of one
item, at the DTU training size and at the eval size, against the stock-torch formulation of the same tables on the same card, and one
validation item end to end.  dev tool; needs an MI355X.

    python scripts/bench_depth_metrics.py [--launches 100] [--rounds 9] [--out profiles/depth_metrics_bench.json]

    train   80x64 (48 shared hypotheses), 160x128 (24 per pixel), 320x256 (8 per pixel), 640x512 (confidence);  B = 1
    eval    200x148, 400x296, 800x592, 1600x1184 in the same roles
    *_smooth the same with a smooth confidence map (a wave's 64 neighbouring pixels fall into one or two bins, as a network's
            confidence does; the plain configurations draw it uniformly at random, so every wave meets all 32 bins: the worst case
            of the wave-level binning)

Bytes per call are the algorithmic ones: est and gt of every map, the first and last hypothesis plane where they are per pixel, the
confidence map, plus the block partials written by the reduction and read by the finalize.  Timing: HIP events around a window of
`launches` back-to-back calls (reduce + finalize) through the C ABI with prebuilt arguments; every call of a window works on the next
of a ring of input sets that together exceed the 256 MiB Infinity Cache twice (capped at 64 sets), so the bytes come from HBM; the
hand-written path and the torch formulation take turns, `rounds` windows each after a warm-up window; median, minimum, maximum.  The
host time of enqueueing a window is recorded beside it: where it is not clearly below the event time the window measured the launch
path ("launch_bound": true).  The item: an eval-mode forward (5 views, 640x512, seeded weights) with the stage tap + the metrics call
against the forward alone, host clock around a synchronise, alternating."""
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
CONFIGS = {"train": (640, 512, False), "train_smooth": (640, 512, True), "eval": (1600, 1184, False), "eval_smooth": (1600, 1184, True)}
DEPTHS = (48, 24, 8)


def make_set(W, H, seed, smooth=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    maps = []
    for s, d in zip((3, 2, 1), DEPTHS):
        h, w = H >> s, W >> s
        gt = 450 + 400 * torch.rand(1, h, w, device=DEV, generator=g)
        gt[torch.rand(1, h, w, device=DEV, generator=g) < 0.15] = 0
        est = gt + 5 * torch.randn(1, h, w, device=DEV, generator=g)
        if s == 3:
            hyp = torch.linspace(425, 935, d, device=DEV).reshape(1, d, 1, 1).contiguous()
        else:
            hyp = (gt.unsqueeze(1) + torch.linspace(-20, 20, d, device=DEV).reshape(1, d, 1, 1)).contiguous()
        maps.append({"est": est, "gt": gt, "hypos": hyp})
    gt = 450 + 400 * torch.rand(1, H, W, device=DEV, generator=g)
    est = gt + 5 * torch.randn(1, H, W, device=DEV, generator=g)
    if smooth:
        yy, xx = torch.meshgrid(torch.arange(H, device=DEV) / H, torch.arange(W, device=DEV) / W, indexing="ij")
        conf = (0.5 + 0.5 * torch.sin(3.0 * xx + 0.1 * seed) * torch.cos(2.0 * yy)).reshape(1, H, W).contiguous()
    else:
        conf = torch.rand(1, H, W, device=DEV, generator=g) * 1.1 - 0.05
    maps.append({"est": est, "gt": gt, "conf": conf})
    return maps


def traffic(maps, ws_bytes):
    by = 0
    for m in maps:
        n = m["est"].numel()
        by += 4 * n * (2 + ("conf" in m) + 2 * ("hypos" in m and m["hypos"].shape[-1] != 1))
    return by + 2 * ws_bytes


def torch_tables(maps, floor, thr):
    """The same tables from stock torch ops (masks, masked float64 sums, bincount for the bins)."""
    out = torch.zeros(len(maps), 33, 9, dtype=torch.float64, device=DEV)
    for i, m in enumerate(maps):
        est, gt = m["est"], m["gt"]
        fin = torch.isfinite(est)
        if "hypos" in m:
            lo, hi = m["hypos"][:, 0].expand_as(est), m["hypos"][:, -1].expand_as(est)
            fin = fin & torch.isfinite(lo) & torch.isfinite(hi)
        if "conf" in m:
            fin = fin & torch.isfinite(m["conf"])
        valid = gt.double() > floor.reshape(-1, 1, 1)
        ok = valid & fin
        e = (est - gt).abs()
        ed = torch.where(ok, e, torch.zeros_like(e)).double()
        out[i, 0, 0] = ok.sum()
        out[i, 0, 1] = (valid & ~fin).sum()
        out[i, 0, 2] = ed.sum()
        under = [ok & (e < thr[:, t].reshape(-1, 1, 1)) for t in range(thr.shape[1])]
        for t, u in enumerate(under):
            out[i, 0, 3 + t] = u.sum()
        if "hypos" in m:
            out[i, 0, 7] = (ok & (lo <= gt) & (gt <= hi)).sum()
            out[i, 0, 8] = torch.where(ok, hi - lo, torch.zeros_like(e)).double().sum()
        if "conf" in m:
            k = torch.clamp(torch.floor(torch.nan_to_num(m["conf"]) * 32.0), 0, 31).long().reshape(-1)
            okf = ok.reshape(-1)
            out[i, 1:, 0] = torch.bincount(k, weights=okf.double(), minlength=32)
            out[i, 1:, 2] = torch.bincount(k, weights=ed.reshape(-1), minlength=32)
            for t, u in enumerate(under):
                out[i, 1:, 3 + t] = torch.bincount(k, weights=u.reshape(-1).double(), minlength=32)
    return out


def prebuilt(maps, floor, thr):
    """-> (call(), keepalive): reduce + finalize through the C ABI with every argument built once."""
    l = lib()
    nm = len(maps)
    arr = lambda vals: (ctypes.c_void_p * nm)(*vals)
    per = (ctypes.c_int64 * nm)(*[m["est"].numel() for m in maps])
    nbytes = l.mdf_depth_metrics_workspace(per, nm, 1)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    table = torch.empty(nm, 33, 9, dtype=torch.float64, device=DEV)
    est, gt = arr([m["est"].data_ptr() for m in maps]), arr([m["gt"].data_ptr() for m in maps])
    hyp = arr([m["hypos"].data_ptr() if "hypos" in m else None for m in maps])
    hd = (ctypes.c_int * nm)(*[m["hypos"].shape[1] if "hypos" in m else 0 for m in maps])
    hpp = (ctypes.c_int * nm)(*[int("hypos" in m and m["hypos"].shape[-1] != 1) for m in maps])
    conf = arr([m["conf"].data_ptr() if "conf" in m else None for m in maps])
    mask = sum(1 << i for i, m in enumerate(maps) if "conf" in m)
    st = ops._stream(table)
    a1 = (est, gt, hyp, hd, hpp, conf, per, nm, floor.data_ptr(), 1, 1, thr.data_ptr(), thr.shape[1], 1, ws.data_ptr(), nbytes, st)
    a2 = (ws.data_ptr(), nbytes, per, nm, 1, mask, table.data_ptr(), st)

    def call():
        return l.mdf_depth_metrics_reduce_multi(*a1) | l.mdf_depth_metrics_finalize(*a2)
    return call, (ws, table, a1, a2), nbytes, table


def stats(ts):
    return {"us_median": round(statistics.median(ts), 3), "us_min": round(min(ts), 3), "us_max": round(max(ts), 3)}


def bench_tables(name, a):
    W, H, smooth = CONFIGS[name]
    floor = torch.tensor([425.0], dtype=torch.float64, device=DEV)
    thr = torch.tensor([[2.0, 4.0, 8.0]], device=DEV)
    probe = make_set(W, H, 0, smooth)
    _, _, ws_bytes, _ = prebuilt(probe, floor, thr)
    by = traffic(probe, ws_bytes)
    ring = min(64, -(-2 * 256 * 1024 * 1024 // by))
    sets = [make_set(W, H, 10 + r, smooth) for r in range(ring)]
    calls = [prebuilt(s, floor, thr) for s in sets]
    # same tables from both formulations (counts equal, sums to float64 rounding) before anything is timed
    rc = calls[0][0]()
    check(rc, name)
    want = torch_tables(sets[0], floor, thr)
    got = calls[0][3]
    torch.cuda.synchronize()
    counts = [0, 1, 3, 4, 5, 6, 7]
    assert torch.equal(got[..., counts], want[..., counts]), "hand-written and torch tables disagree in a count"
    assert torch.allclose(got, want, rtol=1e-11, atol=0), "hand-written and torch tables disagree in a sum"

    def window(kind, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        rc = 0
        for i in range(n):
            if kind == "hip":
                rc |= calls[i % ring][0]()
            else:
                torch_tables(sets[i % ring], floor, thr)
        e1.record()
        host = (time.perf_counter() - t0) * 1e6 / n
        torch.cuda.synchronize()
        check(rc, name)
        return e0.elapsed_time(e1) * 1e3 / n, host
    n_torch = max(4, a.launches // 10)
    window("hip", a.launches), window("torch", n_torch)
    res = {"hip": [], "torch": []}
    for _ in range(a.rounds):
        res["hip"].append(window("hip", a.launches))
        res["torch"].append(window("torch", n_torch))
    out = {"W": W, "H": H, "smooth_confidence": smooth, "maps": [list(m["est"].shape[1:]) for m in probe], "bytes": by, "workspace_bytes": ws_bytes, "ring": ring,
           "hbm_time_us_at_peak": round(by / HBM_PEAK * 1e6, 3)}
    for kind in ("hip", "torch"):
        ts, hs = [t for t, _ in res[kind]], [h for _, h in res[kind]]
        d = stats(ts)
        d["host_enqueue_us_median"] = round(statistics.median(hs), 3)
        d["launch_bound"] = bool(d["host_enqueue_us_median"] >= 0.8 * d["us_median"])
        d["bytes_per_s_at_median"] = by / (d["us_median"] * 1e-6)
        d["share_of_hbm_peak"] = d["bytes_per_s_at_median"] / HBM_PEAK
        out["two_launches" if kind == "hip" else "stock_torch"] = d
        print(f"{name:12s} {kind:5s}: median {d['us_median']:9.2f} us  min {d['us_min']:9.2f}  max {d['us_max']:9.2f}  (host enqueue "
              f"{d['host_enqueue_us_median']:8.2f} us)  {by / 1e6:6.2f} MB  {d['share_of_hbm_peak'] * 100:5.1f} % of HBM peak"
              + ("   [window bound by the launch path]" if d["launch_bound"] else ""))
    out["torch_over_hip"] = round(out["stock_torch"]["us_median"] / out["two_launches"]["us_median"], 2)
    return out


def bench_item(a):
    import contextlib
    import io
    from mdfnet_hip import synth, valmetrics
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        model = config.build_model()
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=1))
    model.eval().to(DEV)
    W, H, V = 640, 512, 5
    from mdfnet_hip import hostmirror
    host = synth.make_scene(W, H, V, batch=1, rot_deg=2.0, seed=3)
    host = (host[0], host[1], host[2], host[3].double())
    imgs, extr, intr, dr = [t.to(DEV) for t in host]
    for d, h in zip((extr, intr, dr), host[1:]):          # the loader's CPU tensors are the host mirrors, as in eval.py
        hostmirror.put(d, h)
    g = torch.Generator(device=DEV).manual_seed(5)
    gt = {str(s): 450 + 400 * torch.rand(1, H >> s, W >> s, device=DEV, generator=g) for s in (3, 2, 1, 0)}
    batch = {"imgs": imgs, "extrinsics": extr, "intrinsics": intr, "depth_range": dr, "ref_depths": gt}
    thr = torch.tensor([[2.0, 4.0, 8.0]], device=DEV)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def plain():
        with torch.no_grad():
            model(imgs, extr, intr, batch["depth_range"])
    item = lambda: valmetrics.validate_batch(model, batch, thr)
    for _ in range(3):
        plain(), item()
    res = {"forward": [], "item": []}
    for _ in range(max(a.rounds, 9)):
        res["forward"].append(timed(plain))
        res["item"].append(timed(item))
    out = {"W": W, "H": H, "views": V, "method": "host clock around a synchronise, forward alone and validation item alternating"}
    for k, ts in res.items():
        out[k] = {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}
    out["metrics_share_of_item"] = round(1 - out["forward"]["ms_median"] / out["item"]["ms_median"], 4)
    print(f"item  : forward {out['forward']['ms_median']:.3f} ms, forward + tap + metrics {out['item']['ms_median']:.3f} ms "
          f"(min {out['item']['ms_min']:.3f}, max {out['item']['ms_max']:.3f})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "depth_metrics_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_metrics.py measures on an MI355X; there is no CPU path"
    report = {"device": torch.cuda.get_device_name(0), "launches_per_window": a.launches, "rounds": a.rounds, "hbm_peak_bytes_per_s": HBM_PEAK,
              "method": "HIP events around windows of back-to-back calls (reduce + finalize) over a ring of input sets, the hand-written "
                        "path and the stock-torch formulation alternating", "configs": {}}
    for name in CONFIGS:
        report["configs"][name] = bench_tables(name, a)
    report["validation_item"] = bench_item(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
