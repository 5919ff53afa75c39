"""Image undistortion (ops.undistort_images: mdf_image_undistort) on generated --width x --height photographs (default 6000 x 4000), an
OPENCV and an OPENCV_FISHEYE camera, at full size (s = 1, one sample a pixel) and at --max_dim (default 3000: s = 0.5, 2 x 2
samples), with the plan tools/colmap/main.py --undistort would make (zoom fitted inside).

Per case: the kernel's time (HIP events around the launch, median and minimum of --repeats after a warm-up, one image and a group of
eight), the bytes the algorithm has to move (the source read once, the output written once) over that time, and beside it a plain
device-to-device copy that moves the same number of bytes (half read, half written), timed in the same run.  Then, for one
photograph, where the wall time of the importer's loop goes: JPEG decode, host-to-device, kernel, device-to-host, JPEG encode
(quality 95), each ended by a device synchronise where the GPU is involved.  There is no pass bar.
  python scripts/bench_undistort.py [--width 6000 --height 4000] [--max_dim 3000] [--repeats 20] [--out profiles/undistort_bench.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def photograph(h, w, seed):
    """A smooth colour image with fine noise on it [h,w,3] uint8 (what a JPEG codec spends realistic time on)."""
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ch = [127.5 + 100.0 * np.sin(rng.uniform(0.002, 0.02) * xx + rng.uniform(0, 6)) * np.cos(rng.uniform(0.002, 0.02) * yy) for _ in range(3)]
    img = np.stack(ch, axis=2) + rng.normal(0.0, 6.0, (h, w, 3)).astype(np.float32)
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def event_ms(fn, repeats):
    """Median and minimum over `repeats` of the device time of fn() (events on the current stream), after one warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def wall(fn, sync):
    import torch
    t0 = time.perf_counter()
    r = fn()
    if sync:
        torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6000)
    ap.add_argument("--height", type=int, default=4000)
    ap.add_argument("--max_dim", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from mdfnet_hip import ops
    from tools.colmap import undistort as UD
    assert torch.cuda.is_available(), "bench_undistort.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    w, h = a.width, a.height
    f = 0.8 * w
    cameras = {"OPENCV": ("OPENCV", w, h, [f, 0.99 * f, w / 2 + 3.5, h / 2 - 5.25, 0.09, 0.02, 0.001, -0.0005]),
               "OPENCV_FISHEYE": ("OPENCV_FISHEYE", w, h, [f, 0.99 * f, w / 2 + 3.5, h / 2 - 5.25, 0.05, -0.01, 0.003, -0.001])}
    img = photograph(h, w, 1)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=95)
    jpeg = buf.getvalue()
    res = {"width": w, "height": h, "max_dim": a.max_dim, "repeats": a.repeats, "jpeg_bytes": len(jpeg), "cases": []}
    for model, cam in cameras.items():
        for max_dim in (0, a.max_dim):
            t0 = time.perf_counter()
            p = UD.plan(cam, max_dim, "inside")
            t_plan = (time.perf_counter() - t0) * 1e3
            ow, oh = p["out_size"]
            run = lambda s: ops.undistort_images(s, p["kind"], p["coeffs"], p["fx"], p["fy"], p["cx"], p["cy"], (oh, ow), zoom=p["z"],
                                                 scale=p["s"], nsub=p["n"])
            case = {"model": model, "s": p["s"], "nsub": p["n"], "zoom": p["z"], "out": [ow, oh], "plan_ms": round(t_plan, 2), "kernel": {}}
            for b in (1, 8):
                src = torch.from_numpy(img).to(dev)[None].repeat(b, 1, 1, 1).contiguous()
                nbytes = b * 3 * (w * h + ow * oh)                       # the source read once, the output written once
                half = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
                other = torch.empty_like(half)
                med, mn = event_ms(lambda: run(src), a.repeats)
                cmed, cmn = event_ms(lambda: other.copy_(half), a.repeats)
                case["kernel"][f"B{b}"] = {"ms_median": round(med, 4), "ms_min": round(mn, 4), "bytes": nbytes,
                                           "GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1),
                                           "samples_per_s": round(b * ow * oh * p["n"] ** 2 / (med * 1e-3), 0),
                                           "copy_ms_median": round(cmed, 4), "copy_ms_min": round(cmn, 4),
                                           "copy_GB_per_s": round(2 * (nbytes // 2) / (cmed * 1e-3) / 1e9, 1)}
                del src, half, other
            # one photograph through the importer's loop
            split = {k: [] for k in ("decode", "h2d", "kernel", "d2h", "encode")}
            for _ in range(3):
                arr, t = wall(lambda: np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"), dtype=np.uint8)), False)
                split["decode"].append(t)
                g, t = wall(lambda: torch.from_numpy(arr[None]).to(dev), True)
                split["h2d"].append(t)
                d, t = wall(lambda: run(g), True)
                split["kernel"].append(t)
                out, t = wall(lambda: d.cpu().numpy(), True)
                split["d2h"].append(t)
                _, t = wall(lambda: Image.fromarray(out[0]).save(io.BytesIO(), format="JPEG", quality=95), False)
                split["encode"].append(t)
            case["wall_ms_one_image"] = {k: round(min(v), 3) for k, v in split.items()}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
