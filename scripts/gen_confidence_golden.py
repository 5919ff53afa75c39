"""Generate tests/golden/confidence_cascade.npz from the REAL reference's net/unit/regress.py:confidence_regress (build container only).

    MDF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python scripts/gen_confidence_golden.py

Loads the reference's regress.py from MDF_REFERENCE (read-only; never copied) and feeds it the three probability volumes
tests/golden/ops.npz already holds (reg0_prob [2,48,8,12], reg1_prob [2,24,16,24], reg2_prob [2,8,32,48]).  It records
  chain32_c{0,1,2}   c0 = f(p0), c1 = f(p1, c0), c2 = f(p2, c1) in the reference's fp32,
  chain64_c{0,1,2}   the same chain on .double() inputs: the yardstick of the cascade kernel,
  n2_32_c{s}, n2_64_c{s}   one call with n=2, pad=(0,0,0,0,0,1) per volume (no last confidence),
  up_prob [2,5,10,14], up_last [2,5,7] (seeded), up_32, up_64   one call with a last confidence that is not a confidence map:
                     uniform in [-0.25, 1.25], so every tap and weight of the bicubic x2 shows.
The float64 yardstick means something only where fp32 and float64 pick the same index trunc(E[d]) at every pixel: asserted here.
Arrays only."""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _indices_agree(ref, prob):
    """trunc(E[d]) of the reference's own expression in fp32 and on .double() inputs -> (all equal, smallest distance of E[d] from
    an integer in float64)."""
    def index(p):
        b, d = p.shape[:2]
        ramp = torch.arange(d, dtype=torch.float).view(1, d, 1, 1).repeat(b, 1, 1, 1)
        return ref.depth_regression(p, ramp)
    e32, e64 = index(prob), index(prob.double())
    return bool((e32.long() == e64.long()).all()), float((e64 - e64.round()).abs().min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "confidence_cascade.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_regress", os.path.join(os.environ["MDF_REFERENCE"], "net", "unit", "regress.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    f = ref.confidence_regress
    g = np.load(os.path.join(ROOT, "tests", "golden", "ops.npz"))
    torch.set_num_threads(1)
    probs = [torch.from_numpy(g[f"reg{s}_prob"]) for s in range(3)]
    out = {}
    for tag, cast in (("32", lambda t: t), ("64", lambda t: t.double())):
        c = None
        for s, p in enumerate(probs):
            c = f(cast(p), c)
            out[f"chain{tag}_c{s}"] = c.numpy()
            out[f"n2_{tag}_c{s}"] = f(cast(p), None, n=2, pad=(0, 0, 0, 0, 0, 1)).numpy()
    rs = np.random.RandomState(24)      # (a seed whose E[d] stays 5e-3 away from every integer: the index is safe in any fp32 order)
    z = rs.standard_normal((2, 5, 10, 14)).astype(np.float32) * np.float32(2)
    z = np.exp(z - z.max(1, keepdims=True))
    up_prob = torch.from_numpy((z / z.sum(1, keepdims=True)).astype(np.float32))
    up_last = torch.from_numpy(rs.uniform(-0.25, 1.25, (2, 5, 7)).astype(np.float32))
    out["up_prob"], out["up_last"] = up_prob.numpy(), up_last.numpy()
    out["up_32"] = f(up_prob, up_last).numpy()
    out["up_64"] = f(up_prob.double(), up_last.double()).numpy()
    for name, p in [(f"reg{s}_prob", p) for s, p in enumerate(probs)] + [("up_prob", up_prob)]:
        same, gap = _indices_agree(ref, p)
        print(f"{name}: fp32 and float64 indices agree: {same}; smallest |E[d] - integer| = {gap:.3e}")
        assert same, f"{name}: fp32 and float64 pick different depth indices; the float64 yardstick does not hold there"
    for k, v in out.items():
        assert v.dtype == (np.float64 if "64" in k else np.float32), (k, v.dtype)
    for s in range(3):
        print(f"stage {s}: max |fp32 - float64| along the chain = {np.abs(out[f'chain32_c{s}'] - out[f'chain64_c{s}']).max():.3e}; "
              f"range of c{s} = [{out[f'chain64_c{s}'].min():.4f}, {out[f'chain64_c{s}'].max():.4f}]")
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
