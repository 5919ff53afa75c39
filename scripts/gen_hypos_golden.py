"""Generate tests/golden/hypos_curves.npz from the REAL reference's net/unit/depthhypos.py:HyposByFit (build container only).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_hypos_golden.py

Loads the reference's depthhypos.py from MDF_REFERENCE (read-only; never copied) and feeds it the inputs tests/golden/ops.npz
already holds: the stage 0 -> 1 transition (reg0_prob, reg0_depth, agg0_hyp: 48 hypotheses shared by all pixels) and the stage
1 -> 2 transition (reg1_prob, reg1_depth, agg1_hyp: 24 hypotheses per pixel), with the depth range of the scene those were made
from.  For gauss0 on both transitions, gauss1 on 1 -> 2 and laplace on 0 -> 1 (the curve / transition pairs the default composition
does not run) it records
  <case>_s32   the fit's s in the reference's fp32,
  <case>_s64   the same function called on .double() inputs: the yardstick of hypos_fit modes 3 and 4,
  <case>_out   forward(..., upsample=True) in fp32,
and <case>_ndepths, <case>_thresh, depth_range.  Arrays only."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MDF_REFERENCE", "/root/reference")
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mdfnet_hip import synth  # noqa: E402

# case -> (curve, transition, ndepths of the stage that is fed, threshold)
CASES = {"gauss0_01": ("gauss0", 0, 24, 0.95), "gauss0_12": ("gauss0", 1, 8, 0.95), "gauss1_12": ("gauss1", 1, 8, 0.95),
         "laplace_01": ("laplace", 0, 24, 1e-5)}
FITS = {"gauss0": "_gauss_fitting0", "gauss1": "_gauss_fitting1", "laplace": "_laplace_fitting"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hypos_curves.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_depthhypos", os.path.join(REF, "net", "unit", "depthhypos.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ops.npz"))
    dr = synth.make_scene(96, 64, 3, batch=2, rot_deg=4.0, seed=5)[3]      # the scene of ops.npz (oracle/gen_golden.py)
    out = {"depth_range": dr.numpy()}
    torch.set_num_threads(1)
    for case, (curve, st, nd, thr) in CASES.items():
        prob, depth, hyp = (torch.from_numpy(g[f"{k}"]) for k in (f"reg{st}_prob", f"reg{st}_depth", f"agg{st}_hyp"))
        mod = ref.HyposByFit(nd, curve, thr)
        fit = getattr(mod, FITS[curve])
        args = (depth, prob, hyp)
        out[f"{case}_s32"] = fit(*args).numpy()
        out[f"{case}_s64"] = fit(*(t.double() for t in args)).numpy()
        out[f"{case}_out"] = mod(depth, dr, prob, hyp, upsample=True).numpy()
        out[f"{case}_ndepths"], out[f"{case}_thresh"] = np.int32(nd), np.float64(thr)
        assert out[f"{case}_s32"].dtype == np.float32 and out[f"{case}_s64"].dtype == np.float64
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
