"""Generate tests/golden/atv_hypos.npz from the REAL reference's net/unit/depthhypos.py:atv_hypos (build container only).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_atv_golden.py

Loads the reference's depthhypos.py from MDF_REFERENCE (read-only; never copied) and feeds it the inputs tests/golden/ops.npz
already holds: the stage 0 -> 1 transition (reg0_prob, reg0_depth, agg0_hyp: 48 hypotheses shared by all pixels) and the stage
1 -> 2 transition (reg1_prob, reg1_depth, agg1_hyp: 24 hypotheses per pixel), with the depth range of the scene those were made
from.  Nothing in the reference computes atv_hypos' second argument; it is UCS-Net's exp_variance,
    e = scale * sqrt(sum_d p_d (x_d - depth)^2),
written here in torch.  Two scales per transition: UCS-Net's 1.5, where e < depth at every pixel, and one wide enough that e2 > d2
at about half of the output pixels, so that both branches of atv_hypos' min run.  Per case it records
  <case>_e32     the spread in torch fp32,
  <case>_e64     the same expression on .double() inputs,
  <case>_out32   atv_hypos(bilinear x2 of the depth [B,1,2h,2w], e32, depth_range, ndepths) in fp32,
  <case>_out64   the same call on doubles with e64,
and <case>_ndepths, <case>_scale, depth_range.  Arrays only."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MDF_REFERENCE", "/root/reference")
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mdfnet_hip import synth  # noqa: E402

# case -> (transition, ndepths of the stage that is fed, scale)
CASES = {"atv_01": (0, 24, 1.5), "atv_12": (1, 8, 1.5), "atv_01_wide": (0, 24, 4.0), "atv_12_wide": (1, 8, 40.0)}


def spread(scale, prob, depth, hyp):
    return scale * torch.sqrt(torch.sum(prob * (hyp - depth.unsqueeze(1)) ** 2, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "atv_hypos.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_depthhypos", os.path.join(REF, "net", "unit", "depthhypos.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ops.npz"))
    dr = synth.make_scene(96, 64, 3, batch=2, rot_deg=4.0, seed=5)[3]      # the scene of ops.npz (oracle/gen_golden.py)
    out = {"depth_range": dr.numpy()}
    torch.set_num_threads(1)
    for case, (st, nd, scale) in CASES.items():
        prob, depth, hyp = (torch.from_numpy(g[k]) for k in (f"reg{st}_prob", f"reg{st}_depth", f"agg{st}_hyp"))
        for tag, cast in (("32", lambda t: t), ("64", lambda t: t.double())):
            p, d, x = cast(prob), cast(depth), cast(hyp)
            e = spread(scale, p, d, x)
            d2 = F.interpolate(d.unsqueeze(1), scale_factor=2, mode="bilinear")
            out[f"{case}_e{tag}"] = e.numpy()
            out[f"{case}_out{tag}"] = ref.atv_hypos(d2, e, dr, nd).numpy()
        out[f"{case}_ndepths"], out[f"{case}_scale"] = np.int32(nd), np.float64(scale)
        assert out[f"{case}_e32"].dtype == out[f"{case}_out32"].dtype == np.float32
        assert out[f"{case}_e64"].dtype == out[f"{case}_out64"].dtype == np.float64
        e2 = F.interpolate(torch.from_numpy(out[f"{case}_e32"]).unsqueeze(1), scale_factor=2, mode="bilinear")
        d2 = F.interpolate(depth.unsqueeze(1), scale_factor=2, mode="bilinear")
        print(f"{case}: e2 > d2 at {float((e2 > d2).float().mean()) * 100:.1f} % of the output pixels; hypotheses "
              f"{out[f'{case}_out32'].min():.1f} .. {out[f'{case}_out32'].max():.1f}")
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
