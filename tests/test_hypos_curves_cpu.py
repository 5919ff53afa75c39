"""CPU: the gauss0 and per-pixel gauss1 hypothesis curves (hypos_fit modes 3 and 4) against the reference's code in float64.

tests/golden/hypos_curves.npz (scripts/gen_hypos_golden.py) holds what the reference's HyposByFit gives on the two inter-stage
transitions of tests/golden/ops.npz, in its fp32 and, the yardstick, on .double() inputs.  tests/hypos_oracle.py has the centred
float64 fits, the fp32 mirror of the kernels' operation order and the bound K(D) * 2^-24 * N the GPU tests hold the kernels to."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import heads_mirror as M  # noqa: E402
import hypos_oracle as H  # noqa: E402

T = torch.from_numpy
# case -> (mode, transition: the stage whose outputs are fitted)
CASES = {"gauss0_01": (3, 0), "gauss0_12": (3, 1), "gauss1_12": (4, 1)}


def inputs(golden, st):
    g = golden("ops.npz")
    return g[f"reg{st}_prob"], g[f"reg{st}_depth"], g[f"agg{st}_hyp"]


def fit64(mode, prob, depth, hyp):
    return H.gauss0_fit64(prob, depth, hyp) if mode == 3 else H.gauss1_fit64(prob, hyp)


def fit32(mode, prob, depth, hyp):
    return H.gauss0_fit32(prob, depth, hyp) if mode == 3 else H.gauss1_fit32(prob, hyp)


@pytest.mark.parametrize("case", list(CASES))
def test_centred_float64_fit_is_the_references_float64(golden, case):
    """1/s of the centred float64 fit against the reference's own code on .double() inputs, relative to the map's median |1/s|:
    <= 1e-6.  (The reference's float64 itself carries conditioning noise near 1e-8 in the per-pixel gauss1 case.)"""
    mode, st = CASES[case]
    b0, _, deg = fit64(mode, *inputs(golden, st))
    ref = 1.0 / golden("hypos_curves.npz")[case + "_s64"]
    assert not deg.any()
    err = float(np.max(np.abs(np.abs(b0) - ref)) / np.median(np.abs(ref)))
    print(f"{case}: centred float64 against the reference's float64, max |d(1/s)| / median |1/s| = {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_mirror_meets_the_gpu_bound_on_the_goldens(golden, case):
    """The kernels' operation order in fp32 (correctly rounded log) against the reference's float64 golden: K(D) * 2^-24 * N."""
    mode, st = CASES[case]
    prob, depth, hyp = inputs(golden, st)
    _, n, _ = fit64(mode, prob, depth, hyp)
    b0_ref = 1.0 / golden("hypos_curves.npz")[case + "_s64"]
    r = H.ratio(fit32(mode, prob, depth, hyp), b0_ref, n, mode, prob.shape[1])
    print(f"{case}: fp32 mirror, max error / bound = {float(r.max()):.4f} (K = {H.K(mode, prob.shape[1])})")
    assert (r <= 1).all()


def test_reference_fp32_is_not_the_bar(golden):
    """For the record: the distance of the reference's own fp32 from its float64, in units of the bound.  On the per-pixel gauss1 map
    it is off by orders of magnitude (a 3x3 normal matrix of uncentred x^2, x, 1), which is why bit parity with it is not the bar;
    there the mirror's mean error must be no larger.  For gauss0 both are dominated by the rounding of the logarithm."""
    c = golden("hypos_curves.npz")
    for case, (mode, st) in CASES.items():
        prob, depth, hyp = inputs(golden, st)
        _, n, _ = fit64(mode, prob, depth, hyp)
        b0_ref = 1.0 / c[case + "_s64"]
        ref32 = H.ratio(c[case + "_s32"], b0_ref, n, mode, prob.shape[1])
        mir = H.ratio(fit32(mode, prob, depth, hyp), b0_ref, n, mode, prob.shape[1])
        rel = np.abs(1.0 / c[case + "_s32"].astype(np.float64) - b0_ref) / b0_ref
        print(f"{case}: reference fp32 error / bound: mean {ref32.mean():.3e} max {ref32.max():.3e} (1/s relative: median "
              f"{np.median(rel):.2e} max {rel.max():.2e}); mirror: mean {mir.mean():.3e} max {mir.max():.3e}")
        if case == "gauss1_12":
            assert mir.mean() <= ref32.mean()


def test_mirror_degenerate_pixels_are_nan():
    """Fewer than 2 distinct u (gauss0) / 3 distinct hypotheses (gauss1): 0/0 = NaN, in the mirror as in the float64 fit."""
    for D in (1, 3, 5, 24):
        prob, _, _ = M.make_probs(1, D, 2, 3, D)
        hyp = M.make_hypos(1, D, 2, 3, True, D)
        hyp[0, :, 0, 0] = hyp[0, 0, 0, 0]                      # all equal
        hyp[0, D // 2:, 0, 1] = hyp[0, -1, 0, 1]               # two distinct values (D >= 3)
        hyp[0, :D // 2, 0, 1] = hyp[0, 0, 0, 1]
        depth = M.depth_regress(prob, hyp)
        s0, s1 = H.gauss0_fit32(prob, depth, hyp), H.gauss1_fit32(prob, hyp)
        d0, d1 = H.gauss0_fit64(prob, depth, hyp)[2], H.gauss1_fit64(prob, hyp)[2]
        assert d0[0, 0, 0] and d1[0, 0, 0] and d1[0, 0, 1]
        assert np.array_equal(np.isnan(s0), d0) and np.array_equal(np.isnan(s1), d1), (D, s0, d0, s1, d1)


# --------------------------------------------------------------------------- the slot through the rehearsal backend
@pytest.mark.parametrize("curve,mode", [("gauss0", 3), ("gauss1", 4)])
def test_slot_rehearsal_backend_per_pixel_hypotheses(golden, rehearsal_backend, curve, mode):
    """HyposByFit(8, curve, 0.95) on the stage 1 -> 2 golden inputs (per-pixel hypotheses) through the stock-op backend: the fit
    within the kernels' bound of the reference's float64, [B,8,2h,2w] out, and the hypotheses those of step 2 fed the float64 s."""
    from net.unit.depthhypos import HyposByFit
    from rehearsal import stockops
    prob, depth, hyp = inputs(golden, 1)
    c = golden("hypos_curves.npz")
    case = f"{curve}_12"
    dr = T(c["depth_range"])
    _, n, _ = fit64(mode, prob, depth, hyp)
    s = stockops._fit(curve, T(depth), T(prob), T(hyp)).numpy()
    assert s.dtype == np.float32
    r = H.ratio(s, 1.0 / c[case + "_s64"], n, mode, prob.shape[1])
    print(f"{case}: rehearsal backend fit, max error / bound = {float(r.max()):.4f}")
    assert (r <= 1).all()
    slot = HyposByFit(8, curve, 0.95)
    out = slot(T(depth), dr, T(prob), T(hyp), upsample=True).numpy()
    B, _, h, w = prob.shape
    assert out.shape == (B, 8, 2 * h, 2 * w) and np.isfinite(out).all()
    lt = float(torch.log(torch.tensor(0.95)))
    want = M.hypos_from_fit64(1, c[case + "_s64"].astype(np.float32), depth, dr.numpy(), lt, 8, True)
    # a relative error e of s moves the range sqrt(-s ln t) by e/2 and a hypothesis by at most half the range; the range is capped at
    # 0.2 (hi - lo).  e <= K 2^-24 N / |b0| per pixel, the bilinear blend and step 2's own roundings add a few ulp of the depth
    e = (H.K(mode, prob.shape[1]) * H.EPS * n * c[case + "_s64"]).max()
    span = float((dr[:, 1] - dr[:, 0]).max())
    tol = 0.25 * e * 0.2 * span + 16 * H.EPS * float(dr.max())
    err = float(np.abs(out - want).max())
    print(f"{case}: slot hypotheses against step 2 of the float64 s: max |d| = {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


def test_slot_unknown_curve_still_raises(golden, rehearsal_backend):
    from net.unit.depthhypos import HyposByFit
    prob, depth, hyp = inputs(golden, 1)
    with pytest.raises(NotImplementedError, match="gauss7"):
        HyposByFit(8, "gauss7", 0.95)(T(depth), T(golden("hypos_curves.npz")["depth_range"]), T(prob), T(hyp), upsample=True)


def test_fit_modes_of_the_curves():
    from net.unit.depthhypos import fit_mode
    assert [fit_mode(c, pp) for c in ("gauss0", "gauss1", "laplace") for pp in (False, True)] == [3, 3, 1, 4, 2, 2]


# --------------------------------------------------------------------------- config.build_model
def _config():
    with contextlib.redirect_stdout(io.StringIO()):
        import config
    return config


def test_build_model_curves_and_thresholds():
    config = _config()
    with contextlib.redirect_stdout(io.StringIO()):
        default, other = config.build_model(), config.build_model(curves=("gauss0", "gauss1"))
        swapped = config.build_model(curves=("laplace", "gauss0"), prob_thresh=(1e-4, 0.9))
    slots = lambda m: [(h.ndepths, h.curve_calss, float(h.prob_thresh)) for h in m.Depth_hypos]     # noqa: E731
    assert slots(default) == [(48, None, 0.0), (24, "gauss1", float(torch.tensor(0.95))), (8, "laplace", float(torch.tensor(1e-5)))]
    assert slots(other)[1:] == [(24, "gauss0", float(torch.tensor(0.95))), (8, "gauss1", float(torch.tensor(1e-5)))]
    assert slots(swapped)[1:] == [(24, "laplace", float(torch.tensor(1e-4))), (8, "gauss0", float(torch.tensor(0.9)))]
    keys = list(default.state_dict())
    assert list(other.state_dict()) == keys and list(swapped.state_dict()) == keys
    assert not any(k.startswith("Depth_hypos") for k in keys)
    # only the default composition's (curve, threshold) pairs consult the logarithms recorded for the pinned goldens
    assert [h.default_curve for h in default.Depth_hypos] == [False, True, True]
    assert [h.default_curve for h in other.Depth_hypos] == [False, False, False]
    for bad in (dict(curves=("gauss2", "laplace")), dict(curves=("gauss1",)), dict(curves="gauss1"),
                dict(prob_thresh=(1.0, 1e-5)), dict(prob_thresh=(0.95, 1.5)), dict(curves=("laplace", "laplace"), prob_thresh=(1.0, 0.5)),
                dict(prob_thresh=(0.95,))):
        with pytest.raises(ValueError):
            config.build_model(**bad)
    assert config.parse_pair("gauss0, gauss1", str) == ("gauss0", "gauss1") and config.parse_pair("0.95,1e-5", float) == (0.95, 1e-5)
    with pytest.raises(ValueError):
        config.parse_pair("gauss1", str)


def test_slot_rehearsal_backend_laplace_on_shared_hypotheses(golden, rehearsal_backend):
    """("laplace", ...) composes the laplace curve with the uniform stage's shared hypotheses: the stock-op slot restates the
    reference's own fp32 operations, so it is held to the reference's fp32 forward (the bar tests/test_regress_gpu.py sets for the
    stage 2 laplace hypotheses: 5e-4 absolute)."""
    from net.unit.depthhypos import HyposByFit
    prob, depth, hyp = inputs(golden, 0)
    c = golden("hypos_curves.npz")
    out = HyposByFit(24, "laplace", 1e-5)(T(depth), T(c["depth_range"]), T(prob), T(hyp), upsample=True).numpy()
    assert out.shape == c["laplace_01_out"].shape
    np.testing.assert_allclose(out, c["laplace_01_out"], rtol=0, atol=5e-4)


def test_abi_argument_checks_of_the_new_modes():
    """Argument errors come back as MDF_EARG before any launch (no GPU needed); modes 1 and 7 keep their answers."""
    import ctypes
    import mdfnet_hip
    lib = mdfnet_hip.lib()
    some = ctypes.c_void_p(8)
    assert lib.mdf_hypos_fit_fwd(3, some, None, some, 1, None, some, 1, 8, 4, 6, None) == -1 and b"depth" in lib.mdf_last_error()
    for mode in (3, 4):
        assert lib.mdf_hypos_fit_fwd(mode, some, some, None, 0, None, some, 1, 8, 4, 6, None) == -1 and b"hypos" in lib.mdf_last_error()
    assert lib.mdf_hypos_fit_fwd(5, some, some, some, 1, None, some, 1, 8, 4, 6, None) == -1 and b"mode" in lib.mdf_last_error()
    assert lib.mdf_hypos_fit_fwd(7, some, None, None, 0, None, some, 1, 1, 1, 1, None) == -1 and b"mode" in lib.mdf_last_error()
    assert lib.mdf_hypos_fit_fwd(1, some, None, some, 1, some, some, 1, 8, 4, 6, None) == -2 and b"per-pixel" in lib.mdf_last_error()
    assert lib.mdf_abi_version() == 1
