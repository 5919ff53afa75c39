"""CPU: the "atv" hypothesis curve (the reference's atv_hypos, depthhypos.py:218-253) -- mirror, goldens, slot, composition, ABI.

tests/golden/atv_hypos.npz (scripts/gen_atv_golden.py) holds what the reference's atv_hypos gives on the two inter-stage transitions
of tests/golden/ops.npz for UCS-Net's scale 1.5 and for a scale wide enough that both branches of its min run, in fp32 and on
.double() inputs.  tests/atv_mirror.py has the explicit-order fp32 mirror of the hypotheses kernel, the float64 spread and the two
bars with their derivations."""
import contextlib
import ctypes
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

import atv_mirror as A  # noqa: E402
import heads_mirror as M  # noqa: E402

T = torch.from_numpy
# case -> transition: the stage whose outputs feed the slot
CASES = {"atv_01": 0, "atv_12": 1, "atv_01_wide": 0, "atv_12_wide": 1}


def inputs(golden, st):
    g = golden("ops.npz")
    return g[f"reg{st}_prob"], g[f"reg{st}_depth"], g[f"agg{st}_hyp"]


def case_bar(c, case, D):
    return A.slot_bar(D, c[case + "_e64"].max(), np.abs(c[case + "_out64"]).max())


@pytest.mark.parametrize("case", list(CASES))
def test_mirror_is_the_references_fp32(golden, case):
    """The explicit-order mirror on the golden's fp32 spread: the reference's fp32 atv_hypos bit for bit."""
    c = golden("atv_hypos.npz")
    _, depth, _ = inputs(golden, CASES[case])
    out = A.atv_hypos(c[case + "_e32"], depth, int(c[case + "_ndepths"]), True)
    assert out.shape == c[case + "_out32"].shape and M.same_bits(out, c[case + "_out32"]).all()


def test_golden_covers_both_branches_of_min(golden):
    """Scale 1.5: e < depth everywhere, and the hypotheses leave the depth range (no clamp); the wide scales: e2 > d2 at some 40 %
    and 53 % of the output pixels.  Every hypothesis is >= 1e-12."""
    c = golden("atv_hypos.npz")
    lo, hi = float(c["depth_range"][:, 0].min()), float(c["depth_range"][:, 1].max())
    for case, st in CASES.items():
        _, depth, _ = inputs(golden, st)
        share = float((M.up2_bilinear(c[case + "_e32"]) > M.up2_bilinear(depth)).mean())
        assert (share == 0) if not case.endswith("wide") else (0.3 < share < 0.7), (case, share)
        assert (c[case + "_out32"] >= np.float32(1e-12)).all()
    assert c["atv_01_out32"].min() < lo and c["atv_01_out32"].max() > hi


@pytest.mark.parametrize("case", list(CASES))
def test_golden_spread_and_fp32_against_float64(golden, case):
    """torch's fp32 spread inside the spread bar of the float64 formula (it uses 0.07 / 0.14 of it), the float64 formula restated in
    tests/atv_mirror.py equal to the golden's, and the reference's fp32 hypotheses inside the slot bar of its float64 ones."""
    c = golden("atv_hypos.npz")
    prob, depth, hyp = inputs(golden, CASES[case])
    scale = float(c[case + "_scale"])
    e64, _ = A.spread64(prob, depth, hyp, scale)
    np.testing.assert_allclose(e64, c[case + "_e64"], rtol=1e-14, atol=0)
    A.check_spread(c[case + "_e32"], prob, depth, hyp, scale, case + " torch fp32")
    err = float(np.abs(c[case + "_out32"] - c[case + "_out64"]).max())
    bar = case_bar(c, case, prob.shape[1])
    print(f"{case}: fp32 hypotheses against float64: max |d| = {err:.3e} (slot bar {bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("case", list(CASES))
def test_slot_rehearsal_backend(golden, rehearsal_backend, case):
    """HyposByFit(D_out, "atv", atv_scale=scale) through the stock-op backend against the reference's fp32 forward: the slot bar."""
    from net.unit.depthhypos import HyposByFit
    c = golden("atv_hypos.npz")
    prob, depth, hyp = inputs(golden, CASES[case])
    slot = HyposByFit(int(c[case + "_ndepths"]), "atv", 0.95, atv_scale=float(c[case + "_scale"]))
    out = slot(T(depth), T(c["depth_range"]), T(prob), T(hyp), upsample=True).numpy()
    assert out.dtype == np.float32 and out.shape == c[case + "_out32"].shape
    err = float(np.abs(out - c[case + "_out32"]).max())
    bar = case_bar(c, case, prob.shape[1])
    print(f"{case}: rehearsal-backend slot against the reference's fp32: max |d| = {err:.3e} (slot bar {bar:.3e})")
    assert err <= bar
    # upsample=False: the two maps as they are
    flat = slot(T(depth), T(c["depth_range"]), T(prob), T(hyp), upsample=False).numpy()
    from rehearsal import stockops
    e = stockops.atv_spread(float(c[case + "_scale"]), T(depth), T(prob), T(hyp)).numpy()
    want = A.atv_hypos(e, depth, int(c[case + "_ndepths"]), False)
    assert flat.shape == want.shape and float(np.abs(flat - want).max()) <= bar


def test_slot_ignores_prob_thresh_and_keeps_the_uniform_stage(golden, rehearsal_backend):
    from net.unit.depthhypos import HyposByFit
    c = golden("atv_hypos.npz")
    prob, depth, hyp = inputs(golden, 0)
    dr = T(c["depth_range"])
    a, b = (HyposByFit(24, "atv", t)(T(depth), dr, T(prob), T(hyp), upsample=True) for t in (0.95, 1e-5))
    assert torch.equal(a, b)
    assert HyposByFit(24, "atv").atv_scale == 1.5 and HyposByFit(24, "gauss1").atv_scale == 1.5
    u_atv, u_def = HyposByFit(48, "atv")(None, dr, None, None), HyposByFit(48, "gauss1")(None, dr, None, None)
    assert u_atv.shape == (2, 48, 1, 1) and torch.equal(u_atv, u_def)


def test_fit_modes_and_unknown_curves(golden, rehearsal_backend):
    from net.unit.depthhypos import CURVES, HyposByFit, fit_mode
    assert [fit_mode(c, pp) for c in ("gauss0", "gauss1", "laplace") for pp in (False, True)] == [3, 3, 1, 4, 2, 2]
    assert "atv" in CURVES and fit_mode("atv", False) is None and fit_mode("atv", True) is None
    with pytest.raises(NotImplementedError, match="atv"):
        fit_mode("gauss7", True)
    prob, depth, hyp = inputs(golden, 1)
    with pytest.raises(NotImplementedError, match="gauss7"):
        HyposByFit(8, "gauss7", 0.95)(T(depth), T(golden("atv_hypos.npz")["depth_range"]), T(prob), T(hyp), upsample=True)


# --------------------------------------------------------------------------- config.build_model
def _config():
    with contextlib.redirect_stdout(io.StringIO()):
        import config
    return config


def test_build_model_with_atv():
    config = _config()
    with contextlib.redirect_stdout(io.StringIO()):
        default = config.build_model()
        models = {cv: config.build_model(curves=cv) for cv in (("atv", "atv"), ("gauss1", "atv"), ("atv", "laplace"))}
        scaled = config.build_model(curves=("atv", "atv"), atv_scale=(2.0, 0.75))
    assert "atv" in config.CURVES
    keys = list(default.state_dict())
    for cv, m in models.items():
        assert list(m.state_dict()) == keys
        assert [h.curve_calss for h in m.Depth_hypos] == [None] + list(cv)
        assert [h.atv_scale for h in m.Depth_hypos] == [1.5, 1.5, 1.5]
        assert type(m.Depth_hypos[1]) is type(default.Depth_hypos[1])
    assert [h.atv_scale for h in scaled.Depth_hypos][1:] == [2.0, 0.75]
    assert [h.atv_scale for h in default.Depth_hypos] == [1.5, 1.5, 1.5]
    from mdfnet_hip import controlplane
    assert controlplane.builtin_slots(models[("atv", "atv")])
    for bad in ((0, 1.5), (1.5, -1), (float("inf"), 1.5), (1.5, float("nan")), 1.5, (1.5,), (1.5, 1.5, 1.5)):
        with pytest.raises(ValueError):
            config.build_model(curves=("atv", "atv"), atv_scale=bad)
    # the thresholds are still checked for every slot, an atv one included
    with pytest.raises(ValueError):
        config.build_model(curves=("atv", "atv"), prob_thresh=(1.0, 0.5))
    # the default composition is the singleton's: same curves and thresholds
    assert [(h.curve_calss, float(h.prob_thresh)) for h in default.Depth_hypos] == \
        [(h.curve_calss, float(h.prob_thresh)) for h in config.model.Depth_hypos]


def test_drivers_accept_atv():
    import train
    import validate
    a = train.build_parser().parse_args(["--curves", "atv,atv", "--atv_scale", "2,0.5"])
    assert a.curves == "atv,atv" and _config().parse_pair(a.atv_scale, float) == (2.0, 0.5)
    assert train.build_parser().parse_args([]).atv_scale == "1.5,1.5"
    v = validate.build_parser().parse_args(["--curves", "gauss1,atv"])
    assert v.curves == "gauss1,atv" and v.atv_scale == "1.5,1.5"


# --------------------------------------------------------------------------- ABI
def test_abi_argument_checks():
    """Argument errors come back as MDF_EARG before any launch (no GPU needed); the fit entries keep rejecting the next free modes."""
    import mdfnet_hip
    lib = mdfnet_hip.lib()
    some = ctypes.c_void_p(8)
    f = ctypes.c_float
    ok = (some, some, some, 0, f(1.5), some, 1, 8, 4, 6, None)
    for k in (0, 1, 2, 5):
        args = list(ok)
        args[k] = None
        assert lib.mdf_atv_spread_fwd(*args) == -1 and b"null" in lib.mdf_last_error(), k
    for k in (6, 7, 8, 9):
        for v in (0, -3):
            args = list(ok)
            args[k] = v
            assert lib.mdf_atv_spread_fwd(*args) == -1 and b"shape" in lib.mdf_last_error(), (k, v)
    for s in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        args = list(ok)
        args[4] = f(s)
        assert lib.mdf_atv_spread_fwd(*args) == -1 and b"scale" in lib.mdf_last_error(), s
    ok = (some, some, some, 1, 8, 4, 6, 1, None)
    for k in (0, 1, 2):
        args = list(ok)
        args[k] = None
        assert lib.mdf_atv_hypos_fwd(*args) == -1 and b"null" in lib.mdf_last_error(), k
    for k in (3, 5, 6):
        args = list(ok)
        args[k] = 0
        assert lib.mdf_atv_hypos_fwd(*args) == -1 and b"shape" in lib.mdf_last_error(), k
    for d_out in (1, 0, -2):
        args = list(ok)
        args[4] = d_out
        assert lib.mdf_atv_hypos_fwd(*args) == -1 and b"D_out" in lib.mdf_last_error(), d_out
    assert lib.mdf_hypos_fit_fwd(5, some, some, some, 1, None, some, 1, 8, 4, 6, None) == -1 and b"mode" in lib.mdf_last_error()
    assert lib.mdf_hypos_from_fit_fwd(3, some, some, some, f(-0.05), some, 1, 8, 4, 6, 1, None) == -1 and b"mode" in lib.mdf_last_error()
    assert lib.mdf_abi_version() == 1


def test_kernels_are_in_the_heads_family():
    from mdfnet_hip import kernel_families as K
    assert K.KERNEL_FAMILY["atv_spread_kernel"] == K.HEADS and K.KERNEL_FAMILY["atv_hypos_kernel"] == K.HEADS
    assert K.family("void (anonymous namespace)::atv_spread_kernel<48>(float const*, float const*, float const*, int, float, float*, int, int, int)") == K.HEADS
