"""CPU: the cascade confidence (confidence_regress with last_confidence, net/unit/regress.py:9-25) without a GPU -- the numpy mirror of
confidence_cascade_kernel against the kernels it extends and against the reference's code on .double() inputs
(tests/golden/confidence_cascade.npz, scripts/gen_confidence_golden.py); argument validation of the slot function; the model option
and the driver flag.

The float64 bars are derived, not measured.  One call in the mirror's order: inputs in [-0.25, 1.25], bicubic weights with
sum |c| = 1.28 per pass; two four-tap passes (4 products + 3 sums each, but a value passes through at most 4 + 4 of them) and the
blend (2 products + 1 sum) round about 12 times at magnitudes <= 1.3: 12 * 2^-24 * 1.3 = 9.3e-7, and the window sum adds 4 roundings
below 1 scaled by 0.2: 2e-6 per call holds with a factor of two to spare.  Along the chain the previous stage's error passes on with
0.8 * 1.28 = 1.024 per stage: 2e-6 * (1 + 1.024 + 1.024^2) = 6.1e-6, stated as 6e-6 at the end of three stages.  A wrong tap, weight or
offset moves these inputs by 1e-3 and more.  Observed (mirror): 6.6e-8 / 9.7e-8 / 1.4e-7 per call, 1.5e-7 at the end of the chain."""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import pytest
import torch

import confidence_mirror as C
import heads_mirror as M

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mdf-net_amd")
BAR_CALL, BAR_CHAIN = 2e-6, 6e-6


def _probs(golden):
    g = golden("ops.npz")
    return [g[f"reg{s}_prob"] for s in range(3)]


def _dev(a, ref):
    d = float(np.abs(np.asarray(a, np.float64) - ref).max())
    return d


# --------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("shape,seed", [((2, 8, 6, 10), 1), ((1, 5, 10, 14), 2), ((2, 24, 7, 9), 3), ((1, 1, 2, 2), 4), ((1, 3, 5, 13), 5)])
def test_mirror_default_window_is_the_confidence_kernel(shape, seed):
    """last=None, n=4, pad_front=1: the bits of heads_mirror.confidence (confidence_kernel), with up2 those of confidence_up2."""
    prob = M.make_probs(*shape, seed)[0]
    assert M.same_bits(C.cascade(prob), M.confidence(prob)[0]).all()
    assert M.same_bits(C.cascade(prob, up2=True), M.confidence_up2(prob)).all()


def test_mirror_default_window_on_the_goldens(golden):
    for p in _probs(golden):
        assert M.same_bits(C.cascade(p), M.confidence(p)[0]).all()


def test_bicubic_weights_are_torchs_coefficients():
    """The weight quadruple is ATen's cubic convolution (A = -0.75) at t = 0.75, exactly; the taps are those of src = o/2 - 0.25."""
    A = -0.75
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1           # noqa: E731  |x| <= 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A     # noqa: E731  1 < |x| < 2
    t = 0.75
    assert [float(v) for v in C.W] == [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]
    idx, c = C.bicubic2_taps(6, 3)
    assert idx.tolist() == [[0, 0, 0, 1], [0, 0, 1, 2], [0, 0, 1, 2], [0, 1, 2, 2], [0, 1, 2, 2], [1, 2, 2, 2]]
    assert (c[0::2] == C.W).all() and (c[1::2] == C.W[::-1]).all()
    for o in range(6):                                           # floor(src) - 1 .. floor(src) + 2, fraction 0.75 / 0.25
        src = 0.5 * (o + 0.5) - 0.5
        f = int(np.floor(src))
        assert idx[o].tolist() == [min(max(f - 1 + j, 0), 2) for j in range(4)] and src - f == (0.25 if o & 1 else 0.75)
    one = np.full((1, 1, 1), 0.625, np.float32)                  # one pixel: every tap clamps onto it; the weights sum to 1
    assert np.abs(C.bicubic_up2(one) - 0.625).max() <= 4 * M.EPS


def test_mirror_against_the_reference_in_float64(golden):
    g, probs = golden("confidence_cascade.npz"), _probs(golden)
    assert [g[f"chain64_c{s}"].shape for s in range(3)] == [(2, 8, 12), (2, 16, 24), (2, 32, 48)] and g["chain64_c2"].dtype == np.float64
    for s, p in enumerate(probs):                                # every call on its own: given the previous stage of the yardstick
        last = None if s == 0 else g[f"chain64_c{s - 1}"].astype(np.float32)
        d = _dev(C.cascade(p, last), g[f"chain64_c{s}"])
        d2 = _dev(C.cascade(p, None, n=2, pad_front=0), g[f"n2_64_c{s}"])
        print(f"stage {s}: per call max |mirror - float64| = {d:.3e}; n=2 window {d2:.3e}")
        assert d <= BAR_CALL and d2 <= BAR_CALL
    chain = C.chain(probs)
    devs = [_dev(c, g[f"chain64_c{s}"]) for s, c in enumerate(chain)]
    print("chain: max |mirror - float64| per stage =", ["%.3e" % d for d in devs])
    assert devs[0] <= BAR_CALL and devs[2] <= BAR_CHAIN and devs[1] <= BAR_CHAIN
    d = _dev(C.cascade(g["up_prob"], g["up_last"]), g["up_64"])
    print(f"[2,5,7] -> [2,10,14] with a uniform last: {d:.3e}")
    assert g["up_64"].shape == (2, 10, 14) and d <= BAR_CALL
    # the reference's own fp32 sits as close to float64 (it is not the mirror's order: no bit equality is asked for)
    assert _dev(g["chain32_c2"], g["chain64_c2"]) <= BAR_CHAIN
    # the mirror with up2 is the nearest x2 of the same values
    assert M.same_bits(C.chain(probs, up2_last=True)[2], M.up2_nearest(chain[2])).all()


def test_a_wrong_tap_or_weight_shows_far_above_the_bar(golden, monkeypatch):
    """What the bars can see: the taps shifted by one, or the weights read backwards, move the golden call by more than 1e-3."""
    g = golden("confidence_cascade.npz")
    real = C.bicubic2_taps
    monkeypatch.setattr(C, "bicubic2_taps", lambda n_out, n_in: (np.clip(real(n_out, n_in)[0] + 1, 0, n_in - 1), real(n_out, n_in)[1]))
    assert _dev(C.cascade(g["up_prob"], g["up_last"]), g["up_64"]) > 1e-3
    monkeypatch.setattr(C, "bicubic2_taps", lambda n_out, n_in: (real(n_out, n_in)[0], real(n_out, n_in)[1][:, ::-1]))
    assert _dev(C.cascade(g["up_prob"], g["up_last"]), g["up_64"]) > 1e-3


# --------------------------------------------------------------------------- the slot function
def test_confidence_regress_validates_on_cpu_tensors():
    from net.unit import regress
    prob = torch.softmax(torch.randn(2, 8, 6, 10), 1)
    for fn in (regress.confidence_regress, regress.confidence_cascade):
        with pytest.raises(ValueError, match="n=3"):
            fn(prob, n=3)
        with pytest.raises(ValueError, match=r"\(0, 0, 0, 0, 1, 1\)"):
            fn(prob, n=4, pad=(0, 0, 0, 0, 1, 1))                       # front + back < n - 1
        with pytest.raises(ValueError, match=r"\(0, 0, 0, 0, 0, 0\)"):
            fn(prob, n=2, pad=(0, 0, 0, 0, 0, 0))
        with pytest.raises(ValueError, match="pad"):
            fn(prob, pad=(0, 1, 0, 0, 1, 2))                            # padding off the depth axis
        with pytest.raises(ValueError, match=r"\(2, 6, 10\)"):
            fn(prob, last_confidence=torch.zeros(2, 6, 10))             # the shape of this stage, not of the previous one
        with pytest.raises(ValueError, match=r"\(1, 3, 5\)"):
            fn(prob, last_confidence=torch.zeros(1, 3, 5))
        with pytest.raises(ValueError, match="even"):
            fn(torch.softmax(torch.randn(1, 8, 5, 10), 1), last_confidence=torch.zeros(1, 2, 5))
        # a valid call gets as far as the device check: there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(prob, last_confidence=torch.zeros(2, 3, 5))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(prob, n=2, pad=(0, 0, 0, 0, 0, 1))
    assert regress.confidence_regress.mdf_builtin and not getattr(regress.confidence_regress, "mdf_cascade", False)
    assert regress.confidence_cascade.mdf_builtin and regress.confidence_cascade.mdf_cascade


def test_ops_confidence_cascade_refuses_cpu_tensors():
    from mdfnet_hip import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.confidence_cascade(torch.rand(1, 4, 4, 4), torch.rand(1, 2, 2))


def test_abi_rejections_need_no_gpu():
    """MDF_REQUIRE answers before any launch: null pointers, shapes, the window, an odd map under a last confidence."""
    import ctypes
    import mdfnet_hip
    lib = mdfnet_hip.lib()
    some, f = ctypes.c_void_p(8), ctypes.c_float
    call = lambda prob, last, n, pf, conf, B, D, H, W: lib.mdf_confidence_cascade_fwd(prob, last, f(0.8), f(0.2), n, pf, 0, conf, B, D, H, W, None)   # noqa: E731
    assert call(None, None, 4, 1, some, 1, 8, 4, 6) == -1 and b"null" in lib.mdf_last_error()
    assert call(some, None, 4, 1, None, 1, 8, 4, 6) == -1 and b"null" in lib.mdf_last_error()
    assert call(some, None, 4, 1, some, 1, 0, 4, 6) == -1 and b"shape" in lib.mdf_last_error()
    for n in (0, 3, 5, 16, -4):
        assert call(some, None, n, 1, some, 1, 8, 4, 6) == -1 and b"n must be 1, 2, 4 or 8" in lib.mdf_last_error()
    assert call(some, None, 4, -1, some, 1, 8, 4, 6) == -1 and b"pad_front" in lib.mdf_last_error()
    assert call(some, some, 4, 1, some, 1, 8, 5, 6) == -1 and b"even" in lib.mdf_last_error()
    assert call(some, some, 4, 1, some, 1, 8, 4, 7) == -1 and b"even" in lib.mdf_last_error()


# --------------------------------------------------------------------------- model option and driver flag
def _config():
    with contextlib.redirect_stdout(io.StringIO()):
        import config
    return config


def test_build_model_confidence_option():
    config = _config()
    from net.unit import regress
    assert config.CONFIDENCES == ("last", "cascade")
    with contextlib.redirect_stdout(io.StringIO()):
        default, last, cascade = config.build_model(), config.build_model(confidence="last"), config.build_model(confidence="cascade")
    assert default.Confidence_regress is regress.confidence_regress and last.Confidence_regress is regress.confidence_regress
    assert cascade.Confidence_regress is regress.confidence_cascade and cascade.Depth_regress is regress.depth_regression
    assert config.model.Confidence_regress is regress.confidence_regress          # the singleton stays the default composition
    sd, sc = default.state_dict(), cascade.state_dict()
    assert list(sd) == list(sc) and all(sd[k].shape == sc[k].shape and sd[k].dtype == sc[k].dtype for k in sd)
    for bad in ("x", "", None, "Cascade"):
        with pytest.raises(ValueError, match="confidence="):
            config.build_model(confidence=bad)


def test_eval_driver_lists_the_flag(monkeypatch, capsys):
    _config()
    spec = importlib.util.spec_from_file_location("mdf_eval_confidence_flag", os.path.join(PKG, "eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["eval.py", "--help"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    text = capsys.readouterr().out
    assert e.value.code == 0 and "--confidence {last,cascade}" in text
    monkeypatch.setattr(sys, "argv", ["eval.py", "--confidence", "both"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 2 and "--confidence" in capsys.readouterr().err
