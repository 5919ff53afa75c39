"""GPU: hypos_fit modes 3 (gauss0) and 4 (gauss1 with hypotheses of either form) against the reference's code in float64.

The bar is   | 1/s_gpu - |b0_64| |  <=  K(D) * 2^-24 * N   with K and N as tests/hypos_oracle.py derives them from the kernels'
operation order (K3 = 2 S(D) + 16, K4 = 2 S(D) + 14, S(D) = min(D, ceil(D/4) + 2): never more than 2 D + 16), b0_64 the centred
float64 fit of the same fp32 inputs (itself tied to the reference's float64 golden in tests/test_hypos_curves_cpu.py), or that
golden directly.  A pixel whose fit is not determined (fewer than 2 distinct (x - depth)^2, fewer than 3 distinct hypotheses) must
be NaN, every other pixel finite or infinite and within the bound.  Each case prints its largest error as a share of the bound.

Shapes: one pixel; below one wave with a batch stride; a wave boundary with a tail; the switch to 256-thread blocks (262 144
pixels); the 8192-block grid cap, where the grid-stride loop takes a second trip.  D: the register forms 48 / 24 / 8, the generic 17,
and the least determined fits (2 for gauss0, 3 for gauss1).  Hypotheses shared and per pixel, strictly increasing."""
import ctypes
import functools
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
import mdfnet_hip  # noqa: E402
from mdfnet_hip import ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"

SMALL = [(1, 1, 1), (2, 5, 7), (1, 9, 31)]
SWITCH = (1, 512, 512)                 # 262 144 pixels: the first size with 256-thread blocks
BIG = (1, 1184, 2000)                  # 2 368 000 pixels > 8192 blocks * 256 threads
CASES = [(m, s, d) for m in (3, 4) for s in SMALL for d in (48, 24, 8, 17, 2 if m == 3 else 3)] + \
        [(m, s, 8) for m in (3, 4) for s in (SWITCH, BIG)]


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(a):
    return T(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def increasing(hyp):
    """make_hypos sorts its draws; two of them can round to one fp32.  Push every tie up by one ulp (before the squaring or the
    centring nothing cares whether a hypothesis leaves the range by an ulp)."""
    hyp = hyp.copy()
    for d in range(1, hyp.shape[1]):
        hyp[:, d] = np.maximum(hyp[:, d], np.nextafter(hyp[:, d - 1], np.float32(np.inf)))
    return hyp


@functools.lru_cache(maxsize=2)
def inputs(shape, D):
    """-> prob, {per_pixel: (hyp, depth)}; shared by the two modes of a (shape, D), never written to."""
    B, h, w = shape
    seed = (B * 1000003 + h * 10007 + w * 101 + D) % (2 ** 31 - 1)
    prob, _, _ = M.make_probs(B, D, h, w, seed)
    hyps = {}
    for per_pixel in (False, True):
        hyp = increasing(M.make_hypos(B, D, h, w, per_pixel, seed))
        hyps[per_pixel] = (hyp, M.depth_regress(prob, hyp))
    return prob, hyps


def check(s, b0, n, deg, mode, D, what):
    """NaN exactly at the undetermined pixels, the bound everywhere else -> the largest error / bound."""
    assert s.dtype == np.float32 and s.shape == b0.shape
    assert np.array_equal(np.isnan(s), deg), f"{what}: NaN at {int(np.isnan(s).sum())} pixels, undetermined are {int(deg.sum())}"
    ok = ~deg
    if not ok.any():
        return 0.0
    assert (s[ok] >= 0).all()
    r = H.ratio(s[ok], b0[ok], n[ok], mode, D)
    worst = float(r.max())
    print(f"{what}: max |1/s - |b0_64|| / (K 2^-24 N) = {worst:.4f}  (K = {H.K(mode, D)}, {int(ok.sum())} pixels)")
    assert (r <= 1).all(), f"{what}: {int((r > 1).sum())} pixels over the bound, worst {worst:.3f}"
    return worst


def run(mode, prob_g, depth, hyp):
    return host(ops.hypos_fit(mode, prob_g, None if mode == 4 else dev(depth), dev(hyp)))


# --------------------------------------------------------------------------- 1, 2: the bound at edge shapes and depths
@pytest.mark.parametrize("mode,shape,D", CASES, ids=[f"mode{m}-{_id(s)}-D{d}" for m, s, d in CASES])
def test_bound_at_edge_shapes(mode, shape, D):
    prob, hyps = inputs(shape, D)
    pg = dev(prob)
    for per_pixel in (False, True):
        hyp, depth = hyps[per_pixel]
        s = run(mode, pg, depth, hyp)
        b0, n, deg = H.gauss0_fit64(prob, depth, hyp) if mode == 3 else H.gauss1_fit64(prob, hyp)
        # strictly increasing hypotheses: every pixel is compared, but for gauss0 at D = 2 where equal probabilities put the depth
        # half way between the two hypotheses and leave one value of u
        assert not (deg & ~((mode == 3 and D == 2) & (prob[:, 0] == prob[:, -1]))).any()
        check(s, b0, n, deg, mode, D, f"mode {mode} {shape} D={D} per_pixel={int(per_pixel)}")
    if shape == BIG:
        assert prob.shape[0] * prob.shape[2] * prob.shape[3] > 8192 * 256


# --------------------------------------------------------------------------- 3: the golden transitions
@pytest.mark.parametrize("case,mode,st", [("gauss0_01", 3, 0), ("gauss0_12", 3, 1), ("gauss1_12", 4, 1)])
def test_golden_transitions_against_the_references_float64(golden, case, mode, st):
    """The inter-stage tensors of tests/golden/ops.npz (stage 1 -> 2: per-pixel hypotheses around the regressed depth) against what
    the reference's own code gives on .double() inputs."""
    g, c = golden("ops.npz"), golden("hypos_curves.npz")
    prob, depth, hyp = g[f"reg{st}_prob"], g[f"reg{st}_depth"], g[f"agg{st}_hyp"]
    s = run(mode, dev(prob), depth, hyp)
    _, n, deg = H.gauss0_fit64(prob, depth, hyp) if mode == 3 else H.gauss1_fit64(prob, hyp)
    check(s, 1.0 / c[case + "_s64"], n, deg, mode, prob.shape[1], case)


def test_laplace_on_shared_hypotheses_golden(golden):
    """mode 2 on the stage 0 -> 1 transition (hypotheses shared by all pixels), the pairing ("laplace", ...) composes: the relative
    bound of test_heads_gpu.py::test_hypos_fit_laplace, (2 D + 8) * 2^-24, against the reference's float64."""
    g, c = golden("ops.npz"), golden("hypos_curves.npz")
    s = host(ops.hypos_fit(2, dev(g["reg0_prob"]), dev(g["reg0_depth"]), dev(g["agg0_hyp"])))
    rel = np.abs(s - c["laplace_01_s64"]) / c["laplace_01_s64"]
    print(f"laplace_01: max rel err / bound = {float(rel.max()) / ((2 * 48 + 8) * H.EPS):.3f}")
    assert (rel <= (2 * 48 + 8) * H.EPS).all()


# --------------------------------------------------------------------------- 4: values
def test_zero_denormal_onehot_and_flat_probabilities():
    """ln max(p, 1e-40f): a zero or a 1e-42 gives ln(float32(1e-40)) = -92.1034, a 1e-39 (a denormal above the clamp) and a 1e-38
    their own logarithms; with denormals flushed the clamp would be 0 and s 0 or NaN.  A one-hot pixel is D - 1 clamped planes.  An
    exactly flat volume has b0 = 0 up to rounding: s is huge or infinite, and 1/s is still within the bound of 0."""
    D = 5
    prob = np.zeros((1, D, 1, 6), np.float32)
    prob[0, 0, 0, :4] = 1.0
    prob[0, 2, 0, :4] = [0.0, 1e-42, 1e-39, 1e-38]
    prob[0, 1, 0, 4] = 1.0                                     # one-hot
    prob[0, :, 0, 5] = 0.2                                     # flat
    z = M.log_clamped64(prob)
    assert abs(z[0, 2, 0, 0] + 92.1034) < 1e-3 and z[0, 2, 0, 0] == z[0, 2, 0, 1] < z[0, 2, 0, 2] < z[0, 2, 0, 3]
    pg = dev(prob)
    for per_pixel in (False, True):
        hyp = increasing(M.make_hypos(1, D, 1, 6, per_pixel, 3))
        depth = M.depth_regress(prob, hyp)
        for mode in (3, 4):
            s = run(mode, pg, depth, hyp)
            b0, n, deg = H.gauss0_fit64(prob, depth, hyp) if mode == 3 else H.gauss1_fit64(prob, hyp)
            assert not deg.any()
            print(f"mode {mode} per_pixel={int(per_pixel)}: s for p = 0, 1e-42, 1e-39, 1e-38, one-hot, flat:", s[0, 0])
            check(s, b0, n, deg, mode, D, f"values mode {mode} per_pixel={int(per_pixel)}")
            if not per_pixel:
                assert s[0, 0, 0] == s[0, 0, 1] != s[0, 0, 2]      # both clamped; the denormal above the clamp is read as itself
            assert np.isfinite(s[0, 0, :5]).all() and s[0, 0, 5] > 1e3 * s[0, 0, :5].max()


# --------------------------------------------------------------------------- 5: undetermined fits
def test_undetermined_pixels_are_nan():
    """D = 1; every hypothesis of a pixel equal; for gauss1 exactly two distinct values: s is NaN there (the reference raises from
    torch.inverse) and finite at the other pixels of the same launch (but where the probabilities are exactly flat: b0 = 0 there and
    s may be infinite)."""
    prob1, _, _ = M.make_probs(2, 1, 3, 5, 1)
    hyp1 = M.make_hypos(2, 1, 3, 5, True, 1)
    for mode in (3, 4):
        assert np.isnan(run(mode, dev(prob1), M.depth_regress(prob1, hyp1), hyp1)).all()
        assert np.isnan(run(mode, dev(prob1), M.depth_regress(prob1, hyp1[:, :, :1, :1]), hyp1[:, :, :1, :1])).all()
    for D in (3, 8, 17, 24):
        B, h, w = 2, 5, 7
        prob, _, _ = M.make_probs(B, D, h, w, D)
        hyp = increasing(M.make_hypos(B, D, h, w, True, D))
        hyp[0, :, 1, 2] = hyp[0, 0, 1, 2]                      # all equal
        hyp[1, :, 4, 6] = np.float32(0.1) * 7919               # all equal, a value whose multiples round
        hyp[1, : D // 2, 0, 0] = hyp[1, 0, 0, 0]               # two distinct values
        hyp[1, D // 2:, 0, 0] = hyp[1, -1, 0, 0]
        hyp[0, 1:, 3, 3] = hyp[0, 1, 3, 3]                     # two distinct values, one of them once
        depth = M.depth_regress(prob, hyp)
        equal = np.zeros((B, h, w), bool)
        equal[0, 1, 2] = equal[1, 4, 6] = True
        two = np.zeros((B, h, w), bool)
        two[1, 0, 0] = two[0, 3, 3] = True
        flat = (prob == prob[:, :1]).all(1)
        s3, s4 = run(3, dev(prob), depth, hyp), run(4, dev(prob), depth, hyp)
        d3, d4 = H.gauss0_fit64(prob, depth, hyp)[2], H.gauss1_fit64(prob, hyp)[2]
        assert np.array_equal(d3, equal) and np.array_equal(d4, equal | two)
        assert np.array_equal(np.isnan(s3), equal) and np.isfinite(s3[~equal & ~flat]).all(), (D, np.argwhere(np.isnan(s3) != equal))
        assert np.array_equal(np.isnan(s4), equal | two) and np.isfinite(s4[~(equal | two | flat)]).all(), (D, np.argwhere(np.isnan(s4) != (equal | two)))
    # hypotheses shared by all pixels, all equal: every pixel
    hyp = np.full((2, 8, 1, 1), 500.0, np.float32)
    prob, _, _ = M.make_probs(2, 8, 5, 7, 8)
    for mode in (3, 4):
        assert np.isnan(run(mode, dev(prob), M.depth_regress(prob, hyp), hyp)).all()


# --------------------------------------------------------------------------- 6, 7: error paths
def test_error_paths():
    prob, _, _ = M.make_probs(1, 8, 4, 6, 1)
    hyp = M.make_hypos(1, 8, 4, 6, True, 1)
    depth = M.depth_regress(prob, hyp)
    with pytest.raises(mdfnet_hip.MdfHipError) as e:
        ops.hypos_fit(3, dev(prob), None, dev(hyp))
    assert "code -1" in str(e.value) and "depth" in str(e.value)          # MDF_EARG
    with pytest.raises(mdfnet_hip.MdfHipError) as e:
        ops.hypos_fit(5, dev(prob), dev(depth), dev(hyp))
    assert "code -1" in str(e.value) and "mode" in str(e.value)
    lib = mdfnet_hip.lib()
    some = ctypes.c_void_p(8)                                               # argument checks come before any launch
    for mode in (3, 4):
        assert lib.mdf_hypos_fit_fwd(mode, some, some, None, 0, None, some, 1, 8, 4, 6, None) == -1 and b"hypos" in lib.mdf_last_error()
    # modes 1, 2 and 7 keep their answers
    with pytest.raises(mdfnet_hip.MdfHipError) as e:
        ops.hypos_fit(1, dev(prob), None, dev(hyp), dev(np.zeros((1, 8), np.float32)))
    assert "code -2" in str(e.value) and "per-pixel" in str(e.value)
    assert lib.mdf_hypos_fit_fwd(7, some, None, None, 0, None, some, 1, 1, 1, 1, None) == -1 and b"mode" in lib.mdf_last_error()
    # mode 4 takes no fit row; mode 3 runs (on the parent commit both are error -1)
    assert np.isfinite(host(ops.hypos_fit(4, dev(prob), None, dev(hyp), None))).all()
    assert np.isfinite(host(ops.hypos_fit(3, dev(prob), dev(depth), dev(hyp)))).all()
    assert mdfnet_hip.lib().mdf_last_launch().decode() == "hypos_curve_fit_kernel"


# --------------------------------------------------------------------------- 8: the model
def _build(curves):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        m = config.build_model(curves=curves)
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=1))
    return m


@pytest.mark.parametrize("curves", [("gauss0", "gauss1"), ("laplace", "gauss0")], ids="-".join)
def test_model_with_other_curves(monkeypatch, curves):
    """Eval forward at 160x128, 3 views: finite outputs, every stage's regressed depth inside the depth range, and every s the model's
    own fits of modes 3 and 4 produce held to the bound on the tensors the model handed them (step 2 given s is bit-exact:
    tests/test_heads_gpu.py).  The refinement net's output is held to finite only: nothing in it clamps to the range, and with the
    seeded weights it leaves the range by hundreds of millimetres for the default composition as well (the CPU oracle's
    core_forward on this scene gives the same)."""
    model = _build(curves).eval().to(DEV)
    scene = synth.make_scene(160, 128, 3, batch=1, rot_deg=2.0, seed=3)
    calls = []
    real = ops.hypos_fit

    def spy(mode, prob, depth, hyp, row=None):
        s = real(mode, prob, depth, hyp, row)
        calls.append((mode, host(prob), host(depth), host(hyp), host(s)))
        return s
    monkeypatch.setattr(ops, "hypos_fit", spy)
    last = []
    model.Refine.register_forward_pre_hook(lambda mod, args: last.append(host(args[0])))
    with torch.no_grad():
        out = model(*[t.to(DEV) for t in scene])
    from net.unit.depthhypos import fit_mode
    assert [c[0] for c in calls] == [fit_mode(curves[0], False), fit_mode(curves[1], True)]
    lo, hi = float(scene[3][0, 0]), float(scene[3][0, 1])
    # a regressed depth is a convex combination of hypotheses clamped to [lo, hi], up to D roundings of a value below hi
    assert len(last) == 1 and last[0].shape == (1, 64, 80)
    for depth in [c[2] for c in calls] + last:
        assert np.isfinite(depth).all() and (depth >= lo - 48 * H.EPS * hi).all() and (depth <= hi + 48 * H.EPS * hi).all()
    for mode, prob, depth, hyp, s in calls:
        D = prob.shape[1]
        if mode in (3, 4):
            b0, n, deg = H.gauss0_fit64(prob, depth, hyp) if mode == 3 else H.gauss1_fit64(prob, hyp)
            print(f"{curves}: mode {mode} D={D} {prob.shape[2:]}: {int(deg.sum())} undetermined pixels")
            check(s, b0, n, deg, mode, D, f"model {curves} mode {mode}")
    depth, conf = host(out["depth"]), host(out["confidence"])
    print(f"{curves}: depth in [{depth.min():.3f}, {depth.max():.3f}] of [{lo}, {hi}], confidence in [{conf.min():.3f}, {conf.max():.3f}]")
    assert depth.shape == (1, 128, 160) and np.isfinite(depth).all() and np.isfinite(conf).all()
    assert (conf >= 0).all() and (conf <= 1 + 4 * H.EPS).all()


# --------------------------------------------------------------------------- 9: training
def test_training_step_eager_and_recorded():
    """One eager training step of the ("gauss0", "gauss1") model at the tiny training shape: loss and every gradient finite; and the
    step recorded as a hipGraph held to the comparison tests/test_train_graph_gpu.py makes for the default model (learning rate 0:
    loss within 2e-5 relative, gradients within 1e-3 in L2, on inputs the recording has not seen).  The new fits take nothing
    from the host and the control plane carries no fit row for this composition."""
    import test_train_graph_gpu as TG
    from mdfnet_hip import controlplane, ddp
    from mdfnet_hip.graphstep import GraphedTrainStep
    from mdfnet_hip.optim import FlatAdam
    from net.loss import Loss
    crit = Loss().to(DEV)
    me, mg = (_build(("gauss0", "gauss1")).train().to(DEV) for _ in range(2))
    be, bg = ddp.FlatBucket(me), ddp.FlatBucket(mg)
    oe, og = FlatAdam(be, lr=0.0), FlatAdam(bg, lr=0.0)
    s0 = TG._scene(0)
    names = [n for n, _ in controlplane.host_pieces(me, s0[2], s0[1], s0[3])[0]]
    assert "row" not in names and "hyp0" in names
    le = TG._eager_step(me, crit, be, oe, s0)
    assert np.isfinite(le) and torch.isfinite(be.flat).all() and float(be.flat.abs().max()) > 0
    for name, p in me.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), name
    step = GraphedTrainStep(mg, crit, bg, og, tuple(t.to(DEV) for t in s0[:4]) + ({k: v.to(DEV) for k, v in s0[4].items()},), warmup=2)
    for k in (1, 2):
        sc = TG._scene(k)
        le = TG._eager_step(me, crit, be, oe, sc)
        lg = float(step(sc[0], sc[1], sc[2], sc[3], sc[4]))
        print(f"scene {k}: loss eager {le:.6f} graph {lg:.6f}; gradient L2 rel {TG._l2(bg.flat, be.flat):.2e}")
        assert abs(lg - le) <= 2e-5 * abs(le)
        assert torch.isfinite(bg.flat).all() and TG._l2(bg.flat, be.flat) < 1e-3
