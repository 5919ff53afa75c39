"""GPU: the "atv" hypothesis curve -- atv_spread_kernel and atv_hypos_kernel (mdf-net_amd/csrc/regress.hip), the slot, the model.

Spread: |e - e64| <= (D/2 + 4) * 2^-24 * e64, e64 the formula in float64 on the same fp32 inputs, and exactly 0 where the sum is
exactly 0 (tests/atv_mirror.py has the derivation; inputs are drawn so that the sum is 0 or >= 1e-30).  Hypotheses given the
spread: bit-identical to the explicit-order fp32 mirror, NaN at the same places.  Each case prints its largest error as a share of
the bar.

Shapes: one pixel; below one wave with a batch stride; a wave boundary with a tail; the switch to 256-thread blocks (262 144
pixels); the 8192-block grid cap, where the grid-stride loop takes a second trip (2 368 000 pixels for the spread, 2 160 000 output
pixels for the hypotheses).  D: the register forms 48 / 24 / 8, the generic 17, and 1."""
import contextlib
import functools
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
import mdfnet_hip  # noqa: E402
from mdfnet_hip import ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
F32 = np.float32

SMALL = [(1, 1, 1), (2, 5, 7), (1, 9, 31)]
SWITCH = (1, 512, 512)                 # 262 144 pixels: the first size with 256-thread blocks
BIG = (1, 1184, 2000)                  # 2 368 000 pixels > 8192 blocks * 256 threads
SPREAD_CASES = [(s, d) for s in SMALL for d in (48, 24, 8, 17, 1)] + [(SWITCH, 8), (BIG, 8)]
HYP_BIG = (1, 600, 900)                # x2: 2 160 000 output pixels > 8192 * 256
HYPOS_CASES = [(s, d) for s in SMALL + [HYP_BIG] for d in (24, 8, 2)]
COMPOSITIONS = [("atv", "atv"), ("gauss1", "atv"), ("atv", "laplace")]


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(a):
    return T(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=2)
def spread_inputs(shape, D):
    """-> prob, {per_pixel: (hyp, depth)}: the seeded volumes of tests/heads_mirror.py (softmax, one-hot, uniform, denormal tails),
    the depth the soft-argmin of each; never written to.  A pixel whose sum falls inside (0, 1e-30) for either form of the
    hypotheses (a one-hot up to a denormal tail) is outside the bound's scope and is redrawn as a uniform volume."""
    B, h, w = shape
    seed = (B * 1000003 + h * 10007 + w * 101 + D) % (2 ** 31 - 1)
    prob, _, _ = M.make_probs(B, D, h, w, seed)
    hyp = {pp: M.make_hypos(B, D, h, w, pp, seed) for pp in (False, True)}
    out = np.zeros((B, h, w), bool)
    for pp in (False, True):
        out |= ~A.in_scope(prob, M.depth_regress(prob, hyp[pp]), hyp[pp])
    prob = np.where(out[:, None], F32(1) / F32(D), prob).astype(F32)
    print(f"inputs {shape} D={D}: {int(out.sum())} of {out.size} pixels redrawn")
    return prob, {pp: (hyp[pp], M.depth_regress(prob, hyp[pp])) for pp in (False, True)}


# --------------------------------------------------------------------------- the spread bar at edge shapes and depths
@pytest.mark.parametrize("shape,D", SPREAD_CASES, ids=[f"{_id(s)}-D{d}" for s, d in SPREAD_CASES])
def test_spread_bar_at_edge_shapes(shape, D):
    prob, hyps = spread_inputs(shape, D)
    pg = dev(prob)
    for per_pixel in (False, True):
        hyp, depth = hyps[per_pixel]
        for scale in (1.5, 0.3):
            e = host(ops.atv_spread(pg, dev(depth), dev(hyp), scale))
            A.check_spread(e, prob, depth, hyp, scale, f"spread {shape} D={D} per_pixel={int(per_pixel)} scale={scale}")
            if shape in (SWITCH, BIG):
                break
    assert mdfnet_hip.lib().mdf_last_launch().decode() == "atv_spread_kernel"
    if shape == BIG:
        assert prob.shape[0] * prob.shape[2] * prob.shape[3] > 8192 * 256


def test_spread_values():
    """One-hot probabilities (the depth on the hot hypothesis: every term an exact zero, e == 0; the depth elsewhere: one term),
    zero probabilities (e == 0), denormal probabilities beside a normal one, and denormal probabilities alone with hypotheses
    far enough apart that the sum is >= 1e-30 (with denormals flushed that pixel would be 0)."""
    for D in (8, 5):
        n = 8
        prob = np.zeros((1, D, 1, n), F32)
        hyp = M.make_hypos(1, D, 1, n, True, 3)
        depth = np.full((1, 1, n), 600.0, F32)
        prob[0, 2, 0, 0] = 1.0
        depth[0, 0, 0] = hyp[0, 2, 0, 0]                    # one-hot, depth on it: e == 0
        prob[0, D - 1, 0, 1] = 1.0
        depth[0, 0, 1] = hyp[0, 0, 0, 1]                    # one-hot, depth on another hypothesis
        prob[0, 0, 0, 2] = 1.0                              # one-hot, depth between the hypotheses
        #                          pixel 3: zero probabilities: e == 0
        prob[0, :, 0, 4] = 1e-42
        prob[0, 1, 0, 4] = 0.75                             # denormals beside a normal value
        prob[0, :, 0, 5] = [F32(1e-39), F32(1e-42)] + [F32(3e-41)] * (D - 2)
        hyp[0, :, 0, 5] = np.arange(D, dtype=F32) * F32(4e5) + F32(1e5)      # denormals alone: p u >= 1e-39 * 1e10
        depth[0, 0, 5] = 0.0
        prob[0, :, 0, 6] = 1.0 / D                          # uniform
        prob[0, :, 0, 7] = 2e-38                            # just above the smallest normal
        hyp[0, :, 0, 7] = hyp[0, :, 0, 5]
        depth[0, 0, 7] = 0.0
        e = host(ops.atv_spread(dev(prob), dev(depth), dev(hyp), 1.5))
        print(f"D={D}: e =", e[0, 0])
        A.check_spread(e, prob, depth, hyp, 1.5, f"values D={D} per-pixel")
        assert e[0, 0, 0] == 0 and e[0, 0, 3] == 0 and (e[0, 0, [1, 2, 4, 5, 6, 7]] > 0).all()
        # the same volumes on hypotheses shared by all pixels
        shared = M.make_hypos(1, D, 1, n, False, 3)
        depth_s = depth.copy()
        depth_s[0, 0, 0] = shared[0, 2, 0, 0]
        e = host(ops.atv_spread(dev(prob[..., :5]), dev(depth_s[..., :5]), dev(shared), 1.5))
        A.check_spread(e, prob[..., :5], depth_s[..., :5], shared, 1.5, f"values D={D} shared")
        assert e[0, 0, 0] == 0 and e[0, 0, 3] == 0


def test_spread_of_a_denormal_tail_stays_relative():
    """Below the drawn scope, where a model's tensors can fall: a one-hot on a hypothesis equal to the depth but for one denormal
    tail probability a few hypotheses away, sum = p_tail * (x - depth)^2 near 1e-38.  An fp32 sum of p * u would round there with an
    absolute error of 2^-150, thousands of times the bar; the kernel sums p * 2^64 and scales the root back, both exact, so the
    same relative bar holds."""
    D, n = 8, 6
    hyp = M.make_hypos(1, D, 1, n, True, 5)
    prob = np.zeros((1, D, 1, n), F32)
    prob[0, 3] = 1.0
    depth = hyp[:, 3].copy()
    prob[0, 6, 0, :] = [1e-45, 1e-42, 3e-41, 1e-39, 1e-38, 0.0]
    s = A.spread64(prob, depth, hyp, 1.0)[1]
    assert ((s[0, 0, :5] > 0) & (s[0, 0, :5] < 1e-30)).all() and s[0, 0, 5] == 0
    e = host(ops.atv_spread(dev(prob), dev(depth), dev(hyp), 1.5))
    print("e =", e[0, 0])
    A.check_spread(e, prob, depth, hyp, 1.5, "denormal tails", drawn=False)
    assert (e[0, 0, :5] > 0).all() and e[0, 0, 5] == 0


# --------------------------------------------------------------------------- the hypotheses: the mirror's bits
@functools.lru_cache(maxsize=2)
def hypos_inputs(shape):
    """e and depth [B,h,w]: e log-uniform over 1e-3 .. 1e4 around depths of 0.5 .. 1000 (both branches of min), and planted: e = 0,
    e > depth, e = inf, e = NaN, each once per 16 pixels (the bilinear blend spreads an inf or a NaN over its neighbours)."""
    B, h, w = shape
    rs = np.random.RandomState(B * 7 + h * 131 + w)
    e = (10.0 ** rs.uniform(-3, 4, shape)).astype(F32)
    depth = M.make_fit_inputs(B, h, w, h + w)[1]
    depth = np.abs(depth) + F32(0.25)
    flat = e.reshape(-1)
    k = np.arange(flat.size)
    flat[k % 16 == 3] = 0.0
    flat[k % 16 == 7] = depth.reshape(-1)[k % 16 == 7] * F32(3)
    flat[k % 16 == 11] = np.inf
    flat[k % 16 == 15] = np.nan
    if flat.size == 1:
        flat[0] = 0.0
    return e, depth


@pytest.mark.parametrize("shape,D_out", HYPOS_CASES, ids=[f"{_id(s)}-D{d}" for s, d in HYPOS_CASES])
def test_hypos_are_the_mirrors_bits(shape, D_out):
    e, depth = hypos_inputs(shape)
    eg, dg = dev(e), dev(depth)
    for upsample in (True, False):
        out = host(ops.atv_hypos(eg, dg, D_out, upsample))
        want = A.atv_hypos(e, depth, D_out, upsample)
        same = M.same_bits(out, want)
        assert same.all(), f"{shape} D_out={D_out} upsample={upsample}: {int((~same).sum())} of {same.size} values differ"
        assert np.array_equal(np.isnan(out), np.isnan(want))
        if e.size >= 16:
            assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
        assert (out[np.isfinite(out)] >= F32(1e-12)).all()
    assert mdfnet_hip.lib().mdf_last_launch().decode() == "atv_hypos_kernel"
    if shape == HYP_BIG:
        assert 4 * e.size > 8192 * 256


def test_single_pixel_planted_values():
    """One pixel, each planted value in turn (the seeded single-pixel case above holds e = 0 only)."""
    for ev in (0.0, 5.0, 2000.0, np.inf, np.nan):
        e, depth = np.full((1, 1, 1), ev, F32), np.full((1, 1, 1), 600.0, F32)
        for upsample in (True, False):
            out = host(ops.atv_hypos(dev(e), dev(depth), 8, upsample))
            assert M.same_bits(out, A.atv_hypos(e, depth, 8, upsample)).all(), (ev, upsample, out.ravel())


# --------------------------------------------------------------------------- the goldens
@pytest.mark.parametrize("case,st", [("atv_01", 0), ("atv_12", 1), ("atv_01_wide", 0), ("atv_12_wide", 1)])
def test_golden_transitions(golden, case, st):
    """The reference's fp32 atv_hypos on the golden transitions: given its spread, bit for bit; and the two kernels end to end (the
    spread held to its bar of the golden float64) inside the slot bar."""
    g, c = golden("ops.npz"), golden("atv_hypos.npz")
    prob, depth, hyp = g[f"reg{st}_prob"], g[f"reg{st}_depth"], g[f"agg{st}_hyp"]
    nd, scale = int(c[case + "_ndepths"]), float(c[case + "_scale"])
    out = host(ops.atv_hypos(dev(c[case + "_e32"]), dev(depth), nd, True))
    assert M.same_bits(out, c[case + "_out32"]).all()
    e = ops.atv_spread(dev(prob), dev(depth), dev(hyp), scale)
    A.check_spread(host(e), prob, depth, hyp, scale, case)
    end = host(ops.atv_hypos(e, dev(depth), nd, True))
    bar = A.slot_bar(prob.shape[1], c[case + "_e64"].max(), np.abs(c[case + "_out64"]).max())
    err = float(np.abs(end - c[case + "_out32"]).max())
    print(f"{case}: both kernels against the reference's fp32: max |d| = {err:.3e} (slot bar {bar:.3e})")
    assert err <= bar


def test_error_paths():
    prob, _, _ = M.make_probs(1, 8, 4, 6, 1)
    hyp = M.make_hypos(1, 8, 4, 6, True, 1)
    depth = M.depth_regress(prob, hyp)
    for bad in (0.0, -1.5, float("inf"), float("nan")):
        with pytest.raises(mdfnet_hip.MdfHipError) as e:
            ops.atv_spread(dev(prob), dev(depth), dev(hyp), bad)
        assert "code -1" in str(e.value) and "scale" in str(e.value)
    with pytest.raises(mdfnet_hip.MdfHipError) as e:
        ops.atv_hypos(dev(depth), dev(depth), 1, True)
    assert "code -1" in str(e.value) and "D_out" in str(e.value)
    with pytest.raises(ValueError):
        ops.atv_spread(dev(prob), dev(depth[:, :2]), dev(hyp), 1.5)
    with pytest.raises(ValueError):
        ops.atv_hypos(dev(depth), dev(depth[:, :2]), 8, True)
    # the fit entries keep rejecting the next free modes
    with pytest.raises(mdfnet_hip.MdfHipError):
        ops.hypos_fit(5, dev(prob), dev(depth), dev(hyp))
    with pytest.raises(mdfnet_hip.MdfHipError):
        ops.hypos_from_fit(3, dev(depth), dev(depth), dev(np.array([[425.0, 935.0]], F32)), -0.05, 8, True)


# --------------------------------------------------------------------------- the model
def _build(curves=None, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        m = config.build_model(curves=curves, **kw)
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=1))
    return m


def _scene():
    return synth.make_scene(160, 128, 3, batch=1, rot_deg=2.0, seed=3)


@pytest.mark.parametrize("curves", COMPOSITIONS, ids="-".join)
def test_model_with_atv(monkeypatch, curves):
    """Eval forward at 160x128, 3 views, seeded weights: finite outputs; every stage's regressed depth inside the interval
    [hyp_0, hyp_last] that stage was given, up to D roundings (a convex combination of D hypotheses); every spread the model
    computed held to the bar on the tensors it was handed; the atv stages make the two launches and no fit."""
    model = _build(curves).eval().to(DEV)
    calls = []
    real = ops.atv_spread

    def spy(prob, depth, hyp, scale=1.5):
        e = real(prob, depth, hyp, scale)
        calls.append((host(prob), host(depth), host(hyp), scale, host(e)))
        return e
    monkeypatch.setattr(ops, "atv_spread", spy)
    taps = []
    ops.count_begin()
    with torch.no_grad():
        out = model(*[t.to(DEV) for t in _scene()], stage_tap=lambda d: taps.append({k: (host(v) if torch.is_tensor(v) else v) for k, v in d.items()}))
    counts = ops.count_end()
    n_atv = sum(c == "atv" for c in curves)
    assert len(calls) == n_atv and counts.get("mdf_atv_hypos_fwd", 0) == n_atv
    assert counts.get("mdf_hypos_fit_fwd", 0) == counts.get("mdf_hypos_from_fit_fwd", 0) == 2 - n_atv
    assert [c[0].shape[1] for c in calls] == [d for d, cv in zip((48, 24), curves) if cv == "atv"]
    for prob, depth, hyp, scale, e in calls:
        assert scale == 1.5
        A.check_spread(e, prob, depth, hyp, scale, f"model {curves} D={prob.shape[1]} {prob.shape[2:]}", drawn=False)
    stages = [t for t in taps if t["stage"] != "final"]
    assert [t["stage"] for t in stages] == [0, 1, 2]
    for t in stages:
        hyp, depth = t["hypos"], t["depth"]
        D = hyp.shape[1]
        lo, hi = np.broadcast_to(hyp[:, 0], depth.shape), np.broadcast_to(hyp[:, -1], depth.shape)
        tol = D * M.EPS * np.abs(hi)
        worst = float(np.maximum((lo - depth) / tol, (depth - hi) / tol).max())
        print(f"{curves} stage {t['stage']}: hypotheses {hyp.min():.3f} .. {hyp.max():.3f}, depth outside its interval by at most "
              f"{max(worst, 0.0):.3f} of D roundings")
        assert np.isfinite(hyp).all() and np.isfinite(depth).all() and (hyp[:, 0] <= hyp[:, -1]).all()
        assert (depth >= lo - tol).all() and (depth <= hi + tol).all()
    depth, conf = host(out["depth"]), host(out["confidence"])
    assert depth.shape == (1, 128, 160) and np.isfinite(depth).all() and np.isfinite(conf).all()
    assert (conf >= 0).all() and (conf <= 1 + 4 * M.EPS).all()


def test_default_model_is_untouched():
    """The default composition runs exactly the launches it ran -- no atv entry -- and gives the same bits before and after an atv
    model has run in the process, whatever atv_scale it was built with (no slot of it reads the scale)."""
    scene = [t.to(DEV) for t in _scene()]
    default = _build().eval().to(DEV)
    ops.count_begin()
    with torch.no_grad():
        before = default(*scene)
    counts = ops.count_end()
    assert not any(k.startswith("mdf_atv") for k in counts) and counts["mdf_hypos_fit_fwd"] == counts["mdf_hypos_from_fit_fwd"] == 2
    with torch.no_grad():
        _build(("atv", "atv")).eval().to(DEV)(*scene)
        after = default(*scene)
        scaled = _build(atv_scale=(3.0, 0.25)).eval().to(DEV)(*scene)
    for k in ("depth", "confidence"):
        assert torch.equal(before[k], after[k]) and torch.equal(before[k], scaled[k])


# --------------------------------------------------------------------------- training
def test_training_step_eager_and_recorded():
    """One eager training step of the ("atv", "atv") model at the tiny training shape: loss and every gradient finite; and the step
    recorded as a hipGraph held to the comparison tests/test_train_graph_gpu.py makes for the default model (learning rate 0:
    loss within 2e-5 relative, gradients within 1e-3 in L2, on inputs the recording has not seen).  The slot takes nothing from the
    host: the control plane carries no fit row for this composition."""
    import test_train_graph_gpu as TG
    from mdfnet_hip import controlplane, ddp
    from mdfnet_hip.graphstep import GraphedTrainStep
    from mdfnet_hip.optim import FlatAdam
    from net.loss import Loss
    crit = Loss().to(DEV)
    me, mg = (_build(("atv", "atv")).train().to(DEV) for _ in range(2))
    assert controlplane.builtin_slots(mg)
    be, bg = ddp.FlatBucket(me), ddp.FlatBucket(mg)
    oe, og = FlatAdam(be, lr=0.0), FlatAdam(bg, lr=0.0)
    s0 = TG._scene(0)
    names = [n for n, _ in controlplane.host_pieces(me, s0[2], s0[1], s0[3])[0]]
    assert "row" not in names and "hyp0" in names
    ops.count_begin()
    le = TG._eager_step(me, crit, be, oe, s0)
    counts = ops.count_end()
    assert counts.get("mdf_atv_spread_fwd") == counts.get("mdf_atv_hypos_fwd") == 2 and "mdf_hypos_fit_fwd" not in counts
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
