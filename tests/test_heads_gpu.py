"""GPU parity of the inter-stage head kernels (csrc/regress.hip) at edge shapes, depths and values.

Every kernel is held to two things: the bits of tests/heads_mirror.py (the explicit statement of the operation order the kernels
promise, tied to the reference's goldens in tests/test_heads_mirror_cpu.py) and a float64 reference computed from the same fp32
inputs, with a bound derived from the operation count, never from what the kernel returns.  Each test prints the largest observed
error as a share of its bound.

Shapes: one pixel, one row, one column, ragged maps, both sides of the 64/256-thread switch of block_for (262 144 elements) and a
map of more than 2 097 152 pixels, where the 8192-block grid cap sends the grid-stride loop on a second trip.  D: the templated
48 / 24 / 8 and the generic 1, 2, 3, 5, 16, 17, 49, 64.  Probabilities: heads_mirror.make_probs (random and peaked softmax, one-hot
at the window edges, uniform, exact zeros, denormals).  Depth ranges differ per batch item."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import heads_mirror as M  # noqa: E402
import mdfnet_hip  # noqa: E402
from mdfnet_hip import ops  # noqa: E402
from oracle import mvs_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
EPS = M.EPS

SMALL = [(1, 1, 1), (1, 1, 70), (2, 64, 1), (3, 7, 33), (2, 13, 37), (1, 5, 16)]
SWITCH = [(1, 511, 513), (1, 512, 512)]            # 262 143 and 262 144 pixels: 64- and 256-thread blocks
BIG = (5, 592, 800)                                # 2 368 000 pixels > 8192 blocks * 256 threads
TEMPLATED = [48, 24, 8]
GENERIC = [1, 2, 3, 5, 16, 17, 49, 64]
ALL_D = TEMPLATED + GENERIC
HEAD_CASES = [(s, d) for s in SMALL for d in ALL_D] + [(s, d) for s in SWITCH for d in (8, 17, 48)] + [(BIG, 8)]
LT = {1: float(torch.log(torch.tensor(0.95))), 2: float(torch.log(torch.tensor(1e-5)))}   # config.py's thresholds


def _seed(shape, d):
    b, h, w = shape
    return (b * 1000003 + h * 10007 + w * 101 + d) % (2 ** 31 - 1)


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(a):
    return T(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def assert_bits(got, want, what):
    bad = ~M.same_bits(got, want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {i}: "
                             f"kernel {got[i]!r} mirror {want[i]!r}")


def onehot_pixels(prob):
    return (prob == 1).any(1) & ((prob != 0).sum(1) == 1)


# --------------------------------------------------------------------------- depth_regress, confidence, confidence_up2
@pytest.mark.parametrize("shape,D", HEAD_CASES, ids=[f"{_id(s)}-D{d}" for s, d in HEAD_CASES])
def test_regress_and_confidence(shape, D):
    """depth_regress / confidence / confidence_up2: bit-equal to the mirror; closed forms on one-hot pixels; float64 bounds.

    Depth against float64: |d - d64| <= D * 2^-24 * sum_d |p_d * h_d| (one rounding per product, D-1 per sum, in any order), plus
    D * 2^-150 for products of planted denormals, which gradual underflow rounds to a fixed step and not to a relative error.

    Index against float64: trunc(E) may differ from trunc(E64) only where E64 lies within D*(D-1)*2^-24 of an integer (one rounding
    per product, D-1 per sum, |p_d * d| <= D-1).  One-hot pixels (and D = 1, where E = p*0) have E integral in both precisions and
    are compared, not excluded.  The share of excluded pixels is held to 0.2 % over the pixels in general position (random
    softmax, with and without planted denormals), the inputs that figure was measured on.  Peaked softmax and uniform 1/D put E next
    to an integer by construction (1/D at odd D: E64 = (D-1)/2 * (1 +- 2^-24)); there the kernel's index is held to the mirror's
    bits, to |idx - E64| < 1 + bound, and to float64 outside the band like every other pixel."""
    B, h, w = shape
    seed = _seed(shape, D)
    prob, kind, plane = M.make_probs(B, D, h, w, seed)
    names = np.array(M.KINDS)[kind]
    hot = plane >= 0
    pg = dev(prob)
    n = B * h * w

    for per_pixel in (False, True):
        hyp = M.make_hypos(B, D, h, w, per_pixel, seed)
        d = host(ops.depth_regress(pg, dev(hyp)))
        assert d.shape == (B, h, w) and d.dtype == np.float32
        assert_bits(d, M.depth_regress(prob, hyp), f"depth_regress per_pixel={per_pixel}")
        d64, a64 = M.depth_regress64(prob, np.broadcast_to(hyp, prob.shape))
        bound = D * EPS * a64 + D * 2.0 ** -150      # a product below FLT_MIN rounds to half a denormal step: absolute, not relative
        assert (np.abs(d - d64) <= bound).all()
        hk = np.take_along_axis(np.broadcast_to(hyp, prob.shape), np.maximum(plane, 0)[:, None], 1)[:, 0]
        assert np.array_equal(d[hot], hk[hot]), "one-hot pixel: depth is not the hot hypothesis"
        print(f"depth_regress {shape} D={D} per_pixel={int(per_pixel)}: max |d - d64| / bound = "
              f"{float(np.max(np.abs(d - d64) / np.where(bound > 0, bound, 1))):.3f}")

    conf_t, idx_t = ops.confidence(pg, return_index=True)
    assert idx_t.dtype == torch.int64
    conf, idx = host(conf_t), host(idx_t)
    mconf, midx = M.confidence(prob)
    assert_bits(idx, midx, "confidence index")
    assert_bits(conf, mconf, "confidence")
    assert_bits(host(ops.confidence(pg)), mconf, "confidence without index")
    assert np.array_equal(idx[hot], plane[hot]) and (conf[hot] == 1.0).all(), "one-hot pixel: index k, confidence 1"

    e64 = M.expectation64(prob)
    band = D * (D - 1) * EPS
    exact = onehot_pixels(prob) | (D == 1)
    near = (np.abs(e64 - np.rint(e64)) <= band) & ~exact
    assert np.array_equal(idx[~near], np.trunc(e64).astype(np.int64)[~near])
    assert ((idx <= e64 + band) & (idx > e64 - 1 - band)).all()
    general = np.isin(names, ("softmax3", "planted") if D >= 4 else ("softmax3",))   # planting leaves D-2 planes of random mass
    share = float((near & general).sum()) / max(int(general.sum()), 1)
    print(f"confidence {shape} D={D}: index pixels within the float64 band: {int((near & general).sum())} of {int(general.sum())} "
          f"in general position ({100 * share:.4f} %), {int((near & ~general).sum())} of {int((~general & ~exact).sum())} peaked/uniform")
    assert share <= 0.002

    up = ops.confidence_up2(pg)
    assert up.shape == (B, 2 * h, 2 * w)
    assert torch.equal(up, F.interpolate(conf_t[:, None], scale_factor=2, mode="nearest")[:, 0])
    assert_bits(host(up), M.confidence_up2(prob), "confidence_up2")
    if shape == BIG:
        assert n > 8192 * 256      # the grid-stride loops took a second trip, and every element was compared above


# --------------------------------------------------------------------------- range_affine
@pytest.mark.parametrize("B,n", [(1, 262143), (1, 262144), (3, 87381), (3, 87382), (3, 1), (1, 70), (5, 473600)])
def test_range_affine(B, n):
    """Bit-equal to the fp32 torch expressions on the CPU (elementwise IEEE: host-independent), both sides of the thread switch."""
    rs = np.random.RandomState(B * 7 + n)
    r = M.depth_ranges(B)
    lo, span = r[:, 0].copy(), (r[:, 1] - r[:, 0]).copy()
    x = rs.uniform(-50, 1100, (B, n)).astype(np.float32)
    u = rs.uniform(-0.2, 1.2, (B, n)).astype(np.float32)
    tl, ts = T(lo).reshape(B, 1), T(span).reshape(B, 1)
    for mode, inp, want in ((0, x, (T(x) - tl) / ts), (1, u, tl + T(u) * ts)):
        got = host(ops.range_affine(dev(inp), dev(lo), dev(span), mode))
        assert_bits(got, want.numpy(), f"range_affine mode {mode}")
        assert_bits(got, M.range_affine(inp, lo, span, mode), f"range_affine mode {mode} vs mirror")
    x4 = x[:, : (n // 2) * 2].reshape(B, 1, -1, 2) if n >= 2 else x.reshape(B, 1, 1, 1)    # the [B,1,h,w] form refine.py passes
    assert_bits(host(ops.range_affine(dev(x4), dev(lo.reshape(B, 1, 1, 1)), dev(span.reshape(B, 1, 1, 1)), 0)),
                M.range_affine(x4, lo, span, 0), "range_affine 4-d")


# --------------------------------------------------------------------------- hypos_fit
FIT_CASES = [(s, d) for s in SMALL for d in ALL_D] + [(s, d) for s in SWITCH for d in (8, 17)] + [(BIG, 8)]


@pytest.mark.parametrize("shape,D", FIT_CASES, ids=[f"{_id(s)}-D{d}" for s, d in FIT_CASES])
def test_hypos_fit_laplace(shape, D):
    """mode 2: every term of sum(x*y) and of sum(x*x) has one sign, so s is held to a RELATIVE bound against float64:
    (2*D + 8) * 2^-24: x one rounding, logf one ulp, the product, D-1 additions: D+2 for each sum, the division and the reciprocal.
    Where the float64 sum(x*x) is 0 (every hypothesis equals the depth: D = 1) both sides are 0/0 = NaN."""
    B, h, w = shape
    seed = _seed(shape, D)
    prob, _, _ = M.make_probs(B, D, h, w, seed)
    pg = dev(prob)
    for per_pixel in ((False,) if shape == BIG else (False, True)):
        hyp = M.make_hypos(B, D, h, w, per_pixel, seed)
        depth = M.depth_regress(prob, hyp)
        s = host(ops.hypos_fit(2, pg, dev(depth), dev(hyp)))
        s64, sxx = M.laplace_fit64(prob, depth, np.broadcast_to(hyp, prob.shape))
        degenerate = sxx == 0
        assert degenerate.all() if D == 1 else not degenerate.any()
        assert np.isnan(s[degenerate]).all() and np.isnan(s64[degenerate]).all()
        ok = ~degenerate
        assert np.isfinite(s[ok]).all() and (s[ok] > 0).all()
        rel = np.abs(s[ok] - s64[ok]) / s64[ok]
        bound = (2 * D + 8) * EPS
        print(f"laplace s {shape} D={D} per_pixel={int(per_pixel)}: max rel err / bound = "
              f"{(float(rel.max()) / bound if rel.size else 0.0):.3f}")
        assert (rel <= bound).all()


def _fit_row(hyp, D, seed):
    if D >= 3:
        return ops.gauss1_fit_row(T(hyp)).numpy()
    # X^T X is singular below three planes; the kernel only needs a row, so give it a seeded one
    return np.random.RandomState(seed).standard_normal((hyp.shape[0], D)).astype(np.float32)


@pytest.mark.parametrize("shape,D", FIT_CASES, ids=[f"{_id(s)}-D{d}" for s, d in FIT_CASES])
def test_hypos_fit_gauss1(shape, D):
    """mode 1: acc = sum_d row_d * ln p_d cancels, so the sum is bounded, not s: with the same row on both sides
    | |acc_gpu| - |acc_64| | <= (D + 3) * 2^-24 * sum_d |row_d * ln p_d|   (logf one ulp, the product, D-1 additions, and the division
    that the kernel's s = |-1/acc| adds before this test inverts it in float64)."""
    B, h, w = shape
    seed = _seed(shape, D)
    prob, _, _ = M.make_probs(B, D, h, w, seed)
    hyp = M.make_hypos(B, D, 1, 1, False, seed)
    row = _fit_row(hyp, D, seed)
    assert np.isfinite(row).all()
    s = host(ops.hypos_fit(1, dev(prob), None, dev(hyp), dev(row)))
    a64, abs64 = M.gauss1_fit64(prob, row)
    with np.errstate(divide="ignore"):
        acc = 1.0 / s.astype(np.float64)
    assert not np.isnan(s).any() and (s >= 0).all()
    bound = (D + 3) * EPS * abs64
    err = np.abs(acc - a64)
    print(f"gauss1 |acc| {shape} D={D}: max err / bound = {float(np.max(err / np.where(bound > 0, bound, 1))):.3f}")
    assert (err <= bound).all()


def test_hypos_fit_log_of_zero_and_denormal_probabilities():
    """ln max(p, 1e-40f): a zero or a 1e-42 gives ln(float32(1e-40)) = -92.1034, a 1e-39 (a denormal above the clamp) its own
    logarithm.  With denormals flushed the clamp would be 0 and s would be 0 or NaN.  A unit fit row reads one plane's ln."""
    D = 5
    prob = np.zeros((1, D, 1, 4), np.float32)
    prob[0, 0] = 1.0
    prob[0, 2] = [0.0, 1e-42, 1e-39, 1e-38]
    row = np.zeros((1, D), np.float32)
    row[0, 2] = 1.0
    hyp = M.make_hypos(1, D, 1, 1, False, 0)
    s = host(ops.hypos_fit(1, dev(prob), None, dev(hyp), dev(row)))[0, 0]
    want = 1.0 / np.abs(np.log(np.maximum(prob[0, 2, 0], M.PCLAMP).astype(np.float64)))
    print("gauss1 s for p = 0, 1e-42, 1e-39, 1e-38 under a unit row:", s, "1/s:", 1 / s.astype(np.float64))
    assert abs(1 / want[0] - 92.1034) < 1e-3 and want[0] == want[1] and want[2] > want[1]
    assert (np.abs(s - want) <= 3 * EPS * want).all()
    # laplace: x = |hyp - depth| with depth = hyp_0, so plane 0 drops out and the zeros' logs carry the sum
    depth = M.depth_regress(prob, hyp)
    s2 = host(ops.hypos_fit(2, dev(prob), dev(depth), dev(hyp)))
    s64, _ = M.laplace_fit64(prob, depth, np.broadcast_to(hyp, prob.shape))
    assert np.isfinite(s2).all() and (np.abs(s2 - s64) <= (2 * D + 8) * EPS * s64).all()


def test_gauss1_refuses_per_pixel_hypotheses():
    prob, _, _ = M.make_probs(1, 8, 4, 6, 1)
    hyp = M.make_hypos(1, 8, 4, 6, True, 1)
    row = np.zeros((1, 8), np.float32)
    with pytest.raises(mdfnet_hip.MdfHipError) as e:
        ops.hypos_fit(1, dev(prob), None, dev(hyp), dev(row))
    assert "code -2" in str(e.value) and "per-pixel" in str(e.value)      # MDF_EUNSUPPORTED


# --------------------------------------------------------------------------- hypos_from_fit
def torch_step2(mode, s, depth, rng, d_out, upsample, monkeypatch):
    """O.hypos_by_fit's step 2 in fp32 on the CPU, fed the given s instead of its own fit."""
    monkeypatch.setattr(O, "gauss1_fit", lambda prob, hyp: T(s.copy()))
    monkeypatch.setattr(O, "laplace_fit", lambda depth_, prob, hyp: T(s.copy()))
    thr = {1: 0.95, 2: 1e-5}[mode]
    return O.hypos_by_fit(T(depth.copy()), T(rng.copy()), None, None, d_out, "gauss1" if mode == 1 else "laplace", thr, upsample).numpy()


def plant(s, variant):
    """inf or NaN at an interior pixel, next to the left and the top border (bilinear weight 0 from column / row 0), and in the
    last row and column; s = 0 and an s so large that both caps bind."""
    s = s.copy()
    _, h, w = s.shape
    v = {"inf": np.inf, "nan": np.nan}[variant]
    for y, x in ((h // 2, w // 2), (h // 2, min(1, w - 1)), (min(1, h - 1), w // 2), (h - 1, w // 3), (h // 3, w - 1)):
        s[0, y, x] = v
    s[-1, h // 4, w // 4] = 0.0
    s[-1, (3 * h) // 4, (3 * w) // 4] = 1e30
    return s


def check_from_fit(mode, shape, d_out, upsample, monkeypatch, compare_torch=True):
    B, h, w = shape
    rng = M.depth_ranges(B)
    s0, depth = M.make_fit_inputs(B, h, w, _seed(shape, d_out))
    lo, hi = rng[:, 0].reshape(B, 1, 1, 1), rng[:, 1].reshape(B, 1, 1, 1)
    worst = 0.0
    for variant in (None, "inf", "nan"):
        s = s0 if variant is None else plant(s0, variant)
        if variant is None:
            s = s.copy()
            s[-1, h // 4, w // 4] = 0.0
            s[-1, (3 * h) // 4, (3 * w) // 4] = 1e30
        out = host(ops.hypos_from_fit(mode, dev(s), dev(depth), dev(rng), LT[mode], d_out, upsample))
        assert out.shape == (B, d_out, 2 * h if upsample else h, 2 * w if upsample else w)
        assert_bits(out, M.hypos_from_fit(mode, s, depth, rng, LT[mode], d_out, upsample), f"hypos_from_fit mode {mode} {variant}")
        fin = np.isfinite(out)
        assert (np.isnan(out) | fin).all() and (fin.all() if variant is None else np.isnan(out).any() or not np.isnan(s).any())
        with np.errstate(invalid="ignore"):
            assert ((out >= lo) & (out <= hi))[fin].all()
            assert (np.diff(out, axis=1) >= 0)[fin[:, 1:] & fin[:, :-1]].all()
        if compare_torch:
            ref = torch_step2(mode, s, depth, rng, d_out, upsample, monkeypatch)
            for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
                assert np.array_equal(f(out), f(ref)), f"{name} positions differ from torch's step 2 ({variant})"
        if variant is None:
            r64 = M.hypos_from_fit64(mode, s, depth, rng, LT[mode], d_out, upsample)
            bound = 16 * EPS * float(np.abs(rng).max())
            worst = float(np.abs(out - r64).max()) / bound
            assert worst <= 1.0, worst
    print(f"hypos_from_fit mode {mode} {shape} D_out={d_out} up={int(upsample)}: max |out - out64| / bound = {worst:.3f}")


@pytest.mark.parametrize("upsample", [False, True], ids=["same", "up2"])
@pytest.mark.parametrize("d_out", [2, 8, 24, 48])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", SMALL, ids=_id)
def test_hypos_from_fit(shape, mode, d_out, upsample, monkeypatch):
    """Bit-equal to the mirror, NaN included; non-finite positions as torch's fp32 step 2 on the CPU; monotone in k and inside
    [lo, hi] where finite; against float64 at most 16 * 2^-24 * max|range| on the unplanted inputs: four bilinear roundings on the
    depth, the same on s (halved by the sqrt), base, step*k and the add, and the two clip pairs."""
    check_from_fit(mode, shape, d_out, upsample, monkeypatch)


FROM_FIT_LARGE = [((1, 255, 257), 8, True), ((1, 256, 256), 8, True),       # 262 140 and 262 144 OUTPUT pixels
                  ((1, 511, 513), 24, False), ((1, 512, 512), 24, False),
                  ((5, 296, 400), 8, True), ((5, 592, 800), 2, False)]          # 2 368 000 output pixels: second grid-stride trip


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape,d_out,upsample", FROM_FIT_LARGE, ids=[f"{_id(s)}-D{d}-{'up2' if u else 'same'}" for s, d, u in FROM_FIT_LARGE])
def test_hypos_from_fit_launch_geometry(shape, d_out, upsample, mode, monkeypatch):
    B, h, w = shape
    if B == 5:
        assert B * h * w * (4 if upsample else 1) > 8192 * 256
    check_from_fit(mode, shape, d_out, upsample, monkeypatch, compare_torch=(B == 1))


# --------------------------------------------------------------------------- wrappers and routes
def test_wrappers_accept_strided_prob_and_float64_range():
    B, D, h, w = 2, 17, 13, 37
    prob, _, _ = M.make_probs(B, D, h, w, 3)
    hyp = M.make_hypos(B, D, h, w, True, 3)
    pc, hc = dev(prob), dev(hyp)
    pv = dev(np.ascontiguousarray(prob.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)      # same values, [B,h,w,D] memory
    hv = dev(np.ascontiguousarray(hyp.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
    assert not pv.is_contiguous() and torch.equal(pv, pc)
    depth = ops.depth_regress(pc, hc)
    assert torch.equal(ops.depth_regress(pv, hv), depth)
    assert torch.equal(ops.confidence(pv), ops.confidence(pc))
    assert torch.equal(ops.confidence_up2(pv), ops.confidence_up2(pc))
    s = ops.hypos_fit(2, pc, depth, hc)
    assert torch.equal(ops.hypos_fit(2, pv, depth.double(), hv), s)
    rng = M.depth_ranges(B)
    a = ops.hypos_from_fit(2, s, depth, dev(rng), LT[2], 8, True)
    # three converted copies in one call: each must live until the launch is enqueued (freed earlier, the next conversion gets the
    # same block of the caching allocator and overwrites it before the kernel reads it)
    b = ops.hypos_from_fit(2, s.double(), depth.double(), dev(rng.astype(np.float64)), LT[2], 8, True)
    assert torch.equal(a, b)
    assert torch.equal(ops.hypos_from_fit(2, s.double(), depth, dev(rng.astype(np.float64)), LT[2], 8, True), a)
    row = ops.gauss1_fit_row(T(M.make_hypos(B, D, 1, 1, False, 3)))
    hp = dev(M.make_hypos(B, D, 1, 1, False, 3))
    assert torch.equal(ops.hypos_fit(1, pv, depth.double(), hp, dev(row.numpy()).double()), ops.hypos_fit(1, pc, None, hp, dev(row.numpy())))
    lo, span = dev(rng[:, 0].astype(np.float64)), dev((rng[:, 1] - rng[:, 0]).astype(np.float64))
    assert torch.equal(ops.range_affine(depth, lo, span, 0), ops.range_affine(depth, lo.float(), span.float(), 0))


def test_routes_taken():
    """Each ABI entry is entered once per call and enqueues the kernel it names, for the templated depths and for a generic one."""
    lib = mdfnet_hip.lib()
    for D in (8, 24, 48, 17):
        prob, _, _ = M.make_probs(1, D, 5, 16, D)
        hyp = M.make_hypos(1, D, 5, 16, False, D)
        pg = dev(prob)
        ops.count_begin()
        s = ops.hypos_fit(2, pg, ops.depth_regress(pg, dev(hyp)), dev(hyp))
        assert lib.mdf_last_launch().decode() == "hypos_fit_kernel"
        up = ops.confidence_up2(pg)
        assert lib.mdf_last_launch().decode() == "confidence_up2_kernel"
        counts = ops.count_end()
        assert counts == {"mdf_depth_regress_fwd": 1, "mdf_hypos_fit_fwd": 1, "mdf_confidence_up2_fwd": 1}, counts
        assert s.shape == (1, 5, 16) and up.shape == (1, 10, 32)
