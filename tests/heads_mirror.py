"""Explicit-order mirror of the inter-stage head kernels (mdf-net_amd/csrc/regress.hip), in numpy.

Why it exists.  The kernels promise the bits of the reference's CPU run, and for `torch.sum(prob * hypos, 1)` that promise has a
scope: ATen's float sum follows the cascade order below only on its vectorised outer-sum path, which covers the pixels inside whole
blocks of four SIMD vectors of the flattened h*w axis (32 floats on an AVX2 host, 64 with AVX-512).  The tail pixels of an odd map go
through a 4-way interleaved row sum and differ in the last bits, so "the bits of live torch" is not one order but depends on the
shape and on the host's CPU.  The goldens (h*w = 96, 384, 1536) have no tail.  The order the kernels promise at EVERY shape is
therefore written down here, tied once to the goldens (tests/test_heads_mirror_cpu.py), and is the definition wherever ATen's own
order is shape-dependent.  Everything else is held to float64 references with bounds derived from operation counts.

fp32 mirrors execute the kernels' operations in the kernels' order, every step rounded to fp32 (numpy float32 arithmetic is IEEE
and keeps denormals).  The float64 references start from the same fp32 inputs and clamp probabilities at np.float32(1e-40), the
(denormal) value the kernels use, not at the double 1e-40.

Nothing here reads the reference tree or needs a GPU."""
import numpy as np

F32 = np.float32
F64 = np.float64
PCLAMP = np.float32(1e-40)          # regress.hip: fmaxf(p, 1e-40f); an fp32 denormal (0x000116c2)
EPS = 2.0 ** -24                    # unit roundoff of fp32
RANGES = np.array([[425.0, 935.0], [300.0, 900.0], [0.5, 1.2], [100.0, 1000.0], [2.0, 9.0]], dtype=np.float32)
KINDS = ("softmax3", "softmax3", "softmax3", "onehot_first", "onehot_last", "onehot_last2", "onehot_mid", "softmax40", "softmax40",
         "uniform", "planted", "planted")


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


# --------------------------------------------------------------------------- fp32 building blocks
def cascade_sum(terms, axis=1):
    """mdf::CascadeSum (common.h): sequential adds into level 0, level 0 folded into level 1 after every 16 elements, level 1
    into level 2 after every 256, level 2 into level 3 after every 4096; result ((l0 + l1) + l2) + l3.  fp32 at every step."""
    t = np.moveaxis(np.asarray(terms, dtype=F32), axis, 0)
    z = np.zeros(t.shape[1:], F32)
    l0, l1, l2, l3 = z, z.copy(), z.copy(), z.copy()
    for n in range(1, t.shape[0] + 1):
        l0 = l0 + t[n - 1]
        if n % 16 == 0:
            l1 = l1 + l0
            l0 = np.zeros_like(z)
            if n % 256 == 0:
                l2 = l2 + l1
                l1 = np.zeros_like(z)
                if n % 4096 == 0:
                    l3 = l3 + l2
                    l2 = np.zeros_like(z)
    return ((l0 + l1) + l2) + l3


def fma32(a, b, c):
    """Correctly rounded fp32 fma.  a*b is exact in float64; the float64 sum is made round-to-odd with the TwoSum error term, so the
    final rounding to fp32 cannot double-round.  Non-finite values pass through the plain float64 expression."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(F64) * b.astype(F64)
        c = c.astype(F64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where((e > 0), np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(F32)


def _hyp_full(hypos, shape):
    return np.broadcast_to(np.asarray(hypos, F32), shape)


# --------------------------------------------------------------------------- fp32 mirrors of the kernels
def depth_regress(prob, hypos):
    """depth_regress_kernel: cascade sum over d of the fp32 products prob_d * hyp_d.  prob [B,D,h,w], hypos [B,D,1,1] | [B,D,h,w]."""
    prob = np.asarray(prob, F32)
    return cascade_sum(prob * _hyp_full(hypos, prob.shape), axis=1)


def confidence(prob):
    """confidence_kernel -> (conf [B,h,w] fp32, idx [B,h,w] int64 as written to idx_out, i.e. before the clamp to [0, D-1]).
    idx = trunc(cascade sum of prob_d * float(d)); conf = ((0 + t[idx-1]) + t[idx]) + t[idx+1]) + t[idx+2] with t = 0 outside [0, D)."""
    prob = np.asarray(prob, F32)
    D = prob.shape[1]
    ramp = np.arange(D, dtype=F32).reshape(1, D, 1, 1)
    e = cascade_sum(prob * ramp, axis=1)
    idx = np.trunc(e).astype(np.int64)
    ic = np.clip(idx, 0, D - 1)
    s = np.zeros(e.shape, F32)
    for k in range(-1, 3):
        kk = ic + k
        v = np.take_along_axis(prob, np.clip(kk, 0, D - 1)[:, None], axis=1)[:, 0]
        s = s + np.where((kk >= 0) & (kk < D), v, F32(0))
    return s, idx


def up2_nearest(m):
    """The x2 nearest placement of confidence_up2_kernel: every value goes to its 2x2 output pixels.  [B,h,w] -> [B,2h,2w]."""
    return np.repeat(np.repeat(np.asarray(m), 2, axis=1), 2, axis=2)


def confidence_up2(prob):
    return up2_nearest(confidence(prob)[0])


def range_affine(x, lo, span, mode):
    """range_affine_kernel: mode 0: (x - lo[b]) / span[b]; mode 1: lo[b] + x * span[b]; separately rounded sub/div and mul/add."""
    x = np.asarray(x, F32)
    sh = (x.shape[0],) + (1,) * (x.ndim - 1)
    lo, span = np.asarray(lo, F32).reshape(sh), np.asarray(span, F32).reshape(sh)
    with np.errstate(all="ignore"):
        return (x - lo) / span if mode == 0 else lo + x * span


def up2_coord(n_out, n_in):
    """regress.hip:up2_coord for every output index: src = (o + 0.5) * 0.5 - 0.5 clamped at 0 -> i0, i1, l0, l1."""
    o = np.arange(n_out, dtype=F32)
    src = (o + F32(0.5)) * F32(0.5) - F32(0.5)
    src = np.where(src < 0, F32(0), src)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(F32)
    l0 = F32(1) - l1
    return i0, i1, l0, l1


def up2_bilinear(m):
    """regress.hip:up2_sample on a whole map [B,h,w] -> [B,2h,2w]:
    w_ij = ly_i * lx_j ; out = fma(w11, v11, fma(w10, v10, fma(w00, v00, w01 * v01)))."""
    m = np.asarray(m, F32)
    _, h, w = m.shape
    y0, y1, ly0, ly1 = up2_coord(2 * h, h)
    x0, x1, lx0, lx1 = up2_coord(2 * w, w)
    v00, v01 = m[:, y0][:, :, x0], m[:, y0][:, :, x1]
    v10, v11 = m[:, y1][:, :, x0], m[:, y1][:, :, x1]
    w00, w01 = ly0[:, None] * lx0[None], ly0[:, None] * lx1[None]
    w10, w11 = ly1[:, None] * lx0[None], ly1[:, None] * lx1[None]
    with np.errstate(invalid="ignore", over="ignore"):
        return fma32(w11, v11, fma32(w10, v10, fma32(w00, v00, w01 * v01)))


def hypos_from_fit(mode, s, depth, rng, log_thresh, d_out, upsample=True, sqrt=np.sqrt):
    """hypos_from_fit_kernel.  s, depth [B,h,w]; rng [B,2]; -> [B,d_out,Ho,Wo].  `x < c ? c : x` keeps a NaN x, as torch.clamp does.
    The square root of mode 1 is the correctly rounded IEEE one, as sqrtf is in the device build.  ATen's vectorised CPU sqrt is not
    (about 1 % of its results are an ulp off on an AVX-512 host), so the mode-1 golden is reproduced bit for bit only up to that ulp
    of `res`; `sqrt` lets a test put another root in."""
    s, depth, rng = np.asarray(s, F32), np.asarray(depth, F32), np.asarray(rng, F32)
    B = s.shape[0]
    lt = F32(log_thresh)
    with np.errstate(all="ignore"):
        gmin, gmax = rng[0, 0], rng[0, 1]
        for b in range(1, B):
            gmin, gmax = np.minimum(gmin, rng[b, 0]), np.maximum(gmax, rng[b, 1])
        cap_all = (gmax - gmin) / F32(2)
        sv, dv = (up2_bilinear(s), up2_bilinear(depth)) if upsample else (s, depth)
        res = f32(sqrt((F32(-1) * sv) * lt)) if mode == 1 else np.abs(sv * lt)
        res = np.where(res < F32(1e-6), F32(1e-6), res)
        res = np.where(res > cap_all, cap_all, res)
        lo, hi = rng[:, 0].reshape(B, 1, 1), rng[:, 1].reshape(B, 1, 1)
        cap_b = (hi - lo) * F32(0.2)
        res = np.where(res > cap_b, cap_b, res).astype(F32)
        step = res / F32(d_out - 1)
        base = dv - F32(0.5) * res
        out = np.empty((B, d_out) + sv.shape[1:], F32)
        for k in range(d_out):
            hk = base + step * F32(k)
            t = hk - lo
            hk = lo + np.where(t < 0, F32(0), t)
            t = hk - hi
            hk = hi + np.where(t > 0, F32(0), t)
            out[:, k] = hk
    return out


def log_clamped32(prob):
    """fp32 ln(max(p, 1e-40f)) from a correctly rounded float64 log (the device logf may differ from it by an ulp)."""
    return np.log(np.maximum(np.asarray(prob, F32), PCLAMP).astype(F64)).astype(F32)


def laplace_fit_given_log(lnp, depth, hypos):
    """hypos_fit_kernel mode 2 given y = ln p (fp32): x = |hyp - depth|; s = 1 / |cascade(x*y) / cascade(x*x)|."""
    lnp = np.asarray(lnp, F32)
    with np.errstate(all="ignore"):
        x = np.abs(_hyp_full(hypos, lnp.shape) - np.asarray(depth, F32)[:, None])
        return F32(1) / np.abs(cascade_sum(x * lnp, 1) / cascade_sum(x * x, 1))


# --------------------------------------------------------------------------- float64 references (from the same fp32 inputs)
def depth_regress64(prob, hypos):
    """-> (sum_d p_d h_d, sum_d |p_d h_d|) in float64."""
    t = np.asarray(prob, F32).astype(F64) * np.asarray(hypos, F32).astype(F64)
    return t.sum(1), np.abs(t).sum(1)


def expectation64(prob):
    p = np.asarray(prob, F32).astype(F64)
    return (p * np.arange(p.shape[1], dtype=F64).reshape(1, -1, 1, 1)).sum(1)


def log_clamped64(prob):
    return np.log(np.maximum(np.asarray(prob, F32), PCLAMP).astype(F64))


def laplace_fit64(prob, depth, hypos):
    """-> (s, sxx) in float64; s is NaN where sxx == 0 (0/0)."""
    y = log_clamped64(prob)
    x = np.abs(np.asarray(hypos, F32).astype(F64) - np.asarray(depth, F32).astype(F64)[:, None])
    sxy, sxx = (x * y).sum(1), (x * x).sum(1)
    with np.errstate(all="ignore"):
        return 1.0 / np.abs(sxy / sxx), sxx


def gauss1_fit64(prob, row):
    """Given the fit row [B,D] -> (|acc|, sum_d |row_d ln p_d|) in float64, acc = sum_d row_d ln p_d; s = 1/|acc|."""
    y = log_clamped64(prob)
    t = np.asarray(row, F32).astype(F64)[:, :, None, None] * y
    return np.abs(t.sum(1)), np.abs(t).sum(1)


def up2_bilinear64(m):
    m = np.asarray(m, F32).astype(F64)
    _, h, w = m.shape
    y0, y1, ly0, ly1 = up2_coord(2 * h, h)
    x0, x1, lx0, lx1 = up2_coord(2 * w, w)
    ly0, ly1, lx0, lx1 = (a.astype(F64) for a in (ly0, ly1, lx0, lx1))
    top = m[:, y0][:, :, x0] * lx0 + m[:, y0][:, :, x1] * lx1
    bot = m[:, y1][:, :, x0] * lx0 + m[:, y1][:, :, x1] * lx1
    return top * ly0[None, :, None] + bot * ly1[None, :, None]


def hypos_from_fit64(mode, s, depth, rng, log_thresh, d_out, upsample=True):
    """float64 reference of step 2 for FINITE s and depth (the fp32 range and fp32 log_thresh are the inputs)."""
    rng = np.asarray(rng, F32).astype(F64)
    B = rng.shape[0]
    lt = float(F32(log_thresh))
    s, depth = np.asarray(s, F32), np.asarray(depth, F32)
    sv, dv = (up2_bilinear64(s), up2_bilinear64(depth)) if upsample else (s.astype(F64), depth.astype(F64))
    with np.errstate(all="ignore"):
        res = np.sqrt(-sv * lt) if mode == 1 else np.abs(sv * lt)
    lo, hi = rng[:, 0].reshape(B, 1, 1), rng[:, 1].reshape(B, 1, 1)
    res = np.minimum(np.clip(res, 1e-6, (rng[:, 1].max() - rng[:, 0].min()) / 2), (hi - lo) * float(F32(0.2)))
    k = np.arange(d_out, dtype=F64).reshape(1, d_out, 1, 1)
    hyp = (dv - 0.5 * res)[:, None] + (res / (d_out - 1))[:, None] * k
    return np.clip(hyp, lo[:, None], hi[:, None])


# --------------------------------------------------------------------------- seeded inputs
def depth_ranges(B):
    """Per-item depth ranges that differ in offset and scale: [425, 935], [300, 900], [0.5, 1.2], ...  -> [B,2] fp32."""
    return RANGES[np.arange(B) % len(RANGES)].copy()


def make_hypos(B, D, h, w, per_pixel, seed):
    """Hypotheses sorted along D inside each item's range; the first and last plane of the per-plane form sit on lo and hi."""
    rs = np.random.RandomState(seed + 7919)
    r = depth_ranges(B)
    lo, hi = r[:, 0].reshape(B, 1, 1, 1), r[:, 1].reshape(B, 1, 1, 1)
    u = np.sort(rs.uniform(0, 1, (B, D, h, w) if per_pixel else (B, D, 1, 1)), axis=1)
    if not per_pixel and D >= 2:
        u[:, 0], u[:, -1] = 0.0, 1.0
    return np.clip(f32(lo + u * (hi - lo)), lo, hi)


def make_probs(B, D, h, w, seed):
    """-> (prob [B,D,h,w] fp32, kind [B,h,w] index into KINDS, plane [B,h,w]: the hot plane of a one-hot pixel, else -1).
    Every pixel draws one of: softmax of randn*3; a one-hot at plane 0, D-1, D-2 or the middle; softmax of randn*40, whose fp32
    result holds exact zeros and denormals; uniform 1/D; a randn*3 softmax with 1e-42 and 1e-39 (both below FLT_MIN) planted.
    The kinds are dealt round-robin over a permutation of the pixels, so a map of 12 or more pixels holds every kind."""
    rs = np.random.RandomState(seed)
    n = B * h * w
    kind = (rs.permutation(n) % len(KINDS)).reshape(B, h, w)
    names = np.array(KINDS)[kind]
    z = rs.standard_normal((B, D, h, w)).astype(F32)
    z *= np.where(names == "softmax40", F32(40), F32(3))[:, None]
    z -= z.max(1, keepdims=True)
    np.exp(z, out=z)
    prob = z / z.sum(1, keepdims=True)
    plane = np.full((B, h, w), -1, np.int64)
    for name, k in (("onehot_first", 0), ("onehot_last", D - 1), ("onehot_last2", max(D - 2, 0)), ("onehot_mid", D // 2)):
        plane[names == name] = k
    hot = plane >= 0
    onehot = (np.arange(D).reshape(1, D, 1, 1) == plane[:, None]).astype(F32)
    prob = np.where(hot[:, None], onehot, prob)
    prob = np.where((names == "uniform")[:, None], F32(1) / F32(D), prob).astype(F32)
    # planted entries go to planes other than the largest one, so the distribution stays one (D = 1 has no such plane, D = 2 one)
    pl = names == "planted"
    am = prob.argmax(1)
    r1 = rs.randint(0, max(D - 1, 1), (B, h, w))
    r2 = (r1 + 1 + rs.randint(0, max(D - 2, 1), (B, h, w))) % max(D - 1, 1)
    ar = np.arange(D).reshape(1, D, 1, 1)
    if D >= 3:
        prob = np.where(pl[:, None] & (ar == ((am + 1 + r2) % D)[:, None]), F32(1e-39), prob)
    if D >= 2:
        prob = np.where(pl[:, None] & (ar == ((am + 1 + r1) % D)[:, None]), F32(1e-42), prob)
    return f32(prob), kind, plane


def make_fit_inputs(B, h, w, seed):
    """s and depth [B,h,w] for hypos_from_fit: s log-uniform over 1e-9 .. 1e6 (below the 1e-6 floor up to where both caps bind),
    depth mostly inside each item's range, a tenth below lo and a tenth above hi."""
    rs = np.random.RandomState(seed + 104729)
    r = depth_ranges(B)
    lo, hi = r[:, 0].reshape(B, 1, 1), r[:, 1].reshape(B, 1, 1)
    s = f32(10.0 ** rs.uniform(-9, 6, (B, h, w)))
    u = rs.uniform(-0.125, 1.125, (B, h, w))
    return s, f32(lo + u * (hi - lo))


def same_bits(a, b):
    """Element-wise: equal bit patterns, or both NaN (a NaN's payload is not part of the promise)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind != "f":
        return a == b
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))
