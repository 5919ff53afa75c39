"""Float64 references of the forward convolution family and the operand generators of its parity tests
(mdf-net_amd/csrc/conv3d.hip, conv3d_hw.hip, convtr3d.hip, conv_lds.hip, wino2d.hip, wino3d.hip, conv1x1.hip, conv_pair.hip, res_pair.hip,
refine_tail.hip).

Every reference restates the FORMULA of its operation as one tap loop over whole arrays in numpy float64 (`taps`): for every kernel tap a
strided slice of the zero-padded input times that tap's [Cin, Cout] matrix (a transposed layer scatters instead of gathering).  Nothing
walks a tile, a fragment or a lane's share.  tests/test_conv_mirror_cpu.py ties it to torch.nn.functional in float64 and to the network's
modules.  Arrays are channels-last as the kernels take them, [B, D, H, W, C]; a 2-D layer is the D = 1, kd = 1 case.

For every operation the reference gives `y64`, the result, and `A`, the same operation on absolute values (sum |x||w|): the scale every
rounding of a sum of products is relative to.

Epilogue (`epilogue`), in the order the sources state it (conv_lds.hip, the loop behind step_mfma; conv3d_common.h, scale_shift_relu and
add_res_store):  o = acc * alpha;  o = o + beta;  o = fmaxf(o, 0);  o = up + o (bilinear x2 of res_up: fp32 positions sy = (oh + .5) * .5
- .5 clamped at 0, weights ly1 = sy - y0, ly0 = 1 - ly1, ...; up = fma(w11, v11, fma(w10, v10, fma(w00, v00, w01 * v01))));
o = rr + o * res_scale.  A 3-D layer has no res_up and no res_scale: o = o + rr.  It is stated once, with `dtype` float64 (every operation
in double) or float32 (one rounding per operation; an fma is one rounding of the exact double product plus the addend).  PixelShuffle(2) is
a store order: GEMM row sub * Cq + oc of pixel (h, w) goes to channel oc of pixel (2h + sub / 2, 2w + sub % 2) (`shuffle2_store`).

fp32 yardstick (`chain32`): the serial fma chain of one output in canonical order (kd, kh, kw, cin), acc = fma(x, w, acc) from 0, then the
fp32 epilogue.  The fma is emulated as float32(double(acc) + double(x) * double(w)): the product of two fp32 numbers is exact in double, the
sum is rounded to 53 bits and then to 24.  That double rounding differs from a true fma only where the 53-bit sum lies within 2^-29 ulp32 of
a rounding boundary and moves a result by one ulp32 when it does; as a yardstick for distances of several ulp it is the same chain.
e_32 is this chain's distance from y64.  torch's fp32 convolution is not used anywhere.

Winograd restatement (`wino32`): F(2x2, 3x3) in fp32 with conv_pack.hip's G (pack_wino_elem: v += G[a][y] * G[b][x] * w in (y, x) order,
no contraction), the input transform B^T d B by fp32 additions, the serial fma chain over (kd, cin) in the transform domain and A^T M A by
fp32 additions.  Its only use is the CPU proof that a correct Winograd kernel can meet the bar, and that the bar catches a wrong one
(`faults`).

Exact generator (`exact_operands`).  x integers in [-4, 4] with about 30 % exact zeros, w in {-1, -1/2, 0, 1/2, 1}, alpha in {1/2, 1, 2,
-1}, beta a multiple of 1/4 in [-2, 2], res and res_up integers in [-4, 4], res_scale 1/2.  Then every product is a multiple of 1/2, every
partial sum in ANY order is a multiple of 1/2 of magnitude <= A, every Winograd intermediate (U = G g G^T: multiples of 1/8, |U| <= 9/4
per tap; V = B^T d B: integers, |V| <= 16) a multiple of 1/8 with partial sums of magnitude <= A_w = sum over (kd, cin) of max|U| max|V|,
and every epilogue value a multiple of 1/64 (alpha 1/2, bilinear weights in sixteenths, res_scale 1/2) bounded by a few times A.  All of
them are fp32 numbers as long as  max(A, A_w) / q < 2^24  with q the smallest unit (`exact_condition`), so ANY correct kernel, direct or
Winograd, split-K or not, owes y64 BIT FOR BIT.  `scale` multiplies x, beta, res and res_up by a power of two (2^100, 2^-130: the latter
puts every value and every intermediate in the denormal range, where the same integers live on the grid 2^-149: the condition is then
that the smallest unit times `scale` is >= 2^-149).

Random generator (`random_operands`), three classes: `normal` N(0,1); `relu` max(0, N(0,1)): non-negative, half exact zeros; `offset`
N(100,1).  Weights N(0,1) / sqrt(K); alpha U(0.5,1.5), beta U(-0.2,0.2), res N(0,1), res_scale 0.1: the existing suites' constants.

The bar on random operands is  e_hip <= 1.5 e_32 + t  in each of the project's three metrics (`metrics`): max = max|d| / max|ref|,
l2 = relative L2, perA = max |d| / A.  1.5 is the margin of DESIGN.md's aggregation parity sections; t = 0.

Nothing here needs a GPU or reads the reference tree."""
import functools

import numpy as np

U = 2.0 ** -24
MARGIN = 1.5
G = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=np.float32)      # conv_pack.hip
RES_SCALE_EXACT, RES_SCALE_RANDOM = 0.5, 0.1
CLASSES = ("normal", "relu", "offset")


def rng(*key):
    h = 17
    for v in key:
        h = (h * 1000003 + int(v)) % (2 ** 31 - 1)
    return np.random.RandomState(h)


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def out_extent(n, k, s, transposed=False):
    return s * n if transposed else (n + 2 * ((k - 1) // 2) - k) // s + 1


# --------------------------------------------------------------------------- the operation, in float64
def taps(x, w, stride=1, transposed=False, combine=None):
    """x [B,D,H,W,Ci], w [Co,Ci,kd,kh,kw] (transposed: [Ci,Co,3,3,3]), stride an int or (sd,sh,sw), padding (k-1)/2 (transposed:
    padding 1, output_padding s-1, so the output is s times the input).  combine(acc, xs, wt): how one tap's [.., Ci] slice and
    [Ci, Co] matrix enter the accumulator; the default is acc + xs @ wt in the arrays' own type."""
    sd, sh, sw = _triple(stride)
    b, d, h, wd, ci = x.shape
    if transposed:
        assert w.shape[0] == ci and tuple(w.shape[2:]) == (3, 3, 3)
        co, (kd, kh, kw) = w.shape[1], (3, 3, 3)
    else:
        assert w.shape[1] == ci
        co, (kd, kh, kw) = w.shape[0], w.shape[2:]
    combine = combine or (lambda acc, xs, wt: acc + xs @ wt)
    if transposed:
        full = np.zeros((b, sd * (d - 1) + 3, sh * (h - 1) + 3, sw * (wd - 1) + 3, co), dtype=x.dtype)
        for a in range(kd):
            for i in range(kh):
                for j in range(kw):
                    view = full[:, a:a + sd * d:sd, i:i + sh * h:sh, j:j + sw * wd:sw]
                    view[...] = combine(view, x, w[:, :, a, i, j])
        return np.ascontiguousarray(full[:, 1:1 + sd * d, 1:1 + sh * h, 1:1 + sw * wd])
    pd, ph, pw = (kd - 1) // 2, (kh - 1) // 2, (kw - 1) // 2
    do, ho, wo = out_extent(d, kd, sd), out_extent(h, kh, sh), out_extent(wd, kw, sw)
    xp = np.zeros((b, d + 2 * pd, h + 2 * ph, wd + 2 * pw, ci), dtype=x.dtype)
    xp[:, pd:pd + d, ph:ph + h, pw:pw + wd] = x
    acc = np.zeros((b, do, ho, wo, co), dtype=x.dtype)
    for a in range(kd):
        for i in range(kh):
            for j in range(kw):
                xs = xp[:, a:a + sd * (do - 1) + 1:sd, i:i + sh * (ho - 1) + 1:sh, j:j + sw * (wo - 1) + 1:sw]
                acc = combine(acc, xs, w[:, :, a, i, j].T)
    return acc


def conv_ref(x, w, stride=1, transposed=False, want_a=True):
    """(y64, A) of a 3-D layer from its fp32 operands (A is None where it is not wanted)."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return taps(x64, w64, stride, transposed), (taps(np.abs(x64), np.abs(w64), stride, transposed) if want_a else None)


def as3d(x, w, stride):
    """A 2-D layer's operands x [B,H,W,Ci], w [Co,Ci,k,k] as the D = 1 case."""
    return x[:, None], w[:, :, None], (1, stride, stride)


def conv2d_ref(x, w, stride=1):
    y, a = conv_ref(*as3d(np.asarray(x), np.asarray(w), stride))
    return y[:, 0], a[:, 0]


def _fma32(acc, a, b):
    """float32(acc + a * b) with the product exact (module docstring: the double rounding)."""
    return (acc.astype(np.float64) + np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).astype(np.float32)


def chain32(x, w, stride=1, transposed=False):
    """The serial fp32 fma chain per output in canonical order (kd, kh, kw, cin)."""
    def combine(acc, xs, wt):
        acc = np.array(acc, dtype=np.float32)
        for c in range(xs.shape[-1]):
            acc = _fma32(acc, xs[..., c, None], wt[c])
        return acc
    return taps(np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32), stride, transposed, combine)


# --------------------------------------------------------------------------- the epilogue, once
def bilinear_up2(top, ho, wo, dtype):
    """F.interpolate(top, scale_factor=2, mode='bilinear', align_corners=False) of a channels-last [B,Hh,Wh,C] map at the [ho, wo]
    grid, with the kernel's fp32 positions and its operation order; dtype float32: one rounding per operation."""
    hh, wh = ho >> 1, wo >> 1
    f = np.float32

    def pos(n, nh):
        s = (np.arange(n, dtype=f) + f(0.5)) * f(0.5) - f(0.5)
        s = np.where(s < 0, f(0), s).astype(f)
        i0 = s.astype(np.int64)
        i1 = i0 + (i0 < nh - 1)
        l1 = (s - i0.astype(f)).astype(f)
        return i0, i1, (f(1) - l1).astype(f), l1
    y0, y1, ly0, ly1 = pos(ho, hh)
    x0, x1, lx0, lx1 = pos(wo, wh)
    w00, w01, w10, w11 = (np.multiply.outer(a, b).astype(f)[None, :, :, None] for a, b in ((ly0, lx0), (ly0, lx1), (ly1, lx0), (ly1, lx1)))
    t = np.asarray(top)
    v00, v01, v10, v11 = (t[:, yy][:, :, xx] for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    if dtype == np.float32:
        up = (w01 * v01.astype(f)).astype(f)
        for wk, vk in ((w00, v00), (w10, v10), (w11, v11)):
            up = _fma32(up, wk, vk)
        return up
    d = np.float64
    return w11.astype(d) * v11.astype(d) + (w10.astype(d) * v10.astype(d) + (w00.astype(d) * v00.astype(d) + w01.astype(d) * v01.astype(d)))


def shuffle2_store(y):
    """[B,H,W,Cout] GEMM rows -> [B,2H,2W,Cout/4]: row sub * Cq + oc of pixel (h, w) is channel oc of pixel (2h + sub / 2, 2w + sub % 2)."""
    b, h, w, c = y.shape
    cq = c // 4
    return np.ascontiguousarray(y.reshape(b, h, w, 2, 2, cq).transpose(0, 1, 3, 2, 4, 5).reshape(b, 2 * h, 2 * w, cq))


def epilogue(acc, alpha=None, beta=None, relu=False, res=None, res_scale=None, res_up=None, dtype=np.float64, fuse_mul_add=False,
             scale_res_instead=False):
    """The stored value from the accumulator.  res_scale None: the 3-D form o + res; a number: the 2-D form res + o * res_scale.
    fuse_mul_add / scale_res_instead are deliberate errors for the CPU test (acc * alpha + beta as one fma; res * res_scale + o)."""
    o = np.asarray(acc).astype(dtype)
    if alpha is not None:
        al, be = np.asarray(alpha).astype(dtype), np.asarray(beta).astype(dtype)
        if fuse_mul_add:
            o = (o.astype(np.float64) * al.astype(np.float64) + be.astype(np.float64)).astype(dtype)
        else:
            o = (o * al).astype(dtype)
            o = (o + be).astype(dtype)
    if relu:
        o = np.fmax(o, dtype(0))                                     # fmaxf: a NaN becomes 0
    if res_up is not None:
        assert o.ndim == 4
        o = (bilinear_up2(res_up, o.shape[1], o.shape[2], dtype) + o).astype(dtype)
    if res is not None:
        rr = np.asarray(res).astype(dtype)
        if res_scale is None:
            o = (o + rr).astype(dtype)
        elif scale_res_instead:
            o = ((rr * dtype(res_scale)).astype(dtype) + o).astype(dtype)
        else:
            o = (rr + (o * dtype(res_scale)).astype(dtype)).astype(dtype)
    return o


# --------------------------------------------------------------------------- Winograd F(2x2, 3x3) in fp32
def wino_weights(w, g=G):
    """U[kd, a, b, co, ci] = (G g_kd G^T)[a, b] in pack_wino_elem's operation order."""
    f = np.float32
    w = np.asarray(w, dtype=f)
    co, ci, kd = w.shape[:3]
    u = np.zeros((kd, 4, 4, co, ci), dtype=f)
    for a in range(4):
        for b in range(4):
            v = np.zeros((kd, co, ci), dtype=f)
            for y in range(3):
                for x in range(3):
                    v = (v + (f(g[a][y] * g[b][x]) * w[:, :, :, y, x].transpose(2, 0, 1)).astype(f)).astype(f)
            u[:, a, b] = v
    return u


def wino32(x, w, g=G, faults=()):
    """Stride-1 3x3 (kd = 1 or 3) layer x [B,D,H,W,Ci], w [Co,Ci,kd,3,3] -> fp32 [B,D,H,W,Co].
    faults: "right_halo" (the column past the volume reads the next row's first pixel instead of zero), "depth_halo" (the plane past
    the volume reads the next batch item's first plane)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    b, d, h, wd, ci = x.shape
    u = wino_weights(w, g)
    kd, co = u.shape[0], u.shape[3]
    pd = (kd - 1) // 2
    th, tw = (h + 1) // 2, (wd + 1) // 2
    xp = np.zeros((b, d + 2 * pd, 2 * th + 2, 2 * tw + 2, ci), dtype=f)
    xp[:, pd:pd + d, 1:1 + h, 1:1 + wd] = x
    if "right_halo" in faults:
        xp[:, pd:pd + d, 1:h, 1 + wd] = x[:, :, 1:, 0]
    if "depth_halo" in faults and pd and b > 1:
        xp[:-1, pd + d, 1:1 + h, 1:1 + wd] = x[1:, 0]
    dd = np.stack([np.stack([xp[:, :, r:r + 2 * th:2, c:c + 2 * tw:2] for c in range(4)], axis=4) for r in range(4)], axis=4)   # [B,Dp,th,tw,4,4,Ci]

    def bt(t, ax):
        t0, t1, t2, t3 = (np.take(t, k, axis=ax) for k in range(4))
        return np.stack([t0 - t2, t1 + t2, t2 - t1, t1 - t3], axis=ax).astype(f)
    v = bt(bt(dd, 4), 5)
    m = np.zeros((b, d, th, tw, 4, 4, co), dtype=f)
    for a in range(kd):
        for c in range(ci):
            m = _fma32(m, v[:, a:a + d, ..., c, None], u[a, :, :, :, c])

    def at(t, ax):
        t0, t1, t2, t3 = (np.take(t, k, axis=ax) for k in range(4))
        return np.stack([((t0 + t1).astype(f) + t2).astype(f), ((t1 - t2).astype(f) - t3).astype(f)], axis=ax)
    y = at(at(m, 4), 5)                                              # [B,D,th,tw,2,2,Co]
    y = y.transpose(0, 1, 2, 4, 3, 5, 6).reshape(b, d, 2 * th, 2 * tw, co)
    return np.ascontiguousarray(y[:, :, :h, :wd])


def wino_bounds(x, w):
    """A_w: the largest magnitude a partial sum of the transform-domain chain can reach, sum over (kd, cin) of max|U| max|V|."""
    u = np.abs(wino_weights(np.abs(np.asarray(w, dtype=np.float32)))).max()
    ci, kd = np.asarray(w).shape[1], np.asarray(w).shape[2]
    return float(u) * 4.0 * float(np.abs(x).max()) * ci * kd          # |V| <= 4 max|x|: two rows of B^T with two entries each


# --------------------------------------------------------------------------- operand generators
def _shapes(xshape, wshape, stride, transposed):
    b, d, h, w, _ = xshape
    co = wshape[1] if transposed else wshape[0]
    kd, kh, kw = wshape[2:]
    sd, sh, sw = _triple(stride)
    return (b, out_extent(d, kd, sd, transposed), out_extent(h, kh, sh, transposed), out_extent(w, kw, sw, transposed), co)


def exact_operands(rs, xshape, wshape, stride=1, transposed=False, scale=1.0):
    """{x, w, alpha, beta, res, res_up, res_scale} fp32 (module docstring); res_up is [B, max(Ho/2,1), max(Wo/2,1), Co] of a D = 1 layer."""
    f = np.float32
    x = rs.randint(-4, 5, xshape).astype(f) * (rs.uniform(size=xshape) >= 0.21)
    w = rs.choice(np.array([-1, -0.5, 0, 0.5, 1], dtype=f), size=wshape)
    osh = _shapes(xshape, wshape, stride, transposed)
    co = osh[-1]
    ops = {"x": x.astype(f) * f(scale), "w": w.astype(f), "alpha": rs.choice(np.array([0.5, 1, 2, -1], dtype=f), size=co),
           "beta": (rs.randint(-8, 9, co) * 0.25).astype(f) * f(scale), "res": rs.randint(-4, 5, osh).astype(f) * f(scale),
           "res_up": rs.randint(-4, 5, (osh[0], max(osh[2] // 2, 1), max(osh[3] // 2, 1), co)).astype(f) * f(scale),
           "res_scale": RES_SCALE_EXACT}
    return ops


def random_operands(rs, cls, xshape, wshape, stride=1, transposed=False):
    f = np.float32
    x = rs.standard_normal(xshape)
    x = {"normal": x, "relu": np.maximum(x, 0), "offset": x + 100.0}[cls]
    ci = wshape[0] if transposed else wshape[1]
    w = rs.standard_normal(wshape) / np.sqrt(float(np.prod(wshape[2:])) * ci)
    osh = _shapes(xshape, wshape, stride, transposed)
    co = osh[-1]
    return {"x": x.astype(f), "w": w.astype(f), "alpha": rs.uniform(0.5, 1.5, co).astype(f), "beta": rs.uniform(-0.2, 0.2, co).astype(f),
            "res": rs.standard_normal(osh).astype(f), "res_up": rs.standard_normal((osh[0], max(osh[2] // 2, 1), max(osh[3] // 2, 1), co)).astype(f),
            "res_scale": RES_SCALE_RANDOM}


def exact_condition(a_max, a_w=0.0, unit=2.0 ** -6, scale=1.0):
    """max(A, A_w) / q < 2^24 on the unit grid q, and q * scale still an fp32 (denormal) number."""
    return max(a_max, a_w) / unit < 2.0 ** 24 and unit * scale >= 2.0 ** -149


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


# --------------------------------------------------------------------------- metrics and the bar
def metrics(got, ref, a):
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    a = np.broadcast_to(a, d.shape)
    live = a > 0
    assert not d[~live].any(), "a difference where the sum of magnitudes is zero"
    return {"max": float(d.max() / np.abs(ref).max()), "l2": float(np.sqrt((d * d).sum() / (ref * ref).sum())),
            "perA": float((d[live] / a[live]).max()) if live.any() else 0.0}


def bar_ratios(e_got, e_32, t=0.0):
    """e_got / (1.5 e_32 + t) per metric: at most 1 passes."""
    return {k: (e_got[k] / (MARGIN * e_32[k] + t) if MARGIN * e_32[k] + t > 0 else (0.0 if e_got[k] == 0 else float("inf"))) for k in e_got}


def epilogue_scale(a, alpha=None, beta=None, res=None, res_scale=None, res_up=None):
    """A of the stored value: the epilogue of magnitudes."""
    o = np.asarray(a, dtype=np.float64)
    if alpha is not None:
        o = o * np.abs(alpha).astype(np.float64) + np.abs(beta).astype(np.float64)
    if res_up is not None:
        o = bilinear_up2(np.abs(res_up), o.shape[1], o.shape[2], np.float64) + o
    if res is not None:
        o = np.abs(res).astype(np.float64) + o * (1.0 if res_scale is None else float(np.float32(res_scale)))
    return o


# --------------------------------------------------------------------------- the fused operations
def pair_planar_ref(x, w1, a1, b1, w2, a2, b2, dtype=np.float64):
    """relu(bn(conv3x3(relu(bn(conv3x3(x)))))), x planar [N,3,H,W] -> ([N,H,W,8], A, A of the intermediate map).  dtype float32: both
    layers' fp32 chains and fp32 epilogues, the intermediate map an fp32 tensor as the kernel keeps it; float64: no rounding anywhere."""
    xl = np.ascontiguousarray(np.asarray(x).transpose(0, 2, 3, 1))
    conv = (lambda t, w: chain32(*as3d(t, w, 1))[:, 0]) if dtype == np.float32 else (lambda t, w: conv2d_ref(t, w)[0])
    mid = epilogue(conv(xl, w1), a1, b1, True, dtype=dtype)
    amid = epilogue_scale(conv2d_ref(np.abs(xl), np.abs(w1))[0], a1, b1)
    y = epilogue(conv(mid, w2), a2, b2, True, dtype=dtype)
    return y, epilogue_scale(conv2d_ref(np.abs(mid), np.abs(w2))[0], a2, b2), amid


def res_pair_ref(x, wa, wb, scale, dtype=np.float64):
    """x + scale * conv3x3(relu(conv3x3(x))), x [N,H,W,8]."""
    conv = (lambda t, w: chain32(*as3d(t, w, 1))[:, 0]) if dtype == np.float32 else (lambda t, w: conv2d_ref(t, w)[0])
    one, zero = np.ones(8, np.float32), np.zeros(8, np.float32)
    mid = epilogue(conv(x, wa), one, zero, True, dtype=dtype)
    amid = conv2d_ref(np.abs(x), np.abs(wa))[0]
    y = epilogue(conv(mid, wb), one, zero, False, res=x, res_scale=scale, dtype=dtype)
    return y, np.abs(x) + float(np.float32(scale)) * conv2d_ref(np.abs(mid), np.abs(wb))[0], amid


def refine_tail_ref(x, w1, w2, lo=None, span=None, dtype=np.float64):
    """[lo +] Conv2d(8,1,k3)(PixelShuffle(2)(Conv2d(8,32,k3)(x))) [* span]; w1 in torch's channel order [32,8,3,3] (the kernel takes
    shuffle2_rows of it: channel oc * 4 + sub is GEMM row sub * 8 + oc).  -> ([B,2H,2W], A, A of the shuffled map).  dtype float32: both
    fp32 chains, the shuffled map an fp32 tensor, then fmul and fadd."""
    w1r = np.asarray(w1).reshape(8, 4, 8, 3, 3).transpose(1, 0, 2, 3, 4).reshape(32, 8, 3, 3)
    conv = (lambda t, w: chain32(*as3d(t, w, 1))[:, 0]) if dtype == np.float32 else (lambda t, w: conv2d_ref(t, w)[0])
    mid, amid = shuffle2_store(conv(x, w1r)), shuffle2_store(conv2d_ref(x, w1r)[1])
    y, a = conv(mid, w2)[..., 0], conv2d_ref(mid, w2)[1][..., 0]
    if lo is not None:
        sp, l = np.asarray(span).astype(dtype)[:, None, None], np.asarray(lo).astype(dtype)[:, None, None]
        y, a = (l + (y * sp).astype(dtype)).astype(dtype), np.abs(l).astype(np.float64) + a * np.abs(sp).astype(np.float64)
    return y, a, amid


def refine_head_ref(depth, lo, span, w, dtype=np.float64):
    """conv0((depth - lo) / span), depth [B,H,W] -> ([B,H,W,8], A); dtype float32: sub, divide, then the fp32 chain."""
    d = np.asarray(depth).astype(dtype)
    if lo is not None:
        d = ((d - np.asarray(lo).astype(dtype)[:, None, None]).astype(dtype) / np.asarray(span).astype(dtype)[:, None, None]).astype(dtype)
    if dtype == np.float32:
        return chain32(*as3d(d[..., None], w, 1))[:, 0], None
    return conv2d_ref(d[..., None], w)


def heads_ref(x, heads, res_ups, dtype=np.float64):
    """conv1x1_heads: per head (w [Co,Ci,1,1], bias or None) over one NHWC input, + bilinear x2 of res_up.  -> (outputs, their A)."""
    out, scales = [], []
    for (w, bias), ru in zip(heads, res_ups):
        acc = chain32(*as3d(x, w, 1))[:, 0] if dtype == np.float32 else conv2d_ref(x, w)[0]
        co = w.shape[0]
        al, be = np.ones(co, np.float32), (np.zeros(co, np.float32) if bias is None else bias)
        out.append(epilogue(acc, al, be, False, res_up=ru, dtype=dtype))
        scales.append(epilogue_scale(conv2d_ref(x, w)[1], al, be, res_up=ru))
    return out, scales


# --------------------------------------------------------------------------- non-finite locality: who may see a planted value
def plant_places(shape, cin):
    """(b, d, h, w, c) of the four plants in a [B,D,H,W] volume (2-D: D = 1): the volume's corner; the last live column of the ragged
    last tile (the last voxel); the first column of the next tile (column 32, the Winograd tiles' width, else 16, the MFMA column
    count, else the middle, where the row is no longer than that); the last channel of a voxel in the middle."""
    b, d, h, w = shape
    col = 32 if 32 < w - 1 else (16 if 16 < w - 1 else w // 2)
    return [(0, 0, 0, 0, 0), (b - 1, d - 1, h - 1, w - 1, 1), (0, d // 2, h // 2, col, 2), (b - 1, d // 2, h // 2, w // 2, cin - 1)]


def _tile_rows(r, n):
    """Output rows of the F(2x2,3x3) tiles whose 4-row patch (rows 2i - 1 .. 2i + 2) holds input row r."""
    rows = np.zeros(n, dtype=bool)
    for i in range((n + 1) // 2):
        if 2 * i - 1 <= r <= 2 * i + 2:
            rows[2 * i:2 * i + 2] = True
    return rows


def receptive_mask(kind, place, xshape, wshape, stride=1, transposed=False):
    """bool [B,Do,Ho,Wo,1]: the outputs that may change when x[place] does.  Everything else owes the clean run bit for bit.
      direct   the outputs whose taps reach the voxel (the tap loop over an indicator).  The direct 3-D kernels load an out-of-range tap
               from the voxel's OWN position and zero it by a multiply (conv3d.hip, load_tap): that makes NaN of an Inf there, in
               outputs that hold the voxel anyway -- the mask is the same, only the NaN set grows (inf * 0).
      tr8      a transposed layer with 8 output channels: along w, input i' + 1 (offset +1) feeds the odd output column only; the rows of
               the even column in that tap slot are structural zeros of the packed weights, and the kernels skip them only as whole
               16-row MFMA tiles (conv3d.hip mul_tap, convtr3d.hip, conv3d_hw.hip).  With 8 output channels both columns share one tile,
               so 0 * NaN reaches output column 2w - 2, over the field's own depth and row range.  Documented here as the kernels'
               behaviour with non-finite inputs; finite inputs add exact zeros.
      wphase   the w-phase forms (conv_lds.hip Cfg::RW = 2, and both layers of conv_pair_kernel and res_pair_kernel): an MFMA column is two
               neighbouring output pixels (2j, 2j + 1) that share four taps along w, input columns 2j - 1 .. 2j + 2; GEMM row = phase * Cout
               + cout, and the rows of phase 0 in the fourth tap and of phase 1 in the first are structural zeros of the packed weights.
               0 * NaN from input column 2j + 2 therefore reaches pixel 2j, and from column 2j - 1 pixel 2j + 1: two columns from the voxel,
               on the side the pair alignment decides (res_pair_kernel's intermediate pairs start one pixel left of its strips).  The mask
               is the field widened to columns w - 2 .. w + 2, over its own depth and row range.
      wino     F(2x2,3x3) along h and w: the 2x2 tiles whose 4x4 patch holds the voxel; depth as direct.
      winodp   the depth-pair forms: the tile rule along the depth too (output planes 2k, 2k + 1 read input planes 2k - 1 .. 2k + 2).
      s2d      a 5x5 stride-2 layer as a 3x3 Winograd layer over the four parity images: the tile rule at (h / 2, w / 2).
    wino2d.hip's kept padding steps of 32 -> 64 (its header, W2Live PAD) multiply zero fragments with the V of the SAME tile: they can
    add NaNs inside the tile mask only, so that form needs no other mask."""
    ind = np.zeros(tuple(xshape[:-1]) + (1,))
    ind[tuple(place[:-1]) + (0,)] = 1.0
    ones = np.ones((1, 1) + tuple(wshape[2:]))
    field = taps(ind, ones, stride, transposed) > 0
    b, d, h, w = place[:4]
    if kind == "direct":
        return field
    if kind == "wphase":
        return taps(ind, np.ones((1, 1) + tuple(wshape[2:4]) + (5,)), stride) > 0
    if kind == "tr8":
        assert transposed
        leak = np.zeros_like(field)
        if w >= 1:
            leak[:, :, :, 2 * w - 2] = field[:, :, :, 2 * w - 1] | field[:, :, :, 2 * w]
        return field | leak
    do, ho, wo = field.shape[1:4]
    m = np.zeros_like(field)
    if kind == "s2d":
        rows, cols, planes = _tile_rows(h // 2, ho), _tile_rows(w // 2, wo), np.ones(do, dtype=bool)
    else:
        rows, cols = _tile_rows(h, ho), _tile_rows(w, wo)
        planes = _tile_rows(d, do) if kind == "winodp" else field[b, :, :, :, 0].any(axis=(1, 2))
    m[b] = (planes[:, None, None] & rows[None, :, None] & cols[None, None, :])[..., None]
    assert not (field & ~m).any()
    return m


# --------------------------------------------------------------------------- the case table
FUSED_SHAPES = [(1, 1, 70), (2, 64, 1), (3, 2, 2), (2, 13, 37), (1, 65, 63), (2, 64, 62)]


@functools.lru_cache(maxsize=None)
def table():
    """Every case of the GPU suite by name -> (family, key).  The conv_lds and conv3d tables are the digest suites' own, imported."""
    import test_conv3d_digests_gpu as T
    import test_conv_lds_routes_gpu as R
    import test_regular_stride_gpu as H
    import test_wino3d_strip_gpu as W
    out = {}
    for setting in R.SETTINGS:
        for name, kind, args, env in R.cases(setting):
            out[f"lds {setting}: {name}"] = ("lds", (setting, kind, args, tuple(sorted(env.items()))))
    for name, (fn, args) in T.CASES.items():
        out[f"digest {name}"] = ("digest", (fn.__name__, args))
    for cin, cout, tr in H.PAIRS:
        for shape in H.SHAPES:
            for route in (None, "1", "2", "3"):
                for kdskip in (("1", "0") if shape[1] <= 3 else ("1",)):
                    out[f"hw {cin}->{cout} {'up' if tr else 'down'} {shape} route {route} kdskip{kdskip}"] = ("hw", (cin, cout, tr, shape, route, kdskip))
    for cin, cout in ((32, 16), (16, 16)):
        for shape in W.SHAPES:
            for strip in ("default", "0"):
                out[f"strip {cin}->{cout} {shape} strip {strip}"] = ("strip", (cin, cout, shape, strip))
    for shape in FUSED_SHAPES:
        for valu in ("1", "0"):
            out[f"fused pair {shape} valu{valu}"] = ("pair", (shape, valu))
        for fam in ("res_pair", "refine_tail", "refine_head", "heads"):
            out[f"fused {fam} {shape}"] = (fam, (shape,))
    return out
