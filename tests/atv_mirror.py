"""The adaptive-thin-volume range ("atv" curve: atv_spread_kernel + atv_hypos_kernel of mdf-net_amd/csrc/regress.hip) in numpy.

spread64      e = scale * sqrt(sum_d p_d (x_d - depth)^2) in float64 from the fp32 inputs: the yardstick of the spread.
spread_bar    (D/2 + 4) * 2^-24 * e64.  For fp32 inputs taken as exact, in any summation order, with or without fma: a term
              p_d (x_d - depth)^2 carries at most 4 roundings (the difference, which is squared: 2; the square: 1; the product: 1),
              the sum of D non-negative terms at most D - 1 more, so the sum is off by at most (D + 3) * 2^-24 relative; the square
              root halves that, and the root and the scale add one rounding each: (D + 3)/2 + 2 <= D/2 + 4.  The bound is relative,
              so it needs every rounding to be relative: inputs are drawn so that the sum is 0 (then e is exactly 0) or >= 1e-30,
              far above where an fp32 sum rounds in the denormal range.
atv_hypos     the explicit-order fp32 mirror of atv_hypos_kernel, on heads_mirror.up2_bilinear: every operation of the reference's
              atv_hypos (depthhypos.py:239-253) rounded on its own, np.minimum handing on a NaN of either side as torch.min does.
slot_bar      (D/2 + 4) * 2^-24 * max e + 8 * 2^-24 * max |hyp|: every hypothesis is d2 + c e2 with |c| <= 1 (low = -e2: c runs from
              -1 to 1; low = -d2: hyp = (d2 + e2) i / (D_out - 1)), so it moves by at most the change in e; the second term covers the
              roundings of the bilinear blend (4) and of the four operations behind it.

Nothing here reads the reference tree or needs a GPU."""
import numpy as np

import heads_mirror as M

F32, F64, EPS = M.F32, M.F64, M.EPS


def spread64(prob, depth, hypos, scale):
    """-> (e64 [B,h,w], the float64 sum under the root)."""
    p = np.asarray(prob, F32).astype(F64)
    t = np.asarray(hypos, F32).astype(F64) - np.asarray(depth, F32).astype(F64)[:, None]
    s = (p * t * t).sum(1)
    return float(F32(scale)) * np.sqrt(s), s


def spread_bar(D, e64):
    return (D / 2 + 4) * EPS * np.asarray(e64, F64)


def in_scope(prob, depth, hypos):
    """Per pixel: the float64 sum is 0 or >= 1e-30 (what a test's drawn inputs must satisfy)."""
    s = spread64(prob, depth, hypos, 1.0)[1]
    return (s == 0) | (s >= 1e-30)


def check_spread(e, prob, depth, hypos, scale, what, drawn=True):
    """The bar at every pixel, exactly 0 where the float64 sum is 0 -> the largest error as a share of the bar.  drawn: the inputs
    are a test's own and must lie in the bound's scope; tensors a model produced (drawn=False) are held to the bar wherever they
    fall: the kernel sums p * 2^64, so its roundings stay relative below 1e-30 as well."""
    e = np.asarray(e)
    e64, s = spread64(prob, depth, hypos, scale)
    assert e.dtype == F32 and e.shape == e64.shape, (e.dtype, e.shape, e64.shape)
    if drawn:
        assert ((s == 0) | (s >= 1e-30)).all(), f"{what}: a sum inside (0, 1e-30) is outside the bound's scope"
    else:
        print(f"{what}: {int(((s > 0) & (s < 1e-30)).sum())} pixels with a sum inside (0, 1e-30)")
    assert (e[s == 0] == 0).all(), f"{what}: the spread of an exactly zero sum must be exactly 0"
    bar = spread_bar(np.asarray(prob).shape[1], e64)
    err = np.abs(e.astype(F64) - e64)
    pos = s > 0
    worst = float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
    print(f"{what}: max |e - e64| / ((D/2 + 4) 2^-24 e64) = {worst:.4f}  ({int(pos.sum())} pixels, {int((~pos).sum())} exact zeros)")
    assert (err <= bar).all(), f"{what}: {int((err > bar).sum())} pixels over the bar, worst {worst:.3f}"
    return worst


def atv_hypos(e, depth, d_out, upsample=True):
    """atv_hypos_kernel.  e, depth [B,h,w] -> [B,d_out,Ho,Wo] fp32."""
    e, depth = np.asarray(e, F32), np.asarray(depth, F32)
    with np.errstate(all="ignore"):
        e2, d2 = (M.up2_bilinear(e), M.up2_bilinear(depth)) if upsample else (e, depth)
        low = -np.minimum(d2, e2)
        step = (e2 - low) / F32(d_out - 1)
        base = d2 + low
        out = np.empty((e.shape[0], d_out) + e2.shape[1:], F32)
        for k in range(d_out):
            out[:, k] = (base + step * F32(k)) + F32(1e-12)
    return out


def slot_bar(D, e_max, hyp_max):
    return (D / 2 + 4) * EPS * float(e_max) + 8 * EPS * float(hyp_max)
