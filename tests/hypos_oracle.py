"""Yardsticks of the gauss0 / per-pixel gauss1 curve fits (hypos_fit modes 3 and 4, mdf-net_amd/csrc/regress.hip), in numpy.

The reference's fp32 arithmetic for these fits is poor (gauss1 inverts a 3x3 normal matrix of uncentred x^2, x, 1 with x near 600 and a
spread of millimetres: its own fp32 is noise), so the kernels are held to what the reference's code gives in float64, not to its fp32
bits.  Three things live here:

  * gauss0_fit64 / gauss1_fit64: the centred least-squares fits in float64, from the same fp32 inputs, with the rounding norm N;
  * gauss0_fit32 / gauss1_fit32: fp32 mirrors that execute the kernels' operations in the kernels' order (numpy float32 arithmetic is
    IEEE and keeps denormals; the logarithm is the correctly rounded one, the device logf may differ from it by an ulp);
  * K(mode, D): the number of roundings the bound allows, derived below from that operation order.

The bound:  | 1/s - |b0_64| |  <=  K(D) * 2^-24 * N,   N = sum_d w_d |z_d|,  z_d = ln max(p_d, 1e-40f),
  gauss0:  w_d = (|u_d| + |u_mean|) / sum (u - u_mean)^2,                  u_d = (x_d - depth)^2
  gauss1:  w_d = (t_d^2 + |alpha t_d| + |beta|) / (sigma^2 * sum q^2),      t_d = (x_d - x_mean) / sigma,  q_d = t_d^2 - alpha t_d - beta
(N does not change when t is rescaled, so it is the same for sigma = max |x - x_mean| and for the kernel's power of two.)

Sums.  Every sum of the kernels runs in four interleaved accumulators, a[d & 3] += term_d (an fma where the term is a product),
combined as (a0 + a1) + (a2 + a3): a chain of ceil(D/4) roundings and two more for the combination, D when that is fewer
(accumulators that never received a term add an exact zero):   S(D) = min(D, ceil(D/4) + 2).

K, mode 3 (gauss0), in units of 2^-24 * N, to first order:
  u_d = (x_d - depth)^2            one subtraction, doubled by the square, and the product: 3 |u_d|
  u_mean                           plain mean, then corrected by the mean of the residuals u_d - mean: what is left is the rounding of
                                   the last addition, 1 |u_mean|, on top of the 3 it inherits from the u_d
  c_d = u_d - u_mean               3 |u_d| + 4 |u_mean| + 1 |c_d| <= 5 (|u_d| + |u_mean|)
  numerator sum c_d z_d            5 from c_d, 2 for logf (one ulp = 2 * 2^-24), S(D) for the sum:              7 + S(D)
  denominator sum c_d^2            an error of u_mean is common to all c_d and drops out (sum c = 0); the others enter twice,
                                   2 * (3 + 1), and the sum adds S(D):                                            8 + S(D)
  s = |den / num|                  one division; the test inverts s in float64:                                   1
                                                                                                     K3(D) = 2 S(D) + 16
K, mode 4 (gauss1):
  t_d = (x_d - x_mean) * 2^-k      an error of x_mean is a common shift, under which b0 does not change; the subtraction rounds
                                   once, the scaling by a power of two is exact:                                  1
  t_d^2 (kept for the moments)     doubles it and rounds:                                                         3
  sum t^2, sum t^3                 S(D)
  alpha, beta                      2x2 solve: a product, an fma, the determinant's product and fma, a division:  5
  q_d = fma(t_d, t_d - alpha, -beta)   a subtraction and an fma:                                                  2
  numerator sum q_d z_d            2 for logf, S(D) for the sum:                                                  2 + S(D)
  s = |ldexp(den / num, 2k)|       one division:                                                                  1
  the longest chain to the result (t_d^2 -> moments -> beta -> q_d -> numerator -> s):               K4(D) = 2 S(D) + 14
  The denominator's chain is the shorter one: errors of alpha and beta change sum q^2 only in second order, q being orthogonal
  to 1 and t.

Both stay within the 2 D + 16 the kernels were specified to (S(D) <= D).  The counts are first-order and per chain; they do not cover
hypotheses so skewed that sum |c| max |c| >> sum c^2.

Nothing here reads the reference tree or needs a GPU."""
import numpy as np

import heads_mirror as M

F32, F64 = np.float32, np.float64
EPS = M.EPS


def S(D):
    return min(D, -(-D // 4) + 2)


def K(mode, D):
    k = 2 * S(D) + {3: 16, 4: 14}[mode]
    assert k <= 2 * D + 16
    return k


def distinct_count(a, axis=1):
    """Number of distinct values along `axis`."""
    srt = np.sort(np.asarray(a), axis=axis)
    return 1 + (np.diff(srt, axis=axis) != 0).sum(axis)


# --------------------------------------------------------------------------- float64 fits (from the same fp32 inputs)
def gauss0_fit64(prob, depth, hypos):
    """-> (b0, N, degenerate) float64 / bool [B,h,w].  b0 is NaN where fewer than 2 values of u are distinct."""
    z = M.log_clamped64(prob)
    x = np.broadcast_to(np.asarray(hypos, F32), z.shape).astype(F64)
    u = (x - np.asarray(depth, F32).astype(F64)[:, None]) ** 2
    um = u.mean(1, keepdims=True)
    c = u - um
    deg = distinct_count(u) < 2
    c = np.where(deg[:, None], 0.0, c)
    den = (c * c).sum(1)
    with np.errstate(all="ignore"):
        b0 = (c * z).sum(1) / den
        n = ((np.abs(u) + np.abs(um)) * np.abs(z)).sum(1) / den
    return b0, n, deg


def gauss1_fit64(prob, hypos):
    """-> (b0, N, degenerate).  b0 is NaN where fewer than 3 hypotheses are distinct."""
    z = M.log_clamped64(prob)
    x = np.broadcast_to(np.asarray(hypos, F32), z.shape).astype(F64)
    d = x.shape[1]
    e = x - x.mean(1, keepdims=True)
    sig = np.abs(e).max(1, keepdims=True)
    deg = distinct_count(x) < 3
    with np.errstate(all="ignore"):
        t = e / sig
        s1, s2, s3 = t.sum(1, keepdims=True), (t * t).sum(1, keepdims=True), (t ** 3).sum(1, keepdims=True)
        det = d * s2 - s1 * s1
        alpha, beta = (d * s3 - s1 * s2) / det, (s2 * s2 - s1 * s3) / det
        q = np.where(deg[:, None], 0.0, t * t - alpha * t - beta)
        den = (q * q).sum(1)
        b0 = (q * z).sum(1) / den / sig[:, 0] ** 2
        n = ((t * t + np.abs(alpha * t) + np.abs(beta)) * np.abs(z)).sum(1) / (sig[:, 0] ** 2 * den)
    return b0, n, deg


def ratio(s, b0_64, n, mode, D):
    """|1/s - |b0_64|| / (K * 2^-24 * N) per pixel (float64); s may be inf (1/s = 0)."""
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.asarray(s, F32).astype(F64)
    return np.abs(inv - np.abs(b0_64)) / (K(mode, D) * EPS * n)


# --------------------------------------------------------------------------- fp32 mirrors in the kernels' operation order
def _sum4(terms):
    """a[d & 3] += term_d; (a0 + a1) + (a2 + a3).  terms [B,D,h,w] fp32."""
    a = [np.zeros(terms.shape[:1] + terms.shape[2:], F32) for _ in range(4)]
    for d in range(terms.shape[1]):
        a[d & 3] = a[d & 3] + terms[:, d]
    return (a[0] + a[1]) + (a[2] + a[3])


def _dot4(x, y):
    """a[d & 3] = fma(x_d, y_d, a[d & 3]); (a0 + a1) + (a2 + a3)."""
    a = [np.zeros(x.shape[:1] + x.shape[2:], F32) for _ in range(4)]
    for d in range(x.shape[1]):
        a[d & 3] = M.fma32(x[:, d], y[:, d], a[d & 3])
    return (a[0] + a[1]) + (a[2] + a[3])


def _mean32(v):
    d = F32(v.shape[1])
    m1 = _sum4(v) / d
    return m1 + _sum4(v - m1[:, None]) / d


def gauss0_fit32(prob, depth, hypos, lnp=None):
    """hypos_fit_kernel mode 3 -> s [B,h,w] fp32."""
    z = M.log_clamped32(prob) if lnp is None else np.asarray(lnp, F32)
    with np.errstate(all="ignore"):
        e = np.broadcast_to(np.asarray(hypos, F32), z.shape) - np.asarray(depth, F32)[:, None]
        u = e * e
        c = u - _mean32(u)[:, None]
        return np.abs(_dot4(c, c) / _dot4(c, z))


def gauss1_fit32(prob, hypos, lnp=None):
    """hypos_fit_kernel mode 4 -> s [B,h,w] fp32."""
    z = M.log_clamped32(prob) if lnp is None else np.asarray(lnp, F32)
    x = np.ascontiguousarray(np.broadcast_to(np.asarray(hypos, F32), z.shape))
    n = F32(x.shape[1])
    with np.errstate(all="ignore"):
        e = x - _mean32(x)[:, None]
        lo, hi = x.min(1, keepdims=True), x.max(1, keepdims=True)
        three = ((x != lo) & (x != hi)).any(1)
        _, k = np.frexp(np.abs(e).max(1))
        k = k.astype(np.int32)
        t = np.ldexp(e, -k[:, None]).astype(F32)
        w = t * t
        s1, s2, s3 = _sum4(t), _sum4(w), _dot4(w, t)
        det = M.fma32(n, s2, -(s1 * s1))
        alpha = M.fma32(n, s3, -(s1 * s2)) / det
        beta = M.fma32(s2, s2, -(s1 * s3)) / det
        q = M.fma32(t, t - alpha[:, None], -beta[:, None])
        num = np.where(three, _dot4(q, z), F32(0))
        den = np.where(three, _dot4(q, q), F32(0))
        return np.abs(np.ldexp(den / num, 2 * k)).astype(F32)
