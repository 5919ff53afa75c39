"""Explicit-order numpy mirror of confidence_cascade_kernel (mdf-net_amd/csrc/regress.hip): the reference's
confidence_regress(prob, last_confidence) (net/unit/regress.py:9-25) in fp32, every product and sum rounded on its own, in the order
the kernel promises.  The index and the default window come from heads_mirror (the kernels share that code path).

    cur  = ((0 + t[idx-pf]) + t[idx-pf+1]) + ... + t[idx-pf+n-1],   t = prob along D, 0 outside [0, D), idx = trunc(cascade E[d]) clamped
    up   = bicubic x2 of last (ATen upsample_bicubic2d, align_corners=False, A = -0.75): at output 2k the taps k-2 .. k+1 with weights W,
           at 2k+1 the taps k-1 .. k+2 with W reversed, tap indices clamped; per tap row ((p0*c0 + p1*c1) + p2*c2) + p3*c3 along x, the
           same form along y over the four row results
    conf = w_last * up + w_cur * cur         (last is None: conf = cur)

It is NOT ATen's fp32 order (its CPU kernel sums the taps differently: an ulp apart here and there); the yardstick of the kernel is
the reference's code on .double() inputs (tests/golden/confidence_cascade.npz).  Nothing here reads the reference tree or needs a GPU."""
import numpy as np

import heads_mirror as M

F32 = np.float32
W = np.array([-0.03515625, 0.26171875, 0.87890625, -0.10546875], dtype=F32)     # cubic convolution, A = -0.75, at t = 0.75; exact
BLEND = (0.8, 0.2)                                                             # regress.py:23


def bicubic2_taps(n_out, n_in):
    """regress.hip:bicubic2_taps for every output index -> (idx [n_out,4] clamped tap indices, c [n_out,4] fp32 weights)."""
    o = np.arange(n_out)
    odd = o & 1
    first = (o >> 1) - 2 + odd
    idx = np.clip(first[:, None] + np.arange(4)[None], 0, n_in - 1)
    c = np.where(odd[:, None] == 1, W[::-1][None], W[None]).astype(F32)
    return idx, c


def _four(v, c):
    """((v0*c0 + v1*c1) + v2*c2) + v3*c3 over the last axis of v, fp32 at every step."""
    return ((v[..., 0] * c[..., 0] + v[..., 1] * c[..., 1]) + v[..., 2] * c[..., 2]) + v[..., 3] * c[..., 3]


def bicubic_up2(last):
    """[B,h,w] -> [B,2h,2w].  A tap row's x pass depends on the source row and the output column only, so it is computed once per
    source row and gathered: the same fp32 values the kernel computes per output pixel."""
    last = np.asarray(last, F32)
    _, h, w = last.shape
    yi, cy = bicubic2_taps(2 * h, h)
    xi, cx = bicubic2_taps(2 * w, w)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = _four(last[:, :, xi], cx[None, None])                      # [B,h,2w]
        return _four(np.moveaxis(rows[:, yi], 2, 3), cy[None, :, None])    # rows[:, yi]: [B,2h,4,2w]


def window_sum(prob, n=4, pad_front=1):
    """-> cur [B,h,w] fp32: n terms from idx - pad_front upwards, ascending, starting from 0.0f."""
    prob = np.asarray(prob, F32)
    D = prob.shape[1]
    ic = np.clip(M.confidence(prob)[1], 0, D - 1)
    s = np.zeros(ic.shape, F32)
    for j in range(n):
        kk = ic - pad_front + j
        v = np.take_along_axis(prob, np.clip(kk, 0, D - 1)[:, None], axis=1)[:, 0]
        s = s + np.where((kk >= 0) & (kk < D), v, F32(0))
    return s


def cascade(prob, last=None, n=4, pad_front=1, weights=BLEND, up2=False):
    """confidence_cascade_kernel -> [B,h,w], or [B,2h,2w] with up2 (every value at its 2x2 pixels)."""
    s = window_sum(prob, n, pad_front)
    if last is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            s = F32(weights[0]) * bicubic_up2(last) + F32(weights[1]) * s
    return M.up2_nearest(s) if up2 else s


def chain(probs, up2_last=False, **kw):
    """c0 = f(p0), c1 = f(p1, c0), ... -> [c0, c1, ...]; up2_last: the last call with the nearest x2 folded in, as CoreNet issues it."""
    out, c = [], None
    for s, p in enumerate(probs):
        c = cascade(p, c, up2=up2_last and s == len(probs) - 1, **kw)
        out.append(c)
    return out
