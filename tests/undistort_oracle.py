"""float64 restatement of mdf_image_undistort (include/mdfnet_hip.h), in numpy and vectorised, for the undistortion tests.  numpy
rounds every elementwise product, sum and quotient once and never contracts, and its sqrt and / are correctly rounded, so for the
rational kind this file and the kernel execute the same operations; for the fisheye kind they differ through atan alone.

THE OPERATION ORDER (every bracket is one rounding; the kernel follows it, and so does tools/colmap/undistort.py on the host):

  sample (b, a) of output pixel (row i, column j), b outer, a, b = 0..n-1:
      X = (j + ((a + 0.5) / n)) / s                 Y = (i + ((b + 0.5) / n)) / s
      x = (X - cx) / (z fx)                         y = (Y - cy) / (z fy)                   [z fx and z fy are one product each]
      (xd, yd) = distort(x, y)
      U = ((fx xd) + cx) - 0.5                      V = ((fy yd) + cy) - 0.5
  rational (k1, k2, p1, p2, k3, k4, k5, k6):
      xx = x x, yy = y y, r2 = xx + yy, r4 = r2 r2, r6 = r4 r2
      rad = (((1 + (k1 r2)) + (k2 r4)) + (k3 r6)) / (((1 + (k4 r2)) + (k5 r4)) + (k6 r6))
      q = 2 (x y)
      xd = (x rad) + ((p1 q) + (p2 (r2 + (2 xx))))  yd = (y rad) + ((p2 q) + (p1 (r2 + (2 yy))))
  fisheye (k1, k2, k3, k4):
      r = sqrt(r2); r == 0: (xd, yd) = (x, y); else t = atan(r), t2 = t t, t4 = t2 t2, t6 = t4 t2, t8 = t4 t4,
      sc = (t ((((1 + (k1 t2)) + (k2 t4)) + (k3 t6)) + (k4 t8))) / r,  xd = x sc, yd = y sc
  blank: U or V not finite, U < -0.5, U > W - 0.5, V < -0.5, V > H - 0.5 (adds 0 to every channel)
  else: u = floor(U), wu = U - u, mu = 1 - wu (v, wv, mv alike), taps at columns max(u, 0), min(u + 1, W - 1) and rows max(v, 0),
      min(v + 1, H - 1); per channel top = (p00 mu) + (p01 wu), bot = (p10 mu) + (p11 wu), value = (top mv) + (bot wv)
  output: mean = (0 + the n n values one after the other in (b, a) order) / (n n); byte = floor(mean + 0.5); valid = no blank sample."""
import numpy as np

RATIONAL, FISHEYE = "rational", "fisheye"


def model_coeffs(model, params):
    """COLMAP (model, params) -> (kind, coeffs [12], fx, fy, cx, cy), from COLMAP's documented parameter order."""
    p = [float(v) for v in params]
    c = np.zeros(12)
    if model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL"):
        fx, fy, cx, cy, rest = p[0], p[0], p[1], p[2], p[3:]
    else:
        fx, fy, cx, cy, rest = p[0], p[1], p[2], p[3], p[4:]
    kind = FISHEYE if model == "OPENCV_FISHEYE" else RATIONAL
    assert len(rest) == {"SIMPLE_PINHOLE": 0, "PINHOLE": 0, "SIMPLE_RADIAL": 1, "RADIAL": 2, "OPENCV": 4, "FULL_OPENCV": 8, "OPENCV_FISHEYE": 4}[model]
    c[:len(rest)] = rest
    return kind, c, fx, fy, cx, cy


def distort(kind, c, x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xx, yy = x * x, y * y
    r2 = xx + yy
    with np.errstate(all="ignore"):
        if kind == RATIONAL:
            r4 = r2 * r2
            r6 = r4 * r2
            num = ((1.0 + (c[0] * r2)) + (c[1] * r4)) + (c[4] * r6)
            den = ((1.0 + (c[5] * r2)) + (c[6] * r4)) + (c[7] * r6)
            rad = num / den
            q = 2.0 * (x * y)
            xd = (x * rad) + ((c[2] * q) + (c[3] * (r2 + (2.0 * xx))))
            yd = (y * rad) + ((c[3] * q) + (c[2] * (r2 + (2.0 * yy))))
            return xd, yd
        assert kind == FISHEYE
        r = np.sqrt(r2)
        t = np.arctan(r)
        t2 = t * t
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t4 * t4
        sc = (t * ((((1.0 + (c[0] * t2)) + (c[1] * t4)) + (c[2] * t6)) + (c[3] * t8))) / r
        return np.where(r == 0.0, x, x * sc), np.where(r == 0.0, y, y * sc)


def sample_coords(kind, c, fx, fy, cx, cy, out_hw, zoom=1.0, scale=1.0, nsub=1):
    """-> U, V [n, n, Hd, Wd] float64 (sample b, sample a, row, column): where each sample falls in the source, in its pixel indices."""
    hd, wd = out_hw
    n = int(nsub)
    sub = (np.arange(n, dtype=np.float64) + 0.5) / float(n)
    X = (np.arange(wd, dtype=np.float64)[None, :] + sub[:, None]) / scale          # [a, j]
    Y = (np.arange(hd, dtype=np.float64)[None, :] + sub[:, None]) / scale          # [b, i]
    zfx, zfy = zoom * fx, zoom * fy
    x = ((X - cx) / zfx)[None, :, None, :]
    y = ((Y - cy) / zfy)[:, None, :, None]
    x, y = np.broadcast_arrays(x, y)
    xd, yd = distort(kind, c, x, y)
    with np.errstate(all="ignore"):
        return ((fx * xd) + cx) - 0.5, ((fy * yd) + cy) - 0.5


def blank_mask(U, V, w, h):
    with np.errstate(invalid="ignore"):
        return ~((U >= -0.5) & (U <= w - 0.5) & (V >= -0.5) & (V <= h - 0.5))        # NaN and infinities land here too


def threshold_distance(U, V, w, h):
    """The smallest distance of any finite U, V from the four blank thresholds (the fisheye test leaves out pixels closer than 1e-9)."""
    with np.errstate(invalid="ignore"):
        d = np.minimum(np.minimum(np.abs(U + 0.5), np.abs(U - (w - 0.5))), np.minimum(np.abs(V + 0.5), np.abs(V - (h - 0.5))))
    return np.where(np.isfinite(d), d, np.inf)


def undistort(src, kind, c, fx, fy, cx, cy, out_hw, zoom=1.0, scale=1.0, nsub=1):
    """src [B,H,W,3] uint8 -> dict: bytes [B,Hd,Wd,3] uint8, valid [B,Hd,Wd] uint8, mean [B,Hd,Wd,3] float64 (before rounding),
    U, V [n,n,Hd,Wd], blank [n,n,Hd,Wd]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4 and src.shape[3] == 3
    B, h, w, _ = src.shape
    n = int(nsub)
    U, V = sample_coords(kind, c, fx, fy, cx, cy, out_hw, zoom, scale, n)
    blank = blank_mask(U, V, w, h)
    Uc, Vc = np.where(blank, 0.0, U), np.where(blank, 0.0, V)
    fu, fv = np.floor(Uc), np.floor(Vc)
    wu, wv = Uc - fu, Vc - fv
    mu, mv = 1.0 - wu, 1.0 - wv
    u0, u1 = np.maximum(fu.astype(np.int64), 0), np.minimum(fu.astype(np.int64) + 1, w - 1)
    v0, v1 = np.maximum(fv.astype(np.int64), 0), np.minimum(fv.astype(np.int64) + 1, h - 1)
    img = src.astype(np.float64)
    acc = np.zeros((B,) + tuple(out_hw) + (3,), dtype=np.float64)
    for b in range(n):
        for a in range(n):
            k = (b, a)
            p00, p01 = img[:, v0[k], u0[k]], img[:, v0[k], u1[k]]                      # [B, Hd, Wd, 3]
            p10, p11 = img[:, v1[k], u0[k]], img[:, v1[k], u1[k]]
            top = (p00 * mu[k][None, :, :, None]) + (p01 * wu[k][None, :, :, None])
            bot = (p10 * mu[k][None, :, :, None]) + (p11 * wu[k][None, :, :, None])
            val = (top * mv[k][None, :, :, None]) + (bot * wv[k][None, :, :, None])
            acc = acc + np.where(blank[k][None, :, :, None], 0.0, val)
    mean = acc / (float(n) * float(n))
    out = np.minimum(np.floor(mean + 0.5), 255.0).astype(np.uint8)
    valid = (~blank.any(axis=(0, 1))).astype(np.uint8)
    return {"bytes": out, "valid": np.broadcast_to(valid, (B,) + valid.shape).copy(), "mean": mean, "U": U, "V": V, "blank": blank}


def smooth_image(h, w, seed=0):
    """A smooth colour image [h,w,3] uint8 (low-frequency sines, a different phase per channel)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ch = []
    for _ in range(3):
        fx, fy, ph = rng.uniform(0.02, 0.09), rng.uniform(0.02, 0.09), rng.uniform(0, 6.28)
        ch.append(127.5 + 120.0 * np.sin(fx * xx + ph) * np.cos(fy * yy - ph))
    return np.clip(np.round(np.stack(ch, axis=2)), 0, 255).astype(np.uint8)


def noise_image(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def ramp_image(h, w):
    """R = column, G = row, B = 0 (h, w <= 256): bilinear interpolation of it is exact, so R reads U and G reads V."""
    assert h <= 256 and w <= 256
    out = np.zeros((h, w, 3), dtype=np.uint8)
    out[:, :, 0] = np.arange(w, dtype=np.uint8)[None, :]
    out[:, :, 1] = np.arange(h, dtype=np.uint8)[:, None]
    return out
