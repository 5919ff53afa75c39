"""Oracle of the DTU consensus fusion (mdf_consensus_fuse_fwd; the fusibile step of the reference's tools/gipuma/main.py -d):
an explicit restatement of the algorithm in torch CPU elementwise arithmetic, in the kernel's order -- every product, sum,
divide and square root is one correctly rounded operation, no matmul whose summation order BLAS chooses.
`dtype=torch.float64` gives the same steps in double precision (the decision-margin yardstick of the GPU test).

Per reference view r and pixel (x, y) with depth d:
    X = M_inv_r (d*x - p4.x, d*y - p4.y, d - p4.z)
    for v != r (ascending): (u, w, z) = P_v X;  pt = (u/z, w/z);  skip unless 0 <= pt.x < W and 0 <= pt.y < H
        d^ = bilinear(depth_v, pt)   texels floor(pt), floor(pt)+1 with wrap, weights frac(pt) in exact arithmetic
        agree = |f*b/z - f*b/d^| < disp_thresh,  b = |C_r - C_v|,  f = K_0[0,0]
        if agree: sum += M_inv_v (d^*floor(pt.x) - p4.x, d^*floor(pt.y) - p4.y, d^ - p4.z); col += bilinear(colour_v, pt); n += 1
    point = sum / (n+1), colour = trunc(col / (n+1)) (sum and col start with r's own point and texel)
    kept when n >= num_consistent and no coordinate is exactly 0; a non-finite point becomes (0, 0, 0)."""
import numpy as np
import torch


def cameras(K, E):
    """Camera table [N, 32] (P[12], M_inv[9], C[3], 8 unused) and the focal length f, as the host prepares them:
    P = K E[:3] in float64 rounded to fp32; M_inv and C in float64 from that fp32 P, rounded to fp32; f = K_0[0,0]."""
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    E = np.asarray(E, dtype=np.float32).astype(np.float64)
    tab = np.zeros((K.shape[0], 32), dtype=np.float32)
    for v in range(K.shape[0]):
        P = np.matmul(K[v], E[v, :3, :]).astype(np.float32)
        m = np.linalg.inv(P[:, :3].astype(np.float64))
        tab[v, :12] = P.ravel()
        tab[v, 12:21] = m.astype(np.float32).ravel()
        tab[v, 21:24] = (-np.matmul(m, P[:, 3].astype(np.float64))).astype(np.float32)
    return tab, np.float32(K[0, 0, 0])


def _dot3(m, x0, x1, x2):
    return (m[0] * x0 + m[1] * x1) + m[2] * x2


def fuse_view(r, depths, images, tab, f, disp_thresh, num_consistent, dtype=torch.float32):
    """Reference view r -> dict(keep [H,W] bool, xyz [H,W,3], rgb [H,W,3] uint8, n [H,W] int, margin [H,W]).
    margin: per pixel, the smallest distance of any view's decision quantity to its threshold -- |disparity difference -
    disp_thresh| of the in-bounds views and the distance of pt to the image border -- in `dtype` arithmetic."""
    dep = torch.as_tensor(np.asarray(depths)).to(dtype)
    img = torch.as_tensor(np.asarray(images))
    cam = torch.as_tensor(np.asarray(tab)).to(dtype)
    N, H, W = dep.shape
    f = torch.tensor(float(f), dtype=dtype)
    thr = torch.tensor(float(np.float32(disp_thresh)), dtype=dtype)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    xf, yf = xs.reshape(-1).to(dtype), ys.reshape(-1).to(dtype)
    cr = cam[r]
    d = dep[r].reshape(-1)
    a0, a1, a2 = d * xf - cr[3], d * yf - cr[7], d - cr[11]
    X0, X1, X2 = _dot3(cr[12:15], a0, a1, a2), _dot3(cr[15:18], a0, a1, a2), _dot3(cr[18:21], a0, a1, a2)
    s0, s1, s2 = X0.clone(), X1.clone(), X2.clone()
    rgb_r = img[r].reshape(-1, 3).to(dtype)
    c = [rgb_r[:, k].clone() for k in range(3)]
    n = torch.zeros(H * W, dtype=torch.int64)
    margin = torch.full((H * W,), float("inf"), dtype=dtype)
    fw, fh = torch.tensor(float(W), dtype=dtype), torch.tensor(float(H), dtype=dtype)
    for v in range(N):
        if v == r:
            continue
        cv = cam[v]
        u = _dot3(cv[0:3], X0, X1, X2) + cv[3]
        q = _dot3(cv[4:7], X0, X1, X2) + cv[7]
        z = _dot3(cv[8:11], X0, X1, X2) + cv[11]
        px, py = u / z, q / z
        inb = (px >= 0) & (px < fw) & (py >= 0) & (py < fh)
        border = torch.minimum(torch.minimum(px.abs(), (fw - px).abs()), torch.minimum(py.abs(), (fh - py).abs()))
        margin = torch.where(torch.isfinite(border), torch.minimum(margin, border), margin)
        if not bool(inb.any()):
            continue
        pxs, pys = torch.where(inb, px, torch.zeros_like(px)), torch.where(inb, py, torch.zeros_like(py))
        x0f, y0f = torch.floor(pxs), torch.floor(pys)
        ix, iy = x0f.long(), y0f.long()
        ix1 = torch.where(ix + 1 == W, torch.zeros_like(ix), ix + 1)
        iy1 = torch.where(iy + 1 == H, torch.zeros_like(iy), iy + 1)
        ax, ay = pxs - x0f, pys - y0f
        bx, by = 1.0 - ax, 1.0 - ay
        w00, w01, w10, w11 = bx * by, ax * by, bx * ay, ax * ay
        i00, i01, i10, i11 = iy * W + ix, iy * W + ix1, iy1 * W + ix, iy1 * W + ix1

        def lerp(t):
            return ((t[i00] * w00 + t[i01] * w01) + t[i10] * w10) + t[i11] * w11
        dh = lerp(dep[v].reshape(-1))
        e = cr[21:24] - cv[21:24]
        # the root through float64: torch's vectorised fp32 sqrt is not correctly rounded (it differs from IEEE by an ulp on
        # some inputs and CPUs), and one ulp of f*b moves disparity decisions that sit on the threshold
        fb = f * torch.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]).double()).to(dtype)
        diff = (fb / z - fb / dh).abs()
        agree = inb & (diff < thr)
        dm = (diff - thr).abs()
        margin = torch.where(inb & torch.isfinite(dm), torch.minimum(margin, dm), margin)
        b0, b1, b2 = dh * ix.to(dtype) - cv[3], dh * iy.to(dtype) - cv[7], dh - cv[11]
        s0 = torch.where(agree, s0 + _dot3(cv[12:15], b0, b1, b2), s0)
        s1 = torch.where(agree, s1 + _dot3(cv[15:18], b0, b1, b2), s1)
        s2 = torch.where(agree, s2 + _dot3(cv[18:21], b0, b1, b2), s2)
        col = img[v].reshape(-1, 3).to(dtype)
        for k in range(3):
            c[k] = torch.where(agree, c[k] + lerp(col[:, k]), c[k])
        n = n + agree.long()
    cnt = n.to(dtype) + 1.0
    x, y, zz = s0 / cnt, s1 / cnt, s2 / cnt
    keep = (n >= num_consistent) & (x != 0) & (y != 0) & (zz != 0)
    fin = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(zz)
    xyz = torch.where(fin[:, None], torch.stack([x, y, zz], 1), torch.zeros(1, 3, dtype=dtype))
    rgb = torch.stack([torch.clamp(ck / cnt, max=255.0).floor() for ck in c], 1).to(torch.uint8)
    return {"keep": keep.reshape(H, W), "xyz": xyz.reshape(H, W, 3), "rgb": rgb.reshape(H, W, 3), "n": n.reshape(H, W),
            "margin": margin.reshape(H, W)}


def fuse(depths, images, K, E, disp_thresh, num_consistent, dtype=torch.float32, ref_views=None):
    """Whole scan (or the listed reference views) -> (xyz [M,3], rgb [M,3] uint8, per-view kept counts, per-view dicts) in the
    kernel's output order."""
    tab, f = cameras(K, E)
    views = range(np.asarray(depths).shape[0]) if ref_views is None else ref_views
    per = {r: fuse_view(r, depths, images, tab, f, disp_thresh, num_consistent, dtype) for r in views}
    xyz = torch.cat([per[r]["xyz"][per[r]["keep"]] for r in views])
    rgb = torch.cat([per[r]["rgb"][per[r]["keep"]] for r in views])
    counts = [int(per[r]["keep"].sum()) for r in views]
    return xyz, rgb, counts, per
