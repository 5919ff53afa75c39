"""Oracle of the point-cloud fusion (mdf_pcd_fuse_fwd / mdf_pcd_compact; the reference's tools/pcd/fusion.py:get_cloud):
an explicit restatement of every stage in torch CPU elementwise arithmetic, in the kernels' operation order -- every product,
sum and divide is one correctly rounded operation, matrix-vector products are the left-to-right chains
((m0*x0 + m1*x1) + m2*x2) [+ m3*x3], square roots go through float64.  `dtype=torch.float64` runs the same steps in double
precision (the decision-margin yardstick).  The two C++ cores of the reference (vis_fusion_core, small_seg_core) are
restated in plain numpy, plus a vectorised torch min-label propagation of small_seg_core for full-size maps.

Camera table per view (CAM_STRIDE floats): K[9] @0, K^-1[9] @9, E[16] @18, E^-1[16] @34, camera centre -R^T t [3] @50.
K^-1, E^-1 and the centre are computed in float64 from the fp32 K and E and rounded to fp32.

Pipeline steps (STEPS): prob filter, vis filter, vis fusion, vis filter, ave fusion, vis filter, small-segment filter.  Each
step computes every view's update from the state before the step, then applies all updates."""
import numpy as np
import torch

CAM_STRIDE = 64
STEPS = ("prob", "vis1", "vis_fusion", "vis2", "ave", "vis3", "seg")
PTHRESH = 0.8
IMG_DIST = 1.0
DEPTH_THRESH = 0.01
SEG_WINDOW, SEG_DIFF, SEG_SIZE = 4, 1e-3, 10


def cameras(K, E):
    K = np.asarray(K, dtype=np.float32)
    E = np.asarray(E, dtype=np.float32)
    tab = np.zeros((K.shape[0], CAM_STRIDE), dtype=np.float32)
    for v in range(K.shape[0]):
        k64, e64 = K[v].astype(np.float64), E[v].astype(np.float64)
        tab[v, 0:9] = K[v].ravel()
        tab[v, 9:18] = np.linalg.inv(k64).astype(np.float32).ravel()
        tab[v, 18:34] = E[v].ravel()
        tab[v, 34:50] = np.linalg.inv(e64).astype(np.float32).ravel()
        tab[v, 50:53] = (-(e64[:3, :3].T @ e64[:3, 3])).astype(np.float32)
    return tab


def vis_need(vthresh):
    """Smallest view count c with c >= vthresh - 1.1 (the comparison runs in fp32: masks.sum() >= (vthresh-1.1))."""
    return int(np.ceil(np.float32(vthresh - 1.1)))


def src_table(pair_srcs, n, view):
    """[[source indices of view i] ...] -> int32 [n, view], the first `view` entries, padded with -1."""
    t = np.full((n, max(view, 1)), -1, dtype=np.int32)
    for i, s in enumerate(pair_srcs):
        s = list(s)[:view]
        t[i, :len(s)] = s
    return t[:, :view] if view > 0 else t[:, :0]


# --------------------------------------------------------------------------------------------------- camera arithmetic
def _d3(m, x0, x1, x2):
    return (m[0] * x0 + m[1] * x1) + m[2] * x2


def _d4(m, x0, x1, x2, x3):
    return ((m[0] * x0 + m[1] * x1) + m[2] * x2) + m[3] * x3


def _eps(dtype):
    return torch.tensor(1e-9, dtype=dtype)


def img2world(c, x, y, z, d):
    """utils.idx_img2world: K^-1 (x,y,z), / (c2 + 1e-9) * d, then E^-1 (c, 1), / (w3 + 1e-9) -> w0..w3."""
    e = _eps(x.dtype)
    ki, ei = c[9:18], c[34:50]
    c0, c1, c2 = _d3(ki[0:3], x, y, z), _d3(ki[3:6], x, y, z), _d3(ki[6:9], x, y, z)
    den = c2 + e
    c0, c1, c2 = c0 / den * d, c1 / den * d, c2 / den * d
    one = torch.ones_like(c0)
    w = [_d4(ei[4 * k:4 * k + 4], c0, c1, c2, one) for k in range(4)]
    den = w[3] + e
    return [wk / den for wk in w]


def world2cam(c, w):
    e = _eps(w[0].dtype)
    em = c[18:34]
    q = [_d4(em[4 * k:4 * k + 4], *w) for k in range(4)]
    den = q[3] + e
    return [qk / den for qk in q]


def cam2img(c, q):
    e = _eps(q[0].dtype)
    den = q[3] + e
    a0, a1, a2 = q[0] / den, q[1] / den, q[2] / den
    km = c[0:9]
    i0, i1, i2 = _d3(km[0:3], a0, a1, a2), _d3(km[3:6], a0, a1, a2), _d3(km[6:9], a0, a1, a2)
    den = i2 + e
    return i0 / den, i1 / den, i2 / den


def grid_nearest(dep, px, py):
    """F.grid_sample(dep, normalize_for_grid_sample(px, py), 'nearest', 'zeros', align_corners=False) and get_in_range of the
    clamped grid.  -> (sampled depth, in_range bool, margin): margin is the smallest distance of the continuous source index
    to a rounding boundary (a half-integer) or of the grid to +-1 (the decision quantities of this sample)."""
    H, W = dep.shape
    dt = px.dtype
    fw, fh = torch.tensor(float(W), dtype=dt), torch.tensor(float(H), dtype=dt)
    gx = (px / fw * 2 - 1).clamp(-1.1, 1.1)
    gy = (py / fh * 2 - 1).clamp(-1.1, 1.1)
    ix = (gx + 1) * (fw / 2) - 0.5
    iy = (gy + 1) * (fh / 2) - 0.5
    rx, ry = torch.round(ix), torch.round(iy)           # round half to even
    inb = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    idx = torch.where(inb, ry * W + rx, torch.zeros_like(rx)).long()
    val = torch.where(inb, dep.reshape(-1)[idx], torch.zeros_like(px))
    in_range = (gx <= 1) & (gx >= -1) & (gy <= 1) & (gy >= -1)
    mr = torch.minimum(((ix - torch.floor(ix)) - 0.5).abs(), ((iy - torch.floor(iy)) - 0.5).abs())
    mg = torch.minimum((gx.abs() - 1).abs(), (gy.abs() - 1).abs())
    margin = torch.minimum(mr, mg)
    margin = torch.where(torch.isfinite(margin), margin, torch.full_like(margin, float("inf")))
    return val, in_range, margin


def _grid(H, W, dtype):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return xs.reshape(-1).to(dtype) + 0.5, ys.reshape(-1).to(dtype) + 0.5


# --------------------------------------------------------------------------------------------------- stages
def reproj(r, dep, tab, srcs, dtype=torch.float32):
    """get_reproj + vis_filter's per-view masks for reference view r over all of its sources.
    -> (rd [V,HW] reprojected depth, m [V,HW] per-view mask (float 0/1), margin [HW] smallest relative decision margin)."""
    N, H, W = dep.shape
    d = dep[r].reshape(-1)
    cr = tab[r]
    xs, ys = _grid(H, W, dtype)
    one = torch.ones_like(xs)
    valid = d > torch.tensor(1e-9, dtype=dtype)
    wr = img2world(cr, xs, ys, one, d)
    rds, ms = [], []
    margin = torch.full_like(d, float("inf"))
    thr = torch.tensor(DEPTH_THRESH, dtype=dtype)
    for s in srcs:
        s = int(s)
        if s < 0 or s >= N:                           # -1 = none; the kernels ignore an index past the scan too
            continue
        cs = tab[s]
        i0, i1, i2 = cam2img(cs, world2cam(cs, wr))
        g, inr, mg = grid_nearest(dep[s], i0, i1)
        inr = inr & (g > torch.tensor(1e-9, dtype=dtype))
        w2 = img2world(cs, i0, i1, i2, g)
        q = world2cam(cr, w2)
        j0, j1, _ = cam2img(cr, q)
        rd = q[2]
        dx, dy = j0 - xs, j1 - ys
        dist = torch.sqrt((dx * dx + dy * dy).double()).to(dtype)
        lim = torch.maximum(d, rd) * thr
        m = inr & valid & (dist < IMG_DIST) & ((d - rd).abs() < lim)
        # zero where the reference pixel is invalid (unflatten of the valid pixels' values)
        rds.append(torch.where(valid, rd, torch.zeros_like(rd)))
        ms.append(m.to(dtype))
        rel = torch.minimum((dist - 1).abs(), ((d - rd).abs() - lim).abs() / lim.abs())
        rel = torch.minimum(rel, mg)
        margin = torch.where(valid & torch.isfinite(rel), torch.minimum(margin, rel), margin)
    if not rds:
        return torch.zeros(0, H * W, dtype=dtype), torch.zeros(0, H * W, dtype=dtype), margin
    return torch.stack(rds), torch.stack(ms), margin


def vis_filter(dep, mask, tab, srcs, need, dtype=torch.float32):
    """-> (new depth, new mask, margin [N,H,W]) after one batch_vis_filter."""
    N, H, W = dep.shape
    dep = dep.to(dtype)
    kept, margins = [], []
    for r in range(N):
        _, m, mg = reproj(r, dep, tab, srcs[r], dtype)
        cnt = m.sum(0) if m.shape[0] else torch.zeros(H * W, dtype=dtype)
        kept.append((cnt >= need).reshape(H, W))
        margins.append(mg.reshape(H, W))
    mask = mask & torch.stack(kept)
    return dep * mask.to(dtype), mask, torch.stack(margins)


def ave_fusion(dep, mask, tab, srcs, dtype=torch.float32):
    N, H, W = dep.shape
    dep = dep.to(dtype)
    out = []
    for r in range(N):
        rd, m, _ = reproj(r, dep, tab, srcs[r], dtype)
        s = torch.zeros(H * W, dtype=dtype)
        c = torch.zeros(H * W, dtype=dtype)
        for v in range(m.shape[0]):
            s = s + rd[v] * m[v]
            c = c + m[v]
        out.append(((s + dep[r].reshape(-1)) / (c + 1)).reshape(H, W))
    return torch.stack(out) * mask.to(dtype)


def fusion_candidates(r, dep, tab, srcs, dtype=torch.float32, with_self=False):
    """vis_fusion's candidates of reference view r -> (d [M], x [M], y [M], violations [M] int, margin [M]) and, with_self,
    self [M] int: the violation the candidate's own source contributed (a source pixel checked against its own depth map --
    its depth against itself re-projected, decided by rounding; 0 for the reference's pixels).  margin leaves those checks out.
    Order: the reference's valid pixels, then each source's valid pixels, row-major."""
    N, H, W = dep.shape
    cr = tab[r]
    xs, ys = _grid(H, W, dtype)
    one = torch.ones_like(xs)
    eps9 = torch.tensor(1e-9, dtype=dtype)
    dr = dep[r].reshape(-1)
    vr = dr > eps9
    ax, ay, az, ad = [xs[vr]], [ys[vr]], [one[vr]], [dr[vr]]
    srcs = [int(s) for s in srcs if 0 <= int(s) < N]
    origin = [torch.full((int(vr.sum()),), -1, dtype=torch.int64)]
    for s in srcs:
        ds = dep[s].reshape(-1)
        vs = ds > eps9
        origin.append(torch.full((int(vs.sum()),), s, dtype=torch.int64))
        w = img2world(tab[s], xs[vs], ys[vs], one[vs], ds[vs])
        q = world2cam(cr, w)
        i0, i1, i2 = cam2img(cr, q)
        ax.append(i0), ay.append(i1), az.append(i2), ad.append(q[2])
    ax, ay, az, ad = torch.cat(ax), torch.cat(ay), torch.cat(az), torch.cat(ad)
    w = img2world(cr, ax, ay, az, ad)
    origin = torch.cat(origin)
    vio = torch.zeros(ad.shape[0], dtype=torch.int32)
    selfv = torch.zeros(ad.shape[0], dtype=torch.int32)
    margin = torch.full_like(ad, float("inf"))
    for s in srcs:
        q = world2cam(tab[s], w)
        i0, i1, _ = cam2img(tab[s], q)
        g, _, mg = grid_nearest(dep[s], i0, i1)
        v = (g > q[2]).int()
        vio += v
        own = origin == s
        selfv += torch.where(own, v, torch.zeros_like(v))
        rel = ((g - q[2]).abs() / q[2].abs())
        rel = torch.where(g == 0, torch.full_like(rel, float("inf")), rel)   # zero padding: no comparison margin
        m = torch.where(torch.isfinite(mg), torch.minimum(mg, rel), rel)
        margin = torch.where(own, margin, torch.minimum(margin, m))
    if with_self:
        return ad, ax, ay, vio, margin, selfv
    return ad, ax, ay, vio, margin


def vis_fusion_core(depth, x, y, violation, valid):
    """numpy restatement of fusion.cpp:vis_fusion_core.  Bin (round_half_away(x - .5), round_half_away(y - .5)) in double,
    kept when in range, depth > 1e-9 (double) and valid[bin]; each bin sorted by (depth, violation); its output is the first
    entry k with k >= violation[k], else the last entry; empty bins give 0."""
    valid = np.asarray(valid, dtype=bool)
    h, w = valid.shape
    depth = np.asarray(depth, dtype=np.float32)
    vio = np.asarray(violation, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        tx = np.asarray(x, dtype=np.float32).astype(np.float64) - 0.5
        ty = np.asarray(y, dtype=np.float32).astype(np.float64) - 0.5
        ok = (tx > -0.5) & (tx < w - 0.5) & (ty > -0.5) & (ty < h - 0.5) & (depth.astype(np.float64) > 1e-9)
    bx = np.where(ok, np.sign(tx) * np.floor(np.abs(tx) + 0.5), 0).astype(np.int64)
    by = np.where(ok, np.sign(ty) * np.floor(np.abs(ty) + 0.5), 0).astype(np.int64)
    ok &= valid[by, bx]
    b = (by * w + bx)[ok]
    d, v = depth[ok], vio[ok]
    out = np.zeros(h * w, dtype=np.float32)
    if b.size == 0:
        return out.reshape(h, w)
    order = np.lexsort((v, d, b))
    b, d, v = b[order], d[order], v[order]
    start = np.r_[0, np.flatnonzero(np.diff(b)) + 1]
    k = np.arange(b.size) - np.repeat(start, np.diff(np.r_[start, b.size]))
    last = np.r_[start[1:] - 1, b.size - 1]
    sel = np.where(k >= v, np.arange(b.size), b.size + 1)
    first = np.minimum.reduceat(sel, start)
    pick = np.where(first <= last, first, last)
    out[b[start]] = d[pick]
    return out.reshape(h, w)


def vis_fusion(dep, mask, tab, srcs, dtype=torch.float32, with_margin=False):
    N, H, W = dep.shape
    dep = dep.to(dtype)
    outs, margins = [], []
    for r in range(N):
        d, x, y, vio, mg = fusion_candidates(r, dep, tab, srcs[r], dtype)
        valid = (dep[r] > torch.tensor(1e-9, dtype=dtype)).numpy()
        outs.append(torch.from_numpy(vis_fusion_core(d.float().numpy(), x.float().numpy(), y.float().numpy(), vio.numpy(), valid))
                    .to(dtype) if dtype == torch.float32 else
                    torch.from_numpy(_core64(d.numpy(), x.numpy(), y.numpy(), vio.numpy(), valid)))
        if with_margin:
            m = np.full(H * W, np.inf)
            tx, ty = x.double().numpy() - 0.5, y.double().numpy() - 0.5
            ok = (tx > -0.5) & (tx < W - 0.5) & (ty > -0.5) & (ty < H - 0.5)
            bx = np.clip(np.round(tx), 0, W - 1).astype(np.int64)
            by = np.clip(np.round(ty), 0, H - 1).astype(np.int64)
            mb = np.minimum(np.abs(np.abs(tx - np.floor(tx)) - 0.5), np.abs(np.abs(ty - np.floor(ty)) - 0.5))
            np.minimum.at(m, (by * W + bx)[ok], np.minimum(mg.double().numpy(), mb)[ok])
            margins.append(m.reshape(H, W))
    out = torch.stack(outs) * mask.to(dtype)
    return (out, np.stack(margins)) if with_margin else out


def _core64(depth, x, y, vio, valid):
    """vis_fusion_core on float64 candidates (the yardstick run): same rule, float64 depths."""
    h, w = valid.shape
    tx, ty = x - 0.5, y - 0.5
    with np.errstate(invalid="ignore"):
        ok = (tx > -0.5) & (tx < w - 0.5) & (ty > -0.5) & (ty < h - 0.5) & (depth > 1e-9)
    bx = np.where(ok, np.sign(tx) * np.floor(np.abs(tx) + 0.5), 0).astype(np.int64)
    by = np.where(ok, np.sign(ty) * np.floor(np.abs(ty) + 0.5), 0).astype(np.int64)
    ok &= valid[by, bx]
    b, d, v = (by * w + bx)[ok], depth[ok], vio[ok].astype(np.int64)
    out = np.zeros(h * w)
    if b.size == 0:
        return out.reshape(h, w)
    order = np.lexsort((v, d, b))
    b, d, v = b[order], d[order], v[order]
    start = np.r_[0, np.flatnonzero(np.diff(b)) + 1]
    k = np.arange(b.size) - np.repeat(start, np.diff(np.r_[start, b.size]))
    last = np.r_[start[1:] - 1, b.size - 1]
    first = np.minimum.reduceat(np.where(k >= v, np.arange(b.size), b.size + 1), start)
    out[b[start]] = d[np.where(first <= last, first, last)]
    return out.reshape(h, w)


def small_seg_core(depth, window_size=SEG_WINDOW, diff_thresh=SEG_DIFF, size_thresh=SEG_SIZE):
    """Plain-Python restatement of fusion.cpp:small_seg_core (BFS flood fill, float arithmetic of the predicate)."""
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    thr = np.float32(diff_thresh)
    out = np.ones((h, w), dtype=np.uint8)
    visit = np.zeros((h, w), dtype=np.uint8)
    bad = depth.astype(np.float64) < 1e-9
    visit[bad] = 2
    out[bad] = 0
    nb = [(i, j) for i in range(-window_size, window_size + 1) for j in range(-window_size, window_size + 1) if (i, j) != (0, 0)]
    for i in range(h):
        for j in range(w):
            if visit[i, j] == 2:
                continue
            queue = [(i, j)]
            visit[i, j] = 1
            k = 0
            while k < len(queue):
                ci, cj = queue[k]
                cd = depth[ci, cj]
                for di, dj in nb:
                    ni, nj = ci + di, cj + dj
                    if not (0 <= ni < h and 0 <= nj < w) or visit[ni, nj] != 0:
                        continue
                    nd = depth[ni, nj]
                    if np.abs(cd - nd) >= thr * (cd + nd):
                        continue
                    queue.append((ni, nj))
                    visit[ni, nj] = 1
                visit[ci, cj] = 2
                k += 1
            if len(queue) < size_thresh:
                for ci, cj in queue:
                    out[ci, cj] = 0
    return out


def small_seg_torch(depth, window_size=SEG_WINDOW, diff_thresh=SEG_DIFF, size_thresh=SEG_SIZE):
    """small_seg_core by vectorised min-label propagation (full-size maps): every valid pixel starts with its own index, takes
    the minimum label over its linked neighbours until nothing changes (with pointer jumping), and components are counted by
    label.  Independent of the kernel's union-find.  -> uint8 [h, w]."""
    d = torch.as_tensor(np.asarray(depth, dtype=np.float32))
    h, w = d.shape
    thr = torch.tensor(diff_thresh, dtype=torch.float32)
    valid = ~(d.double() < 1e-9)
    big = h * w
    lab = torch.where(valid, torch.arange(big).reshape(h, w), torch.full((h, w), big))
    offs = [(i, j) for i in range(0, window_size + 1) for j in range(-window_size, window_size + 1) if i > 0 or j > 0]
    links = []
    for di, dj in offs:      # link between (y, x) and (y+di, x+dj), stored at the first pixel's position
        ys0, ys1 = 0, h - di
        xs0, xs1 = max(0, -dj), min(w, w - dj)
        a = d[ys0:ys1, xs0:xs1]
        b = d[ys0 + di:ys1 + di, xs0 + dj:xs1 + dj]
        l = valid[ys0:ys1, xs0:xs1] & valid[ys0 + di:ys1 + di, xs0 + dj:xs1 + dj] & ~((a - b).abs() >= thr * (a + b))
        links.append((di, dj, ys0, ys1, xs0, xs1, l))
    flat_ok = valid.reshape(-1)
    while True:
        new = lab.clone()
        for di, dj, ys0, ys1, xs0, xs1, l in links:
            a = new[ys0:ys1, xs0:xs1]
            b = new[ys0 + di:ys1 + di, xs0 + dj:xs1 + dj]
            m = torch.where(l, torch.minimum(a, b), torch.full_like(a, big))
            new[ys0:ys1, xs0:xs1] = torch.minimum(a, m)
            new[ys0 + di:ys1 + di, xs0 + dj:xs1 + dj] = torch.minimum(new[ys0 + di:ys1 + di, xs0 + dj:xs1 + dj], m)
        f = new.reshape(-1)
        while True:                                   # pointer jumping: a label is a pixel index of the same component
            g = torch.where(flat_ok, f[f.clamp(max=big - 1)], f)
            if torch.equal(g, f):
                break
            f = g
        new = f.reshape(h, w)
        if torch.equal(new, lab):
            break
        lab = new
    f = lab.reshape(-1)
    sizes = torch.bincount(f[flat_ok], minlength=big)
    keep = flat_ok & (sizes[f.clamp(max=big - 1)] >= size_thresh)
    return keep.reshape(h, w).to(torch.uint8).numpy()


def seg_filter(dep, mask, core=small_seg_core):
    seg = torch.stack([torch.from_numpy(core(dep[r].float().numpy()).astype(bool)) for r in range(dep.shape[0])])
    mask = mask & seg
    return dep * mask.to(dep.dtype), mask


def back_project(dep, mask, images, tab):
    """get_cloud's back projection of the mask-true pixels: -> (xyz [M,3], rgb [M,3] uint8, dirs [M,3]) in view, then row-major
    pixel order (dirs: camera centre - point)."""
    N, H, W = dep.shape
    xs, ys = _grid(H, W, torch.float32)
    one = torch.ones_like(xs)
    P, C, D = [], [], []
    for r in range(N):
        t = torch.as_tensor(tab[r])
        w = img2world(t, xs, ys, one, dep[r].reshape(-1).float())
        m = mask[r].reshape(-1)
        p = torch.stack(w[:3], 1)
        c = t[50:53]
        P.append(p[m])
        D.append((c[None, :] - p)[m])
        C.append(torch.as_tensor(np.asarray(images[r])).reshape(-1, 3)[m])
    return torch.cat(P), torch.cat(C), torch.cat(D)


def run(depths, probs, K, E, srcs, vthresh=4, stop=len(STEPS), dtype=torch.float32, seg_core=small_seg_core, record=None):
    """Steps 1..stop of the pipeline on one scan -> (depth [N,H,W], mask [N,H,W] bool).  record(name, depth, mask) is
    called after every step."""
    tab = torch.from_numpy(cameras(K, E)).to(dtype)
    dep = torch.as_tensor(np.asarray(depths, dtype=np.float32))
    prob = torch.as_tensor(np.asarray(probs, dtype=np.float32))
    srcs = np.asarray(srcs)
    need = vis_need(vthresh)
    mask = prob > PTHRESH
    dep = (dep * mask.float()).to(dtype)
    if record:
        record("prob", dep, mask)
    for name in STEPS[1:stop]:
        if name.startswith("vis") and name != "vis_fusion":
            dep, mask, _ = vis_filter(dep, mask, tab, srcs, need, dtype)
        elif name == "vis_fusion":
            dep = vis_fusion(dep, mask, tab, srcs, dtype)
        elif name == "ave":
            dep = ave_fusion(dep, mask, tab, srcs, dtype)
        else:
            dep, mask = seg_filter(dep, mask, seg_core)
        if record:
            record(name, dep, mask)
    return dep, mask
