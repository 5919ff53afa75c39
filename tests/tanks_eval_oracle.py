"""Oracle of the Tanks and Temples F-score evaluation: numpy fp64 elementwise arithmetic, with
scipy.spatial.cKDTree only to FIND nearest-neighbour candidates.

Distances are recomputed as d^2 = ((dx*dx) + dy*dy) + dz*dz (numpy never contracts elementwise products into fmas), the formula
the kernels use, and ties go to the lowest index, so distances and indices compare bit for bit.  The voxel sums run through
np.add.at, which adds sequentially in input order.  The ICP sums use numpy's own (pairwise) summation: they agree with the
kernels' fixed tree only within the rounding bound update_bound() derives from the data."""
import os

import numpy as np
from scipy.spatial import cKDTree

TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01, "Truck": 0.005}
U = 2.0 ** -53
MAX_CELLS = 1 << 21


def dist2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def transform(pts, T):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)


def uv_axes(axis):
    return (1 if axis == 0 else 0), (1 if axis == 2 else 2)


def crop(pts, axis, axis_min, axis_max, polygon):
    """keep [n] bool: the axis interval (closed) and the even-odd count of the crossings u_i + ((v - v_i) / (v_j - v_i)) * (u_j - u_i)
    < u over the edges with (v_i < v <= v_j) or (v_j < v <= v_i)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    poly = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    iu, iv = uv_axes(axis)
    w, x, y = pts[:, axis], pts[:, iu], pts[:, iv]
    cnt = np.zeros(len(pts), dtype=np.int64)
    k = len(poly)
    for i in range(k):
        j = (i + 1) % k
        ui, vi, uj, vj = poly[i, 0], poly[i, 1], poly[j, 0], poly[j, 1]
        cross = ((vi < y) & (vj >= y)) | ((vj < y) & (vi >= y))
        with np.errstate(divide="ignore", invalid="ignore"):
            node = ui + ((y - vi) / (vj - vi)) * (uj - ui)
        cnt += cross & (node < x)
    return (w >= axis_min) & (w <= axis_max) & ((cnt & 1) == 1)


def voxel(pts, v, attrs=None):
    """-> (points [m,3], attrs [m,k] or None, counts [m]) in ascending (x, y, z) cell order."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    k = 0 if attrs is None else np.asarray(attrs).shape[-1]
    if n == 0:
        return np.zeros((0, 3)), (np.zeros((0, k)) if attrs is not None else None), np.zeros(0, dtype=np.int32)
    origin = pts.min(0) - v / 2
    cell = np.floor((pts - origin) / v)
    if cell.max() >= MAX_CELLS:
        raise ValueError("more than 2^21 cells on an axis")
    cell = cell.astype(np.int64)
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(n, dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    seg = np.cumsum(head) - 1                      # segment of sorted position s
    m = int(seg[-1]) + 1
    sums = np.zeros((m, 3))
    np.add.at(sums, seg, pts[order])               # sequential, the cell's points in input order (the sort is stable)
    counts = np.bincount(seg, minlength=m)
    out_a = None
    if attrs is not None:
        a = np.asarray(attrs, dtype=np.float64).reshape(n, k)
        sa = np.zeros((m, k))
        np.add.at(sa, seg, a[order])
        out_a = sa / counts[:, None]
    return sums / counts[:, None], out_a, counts.astype(np.int32)


def nn(to, frm, cap, k=8):
    """-> (dist [m], nearest [m] int32, d2 [m]): the exact nearest neighbour under dist2(), ties to the lowest index; (cap, -1, inf)
    when no point lies within d < cap."""
    to = np.asarray(to, dtype=np.float64).reshape(-1, 3)
    frm = np.asarray(frm, dtype=np.float64).reshape(-1, 3)
    m = len(frm)
    dist, idx, d2o = np.full(m, float(cap)), np.full(m, -1, dtype=np.int32), np.full(m, np.inf)
    if len(to) == 0 or m == 0:
        return dist, idx, d2o
    tree = cKDTree(to)
    k = min(k, len(to))
    _, cand = tree.query(frm, k=k)
    cand = cand.reshape(m, k)
    d2 = dist2(frm[:, None, :], to[cand])
    best = d2.min(1)
    pick = np.where(d2 == best[:, None], cand, len(to)).min(1)
    # every candidate as near as the best one (a pile of equal points): the k candidates may not hold them all
    crowded = np.nonzero((d2.max(1) <= best * (1 + 1e-12)) & (len(to) > k))[0]
    for q in crowded:
        ball = np.asarray(tree.query_ball_point(frm[q], np.sqrt(best[q]) * (1 + 1e-9) + 1e-300), dtype=np.int64)
        bd = dist2(frm[q][None, :], to[ball])
        best[q] = bd.min()
        pick[q] = ball[bd == best[q]].min()
    d = np.sqrt(best)
    found = d < cap
    dist[found], idx[found], d2o[found] = d[found], pick[found], best[found]
    return dist, idx, d2o


def nn_brute(to, frm, cap):
    """The same by an O(nm) search (small scenes)."""
    to = np.asarray(to, dtype=np.float64).reshape(-1, 3)
    frm = np.asarray(frm, dtype=np.float64).reshape(-1, 3)
    dist, idx, d2o = np.full(len(frm), float(cap)), np.full(len(frm), -1, dtype=np.int32), np.full(len(frm), np.inf)
    if len(to) == 0:
        return dist, idx, d2o
    for q in range(len(frm)):
        d2 = dist2(frm[q][None, :], to)
        j = int(np.argmin(d2))                      # argmin: the first (lowest-index) minimum
        if np.sqrt(d2[j]) < cap:
            dist[q], idx[q], d2o[q] = np.sqrt(d2[j]), j, d2[j]
    return dist, idx, d2o


def icp_sums(src, tgt, nearest, d2, threshold):
    """-> [17]: count, sum d2, source centroid, target centroid, H row-major (H[a][b] = sum (s_a - cs_a)(t_b - ct_b))."""
    inl = (nearest >= 0) & (np.sqrt(d2) < threshold)
    P, Q = src[inl], tgt[nearest[inl]]
    out = np.zeros(17)
    out[0] = inl.sum()
    if out[0] == 0:
        return out
    out[1] = d2[inl].sum()
    out[2:5], out[5:8] = P.sum(0) / out[0], Q.sum(0) / out[0]
    out[8:17] = ((P - out[2:5]).T @ (Q - out[5:8])).reshape(-1)
    return out


def rigid_update(sums):
    cs, ct, H = sums[2:5], sums[5:8], sums[8:17].reshape(3, 3)
    Uu, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ Uu.T) >= 0 else -1.0])
    R = Vt.T @ D @ Uu.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = ct - R @ cs
    return T


def update_bound(P, Q, eps=0.0):
    """How far two evaluations of rigid_update can differ when both sum the same inlier pairs (P[i], Q[i]) in fp64 in any order and
    every source point carries a position error of at most eps: -> (bound on ||dR||_F, bound on |dt|_inf).
    A sum of n terms in any order is within n u sum|terms| of the exact sum (u = 2^-53), so two such sums differ by at most twice
    that.  Centroids: dc <= 2 u max_a sum|x_a| + u |c| (+ eps on the source side).  H: its terms move by (eps + dcs)|q| + |p| dct and
    by 4 u |p||q| of rounding, its sum by 2 n u sum|p||q|; the SVD itself is backward stable, counted as 64 u ||H||_F.  The rotation
    of the orthogonal Procrustes problem moves by at most 2 ||dH||_F / (s2 + s3), the two smallest singular values of H (the
    perturbation bound of the orthogonal polar factor).  t = ct - R cs moves by dct + ||dR|| |cs| + sqrt(3) dcs plus rounding."""
    n = len(P)
    cs, ct = P.mean(0), Q.mean(0)
    dcs = 2 * U * np.abs(P).sum(0).max() + U * np.abs(cs).max() + eps
    dct = 2 * U * np.abs(Q).sum(0).max() + U * np.abs(ct).max()
    p, q = np.abs(P - cs), np.abs(Q - ct)
    pq = p.T @ q                                   # sum |p_a||q_b|
    dH = (2 * n + 4) * U * pq + (eps + dcs) * q.sum(0)[None, :] + dct * p.sum(0)[:, None]
    H = (P - cs).T @ (Q - ct)
    s = np.linalg.svd(H, compute_uv=False)
    dHF = np.sqrt((dH * dH).sum()) + 64 * U * np.sqrt((H * H).sum())
    dR = 2 * dHF / (s[1] + s[2])
    dt = dct + dR * np.sqrt((cs * cs).sum()) + np.sqrt(3.0) * dcs + 8 * U * (np.abs(ct).max() + np.abs(cs).sum())
    return float(dR), float(dt)


def rel_small(a, b, tol):
    return abs(a - b) < tol * max(abs(b), 1e-300)


def icp(src, tgt, threshold, init=None, max_iter=20, rel_tol=1e-6, trace=None):
    """-> (T, fitness, rmse, iterations).  trace (a list) receives per evaluation a dict: T, cur, nearest, d2, sums, and margin =
    the least |d - threshold| / threshold over the source points with a neighbour in reach of 2 * threshold."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    n = len(src)

    def evaluate(T):
        cur = transform(src, T)
        d, nearest, d2 = nn(tgt, cur, threshold)
        s = icp_sums(cur, tgt, nearest, d2, threshold)
        if trace is not None:
            dd = nn(tgt, cur, 2 * threshold)[0]
            trace.append({"T": T.copy(), "cur": cur, "nearest": nearest, "d2": d2, "sums": s,
                          "margin": float(np.abs(dd - threshold).min() / threshold) if n else np.inf})
        return s, (s[0] / n if n else 0.0), (float(np.sqrt(s[1] / s[0])) if s[0] > 0 else 0.0)

    sums, fit, rmse = evaluate(T)
    it = 0
    while it < max_iter and sums[0] > 0:
        T = rigid_update(sums) @ T
        it += 1
        pf, pr = fit, rmse
        sums, fit, rmse = evaluate(T)
        if rel_small(fit, pf, rel_tol) and rel_small(rmse, pr, rel_tol):
            break
    return T, float(fit), float(rmse), it


def icp_bound(src, tgt, trace):
    """How far the final T of two ICP runs can differ when both follow the same matches at every iteration (trace of icp(), one
    entry per evaluation; entry k is the input of update k+1): -> (bound on ||dR_T||_F, bound on |dt_T|_inf).
    The update is equivariant: if the source under T is off by a rigid motion, the best update absorbs that motion exactly, so
    dT T is the best rigid map of the ORIGINAL source onto the matches whatever T was.  T's own error therefore does not
    accumulate; what does is T's departure from a rigid motion, nu, which grows by the rounding of one 4x4 product (16 u sqrt(3))
    per update and acts on the points like a position error nu |cur|, next to the transform's rounding 4 u |cur|.  The bound is
    that of the last update with this eps (update_bound), carried through dT T (||R_T||_F = sqrt(3), |t_T|), plus nu and the
    product's rounding, and doubled because each run carries its own eps."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    nu = ER = Et = 0.0
    for ev in trace[:-1]:
        inl = ev["nearest"] >= 0
        if not inl.any():
            break
        cmax = np.sqrt((ev["cur"] ** 2).sum(1)).max()
        dR, dt = update_bound(ev["cur"][inl], tgt[ev["nearest"][inl]], (4 * U + nu) * cmax)
        tT = np.sqrt((ev["T"][:3, 3] ** 2).sum())
        ER = 2 * (np.sqrt(3.0) * (dR + nu) + 16 * U)
        Et = 2 * (dR * tT + dt + (nu + 16 * U) * (1 + tT))
        nu += 16 * U * np.sqrt(3.0)
    return float(ER), float(Et)


def umeyama(src, dst, with_scale=True):
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    Uu, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Uu) * np.linalg.det(Vt) >= 0 else -1.0])
    R = Uu @ D @ Vt
    c = (S * np.diag(D)).sum() / ((a * a).sum() / len(src)) if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = md - c * R @ ms
    return T


def initial_alignment(est_poses, ref_poses, trans):
    est = np.asarray(est_poses, dtype=np.float64).reshape(-1, 4, 4)
    ref = np.asarray(ref_poses, dtype=np.float64).reshape(-1, 4, 4)
    assert len(est) == len(ref)
    return umeyama(est[:, :3, 3], ref[:, :3, 3] @ trans[:3, :3].T + trans[:3, 3])


def fscore(d_est, d_gt, tau):
    p = float((d_est < tau).mean()) if d_est.size else 0.0
    r = float((d_gt < tau).mean()) if d_gt.size else 0.0
    f = 2 * p * r / (p + r) if p + r > 0 else 0.0
    hs = [np.cumsum(np.histogram(d, bins=100, range=(0.0, 5 * tau))[0]).astype(np.float64) / max(d.size, 1) for d in (d_est, d_gt)]
    return p, r, f, hs[0], hs[1]


def score(est, gt, crp, tau, T):
    """Step 6 for a given T -> dict (precision, recall, fscore, the distances, the counts)."""
    def cropped(p):
        return p[crop(p, crp["axis"], crp["axis_min"], crp["axis_max"], crp["polygon"])]
    ec, gc = cropped(transform(est, T)), cropped(np.asarray(gt, dtype=np.float64))
    ed, gd = voxel(ec, tau / 2)[0], voxel(gc, tau / 2)[0]
    d1, d2 = nn(gd, ed, 10 * tau)[0], nn(ed, gd, 10 * tau)[0]
    p, r, f, h1, h2 = fscore(d1, d2, tau)
    return {"precision": p, "recall": r, "fscore": f, "hist_est": h1, "hist_gt": h2, "dist_est": d1, "dist_gt": d2,
            "n_est_crop": len(ec), "n_gt_crop": len(gc), "n_est_down": len(ed), "n_gt_down": len(gd)}


def eval_scene(est, gt, crp, tau, init, traces=None):
    """The whole protocol (steps 2-6).  traces (a dict) receives the ICP trace of every stage."""
    est, gt = np.asarray(est, dtype=np.float64).reshape(-1, 3), np.asarray(gt, dtype=np.float64).reshape(-1, 3)
    T = np.array(init, dtype=np.float64)
    res = {"tau": tau, "T_init": T.copy(), "n_est": len(est), "n_gt": len(gt)}
    sT, sf, sr, si = [], [], [], []
    for name, vox, thr in (("A", tau, 80 * tau), ("B", tau / 2, 20 * tau), ("C", None, 2 * tau)):
        s = transform(est, T)
        s = s[crop(s, crp["axis"], crp["axis_min"], crp["axis_max"], crp["polygon"])]
        res[f"n_crop_{name}"] = len(s)
        s = voxel(s, vox)[0] if vox is not None else s[::max(int(round(len(s) / 4e6)), 1)]
        res[f"n_down_{name}"] = len(s)
        tr = [] if traces is not None else None
        dT, fit, rmse, its = icp(s, gt, thr, trace=tr)
        if traces is not None:
            traces[name] = tr
        T = dT @ T
        sT.append(T.copy()); sf.append(fit); sr.append(rmse); si.append(its)
    res.update(score(est, gt, crp, tau, T))
    res.update(T=T, stage_T=np.stack(sT), stage_fitness=np.array(sf), stage_rmse=np.array(sr), stage_iterations=np.array(si))
    return res


def undecided(d, tau, rel=1e-6):
    """How many distances lie within rel * tau of tau (the band inside which precision / recall may differ)."""
    return int((np.abs(np.asarray(d) - tau) <= rel * tau).sum())


# ---------------------------------------------------------------------------------------------------- the fixture scene
def fixture_scene(seed=0, n_gt=50000, n_est=45000, tau=0.01):
    """A curved surface sampled as ground truth; an estimate covering part of it with noise near 0.7 tau, a few percent of uniform
    outliers and a rigid offset of a few tau; a polygon crop (orthogonal axis Y, as the real scenes) that cuts both clouds;
    a camera ring for the initial alignment.  -> dict."""
    rng = np.random.RandomState(seed)

    def surface(u, v):
        return np.stack([u, 0.15 * np.sin(3 * u) * np.cos(2 * v) + 0.05 * u * v, v], 1)

    side = 1.2
    gu, gv = rng.uniform(-side, side, n_gt), rng.uniform(-side, side, n_gt)
    gt = surface(gu, gv)
    n_out = n_est // 25
    eu, ev = rng.uniform(-side, 0.5 * side, n_est - n_out), rng.uniform(-0.8 * side, side, n_est - n_out)
    est = surface(eu, ev) + rng.normal(0, 0.7 * tau / np.sqrt(3.0), (n_est - n_out, 3))
    est = np.concatenate([est, rng.uniform(-side, side, (n_out, 3)) * [1, 0.4, 1]])
    est = est[rng.permutation(len(est))]
    # the estimate lives in its own frame: a similarity away from the ground truth's, plus a rigid offset of a few tau that the
    # camera-based alignment does not see (the ICP has to find it)
    ang = 0.004
    off = np.eye(4)
    off[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    off[:3, 3] = [2.5 * tau, -1.5 * tau, 2.0 * tau]
    a, b, sc = 0.7, -0.4, 1.7
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    S = np.eye(4)                                   # estimate frame -> ground-truth frame
    S[:3, :3] = sc * Rz @ Rx
    S[:3, 3] = [0.3, -0.2, 0.5]
    Sinv = np.linalg.inv(S)
    est_own = transform(transform(est, np.linalg.inv(off)), Sinv)        # S est_own = off^-1 est: off is left for the ICP
    ncam = 24
    th = np.linspace(0, 2 * np.pi, ncam, endpoint=False)
    centres = np.stack([2.5 * np.cos(th), 1.5 + 0.2 * np.sin(3 * th), 2.5 * np.sin(th)], 1)
    trans = np.eye(4)
    trans[:3, :3] = Rx.T
    trans[:3, 3] = [0.1, 0.0, -0.3]
    tinv = np.linalg.inv(trans)
    ref_poses = np.tile(np.eye(4), (ncam, 1, 1))
    ref_poses[:, :3, 3] = transform(centres, tinv)              # trans maps them onto `centres`
    est_poses = np.tile(np.eye(4), (ncam, 1, 1))
    est_poses[:, :3, 3] = transform(centres, Sinv)
    poly3 = np.array([[-1.0, 0.0, -0.9], [0.2, 0.0, -1.05], [0.9, 0.0, -0.4], [0.75, 0.0, 0.8], [-0.1, 0.0, 0.55], [-0.95, 0.0, 0.9]])
    crp = {"axis": 1, "axis_min": -0.12, "axis_max": 0.3, "polygon": np.ascontiguousarray(poly3[:, [0, 2]]), "polygon3": poly3}
    return {"est": est_own, "gt": gt, "crop": crp, "tau": tau, "trans": trans, "ref_poses": ref_poses, "est_poses": est_poses,
            "S": S, "off": off}


def write_tanks_tree(data, ply, traj, scenes):
    """{scene: fixture_scene dict} -> the files the driver reads (PLYs by write_ply, the rest by the new writers)."""
    from tools.data_io import write_crop_json, write_matrix_txt, write_ply, write_trajectory_log
    os.makedirs(ply, exist_ok=True)
    os.makedirs(traj, exist_ok=True)
    for name, sc in scenes.items():
        d = os.path.join(data, name)
        os.makedirs(d, exist_ok=True)
        write_ply(os.path.join(ply, f"{name}.ply"), sc["est"], np.zeros((len(sc["est"]), 3), dtype=np.uint8))
        write_ply(os.path.join(d, f"{name}.ply"), sc["gt"], np.zeros((len(sc["gt"]), 3), dtype=np.uint8))
        write_crop_json(os.path.join(d, f"{name}.json"), sc["crop"]["axis"], sc["crop"]["axis_min"], sc["crop"]["axis_max"],
                        sc["crop"]["polygon3"])
        write_matrix_txt(os.path.join(d, f"{name}_trans.txt"), sc["trans"])
        write_trajectory_log(os.path.join(d, f"{name}_COLMAP_SfM.log"), sc["ref_poses"])
        write_trajectory_log(os.path.join(traj, f"{name}.log"), sc["est_poses"])
