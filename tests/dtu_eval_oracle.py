"""Oracle of the DTU point-cloud evaluation: the MATLAB scorer (BaseEvalMain_web.m, PointCompareMain.m, reducePts_haa.m,
MaxDistCP.m, ComputeStat_web.m) restated in numpy fp64 elementwise arithmetic, no scipy.

Distances are d^2 = ((dx*dx) + dy*dy) + dz*dz (numpy never contracts elementwise products into fmas), d = sqrt(d^2): the formula
the kernels use, so distances compare bit for bit.  Two restatements of MaxDistCP are here: the literal box loop (max_dist_cp)
and "exact nearest neighbour + region + cap" (nn_capped), the formulation the kernel implements; the CPU tests prove they agree
below the cap."""
import os

import numpy as np

USED_SETS = [1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118]


def dist2(a, b):
    """a [k,3], b [k,3] (or broadcastable) -> d^2 [k]"""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _nn_d2(to, frm, chunk=2048):
    """exact min d^2 from every frm point to the to set (inf when to is empty), brute force in chunks"""
    out = np.full(len(frm), np.inf)
    if len(to) == 0:
        return out
    step = max(1, (1 << 22) // max(1, len(to)))
    for s in range(0, len(frm), min(chunk, step)):
        f = frm[s:s + min(chunk, step)]
        out[s:s + len(f)] = dist2(f[:, None, :], to[None, :, :]).min(1)
    return out


def in_region(frm, bb, cap):
    """The union of MaxDistCP's cubes: on each axis some k in 0..floor((BB2-BB1)/cap) with fl(BB1 + k*cap) <= f < fl(low + cap)."""
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    ok = np.ones(len(frm), dtype=bool)
    for a in range(3):
        rng = np.floor((bb[1, a] - bb[0, a]) / cap)
        f = frm[:, a]
        with np.errstate(invalid="ignore"):
            k0 = np.floor((f - bb[0, a]) / cap)
        hit = np.zeros(len(frm), dtype=bool)
        for dk in (-1, 0, 1):
            k = k0 + dk
            low = bb[0, a] + k * cap
            high = low + cap
            hit |= (k >= 0) & (k <= rng) & (f >= low) & (f < high)
        ok &= hit
    return ok


def nn_capped(to, frm, bb, cap):
    """D = exact nearest-neighbour distance if the from-point lies in the region (bb None: everywhere) and d < cap, else cap."""
    to = np.asarray(to, dtype=np.float64).reshape(-1, 3)
    frm = np.asarray(frm, dtype=np.float64).reshape(-1, 3)
    d = np.sqrt(_nn_d2(to, frm))
    out = np.where(d < cap, d, cap)
    if bb is not None:
        out[~in_region(frm, bb, cap)] = cap
    return out


def max_dist_cp(Qto, Qfrom, BB, MaxDist):
    """The literal loop of MaxDistCP.m (points as rows): cubes of side MaxDist from BB(1,:), the to-points of the cube widened by
    MaxDist on every side searched brute force; Dist keeps MaxDist where no cube holds the point or its widened cube is empty."""
    Qto = np.asarray(Qto, dtype=np.float64).reshape(-1, 3)
    Qfrom = np.asarray(Qfrom, dtype=np.float64).reshape(-1, 3)
    BB = np.asarray(BB, dtype=np.float64).reshape(2, 3)
    Dist = np.full(len(Qfrom), float(MaxDist))
    Range = np.floor((BB[1] - BB[0]) / MaxDist).astype(np.int64)
    for x in range(Range[0] + 1):
        for y in range(Range[1] + 1):
            for z in range(Range[2] + 1):
                Low = BB[0] + np.array([x, y, z], dtype=np.float64) * MaxDist
                High = Low + MaxDist
                idxF = np.nonzero((Qfrom >= Low).all(1) & (Qfrom < High).all(1))[0]
                Low = Low - MaxDist
                High = High + MaxDist
                SQto = Qto[(Qto >= Low).all(1) & (Qto < High).all(1)]
                if len(SQto) == 0:
                    Dist[idxF] = MaxDist
                else:
                    Dist[idxF] = np.sqrt(_nn_d2(SQto, Qfrom[idxF]))
    return Dist


def neighbours(pts, dst):
    """CSR (offsets [n+1], idx) of every j != i with d(i, j) <= dst, from a grid hash of cell side dst plus the exact test."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    if n == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cell = np.floor((pts - pts.min(0)) / dst).astype(np.int64)
    dims = cell.max(0) + 3
    key = ((cell[:, 0] + 1) * dims[1] + (cell[:, 1] + 1)) * dims[2] + (cell[:, 2] + 1)
    srt = np.argsort(key, kind="stable")
    ks = key[srt]
    ii, jj = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                target = key + (ox * dims[1] + oy) * dims[2] + oz
                lo = np.searchsorted(ks, target, "left")
                hi = np.searchsorted(ks, target, "right")
                cnt = hi - lo
                src = np.repeat(np.arange(n), cnt)
                start = np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
                dst_idx = srt[start + np.arange(cnt.sum())]
                ok = (src != dst_idx) & (np.sqrt(dist2(pts[src], pts[dst_idx])) <= dst)
                ii.append(src[ok])
                jj.append(dst_idx[ok])
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    o = np.lexsort((jj, ii))
    ii, jj = ii[o], jj[o]
    offs = np.zeros(n + 1, dtype=np.int64)
    np.add.at(offs, ii + 1, 1)
    return np.cumsum(offs), jj


def reduce_pts(pts, dst, order):
    """reducePts_haa.m with the visiting order `order` (RandOrd): the literal sequential loop.  -> keep mask [n] bool."""
    offs, idx = neighbours(pts, dst)
    keep = np.ones(len(offs) - 1, dtype=bool)
    for i in np.asarray(order, dtype=np.int64):
        if keep[i]:
            keep[idx[offs[i]:offs[i + 1]]] = False
            keep[i] = True
    return keep


def matlab_round(x):
    """MATLAB's round: halves away from zero"""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def data_in_mask(Qdata, ObsMask, BB, Res):
    """PointCompareMain.m: Qv = round((Qdata - BB(1,:)) / Res + 1); in mask iff inside [1, size] and ObsMask(Qv) (1-based,
    column-major).  Qdata as rows."""
    Q = np.asarray(Qdata, dtype=np.float64).reshape(-1, 3)
    BB = np.asarray(BB, dtype=np.float64).reshape(2, 3)
    Qv = matlab_round((Q - BB[0]) / Res + 1)
    s = np.asarray(ObsMask).shape
    ok = np.ones(len(Q), dtype=bool)
    for a in range(3):
        ok &= (Qv[:, a] > 0) & (Qv[:, a] <= s[a])
    out = np.zeros(len(Q), dtype=bool)
    v = Qv[ok].astype(np.int64) - 1
    out[ok] = np.asarray(ObsMask, dtype=bool)[v[:, 0], v[:, 1], v[:, 2]]
    return out


def stl_above_plane(Qstl, P):
    Q = np.asarray(Qstl, dtype=np.float64).reshape(-1, 3)
    P = np.asarray(P, dtype=np.float64).reshape(4)
    return ((P[0] * Q[:, 0] + P[1] * Q[:, 1]) + P[2] * Q[:, 2]) + P[3] > 0


def stat(d):
    """(count, mean, var (n-1), median) of ComputeStat_web.m; NaN for [] as MATLAB, var 0 for one value"""
    d = np.sort(np.asarray(d, dtype=np.float64).reshape(-1))
    n = len(d)
    if n == 0:
        return 0, float("nan"), float("nan"), float("nan")
    mean = float(np.mean(d))
    var = float(np.sum((d - mean) ** 2) / (n - 1)) if n > 1 else 0.0
    med = float(d[n // 2]) if n % 2 else float((d[n // 2 - 1] + d[n // 2]) / 2)
    return n, mean, var, med


def eval_scan(qdata, qstl, obs_mask, bb, res, plane, dst=0.2, seed=0, max_dist=20.0):
    """PointCompareMain.m + the statistics, with the visiting order numpy.random.RandomState(seed).permutation(n)."""
    q = np.asarray(qdata, dtype=np.float64).reshape(-1, 3)
    s = np.asarray(qstl, dtype=np.float64).reshape(-1, 3)
    keep = reduce_pts(q, dst, np.random.RandomState(seed).permutation(len(q)))
    qr = q[keep]
    ddata = nn_capped(s, qr, bb, 60.0)
    dstl = nn_capped(qr, s, bb, 60.0)
    inm = data_in_mask(qr, obs_mask, bb, res)
    above = stl_above_plane(s, plane)
    dd, ds = ddata[inm], dstl[above]
    nd, md, vd, medd = stat(dd[dd < max_dist])
    ns, ms, vs, meds = stat(ds[ds < max_dist])
    return {"Qdata": qr.T, "Ddata": ddata, "Qstl": s.T, "Dstl": dstl, "DataInMask": inm, "StlAbovePlane": above,
            "nData": nd, "MeanData": md, "VarData": vd, "MedData": medd, "nStl": ns, "MeanStl": ms, "VarStl": vs, "MedStl": meds}


def write_dtu_tree(data_path, ply_path, scenes, method="ours", light="l3"):
    """Write the files the scorer reads for {scan: scene} (scenes as mdfnet_hip.synth.dtu_eval_scene returns them):
    {data}/Points/stl/stl{scan:03d}_total.ply, {data}/ObsMask/ObsMask{scan}_10.mat (ObsMask, BB, Res),
    {data}/ObsMask/Plane{scan}.mat (P) and {ply}/{method}{scan:03d}_{light}.ply."""
    from tools.data_io import write_mat, write_ply
    os.makedirs(os.path.join(data_path, "Points", "stl"), exist_ok=True)
    os.makedirs(os.path.join(data_path, "ObsMask"), exist_ok=True)
    os.makedirs(ply_path, exist_ok=True)
    for scan, sc in scenes.items():
        write_ply(os.path.join(data_path, "Points", "stl", f"stl{scan:03d}_total.ply"), sc["qstl"].astype(np.float32),
                  np.zeros((len(sc["qstl"]), 3), np.uint8))
        write_mat(os.path.join(data_path, "ObsMask", f"ObsMask{scan}_10.mat"), {"ObsMask": sc["obs_mask"], "BB": sc["bb"],
                                                                                "Res": np.float64(sc["res"])})
        write_mat(os.path.join(data_path, "ObsMask", f"Plane{scan}.mat"), {"P": np.asarray(sc["plane"], np.float64).reshape(4, 1)})
        write_ply(os.path.join(ply_path, f"{method}{scan:03d}_{light}.ply"), sc["qdata"], np.zeros((len(sc["qdata"]), 3), np.uint8))
