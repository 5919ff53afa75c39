"""Oracle of the scene-import kernels (include/mdfnet_hip.h, "Scene import from a sparse model"): a plain numpy restatement with
explicit loops in the stated order (no np.sum, no @), every operation rounded once in `dtype`.  The same code runs in np.float64
(what the kernels compute; the integer outputs, the ranges and the camera centres must match it bit for bit) and in np.longdouble
(the yardstick of the scores, whose atan2 / exp differ between the device's and the host's libm).  Also the seeded scene
generator the tests share."""
import numpy as np

DEGREES = 57.29577951308232


def centres(rot, trans, dtype=np.float64):
    """c_i[a] = -(((R_i[0][a] t_i[0]) + R_i[1][a] t_i[1]) + R_i[2][a] t_i[2]) -> [N,3]."""
    R, t = np.asarray(rot, dtype=dtype).reshape(-1, 3, 3), np.asarray(trans, dtype=dtype).reshape(-1, 3)
    c = np.zeros((len(R), 3), dtype=dtype)
    for i in range(len(R)):
        for a in range(3):
            c[i, a] = -(((R[i, 0, a] * t[i, 0]) + R[i, 1, a] * t[i, 1]) + R[i, 2, a] * t[i, 2])
    return c


def valid_tracks(track_off, track_img, n_img):
    """Per point: True when its offsets lie inside [0, n_obs] and ascend and its image indices lie inside [0, n_img) and ascend
    strictly.  A track that fails is skipped as a whole."""
    off, img = np.asarray(track_off, dtype=np.int64), np.asarray(track_img, dtype=np.int64)
    ok = np.zeros(len(off) - 1, dtype=bool)
    for p in range(len(ok)):
        lo, hi = off[p], off[p + 1]
        if lo < 0 or hi < lo or hi > len(img):
            continue
        tr = img[lo:hi]
        ok[p] = bool(np.all((tr >= 0) & (tr < n_img)) and np.all(tr[1:] > tr[:-1]))
    return ok


def orderable(x):
    """The total order of the depths: the bits of a double, sign bit flipped for positive values, all bits for negative ones."""
    b = np.asarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def depth_ranges(rot, trans, pts, track_off, track_img, q_lo=0.01, q_hi=0.99):
    """-> range [N,2] float64 (NaN for an image without observations), count [N] int32, depths (list of N arrays, CSR order)."""
    R, t = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3), np.asarray(trans, dtype=np.float64).reshape(-1, 3)
    P = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(R)
    ok = valid_tracks(track_off, track_img, n)
    depths = [[] for _ in range(n)]
    for p in range(len(P)):
        if not ok[p]:
            continue
        for o in range(track_off[p], track_off[p + 1]):
            i = int(track_img[o])
            depths[i].append((((R[i, 2, 0] * P[p, 0]) + R[i, 2, 1] * P[p, 1]) + R[i, 2, 2] * P[p, 2]) + t[i, 2])
    rng = np.full((n, 2), np.nan, dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    for i in range(n):
        d = np.array(depths[i], dtype=np.float64)
        depths[i] = d
        cnt[i] = len(d)
        if len(d):
            s = d[np.argsort(orderable(d), kind="stable")]
            rng[i, 0] = s[min(int(np.float64(q_lo) * np.float64(len(d))), len(d) - 1)]
            rng[i, 1] = s[min(int(np.float64(q_hi) * np.float64(len(d))), len(d) - 1)]
    return rng, cnt, depths


def angle_deg(ci, cj, p, dtype=np.float64):
    """theta of one (image pair, point), in degrees, as the kernel states it."""
    u = [ci[a] - p[a] for a in range(3)]
    v = [cj[a] - p[a] for a in range(3)]
    cx = u[1] * v[2] - u[2] * v[1]
    cy = u[2] * v[0] - u[0] * v[2]
    cz = u[0] * v[1] - u[1] * v[0]
    s = np.sqrt(((cx * cx) + cy * cy) + cz * cz)
    d = ((u[0] * v[0]) + u[1] * v[1]) + u[2] * v[2]
    return np.arctan2(s, d) * dtype(DEGREES)


def scores(rot, trans, pts, track_off, track_img, theta0=5.0, sigma1=1.0, sigma2=10.0, dtype=np.float64):
    """-> score [N,N] dtype (symmetric, zero diagonal), shared [N,N] int32."""
    c = centres(rot, trans, dtype)
    P = np.asarray(pts, dtype=dtype).reshape(-1, 3)
    n = len(c)
    ok = valid_tracks(track_off, track_img, n)
    th0, s1, s2, two = dtype(theta0), dtype(sigma1), dtype(sigma2), dtype(2.0)
    score = np.zeros((n, n), dtype=dtype)
    shared = np.zeros((n, n), dtype=np.int32)
    for p in range(len(P)):                           # ascending point index: the order of every pair's sum
        if not ok[p]:
            continue
        tr = [int(x) for x in track_img[track_off[p]:track_off[p + 1]]]
        for a in range(len(tr)):
            for b in range(a + 1, len(tr)):
                i, j = tr[a], tr[b]
                theta = angle_deg(c[i], c[j], P[p], dtype)
                e = theta - th0
                sigma = s1 if theta <= th0 else s2
                term = np.exp(-(e * e) / ((two * sigma) * sigma))
                score[i, j] = score[i, j] + term
                shared[i, j] += 1
    for i in range(n):
        for j in range(i + 1, n):
            score[j, i] = score[i, j]
            shared[j, i] = shared[i, j]
    return score, shared


def n_records(track_off):
    t = np.diff(np.asarray(track_off, dtype=np.int64))
    return int((t * (t - 1) // 2).sum())


def rank_gap(score, sources):
    """The smallest relative gap between scores the selection compares: consecutive selected sources of a row, and the last
    selected one against the best one left out."""
    gap = np.inf
    n = score.shape[0]
    for i in range(n):
        rest = [j for j in range(n) if j != i and j not in set(int(x) for x in sources[i])]
        chain = [float(score[i, j]) for j in sources[i]]
        if rest:
            chain.append(max(float(score[i, j]) for j in rest))
        for a, b in zip(chain[:-1], chain[1:]):
            gap = min(gap, (a - b) / a if a > 0 else 0.0)
    return gap


# ---------------------------------------------------------------------------------------------------- scenes
def look_at(centre, target, up=(0.0, 0.0, 1.0)):
    """World -> camera rotation of a camera at `centre` looking at `target` (z forward, x right, y down) and its translation."""
    f = np.asarray(target, dtype=np.float64) - centre
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    return R, -R @ centre


def make_scene(n_img, n_pts, seed, arc_deg=120.0, radius=5.0, window=3, drop=0.3):
    """Cameras on a partial ring around the origin, looking at a point cloud there; every point is visible in a window of
    neighbouring cameras around a random one, with random drop-outs.
    -> rot [N,3,3], trans [N,3], pts [P,3] float64, track_off [P+1] int64, track_img [T] int32 (ascending inside a track)."""
    rng = np.random.RandomState(seed)
    rot, trans = np.zeros((n_img, 3, 3)), np.zeros((n_img, 3))
    for i in range(n_img):
        a = np.deg2rad(arc_deg) * (i / max(n_img - 1, 1) - 0.5) + rng.uniform(-0.01, 0.01)
        c = np.array([radius * np.cos(a), radius * np.sin(a), rng.uniform(-0.3, 0.3)])
        rot[i], trans[i] = look_at(c, rng.uniform(-0.1, 0.1, 3))
    pts = rng.normal(0.0, 0.6, (n_pts, 3))
    off, img = [0], []
    for p in range(n_pts):
        k = rng.randint(0, n_img)
        seen = [i for i in range(max(k - window, 0), min(k + window, n_img - 1) + 1) if rng.uniform() >= drop]
        img += seen
        off.append(len(img))
    return rot, trans, pts, np.array(off, dtype=np.int64), np.array(img, dtype=np.int32)


def tracks_from_lists(lists):
    off, img = [0], []
    for tr in lists:
        img += list(tr)
        off.append(len(img))
    return np.array(off, dtype=np.int64), np.array(img, dtype=np.int32)
