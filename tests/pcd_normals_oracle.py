"""Oracle of the point-cloud post-processing (k nearest neighbours, normal estimation, neighbour spacing, the
colour rule of the voxel grid): numpy fp64 elementwise arithmetic and brute force.

Distances are d^2 = ((dx*dx) + dy*dy) + dz*dz (numpy never contracts elementwise products into fmas), the formula the kernels
use; neighbours are ordered by ascending (d^2, index), a total order.  The covariance sums run through np.add.accumulate, which
adds sequentially, in that neighbour order, so the kernels' covariance compares bit for bit.  The eigenvector comes from
numpy.linalg.eigh: the kernels' solver differs, and is held to eigh's own residual."""
import numpy as np

KNN = 30            # the default neighbour count of the reference's estimate_normals()


# ---------------------------------------------------------------------------------------------------- the test clouds
def f32(pts):
    """Round through fp32, as pcd_fuse's points are."""
    return np.ascontiguousarray(np.asarray(pts, dtype=np.float32).astype(np.float64))


def surface(n, scale, offset, seed=0):
    """z = 0.2 sin 3x + 0.01 noise over [-1, 1]^2, scaled and offset."""
    rng = np.random.RandomState(seed)
    xy = rng.uniform(-1, 1, (n, 2))
    z = 0.2 * np.sin(3 * xy[:, 0]) + 0.01 * rng.standard_normal(n)
    return f32(np.column_stack([xy, z]) * scale + np.asarray(offset, dtype=np.float64))


def dtu_surface(n=3000, seed=0):
    return surface(n, 60.0, (100.0, -50.0, 650.0), seed)


def tanks_surface(n=3000, seed=1):
    return surface(n, 2.0, (0.3, -1.0, 4.0), seed)


def lattice(nx=12, ny=12, nz=5):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return f32(g)


def degenerate(seed=2):
    """5 points repeated 20 times each (interleaved, so duplicates are far apart in the input), then 100 collinear points."""
    rng = np.random.RandomState(seed)
    five = rng.uniform(-1, 1, (5, 3))
    t = np.sort(rng.uniform(0, 4, 100))
    line = np.array([2.0, 0.5, -1.0]) + t[:, None] * np.array([1.0, 2.0, 0.5])
    return f32(np.concatenate([np.tile(five, (20, 1)), line]))


def ragged(n, seed=3):
    rng = np.random.RandomState(seed + n)
    return f32(rng.uniform(-1, 1, (n, 3)) * 5.0 + np.array([1.0, 2.0, 30.0]))


# ---------------------------------------------------------------------------------------------------- k nearest neighbours
def dist2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def knn(pts, queries, k, chunk=512):
    """Brute force: -> (nbr [m,k] int32, d2 [m,k]); row i = the min(k, n) nearest of pts to queries[i] in ascending (d^2, index)
    order, padded with -1 / +inf."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    n, m = len(pts), len(q)
    ke = min(k, n)
    nbr = np.full((m, k), -1, dtype=np.int32)
    d2o = np.full((m, k), np.inf)
    if ke == 0:
        return nbr, d2o
    for lo in range(0, m, chunk):
        d2 = dist2(pts[None, :, :], q[lo:lo + chunk, None, :])               # [c, n]
        if n <= 4 * k:
            order = np.argsort(d2, axis=1, kind="stable")[:, :ke]            # stable: equal d^2 keep ascending index
            nbr[lo:lo + chunk, :ke] = order
            d2o[lo:lo + chunk, :ke] = np.take_along_axis(d2, order, 1)
            continue
        kth = np.partition(d2, ke - 1, axis=1)[:, ke - 1]
        for r in range(len(d2)):
            cand = np.nonzero(d2[r] <= kth[r])[0]                            # ascending index
            cand = cand[np.argsort(d2[r, cand], kind="stable")][:ke]
            nbr[lo + r, :ke] = cand
            d2o[lo + r, :ke] = d2[r, cand]
    return nbr, d2o


def knn_slab(pts, queries, k, width, radius):
    """knn() for a large cloud, still brute force but over a slab: only the points with |x - qx| <= width are looked at, and every
    query must have k of them at d^2 < radius^2 with radius < width (asserted), so no point outside the slab (d^2 >= about
    width^2) can be among its k nearest.  test_pcd_normals_cpu.py ties it to knn()."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    assert radius <= 0.99 * width
    order = np.argsort(pts[:, 0], kind="stable")
    xs = pts[order, 0]
    lo = np.searchsorted(xs, q[:, 0] - width, "left")
    hi = np.searchsorted(xs, q[:, 0] + width, "right")
    nbr = np.empty((len(q), k), dtype=np.int32)
    d2o = np.empty((len(q), k))
    for i in range(len(q)):
        cand = np.sort(order[lo[i]:hi[i]])                                   # ascending index
        d2 = dist2(pts[cand], q[i])
        assert int((d2 < radius * radius).sum()) >= k, "the slab does not prove the neighbours: widen it"
        o = np.argsort(d2, kind="stable")[:k]
        nbr[i], d2o[i] = cand[o], d2[o]
    return nbr, d2o


def tie_fraction(pts, k):
    """Fraction of self-queries whose k-th and (k+1)-th neighbour lie at the same d^2 (the index decides who is in)."""
    _, d2 = knn(pts, pts, k + 1)
    return float(np.mean(d2[:, k - 1] == d2[:, k]))


# ---------------------------------------------------------------------------------------------------- covariance, normals
def covariance(pts, nbr):
    """[m,6] xx, xy, xz, yy, yz, zz: nine sequential sums over the row's neighbours in order, / k_eff, C_ab = E[ab] - E[a] E[b]."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    ke = int((nbr[0] >= 0).sum()) if len(nbr) else 0
    p = pts[nbr[:, :ke]]                                                     # [m, ke, 3]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    seq = lambda v: np.add.accumulate(v, axis=1)[:, -1] / ke                 # ((0 + v0) + v1) + ...
    ex, ey, ez = seq(x), seq(y), seq(z)
    return np.stack([seq(x * x) - ex * ex, seq(x * y) - ex * ey, seq(x * z) - ex * ez, seq(y * y) - ey * ey, seq(y * z) - ey * ez,
                     seq(z * z) - ez * ez], 1)


def sym(c6):
    c6 = np.asarray(c6, dtype=np.float64)
    return np.stack([np.stack([c6[:, 0], c6[:, 1], c6[:, 2]], 1), np.stack([c6[:, 1], c6[:, 3], c6[:, 4]], 1),
                     np.stack([c6[:, 2], c6[:, 4], c6[:, 5]], 1)], 1)


def eigh_smallest(c6):
    """-> (eigenvalue [m], unit eigenvector [m,3]) of the smallest eigenvalue, by numpy.linalg.eigh."""
    w, v = np.linalg.eigh(sym(c6))
    return w[:, 0], v[:, :, 0]


def residual(c6, nrm):
    """-> (||C n - (n^T C n) n|| / ||C||_F [m], the Rayleigh quotient n^T C n [m], ||C||_F [m]); a row with ||C||_F == 0 has
    residual 0."""
    C = sym(c6)
    fro = np.sqrt((C * C).sum((1, 2)))
    cn = np.einsum("mab,mb->ma", C, nrm)
    ray = (nrm * cn).sum(1)
    r = np.linalg.norm(cn - ray[:, None] * nrm, axis=1)
    safe = np.where(fro > 0, fro, 1.0)
    return np.where(fro > 0, r / safe, 0.0), ray, fro


def _rotate(A, V, p, q, r):
    apq = A[:, p, q].copy()
    with np.errstate(all="ignore"):
        theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
        t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    t = np.where(apq != 0, t, 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    A[:, p, p] -= h
    A[:, q, q] += h
    A[:, p, q] = A[:, q, p] = 0.0
    rp, rq = A[:, r, p].copy(), A[:, r, q].copy()
    A[:, r, p] = A[:, p, r] = c * rp - s * rq
    A[:, r, q] = A[:, q, r] = s * rp + c * rq
    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
    V[:, :, p] = c[:, None] * vp - s[:, None] * vq
    V[:, :, q] = s[:, None] * vp + c[:, None] * vq


def jacobi_smallest(c6, sweeps=6):
    """The method of the kernel, restated (not its bit pattern: the tests hold the kernel to eigh's residual, not to this): cyclic
    Jacobi, `sweeps` sweeps over (0,1), (0,2), (1,2), the column of the smallest diagonal entry (the first among equals),
    normalised.  -> unit vectors [m,3]."""
    A = sym(c6).copy()
    V = np.tile(np.eye(3), (len(A), 1, 1))
    for _ in range(sweeps):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    d = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1)
    use1 = d[:, 1] < d[:, 0]
    lam = np.where(use1, d[:, 1], d[:, 0])
    pick = np.where(d[:, 2] < lam, 2, np.where(use1, 1, 0))
    n = V[np.arange(len(A)), :, pick]
    return n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]


def orient(nrm, dirs):
    """Keep n where ((nx*dx) + ny*dy) + nz*dz > 0 (dirs fp32 widened), negate elsewhere: an exact 0 negates."""
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64)
    s = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]
    return np.where((s > 0)[:, None], nrm, -nrm)


def normals(pts, dirs=None, k=KNN):
    """-> (normals [n,3], cov [n,6]): eigh's smallest eigenvector, (0, 0, 1) when min(k, n) < 3, oriented by dirs when given."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    nbr, _ = knn(pts, pts, k)
    c6 = covariance(pts, nbr)
    if min(k, len(pts)) >= 3:
        nrm = eigh_smallest(c6)[1]
    else:
        nrm = np.tile(np.array([0.0, 0.0, 1.0]), (len(pts), 1))
    return (orient(nrm, dirs) if dirs is not None else nrm), c6


# ---------------------------------------------------------------------------------------------------- spacing, voxel size, colours
def nn_spacing(pts):
    """The distance to the second entry of a k = 2 self-query (0 for a duplicated point)."""
    return np.sqrt(knn(pts, pts, 2)[1][:, 1])


def percentile90(v):
    """numpy.percentile(v, 90) (linear), spelled out: position 0.9 (M - 1), then numpy's two-sided lerp."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    m = len(s)
    pos = (m - 1) * (90 / 100)
    lo = int(np.floor(pos))
    t = pos - lo
    lo, hi = min(max(lo, 0), m - 1), min(max(lo + 1, 0), m - 1)
    a, b = float(s[lo]), float(s[hi])
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def colour_attrs(rgb):
    """uint8 [n,3] -> the reference's colours: fp32(u8) / fp32(255), widened to fp64."""
    return (np.asarray(rgb, dtype=np.uint8).astype(np.float32) / np.float32(255)).astype(np.float64)


def colour_u8(mean):
    """uint8(round_half_away(clamp(mean, 0, 1) * 255))."""
    v = np.clip(np.asarray(mean, dtype=np.float64), 0.0, 1.0) * 255.0
    r = np.floor(v)
    return (r + ((v - r) >= 0.5)).astype(np.uint8)
