"""Independent numpy oracle of the meshing kernels (csrc/tsdf_mesh.hip; DESIGN section 7 "TSDF meshing"): an fp32 mirror of the
TSDF integration (one correctly rounded numpy operation per kernel operation, same order), the same definitions in float64,
marching tetrahedra over the Kuhn split, the vertex colouring, and the synthetic scenes the tests share.

Volume: dims = (nx, ny, nz) lattice points, x fastest, arrays [nz, ny, nx]; point (i,j,k) sits at origin + voxel * (i,j,k).
A view: K [3,3], E [4,4] (p_cam = E[:3,:3] x + E[:3,3]), a depth map [h,w]; pixel centres are integers."""
import numpy as np

F = np.float32
CORNERS = [(c & 1, c >> 1 & 1, c >> 2 & 1) for c in range(8)]
# the six tetrahedra (0, a, a|b, 7) for the permutations (a, b, c) of (1, 2, 4), lexicographic in (a, b); odd = negatively oriented
TETS = [((0, a, a | b, 7), odd) for a, b, odd in ((1, 2, False), (1, 4, True), (2, 1, True), (2, 4, False), (4, 1, False), (4, 2, True))]


def lattice_points(origin, voxel, dims, dt):
    nx, ny, nz = dims
    o, s = np.asarray(origin, dt), dt(voxel)
    x = o[0] + s * np.arange(nx, dtype=dt)
    y = o[1] + s * np.arange(ny, dtype=dt)
    z = o[2] + s * np.arange(nz, dtype=dt)
    return np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None])


def project(K, E, x, y, z, h, w, dt):
    """-> (ok, u, v, pz): ok = in front of the camera, finite, on the map; u, v int64 (valid where ok)."""
    K, E = np.asarray(K, dt), np.asarray(E, dt)
    with np.errstate(all="ignore"):
        p = [((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)]
        ok = (p[2] > 0) & np.isfinite(p[2])
        u = np.floor((K[0, 0] * p[0] / p[2] + K[0, 2]) + dt(0.5))
        v = np.floor((K[1, 1] * p[1] / p[2] + K[1, 2]) + dt(0.5))
        ok = ok & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    ui = np.where(ok, u, 0).astype(np.int64)
    vi = np.where(ok, v, 0).astype(np.int64)
    return ok, ui, vi, p[2]


def integrate(depths, Ks, Es, origin, voxel, dims, trunc, dt=F, state=None, trace=None):
    """-> (D, W) [nz,ny,nx] of dtype dt.  dt=float32 mirrors the kernel bit for bit; dt=float64 evaluates the same definitions from
    the same fp32 inputs.  trace: a list that receives per view (ok-and-used mask, u, v) for the tie analysis."""
    nx, ny, nz = dims
    x, y, z = lattice_points(origin, voxel, dims, dt)
    D = np.zeros((nz, ny, nx), dt) if state is None else np.array(state[0], dt)
    W = np.zeros((nz, ny, nx), dt) if state is None else np.array(state[1], dt)
    tau = dt(F(trunc))
    for dep, K, E in zip(depths, Ks, Es):
        dep = np.asarray(dep, F)
        h, w = dep.shape
        ok, u, v, pz = project(np.asarray(K, F), np.asarray(E, F), x, y, z, h, w, dt)
        with np.errstate(all="ignore"):
            d = dep[v, u].astype(dt)
            ok = ok & np.isfinite(d) & (d > 0)
            sdf = d - pz
            ok = ok & ~(sdf < -tau)
            f = np.minimum(dt(1), sdf / tau)
            w1 = W + dt(1)
            Dn = (D * W + f) / w1
        D = np.where(ok, Dn, D).astype(dt)
        W = np.where(ok, w1, W).astype(dt)
        if trace is not None:
            trace.append((ok, u, v))
    return D, W


def marching_tets(D, W, origin, voxel, min_weight=1, dt=F):
    """-> (vertices [N,3] dt, triangles [M,3] int32), in the defined order: vertices by (lattice index, d), triangles by
    (cell index, tetrahedron, triangle); normals towards D > 0."""
    D, W = np.asarray(D), np.asarray(W)
    nz, ny, nx = D.shape
    seen = W >= min_weight
    inside = seen & (D < 0)
    empty = np.zeros((0, 3), dt), np.zeros((0, 3), np.int32)
    if nx < 2 or ny < 2 or nz < 2:
        return empty

    def sub(a, c):
        ox, oy, oz = CORNERS[c]
        return a[oz:nz - 1 + oz, oy:ny - 1 + oy, ox:nx - 1 + ox]

    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    mask = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for c in range(8):
        valid &= sub(seen, c)
        mask |= sub(inside, c).astype(np.int32) << c
    active = valid & (mask > 0) & (mask < 255)
    cells = np.argwhere(active)                      # (k, j, i) in increasing cell index
    marks = set()
    raw = []                                         # triangles as triples of edge keys (lattice index, d)

    def key(k, j, i, ca, cb):
        lo = min(ca, cb)
        ox, oy, oz = CORNERS[lo]
        q = ((k + oz) * ny + (j + oy)) * nx + (i + ox)
        e = (q, ca ^ cb)
        marks.add(e)
        return e

    for k, j, i in cells:
        m = int(mask[k, j, i])
        for tet, odd in TETS:
            pos_in = [p for p in range(4) if m >> tet[p] & 1]
            pos_out = [p for p in range(4) if not m >> tet[p] & 1]
            if not pos_in or not pos_out:
                continue
            if len(pos_in) == 2:
                a1, a2 = (tet[p] for p in pos_in)
                b1, b2 = (tet[p] for p in pos_out)
                quad = [key(k, j, i, a1, b1), key(k, j, i, a1, b2), key(k, j, i, a2, b2), key(k, j, i, a2, b1)]
                flip = bool((pos_in[0] + pos_in[1] + 1) & 1) != odd
                t1, t2 = [quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]
                if flip:
                    t1, t2 = [t1[0], t1[2], t1[1]], [t2[0], t2[2], t2[1]]
                raw += [t1, t2]
            else:
                lone_in = len(pos_in) == 1
                apex_pos = pos_in[0] if lone_in else pos_out[0]
                base = pos_out if lone_in else pos_in
                tri = [key(k, j, i, tet[apex_pos], tet[p]) for p in base]
                away = bool(apex_pos & 1) == odd
                if (not away) if lone_in else away:
                    tri = [tri[0], tri[2], tri[1]]
                raw.append(tri)
    if not raw:
        return empty
    order = sorted(marks)
    index = {e: n for n, e in enumerate(order)}
    o, s = np.asarray(origin, dt), dt(voxel)
    Df = D.reshape(-1).astype(dt)
    verts = np.zeros((len(order), 3), dt)
    for n, (q, d) in enumerate(order):
        i, j, k = q % nx, q // nx % ny, q // nx // ny
        qb = q + (d & 1) + ((d >> 1 & 1) + (d >> 2 & 1) * ny) * nx
        da, db = Df[q], Df[qb]
        t = da / (da - db)
        for ax, (base, bit) in enumerate(((i, 1), (j, 2), (k, 4))):
            fi = dt(base) + t if d & bit else dt(base)
            verts[n, ax] = o[ax] + s * fi
    tris = np.array([[index[e] for e in t] for t in raw], np.int32)
    return verts, tris


def colour(vertices, depths, images, Ks, Es, trunc, dt=F):
    """-> uint8 [N,3]: the mean, rounded half up, of the nearest texels over the views that see the vertex with |d - z| <= trunc."""
    vtx = np.asarray(vertices, F).astype(dt)
    n = len(vtx)
    acc = np.zeros((n, 4), dt)
    tau = dt(F(trunc))
    for dep, img, K, E in zip(depths, images, Ks, Es):
        dep = np.asarray(dep, F)
        h, w = dep.shape
        ok, u, v, pz = project(np.asarray(K, F), np.asarray(E, F), vtx[:, 0], vtx[:, 1], vtx[:, 2], h, w, dt)
        with np.errstate(all="ignore"):
            d = dep[v, u].astype(dt)
            ok = ok & np.isfinite(d) & (d > 0)
            ok = ok & (np.abs(d - pz) <= tau)
        add = np.concatenate([np.asarray(img)[v, u].astype(dt), np.ones((n, 1), dt)], 1)
        acc = np.where(ok[:, None], acc + add, acc).astype(dt)
    out = np.full((n, 3), 128, np.uint8)
    got = acc[:, 3] > 0
    with np.errstate(all="ignore"):
        mean = np.floor(acc[:, :3] / acc[:, 3:4] + dt(0.5))
    out[got] = mean[got].astype(np.uint8)
    return out


# --------------------------------------------------------------------------- mesh checks
def topology(vertices, triangles):
    """-> dict(closed: every edge in exactly two triangles, once in each direction; euler; volume; all_referenced)."""
    t = np.asarray(triangles, np.int64)
    v = np.asarray(vertices, np.float64)
    directed = {}
    for a, b in np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]):
        directed[(a, b)] = directed.get((a, b), 0) + 1
    closed = all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
    n_edges = len({(min(a, b), max(a, b)) for a, b in directed})
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    volume = float(np.sum(np.einsum("ij,ij->i", p0, np.cross(p1, p2))) / 6.0)
    return {"closed": closed, "euler": len(v) - n_edges + len(t), "volume": volume,
            "all_referenced": len(np.unique(t)) == len(v)}


# --------------------------------------------------------------------------- scenes
def look_at(centre, target, up):
    """World-to-camera E [4,4] float32 of a camera at `centre` looking at `target` (z forward, x right, y down)."""
    c, t = np.asarray(centre, np.float64), np.asarray(target, np.float64)
    f = (t - c) / np.linalg.norm(t - c)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ c
    return E.astype(F)


def pinhole(f, h, w, dx=0.0, dy=0.0):
    return np.array([[f, 0, (w - 1) / 2 + dx], [0, f, (h - 1) / 2 + dy], [0, 0, 1]], F)


def pixel_rays(K, E, h, w):
    """float64 camera centre and unit-z ray directions (world) of every pixel centre, [h,w,3]."""
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    R, t = E[:3, :3], E[:3, 3]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    cam = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    return -R.T @ t, cam @ R                          # rows of R^T applied: world direction = R^T cam


def sphere_depth(K, E, h, w, centre, radius):
    """Analytic depth (camera z) of the sphere along every pixel ray; 0 where the ray misses."""
    c, dirs = pixel_rays(K, E, h, w)
    oc = c - np.asarray(centre, np.float64)
    a = np.einsum("hwk,hwk->hw", dirs, dirs)
    b = 2.0 * dirs @ oc
    cc = oc @ oc - radius * radius
    disc = b * b - 4 * a * cc
    with np.errstate(invalid="ignore"):
        s = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (s > 0), s, 0.0).astype(F)   # directions have unit z, so the ray parameter is the depth


def plane_depth(K, E, h, w, normal, offset):
    """Depth of the plane normal . x = offset along every pixel ray; 0 where it is behind or parallel."""
    c, dirs = pixel_rays(K, E, h, w)
    n = np.asarray(normal, np.float64)
    with np.errstate(all="ignore"):
        s = (offset - n @ c) / (dirs @ n)
    return np.where(np.isfinite(s) & (s > 0), s, 0.0).astype(F)


def lattice_for(dims, half=1.3, centre=(0.013, -0.007, 0.021)):
    """A box of half-extent `half` along its longest side around `centre`: -> (origin float32 [3], voxel float32)."""
    voxel = F(2 * half / (max(dims) - 1)) if max(dims) > 1 else F(1)
    origin = np.array([centre[a] - float(voxel) * (dims[a] - 1) / 2 for a in range(3)], F)
    return origin, voxel


SPHERE_CENTRE, SPHERE_RADIUS = (0.013, -0.007, 0.021), 0.8


def sphere_field(dims, dt=F):
    """The analytic distance field of a sphere that fits the lattice (radius 0.37 of the shortest side, centre off the lattice),
    in units of a 3-voxel truncation and clipped to 1, every point observed once: -> (D, W, origin, voxel, centre, radius)."""
    origin, voxel = lattice_for(dims)
    x, y, z = lattice_points(origin, voxel, dims, np.float64)
    centre = np.array([float(origin[a]) + float(voxel) * (dims[a] - 1) * (0.5 + 0.013 * (a + 1)) for a in range(3)])
    radius = 0.37 * float(voxel) * (min(dims) - 1)
    dist = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    D = np.minimum(1.0, dist / (3.0 * float(voxel))).astype(dt)
    return D, np.ones_like(D), origin, voxel, centre, radius


def sphere_scene(dims, h=96, w=128, nviews=6, dist=20.0, focal=None):
    """The sphere seen by pinhole cameras on the coordinate axes (the first six; further views repeat them at slightly larger
    distances), analytic depth maps with a zero background.  The default focal length gives a pixel footprint of half a voxel at
    the sphere's centre (less on the surface that faces the camera).  Points whose rays miss the sphere in every view stay
    unobserved, so the far cameras matter: from dist = 20 the exterior points up to ~0.15 radii off the surface are seen by some
    camera, and with the radius at 10 voxels or more (a lattice of 33 points or more along the 2.6-unit box) every cell that the
    surface crosses has its 8 corners observed.  Coarser lattices give an open mesh by construction of the scene."""
    origin, voxel = lattice_for(dims)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    ups = [(0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 1, 0), (0, 1, 0)]
    Ks, Es, depths = [], [], []
    for n in range(nviews):
        a, up = axes[n % 6], ups[n % 6]
        r = dist + 0.173 * (n // 6)
        c = np.asarray(SPHERE_CENTRE) + r * np.asarray(a, np.float64) + np.array([0.0131, 0.0177, 0.0113]) * (1 + n)
        E = look_at(c, SPHERE_CENTRE, up)
        f = focal if focal is not None else r / (0.5 * float(voxel))
        K = pinhole(f, h, w, dx=0.231 + 0.01 * n, dy=-0.177)
        Ks.append(K)
        Es.append(E)
        depths.append(sphere_depth(K, E, h, w, SPHERE_CENTRE, SPHERE_RADIUS))
    return {"depths": depths, "K": np.stack(Ks), "E": np.stack(Es), "origin": origin, "voxel": voxel, "dims": tuple(dims),
            "trunc": F(3) * voxel}


def plane_scene(dims, h=48, w=64):
    """A slanted plane through the box seen by 2 cameras on its positive side; truncation 1.2 world units (the cameras are ~3
    units away: the fp32 error of (d - z) / trunc grows with z / trunc, see test_tsdf_mesh_cpu.py)."""
    origin, voxel = lattice_for(dims)
    n = np.array([0.31, -0.22, 0.92])
    n /= np.linalg.norm(n)
    Ks, Es, depths = [], [], []
    for c in ((0.4, -0.3, 2.9), (-0.9, 0.5, 2.6)):
        E = look_at(c, (0.02, 0.01, 0.0), (0, 1, 0))
        K = pinhole(0.55 * min(h, w), h, w, dx=0.137, dy=0.291)
        Ks.append(K)
        Es.append(E)
        depths.append(plane_depth(K, E, h, w, n, 0.05))
    return {"depths": depths, "K": np.stack(Ks), "E": np.stack(Es), "origin": origin, "voxel": voxel, "dims": tuple(dims),
            "trunc": F(1.2)}


def awkward_scene(dims, h=5, w=7, nviews=5):
    """Everything the skip rules name: a camera inside the volume (lattice points at z <= 0), depth maps with NaN, +inf, 0 and
    negative texels, one view whose frustum misses the box, and an axis-aligned camera in front of a constant-depth map placed so
    that lattice planes sit exactly at sdf = -trunc and sdf = +trunc."""
    origin = np.array([-1.0, -1.0, -1.0], F)
    voxel = F(0.25)
    trunc = F(0.5)
    rng = np.random.RandomState(7)
    Ks, Es, depths = [], [], []
    for n in range(nviews):
        kind = n % 5
        K = pinhole(0.9 * min(h, w) + 0.5, h, w, dx=0.21, dy=-0.13)
        if kind == 0:      # axis-aligned, looking down +z from z = -3: depth 2.5 -> lattice planes at z = -0.5 (sdf 0), 0 (-tau), -1 (+tau)
            E = np.eye(4, dtype=F)
            E[2, 3] = 3.0
            dep = np.full((h, w), 2.5, F)
        elif kind == 1:    # inside the volume
            E = look_at((0.1, -0.05, 0.12), (1.0, 0.3, 0.2), (0, 0, 1))
            dep = (0.3 + rng.rand(h, w)).astype(F)
        elif kind == 2:    # bad texels
            E = look_at((2.5, 0.3, 0.2), (0, 0, 0), (0, 0, 1))
            dep = (2.0 + rng.rand(h, w)).astype(F)
            bad = [np.nan, np.inf, 0.0, -1.5, -np.inf]
            flat = dep.reshape(-1)
            for q in range(flat.size):
                if q % 2 == 0:
                    flat[q] = bad[(q // 2) % len(bad)]
        elif kind == 3:    # looks away from the box
            E = look_at((3.0, 3.0, 3.0), (6.0, 6.0, 7.0), (0, 0, 1))
            dep = np.full((h, w), 1.0, F)
        else:              # grazing, far
            E = look_at((-0.3, -4.0, 0.4), (0.2, 0, 0), (0, 0, 1))
            dep = (3.5 + rng.rand(h, w)).astype(F)
        Ks.append(K)
        Es.append(E)
        depths.append(dep)
    return {"depths": depths, "K": np.stack(Ks), "E": np.stack(Es), "origin": origin, "voxel": voxel, "dims": tuple(dims),
            "trunc": trunc}


def scene_images(scene, seed=3):
    """uint8 [h,w,3] images for a scene's views (random texture: colour has no geometry to respect)."""
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=d.shape + (3,)).astype(np.uint8) for d in scene["depths"]]
