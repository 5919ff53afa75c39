"""GPU: the point-cloud post-processing kernels (mdf_pts_knn, mdf_pts_normals; ops.knn_search / estimate_normals / nn_spacing and
stages 7 and 8 of ops.pcd_fuse) against tests/pcd_normals_oracle.py, and the tools/pcd/cloud.py driver end to end.

Bars.  Neighbour indices, d^2, the covariance, the spacing, the voxel size and the voxel means: bit-identical (the kernels and
the oracle execute the same correctly rounded operations in the same order, and (d^2, index) is a total order).  The normal: a
unit vector within 4 eps whose residual ||C n - (n^T C n) n|| / ||C||_F and whose excess (n^T C n - lambda_0) / ||C||_F over
numpy.linalg.eigh's smallest eigenvalue are both <= 4 R, R = the largest residual of eigh's own eigenvector over the same
matrices.  No point is left out: the two quantities together bound the angle to the true normal by residual / eigen-gap.

R is a maximum, so it needs a population: the four named clouds give 200 to 3000 different matrices each and are held to their
own R.  A cloud of n <= 30 points has ONE matrix (every point has the same n neighbours), and eigh's residual on a single matrix
says nothing about LAPACK's level (on the 3-point cloud it happens to be 4e-18), so the ragged sizes with k_eff >= 3 are held
together, as one set of matrices with one R.

Measured on an MI355X (R / kernel residual / kernel excess): see DESIGN section 7."""
import ctypes
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcd_normals_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -52
KS = (1, 2, 30, 32)
RAGGED = (1, 2, 3, 29, 30, 31, 32, 33, 64, 65)
CLOUDS = {"dtu": O.dtu_surface, "tanks": O.tanks_surface, "lattice": O.lattice, "degenerate": O.degenerate}
CLOUDS.update({f"ragged{n}": functools.partial(O.ragged, n) for n in RAGGED})
NAMED = ("dtu", "tanks", "lattice", "degenerate")


def gpu(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).to(DEV)             # a copy: the cached clouds are read-only
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=None)
def cloud(name):
    """-> (pts, queries, oracle self k-NN at k = 32, oracle k-NN of the queries at k = 32).  A row of a smaller k is a prefix of
    the k = 32 row ((d^2, index) is a total order), so one brute-force pass serves every k.  The queries are another set: points
    of the cloud pushed off it, and points well outside its box."""
    pts = CLOUDS[name]()
    rng = np.random.RandomState(len(pts) + 11)
    ext = pts.max(0) - pts.min(0) + 1.0
    near = pts[rng.randint(0, len(pts), 150)] + rng.uniform(-0.05, 0.05, (150, 3)) * ext
    far = pts.mean(0) + rng.uniform(-3, 3, (50, 3)) * ext
    q = O.f32(np.concatenate([near, far]))
    for a in (pts, q):
        a.setflags(write=False)
    own, qs = O.knn(pts, pts, 32), O.knn(pts, q, 32)
    for a in own + qs:
        a.setflags(write=False)
    return pts, q, own, qs


def prefix(knn32, k, n):
    """The oracle's k = 32 rows cut to k: slots past min(k, n) hold -1 / +inf already."""
    return knn32[0][:, :k], knn32[1][:, :k]


@functools.lru_cache(maxsize=None)
def oracle_cov(name, k=30):
    pts, _, own, _ = cloud(name)
    c6 = O.covariance(pts, own[0][:, :k])
    c6.setflags(write=False)
    return c6


def check_normals(c6, nrm, label):
    """The bar of the module docstring for normals `nrm` of covariances `c6`; prints R and the kernel's maxima."""
    assert np.isfinite(nrm).all()
    norm_err = np.abs(np.sqrt((nrm * nrm).sum(1)) - 1).max()
    lam, v = O.eigh_smallest(c6)
    R = O.residual(c6, v)[0].max()
    res, ray, fro = O.residual(c6, nrm)
    ok = fro > 0
    exc = ((ray - lam)[ok] / fro[ok]).max() if ok.any() else 0.0
    print(f"{label}: {len(c6)} matrices ({int((~ok).sum())} zero), R = {R:.3e}, kernel residual {res.max():.3e} "
          f"({res.max() / R if R else 0:.2f} R), excess {exc:.3e} ({exc / R if R else 0:.2f} R), | |n| - 1 | {norm_err:.2e}")
    assert norm_err <= 4 * EPS
    assert res.max() <= 4 * R and exc <= 4 * R
    return R, res.max(), exc


# ---------------------------------------------------------------------------------------------------- k nearest neighbours
@pytest.mark.parametrize("name", list(CLOUDS))
def test_knn_bit_identical(name):
    from mdfnet_hip import ops
    pts, q, own, qs = cloud(name)
    n = len(pts)
    index = ops.point_index(gpu(pts))
    qindex = ops.point_index(gpu(q))
    for k in KS:
        for label, queries, want in (("array", gpu(pts), own), ("index", index, own), ("other array", gpu(q), qs),
                                     ("other index", qindex, qs)):
            nbr, d2, visits = ops.knn_search(index, queries, k, return_d2=True, return_visits=True)
            wn, wd = prefix(want, k, n)
            assert nbr.dtype == torch.int32 and tuple(nbr.shape) == wn.shape
            np.testing.assert_array_equal(nbr.cpu().numpy(), wn, err_msg=f"{name} k={k} {label}")
            np.testing.assert_array_equal(d2.cpu().numpy(), wd, err_msg=f"{name} k={k} {label}")
            v = visits.cpu().numpy()
            assert (v >= 1).all() and (v <= (n + 31) // 32).all()
        assert torch.equal(ops.knn_search(index, index, k), gpu(prefix(own, k, n)[0]))
    if n >= 2:                      # a self-query finds the point itself, or a lower-indexed duplicate
        first = ops.knn_search(index, index, 1)[:, 0].cpu().numpy()
        assert (first <= np.arange(n)).all() and (pts[first] == pts).all()


def test_knn_error_paths():
    import mdfnet_hip
    l = mdfnet_hip.lib()
    pts = torch.rand((100, 3), device=DEV, dtype=torch.float64)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = l.mdf_pts_index_workspace(100)
    buf = torch.empty(nb, device=DEV, dtype=torch.uint8)
    assert l.mdf_pts_index_build(pts.data_ptr(), 100, buf.data_ptr(), nb, s) == 0
    nbr = torch.empty((100, 33), device=DEV, dtype=torch.int32)
    nrm = torch.empty((100, 3), device=DEV, dtype=torch.float64)
    for k in (0, 33, -1):
        assert l.mdf_pts_knn(buf.data_ptr(), 100, nb, None, pts.data_ptr(), 100, 0, k, nbr.data_ptr(), None, None, s) == -1
        assert b"k=" in l.mdf_last_error() and b"32" in l.mdf_last_error()
        assert l.mdf_pts_normals(buf.data_ptr(), 100, nb, k, None, nrm.data_ptr(), None, s) == -1 and b"k=" in l.mdf_last_error()
    assert l.mdf_pts_knn(buf.data_ptr(), 100, nb, None, pts.data_ptr(), 100, 0, 32, nbr.data_ptr(), None, None, s) == 0
    assert l.mdf_pts_knn(buf.data_ptr(), 100, nb, None, pts.data_ptr(), 100, 0, 4, None, None, None, s) == -1
    assert b"null" in l.mdf_last_error()
    assert l.mdf_pts_knn(buf.data_ptr(), 100, nb, buf.data_ptr(), pts.data_ptr(), 100, nb, 4, nbr.data_ptr(), None, None, s) == -1
    assert b"exactly one" in l.mdf_last_error()
    assert l.mdf_pts_knn(buf.data_ptr(), 100, nb // 2, None, pts.data_ptr(), 100, 0, 4, nbr.data_ptr(), None, None, s) == -1
    assert b"too small" in l.mdf_last_error()
    assert l.mdf_pts_normals(buf.data_ptr(), 100, nb, 30, None, None, None, s) == -1 and b"null" in l.mdf_last_error()
    assert l.mdf_pts_normals(buf.data_ptr(), 100, nb, 30, None, nrm.data_ptr(), None, s) == 0
    torch.cuda.synchronize()
    with pytest.raises(mdfnet_hip.MdfHipError, match="k=33"):
        from mdfnet_hip import ops
        ops.knn_search(ops.point_index(pts), pts, 33)


# ---------------------------------------------------------------------------------------------------- covariance and normals
@pytest.mark.parametrize("name", list(CLOUDS))
def test_covariance_bit_identical(name):
    from mdfnet_hip import ops
    pts = cloud(name)[0]
    for src in (gpu(pts), ops.point_index(gpu(pts))):
        nrm, cov = ops.estimate_normals(src, k=30, return_cov=True)
        np.testing.assert_array_equal(cov.cpu().numpy(), oracle_cov(name))
        assert torch.equal(nrm, ops.estimate_normals(src, k=30))


@pytest.mark.parametrize("name", NAMED)
def test_normals_residual(name):
    from mdfnet_hip import ops
    nrm = ops.estimate_normals(gpu(cloud(name)[0]), k=30).cpu().numpy()
    check_normals(oracle_cov(name), nrm, name)


def test_normals_residual_ragged_sizes():
    from mdfnet_hip import ops
    c6, nrm = [], []
    for n in RAGGED:
        got = ops.estimate_normals(gpu(cloud(f"ragged{n}")[0]), k=30).cpu().numpy()
        if n < 3:
            np.testing.assert_array_equal(got, np.tile([0.0, 0.0, 1.0], (n, 1)))
            continue
        c6.append(oracle_cov(f"ragged{n}"))
        nrm.append(got)
    check_normals(np.concatenate(c6), np.concatenate(nrm), "ragged sizes 3..65")


def test_normals_other_k():
    """k = 3 (the smallest with an eigenvector) and k = 32 (the largest): covariance bit for bit, the normal to the same bar."""
    from mdfnet_hip import ops
    pts, _, own, _ = cloud("tanks")
    for k in (3, 32):
        nrm, cov = ops.estimate_normals(gpu(pts), k=k, return_cov=True)
        c6 = O.covariance(pts, own[0][:, :k])
        np.testing.assert_array_equal(cov.cpu().numpy(), c6)
        check_normals(c6, nrm.cpu().numpy(), f"tanks k={k}")
    nrm = ops.estimate_normals(gpu(pts), k=2).cpu().numpy()
    np.testing.assert_array_equal(nrm, np.tile([0.0, 0.0, 1.0], (len(pts), 1)))


# ---------------------------------------------------------------------------------------------------- orientation
@pytest.mark.parametrize("name", ("tanks", "degenerate", "ragged1", "ragged2", "ragged33"))
def test_orientation(name):
    from mdfnet_hip import ops
    pts = cloud(name)[0]
    n = len(pts)
    dirs = np.random.RandomState(n).standard_normal((n, 3)).astype(np.float32)
    free = ops.estimate_normals(gpu(pts), k=30).cpu().numpy()
    got = ops.estimate_normals(gpu(pts), dirs=gpu(dirs), k=30).cpu().numpy()
    d = dirs.astype(np.float64)
    s = (got[:, 0] * d[:, 0] + got[:, 1] * d[:, 1]) + got[:, 2] * d[:, 2]
    assert (s >= 0).all()
    np.testing.assert_array_equal(got, O.orient(free, dirs))           # the un-oriented normal up to the sign the rule gives
    assert (np.abs(got) == np.abs(free)).all()
    if n < 3:
        assert (got[:, :2] == 0).all() and (got[:, 2] == np.where(dirs[:, 2] > 0, 1.0, -1.0)).all()


def test_orientation_flips_at_zero():
    """Points of the plane z = 0: the covariance has an exactly zero z row, so the normal is (0, 0, 1) exactly, and dirs in the
    plane give s = (0*dx + 0*dy) + 1*0 == 0, which negates."""
    from mdfnet_hip import ops
    rng = np.random.RandomState(8)
    pts = O.f32(np.column_stack([rng.uniform(-3, 3, (500, 2)), np.zeros(500)]))
    dirs = np.column_stack([rng.standard_normal((500, 2)), np.zeros(500)]).astype(np.float32)
    free = ops.estimate_normals(gpu(pts), k=30).cpu().numpy()
    np.testing.assert_array_equal(free, np.tile([0.0, 0.0, 1.0], (500, 1)))
    got = ops.estimate_normals(gpu(pts), dirs=gpu(dirs), k=30).cpu().numpy()
    np.testing.assert_array_equal(got, -free)
    up = ops.estimate_normals(gpu(pts), dirs=gpu(np.tile(np.float32([0, 0, 1e-30]), (500, 1))), k=30).cpu().numpy()
    np.testing.assert_array_equal(up, free)


# ---------------------------------------------------------------------------------------------------- spacing
@pytest.mark.parametrize("name", NAMED + ("ragged2", "ragged33"))
def test_nn_spacing_bit_identical(name):
    from mdfnet_hip import ops
    pts, _, own, _ = cloud(name)
    sp = ops.nn_spacing(ops.point_index(gpu(pts))).cpu().numpy()
    np.testing.assert_array_equal(sp, np.sqrt(own[1][:, 1]))
    if name == "degenerate":
        assert (sp[:100] == 0).all() and (sp[100:] > 0).all()


# ---------------------------------------------------------------------------------------------------- pcd_fuse, stages 7 and 8
@functools.lru_cache(maxsize=None)
def fused():
    """-> (scan arguments, today's result, the normals=True result, the oracle's k = 30 self k-NN of the returned points)."""
    from mdfnet_hip import ops, synth
    s = synth.pcd_scan(8, 48, 64, seed=1, nsrc=10)
    args = (gpu(s["depths"]), gpu(s["probs"]), gpu(s["images"]), s["K"], s["E"], s["srcs"])
    base = ops.pcd_fuse(*args, view=10, vthresh=4)
    withn = ops.pcd_fuse(*args, view=10, vthresh=4, normals=True)
    xyz = withn["xyz"].double().cpu().numpy()
    return args, base, withn, O.knn(xyz, xyz, 30)


def test_pcd_fuse_normals():
    args, base, withn, own = fused()
    assert set(withn) == set(base) | {"normals"} and "voxel" not in withn
    for key in ("xyz", "rgb", "dirs", "masks", "depths", "counts"):
        assert torch.equal(withn[key], base[key]), key
    m = base["xyz"].shape[0]
    assert m > 2000 and withn["normals"].dtype == torch.float64 and tuple(withn["normals"].shape) == (m, 3)
    xyz = withn["xyz"].double().cpu().numpy()
    nrm, dirs = withn["normals"].cpu().numpy(), withn["dirs"].cpu().numpy()
    check_normals(O.covariance(xyz, own[0]), nrm, f"pcd_fuse, {m} points")
    d = dirs.astype(np.float64)
    assert ((nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2] >= 0).all()
    # the scan is a slanted plane seen from one side: every oriented normal points back at the cameras (z < 0)
    assert (nrm[:, 2] < 0).mean() > 0.95


def test_pcd_fuse_downsample():
    from mdfnet_hip import ops
    import tanks_eval_oracle as TO
    args, base, withn, own = fused()
    xyz = withn["xyz"].double().cpu().numpy()
    voxel = O.percentile90(np.sqrt(own[1][:, 1]))
    attrs = np.concatenate([O.colour_attrs(withn["rgb"].cpu().numpy()), withn["normals"].cpu().numpy()], 1)
    wp, wa, _ = TO.voxel(xyz, voxel, attrs)
    out = ops.pcd_fuse(*args, view=10, vthresh=4, normals=True, downsample=-1)
    assert out["voxel"] == voxel and "dirs" not in out
    assert 0 < out["xyz"].shape[0] == len(wp) < len(xyz)
    print(f"pcd_fuse downsample=-1: voxel {voxel:.6g}, {len(xyz)} -> {len(wp)} points")
    assert out["xyz"].dtype == torch.float32 and out["rgb"].dtype == torch.uint8 and out["normals"].dtype == torch.float64
    np.testing.assert_array_equal(out["xyz"].cpu().numpy(), wp.astype(np.float32))
    np.testing.assert_array_equal(out["rgb"].cpu().numpy(), O.colour_u8(wa[:, :3]))
    np.testing.assert_array_equal(out["normals"].cpu().numpy(), wa[:, 3:])
    for key in ("masks", "depths", "counts"):
        assert torch.equal(out[key], base[key]), key
    # a given size, without normals: colours only
    wp2, wa2, _ = TO.voxel(xyz, 2.5, attrs[:, :3])
    out2 = ops.pcd_fuse(*args, view=10, vthresh=4, downsample=2.5)
    assert out2["voxel"] == 2.5 and "normals" not in out2 and "dirs" not in out2
    np.testing.assert_array_equal(out2["xyz"].cpu().numpy(), wp2.astype(np.float32))
    np.testing.assert_array_equal(out2["rgb"].cpu().numpy(), O.colour_u8(wa2))


def test_pcd_fuse_refuses_bad_voxel_sizes_and_repeats():
    from mdfnet_hip import ops
    args, base, withn, _ = fused()
    for bad in (0, -2, float("nan")):
        with pytest.raises(ValueError):
            ops.pcd_fuse(*args, view=10, vthresh=4, downsample=bad)
    a = ops.pcd_fuse(*args, view=10, vthresh=4, normals=True, downsample=-1)
    b = ops.pcd_fuse(*args, view=10, vthresh=4, normals=True, downsample=-1)
    assert a["voxel"] == b["voxel"] and set(a) == set(b)
    for key in a:
        if key != "voxel":
            assert torch.equal(a[key], b[key]), key
    assert torch.equal(ops.pcd_fuse(*args, view=10, vthresh=4, normals=True)["normals"], withn["normals"])
    again = ops.pcd_fuse(*args, view=10, vthresh=4)
    assert set(again) == set(base) and all(torch.equal(again[k], base[k]) for k in base)


# ---------------------------------------------------------------------------------------------------- one mid-size run
def test_normals_mid_size():
    """200 k points: a tree several levels deeper than the small clouds'.  2000 sampled points against brute force (a whole-cloud
    pass for 2000 queries takes 10 s on the host, so it runs for 150 of them and the slab form, which is proved per query to
    hold the same neighbours, for all 2000)."""
    from mdfnet_hip import ops
    pts = O.surface(200000, 60.0, (100.0, -50.0, 650.0), seed=4)
    g = gpu(pts)
    index = ops.point_index(g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nrm, cov = ops.estimate_normals(index, k=30, return_cov=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sel = np.random.RandomState(1).choice(len(pts), 2000, replace=False)
    nbr, d2, visits = ops.knn_search(index, g[gpu(sel)], 30, return_d2=True, return_visits=True)
    print(f"200000 points, k = 30: normals in {dt * 1e3:.1f} ms = {len(pts) / dt:.3e} points/s (first call), "
          f"{visits.double().mean().item():.1f} leaves visited per query")
    # brute force over the slab |x - qx| <= 3 (13.9 points per unit area: a quarter disc of radius 2.9 holds ~90 >= 30, which
    # knn_slab asserts per query), and over the whole cloud for the first 150 of them
    wn, wd = O.knn_slab(pts, pts[sel], 30, 3.0, 2.9)
    full = O.knn(pts, pts[sel[:150]], 30, chunk=50)
    np.testing.assert_array_equal(wn[:150], full[0])
    np.testing.assert_array_equal(wd[:150], full[1])
    np.testing.assert_array_equal(nbr.cpu().numpy(), wn)
    np.testing.assert_array_equal(d2.cpu().numpy(), wd)
    c6 = O.covariance(pts, wn)
    np.testing.assert_array_equal(cov.cpu().numpy()[sel], c6)
    check_normals(c6, nrm.cpu().numpy()[sel], "200 k surface, 2000 sampled")


# ---------------------------------------------------------------------------------------------------- driver
def test_cloud_driver_end_to_end(tmp_path):
    from mdfnet_hip import ops
    from test_pcd_fusion_cpu import make_scan_on_disk
    from tools.data_io import read_ply_normals
    from tools.pcd import fusion as F
    root, ev, out = make_scan_on_disk(tmp_path, "Horse", n=6, h=40, w=56)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mdf-net_amd", "tools", "pcd", "cloud.py"),
           "-r", str(root), "-e", str(ev), "-o", str(out), "-d", "tanks", "-s", "intermediate", "--scans", "Horse",
           "--view", "4", "--vthresh", "3"]
    sc = F.load_scan(os.path.join(str(root), "TankandTemples", "intermediate", "Horse"), os.path.join(str(ev), "Horse"),
                     "images", "cams_1")
    args = (gpu(sc["depths"]), gpu(sc["probs"]), gpu(sc["images"]), sc["K"], sc["E"], sc["srcs"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    xyz, rgb, nrm = read_ply_normals(str(out / "Horse.ply"))
    want = ops.pcd_fuse(*args, view=4, vthresh=3, normals=True)
    assert len(xyz) == want["xyz"].shape[0] > 0
    np.testing.assert_array_equal(xyz, want["xyz"].cpu().numpy())
    np.testing.assert_array_equal(rgb, want["rgb"].cpu().numpy())
    np.testing.assert_array_equal(nrm, want["normals"].float().cpu().numpy())
    r = subprocess.run(cmd + ["--downsample", "-1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    x2, c2, n2 = read_ply_normals(str(out / "Horse.ply"))
    down = ops.pcd_fuse(*args, view=4, vthresh=3, normals=True, downsample=-1)
    assert 0 < len(x2) < len(xyz)
    assert f"downsampled {len(xyz)} -> {len(x2)} points at voxel size {down['voxel']:.9g}" in r.stdout, r.stdout
    np.testing.assert_array_equal(x2, down["xyz"].cpu().numpy())
    np.testing.assert_array_equal(c2, down["rgb"].cpu().numpy())
    np.testing.assert_array_equal(n2, down["normals"].float().cpu().numpy())
