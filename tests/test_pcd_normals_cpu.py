"""CPU: the oracle of the point-cloud post-processing (tests/pcd_normals_oracle.py) against independent code (scipy's k-d tree,
numpy.percentile, a dictionary of lists), the conditions the GPU tests' clouds have to meet (ties at the 30th neighbour, duplicated
points), the declarations and exports of the new entries, and the two drivers' arguments."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcd_normals_oracle as O  # noqa: E402

NEW_ENTRIES = ["mdf_pts_knn", "mdf_pts_normals"]
NEW_OPS = ["knn_search", "estimate_normals", "nn_spacing"]
NEW_KERNELS = ["pts_knn_kernel", "pts_normals_kernel"]


def test_new_entries_declared_and_exported():
    """The header, the ctypes table, the built library, the ops and the kernel-family table all know the new entries (fails
    before this feature)."""
    import mdfnet_hip
    from mdfnet_hip import kernel_families, ops
    text = open(os.path.join(ROOT, "include", "mdfnet_hip.h")).read()
    assert re.search(r"#define\s+MDF_PTS_KNN_MAX\s+32\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mdf_[a-z0-9_]+)\s*\(", text))
    lib = mdfnet_hip.lib()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in mdfnet_hip.SIGNATURES, name
        assert callable(getattr(lib, name)), name
    assert len(mdfnet_hip.SIGNATURES["mdf_pts_knn"][1]) == 12 and len(mdfnet_hip.SIGNATURES["mdf_pts_normals"][1]) == 8
    for name in NEW_OPS:
        assert callable(getattr(ops, name, None)), name
    for k in NEW_KERNELS:
        assert kernel_families.KERNEL_FAMILY.get(k) == kernel_families.POINT_EVAL, k
    assert ops.PCD_NORMAL_KNN == O.KNN == 30 and ops.KNN_MAX == 32
    assert lib.mdf_abi_version() == 1


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from mdfnet_hip import ops
    pts = torch.rand(10, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.estimate_normals(pts)
    with pytest.raises(TypeError):
        ops.knn_search(pts, pts, 3)
    with pytest.raises(TypeError):
        ops.nn_spacing(pts)
    z = torch.zeros((1, 2, 2))
    for bad in (0, -2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="downsample"):
            ops.pcd_fuse(z, z, torch.zeros((1, 2, 2, 3), dtype=torch.uint8), np.eye(3)[None], np.eye(4)[None], [[]], downsample=bad)


# ---------------------------------------------------------------------------------------------------- the oracle's k-NN
def test_knn_equals_kdtree_on_a_tie_free_cloud():
    from scipy.spatial import cKDTree
    pts = O.tanks_surface()
    nbr, d2 = O.knn(pts, pts, 30)
    assert (np.diff(d2, axis=1) > 0).all(), "the cloud has ties"
    _, want = cKDTree(pts).query(pts, k=30)
    np.testing.assert_array_equal(nbr, want)
    assert (nbr[:, 0] == np.arange(len(pts))).all() and (d2[:, 0] == 0).all()
    np.testing.assert_array_equal(d2, O.dist2(pts[nbr], pts[:, None, :]))
    q = pts[::7] + 0.05
    nq, _ = O.knn(pts, q, 30)
    np.testing.assert_array_equal(nq, cKDTree(pts).query(q, k=30)[1])


def test_knn_slab_equals_brute_force():
    pts = O.surface(20000, 60.0, (100.0, -50.0, 650.0), seed=4)
    q = pts[np.random.RandomState(1).choice(len(pts), 300, replace=False)]
    a, b = O.knn_slab(pts, q, 30, 9.0, 8.5), O.knn(pts, q, 30)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(AssertionError, match="slab"):
        O.knn_slab(pts, q, 30, 0.5, 0.4)


def python_knn(pts, q, k):
    """Independent restatement: Python's sort of (d^2, index) tuples."""
    rows = []
    for p in q:
        c = sorted((float(((a[0] - p[0]) * (a[0] - p[0]) + (a[1] - p[1]) * (a[1] - p[1])) + (a[2] - p[2]) * (a[2] - p[2])), i)
                   for i, a in enumerate(pts))[:k]
        rows.append([i for _, i in c] + [-1] * (k - len(c)))
    return np.array(rows, dtype=np.int32)


def test_knn_tie_rule_on_the_lattice():
    pts = O.lattice()
    assert len(pts) == 720
    assert O.tie_fraction(pts, 30) > 0.9              # the index decides the 30th neighbour of nearly every point
    nbr, d2 = O.knn(pts, pts, 30)
    sel = np.arange(0, 720, 9)
    np.testing.assert_array_equal(nbr[sel], python_knn(pts, pts[sel], 30))
    assert (np.diff(d2, axis=1) >= 0).all()
    tied = np.diff(d2, axis=1) == 0
    assert (np.diff(nbr, axis=1)[tied] > 0).all()    # equal d^2: ascending index


def test_knn_small_and_duplicated_clouds():
    for n in (1, 2, 3, 29, 30, 31, 33):
        pts = O.ragged(n)
        nbr, d2 = O.knn(pts, pts, 30)
        np.testing.assert_array_equal(nbr, python_knn(pts, pts, 30))
        assert (nbr[:, min(n, 30):] == -1).all() and np.isinf(d2[:, min(n, 30):]).all()
    pts = O.degenerate()
    assert len(pts) == 200
    nbr, d2 = O.knn(pts, pts, 30)
    np.testing.assert_array_equal(nbr, python_knn(pts, pts, 30))
    assert (nbr[:100, 0] == np.arange(100) % 5).all()                  # a self-query finds the lowest-indexed duplicate first
    assert (d2[:100, :20] == 0).all() and (d2[:100, 20] > 0).all()
    sp = O.nn_spacing(pts)
    assert (sp[:100] == 0).all() and (sp[100:] > 0).all()


# ---------------------------------------------------------------------------------------------------- covariance, eigenvectors
def test_covariance_is_the_sequential_sum():
    pts = O.dtu_surface(300)
    nbr, _ = O.knn(pts, pts, 30)
    c6 = O.covariance(pts, nbr)
    for i in (0, 17, 299):
        s = [0.0] * 9
        for j in nbr[i]:
            x, y, z = (float(v) for v in pts[j])
            for t, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
                s[t] = s[t] + v
        e = [v / 30 for v in s]
        want = [e[3] - e[0] * e[0], e[4] - e[0] * e[1], e[5] - e[0] * e[2], e[6] - e[1] * e[1], e[7] - e[1] * e[2], e[8] - e[2] * e[2]]
        assert c6[i].tolist() == want
    # against the two-pass covariance in extended precision: equal up to the cancellation of E[ab] - E[a] E[b]
    p = pts[nbr].astype(np.longdouble)
    d = p - p.mean(1, keepdims=True)
    two = np.einsum("mka,mkb->mab", d, d) / 30
    scale = float((pts * pts).sum(1).max())
    assert np.abs(O.sym(c6) - two.astype(np.float64)).max() <= 64 * 2.0 ** -53 * scale


def test_jacobi_restatement_meets_the_eigh_bar():
    """The solver the kernel uses, restated in numpy, against the bar of the GPU tests: residual and excess <= 4 R."""
    for name, pts in (("dtu", O.dtu_surface()), ("tanks", O.tanks_surface()), ("lattice", O.lattice()), ("degenerate", O.degenerate())):
        c6 = O.covariance(pts, O.knn(pts, pts, 30)[0])
        lam, v = O.eigh_smallest(c6)
        R = O.residual(c6, v)[0].max()
        n = O.jacobi_smallest(c6)
        res, ray, fro = O.residual(c6, n)
        ok = fro > 0
        exc = ((ray - lam)[ok] / fro[ok]).max()
        print(f"{name}: R = {R:.3e}, Jacobi residual {res.max():.3e}, excess {exc:.3e}")
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 4 * 2.0 ** -52
        assert res.max() <= 4 * R and exc <= 4 * R


def test_orientation_rule():
    n = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
    d = np.array([[0.0, 0.0, 2.0], [1.0, 5.0, 0.0], [0.0, 0.0, -1.0], [-0.8, 3.0, 0.6]], dtype=np.float32)
    out = O.orient(n, d)
    np.testing.assert_array_equal(out[0], n[0])
    np.testing.assert_array_equal(out[1], -n[1])              # s == 0 negates, as (s > 0) * 2 - 1 does
    np.testing.assert_array_equal(out[2], -n[2])
    ref = n.copy()                                            # the reference's two lines, on the same numbers
    ref *= ((ref * d).sum(-1, keepdims=True) > 0).astype(np.float32) * 2 - 1
    np.testing.assert_array_equal(out, ref)
    nrm, _ = O.normals(O.ragged(2), dirs=np.array([[0, 0, 1], [0, 0, -1]], dtype=np.float32))
    np.testing.assert_array_equal(nrm, [[0, 0, 1], [0, 0, -1]])


# ---------------------------------------------------------------------------------------------------- voxel size, colours
def test_percentile_equals_numpy():
    rng = np.random.RandomState(5)
    for m in (2, 3, 10, 11, 12, 101, 1000, 3000, 12345, 99991):
        v = rng.uniform(0, 3, m)
        assert O.percentile90(v) == np.percentile(v, 90), m
    for pts in (O.dtu_surface(), O.tanks_surface(), O.lattice(), O.degenerate()):
        sp = O.nn_spacing(pts)
        assert O.percentile90(sp) == np.percentile(sp, 90)
    assert O.percentile90(O.nn_spacing(O.lattice())) == 1.0


def test_colour_rule():
    rgb = np.arange(256, dtype=np.uint8).reshape(-1, 1).repeat(3, 1)
    a = O.colour_attrs(rgb)
    assert a.dtype == np.float64 and (a == (rgb.astype(np.float32) / np.float32(255))).all()
    np.testing.assert_array_equal(O.colour_u8(a), rgb)                  # a cell of one point keeps its colour
    np.testing.assert_array_equal(O.colour_u8([0.5 / 255, 1.5 / 255 + 1e-12, 2.4999 / 255, -0.2, 1.7]), [1, 2, 2, 0, 255])
    np.testing.assert_array_equal(O.colour_u8(np.array([2.5, 3.5, 254.5]) / 255 * (1 + 2.0 ** -52)), [3, 4, 255])


# ---------------------------------------------------------------------------------------------------- drivers
def test_cloud_parser_defaults_match_the_reference():
    from tools.pcd import cloud, fusion
    assert cloud.build_parser is fusion.build_parser
    a = cloud.build_parser().parse_args([])
    assert (a.view, a.vthresh, a.cam_scale, a.downsample, a.no_normal, a.write_mask) == (10, 4, 1, None, False, False)
    assert (a.dataset, a.set, a.filter_folder) == ("tanks", "intermediate", "filter")
    b = cloud.build_parser().parse_args(["--no_normal", "--downsample", "-1", "-d", "dtu"])
    assert b.no_normal is True and b.downsample == -1.0 and b.dataset == "dtu"


def test_fusion_main_still_refuses():
    from tools.pcd import fusion as F
    with pytest.raises(SystemExit, match="not implemented"):
        F.main(["-d", "tanks"])
    with pytest.raises(SystemExit, match="not implemented"):
        F.main(["-d", "tanks", "--no_normal", "--downsample", "0.5"])
    with pytest.raises(SystemExit, match=r"cloud\.py"):
        F.main(["-d", "tanks", "--downsample", "-1"])
