"""CPU: the Tanks and Temples evaluation's oracle (tests/tanks_eval_oracle.py) against independent brute-force restatements, the
new readers / writers, the host-side alignment, the declarations of the new entries, and the conditions the GPU tests' fixture
scene has to meet (mid-range scores, an empty undecided band, no inlier decision near an ICP threshold)."""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import tanks_eval_oracle as O  # noqa: E402

NEW_ENTRIES = ["mdf_pts_nn", "mdf_pts_transform", "mdf_pts_crop", "mdf_pts_voxel_workspace", "mdf_pts_voxel_downsample",
               "mdf_pts_icp_workspace", "mdf_pts_icp_sums"]
NEW_OPS = ["nn_search", "transform_points", "crop_volume", "voxel_downsample", "icp_point_to_point", "tanks_eval_scene"]


def test_new_entries_declared_everywhere():
    """The header, the ctypes table, the ops and the kernel-family table all know the new entries (fails before this feature)."""
    import mdfnet_hip
    from mdfnet_hip import kernel_families, ops
    text = open(os.path.join(ROOT, "include", "mdfnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mdf_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in mdfnet_hip.SIGNATURES, name
    for name in NEW_OPS:
        assert callable(getattr(ops, name, None)), name
    for k in ("pts_nn_idx_kernel", "pts_transform_kernel", "pts_crop_kernel", "pts_vox_key_kernel", "pts_vox_mean_kernel",
              "pts_icp_moment_kernel", "pts_icp_final_kernel"):
        assert kernel_families.KERNEL_FAMILY.get(k) == kernel_families.POINT_EVAL, k
    assert ops.TANKS_TAU == O.TAU and len(O.TAU) == 7


def test_ops_refuse_cpu_tensors():
    import torch
    from mdfnet_hip import ops
    pts = torch.rand(10, 3, dtype=torch.float64)
    poly = [[0, 0], [1, 0], [0, 1]]
    for call in (lambda: ops.transform_points(pts, np.eye(4)), lambda: ops.crop_volume(pts, 1, 0, 1, poly),
                 lambda: ops.voxel_downsample(pts, 0.1), lambda: ops.icp_point_to_point(pts, pts, 0.1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---------------------------------------------------------------------------------------------------- voxel grid
def dict_voxel(pts, v, attrs=None):
    """Independent restatement: a dictionary of lists, filled in input order, summed left to right in Python floats."""
    origin = pts.min(0) - v / 2
    cells = {}
    for i, p in enumerate(pts):
        key = tuple(int(np.floor((p[a] - origin[a]) / v)) for a in range(3))
        cells.setdefault(key, []).append(i)
    out, oa, cnt = [], [], []
    for key in sorted(cells):
        s = [0.0, 0.0, 0.0]
        t = [0.0] * (0 if attrs is None else attrs.shape[1])
        for i in cells[key]:
            for a in range(3):
                s[a] = s[a] + float(pts[i, a])
            for a in range(len(t)):
                t[a] = t[a] + float(attrs[i, a])
        c = len(cells[key])
        out.append([x / c for x in s]); oa.append([x / c for x in t]); cnt.append(c)
    return np.array(out).reshape(-1, 3), np.array(oa).reshape(len(out), -1), np.array(cnt, dtype=np.int32)


def voxel_scene(seed, n=3000):
    rng = np.random.RandomState(seed)
    pts = rng.uniform(-1, 1, (n, 3)) * [1, 0.3, 0.6]
    pts[:400] = pts[0] + rng.uniform(0, 0.01, (400, 3))          # a clump
    pts[400:440] = pts[500]                                         # exact duplicates
    return pts, rng.uniform(0, 255, (n, 6))


@pytest.mark.parametrize("seed,v", [(0, 0.05), (1, 0.013), (2, 0.5)])
def test_voxel_oracle_against_dictionary(seed, v):
    pts, attrs = voxel_scene(seed)
    got_p, got_a, got_c = O.voxel(pts, v, attrs)
    want_p, want_a, want_c = dict_voxel(pts, v, attrs)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_a, want_a) and np.array_equal(got_c, want_c)
    assert got_c.sum() == len(pts) and got_c.max() >= 40
    p1, a1, c1 = O.voxel(pts[:1], v)
    assert np.array_equal(p1, pts[:1]) and a1 is None and c1.tolist() == [1]
    assert O.voxel(np.zeros((0, 3)), v)[0].shape == (0, 3)


def test_voxel_oracle_points_on_cell_faces_and_too_many_cells():
    v = 0.25
    base = np.array([[0.0, 0.0, 0.0]])
    grid = base + v / 2 + v * np.array([[1, 0, 0], [2, 0, 0], [2, 1, 0], [0, 0, 3], [1, 0, 0]], dtype=np.float64)   # on faces
    pts = np.concatenate([base, grid])
    got = O.voxel(pts, v)
    want = dict_voxel(pts, v)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and got[2].tolist() == [1, 1, 2, 1, 1]
    with pytest.raises(ValueError, match="2\\^21"):
        O.voxel(np.array([[0.0, 0, 0], [3.0, 0, 0]]), 1e-6)


# ---------------------------------------------------------------------------------------------------- nearest neighbour
def nn_scene(seed, n=1500, m=700):
    rng = np.random.RandomState(seed)
    to = rng.uniform(-1, 1, (n, 3))
    to[:300] = to[0] + rng.uniform(-1e-4, 1e-4, (300, 3))
    to[300:340] = to[400]                                           # 41 equal points: ties
    to[1000:1010] = to[20]                                          # a tie with a LOWER index far away in the array
    frm = np.concatenate([to[rng.randint(0, n, m)] + rng.normal(0, 0.01, (m, 3)), to[395:405], to[15:25], rng.uniform(2, 3, (50, 3))])
    return to, frm


@pytest.mark.parametrize("seed", [0, 1])
def test_nn_oracle_against_brute_force(seed):
    to, frm = nn_scene(seed)
    for cap in (0.5, 0.02):
        d, i, d2 = O.nn(to, frm, cap)
        bd, bi, bd2 = O.nn_brute(to, frm, cap)
        assert np.array_equal(d, bd) and np.array_equal(i, bi) and np.array_equal(d2, bd2)
    assert (i == -1).sum() >= 50 and (i == 300).sum() >= 1 and (i == 20).sum() >= 1 and not (i == 1000).any()
    assert np.array_equal(O.nn(np.zeros((0, 3)), frm, 1.0)[1], np.full(len(frm), -1))
    assert np.array_equal(O.nn(to[:3], frm, 9.0)[1], O.nn_brute(to[:3], frm, 9.0)[1])


# ---------------------------------------------------------------------------------------------------- crop
def winding_inside(poly, x, y):
    """A second polygon test (the winding number by summed signed angles), valid away from the edges."""
    ang = 0.0
    k = len(poly)
    for i in range(k):
        a, b = poly[i] - (x, y), poly[(i + 1) % k] - (x, y)
        ang += np.arctan2(a[0] * b[1] - a[1] * b[0], a[0] * b[0] + a[1] * b[1])
    return abs(ang) > np.pi


def edge_distance(poly, x, y):
    d = np.inf
    k = len(poly)
    for i in range(k):
        a, b = poly[i], poly[(i + 1) % k]
        t = np.clip(((x - a[0]) * (b[0] - a[0]) + (y - a[1]) * (b[1] - a[1])) / ((b - a) ** 2).sum(), 0, 1)
        d = min(d, np.hypot(x - a[0] - t * (b[0] - a[0]), y - a[1] - t * (b[1] - a[1])))
    return d


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_crop_oracle_against_winding_number(axis):
    rng = np.random.RandomState(axis)
    poly = np.array([[-1.0, -0.9], [0.2, -1.05], [0.9, -0.4], [0.3, 0.1], [0.75, 0.8], [-0.1, 0.55], [-0.95, 0.9]])   # not convex
    pts = rng.uniform(-1.3, 1.3, (4000, 3))
    iu, iv = O.uv_axes(axis)
    assert sorted((axis, iu, iv)) == [0, 1, 2] and iu < iv
    keep = O.crop(pts, axis, -0.5, 0.7, poly)
    checked = 0
    for p, k in zip(pts, keep):
        if edge_distance(poly, p[iu], p[iv]) < 1e-3 or min(abs(p[axis] + 0.5), abs(p[axis] - 0.7)) < 1e-9:
            continue
        assert k == (winding_inside(poly, p[iu], p[iv]) and -0.5 <= p[axis] <= 0.7)
        checked += 1
    assert checked > 3500 and 0.1 < keep.mean() < 0.6
    on = np.zeros((2, 3))
    on[0, axis], on[1, axis] = -0.5, 0.7                        # the interval is closed
    on[:, iu], on[:, iv] = -0.2, 0.0
    assert O.crop(on, axis, -0.5, 0.7, poly).all()


# ---------------------------------------------------------------------------------------------------- files and alignment
def test_reader_writer_round_trips(tmp_path):
    from tools import data_io
    rng = np.random.RandomState(3)
    poses = rng.normal(0, 1, (5, 4, 4))
    data_io.write_trajectory_log(str(tmp_path / "t.log"), poses)
    assert np.array_equal(data_io.read_trajectory_log(str(tmp_path / "t.log")), poses)
    assert open(str(tmp_path / "t.log")).readline() == "0 0 0\n"
    m = rng.normal(0, 1, (4, 4))
    data_io.write_matrix_txt(str(tmp_path / "m.txt"), m)
    assert np.array_equal(data_io.read_matrix_txt(str(tmp_path / "m.txt")), m)
    poly3 = rng.normal(0, 1, (7, 3))
    for axis in (0, 1, 2):
        data_io.write_crop_json(str(tmp_path / "c.json"), axis, -0.25, 1.5, poly3)
        c = data_io.read_crop_json(str(tmp_path / "c.json"))
        iu, iv = O.uv_axes(axis)
        assert c["axis"] == axis and c["axis_min"] == -0.25 and c["axis_max"] == 1.5
        assert np.array_equal(c["polygon3"], poly3) and np.array_equal(c["polygon"], poly3[:, [iu, iv]])
        assert data_io.crop_uv_axes(axis) == (iu, iv)
    with open(str(tmp_path / "bad.log"), "w") as f:
        f.write("0 0 0\n1 0 0 0\n")
    with pytest.raises(ValueError):
        data_io.read_trajectory_log(str(tmp_path / "bad.log"))


def test_umeyama_recovers_a_known_similarity():
    from mdfnet_hip import ops
    rng = np.random.RandomState(5)
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    q *= np.sign(np.linalg.det(q))
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = 2.3 * q, [0.4, -1.0, 3.0]
    src = rng.normal(0, 1, (30, 3))
    dst = src @ S[:3, :3].T + S[:3, 3]
    for f in (ops.umeyama, O.umeyama):
        assert np.abs(f(src, dst) - S).max() < 1e-12
    rigid = ops.umeyama(src, src @ q.T + 1.0, with_scale=False)
    assert np.abs(rigid[:3, :3] - q).max() < 1e-12
    sc = O.fixture_scene()
    got = ops.tanks_initial_alignment(sc["est_poses"], sc["ref_poses"], sc["trans"])
    assert np.abs(got - sc["S"]).max() < 1e-12
    assert np.abs(got - O.initial_alignment(sc["est_poses"], sc["ref_poses"], sc["trans"])).max() < 1e-12
    with pytest.raises(ValueError, match="cameras"):
        ops.tanks_initial_alignment(sc["est_poses"][:-1], sc["ref_poses"], sc["trans"])


def test_icp_oracle_step_and_bound():
    """One oracle step on exact correspondences recovers the motion, and update_bound covers a shuffled summation order."""
    rng = np.random.RandomState(6)
    tgt = rng.uniform(-1, 1, (2000, 3))
    ang = 0.01
    M = np.eye(4)
    M[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    M[:3, 3] = [0.003, -0.002, 0.001]
    src = O.transform(tgt, np.linalg.inv(M))
    idx = np.arange(len(tgt), dtype=np.int32)
    s = O.icp_sums(src, tgt, idx, O.dist2(src, tgt), 1.0)
    assert s[0] == len(tgt) and np.abs(O.rigid_update(s) - M).max() < 1e-12
    perm = rng.permutation(len(tgt))
    s2 = O.icp_sums(src[perm], tgt, idx[perm], O.dist2(src, tgt)[perm], 1.0)
    dR, dt = O.update_bound(src, tgt)
    d = O.rigid_update(s) - O.rigid_update(s2)
    assert np.sqrt((d[:3, :3] ** 2).sum()) <= dR < 1e-9 and np.abs(d[:3, 3]).max() <= dt < 1e-9
    T, fit, rmse, its = O.icp(src + rng.normal(0, 1e-3, src.shape), tgt, 0.05)
    assert np.abs(T - M).max() < 2e-4 and fit == 1.0 and 1e-3 < rmse < 3e-3 and 1 <= its < 20


def test_fscore_histograms():
    p, r, f, h1, h2 = O.fscore(np.array([0.0, 0.5, 1.5, 4.9, 5.0, 10.0]), np.array([0.2, 3.0]), 1.0)
    assert (p, r) == (2 / 6, 0.5) and np.isclose(f, 2 * p * r / (p + r))
    assert h1[-1] == 5 / 6 and h1[0] == 1 / 6 and h2[-1] == 1.0 and len(h1) == 100
    assert O.fscore(np.zeros(0), np.zeros(0), 1.0)[:3] == (0.0, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------- the fixture's conditions
@functools.lru_cache(maxsize=1)
def fixture_run():
    sc = O.fixture_scene()
    traces = {}
    init = O.initial_alignment(sc["est_poses"], sc["ref_poses"], sc["trans"])
    return sc, O.eval_scene(sc["est"], sc["gt"], sc["crop"], sc["tau"], init, traces=traces), traces, init


def test_fixture_conditions():
    sc, res, traces, init = fixture_run()
    tau = sc["tau"]
    assert len(sc["est"]) <= 60000 and len(sc["gt"]) <= 60000
    print("fixture:", {k: res[k] for k in ("precision", "recall", "fscore", "n_est_crop", "n_gt_crop", "n_est_down", "n_gt_down")},
          res["stage_iterations"], res["stage_fitness"], res["stage_rmse"])
    assert 0.3 <= res["precision"] <= 0.95 and 0.3 <= res["recall"] <= 0.95
    # the crop cuts both clouds
    assert 0.1 * res["n_est"] < res["n_est_crop"] < 0.9 * res["n_est"] and 0.1 * res["n_gt"] < res["n_gt_crop"] < 0.9 * res["n_gt"]
    # the undecided band holds at most 0.1 % of either cloud
    assert O.undecided(res["dist_est"], tau) <= 1e-3 * res["n_est_down"]
    assert O.undecided(res["dist_gt"], tau) <= 1e-3 * res["n_gt_down"]
    # no inlier decision within 1e-6 * threshold of an ICP threshold along the oracle's iterations
    for name, tr in traces.items():
        assert len(tr) == res["stage_iterations"]["ABC".index(name)] + 1
        assert min(ev["margin"] for ev in tr) > 1e-6, name
    # the registration matters: the offset is a few tau and the unregistered score is clearly worse
    raw = O.score(sc["est"], sc["gt"], sc["crop"], tau, init)
    print("unregistered:", raw["precision"], raw["recall"], raw["fscore"])
    assert res["fscore"] > raw["fscore"] + 0.1
    # ... and most of the offset (2.5 tau at the largest) is found; a smooth surface lets point-to-point ICP slide a little
    assert np.abs(res["T"] @ np.linalg.inv(init) - sc["off"]).max() < tau
