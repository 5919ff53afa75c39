"""GPU: the DTU evaluation kernels (mdf_pts_*, mdf_dtu_masks; ops.point_index / nn_distance / reduce_points / dtu_masks /
dtu_eval_scan) against tests/dtu_eval_oracle.py, the tools/dtu_eval driver end to end on a synthetic DTU tree, and the ABI's
error paths.

Bar: distances bit-identical (the kernels and the oracle evaluate the same correctly rounded fp64 formula; the minimum and the
cap / region tests are exact), keep masks and masks identical, statistics: counts and medians exact, means to rtol 1e-12."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import dtu_eval_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BB = np.array([[-100.0, -80.0, -50.0], [100.0, 95.0, 40.0]])


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1, 3)).to(DEV)


def nn_scene(seed):
    """to: a surface-like cloud with a dense clump (a whole bucket of near-duplicates) and exact duplicates; from: near points,
    outliers 30-90 mm away (past the cap), points outside BB."""
    rng = np.random.RandomState(seed)
    to = rng.uniform(-100, 100, (6000, 3)) * [1, 0.9, 0.4]
    to[:700] = to[0] + rng.uniform(-0.05, 0.05, (700, 3))           # clump: 700 points within 0.1 mm
    to[700:800] = to[800]                                            # exact duplicates
    frm = np.concatenate([to[rng.randint(0, 6000, 3000)] + rng.normal(0, 0.5, (3000, 3)),
                          to[:300] + rng.normal(0, 0.01, (300, 3)),
                          rng.uniform(-100, 100, (500, 3)) * [1, 0.9, 0.4] + rng.choice([-1, 1], (500, 3)) * rng.uniform(30, 90, (500, 3)),
                          rng.uniform(-250, 250, (400, 3)),
                          to[900:950]])                                # exactly on to-points: distance 0
    return to, frm


@pytest.mark.parametrize("seed", [0, 1])
def test_nn_distance_bit_identical(seed):
    from mdfnet_hip import ops
    to, frm = nn_scene(seed)
    idx = ops.point_index(gpu(to))
    for bb in (BB, None):
        want = O.nn_capped(to, frm, bb, 60.0)
        got = ops.nn_distance(idx, gpu(frm), bb=bb, cap=60.0).cpu().numpy()
        assert np.array_equal(got, want), (np.abs(got - want).max(), int((got != want).sum()))
        assert (want == 60.0).sum() > 100 and (want < 1e-9).sum() >= 30
        # queries through their own index: the same values at the input positions
        got2 = ops.nn_distance(idx, ops.point_index(gpu(frm)), bb=bb, cap=60.0).cpu().numpy()
        assert np.array_equal(got2, want)
    # another cap
    assert np.array_equal(ops.nn_distance(idx, gpu(frm), bb=None, cap=7.5).cpu().numpy(), O.nn_capped(to, frm, None, 7.5))


def test_nn_distance_small_and_empty():
    from mdfnet_hip import ops
    rng = np.random.RandomState(4)
    frm = rng.uniform(-50, 50, (257, 3))
    one = rng.uniform(-50, 50, (1, 3))
    for to in (one, frm[:33], np.zeros((0, 3))):
        idx = ops.point_index(gpu(to))
        assert np.array_equal(ops.nn_distance(idx, gpu(frm), bb=BB).cpu().numpy(), O.nn_capped(to, frm, BB, 60.0))
        assert np.array_equal(ops.nn_distance(idx, gpu(one), bb=BB).cpu().numpy(), O.nn_capped(to, one, BB, 60.0))
    empty = ops.point_index(gpu(np.zeros((0, 3))))
    assert (ops.nn_distance(empty, gpu(frm)).cpu().numpy() == 60.0).all()
    assert ops.nn_distance(ops.point_index(gpu(frm)), gpu(np.zeros((0, 3)))).numel() == 0


def test_nn_distance_repeat_is_bit_identical():
    from mdfnet_hip import ops
    to, frm = nn_scene(7)
    a, va = ops.nn_distance(ops.point_index(gpu(to)), gpu(frm), bb=BB, return_visits=True)
    b, vb = ops.nn_distance(ops.point_index(gpu(to)), gpu(frm), bb=BB, return_visits=True)
    assert torch.equal(a, b) and torch.equal(va, vb) and int(va.max()) >= 1


def reduce_cases():
    rng = np.random.RandomState(11)
    clump = rng.uniform(0, 0.3, (5000, 3))                           # long dependency chains
    chain = np.stack([np.arange(3000) * 0.15, np.zeros(3000), np.zeros(3000)], 1)
    dup = np.repeat(rng.uniform(0, 2, (300, 3)), 4, 0)               # exact duplicates
    cloud = rng.uniform(0, 1, (20000, 3)) * [20, 20, 1]
    return {"clump": clump, "chain": chain, "dup": dup, "cloud": cloud, "single": rng.uniform(0, 1, (1, 3))}


@pytest.mark.parametrize("case", ["clump", "chain", "dup", "cloud", "single"])
def test_reduce_points_identical_to_sequential(case):
    from mdfnet_hip import ops
    pts = reduce_cases()[case]
    for seed in (0, 1, 2):
        order = np.random.RandomState(seed).permutation(len(pts))
        want = O.reduce_pts(pts, 0.2, order)
        stats = {}
        keep, rounds = ops.reduce_points(gpu(pts), 0.2, order, stats=stats)
        assert np.array_equal(keep.cpu().numpy(), want), (case, seed, int((keep.cpu().numpy() != want).sum()))
        assert rounds >= 1 and stats["rounds"] == rounds
    if case == "clump":
        assert stats["edges"] > 1_000_000


def test_reduce_points_200k_cloud_and_repeat():
    from mdfnet_hip import ops, synth
    pts = synth.dtu_eval_scene(1000, 200_000, seed=5, half=20.0)["qdata"].astype(np.float64)
    order = np.random.RandomState(0).permutation(len(pts))
    want = O.reduce_pts(pts, 0.2, order)
    s1, s2 = {}, {}
    k1, r1 = ops.reduce_points(gpu(pts), 0.2, order, stats=s1)
    k2, r2 = ops.reduce_points(gpu(pts), 0.2, order, stats=s2)
    assert np.array_equal(k1.cpu().numpy(), want)
    assert torch.equal(k1, k2) and (r1, s1["edges"]) == (r2, s2["edges"])
    assert 0.05 < want.mean() < 0.9


def test_masks_identical():
    from mdfnet_hip import ops
    rng = np.random.RandomState(2)
    obs = rng.rand(40, 30, 20) > 0.5
    bb = np.array([[0.0, 0.0, 0.0], [20.0, 15.0, 10.0]])
    res = 0.5
    q = rng.uniform(-2, 22, (20000, 3))
    q[:2000] = (rng.randint(-2, 44, (2000, 3)) + 0.5) * res - res    # (q - BB1)/Res + 1 lands on halves
    q[2000:2100] = -0.75                                              # Qv = -0.5: rounds to -1
    stl = rng.uniform(-5, 5, (5000, 3))
    plane = np.array([0.3, -0.2, 1.0, 0.5])
    inm, above = ops.dtu_masks(gpu(q), obs, bb, res, gpu(stl), plane)
    want = O.data_in_mask(q, obs, bb, res)
    assert np.array_equal(inm.cpu().numpy(), want) and 0.1 < want.mean() < 0.9
    assert np.array_equal(above.cpu().numpy(), O.stl_above_plane(stl, plane))
    inm_t, _ = ops.dtu_masks(gpu(q), torch.from_numpy(obs), bb, res, gpu(stl), plane)     # mask given as a tensor
    assert torch.equal(inm_t, inm)


def test_eval_scan_against_oracle():
    from mdfnet_hip import ops, synth
    sc = synth.dtu_eval_scene(20000, 40000, seed=3, half=60.0)
    got = ops.dtu_eval_scan(sc["qdata"], sc["qstl"], sc["obs_mask"], sc["bb"], sc["res"], sc["plane"], seed=1)
    want = O.eval_scan(sc["qdata"], sc["qstl"], sc["obs_mask"], sc["bb"], sc["res"], sc["plane"], seed=1)
    for k in ("Qdata", "Ddata", "Qstl", "Dstl", "DataInMask", "StlAbovePlane"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("nData", "nStl", "MedData", "MedStl"):
        assert got[k] == want[k], k
    for k in ("MeanData", "MeanStl", "VarData", "VarStl"):
        assert np.isclose(got[k], want[k], rtol=1e-12), k
    assert got["nData"] > 1000 and got["nStl"] > 1000 and (got["Ddata"] == 60.0).any()


def test_driver_end_to_end(tmp_path):
    """tools/dtu_eval/main.py on a synthetic DTU tree (MAT files by write_mat, PLYs by write_ply) in a fresh process, twice:
    the second run reuses the results; a fresh run into another folder is bit-identical."""
    from mdfnet_hip import synth
    scenes = {1: synth.dtu_eval_scene(8000, 16000, seed=1, half=40.0), 4: synth.dtu_eval_scene(6000, 9000, seed=2, half=40.0)}
    data, ply = str(tmp_path / "MVS Data"), str(tmp_path / "ply")
    O.write_dtu_tree(data, ply, scenes)
    cmd = [sys.executable, os.path.join(ROOT, "mdf-net_amd", "tools", "dtu_eval", "main.py"), "--data_path", data, "--ply_path", ply,
           "--scans", "1,4"]
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "final evaluation result on all scans" in r.stdout
    means = []
    for cset, sc in scenes.items():
        want = O.eval_scan(sc["qdata"].astype(np.float32).astype(np.float64), sc["qstl"].astype(np.float32).astype(np.float64),
                           sc["obs_mask"], sc["bb"], sc["res"], sc["plane"])
        with np.load(os.path.join(ply, f"ours_Eval_{cset}.npz")) as z:
            for k in ("Qdata", "Ddata", "Qstl", "Dstl", "DataInMask", "StlAbovePlane"):
                assert np.array_equal(z[k], want[k]), (cset, k)
            assert z["Margin"] == 10 and z["dst"] == 0.2 and z["GroundPlane"].shape == (4, 1)
        line = [l for l in r.stdout.splitlines() if l.startswith(f"scan {cset}: mean/median")][0]
        assert f"{want['MeanData']:f}/{want['MedData']:f}" in line and f"{want['MeanStl']:f}/{want['MedStl']:f}" in line
        means.append((want["MeanData"], want["MeanStl"]))
    acc, comp = np.mean([m[0] for m in means]), np.mean([m[1] for m in means])
    assert f"acc.: {acc:f}, comp.: {comp:f}, overall: {(acc + comp) / 2:f}" in r.stdout
    r2 = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r2.returncode == 0 and r2.stdout.count("reusing") == 2
    r3 = subprocess.run(cmd + ["--results_path", str(tmp_path / "again")], capture_output=True, text=True, timeout=600, env=env)
    assert r3.returncode == 0, r3.stderr
    for cset in scenes:
        with np.load(os.path.join(ply, f"ours_Eval_{cset}.npz")) as a, np.load(str(tmp_path / "again" / f"ours_Eval_{cset}.npz")) as b:
            for k in a.files:
                assert np.array_equal(a[k], b[k]), k


def test_abi_error_paths():
    import mdfnet_hip
    l = mdfnet_hip.lib()
    pts = gpu(np.random.RandomState(0).rand(100, 3))
    nb = l.mdf_pts_index_workspace(100)
    buf = torch.empty(nb, device=DEV, dtype=torch.uint8)
    s = None
    assert l.mdf_pts_index_workspace(-1) == 0
    assert l.mdf_pts_index_build(pts.data_ptr(), -5, buf.data_ptr(), nb, s) == -1 and b"out of range" in l.mdf_last_error()
    assert l.mdf_pts_index_build(None, 100, buf.data_ptr(), nb, s) == -1 and b"null" in l.mdf_last_error()
    assert l.mdf_pts_index_build(pts.data_ptr(), 100, None, nb, s) == -1 and b"null" in l.mdf_last_error()
    assert l.mdf_pts_index_build(pts.data_ptr(), 100, buf.data_ptr(), nb - 1, s) == -1 and b"too small" in l.mdf_last_error()
    assert l.mdf_pts_index_build(pts.data_ptr(), 100, buf.data_ptr(), nb, s) == 0
    dist = torch.empty(100, device=DEV, dtype=torch.float64)
    assert l.mdf_pts_nn_dist(buf.data_ptr(), 100, nb, None, pts.data_ptr(), -1, 0, None, 60.0, dist.data_ptr(), None, s) == -1
    assert l.mdf_pts_nn_dist(buf.data_ptr(), 100, nb, None, pts.data_ptr(), 100, 0, None, 0.0, dist.data_ptr(), None, s) == -1
    assert b"cap" in l.mdf_last_error()
    assert l.mdf_pts_nn_dist(buf.data_ptr(), 100, nb, None, pts.data_ptr(), 100, 0, None, 60.0, None, None, s) == -1
    assert l.mdf_pts_nn_dist(buf.data_ptr(), 100, nb, buf.data_ptr(), pts.data_ptr(), 100, nb, None, 60.0, dist.data_ptr(), None,
                             s) == -1 and b"exactly one" in l.mdf_last_error()
    assert l.mdf_pts_nn_dist(buf.data_ptr(), 100, nb // 2, None, pts.data_ptr(), 100, 0, None, 60.0, dist.data_ptr(), None, s) == -1
    rank = torch.arange(100, device=DEV, dtype=torch.int32)
    wb = l.mdf_pts_reduce_workspace(100)
    ws = torch.empty(wb, device=DEV, dtype=torch.uint8)
    edges = torch.zeros(1, device=DEV, dtype=torch.int64)
    assert l.mdf_pts_reduce_count(buf.data_ptr(), 100, nb, rank.data_ptr(), 0.0, ws.data_ptr(), wb, edges.data_ptr(), s) == -1
    assert b"dst" in l.mdf_last_error()
    assert l.mdf_pts_reduce_count(buf.data_ptr(), 100, nb, rank.data_ptr(), -0.2, ws.data_ptr(), wb, edges.data_ptr(), s) == -1
    assert l.mdf_pts_reduce_count(buf.data_ptr(), 100, nb, rank.data_ptr(), 0.2, ws.data_ptr(), wb - 16, edges.data_ptr(), s) == -1
    assert b"too small" in l.mdf_last_error()
    assert l.mdf_pts_reduce_count(buf.data_ptr(), 100, nb, None, 0.2, ws.data_ptr(), wb, edges.data_ptr(), s) == -1
    assert l.mdf_pts_reduce_count(buf.data_ptr(), 100, nb, rank.data_ptr(), 0.2, ws.data_ptr(), wb, edges.data_ptr(), s) == 0
    keep = torch.empty(100, device=DEV, dtype=torch.uint8)
    state = torch.zeros(3, device=DEV, dtype=torch.int32)
    assert l.mdf_pts_reduce(buf.data_ptr(), 100, nb, rank.data_ptr(), 0.2, ws.data_ptr(), wb, None, -1, 0, 8, keep.data_ptr(),
                            state.data_ptr(), s) == -1
    assert l.mdf_pts_reduce(buf.data_ptr(), 100, nb, rank.data_ptr(), 0.2, ws.data_ptr(), wb, None, 0, 0, -1, keep.data_ptr(),
                            state.data_ptr(), s) == -1
    # a CSR that does not fit is reported, not written past
    if int(edges.item()) > 0:
        small = torch.empty(1, device=DEV, dtype=torch.int32)
        assert l.mdf_pts_reduce(buf.data_ptr(), 100, nb, rank.data_ptr(), 0.2, ws.data_ptr(), wb, small.data_ptr(), 0, 0, 8,
                                keep.data_ptr(), state.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert state.tolist()[2] == 1
    bb = (ctypes.c_double * 6)(0, 0, 0, 1, 1, 1)
    plane = (ctypes.c_double * 4)(0, 0, 1, 0)
    om = torch.ones(8, device=DEV, dtype=torch.uint8)
    out = torch.empty(100, device=DEV, dtype=torch.uint8)
    assert l.mdf_dtu_masks(pts.data_ptr(), -1, om.data_ptr(), 2, 2, 2, bb, 0.5, out.data_ptr(), pts.data_ptr(), 100, plane,
                           out.data_ptr(), s) == -1
    assert l.mdf_dtu_masks(pts.data_ptr(), 100, None, 2, 2, 2, bb, 0.5, out.data_ptr(), pts.data_ptr(), 100, plane,
                           out.data_ptr(), s) == -1
    assert l.mdf_dtu_masks(pts.data_ptr(), 100, om.data_ptr(), 2, 2, 2, bb, 0.0, out.data_ptr(), pts.data_ptr(), 100, plane,
                           out.data_ptr(), s) == -1 and b"res" in l.mdf_last_error()
    assert l.mdf_dtu_masks(pts.data_ptr(), 100, om.data_ptr(), 2, -2, 2, bb, 0.5, out.data_ptr(), pts.data_ptr(), 100, plane,
                           out.data_ptr(), s) == -1
    from mdfnet_hip import ops
    with pytest.raises(ValueError, match="permutation"):
        ops.reduce_points(pts, 0.2, np.zeros(100, dtype=np.int64))
    with pytest.raises(ValueError, match="dst"):
        ops.reduce_points(pts, 0.0, np.arange(100))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.point_index(torch.zeros(4, 3, dtype=torch.float64))
    torch.cuda.synchronize()
