"""CPU: the DTU evaluation's oracle (tests/dtu_eval_oracle.py) on analytic cases, the literal MaxDistCP loop against the
"exact nearest neighbour + region + cap" formulation the kernel implements, the masks' rounding, the PLY / MAT readers and the
driver's statistics from stored results."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import dtu_eval_oracle as O  # noqa: E402


# ---------------------------------------------------------------------------------------------------- reducePts
def test_reduce_chain_depends_on_the_order():
    """Points 0.15 apart on a line, dst 0.2: each point neighbours only the next one, so the kept set follows the order."""
    pts = np.stack([np.arange(6) * 0.15, np.zeros(6), np.zeros(6)], 1)
    assert O.reduce_pts(pts, 0.2, [0, 1, 2, 3, 4, 5]).tolist() == [1, 0, 1, 0, 1, 0]
    assert O.reduce_pts(pts, 0.2, [5, 4, 3, 2, 1, 0]).tolist() == [0, 1, 0, 1, 0, 1]
    assert O.reduce_pts(pts, 0.2, [1, 4, 0, 2, 3, 5]).tolist() == [0, 1, 0, 0, 1, 0]
    # a greedy result is maximal and independent
    keep = O.reduce_pts(pts, 0.2, [2, 5, 0, 3, 1, 4])
    assert not (keep[:-1] & keep[1:]).any() and all(keep[i] or keep[i - 1] or keep[i + 1] for i in range(1, 5))


def test_reduce_distance_exactly_dst_is_a_neighbour():
    """rangesearch is inclusive: two points exactly dst apart (0.25 is exact in binary) are neighbours; 0.25 + 1 ulp is not."""
    dst = 0.25
    pts = np.array([[0.0, 0.0, 0.0], [dst, 0.0, 0.0]])
    assert O.reduce_pts(pts, dst, [0, 1]).tolist() == [True, False]
    pts[1, 0] = np.nextafter(dst, 1.0)
    assert O.reduce_pts(pts, dst, [0, 1]).tolist() == [True, True]


def test_reduce_duplicates_and_brute_force():
    rng = np.random.RandomState(3)
    pts = rng.uniform(0, 1.0, (400, 3))
    pts[100:120] = pts[7]                                            # exact duplicates
    order = rng.permutation(len(pts))
    keep = O.reduce_pts(pts, 0.2, order)
    ref = np.ones(len(pts), dtype=bool)                              # O(n^2) restatement of the loop
    d = np.sqrt(O.dist2(pts[:, None, :], pts[None, :, :]))
    for i in order:
        if ref[i]:
            ref[d[i] <= 0.2] = False
            ref[i] = True
    assert (keep == ref).all()
    assert keep[[7] + list(range(100, 120))].sum() <= 1


# ---------------------------------------------------------------------------------------------------- MaxDistCP
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_literal_maxdistcp_equals_capped_nn_in_region(seed):
    """MaxDistCP's box loop equals "exact NN if the point lies in the cubes and d < 60, else 60" wherever that is < 60, and is
    >= 60 elsewhere: points outside BB, far outliers, an empty neighbourhood and points on cube faces included."""
    rng = np.random.RandomState(seed)
    bb = np.array([[-100.0, -80.0, -50.0], [100.0, 95.0, 40.0]])
    to = np.concatenate([rng.uniform(-100, 100, (1500, 3)) * [1, 0.9, 0.4], rng.uniform(-200, 200, (30, 3))])
    frm = np.concatenate([rng.uniform(-100, 100, (1200, 3)) * [1, 0.9, 0.4] + rng.normal(0, 2, (1200, 3)),
                          rng.uniform(-250, 250, (300, 3)),                    # outside BB / far from everything
                          np.array([[-100.0, -80.0, -50.0], [-40.0, -20.0, 10.0], [20.0, 100.0 - 5, 10.0],
                                    [bb[0, 0] + 4 * 60.0, 0.0, 0.0]])])       # on cube faces, past the last cube
    lit = O.max_dist_cp(to, frm, bb, 60.0)
    cap = O.nn_capped(to, frm, bb, 60.0)
    below = cap < 60.0
    assert below.sum() > 1000 and (~below).sum() > 50
    assert np.array_equal(lit[below], cap[below])
    assert (lit[~below] >= 60.0).all()
    assert np.array_equal(np.minimum(lit, 60.0), cap)
    # no to-point at all: every distance is the cap
    assert (O.max_dist_cp(np.zeros((0, 3)), frm, bb, 60.0) == 60.0).all()
    assert (O.nn_capped(np.zeros((0, 3)), frm, bb, 60.0) == 60.0).all()


def test_region_is_the_union_of_cubes():
    bb = np.array([[0.0, 0.0, 0.0], [130.0, 59.0, 61.0]])            # ranges 2, 0, 1 -> 180 x 60 x 120 mm
    f = np.array([[0.0, 0.0, 0.0], [179.9, 59.9, 119.9], [180.0, 1, 1], [1, 60.0, 1], [1, 1, 120.0], [-1e-9, 1, 1]])
    assert O.in_region(f, bb, 60.0).tolist() == [True, True, False, False, False, False]


# ---------------------------------------------------------------------------------------------------- masks
def test_mask_rounds_halves_away_from_zero():
    """Qv = (q - BB1) / Res + 1 = k + 0.5 exactly rounds up (MATLAB), where numpy's round would go to the even neighbour."""
    obs = np.zeros((4, 4, 4), dtype=bool)
    obs[2, 0, 0] = True                                              # MATLAB index (3, 1, 1)
    bb = np.array([[0.0, 0.0, 0.0], [3.0, 3.0, 3.0]])
    q = np.array([[1.5, 0.0, 0.0],                                   # Qv 2.5 -> 3: in
                  [0.5, 0.0, 0.0],                                   # Qv 1.5 -> 2: out (numpy: 2 too)
                  [2.5, 0.0, 0.0],                                   # Qv 3.5 -> 4: out (numpy: 4)
                  [1.4999, 0.0, 0.0],                                # -> 2: out
                  [-0.5, 0.0, 0.0],                                  # Qv 0.5 -> 1 (numpy: 0, outside): obs(1,1,1) false
                  [2.0, -0.6, 0.0],                                  # Qv_y 0.4 -> 0: outside
                  [2.0, 0.0, 3.4]])                                  # Qv_z 4.4 -> 4: inside, false
    assert O.data_in_mask(q, obs, bb, 1.0).tolist() == [True, False, False, False, False, False, False]
    assert np.round(2.5) == 2.0 and O.matlab_round(np.array([2.5, -2.5, 0.5]))[0] == 3.0
    assert O.matlab_round(np.array([-2.5]))[0] == -3.0
    obs[0, 0, 0] = True
    assert O.data_in_mask(np.array([[-0.5, 0.0, 0.0], [-0.5000001, 0.0, 0.0]]), obs, bb, 1.0).tolist() == [True, False]


def test_mask_is_column_major():
    obs = np.zeros((3, 4, 5), dtype=bool)
    obs[1, 2, 3] = True
    bb = np.zeros((2, 3))
    assert O.data_in_mask(np.array([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]]), obs, bb, 1.0).tolist() == [True, False]


def test_plane():
    P = np.array([0.0, 0.0, 1.0, -2.0])
    q = np.array([[5.0, 5.0, 2.0], [0.0, 0.0, 2.5], [0.0, 0.0, 1.0]])
    assert O.stl_above_plane(q, P).tolist() == [False, True, False]


# ---------------------------------------------------------------------------------------------------- PLY
def _ply(path, fmt, props, rows, pre=None, post=None, extra_header=""):
    """A PLY written by hand: props [(type, name)], rows of values; pre / post: (name, [(type, name)], rows) elements."""
    codes = {"char": "b", "uchar": "B", "short": "h", "ushort": "H", "int": "i", "uint": "I", "float": "f", "double": "d"}
    head = ["ply", f"format {fmt} 1.0", "comment hand-written", extra_header]
    els = ([pre] if pre else []) + [("vertex", props, rows)] + ([post] if post else [])
    for name, pr, rw in els:
        head.append(f"element {name} {len(rw)}")
        for t, n in pr:
            head.append(f"property list uchar int {n}" if t == "list" else f"property {t} {n}")
    head.append("end_header")
    body = b""
    end = "<" if fmt == "binary_little_endian" else ">"
    for name, pr, rw in els:
        for r in rw:
            if fmt == "ascii":
                vals = []
                for (t, _), v in zip(pr, r):
                    vals += [str(len(v))] + [str(x) for x in v] if t == "list" else [repr(v)]
                body += (" ".join(vals) + "\n").encode()
            else:
                for (t, _), v in zip(pr, r):
                    body += struct.pack(end + "B" + "i" * len(v), len(v), *v) if t == "list" else struct.pack(end + codes[t], v)
    with open(path, "wb") as f:
        f.write(("\n".join(h for h in head if h) + "\n").encode() + body)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_read_ply_vertices_formats(tmp_path, fmt):
    from tools.data_io import read_ply_vertices
    xyz = [(1.5, -2.25, 3.0), (0.1, 0.2, 0.3), (-7.0, 8.5, 1e-3)]
    # doubles with extra properties before, between and after the coordinates
    props = [("uchar", "flag"), ("double", "x"), ("short", "s"), ("double", "y"), ("double", "z"), ("float", "nx")]
    rows = [(1, x, -3, y, z, 0.5) for x, y, z in xyz]
    _ply(tmp_path / "a.ply", fmt, props, rows)
    assert np.array_equal(read_ply_vertices(str(tmp_path / "a.ply")), np.array(xyz))
    # floats, another element (with a list property) before the vertices and faces after them
    props = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red")]
    rows = [(x, y, z, 7) for x, y, z in xyz]
    pre = ("camera", [("int", "id"), ("list", "ids")], [(1, (1, 2, 3)), (2, ())])
    post = ("face", [("list", "vertex_indices")], [((0, 1, 2),)])
    _ply(tmp_path / "b.ply", fmt, props, rows, pre=pre, post=post, extra_header="obj_info made by hand")
    got = read_ply_vertices(str(tmp_path / "b.ply"))
    want = np.array(xyz) if fmt == "ascii" else np.array(xyz, dtype=np.float32).astype(np.float64)     # text is read as written
    assert got.dtype == np.float64 and np.array_equal(got, want)
    # integer coordinates
    _ply(tmp_path / "c.ply", fmt, [("int", "x"), ("int", "y"), ("int", "z")], [(1, -2, 3), (4, 5, -6)])
    assert np.array_equal(read_ply_vertices(str(tmp_path / "c.ply")), np.array([[1, -2, 3], [4, 5, -6]], dtype=np.float64))


def test_read_ply_vertices_reads_write_ply(tmp_path):
    from tools.data_io import read_ply_vertices, write_ply
    xyz = np.random.RandomState(0).uniform(-300, 300, (1000, 3)).astype(np.float32)
    write_ply(str(tmp_path / "p.ply"), xyz, np.zeros((1000, 3), np.uint8))
    assert np.array_equal(read_ply_vertices(str(tmp_path / "p.ply")), xyz.astype(np.float64))
    write_ply(str(tmp_path / "n.ply"), xyz, np.zeros((1000, 3), np.uint8), normals=xyz)
    assert np.array_equal(read_ply_vertices(str(tmp_path / "n.ply")), xyz.astype(np.float64))


# ---------------------------------------------------------------------------------------------------- MAT
def _mat_arrays():
    rng = np.random.RandomState(1)
    return {"ObsMask": rng.rand(7, 5, 3) > 0.6, "BB": np.array([[-1.5, 2.0, 3.0], [4.0, 5.0, 6.25]]), "Res": np.float64(0.2),
            "P": np.array([[0.1], [0.2], [0.3], [-4.0]]), "i32": np.arange(12, dtype=np.int32).reshape(3, 4),
            "f32": rng.rand(2, 3).astype(np.float32)}


def test_mat_round_trip(tmp_path):
    from tools.data_io import read_mat, write_mat
    a = _mat_arrays()
    write_mat(str(tmp_path / "a.mat"), a)
    got = read_mat(str(tmp_path / "a.mat"))
    assert got["ObsMask"].dtype == np.bool_ and np.array_equal(got["ObsMask"], a["ObsMask"])
    assert np.array_equal(got["BB"], a["BB"]) and got["Res"].shape == (1, 1) and got["Res"][0, 0] == 0.2
    assert np.array_equal(got["P"], a["P"]) and np.array_equal(got["i32"], a["i32"]) and got["f32"].dtype == np.float32


def test_mat_compressed_and_column_major(tmp_path):
    """A zlib-compressed element (miCOMPRESSED) written by hand, holding a 2x3 double array in column-major order."""
    import zlib
    from tools.data_io import read_mat

    def el(t, payload):
        return struct.pack("<II", t, len(payload)) + payload + b"\0" * ((-len(payload)) % 8)
    data = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    sub = el(6, struct.pack("<II", 6, 0)) + el(5, struct.pack("<ii", 2, 3)) + struct.pack("<HH", 1, 1) + b"A\0\0\0" \
        + el(9, data.tobytes(order="F"))
    comp = zlib.compress(el(14, sub))
    head = b"MATLAB 5.0 MAT-file".ljust(116, b" ") + b"\0" * 8 + struct.pack("<H", 0x0100) + b"IM"
    (tmp_path / "c.mat").write_bytes(head + struct.pack("<II", 15, len(comp)) + comp)
    assert np.array_equal(read_mat(str(tmp_path / "c.mat"))["A"], data)


def test_mat_against_scipy_where_available(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from tools.data_io import read_mat, write_mat
    a = _mat_arrays()
    write_mat(str(tmp_path / "ours.mat"), a)
    theirs = sio.loadmat(str(tmp_path / "ours.mat"))
    for k, v in a.items():
        assert np.array_equal(np.asarray(theirs[k]).astype(np.asarray(v).dtype).reshape(np.shape(v) or (1, 1)),
                              np.asarray(v).reshape(np.shape(v) or (1, 1))), k
    for comp in (False, True):
        sio.savemat(str(tmp_path / "s.mat"), a, do_compression=comp)
        got = read_mat(str(tmp_path / "s.mat"))
        for k, v in a.items():
            assert np.array_equal(got[k].reshape(-1), np.asarray(v).reshape(-1, order="F")) or \
                np.array_equal(got[k], np.asarray(v).reshape(got[k].shape)), k
        assert np.array_equal(got["ObsMask"], a["ObsMask"])


# ---------------------------------------------------------------------------------------------------- driver statistics
def test_driver_statistics_from_stored_results(tmp_path, capsys):
    from mdfnet_hip import ops
    sys.path.insert(0, os.path.join(ROOT, "mdf-net_amd", "tools", "dtu_eval"))
    import importlib
    main = importlib.import_module("tools.dtu_eval.main")
    args = main.parse(["--data_path", str(tmp_path), "--ply_path", str(tmp_path), "--scans", "1,4"])
    rng = np.random.RandomState(5)
    expect = []
    for cset in (1, 4):
        ev = {"Ddata": rng.uniform(0, 30, 500), "DataInMask": rng.rand(500) > 0.3, "Dstl": rng.uniform(0, 60, 400),
              "StlAbovePlane": rng.rand(400) > 0.2}
        ev["Ddata"][:5] = 20.0                                       # the threshold itself is an outlier
        np.savez(main.scan_paths(args, cset)["result"], cSet=cset, Qdata=np.zeros((3, 500)), Qstl=np.zeros((3, 400)),
                 GroundPlane=np.zeros((4, 1)), dst=0.2, Margin=10, **ev)
        dd = ev["Ddata"][ev["DataInMask"]]
        ds = ev["Dstl"][ev["StlAbovePlane"]]
        expect.append((O.stat(dd[dd < 20]), O.stat(ds[ds < 20])))
    rows, (acc, comp, overall) = main.summary(args, [1, 4])
    for r, (sd, ss) in zip(rows, expect):
        assert (r["nData"], r["nStl"]) == (sd[0], ss[0]) and r["MedData"] == sd[3] and r["MedStl"] == ss[3]
        assert np.isclose(r["MeanData"], sd[1], rtol=1e-12) and np.isclose(r["VarStl"], ss[2], rtol=1e-12)
    assert np.isclose(acc, (expect[0][0][1] + expect[1][0][1]) / 2, rtol=1e-12)
    assert np.isclose(overall, (acc + comp) / 2, rtol=1e-15)
    out = capsys.readouterr().out
    assert "final evaluation result on all scans: acc.:" in out and "mean/median Data (acc.)" in out
    assert ops.dtu_stats([]) [0] == 0 and np.isnan(ops.dtu_stats([])[1]) and ops.dtu_stats([3.0])[2] == 0.0


def test_driver_reuses_existing_results(tmp_path):
    import importlib
    main = importlib.import_module("tools.dtu_eval.main")
    args = main.parse(["--data_path", str(tmp_path), "--ply_path", str(tmp_path), "--scans", "9"])
    assert args.scans == [9] and args.results_path == str(tmp_path) and args.dst == 0.2 and args.seed == 0
    path = main.scan_paths(args, 9)["result"]
    assert os.path.basename(path) == "ours_Eval_9.npz"
    np.savez(path, x=1)
    assert main.eval_scan(args, 9) == path                            # no PLY exists: only the reuse can succeed
    assert main.parse([]).scans == O.USED_SETS
