"""CPU: the meshing oracle (tests/tsdf_mesh_oracle.py) is itself sound, the mesh PLY round-trips, and the driver parses its flags
and names the missing filter outputs.  The kernels are held to this oracle bit for bit in test_tsdf_mesh_gpu.py.

fp32 mirror against float64 (test 2).  The bound |D32 - D64| <= 8 * 2^-24 * V is met by scenes whose camera depths stay within a
few truncation distances: the fp32 chain of one view loses about (3 z / trunc + 1) * 2^-24 in f = (d - z) / trunc (three roundings
of magnitude ~z in the row of the extrinsic, one in the quotient) and 3 * 2^-24 in the running mean, so z / trunc <= (8 V - 4) / 3
is what the scene builders keep to: 8.9 <= 14.7 for the sphere at distance 4 (V = 6), about 4 <= 4.0 for the plane (V = 2: at the
worst-case model's limit), 11 <= 12 for the awkward set (V = 5).  Measured: 7.84, 3.60 and 7.69 x 2^-24 against the bounds 48, 16
and 40, no lattice point left out; the figures are printed by the test and recorded in DESIGN section 7."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_mesh_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- 1. topology and order
def lattice_keys(vertices, triangles, origin, voxel):
    """From float64 vertex positions: each vertex's (lattice index of its edge's owner, direction) as sortable tuples, and each
    triangle's cell (the componentwise floor of its smallest coordinates), both in lattice units (k, j, i)."""
    g = (np.asarray(vertices, np.float64) - np.asarray(origin, np.float64)) / float(voxel)
    near = np.abs(g - np.round(g)) < 1e-6
    g = np.where(near, np.round(g), g)
    base = np.floor(g).astype(np.int64)
    d = (~near).astype(np.int64) @ np.array([1, 2, 4])
    cell = np.floor(g[np.asarray(triangles)].min(axis=1)).astype(np.int64)
    return base, d, cell


def assert_closed_sphere(vertices, triangles):
    top = O.topology(vertices, triangles)
    assert top["closed"], "an edge is not shared by exactly two triangles in opposite directions"
    assert top["euler"] == 2, top
    assert top["volume"] > 0, top
    assert top["all_referenced"], top
    return top


@pytest.mark.parametrize("dims", [(6, 6, 6), (12, 12, 12), (33, 17, 9)])
def test_oracle_mesh_of_a_sphere_is_a_closed_oriented_manifold_in_order(dims):
    D, W, origin, voxel, centre, radius = O.sphere_field(dims, np.float64)
    v, t = O.marching_tets(D, W, origin, voxel, 1, dt=np.float64)
    assert len(v) > 0 and len(t) > 0
    top = assert_closed_sphere(v, t)
    assert abs(top["volume"] / (4 / 3 * np.pi * radius ** 3) - 1) < 0.35, top       # a coarse polyhedron inside the sphere's shell
    nx, ny, nz = dims
    base, d, cell = lattice_keys(v, t, origin, voxel)
    assert (d > 0).all()
    vkey = ((base[:, 2] * ny + base[:, 1]) * nx + base[:, 0]) * 8 + d
    assert (np.diff(vkey) > 0).all(), "vertices are not in increasing (lattice index, d)"
    ckey = (cell[:, 2] * ny + cell[:, 1]) * nx + cell[:, 0]
    assert (np.diff(ckey) >= 0).all(), "triangles are not in increasing cell index"
    # the fp32 mesh of the same field has the same connectivity
    v32, t32 = O.marching_tets(D.astype(np.float32), W.astype(np.float32), origin, voxel, 1)
    if np.array_equal(D.astype(np.float32) < 0, D < 0):
        np.testing.assert_array_equal(t32, t)
        assert np.abs(v32.astype(np.float64) - v).max() < 1e-5 * max(1.0, np.abs(v).max())


def test_oracle_mesh_with_exact_zeros_is_still_a_manifold_by_index():
    """D == 0 counts as outside: the vertices of its edges coincide with the lattice point (zero-area triangles), the index
    structure stays closed."""
    D, W, origin, voxel, _, _ = O.sphere_field((9, 9, 9), np.float32)
    D[np.abs(D) < 0.12] = 0.0
    assert (D == 0).sum() > 10
    v, t = O.marching_tets(D, W, origin, voxel, 1)
    top = O.topology(v, t)
    assert top["closed"] and top["euler"] == 2 and top["all_referenced"], top


def test_oracle_mesh_needs_observed_cells_and_a_sign_change():
    D, W, origin, voxel, _, _ = O.sphere_field((7, 6, 5), np.float32)
    for v, t in (O.marching_tets(np.abs(D) + 0.1, W, origin, voxel), O.marching_tets(D, np.zeros_like(W), origin, voxel),
                 O.marching_tets(D, W, origin, voxel, min_weight=2)):
        assert v.shape == (0, 3) and t.shape == (0, 3) and t.dtype == np.int32


# ---------------------------------------------------------------------------------------------------- 2. fp32 mirror vs float64
def scenes_for_precision():
    return {"sphere": O.sphere_scene((12, 12, 12), h=48, w=64, dist=4.0), "plane": O.plane_scene((12, 11, 10)),
            "awkward": O.awkward_scene((9, 9, 9))}


@pytest.mark.parametrize("name", ["sphere", "plane", "awkward"])
def test_fp32_mirror_against_float64(name):
    sc = scenes_for_precision()[name]
    nviews = len(sc["depths"])
    tr32, tr64 = [], []
    args = (sc["depths"], sc["K"], sc["E"], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"])
    D32, W32 = O.integrate(*args, dt=np.float32, trace=tr32)
    D64, W64 = O.integrate(*args, dt=np.float64, trace=tr64)
    differ = np.zeros(D32.shape, bool)
    for (ok_a, u_a, v_a), (ok_b, u_b, v_b) in zip(tr32, tr64):
        differ |= (ok_a != ok_b) | (ok_a & ((u_a != u_b) | (v_a != v_b)))
    share = differ.mean()
    keep = ~differ
    err = np.abs(D32.astype(np.float64) - D64)[keep].max()
    print(f"{name}: V={nviews}, {differ.sum()} of {differ.size} lattice points left out ({100 * share:.3f} %), "
          f"max |D32 - D64| = {err / EPS:.2f} * 2^-24 (bound {8 * nviews}), observed points {int((W64 > 0).sum())}")
    assert (W64 > 0).mean() > 0.2, "the scene observes too little of the lattice to test anything"
    assert share <= 0.005
    np.testing.assert_array_equal(W32[keep], W64[keep])
    assert err <= 8 * EPS * nviews


def test_awkward_scene_has_what_it_promises():
    sc = O.awkward_scene((9, 9, 9))
    x, y, z = O.lattice_points(sc["origin"], sc["voxel"], sc["dims"], np.float32)
    E = sc["E"]
    pz1 = E[1, 2, 0] * x + E[1, 2, 1] * y + E[1, 2, 2] * z + E[1, 2, 3]
    assert (pz1 <= 0).any() and (pz1 > 0).any()                        # a camera inside the volume
    bad = sc["depths"][2]
    assert np.isnan(bad).any() and np.isposinf(bad).any() and (bad == 0).any() and (bad < 0).any()
    sdf = np.float32(2.5) - (z + np.float32(3.0))                      # view 0: exact in fp32
    assert (sdf == -sc["trunc"]).any() and (sdf == sc["trunc"]).any() and (sdf == 0).any()
    D, W = O.integrate(sc["depths"][3:4], sc["K"][3:4], sc["E"][3:4], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"])
    assert not W.any()                                                 # the view that looks away sees nothing
    D, W = O.integrate(sc["depths"][:1], sc["K"][:1], sc["E"][:1], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"])
    hit = W > 0
    plane = np.broadcast_to(sdf, W.shape)
    assert (D[hit & (plane == -sc["trunc"])] == -1).all() and (hit & (plane == -sc["trunc"])).any()    # sdf = -trunc is kept
    assert (D[hit & (plane >= sc["trunc"])] == 1).all() and not (hit & (plane < -sc["trunc"])).any()


# ---------------------------------------------------------------------------------------------------- 3. the sphere scene
@pytest.mark.parametrize("dims", [(33, 33, 33), (41, 37, 35)])
def test_sphere_scene_vertices_lie_within_a_voxel_of_the_sphere(dims):
    """A condition on the scene (6 far cameras, truncation 3 voxels, radius >= 10 voxels), not a tolerance on a kernel."""
    sc = O.sphere_scene(dims)
    assert all(float(np.nanmax(d)) / float(k[0, 0]) <= 0.5 * float(sc["voxel"]) * 1.05 for d, k in zip(sc["depths"], sc["K"]))
    D, W = O.integrate(sc["depths"], sc["K"], sc["E"], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"], dt=np.float64)
    v, t = O.marching_tets(D, W, sc["origin"], sc["voxel"], 1, dt=np.float64)
    assert_closed_sphere(v, t)
    off = np.abs(np.linalg.norm(v - np.asarray(O.SPHERE_CENTRE), axis=1) - O.SPHERE_RADIUS) / float(sc["voxel"])
    print(f"sphere scene {dims}: {len(v)} vertices, {len(t)} triangles, max distance to the sphere {off.max():.3f} voxels")
    assert off.max() <= 1.0


# ---------------------------------------------------------------------------------------------------- 4. PLY
def test_mesh_ply_round_trip_and_byte_layout(tmp_path):
    from tools.data_io import write_ply_mesh, read_ply_mesh, read_ply_vertices
    rng = np.random.RandomState(0)
    xyz = rng.randn(5, 3).astype(np.float32)
    rgb = rng.randint(0, 256, (5, 3)).astype(np.uint8)
    faces = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 3]], np.int32)
    path = str(tmp_path / "m.ply")
    write_ply_mesh(path, xyz, rgb, faces)
    raw = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 3\n"
              b"property list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header)
    body = raw[len(header):]
    assert len(body) == 5 * 15 + 3 * 13
    assert body[:12] == xyz[0].astype("<f4").tobytes() and body[12:15] == rgb[0].tobytes()
    assert body[75:76] == b"\x03" and body[76:88] == faces[0].astype("<i4").tobytes()
    x2, c2, f2 = read_ply_mesh(path)
    np.testing.assert_array_equal(x2, xyz)
    np.testing.assert_array_equal(c2, rgb)
    np.testing.assert_array_equal(f2, faces)
    assert f2.dtype == np.int32 and c2.dtype == np.uint8 and x2.dtype == np.float32
    np.testing.assert_array_equal(read_ply_vertices(path), xyz.astype(np.float64))      # the general reader skips the faces
    write_ply_mesh(path, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    x0, c0, f0 = read_ply_mesh(path)
    assert x0.shape == (0, 3) and c0.shape == (0, 3) and f0.shape == (0, 3)
    with pytest.raises(ValueError, match="out of range"):
        write_ply_mesh(path, xyz, rgb, np.array([[0, 1, 5]]))


# ---------------------------------------------------------------------------------------------------- 5. driver
def write_scene_on_disk(tmp_path, scan, scene, images, filter_outputs=True, filter_folder="filter"):
    """A `-d scene` folder <root>/<scan>/{pair.txt, images/*.jpg, cams/*_cam.txt} and, with filter_outputs, the filter's
    <eval>/<scan>/<filter>/<v>_depth_est.pfm and <eval>/<scan>/<scan>.ply (the back-projected valid texels).  -> (root, eval)."""
    from PIL import Image
    from tools.data_io import save_pfm, write_ply
    root, ev = tmp_path / "data", tmp_path / "outputs"
    sd = root / scan
    for d in (sd / "images", sd / "cams", ev / scan / filter_folder):
        d.mkdir(parents=True, exist_ok=True)
    n = len(scene["depths"])
    with open(sd / "pair.txt", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            srcs = [j for j in range(n) if j != i][:3]
            f.write(f"{i}\n{len(srcs)} " + " ".join(f"{j} {10 - k}.0" for k, j in enumerate(srcs)) + "\n")
    points = []
    for i in range(n):
        name = f"{i:08d}"
        Image.fromarray(images[i]).save(str(sd / "images" / (name + ".jpg")), quality=95)
        with open(sd / "cams" / (name + "_cam.txt"), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in scene["E"][i]) + "\n\n")
            f.write("intrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in scene["K"][i]) + "\n\n")
            f.write("1.0 0.1\n")
        if filter_outputs:
            dep = scene["depths"][i]
            save_pfm(str(ev / scan / filter_folder / f"{i}_depth_est.pfm"), dep)
            c, dirs = O.pixel_rays(scene["K"][i], scene["E"][i], *dep.shape)
            points.append((c + dirs * dep[..., None].astype(np.float64))[dep > 0])
    if filter_outputs:
        pts = np.concatenate(points)
        write_ply(str(ev / scan / (scan + ".ply")), pts, np.full((len(pts), 3), 200, np.uint8))
    return root, ev


def test_driver_arguments():
    from tools.mesh import main as M
    a = M.build_parser().parse_args(["-d", "scene", "-r", "R", "-e", "E", "--scans", "a,b"])
    assert (a.resolution, a.voxel, a.trunc, a.min_weight, a.filter_folder, a.outply_folder) == (512, None, 3.0, 1, "filter", None)
    assert M.scans_of(a) == ("R", ["a", "b"], "images", "cams")
    a = M.build_parser().parse_args(["-d", "tanks", "-s", "advanced", "-r", "R", "-e", "E", "-o", "P", "-f", "flt", "--resolution", "256",
                                     "--voxel", "0.5", "--trunc", "4", "--min_weight", "2"])
    assert (a.resolution, a.voxel, a.trunc, a.min_weight, a.filter_folder, a.outply_folder) == (256, 0.5, 4.0, 2, "flt", "P")
    root, scans, img, cam = M.scans_of(a)
    assert root == os.path.join("R", "TankandTemples", "advanced") and "Temple" in scans and cam == "cams_1"
    assert M.scans_of(M.build_parser().parse_args(["-d", "dtu", "-r", "R"]))[0] == os.path.join("R", "dtu1600x1200")
    for bad in (["-d", "scene"], ["-d", "nothing"]):
        with pytest.raises(SystemExit):
            M.scans_of(M.build_parser().parse_args(bad))
    for bad in (["--voxel", "0"], ["--trunc", "-1"], ["--resolution", "6"], ["--min_weight", "0"]):
        with pytest.raises(SystemExit):
            M.check_args(M.build_parser().parse_args(bad))


def test_driver_box():
    from tools.mesh import main as M
    rng = np.random.RandomState(2)
    pts = rng.rand(5000, 3) * np.array([4.0, 2.0, 1.0]) + np.array([10.0, -3.0, 0.5])
    origin, voxel, dims, tau = M.mesh_box(pts, resolution=64, trunc=3.0)
    assert dims[0] == 64 and dims[1] < dims[0] and dims[2] < dims[1]
    assert tau == np.float32(3.0) * voxel and origin.dtype == np.float32
    lo, hi = np.quantile(pts, 0.01, axis=0), np.quantile(pts, 0.99, axis=0)
    end = origin.astype(np.float64) + float(voxel) * (np.array(dims) - 1)
    grown_lo, grown_hi = lo - 0.05 * (hi - lo) - float(tau), hi + 0.05 * (hi - lo) + float(tau)
    assert (origin <= grown_lo + 1e-5).all() and (end >= grown_hi - 1e-5).all() and (end <= grown_hi + float(voxel)).all()
    o2, v2, d2, t2 = M.mesh_box(pts, voxel=0.25, trunc=2.0)
    assert v2 == np.float32(0.25) and t2 == np.float32(0.5)
    side = (hi - lo) * 1.1 + 2 * 0.5
    assert d2 == tuple(int(np.ceil(s / 0.25 - 1e-4)) + 1 for s in side)
    np.testing.assert_allclose(o2, lo - 0.05 * (hi - lo) - 0.5, rtol=1e-6)


def test_driver_names_the_command_that_writes_missing_filter_outputs(tmp_path):
    from tools.mesh import main as M
    sc = O.sphere_scene((6, 6, 6), h=8, w=10)
    root, ev = write_scene_on_disk(tmp_path, "ball", sc, O.scene_images(sc), filter_outputs=False)
    args = M.build_parser().parse_args(["-d", "scene", "-r", str(root), "-e", str(ev), "--scans", "ball"])
    with pytest.raises(M.MissingFilterOutput) as e:
        M.load_scan(args, *[x if i != 1 else "ball" for i, x in enumerate(M.scans_of(args))])
    msg = str(e.value)
    assert "tools/filter/dynamic_filter_gpu.py -d scene" in msg and "--scans ball" in msg and "0_depth_est.pfm" in msg
    root, ev = write_scene_on_disk(tmp_path, "ball", sc, O.scene_images(sc))
    got = M.load_scan(args, str(root), "ball", "images", "cams")
    np.testing.assert_array_equal(got["depths"], np.stack(sc["depths"]))
    np.testing.assert_array_equal(got["K"], sc["K"])
    np.testing.assert_array_equal(got["E"], sc["E"])
    assert got["images"].shape == (6, 8, 10, 3) and got["images"].dtype == np.uint8 and len(got["points"]) > 0


# ---------------------------------------------------------------------------------------------------- 6. no CPU fallback
def test_ops_refuse_cpu_tensors():
    from mdfnet_hip import ops
    sc = O.plane_scene((5, 5, 5), h=5, w=7)
    dep = torch.from_numpy(np.stack(sc["depths"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsdf_integrate(dep, sc["K"], sc["E"], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsdf_mesh(torch.zeros(3, 3, 3), torch.ones(3, 3, 3), sc["origin"], sc["voxel"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_colour(torch.zeros(4, 3), dep, torch.zeros(2, 5, 7, 3, dtype=torch.uint8), sc["K"], sc["E"], sc["trunc"])
