"""GPU: the meshing kernels (csrc/tsdf_mesh.hip) against the numpy oracle (tests/tsdf_mesh_oracle.py), bit for bit: D and W of
the integration for every chunking, continuation and with the brick culling off; vertices (as fp32 bit patterns) and triangles,
in order; colours; the argument errors of the four C-ABI entries; the mesh driver end to end in a child process.

Run as `python tests/test_tsdf_mesh_gpu.py child OUT.npz` this file integrates the culling cases and saves D and W (the parent
sets MDF_TSDF_CULL=0 for it)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import tsdf_mesh_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


def gpu(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared references are read-only)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    got, want = got.cpu().numpy() if torch.is_tensor(got) else got, np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][0]!r} != {want[bad][0]!r}"


# name -> scene: every lattice, view count, map size and scene of the issue's list appears at least once
def build_case(name):
    if name == "point-plane-1view-1x1":
        sc = O.plane_scene((1, 1, 1), h=1, w=1)
        return dict(sc, depths=sc["depths"][:1], K=sc["K"][:1], E=sc["E"][:1])
    if name == "2cube-plane-2views-7x5":
        return O.plane_scene((2, 2, 2), h=5, w=7)
    if name == "5x7x3-awkward-5views-7x5":
        return O.awkward_scene((5, 7, 3), h=5, w=7, nviews=5)
    if name == "5x7x3-awkward-70views-1x1":
        return O.awkward_scene((5, 7, 3), h=1, w=1, nviews=70)
    if name == "33x17x9-sphere-5views-64x48":
        return O.sphere_scene((33, 17, 9), h=48, w=64, nviews=5, dist=4.0, focal=60.0)
    if name == "33x17x9-awkward-5views-64x48":
        return O.awkward_scene((33, 17, 9), h=48, w=64, nviews=5)
    if name == "65x64x63-sphere-70views-64x48":
        return O.sphere_scene((65, 64, 63), h=48, w=64, nviews=70, dist=4.0, focal=70.0)
    if name == "65x64x63-plane-2views-64x48":
        return O.plane_scene((65, 64, 63), h=48, w=64)
    if name == "65x64x63-awkward-70views-7x5":
        return O.awkward_scene((65, 64, 63), h=5, w=7, nviews=70)
    raise KeyError(name)


CASES = ["point-plane-1view-1x1", "2cube-plane-2views-7x5", "5x7x3-awkward-5views-7x5", "5x7x3-awkward-70views-1x1",
         "33x17x9-sphere-5views-64x48", "33x17x9-awkward-5views-64x48", "65x64x63-sphere-70views-64x48",
         "65x64x63-plane-2views-64x48", "65x64x63-awkward-70views-7x5"]
CULL_CASES = ["5x7x3-awkward-5views-7x5", "33x17x9-sphere-5views-64x48", "33x17x9-awkward-5views-64x48", "65x64x63-sphere-70views-64x48",
              "65x64x63-awkward-70views-7x5"]
_reference = {}


def reference(name):
    """(scene, D, W) of the fp32 mirror, computed once and shared."""
    if name not in _reference:
        sc = build_case(name)
        D, W = O.integrate(sc["depths"], sc["K"], sc["E"], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"])
        D.setflags(write=False)
        W.setflags(write=False)
        _reference[name] = (sc, D, W)
    return _reference[name]


def integrate_gpu(sc, views=slice(None), **kw):
    from mdfnet_hip import ops
    dep = gpu(np.stack(sc["depths"][views]))
    return ops.tsdf_integrate(dep, sc["K"][views], sc["E"][views], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"], **kw)


# ---------------------------------------------------------------------------------------------------- 1. integration
@pytest.mark.parametrize("name", CASES)
def test_integration_is_bit_identical_to_the_fp32_mirror(name):
    sc, D, W = reference(name)
    nviews = len(sc["depths"])
    print(f"{name}: {int((W > 0).sum())} of {W.size} lattice points observed, W max {W.max():.0f}")
    gd, gw = integrate_gpu(sc)
    assert tuple(gd.shape) == sc["dims"][::-1]
    assert_same_bits(gd, D, "D")
    assert_same_bits(gw, W, "W")
    for chunk in (1, 3):
        cd, cw = integrate_gpu(sc, chunk=chunk)
        assert_same_bits(cd, D, f"D, chunk {chunk}")
        assert_same_bits(cw, W, f"W, chunk {chunk}")
    if nviews > 1:
        cut = max(1, nviews // 3)
        state = integrate_gpu(sc, slice(0, cut))
        sd, sw = integrate_gpu(sc, slice(cut, None), state=state, chunk=3)
        assert sd is state[0] and sw is state[1]
        assert_same_bits(sd, D, "D, continued from a state")
        assert_same_bits(sw, W, "W, continued from a state")


def test_culling_changes_no_bit(tmp_path):
    """MDF_TSDF_CULL=0 in a fresh child process: no brick skips a view; the same bits as the default (and as the mirror)."""
    out = str(tmp_path / "nocull.npz")
    env = dict(os.environ, MDF_TSDF_CULL="0")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "child", out], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    saved = np.load(out)
    assert "MDF_TSDF_CULL" not in os.environ
    for name in CULL_CASES:
        sc, D, W = reference(name)
        gd, gw = integrate_gpu(sc)
        assert_same_bits(saved[name + "/D"], gd.cpu().numpy(), f"{name}: D without culling against D with it")
        assert_same_bits(saved[name + "/W"], gw.cpu().numpy(), f"{name}: W without culling against W with it")
        assert_same_bits(saved[name + "/D"], D, f"{name}: D without culling")


def child(out):
    res = {}
    assert os.environ.get("MDF_TSDF_CULL") == "0"
    for name in CULL_CASES:
        gd, gw = integrate_gpu(build_case(name))
        res[name + "/D"], res[name + "/W"] = gd.cpu().numpy(), gw.cpu().numpy()
    np.savez(out, **res)


# ---------------------------------------------------------------------------------------------------- 2. mesh
def mesh_gpu(D, W, origin, voxel, min_weight=1):
    from mdfnet_hip import ops
    ops.count_begin()
    try:
        v, t = ops.tsdf_mesh(gpu(D), gpu(W), origin, voxel, min_weight)
    finally:
        calls = ops.count_end()
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    return v.cpu().numpy(), t.cpu().numpy(), calls


def assert_mesh_equals_oracle(D, W, origin, voxel, min_weight, what):
    wv, wt = O.marching_tets(D, W, origin, voxel, min_weight)
    gv, gt, calls = mesh_gpu(D, W, origin, voxel, min_weight)
    print(f"{what}, min_weight {min_weight}: {len(wv)} vertices, {len(wt)} triangles")
    assert_same_bits(gv, wv, f"{what}: vertices")
    np.testing.assert_array_equal(gt, wt, err_msg=f"{what}: triangles")
    assert ("mdf_mesh_emit" in calls) == (len(wt) > 0)
    return gv, gt


@pytest.mark.parametrize("name", CASES)
def test_mesh_is_identical_to_the_oracle_in_order(name):
    sc, D, W = reference(name)
    for min_weight in (1, 2):
        assert_mesh_equals_oracle(D, W, sc["origin"], sc["voxel"], min_weight, name)


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 7, 3), (12, 12, 12), (33, 17, 9), (65, 64, 63)])
def test_mesh_of_a_sphere_field_is_closed(dims):
    from test_tsdf_mesh_cpu import assert_closed_sphere
    D, W, origin, voxel, _, _ = O.sphere_field(dims)
    gv, gt = assert_mesh_equals_oracle(D, W, origin, voxel, 1, f"sphere field {dims}")
    if min(dims) >= 5:
        assert len(gt) > 0
        assert_closed_sphere(gv, gt)


def test_mesh_of_the_integrated_sphere_scene_is_closed():
    from test_tsdf_mesh_cpu import assert_closed_sphere
    sc = O.sphere_scene((33, 33, 33))
    gd, gw = integrate_gpu(sc)
    D, W = O.integrate(sc["depths"], sc["K"], sc["E"], sc["origin"], sc["voxel"], sc["dims"], sc["trunc"])
    assert_same_bits(gd, D, "D")
    assert_same_bits(gw, W, "W")
    gv, gt = assert_mesh_equals_oracle(D, W, sc["origin"], sc["voxel"], 1, "sphere scene 33^3")
    assert_closed_sphere(gv, gt)


def test_empty_meshes_launch_no_emit():
    D, W, origin, voxel, _, _ = O.sphere_field((7, 6, 5))
    for what, d, w, mw in (("no sign change", np.abs(D) + np.float32(0.1), W, 1), ("nobody observed it", D, np.zeros_like(W), 1),
                           ("all inside", -np.abs(D) - np.float32(0.1), W, 1), ("min_weight above every W", D, W, 2)):
        gv, gt, calls = mesh_gpu(d, w, origin, voxel, mw)
        assert gv.shape == (0, 3) and gt.shape == (0, 3), what
        assert calls.get("mdf_mesh_count") == 1 and "mdf_mesh_emit" not in calls, (what, calls)


def test_exact_zeros_give_a_manifold_by_index():
    D, W, origin, voxel, _, _ = O.sphere_field((9, 9, 9))
    D = D.copy()
    D[np.abs(D) < 0.12] = 0.0
    gv, gt = assert_mesh_equals_oracle(D, W, origin, voxel, 1, "sphere field with exact zeros")
    top = O.topology(gv, gt)
    assert top["closed"] and top["euler"] == 2 and top["all_referenced"], top
    p0, p1, p2 = (gv[gt[:, k]].astype(np.float64) for k in range(3))
    assert (np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1) == 0).any()       # zero-area triangles are there, and allowed


# ---------------------------------------------------------------------------------------------------- 3. colour
@pytest.mark.parametrize("name", ["33x17x9-awkward-5views-64x48", "65x64x63-sphere-70views-64x48", "2cube-plane-2views-7x5"])
def test_colours_are_identical_to_the_oracle(name):
    from mdfnet_hip import ops
    sc, D, W = reference(name)
    images = O.scene_images(sc)
    v, _ = O.marching_tets(D, W, sc["origin"], sc["voxel"], 1)
    # plus: a vertex no view sees, and the surface points behind the corner pixels of view 0 (on the image border)
    h, w = sc["depths"][0].shape
    c, dirs = O.pixel_rays(sc["K"][0], sc["E"][0], h, w)
    border = []
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        d = sc["depths"][0][y, x]
        border.append(c + dirs[y, x] * float(d if np.isfinite(d) and d > 0 else 1.0))
    v = np.concatenate([v, np.array([[1e4, -2e4, 3e4]], np.float32), np.array(border, np.float32)])
    want = O.colour(v, sc["depths"], images, sc["K"], sc["E"], sc["trunc"])
    got = ops.mesh_colour(gpu(v), gpu(np.stack(sc["depths"])), gpu(np.stack(images)), sc["K"], sc["E"], sc["trunc"])
    seen = (want != 128).any(axis=1)
    print(f"{name}: {len(v)} vertices, {int(seen.sum())} coloured by a view")
    assert got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert (want[len(v) - 5] == 128).all()
    if name != "2cube-plane-2views-7x5":
        assert seen.sum() > 10
    ok, u, vv, _ = O.project(sc["K"][0], sc["E"][0], v[-4:, 0], v[-4:, 1], v[-4:, 2], h, w, np.float32)
    assert ok.all() and set(zip(vv.tolist(), u.tolist())) == {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}


# ---------------------------------------------------------------------------------------------------- 4. argument errors
def test_argument_errors_return_minus_one_without_a_launch():
    import mdfnet_hip
    from mdfnet_hip import ops
    l = mdfnet_hip.lib()
    dev = torch.device("cuda")
    D, W = torch.zeros(3, 3, 3, device=dev), torch.zeros(3, 3, 3, device=dev)
    ops.tsdf_mesh(D, W, (0, 0, 0), 1.0)                              # a launch of this thread to compare against
    last = l.mdf_last_launch()
    dep = torch.ones(2, 2, device=dev)
    img = torch.zeros(2, 2, 3, device=dev, dtype=torch.uint8)
    dims, zero_dims = (ctypes.c_int * 3)(3, 3, 3), (ctypes.c_int * 3)(3, 0, 3)
    origin = (ctypes.c_float * 3)(0, 0, 0)
    maps, imgs = (ctypes.c_void_p * 1)(dep.data_ptr()), (ctypes.c_void_p * 1)(img.data_ptr())
    cams = np.zeros((1, ops.TSDF_CAM_FLOATS), np.float32)
    cp = cams.ctypes.data_as(ctypes.c_void_p)
    ws = torch.empty(ops.mesh_workspace_bytes(27), device=dev, dtype=torch.uint8)
    tot = torch.zeros(2, device=dev, dtype=torch.int64)
    vtx, tri = torch.zeros(4, 3, device=dev), torch.zeros(4, 3, device=dev, dtype=torch.int32)
    acc, rgb = torch.zeros(4, 4, device=dev), torch.zeros(4, 3, device=dev, dtype=torch.uint8)
    d, w_, f = D.data_ptr(), W.data_ptr(), ctypes.c_float

    def integrate(D=d, W=w_, dims=dims, voxel=1.0, trunc=1.0, maps=maps, chunk=0):
        return l.mdf_tsdf_integrate(D, W, dims, origin, f(voxel), f(trunc), maps, cp, 1, 2, 2, chunk, None)

    def count(D=d, dims=dims, voxel=1.0, mw=1.0, nbytes=ws.numel(), tot=tot.data_ptr()):
        return l.mdf_mesh_count(D, w_, dims, origin, f(voxel), f(mw), ws.data_ptr(), nbytes, tot, None)

    def emit(D=d, dims=dims, voxel=1.0, nv=4, nt=4, vtx=vtx.data_ptr()):
        return l.mdf_mesh_emit(D, w_, dims, origin, f(voxel), f(1.0), ws.data_ptr(), ws.numel(), nv, nt, vtx, tri.data_ptr(), None)

    def colour(vtx=vtx.data_ptr(), n=4, trunc=1.0, maps=maps, acc=acc.data_ptr()):
        return l.mdf_mesh_colour(vtx, n, maps, imgs, cp, 1, 2, 2, f(trunc), acc, rgb.data_ptr(), None)

    bad = {"integrate: null volume": lambda: integrate(D=None), "integrate: null W": lambda: integrate(W=None),
           "integrate: dims with a zero": lambda: integrate(dims=zero_dims), "integrate: trunc 0": lambda: integrate(trunc=0.0),
           "integrate: trunc < 0": lambda: integrate(trunc=-1.0), "integrate: voxel 0": lambda: integrate(voxel=0.0),
           "integrate: voxel < 0": lambda: integrate(voxel=-2.0), "integrate: null maps": lambda: integrate(maps=None),
           "integrate: chunk too large": lambda: integrate(chunk=17),
           "count: null volume": lambda: count(D=None), "count: dims with a zero": lambda: count(dims=zero_dims),
           "count: voxel 0": lambda: count(voxel=0.0), "count: min_weight 0": lambda: count(mw=0.0),
           "count: small workspace": lambda: count(nbytes=100), "count: null totals": lambda: count(tot=None),
           "emit: null volume": lambda: emit(D=None), "emit: dims with a zero": lambda: emit(dims=zero_dims),
           "emit: voxel < 0": lambda: emit(voxel=-1.0), "emit: null vertices": lambda: emit(vtx=None),
           "emit: empty mesh": lambda: emit(nv=0),
           "colour: null vertices": lambda: colour(vtx=None), "colour: trunc 0": lambda: colour(trunc=0.0),
           "colour: no vertices": lambda: colour(n=0), "colour: null maps": lambda: colour(maps=None),
           "colour: null acc": lambda: colour(acc=None)}
    for what, call in bad.items():
        assert call() == -1, what
        assert l.mdf_last_error(), what
        assert l.mdf_last_launch() == last, what
    assert emit(nv=2 ** 31) == -2 and b"int32" in l.mdf_last_error() and l.mdf_last_launch() == last
    assert emit(nt=2 ** 31) == -2 and l.mdf_last_launch() == last
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.tsdf_integrate(dep[None], cams[:, :9].reshape(1, 3, 3), np.eye(4)[None], (0, 0, 0), 1.0, (3, 3), 1.0)


# ---------------------------------------------------------------------------------------------------- 5. driver
def test_mesh_driver_end_to_end(tmp_path):
    from test_tsdf_mesh_cpu import write_scene_on_disk, assert_closed_sphere
    from tools.data_io import read_ply_mesh
    from tools.mesh import main as M
    sc = O.sphere_scene((65, 65, 65))
    root, ev = write_scene_on_disk(tmp_path, "ball", sc, O.scene_images(sc))
    argv = ["-d", "scene", "-r", str(root), "-e", str(ev), "--scans", "ball", "--resolution", "40"]
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mdf-net_amd", "tools", "mesh", "main.py")] + argv
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    xyz, rgb, faces = read_ply_mesh(str(ev / "ball" / "ball_mesh.ply"))
    args = M.build_parser().parse_args(argv)
    got = M.load_scan(args, str(root), "ball", "images", "cams")
    origin, voxel, dims, tau = M.mesh_box(got["points"], args.resolution, args.voxel, args.trunc)
    assert max(dims) == 40
    D, W = O.integrate(got["depths"], got["K"], got["E"], origin, voxel, dims, tau)
    wv, wt = O.marching_tets(D, W, origin, voxel, 1)
    assert len(wt) > 1000 and f"{len(wv)} vertices, {len(wt)} triangles" in r.stdout, r.stdout
    assert_same_bits(xyz, wv, "vertices of ball_mesh.ply")
    np.testing.assert_array_equal(faces, wt)
    np.testing.assert_array_equal(rgb, O.colour(wv, got["depths"], got["images"], got["K"], got["E"], tau))
    assert_closed_sphere(xyz, faces)
    off = np.abs(np.linalg.norm(xyz.astype(np.float64) - np.asarray(O.SPHERE_CENTRE), axis=1) - O.SPHERE_RADIUS) / float(voxel)
    assert off.max() <= 1.0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        raise SystemExit("usage: test_tsdf_mesh_gpu.py child OUT.npz")
