"""GPU: mdf_consensus_fuse_fwd / mdf_consensus_compact (ops.consensus_fuse) against tests/consensus_oracle.py on seeded scenes and
on the analytic wrap / zero-depth cases, its float64 decision margins, one DTU-size scan, the gipuma driver end to end, and the
ABI's error paths.

Bar for xyz and rgb: bit-identical.  The kernel and the fp32 oracle execute the same correctly rounded operations in the same
order (no fma, IEEE divides, the square root through float64), so any difference is a change of arithmetic, not noise."""
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

import consensus_oracle as CO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def seeded_scene(n, h, w, seed, isolated=False):
    from oracle.gen_golden import filter_scene
    depths, _, K, E = filter_scene(h=h, w=w, nsrc=n - 1, seed=seed)
    rng = np.random.RandomState(seed + 100)
    depths = depths.copy()
    depths[rng.rand(*depths.shape) < 0.1] = 0.0                # what the probability filter leaves behind
    images = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    if isolated:                                                # views far apart along x: no view sees another's surface
        E = E.copy()
        E[:, 0, 3] += 5.0e4 * np.arange(n, dtype=np.float32)
    return depths, images, K, E


def run_kernel(depths, images, K, E, thr, k):
    xyz, rgb, counts = __import__("mdfnet_hip.ops", fromlist=["ops"]).consensus_fuse(
        torch.from_numpy(depths).to(DEV), torch.from_numpy(images).to(DEV), K, E, thr, k)
    torch.cuda.synchronize()
    return xyz.cpu(), rgb.cpu(), counts.cpu().tolist()


def assert_matches_oracle(depths, images, K, E, thr, k, ref_views=None):
    xyz, rgb, counts = run_kernel(depths, images, K, E, thr, k)
    oxyz, orgb, ocounts, per = CO.fuse(depths, images, K, E, thr, k, torch.float32, ref_views=ref_views)
    if ref_views is not None:          # the kernel fused every view: cut its output down to the listed ones
        starts = np.concatenate([[0], np.cumsum(counts)])
        sel = torch.cat([torch.arange(starts[r], starts[r + 1]) for r in ref_views])
        xyz, rgb, counts = xyz[sel], rgb[sel], [counts[r] for r in ref_views]
    assert counts == ocounts
    assert xyz.shape == oxyz.shape and rgb.shape == orgb.shape
    assert torch.equal(xyz, oxyz), float((xyz - oxyz).abs().max())
    assert torch.equal(rgb, orgb)
    return per, sum(counts)


@pytest.mark.parametrize("n,h,w,seed,isolated", [(3, 37, 53, 1, False), (11, 61, 83, 2, False), (49, 33, 45, 3, False),
                                                  (5, 29, 31, 4, True)])
def test_kernel_matches_oracle(n, h, w, seed, isolated):
    depths, images, K, E = seeded_scene(n, h, w, seed, isolated)
    thr, k = 0.25, (0 if isolated else 2)
    per, m = assert_matches_oracle(depths, images, K, E, thr, k)
    print(f"N={n} {w}x{h}: {m} points, bit-identical")
    assert m > 0
    if isolated:                       # nothing agrees: every kept point is the reference's own, n = 0 everywhere
        assert all(int(p["n"].max()) == 0 for p in per.values())
    else:
        assert max(int(p["n"].max()) for p in per.values()) >= 2
    # float64 yardstick: decisions may differ only where the float64 margin is below 1e-4
    flips = 0
    for r in per:
        p64 = CO.fuse_view(r, depths, images, *CO.cameras(K, E), thr, k, torch.float64)
        bad = per[r]["keep"] != p64["keep"]
        flips += int(bad.sum())
        assert bool((p64["margin"][bad] < 1e-4).all())
    print(f"N={n}: {flips} keep decisions differ from float64 (all within 1e-4 of a threshold)")


def test_dtu_size_scan_subsampled():
    """49 x 1184 x 1600 (a DTU scan at eval resolution): the kernel fuses the whole scan; three reference views are checked."""
    from oracle.gen_golden import filter_scene
    depths, _, K, E = filter_scene(h=1184, w=1600, nsrc=48, seed=7)
    rng = np.random.RandomState(7)
    images = rng.randint(0, 256, depths.shape + (3,)).astype(np.uint8)
    depths = depths.copy()
    depths[rng.rand(*depths.shape) < 0.05] = 0.0
    _, m = assert_matches_oracle(depths, images, K, E, 0.25, 3, ref_views=[0, 24, 48])
    print(f"DTU size: {m} points in views 0, 24, 48, bit-identical")
    assert m > 0


def test_kernel_wraps_last_column_to_column_zero():
    """The analytic two-camera scene of the CPU test through the kernel: reference pixel (0, y) lands at pt.x = 7.25 in view 1,
    whose +1 neighbour is column 0: d^ = 0.75 * 100 + 0.25 * 104 = 101, so the fused z is 100.5 (clamping would give 100)."""
    from test_consensus_fuse_cpu import wrap_scene
    depths, images, K, E = wrap_scene()
    xyz, rgb, counts = run_kernel(depths, images, K, E, 0.25, 1)
    # view 0: rows 1..3 of column 0 (row 0 sits at world y = 0 and is dropped); view 1: its pixels project past view 0's left edge
    assert counts == [3, 0]
    assert xyz[:, 2].tolist() == [100.5] * 3
    assert rgb[0].tolist() == [int((10 + 75 + 50) / 2), int((20 + 75) / 2), int((30 + 75 + 10) / 2)]
    assert_matches_oracle(depths, images, K, E, 0.25, 1)


def test_kernel_zero_depth_pixels():
    """d = 0 is not special: the pixel lifts to its camera centre, which no view confirms; with num_consistent 0 the centre is
    emitted, at the origin (camera 0 of the wrap scene) it is dropped by the zero-coordinate rule."""
    from test_consensus_fuse_cpu import scene, wrap_scene
    depths, images, K, E = scene()
    depths = depths.copy()
    depths[2, 5:9, 7:20] = 0.0
    assert_matches_oracle(depths, images, K, E, 0.25, 0)
    d2, im2, K2, E2 = wrap_scene()
    d2[0] = 0.0
    _, _, counts = run_kernel(d2, im2, K2, E2, 0.25, 0)
    assert counts[0] == 0
    assert_matches_oracle(d2, im2, K2, E2, 0.25, 0)


def test_driver_end_to_end(tmp_path):
    from test_consensus_fuse_cpu import make_tiny_scan
    from tools.data_io import read_ply
    from tools.gipuma import main as G
    s = make_tiny_scan(tmp_path, n=4, h=40, w=56, img_h=44, img_w=60)
    out = tmp_path / "ply"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mdf-net_amd", "tools", "gipuma", "main.py"), "-f", "-m",
           "-d", "--scans", "7", "-e", s["eval"], "-r", s["root"], "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "not needed" in r.stdout
    xyz, rgb = read_ply(str(out / "ours007_l3.ply"))
    views, depths, images, K, E = G.load_scan(s["data"], s["ev"], 49, 0.6)
    exyz, ergb, counts = run_kernel(depths, images, K, E, 0.25, 3)
    assert len(xyz) == len(exyz) == sum(counts)
    np.testing.assert_array_equal(xyz, exyz.numpy())
    np.testing.assert_array_equal(rgb, ergb.numpy())


def test_abi_error_paths():
    import mdfnet_hip
    l = mdfnet_hip.lib()
    d = torch.zeros((2, 8, 8), device=DEV)
    c = torch.zeros((2, 8, 8, 4), device=DEV, dtype=torch.uint8)
    cams = torch.zeros((2, 32), device=DEV)
    ws = torch.empty(int(l.mdf_consensus_fuse_workspace(2, 8, 8)), device=DEV, dtype=torch.uint8)
    xyz = torch.empty((128, 3), device=DEV)
    rgb = torch.empty((128, 3), device=DEV, dtype=torch.uint8)
    cnt = torch.empty(2, device=DEV, dtype=torch.int32)
    tot = torch.empty(1, device=DEV, dtype=torch.int64)
    P = lambda t: t.data_ptr()

    def call(n, depths=P(d), h=8, w=8, workspace=P(ws)):
        return l.mdf_consensus_fuse_fwd(depths, P(c), P(cams), n, h, w, ctypes.c_float(1.0), ctypes.c_float(0.25), 3, workspace,
                                        P(xyz), P(rgb), 128, P(cnt), P(tot), None)
    assert call(1) == -1 and b"out of range" in l.mdf_last_error()
    assert call(1025) == -1 and b"out of range" in l.mdf_last_error()
    assert call(2, depths=None) == -1 and b"null" in l.mdf_last_error()
    assert call(2, workspace=None) == -1 and b"null" in l.mdf_last_error()
    assert call(2, h=0) == -1 and b"shape" in l.mdf_last_error()
    assert call(2) == 0                                           # the same buffers with valid arguments run
    torch.cuda.synchronize()
    assert tot.item() == 0 and cnt.tolist() == [0, 0]             # all-zero cameras: every point is exactly 0 and dropped
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mdfnet_hip.ops.consensus_fuse(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, 3, dtype=torch.uint8), np.zeros((2, 3, 3)),
                                      np.zeros((2, 4, 4)), 0.25, 3)
