"""GPU: mdf_pcd_fuse_fwd / mdf_pcd_compact (ops.pcd_fuse) against tests/pcd_oracle.py, step by step on seeded scenes (one with a
source that sees points behind its camera), a bin of more than 1000 candidates, the small-segment filter on a full-size map,
a full-size scan twice, the tools/pcd driver end to end and the ABI's error paths.

Bar: bit-identical.  The kernels and the fp32 oracle execute the same correctly rounded operations in the same order (no fma,
IEEE divides, the square root through float64), so any difference is a change of arithmetic, not noise."""
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

import pcd_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def filter_based_scene(n, h, w, seed, behind):
    """oracle.gen_golden.filter_scene with probabilities and images; with `behind`, the last camera is turned by 180 degrees about
    its y axis, so every point of the scene lies behind it."""
    from oracle.gen_golden import filter_scene
    depths, _, K, E = filter_scene(h=h, w=w, nsrc=n - 1, seed=seed)
    rng = np.random.RandomState(seed + 50)
    E = E.copy()
    if behind:
        E[-1, :3, :] = np.diag([-1.0, 1.0, -1.0]).astype(np.float32) @ E[-1, :3, :]
    srcs = [sorted((j for j in range(n) if j != i), key=lambda j: (abs(i - j), j)) for i in range(n)]
    return {"depths": depths, "probs": rng.uniform(0.6, 1.0, depths.shape).astype(np.float32),
            "images": rng.randint(0, 256, depths.shape + (3,)).astype(np.uint8), "K": K, "E": E, "srcs": srcs}


def scenes():
    from mdfnet_hip import synth
    return {"plane8": (synth.pcd_scan(8, 48, 64, seed=1, nsrc=10), 10, 4),
            "plane5": (synth.pcd_scan(5, 37, 53, seed=2, nsrc=3), 3, 3),
            "behind": (filter_based_scene(7, 40, 56, seed=3, behind=True), 6, 3)}


def gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def kernel_step(dep, mask, s, view, vthresh, step):
    from mdfnet_hip import ops
    n = dep.shape[0]
    d = gpu(dep.float().numpy())
    m = gpu(mask.numpy().astype(np.uint8))
    cams = gpu(ops.pcd_cameras(s["K"], s["E"]))
    srcs = gpu(ops.pcd_sources(s["srcs"], n, view))
    _, counts, total = ops.pcd_steps(d, m, cams, srcs, O.vis_need(vthresh), step, step)
    torch.cuda.synchronize()
    return d.cpu(), m.cpu().bool(), counts.cpu(), total


@pytest.mark.parametrize("name", ["plane8", "plane5", "behind"])
def test_each_step_matches_oracle(name):
    s, view, vthresh = scenes()[name]
    n = s["depths"].shape[0]
    states = []
    O.run(s["depths"], s["probs"], s["K"], s["E"], O.src_table(s["srcs"], n, view), vthresh,
          record=lambda nm, d, m: states.append((nm, d.clone(), m.clone())))
    for k in range(1, len(O.STEPS)):
        nm, want_d, want_m = states[k]
        _, prev_d, prev_m = states[k - 1]
        d, m, counts, total = kernel_step(prev_d, prev_m, s, view, vthresh, k)
        assert torch.equal(m, want_m), f"{name} step {nm}: {int((m != want_m).sum())} mask pixels differ"
        bad = (d.view(torch.int32) != want_d.view(torch.int32))
        assert not bool(bad.any()), f"{name} step {nm}: {int(bad.sum())} depths differ, max {float((d - want_d).abs().max())}"
        assert counts.tolist() == want_m.reshape(n, -1).sum(1).tolist() and total == int(want_m.sum())
        print(f"{name} step {nm}: {int(want_m.sum())} pixels kept, bit-identical")
    assert int(states[-1][2].sum()) > 0


@pytest.mark.parametrize("name", ["plane8", "behind"])
def test_whole_pipeline_points_match_oracle(name):
    from mdfnet_hip import ops
    s, view, vthresh = scenes()[name]
    n = s["depths"].shape[0]
    out = ops.pcd_fuse(gpu(s["depths"]), gpu(s["probs"]), gpu(s["images"]), s["K"], s["E"], s["srcs"], view=view, vthresh=vthresh)
    torch.cuda.synchronize()
    dep, mask = O.run(s["depths"], s["probs"], s["K"], s["E"], O.src_table(s["srcs"], n, view), vthresh)
    xyz, rgb, dirs = O.back_project(dep, mask, s["images"], O.cameras(s["K"], s["E"]))
    assert torch.equal(out["masks"].cpu(), mask)
    assert torch.equal(out["depths"].cpu(), dep)
    assert out["xyz"].shape[0] == xyz.shape[0] > 0
    assert torch.equal(out["xyz"].cpu(), xyz) and torch.equal(out["dirs"].cpu(), dirs) and torch.equal(out["rgb"].cpu(), rgb)
    # the stage switch returns the state after the chosen step
    part = ops.pcd_fuse(gpu(s["depths"]), gpu(s["probs"]), gpu(s["images"]), s["K"], s["E"], s["srcs"], view=view,
                        vthresh=vthresh, stages=3)
    states = []
    O.run(s["depths"], s["probs"], s["K"], s["E"], O.src_table(s["srcs"], n, view), vthresh, stop=3,
          record=lambda nm, d, m: states.append((d, m)))
    assert torch.equal(part["depths"].cpu(), states[-1][0]) and torch.equal(part["masks"].cpu(), states[-1][1])
    assert "xyz" not in part


def large_bin_scene(h=40, w=48):
    """Reference camera 0 at the origin looking down +z at a wall 600 away; source camera 1 sits 500 in front of it on the same
    axis and sees its pixels at depth 0.01, i.e. within 0.01 of its centre: all h*w of them land in the reference pixel the
    source centre projects to (the principal point), a bin of h*w + 1 candidates."""
    f = 50.0
    K = np.array([[[f, 0, w / 2.0 + 0.5], [0, f, h / 2.0 + 0.5], [0, 0, 1]]] * 2, dtype=np.float32)
    E = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    E[1, 2, 3] = -500.0
    depths = np.stack([np.full((h, w), 600.0), np.full((h, w), 0.01)]).astype(np.float32)
    rng = np.random.RandomState(5)
    depths[1] *= rng.uniform(0.5, 1.5, (h, w)).astype(np.float32)
    return depths, K, E, [[1], [0]]


def test_bin_of_more_than_1000_candidates():
    depths, K, E, srcs = large_bin_scene()
    s = {"K": K, "E": E, "srcs": srcs}
    n, h, w = depths.shape
    tab = torch.from_numpy(O.cameras(K, E))
    dep = torch.from_numpy(depths)
    d, x, y, vio, _ = O.fusion_candidates(0, dep, tab, [1])
    bins = np.round(x.double().numpy() - 0.5).astype(np.int64) + w * np.round(y.double().numpy() - 0.5).astype(np.int64)
    big = int(np.bincount(bins[(bins >= 0) & (bins < h * w)]).max())
    assert big >= 1000, big
    mask = torch.ones(depths.shape, dtype=torch.bool)
    want = O.vis_fusion(dep, mask, tab, np.array([[1], [0]]))
    got, _, _, _ = kernel_step(dep, mask, s, 1, 2, 2)
    assert torch.equal(got, want)
    print(f"largest bin: {big} candidates, bit-identical")


def seg_map(h, w, seed):
    """Piecewise-smooth depth: random rectangles of slanted planes, small speckle islands (3x3 .. 1x1), zero holes."""
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = (500.0 + 0.05 * xs + 0.02 * ys).astype(np.float64)
    for _ in range(60):
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        hh, ww = rng.randint(1, 200), rng.randint(1, 300)
        d[y0:y0 + hh, x0:x0 + ww] = rng.uniform(300, 900) + rng.uniform(-0.1, 0.1) * xs[y0:y0 + hh, x0:x0 + ww]
    for _ in range(4000):
        y0, x0, k = rng.randint(0, h), rng.randint(0, w), rng.randint(1, 4)
        d[y0:y0 + k, x0:x0 + k] = rng.uniform(300, 900)
    d[rng.rand(h, w) < 0.05] = 0.0
    d *= 1 + 3e-4 * rng.standard_normal((h, w))
    return d.astype(np.float32)


def test_small_segments_full_size_map():
    h, w = 1056, 1920
    dep = torch.from_numpy(seg_map(h, w, 11))[None]
    mask = torch.ones_like(dep, dtype=torch.bool)
    want = torch.from_numpy(O.small_seg_torch(dep[0].numpy()).astype(bool))[None]
    d, m, _, _ = kernel_step(dep, mask, {"K": np.eye(3)[None], "E": np.eye(4)[None], "srcs": [[]]}, 0, 4, 6)
    assert torch.equal(m, want), int((m != want).sum())
    assert torch.equal(d, dep * want.float())
    print(f"1056x1920: {int(want.sum())} of {int((dep > 0).sum())} valid pixels in segments of >= 10")


def test_full_size_scan_runs_and_repeats():
    """64 views at 1056 x 1920 with 10 sources (a Tanks-size scan): two calls give identical outputs."""
    from mdfnet_hip import ops, synth
    s = synth.pcd_scan(64, 1056, 1920, seed=21, nsrc=10)
    args = (gpu(s["depths"]), gpu(s["probs"]), gpu(s["images"]), s["K"], s["E"], s["srcs"])
    a = ops.pcd_fuse(*args)
    b = ops.pcd_fuse(*args)
    torch.cuda.synchronize()
    for k in ("depths", "masks", "counts", "xyz", "rgb", "dirs"):
        assert torch.equal(a[k], b[k]), k
    kept = int(a["counts"].sum())
    print(f"64x1056x1920: {kept} points ({kept / (64 * 1056 * 1920):.3f} of the pixels)")
    assert kept > 0.3 * 64 * 1056 * 1920


def test_driver_end_to_end(tmp_path):
    from mdfnet_hip import ops
    from test_pcd_fusion_cpu import make_scan_on_disk
    from tools.data_io import read_ply
    from tools.pcd import fusion as F
    root, ev, out = make_scan_on_disk(tmp_path, "Horse", n=6, h=40, w=56)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mdf-net_amd", "tools", "pcd", "fusion.py"),
           "-r", str(root), "-e", str(ev), "-o", str(out), "-d", "tanks", "-s", "intermediate", "--scans", "Horse",
           "--view", "4", "--vthresh", "3", "--no_normal", "--write_mask"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    xyz, rgb = read_ply(str(out / "Horse.ply"))
    sc = F.load_scan(os.path.join(str(root), "TankandTemples", "intermediate", "Horse"), os.path.join(str(ev), "Horse"),
                     "images", "cams_1")
    want = ops.pcd_fuse(gpu(sc["depths"]), gpu(sc["probs"]), gpu(sc["images"]), sc["K"], sc["E"], sc["srcs"], view=4, vthresh=3)
    assert len(xyz) == want["xyz"].shape[0] > 0
    np.testing.assert_array_equal(xyz, want["xyz"].cpu().numpy())
    np.testing.assert_array_equal(rgb, want["rgb"].cpu().numpy())
    from PIL import Image
    m0 = np.asarray(Image.open(os.path.join(str(ev), "Horse", "filter", "00000000_mask.png")))
    np.testing.assert_array_equal(m0 > 0, want["masks"][0].cpu().numpy())


def test_abi_error_paths():
    import mdfnet_hip
    l = mdfnet_hip.lib()
    n, h, w, v = 2, 8, 8, 1
    d = torch.zeros((n, h, w), device=DEV)
    m = torch.zeros((n, h, w), device=DEV, dtype=torch.uint8)
    cams = torch.zeros((n, 64), device=DEV)
    srcs = torch.tensor([[1], [0]], device=DEV, dtype=torch.int32)
    ws = torch.empty(int(l.mdf_pcd_fuse_workspace(n, h, w, v)), device=DEV, dtype=torch.uint8)
    cnt = torch.empty(n, device=DEV, dtype=torch.int32)
    tot = torch.empty(1, device=DEV, dtype=torch.int64)
    P = lambda t: t.data_ptr()

    def call(n=n, v=v, depths=P(d), workspace=P(ws), h=h, first=1, last=6):
        return l.mdf_pcd_fuse_fwd(depths, P(m), P(cams), P(srcs), n, h, w, v, 3, first, last, workspace, P(cnt), P(tot), None)
    assert call(n=0) == -1 and b"out of range" in l.mdf_last_error()
    assert call(n=1025) == -1 and b"out of range" in l.mdf_last_error()
    assert call(v=65) == -1 and b"out of range" in l.mdf_last_error()
    assert call(depths=None) == -1 and b"null" in l.mdf_last_error()
    assert call(workspace=None) == -1 and b"null" in l.mdf_last_error()
    assert call(h=0) == -1 and b"shape" in l.mdf_last_error()
    assert call(first=0) == -1 and b"steps" in l.mdf_last_error()
    assert call(last=7) == -1 and b"steps" in l.mdf_last_error()
    assert l.mdf_pcd_compact(P(d), P(m), None, P(cams), n, h, w, v, P(ws), None, None, None, 0, None) == -1
    assert l.mdf_pcd_fuse_workspace(0, h, w, v) == 0
    assert call() == 0                                           # the same buffers with valid arguments run
    torch.cuda.synchronize()
    assert tot.item() == 0 and cnt.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mdfnet_hip.ops.pcd_fuse(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, 3, dtype=torch.uint8),
                                np.zeros((2, 3, 3)), np.zeros((2, 4, 4)), [[1], [0]])


def seg_kernel(d):
    """The small-segment step of the kernel on one map (all-true mask) -> uint8 [h, w]."""
    dep = torch.from_numpy(np.asarray(d, np.float32))[None]
    _, m, _, _ = kernel_step(dep, torch.ones_like(dep, dtype=torch.bool), {"K": np.eye(3)[None], "E": np.eye(4)[None], "srcs": [[]]},
                             0, 4, 6)
    return m[0].numpy().astype(np.uint8)


def test_small_segment_kernel_analytic_cases():
    """The CPU suite's analytic cases of small_seg_core, through the kernel: window reach 4 links and 5 does not, the relative
    threshold at its last linking float, zero depth splitting a segment, segments of 9 dropped and 10 kept."""
    d = np.zeros((1, 30), np.float32)
    d[0, 0:5] = 10.0
    d[0, 8:13] = 10.0
    assert seg_kernel(d).sum() == 10
    d[0, 8:13] = 0.0
    d[0, 9:14] = 10.0
    assert seg_kernel(d).sum() == 0
    a, thr, b = np.float32(1000.0), np.float32(1e-3), np.float32(1003.0)
    while not (np.abs(a - b) < thr * (a + b)):
        b = np.nextafter(b, np.float32(0))
    for bb, want in ((b, 10), (np.nextafter(b, np.float32(np.inf)), 0)):
        d = np.zeros((1, 12), np.float32)
        d[0, 0:5], d[0, 5:10] = a, bb
        assert seg_kernel(d).sum() == want
    d = np.full((1, 30), 5.0, np.float32)
    d[0, 10:15] = 0.0
    assert seg_kernel(d).sum() == 25
    d[0, 5:10] = 0.0
    assert seg_kernel(d).sum() == 15
    d = np.zeros((12, 40), np.float32)
    d[0, 0:9], d[8, 20:30] = 7.0, 9.0
    out = seg_kernel(d)
    assert out[0, 0:9].sum() == 0 and out[8, 20:30].sum() == 10 and out.sum() == 10
    rng = np.random.RandomState(0)
    for _ in range(3):
        d = (500 + rng.randint(0, 4, (40, 56)) * 0.3).astype(np.float32)
        d[rng.rand(40, 56) < 0.4] = 0.0
        np.testing.assert_array_equal(seg_kernel(d), O.small_seg_core(d))


def test_source_index_past_the_scan_is_ignored():
    """A direct ABI caller's source index >= n is treated as none (-1), never read."""
    from mdfnet_hip import ops
    s, view, vthresh = scenes()["plane5"]
    n = s["depths"].shape[0]
    states = []
    O.run(s["depths"], s["probs"], s["K"], s["E"], O.src_table(s["srcs"], n, view), vthresh, stop=2,
          record=lambda nm, d, m: states.append((d, m)))
    dep, mask = states[0]
    cams = gpu(ops.pcd_cameras(s["K"], s["E"]))
    for step in (1, 2, 4):
        outs = []
        for bad in (-1, n + 1000):
            t = ops.pcd_sources(s["srcs"], n, view)
            t[:, -1] = bad
            d, m = gpu(dep.numpy()), gpu(mask.numpy().astype(np.uint8))
            ops.pcd_steps(d, m, cams, gpu(t), O.vis_need(vthresh), step, step)
            outs.append((d.cpu(), m.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), step
