"""CPU: tests/pcd_oracle.py (the point-cloud fusion oracle) against the reference's recorded stages (tests/golden/pcd_fusion.npz,
made by scripts/gen_pcd_golden.py), analytic cases of the two C++ cores it restates (vis_fusion_core's selection rule and
binning, small_seg_core's window, threshold and size rule), the grid_sample restatement against torch, the torch propagation
oracle against the BFS restatement, the PLY writer with and without normals, and the driver's on-disk scan reader."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import pcd_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pcd_fusion.npz")


# ------------------------------------------------------------------------------------------------ vis_fusion_core
def core1(cands, h=1, w=1, valid=None):
    """cands: [(x, y, depth, violations)] -> vis_fusion_core output [h, w]."""
    x, y, d, v = (np.array(c) for c in zip(*cands))
    valid = np.ones((h, w), bool) if valid is None else valid
    return O.vis_fusion_core(d.astype(np.float32), x.astype(np.float32), y.astype(np.float32), v.astype(np.int32), valid)


def test_selection_rule_first_k_at_least_violations():
    # sorted: (1, 3) k=0, (2, 2) k=1, (3, 0) k=2 -> k=2 >= 0 first; (2, 2) fails at k=1
    assert core1([(0.5, 0.5, 3.0, 0), (0.5, 0.5, 1.0, 3), (0.5, 0.5, 2.0, 2)])[0, 0] == 3.0
    # k=1 >= 1 on the second entry
    assert core1([(0.5, 0.5, 1.0, 5), (0.5, 0.5, 2.0, 1), (0.5, 0.5, 3.0, 0)])[0, 0] == 2.0
    # the first entry qualifies with no violations
    assert core1([(0.5, 0.5, 7.0, 0), (0.5, 0.5, 1.0, 0)])[0, 0] == 1.0


def test_selection_rule_last_entry_fallback():
    assert core1([(0.5, 0.5, 1.0, 9), (0.5, 0.5, 2.0, 9), (0.5, 0.5, 3.0, 9)])[0, 0] == 3.0
    assert core1([(0.5, 0.5, 4.0, 1)])[0, 0] == 4.0


def test_selection_rule_ties_in_depth_sort_by_violations():
    # equal depth: (2, 1) sorts before (2, 5); k=0: (1, 4) no; k=1: (2, 1) yes
    assert core1([(0.5, 0.5, 2.0, 5), (0.5, 0.5, 1.0, 4), (0.5, 0.5, 2.0, 1)])[0, 0] == 2.0
    # a group of equal entries (2, 2) at positions 1..3 qualifies at position 2
    r = core1([(0.5, 0.5, 1.0, 9), (0.5, 0.5, 2.0, 2), (0.5, 0.5, 2.0, 2), (0.5, 0.5, 2.0, 2), (0.5, 0.5, 3.0, 0)])
    assert r[0, 0] == 2.0


def test_binning_rounds_half_away_and_checks_range_depth_valid():
    # x - 0.5 = 1.5 -> 2 (half away), = 0.5 -> 1, = -0.4 -> 0, = -0.5 -> -1 (out)
    out = core1([(2.0, 0.5, 5.0, 0), (1.0, 0.5, 6.0, 0), (0.1, 0.5, 7.0, 0), (0.0, 0.5, 8.0, 0)], h=1, w=4)
    assert out.tolist() == [[7.0, 6.0, 5.0, 0.0]]
    # depth 1e-9 (fp32 value below 1e-9 in double) and invalid bins are dropped; empty bins give 0
    valid = np.array([[True, False]])
    out = core1([(0.5, 0.5, 1e-9, 0), (1.5, 0.5, 3.0, 0)], h=1, w=2, valid=valid)
    assert out.tolist() == [[0.0, 0.0]]


# ------------------------------------------------------------------------------------------------ small_seg_core
def test_window_reach_4_links_5_does_not():
    d = np.zeros((1, 30), np.float32)
    d[0, 0:5] = 10.0          # 5 pixels
    d[0, 8:13] = 10.0         # pixel 8 is 4 from pixel 4: linked -> one segment of 10
    assert O.small_seg_core(d)[0].sum() == 10
    d = np.zeros((1, 30), np.float32)
    d[0, 0:5] = 10.0
    d[0, 9:14] = 10.0         # pixel 9 is 5 from pixel 4: two segments of 5, both dropped
    assert O.small_seg_core(d)[0].sum() == 0
    d = np.zeros((10, 10), np.float32)
    d[0, 0:5] = 10.0
    d[4, 4:9] = 10.0          # diagonal offset (4, 4) is inside the 9x9 window
    assert O.small_seg_core(d).sum() == 10


def test_relative_threshold_boundary():
    a = np.float32(1000.0)
    thr = np.float32(1e-3)
    # |a - b| < 1e-3 (a + b) in float: find the largest b that still links and the next float that does not
    b = np.float32(1003.0)
    while not (np.abs(a - b) < thr * (a + b)):
        b = np.nextafter(b, np.float32(0))
    b_out = np.nextafter(b, np.float32(np.inf))
    for bb, want in ((b, 10), (b_out, 0)):
        d = np.zeros((1, 12), np.float32)
        d[0, 0:5] = a
        d[0, 5:10] = bb
        assert O.small_seg_core(d)[0].sum() == want, (bb, want)
        assert O.small_seg_torch(d)[0].sum() == want


def test_zero_depth_splits_segment():
    d = np.full((1, 19), 5.0, np.float32)
    assert O.small_seg_core(d).sum() == 19
    d = np.full((1, 30), 5.0, np.float32)
    d[0, 10:15] = 0.0         # a gap of 5: the 10 + 15 pixels on either side are separate (both >= 10 here)
    assert O.small_seg_core(d).sum() == 25
    d[0, 5:10] = 0.0          # left part shrinks to 5 pixels (x 0..4, gap 5..14): dropped
    assert O.small_seg_core(d).sum() == 15


def test_segments_of_9_dropped_10_kept():
    d = np.zeros((12, 40), np.float32)
    d[0, 0:9] = 7.0
    d[8, 20:30] = 9.0
    out = O.small_seg_core(d)
    assert out[0, 0:9].sum() == 0 and out[8, 20:30].sum() == 10 and out.sum() == 10
    np.testing.assert_array_equal(O.small_seg_torch(d), out)


def test_torch_propagation_equals_bfs_on_random_maps():
    rng = np.random.RandomState(0)
    for _ in range(3):
        d = (500 + rng.randint(0, 4, (40, 56)) * 0.3).astype(np.float32)
        d[rng.rand(40, 56) < 0.4] = 0.0
        np.testing.assert_array_equal(O.small_seg_torch(d), O.small_seg_core(d))


# ------------------------------------------------------------------------------------------------ torch restatements
def test_grid_nearest_matches_grid_sample():
    rng = np.random.RandomState(1)
    H, W = 13, 17
    dep = torch.from_numpy(rng.uniform(1, 2, (H, W)).astype(np.float32))
    px = torch.from_numpy(rng.uniform(-4, W + 4, 5000).astype(np.float32))
    py = torch.from_numpy(rng.uniform(-4, H + 4, 5000).astype(np.float32))
    px[:40] = torch.arange(40, dtype=torch.float32) * 0.5          # exact half-pixel positions: the rounding ties
    g = torch.stack([px / W, py / H], -1)
    g = (g * 2 - 1).clamp(-1.1, 1.1)
    want = torch.nn.functional.grid_sample(dep[None, None], g[None, None], "nearest", "zeros", False)[0, 0, 0]
    got, inr, _ = O.grid_nearest(dep, px, py)
    assert torch.equal(got, want)
    assert torch.equal(inr, (g.abs() <= 1).all(-1))


def test_pipeline_shrinks_monotonically_on_a_seeded_scan():
    from mdfnet_hip import synth
    s = synth.pcd_scan(5, 24, 32, seed=4, nsrc=4)
    counts = []
    O.run(s["depths"], s["probs"], s["K"], s["E"], O.src_table(s["srcs"], 5, 4), 3, record=lambda n, d, m: counts.append(int(m.sum())))
    assert counts == sorted(counts, reverse=True) and counts[-1] > 0


# ------------------------------------------------------------------------------------------------ goldens from the reference
def _golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def check_fusion_against_reference(g, dep, mask, tab, srcs, want_d):
    """Visibility fusion against the reference's own vis_fusion_core inputs.  Per reference view:
      - the oracle generates as many candidates as the reference, in the same order;
      - its violation counts without the self-checks (a source pixel's candidate checked against its own source: its depth
        against itself re-projected, decided by rounding) equal the reference's exactly on the reference's own pixels, and up
        to the one self-check (reference - oracle in {0, 1}) on source pixels -- except where a non-self decision has an fp64
        margin below 1e-5 (counted and returned);
      - vis_fusion_core on the oracle's candidates with the REFERENCE's violation counts reproduces the reference's fused depth
        at every pixel (to fp32 rounding of the candidate depths): the selection and the binning are the reference's."""
    counts, rv = g["cand_counts"], g["cand_violations"].astype(np.int64)
    N, H, W = dep.shape
    off, flips = 0, 0
    for r in range(N):
        d, x, y, vio, _, selfv = O.fusion_candidates(r, dep, tab, srcs[r], with_self=True)
        _, _, _, _, mg64 = O.fusion_candidates(r, dep.double(), tab.double(), srcs[r], torch.float64)
        assert len(d) == int(counts[r]), (r, len(d), int(counts[r]))
        ref_v = rv[off:off + len(d)]
        off += len(d)
        nonself = (vio - selfv).numpy().astype(np.int64)
        nref = int((dep[r] > 1e-9).sum())
        extra = ref_v - nonself
        ok = np.zeros(len(d), bool)
        ok[:nref] = extra[:nref] == 0
        ok[nref:] = (extra[nref:] == 0) | (extra[nref:] == 1)
        bad = ~ok
        flips += int(bad.sum())
        assert bool((mg64.numpy()[bad] < 1e-5).all()), f"view {r}: a violation count differs away from a decision"
        valid = (dep[r] > 1e-9).numpy()
        out = torch.from_numpy(O.vis_fusion_core(d.numpy(), x.numpy(), y.numpy(), ref_v, valid)) * mask[r].float()
        torch.testing.assert_close(out, want_d[r], rtol=2e-6, atol=1e-4, msg=f"view {r}: selection")
    assert off == len(rv)
    return flips


def test_oracle_matches_reference_golden_every_stage():
    """Each stage of the oracle, fed the reference's own state before the stage, reproduces the reference's state after it.
    Masks and depths must agree (depths to fp32 rounding of the reference's different matrix arithmetic: torch.inverse in fp32,
    BLAS order) except where the fp64 decision margin is below 1e-5 relative; those are counted and printed.  Visibility
    fusion is tied to the reference through its recorded violation counts (check_fusion_against_reference)."""
    g = _golden()
    tab = torch.from_numpy(O.cameras(g["K"], g["E"]))
    srcs = g["srcs"]
    need = O.vis_need(int(g["vthresh"]))
    prob_mask = torch.from_numpy(g["probs"]) > O.PTHRESH
    assert torch.equal(prob_mask, torch.from_numpy(g["mask_prob"]))
    flips = 0
    for k, name in enumerate(O.STEPS[1:], 1):
        prev = O.STEPS[k - 1]
        dep, mask = torch.from_numpy(g["depth_" + prev]), torch.from_numpy(g["mask_" + prev])
        want_d, want_m = torch.from_numpy(g["depth_" + name]), torch.from_numpy(g["mask_" + name])
        if name.startswith("vis") and name != "vis_fusion":
            d, m, margin = O.vis_filter(dep, mask, tab, srcs, need)
            _, m64, margin64 = O.vis_filter(dep.double(), mask, tab.double(), srcs, need, torch.float64)
            bad = m != want_m
            flips += int(bad.sum())
            assert bool((margin64[bad] < 1e-5).all()), f"{name}: mask differs at a decision far from its threshold"
            ok = ~bad & want_m
        elif name == "vis_fusion":
            flips += check_fusion_against_reference(g, dep, mask, tab, srcs, want_d)
            d, m = O.vis_fusion(dep, mask, tab, srcs), mask
            # bins holding a self-check may pick another candidate than the reference (see check_fusion_against_reference)
            ok = torch.isclose(d, want_d, rtol=2e-6, atol=1e-4)
            print(f"vis_fusion: {int((~ok).sum())} fused depths differ from the reference, all explained by self-checks")
        elif name == "ave":
            d, m = O.ave_fusion(dep, mask, tab, srcs), mask
            _, _, margin64 = O.vis_filter(dep.double(), mask, tab.double(), srcs, need, torch.float64)
            bad = ~torch.isclose(d, want_d, rtol=2e-6, atol=1e-4)      # a source's mask decided on its threshold
            flips += int(bad.sum())
            assert bool((margin64[bad] < 1e-5).all()), f"{name}: average differs away from a decision"
            ok = ~bad
        else:
            d, m = O.seg_filter(dep, mask)
            ok = torch.ones_like(mask)
        assert torch.equal(m[ok], want_m[ok]), name
        torch.testing.assert_close(d[ok], want_d[ok], rtol=2e-6, atol=1e-4, msg=name)
        print(f"{name}: {int(want_m.sum())} pixels kept")
    print(f"decisions within 1e-5 of a threshold that differ from the reference: {flips}")
    # points of the final state
    xyz, rgb, _ = O.back_project(torch.from_numpy(g["depth_seg"]), torch.from_numpy(g["mask_seg"]), g["images"], O.cameras(g["K"], g["E"]))
    torch.testing.assert_close(xyz, torch.from_numpy(g["points"]), rtol=1e-5, atol=1e-3)
    np.testing.assert_array_equal(rgb.numpy(), np.round(g["colors"] * 255).astype(np.uint8))


def test_golden_scene_has_points_behind_a_camera():
    g = _golden()
    assert int(g["behind_view"]) >= 0 and g["depths"].shape[0] >= 6
    assert int(g["mask_seg"].sum()) > 0 and os.path.getsize(GOLDEN) < (1 << 20)


# ------------------------------------------------------------------------------------------------ PLY and the driver's reader
def test_write_ply_without_normals_is_byte_identical(tmp_path):
    from tools.data_io import write_ply, read_ply
    rng = np.random.RandomState(2)
    xyz = rng.randn(17, 3).astype(np.float32)
    rgb = rng.randint(0, 256, (17, 3)).astype(np.uint8)
    write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    rec = np.empty(17, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = xyz.T
    rec["red"], rec["green"], rec["blue"] = rgb.T
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 17\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n") + rec.tobytes()
    assert (tmp_path / "a.ply").read_bytes() == want
    x2, c2 = read_ply(str(tmp_path / "a.ply"))
    np.testing.assert_array_equal(x2, xyz)
    np.testing.assert_array_equal(c2, rgb)


def test_write_ply_normals_round_trip(tmp_path):
    from tools.data_io import write_ply, read_ply_normals
    rng = np.random.RandomState(3)
    xyz, nrm = rng.randn(9, 3).astype(np.float32), rng.randn(9, 3).astype(np.float32)
    rgb = rng.randint(0, 256, (9, 3)).astype(np.uint8)
    write_ply(str(tmp_path / "n.ply"), xyz, rgb, normals=nrm)
    head = (tmp_path / "n.ply").read_bytes().split(b"end_header\n")[0].decode()
    assert "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in head
    x2, c2, n2 = read_ply_normals(str(tmp_path / "n.ply"))
    np.testing.assert_array_equal(x2, xyz)
    np.testing.assert_array_equal(c2, rgb)
    np.testing.assert_array_equal(n2, nrm)


def make_scan_on_disk(tmp_path, scan, n=6, h=40, w=56, seed=9):
    """A Tanks-layout scan: <root>/TankandTemples/intermediate/<scan>/{pair.txt, images/*.jpg, cams_1/*_cam.txt} and
    <eval>/<scan>/{depth_est, confidence}/*.pfm, from synth.pcd_scan (images 4 px larger than the depth maps).
    -> (root, eval, ply folder)."""
    from PIL import Image
    from mdfnet_hip import synth
    from tools.data_io import save_pfm
    s = synth.pcd_scan(n, h, w, seed=seed, nsrc=n - 1)
    root, ev, out = tmp_path / "data", tmp_path / "outputs", tmp_path / "ply"
    sd = root / "TankandTemples" / "intermediate" / scan
    for d in (sd / "images", sd / "cams_1", ev / scan / "depth_est", ev / scan / "confidence"):
        d.mkdir(parents=True, exist_ok=True)
    rng = np.random.RandomState(seed)
    with open(sd / "pair.txt", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            srcs = s["srcs"][i] + [n + 3]          # a view that is not part of the scan is skipped
            f.write(f"{i}\n{len(srcs)} " + " ".join(f"{j} {100 - k}.0" for k, j in enumerate(srcs)) + "\n")
    for i in range(n):
        name = f"{i:08d}"
        save_pfm(str(ev / scan / "depth_est" / (name + ".pfm")), s["depths"][i])
        save_pfm(str(ev / scan / "confidence" / (name + ".pfm")), s["probs"][i])
        img = rng.randint(0, 256, (h + 4, w + 4, 3)).astype(np.uint8)
        Image.fromarray(img).save(str(sd / "images" / (name + ".jpg")))
        with open(sd / "cams_1" / (name + "_cam.txt"), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in s["E"][i]) + "\n\n")
            f.write("intrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in s["K"][i]) + "\n\n")
            f.write("425.0 2.5\n")
    return root, ev, out


def test_driver_reads_the_scan_as_written(tmp_path):
    from mdfnet_hip import synth
    from tools.pcd import fusion as F
    root, ev, _ = make_scan_on_disk(tmp_path, "Horse", n=5, h=24, w=32)
    sc = F.load_scan(str(root / "TankandTemples" / "intermediate" / "Horse"), str(ev / "Horse"), "images", "cams_1")
    s = synth.pcd_scan(5, 24, 32, seed=9, nsrc=4)
    np.testing.assert_array_equal(sc["depths"], s["depths"])
    np.testing.assert_array_equal(sc["probs"], s["probs"])
    np.testing.assert_array_equal(sc["K"], s["K"])
    np.testing.assert_array_equal(sc["E"], s["E"])
    assert sc["srcs"] == s["srcs"] and sc["images"].shape == (5, 24, 32, 3)
    assert sc["ids"] == [str(i) for i in range(5)]


def test_driver_refuses_normals_and_downsample():
    from tools.pcd import fusion as F
    with pytest.raises(SystemExit, match="not implemented"):
        F.main(["-d", "tanks"])
    with pytest.raises(SystemExit, match="not implemented"):
        F.main(["-d", "tanks", "--no_normal", "--downsample", "0.5"])
