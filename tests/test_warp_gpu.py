"""GPU parity: fused warp / aggregation kernels (through the C ABI) vs the oracle and the reference goldens.
Bar: corner indices and warped values bit-exact; aggregated cost within a stated fp tolerance."""
import numpy as np
import pytest
import torch

from mdfnet_hip import ops, synth
from oracle import mvs_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"


def _scene_ops():
    return synth.make_scene(96, 64, 3, batch=2, rot_deg=4.0, seed=5)


def sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


@pytest.mark.parametrize("stage,case,view", [(0, "warp0", 0), (1, "warp1", 1)])
def test_corner_indices_bit_exact(golden, stage, case, view):
    g = golden("ops.npz")
    _, extr, intr, _ = _scene_ops()
    rp, sps = O.scale_cam(intr, extr, stage)
    hyp = T(g[case + "_hyp"])
    h, w = g[case + "_src"].shape[-2:]
    proj = ops.relative_projections(rp, sps)
    assert torch.equal(proj[view].reshape(-1, 3, 4), O.relative_projection(sps[view], rp)[:, :3, :4])
    ix, iy = O.warp_positions(O.relative_projection(sps[view], rp), hyp, h, w)
    x0, y0, _, _ = O.warp_corners(ix.expand(2, hyp.shape[1], h * w), iy.expand(2, hyp.shape[1], h * w), h, w)
    got = ops.warp_corner_indices(proj[view].to(DEV), hyp.to(DEV), h, w).cpu()
    exp = torch.stack([x0, y0], -1).reshape(got.shape)
    nbad = int((got != exp).sum())
    assert nbad == 0, f"{nbad} corner-index mismatches of {exp.numel()}"


@pytest.mark.parametrize("stage,case,view", [(0, "warp0", 0), (1, "warp1", 1)])
def test_homo_warp_bit_exact_vs_reference_golden(golden, stage, case, view):
    g = golden("ops.npz")
    _, extr, intr, _ = _scene_ops()
    rp, sps = O.scale_cam(intr, extr, stage)
    proj = ops.relative_projections(rp, sps)
    out = ops.homo_warp(T(g[case + "_src"]).to(DEV), proj[view].to(DEV), T(g[case + "_hyp"]).to(DEV)).cpu().numpy()
    assert np.array_equal(out, g[case + "_out"])


def test_homo_warp_degenerate_planes(golden):
    """H4: z<0 plane -> finite mirrored samples (bit-exact); z==0 -> NaN like grid_sample, not zero."""
    g = golden("ops.npz")
    _, extr, intr, _ = _scene_ops()
    rp, sps = O.scale_cam(intr, extr, 0)
    proj = ops.relative_projections(rp, sps)
    src = T(g["warp0_src"]).to(DEV)
    out = ops.homo_warp(src, proj[0].to(DEV), T(g["warpneg_hyp"]).to(DEV)).cpu().numpy()
    assert np.array_equal(out, g["warpneg_out"], equal_nan=True)
    pz = ops.relative_projections(rp, [T(g["warpz0_srcproj"])])
    out = ops.homo_warp(src, pz[0].to(DEV), T(g["warp0_hyp"])[:, :3].to(DEV)).cpu().numpy()
    assert np.isnan(out).all() and np.isnan(g["warpz0_out"]).all()


@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("channels_last", [True, False])
def test_vector_aggregate_vs_reference_golden(golden, seeded_sd, stage, channels_last):
    g = golden("ops.npz")
    _, extr, intr, _ = _scene_ops()
    rp, sps = O.scale_cam(intr, extr, stage)
    proj = ops.relative_projections(rp, sps).to(DEV)
    feas = [f.to(DEV) for f in T(g[f"agg{stage}_feas"])]
    G = synth.NGROUPS[stage]
    wpar = ops.fold_view_weight(sub(seeded_sd, f"Homoaggre.{stage}."), G).to(DEV)
    cost = ops.warp_aggregate_vec(feas, proj, T(g[f"agg{stage}_hyp"]).to(DEV), wpar, G, channels_last)
    assert cost.shape == g[f"agg{stage}_cost"].shape
    # tolerance: cost is a weighted mean of similarities in [0,1]; fp32 exp/rcp/sum-order differences only
    np.testing.assert_allclose(cost.cpu().numpy(), g[f"agg{stage}_cost"], rtol=0, atol=2e-6)


def test_variance_aggregate_vs_reference_golden(golden):
    g = golden("ops.npz")
    _, extr, intr, dr = _scene_ops()
    rp, sps = O.scale_cam(intr, extr, 0)
    hyp0 = O.uniform_hypos(dr, 48)[:, ::4]
    v0 = ops.warp_aggregate_var([f.to(DEV) for f in T(g["agg0_feas"])], ops.relative_projections(rp, sps).to(DEV),
                                hyp0.to(DEV))
    np.testing.assert_allclose(v0.cpu().numpy(), g["var0_cost"], rtol=0, atol=2e-6)
    rp2, sps2 = O.scale_cam(intr, extr, 2)
    v2 = ops.warp_aggregate_var([f.to(DEV) for f in T(g["agg2_feas"])], ops.relative_projections(rp2, sps2).to(DEV),
                                T(g["agg2_hyp"])[:, ::2].to(DEV), channels_last=True)
    np.testing.assert_allclose(v2.cpu().numpy(), g["var2_cost"], rtol=0, atol=2e-6)


def test_ragged_and_edge_shapes(seeded_sd):
    """Pixel counts that are not multiples of the block tile, 1 and 10 source views, D=1; and both forms of the tap-table fill of
    every kernel these shapes select: 3 source views at 16 channels (the generic fill of the 4-channel kernel: 64 x 3 pairs do not
    divide the block), 8 at 32 channels (two pairs per thread in the 8-channel kernel), on a 5 x 7 map ragged against every tile."""
    for (h, w, c, nsrc, d, seed) in [(7, 9, 64, 1, 1, 1), (13, 11, 32, 10, 3, 2), (5, 31, 16, 2, 5, 3), (5, 7, 16, 3, 5, 4),
                                     (5, 7, 32, 8, 5, 5)]:
        rng = np.random.RandomState(seed)
        stage = {64: 0, 32: 1, 16: 2}[c]
        intr, extr, dr = synth.make_cameras(w * 2 ** (3 - stage), h * 2 ** (3 - stage), nsrc + 1, batch=1,
                                            rot_deg=2.0, seed=seed)
        rp, sps = O.scale_cam(intr, extr, stage)
        feas = [T(rng.randn(1, c, h, w).astype(np.float32)) for _ in range(nsrc + 1)]
        hyp = T((500 + 300 * rng.rand(1, d, h, w)).astype(np.float32))
        p = sub(seeded_sd, f"Homoaggre.{stage}.")
        exp = O.vector_aggregate(feas, rp, sps, hyp, c // 2, p, warp=O.homo_warping_explicit)
        got = ops.warp_aggregate_vec([f.to(DEV) for f in feas], ops.relative_projections(rp, sps).to(DEV),
                                     hyp.to(DEV), ops.fold_view_weight(p, c // 2).to(DEV), c // 2)
        np.testing.assert_allclose(got.cpu().numpy(), exp.numpy(), rtol=0, atol=2e-6)


def test_full_size_stage2_against_oracle_and_plane_independence(seeded_sd):
    """BASELINE config-2 spatial size (800x592 at 1/2 res, 5 views): direct oracle comparison on 2 planes,
    plus the size-independent property that planes are independent (chunking of D is exact, bitwise)."""
    h, w, c, v = 592, 800, 16, 5
    rng = np.random.RandomState(0)
    intr, extr, dr = synth.make_cameras(1600, 1184, v, batch=1, rot_deg=3.0, seed=1)
    rp, sps = O.scale_cam(intr, extr, 2)
    feas = [T(rng.randn(1, c, h, w).astype(np.float32)) for _ in range(v)]
    hyp = T((450 + 450 * rng.rand(1, 1, h, w)).astype(np.float32)) + torch.linspace(-5, 5, 8).reshape(1, 8, 1, 1)
    p = sub(seeded_sd, "Homoaggre.2.")
    proj = ops.relative_projections(rp, sps).to(DEV)
    gf = [f.to(DEV) for f in feas]
    wpar = ops.fold_view_weight(p, 8).to(DEV)
    full = ops.warp_aggregate_vec(gf, proj, hyp.to(DEV), wpar, 8)
    part = ops.warp_aggregate_vec(gf, proj, hyp[:, 2:4].contiguous().to(DEV), wpar, 8)
    assert torch.equal(full[:, :, 2:4], part)
    # live oracle on this host: use the explicit-arithmetic warp (hardware independent, pinned bitwise by the
    # goldens); the ATen-based homo_warping depends on the host CPU's BLAS kernels (observed on the GPU box).
    exp = O.vector_aggregate(feas, rp, sps, hyp[:, 2:4].contiguous(), 8, p, warp=O.homo_warping_explicit)
    np.testing.assert_allclose(part.cpu().numpy(), exp.numpy(), rtol=0, atol=2e-6)
    aten = O.homo_warping(feas[1], sps[0], rp, hyp[:, 2:3].contiguous())
    expl = O.homo_warping_explicit(feas[1], sps[0], rp, hyp[:, 2:3].contiguous())
    print("host ATen-vs-explicit warp mismatches on this CPU:", int((aten != expl).sum()), "of", aten.numel())


@pytest.mark.parametrize("stage,rot,nv", [(0, 3.0, 5), (1, 3.0, 5), (2, 3.0, 5), (2, 25.0, 3), (0, 0.0, 11)])
def test_lds_window_variant_is_bit_identical(seeded_sd, stage, rot, nv, monkeypatch):
    """The LDS-staged-window form of the eval aggregation (warp_vec_win_kernel, opt-in with MDF_WARP_WINDOW=1: measured
    slower than the L1 gather) returns the plain kernel's cost volume bit for bit -- including a strongly rotated
    view whose footprint does not fit the window pool (per-view fallback to the memory gather) and 10 source views."""
    from net.unit.scale import scale_cam
    c, g, d = ((64, 32, 48), (32, 16, 24), (16, 8, 8))[stage]
    h, w = (37, 50) if stage == 0 else ((74, 100) if stage == 1 else (148, 200))
    torch.manual_seed(stage * 7 + nv)
    intr, extr, dr = synth.make_cameras(w * 2 ** (3 - stage), h * 2 ** (3 - stage), nv, batch=2, rot_deg=rot, seed=3)
    rp, sps = scale_cam(intr, extr, stage)
    proj = ops.relative_projections(rp, list(sps)).to(DEV)
    feats = [torch.randn(2, c, h, w, device=DEV) for _ in range(nv)]
    if stage == 0:
        hyp = torch.linspace(425, 935, d, device=DEV).reshape(1, d, 1, 1).repeat(2, 1, 1, 1)
    else:
        hyp = (425 + 510 * torch.rand(2, 1, h, w, device=DEV)) + torch.linspace(-20, 20, d, device=DEV).reshape(1, d, 1, 1)
    wpar = torch.randn(g + 4, device=DEV)
    monkeypatch.delenv("MDF_WARP_WINDOW", raising=False)
    plain = ops.warp_aggregate_vec(feats, proj, hyp, wpar, g).clone()
    monkeypatch.setenv("MDF_WARP_WINDOW", "1")
    win = ops.warp_aggregate_vec(feats, proj, hyp, wpar, g)
    assert torch.equal(plain, win)


@pytest.mark.parametrize("stage,nv", [(0, 5), (1, 5), (2, 5), (1, 3), (2, 11), (0, 2)])
def test_eight_channels_per_lane_variant_is_bit_identical(seeded_sd, stage, nv, monkeypatch):
    """warp_vec8_kernel (a lane owns 8 channels = the work of two lanes of warp_kernel<C,kVec>; their two partial dot products are
    added first, which is the first step of that kernel's reduction tree) returns the same cost volume bit for bit -- all three
    channel counts, 1 / 2 pairs per thread and the generic tap-table path (10 source views)."""
    from net.unit.scale import scale_cam
    c, g, d = ((64, 32, 48), (32, 16, 24), (16, 8, 8))[stage]
    h, w = (37, 50) if stage == 0 else ((74, 100) if stage == 1 else (148, 200))
    torch.manual_seed(stage * 5 + nv)
    intr, extr, dr = synth.make_cameras(w * 2 ** (3 - stage), h * 2 ** (3 - stage), nv, batch=2, rot_deg=3.0, seed=3)
    rp, sps = scale_cam(intr, extr, stage)
    proj = ops.relative_projections(rp, list(sps)).to(DEV)
    feats = [torch.randn(2, c, h, w, device=DEV) for _ in range(nv)]
    if stage == 0:
        hyp = torch.linspace(425, 935, d, device=DEV).reshape(1, d, 1, 1).repeat(2, 1, 1, 1)
    else:
        hyp = (425 + 510 * torch.rand(2, 1, h, w, device=DEV)) + torch.linspace(-20, 20, d, device=DEV).reshape(1, d, 1, 1)
    wpar = torch.randn(g + 4, device=DEV)
    monkeypatch.setenv("MDF_WARP_VEC8", "0")
    four = ops.warp_aggregate_vec(feats, proj, hyp, wpar, g).clone()
    monkeypatch.setenv("MDF_WARP_VEC8", "2")
    eight = ops.warp_aggregate_vec(feats, proj, hyp, wpar, g)
    assert torch.equal(four, eight)
