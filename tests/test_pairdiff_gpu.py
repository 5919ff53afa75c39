"""GPU: the pair-difference route of the eval forward.  With C/G = 2 the aggregation reads a feature pair (a, b) only through
b - a, so the feature pyramid's composed heads emit d[g] = f[2g+1] - f[2g] directly (half the channels) and a warp+aggregate
kernel over those maps (mdf_warp_aggregate_pairdiff_fwd) replaces mdf_warp_aggregate_vec_fwd.  Checked here: the difference heads
against an fp64 evaluation of the reference head formula, the kernel against the full-feature kernel and the oracle at the bar
that operator is held to (atol 2e-6, tests/test_warp_gpu.py), and which route a forward takes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mdfnet_hip import ops, synth
from oracle import mvs_oracle as O
from modelutil import build_model

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
STAGES = ((64, 32, 48), (32, 16, 24), (16, 8, 8))     # (C, G, D) of the three stages


def sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def pair_diff(f):
    return f[:, 1::2] - f[:, 0::2]


@pytest.fixture(scope="module")
def model(seeded_sd):
    m = build_model()
    m.load_state_dict(seeded_sd)
    return m.eval().to(DEV)


# ------------------------------------------------------------------------------------------------------------------ heads
def test_difference_heads_vs_fp64_reference_formula(model, seeded_sd):
    """Difference pyramids vs the reference head formula (oracle.fpn_4scales' last seven lines) evaluated in fp64 on the product's own
    t2 / t3 / t4 and differenced.  Yardstick: the error of the present full-channel heads, differenced, against the same fp64 values
    on the same input; the difference heads may be at most 2x that (both are fp32 evaluations of one fp64 quantity; the factor covers
    the rounding of the composed difference rows)."""
    bb = model.Backbone
    imgs = synth.make_scene(320, 256, 5, rot_deg=2.0, seed=11)[0]
    t2, t3, t4 = bb._hip_trunk(imgs[0].to(DEV))
    p = {k: v.double() for k, v in sub(seeded_sd, "Backbone.").items() if k.split(".")[0] in ("out2", "out3", "out4", "lat2", "lat3")}
    x2, x3, x4 = (t.permute(0, 3, 1, 2).double().cpu() for t in (t2, t3, t4))
    y4 = F.conv2d(x4, p["out4.weight"])
    x3 = F.interpolate(x4, scale_factor=2.0, mode="bilinear", align_corners=False) + F.conv2d(x3, p["lat3.weight"], p["lat3.bias"])
    y3 = F.conv2d(x3, p["out3.weight"])
    x2 = F.interpolate(x3, scale_factor=2.0, mode="bilinear", align_corners=False) + F.conv2d(x2, p["lat2.weight"], p["lat2.bias"])
    y2 = F.conv2d(x2, p["out2.weight"])
    full = bb._hip_heads(t2, t3, t4, pair_diff=False)
    diff = bb._hip_heads(t2, t3, t4, pair_diff=True)
    for name, ref, f, d, g in zip(("1/8", "1/4", "1/2"), (y4, y3, y2), full, diff, (32, 16, 8)):
        assert d.shape == (f.shape[0], g, f.shape[2], f.shape[3]) and f.shape[1] == 2 * g
        want = pair_diff(ref)
        e_full = (pair_diff(f.double().cpu()) - want).abs()
        e_diff = (d.double().cpu() - want).abs()
        print(f"\nlevel {name}: |difference| max {want.abs().max():.3f}; full heads, differenced: max {e_full.max():.3e} mean {e_full.mean():.3e} | "
              f"difference heads: max {e_diff.max():.3e} mean {e_diff.mean():.3e}")
        assert e_diff.max() <= 2 * e_full.max(), (name, float(e_diff.max()), float(e_full.max()))
        assert e_diff.mean() <= 2 * e_full.mean(), (name, float(e_diff.mean()), float(e_full.mean()))


# ------------------------------------------------------------------------------------------------------------------ kernel
def _case(stage, h, w, nsrc, batch, per_pixel, seed):
    c, g, d = STAGES[stage]
    rng = np.random.RandomState(seed)
    intr, extr, dr = synth.make_cameras(w * 2 ** (3 - stage), h * 2 ** (3 - stage), nsrc + 1, batch=batch, rot_deg=2.0, seed=seed)
    rp, sps = O.scale_cam(intr, extr, stage)
    feas = [T(rng.randn(batch, c, h, w).astype(np.float32)) for _ in range(nsrc + 1)]
    if per_pixel:
        hyp = T((500 + 300 * rng.rand(batch, d, h, w)).astype(np.float32))
    else:
        hyp = torch.linspace(425, 935, d).reshape(1, d, 1, 1).repeat(batch, 1, 1, 1).contiguous()
    return feas, rp, sps, hyp


def _run_both(feas, rp, sps, hyp, p, g, channels_last=True):
    proj = ops.relative_projections(rp, list(sps)).to(DEV)
    wpar = ops.fold_view_weight(p, g).to(DEV)
    gf = [f.to(DEV) for f in feas]
    full = ops.warp_aggregate_vec(gf, proj, hyp.to(DEV), wpar, g, channels_last)
    got = ops.warp_aggregate_pairdiff([pair_diff(f) for f in gf], proj, hyp.to(DEV), wpar, channels_last)
    return full, got


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_kernel_vs_full_feature_kernel_and_oracle(seeded_sd, stage, per_pixel, channels_last):
    """The three (C, D) stage shapes, per-plane and per-pixel hypotheses, both output layouts, on a ragged 13 x 11 map (143 pixels:
    no multiple of any tile), batch 2, four source views."""
    c, g, d = STAGES[stage]
    feas, rp, sps, hyp = _case(stage, 13, 11, 4, 2, per_pixel, seed=20 + stage)
    p = sub(seeded_sd, f"Homoaggre.{stage}.")
    full, got = _run_both(feas, rp, sps, hyp, p, g, channels_last)
    assert got.shape == full.shape == (2, g, d, 13, 11)
    assert got.is_contiguous() == full.is_contiguous() and got.stride() == full.stride()
    exp = O.vector_aggregate(feas, rp, sps, hyp, g, p, warp=O.homo_warping_explicit)
    dk, do = (got - full).abs().max().item(), (got.cpu() - exp).abs().max().item()
    print(f"\nstage {stage} per_pixel={per_pixel} ndhwc={channels_last}: max|d| vs full-feature kernel {dk:.3e}, vs oracle {do:.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), full.cpu().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(got.cpu().numpy(), exp.numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("gpl", ["4", "8"])
@pytest.mark.parametrize("nsrc", [1, 4, 6, 10])
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_kernel_view_counts_and_lane_mappings(seeded_sd, monkeypatch, stage, nsrc, gpl):
    """2-, 5-, 7- and 11-view items (one / two (pixel, view) pairs per thread and the generic tap-table loop) under both lane
    mappings of the kernel (4 and 8 groups per lane), ragged 9 x 31 map, per-pixel hypotheses."""
    c, g, d = STAGES[stage]
    feas, rp, sps, hyp = _case(stage, 9, 31, nsrc, 1, True, seed=40 + 3 * nsrc + stage)
    p = sub(seeded_sd, f"Homoaggre.{stage}.")
    monkeypatch.setenv("MDF_PAIRDIFF_GPL", gpl)
    full, got = _run_both(feas, rp, sps, hyp, p, g)
    exp = O.vector_aggregate(feas, rp, sps, hyp, g, p, warp=O.homo_warping_explicit)
    np.testing.assert_allclose(got.cpu().numpy(), full.cpu().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(got.cpu().numpy(), exp.numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("gpl", ["4", "8"])
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_kernel_out_of_frame_and_degenerate_planes(seeded_sd, monkeypatch, stage, gpl):
    """Samples out of frame, behind the camera (z < 0) and on its plane (z == 0 -> NaN, as grid_sample): the NaN positions of the
    new kernel, the full-feature kernel and the oracle coincide exactly, the finite values agree at the operator's bar."""
    c, g, _ = STAGES[stage]
    h, w = 12, 20
    rng = np.random.RandomState(7 + stage)
    eye = torch.eye(4).unsqueeze(0)

    def cam(t):
        m = torch.eye(4)
        m[:3, 3] = torch.tensor(t)
        return m.unsqueeze(0)
    # reference projection = identity: the relative projection is the source matrix itself, exactly.  View 0: z = depth - 600 (zero
    # on the 600 plane, negative below it), x = x_ref * depth / z runs out of frame; view 1: z = depth - 300 > 0, half in frame.
    sps = [cam([3.0, -2.0, -600.0]), cam([-100.0, 50.0, -300.0])]
    hyp = torch.tensor([500.0, 600.0, 700.0, 650.0, 610.0]).reshape(1, 5, 1, 1)
    feas = [T(rng.randn(1, c, h, w).astype(np.float32)) for _ in range(3)]
    p = sub(seeded_sd, f"Homoaggre.{stage}.")
    monkeypatch.setenv("MDF_PAIRDIFF_GPL", gpl)
    full, got = _run_both(feas, eye, sps, hyp, p, g)
    exp = O.vector_aggregate(feas, eye, sps, hyp, g, p, warp=O.homo_warping_explicit)
    nan_new, nan_full, nan_exp = torch.isnan(got).cpu(), torch.isnan(full).cpu(), torch.isnan(exp)
    assert nan_new.any() and not nan_new.all()
    assert bool(nan_new[:, :, 1].all())                       # the z == 0 plane
    assert torch.equal(nan_new, nan_full) and torch.equal(nan_new, nan_exp)
    ok = ~nan_new
    np.testing.assert_allclose(got.cpu()[ok].numpy(), full.cpu()[ok].numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(got.cpu()[ok].numpy(), exp[ok].numpy(), rtol=0, atol=2e-6)


def test_kernel_refuses_what_is_not_built():
    import mdfnet_hip
    feas = [torch.randn(1, 12, 8, 8, device=DEV) for _ in range(2)]
    proj = torch.zeros(1, 1, 12, device=DEV)
    hyp = torch.full((1, 2, 1, 1), 500.0, device=DEV)
    with pytest.raises(mdfnet_hip.MdfHipError, match="G=12"):
        ops.warp_aggregate_pairdiff(feas, proj, hyp, torch.zeros(16, device=DEV))
    with pytest.raises(ValueError, match="G \\+ 4"):
        ops.warp_aggregate_pairdiff([f[:, :8] for f in feas], proj, hyp, torch.zeros(20, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ route
NEW, OLD = "mdf_warp_aggregate_pairdiff_fwd", "mdf_warp_aggregate_vec_fwd"


class _Foreign(torch.nn.Module):
    """An aggregation slot CoreNet does not know (it wraps the built-in one: same result, full features in)."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, features, ref_proj, src_projs, depth_hypos):
        return self.inner(features, ref_proj, src_projs, depth_hypos)


def _forward_counted(m, scene):
    ops.count_begin()
    try:
        with torch.no_grad():
            out = m(*[t.to(DEV) for t in scene])
        torch.cuda.synchronize()
    finally:
        counts = ops.count_end()
    return out, counts


def test_route_taken_and_depth_of_both_routes_vs_live_oracle(model, seeded_sd, monkeypatch):
    """A default eval forward calls the new entry once per stage and the full-feature entry never; with the development switch off,
    or with one aggregation slot replaced by a foreign module, the reverse.  Depth of both routes at 320 x 256 x 5 within 1e-3 mm
    (mean) of the live oracle, the metric's own bar (tests/test_e2e_gpu.py)."""
    from net.unit import backbone
    scene = synth.make_scene(320, 256, 5, rot_deg=2.0, seed=21)
    out_new, c_new = _forward_counted(model, scene)
    assert c_new.get(NEW, 0) == 3 and c_new.get(OLD, 0) == 0, c_new
    monkeypatch.setattr(backbone, "_PAIR_DIFF", False)
    out_old, c_old = _forward_counted(model, scene)
    assert c_old.get(NEW, 0) == 0 and c_old.get(OLD, 0) == 3, c_old
    monkeypatch.setattr(backbone, "_PAIR_DIFF", True)
    slot = model.Homoaggre[1]
    try:
        model.Homoaggre[1] = _Foreign(slot)
        out_foreign, c_foreign = _forward_counted(model, scene)
    finally:
        model.Homoaggre[1] = slot
    assert c_foreign.get(NEW, 0) == 0 and c_foreign.get(OLD, 0) == 3, c_foreign
    assert torch.equal(out_foreign["depth"], out_old["depth"])            # the same kernels on the same features
    with torch.no_grad():
        live = O.core_forward(seeded_sd, *scene, warp=O.homo_warping_explicit)
    e_new = (out_new["depth"].cpu() - live["depth"]).abs()
    e_old = (out_old["depth"].cpu() - live["depth"]).abs()
    between = (out_new["depth"] - out_old["depth"]).abs()
    print(f"\nmean|d depth| vs live oracle: pair-difference route {e_new.mean():.3e} mm (max {e_new.max():.3e}), full-feature route "
          f"{e_old.mean():.3e} mm (max {e_old.max():.3e}); between the routes mean {between.mean():.3e} max {between.max():.3e}")
    assert out_new["depth"].shape == (1, 256, 320)
    assert e_new.mean() <= 1e-3 and e_old.mean() <= 1e-3


def test_direct_backbone_call_and_training_mode_keep_full_features(model):
    imgs = synth.make_scene(160, 128, 3, rot_deg=2.0, seed=3)[0][:, 0].to(DEV)
    with torch.no_grad():
        assert [f.shape[1] for f in model.Backbone(imgs)] == [64, 32, 16]
        assert [f.shape[1] for f in model.Backbone(imgs, pair_diff=True)] == [32, 16, 8]
    model.train()
    try:
        assert not model._pair_diff_route(imgs)
    finally:
        model.eval()
    assert model._pair_diff_route(imgs)


def test_feature_cache_never_mixes_the_two_forms(model, monkeypatch):
    """A cache filled on one route and read on the other (the development switch flipped in between) recomputes the pyramids instead
    of feeding difference maps to the full-feature kernel or the reverse; cached and uncached runs of one route are bit-identical."""
    from net.unit import backbone
    scene = [t.to(DEV) for t in synth.make_scene(160, 128, 3, rot_deg=2.0, seed=5)]
    keys = [("scan", v) for v in range(3)]
    cache = {}
    with torch.no_grad():
        plain_new = model(*scene)["depth"]
        cached_new = model(*scene, feature_cache=cache, view_keys=keys)["depth"]
        again_new = model(*scene, feature_cache=cache, view_keys=keys)["depth"]
        monkeypatch.setattr(backbone, "_PAIR_DIFF", False)
        plain_old = model(*scene)["depth"]
        cached_old = model(*scene, feature_cache=cache, view_keys=keys)["depth"]
    assert torch.equal(plain_new, cached_new) and torch.equal(plain_new, again_new)
    assert torch.equal(plain_old, cached_old)
    assert all(cache[k][0][0].shape[1] == 64 for k in keys)
