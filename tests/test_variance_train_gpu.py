"""GPU: training of the variance cost-volume aggregation (homo_aggregate_by_variance, net/unit/homoaggregate.py:49-69) and of the
stand-alone homo_warping on the hand-written kernels (csrc/warp_variance_train.hip, train_ops.VarianceAggregateTrainFn /
HomoWarpTrainFn), and of the whole model composed with it (config.build_model(aggregate="variance")).

Checker: torch autograd over the ORACLE's restatements (oracle.mvs_oracle.variance_aggregate / homo_warping and, for the whole
model, the same composition written from the oracle's public functions) in fp32 and in float64.  The rehearsal backend is not a
checker.  Slot bars are those of the sibling slot (tests/test_train_gpu.py::test_vector_aggregate_training_forward_backward: the
same warp, soft-max and scatter arithmetic) against the fp32 oracle, whose sample positions the kernels share bit for bit; the
float64 distances are printed -- the float64 run rounds the sampling grid differently, so on the large maps the fp32 oracle itself
is up to ~1e-4 away from it.  The whole model is judged by the project's standing rule: never farther from float64 than 1.5 x the
farthest fp32-oracle run over the unperturbed input and six one-ulp draws."""
import contextlib
import io

import numpy as np
import pytest
import torch

from mdfnet_hip import ddp, ops, synth
from oracle import mvs_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
CDS = ((64, 48), (32, 24), (16, 8))        # (feature channels, depth planes) of the three stages


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _variance_model():
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        m = config.build_model(aggregate="variance")
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=1))
    return m


# ----------------------------------------------------------------------------------------------- the oracle runs
def _oracle_variance(feats, rp, sps, hyp, dcost, dtype):
    """autograd over oracle.mvs_oracle.variance_aggregate, in the manner of oracle/train_check.py:aggregate."""
    f = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in feats]
    with O.precision(dtype):
        cost = O.variance_aggregate(f, rp.to(dtype), tuple(s.to(dtype) for s in sps), hyp.to(dtype))
    cost.backward(dcost.detach().cpu().to(dtype))
    return {"cost": cost.detach(), "dfeats": [t.grad for t in f]}


def _oracle_warp(src, sp, rp, hyp, dvol, dtype):
    s = src.detach().cpu().to(dtype).clone().requires_grad_(True)
    with O.precision(dtype):
        vol = O.homo_warping(s, sp.to(dtype), rp.to(dtype), hyp.to(dtype))
    vol.backward(dvol.detach().cpu().to(dtype))
    return {"vol": vol.detach(), "dsrc": s.grad}


def _slot_case(stage, b, h, w, nviews, per_pixel, cam_seed, feat_seed):
    from net.unit.scale import scale_cam
    c, d = CDS[stage]
    torch.manual_seed(feat_seed)
    intr, extr, dr = synth.make_cameras(w * 2 ** (3 - stage), h * 2 ** (3 - stage), nviews, batch=b, rot_deg=2.0, seed=cam_seed)
    rp, sps = scale_cam(intr, extr, stage)
    feats = [torch.randn(b, c, h, w) for _ in range(nviews)]
    if per_pixel:
        hyp = (425 + 510 * torch.rand(b, 1, h, w)) + torch.linspace(-20, 20, d).reshape(1, d, 1, 1)
    else:
        hyp = torch.linspace(425, 935, d).reshape(1, d, 1, 1).repeat(b, 1, 1, 1)
    dcost = torch.randn(b, c, d, h, w)
    return feats, rp, sps, hyp, dcost


def _run_slot(feats, rp, sps, hyp, dcost):
    from net.unit.homoaggregate import homo_aggregate_by_variance
    fd = [f.to(DEV).requires_grad_(True) for f in feats]
    cost = homo_aggregate_by_variance(fd, rp.to(DEV), tuple(s.to(DEV) for s in sps), hyp.to(DEV))
    cost.backward(dcost.to(DEV))
    return cost.detach(), fd


SLOT_CASES = [
    # the three of test_vector_aggregate_training_forward_backward (same cameras, same hypotheses) ...
    (0, 2, 12, 20, 3, False), (1, 1, 24, 36, 4, True), (2, 1, 32, 48, 5, True),
    # ... and the three cfg3 stage shapes (768 x 576, 5 views)
    (0, 1, 72, 96, 5, False), (1, 1, 144, 192, 5, True), (2, 1, 288, 384, 5, True)]


# ----------------------------------------------------------------------------------------------- 1. slot forward + backward
@pytest.mark.parametrize("stage,b,h,w,nviews,per_pixel", SLOT_CASES)
def test_variance_aggregate_training_forward_backward(stage, b, h, w, nviews, per_pixel):
    """Forward max|d|/max|ref| < 2e-5 and every feature gradient < 2e-4 against the fp32 oracle; the training forward is
    bit-identical to the eval kernel (it is that kernel, writing NDHWC)."""
    feats, rp, sps, hyp, dcost = _slot_case(stage, b, h, w, nviews, per_pixel, cam_seed=stage + 7, feat_seed=stage)
    r32 = _oracle_variance(feats, rp, sps, hyp, dcost, torch.float32)
    r64 = _oracle_variance(feats, rp, sps, hyp, dcost, torch.float64)
    assert not torch.isnan(r32["cost"]).any()
    with torch.no_grad():
        outside = (O.homo_warping(torch.ones(b, 1, h, w), sps[0], rp, hyp) == 0).float().mean()
    cost, fd = _run_slot(feats, rp, sps, hyp, dcost)
    with torch.no_grad():
        proj = ops.relative_projections(rp, list(sps)).to(DEV)
        ev = ops.warp_aggregate_var([f.to(DEV) for f in feats], proj, hyp.to(DEV), channels_last=True)
    e_cost = _rel(cost, r32["cost"])
    e_grads = [_rel(a.grad, r_) for a, r_ in zip(fd, r32["dfeats"])]
    print(f"\nstage {stage} {w}x{h} V{nviews}: {float(outside):.1%} of view 1's samples fully outside; vs fp32 oracle: cost {e_cost:.1e}, "
          f"d feats {[f'{e:.1e}' for e in e_grads]}; L2 vs float64: cost HIP {_l2(cost, r64['cost']):.1e} | oracle {_l2(r32['cost'], r64['cost']):.1e}; "
          f"d ref HIP {_l2(fd[0].grad, r64['dfeats'][0]):.1e} | oracle {_l2(r32['dfeats'][0], r64['dfeats'][0]):.1e}; "
          f"d src1 HIP {_l2(fd[1].grad, r64['dfeats'][1]):.1e} | oracle {_l2(r32['dfeats'][1], r64['dfeats'][1]):.1e}")
    assert cost.shape == r32["cost"].shape and ops.to_ndhwc(cost).data_ptr() == cost.data_ptr()       # NDHWC memory: no layout pass
    assert torch.equal(cost, ev)
    assert e_cost < 2e-5
    for i, e in enumerate(e_grads):
        assert e < 2e-4, f"feature {i}: {e}"


def test_view_major_features_take_and_return_one_tensor():
    """The `_mdf_parent` convention of FPN_4Scales.forward_views: the views as slices of ONE view-major tensor give the same
    cost and the gradient as one tensor."""
    from net.unit.homoaggregate import homo_aggregate_by_variance
    feats, rp, sps, hyp, dcost = _slot_case(1, 2, 24, 36, 4, True, cam_seed=8, feat_seed=1)
    cost, fd = _run_slot(feats, rp, sps, hyp, dcost)
    allv = torch.cat(feats, 0).to(DEV).requires_grad_(True)
    views = [allv[v * 2:(v + 1) * 2] for v in range(4)]
    for v, t in enumerate(views):
        t._mdf_parent = (allv, v, 4)
    cost2 = homo_aggregate_by_variance(views, rp.to(DEV), tuple(s.to(DEV) for s in sps), hyp.to(DEV))
    cost2.backward(dcost.to(DEV))
    assert torch.equal(cost2, cost)
    for v in range(4):
        assert _rel(allv.grad[v * 2:(v + 1) * 2], fd[v].grad) < 2e-5      # (float atomics: summation order only)


# ----------------------------------------------------------------------------------------------- 2. homo_warping stand-alone
@pytest.mark.parametrize("stage,b,h,w,nviews,per_pixel", SLOT_CASES[:3])
def test_homo_warping_backward(stage, b, h, w, nviews, per_pixel):
    from net.unit.base import homo_warping
    feats, rp, sps, hyp, dcost = _slot_case(stage, b, h, w, nviews, per_pixel, cam_seed=stage + 7, feat_seed=stage)
    src, dvol = feats[1], dcost
    r32 = _oracle_warp(src, sps[0], rp, hyp, dvol, torch.float32)
    r64 = _oracle_warp(src, sps[0], rp, hyp, dvol, torch.float64)
    with torch.no_grad():
        ev = homo_warping(src.to(DEV), sps[0].to(DEV), rp.to(DEV), hyp.to(DEV))
    sd = src.to(DEV).requires_grad_(True)
    vol = homo_warping(sd, sps[0].to(DEV), rp.to(DEV), hyp.to(DEV))
    assert vol.requires_grad and torch.equal(vol, ev)
    vol.backward(dvol.to(DEV))
    e = _rel(sd.grad, r32["dsrc"])
    print(f"\nstage {stage}: d src vs fp32 oracle {e:.1e}; L2 vs float64: HIP {_l2(sd.grad, r64['dsrc']):.1e} | oracle {_l2(r32['dsrc'], r64['dsrc']):.1e}")
    assert _rel(vol, r32["vol"]) < 2e-5
    assert e < 2e-4


# ----------------------------------------------------------------------------------------------- 3. ragged and extreme shapes
@pytest.mark.parametrize("h,w,c,nsrc,d,seed", [(7, 9, 64, 1, 1, 1), (13, 11, 32, 10, 3, 2), (5, 31, 16, 2, 5, 3)])
def test_ragged_and_edge_shapes(h, w, c, nsrc, d, seed):
    """Pixel counts that are not multiples of the tile, 1 and 10 source views, D = 1 (tests/test_warp_gpu.py's shapes)."""
    from net.unit.base import homo_warping
    rng = np.random.RandomState(seed)
    stage = {64: 0, 32: 1, 16: 2}[c]
    intr, extr, dr = synth.make_cameras(w * 2 ** (3 - stage), h * 2 ** (3 - stage), nsrc + 1, batch=1, rot_deg=2.0, seed=seed)
    rp, sps = O.scale_cam(intr, extr, stage)
    feats = [T(rng.randn(1, c, h, w).astype(np.float32)) for _ in range(nsrc + 1)]
    hyp = T((500 + 300 * rng.rand(1, d, h, w)).astype(np.float32))
    dcost = T(rng.randn(1, c, d, h, w).astype(np.float32))
    r32 = _oracle_variance(feats, rp, sps, hyp, dcost, torch.float32)
    cost, fd = _run_slot(feats, rp, sps, hyp, dcost)
    assert _rel(cost, r32["cost"]) < 2e-5
    for i, (a, r_) in enumerate(zip(fd, r32["dfeats"])):
        assert _rel(a.grad, r_) < 2e-4, f"feature {i}"
    w32 = _oracle_warp(feats[-1], sps[-1], rp, hyp, dcost, torch.float32)
    sd = feats[-1].to(DEV).requires_grad_(True)
    homo_warping(sd, sps[-1].to(DEV), rp.to(DEV), hyp.to(DEV)).backward(dcost.to(DEV))
    assert _rel(sd.grad, w32["dsrc"]) < 2e-4


def _magnifying_cameras():
    """Reference projection = identity, so the relative projection is the source matrix itself, in pixel units: x' = (x d + tx) /
    (d + tz).  With tz close to -d a source view magnifies 2x..6x over the depth range 500..800, so the taps of a 4 x 4 pixel tile
    over one chunk of planes cover more texels than the scatter's LDS window holds near the map's origin (the direct-to-memory
    path), and run out of frame further out (windows of the few live taps).
    The arithmetic for view 0 (tz = -420, magnification d / (d - 420) = 6.25 at d = 500 down to 2.1 at d = 800, per-pixel d anywhere
    between): the tile at the origin (x, y in 0..3) maps to x' = 0..18.75, y' = 0..18.75, clamped into the 15 x 13 map: a live box of
    15 x 13 = 195 texels, above both window sizes (4096 floats / 64 channels = 64 texels, / 32 groups = 128 texels) -> direct to
    memory.  The tile at x0 = 4, y0 = 4 maps to x' >= 8.4, y' >= 8.4, in frame only up to 14 and 12: at most 7 x 5 = 35 texels ->
    window.  (Also run once with a library built with a 64-float window, where every footprint takes the direct path.)"""
    def cam(t):
        m = torch.eye(4)
        m[:3, 3] = torch.tensor(t)
        return m.unsqueeze(0)
    return torch.eye(4).unsqueeze(0), [cam([0.0, 0.0, -420.0]), cam([10.0, -5.0, -400.0])]


def test_scatter_window_and_direct_to_memory_paths():
    """Both ways of the scatter in one launch, for the variance backward and the stand-alone warp backward: tiles whose footprint
    fits the LDS window and tiles that scatter to memory directly (13 x 15 map, 64 channels: a window holds 64 texels).  Same
    oracle and bars as test_ragged_and_edge_shapes."""
    from net.unit.base import homo_warping
    h, w, c, d = 13, 15, 64, 5
    rng = np.random.RandomState(5)
    rp, sps = _magnifying_cameras()
    feats = [T(rng.randn(1, c, h, w).astype(np.float32)) for _ in range(3)]
    hyp = T((500 + 300 * rng.rand(1, d, h, w)).astype(np.float32))
    dcost = T(rng.randn(1, c, d, h, w).astype(np.float32))
    r32 = _oracle_variance(feats, rp, sps, hyp, dcost, torch.float32)
    cost, fd = _run_slot(feats, rp, sps, hyp, dcost)
    e_cost, e_grads = _rel(cost, r32["cost"]), [_rel(a.grad, r_) for a, r_ in zip(fd, r32["dfeats"])]
    w32 = _oracle_warp(feats[1], sps[0], rp, hyp, dcost, torch.float32)
    sd = feats[1].to(DEV).requires_grad_(True)
    homo_warping(sd, sps[0].to(DEV), rp.to(DEV), hyp.to(DEV)).backward(dcost.to(DEV))
    e_warp = _rel(sd.grad, w32["dsrc"])
    print(f"\ncost {e_cost:.1e}, d feats {[f'{e:.1e}' for e in e_grads]}, warp d src {e_warp:.1e}")
    assert e_cost < 2e-5
    for i, e in enumerate(e_grads):
        assert e < 2e-4, f"feature {i}: {e}"
    assert e_warp < 2e-4


# ----------------------------------------------------------------------------------------------- 4. non-finite upstream gradient
@pytest.mark.parametrize("stage", [0, 2])
def test_nonfinite_upstream_gradient_propagates_like_the_oracle(stage):
    """The strong-parallax cameras of test_aggregate_backward_nonfinite_gradient_does_not_fault (many samples leave the source
    maps: out-of-bounds taps next to live ones), d cost NaN on every other plane and inf on some: the gradients are NaN exactly
    where autograd over the oracle (grid_sample's backward) has NaN -- a zero-weight out-of-bounds tap receives nothing --, and the
    finite case right after is finite and within the bars."""
    from net.unit.scale import scale_cam
    c, d = CDS[stage]
    h, w = 192 >> (3 - stage), 256 >> (3 - stage)
    torch.manual_seed(60 + stage)
    intr, extr, dr = synth.make_cameras(256, 192, 4, batch=1, rot_deg=2.0, seed=60 + stage + 7)
    rp, sps = scale_cam(intr, extr, stage)
    feats = [torch.randn(1, c, h, w) for _ in range(4)]
    if stage == 0:
        hyp = torch.linspace(425, 935, d).reshape(1, d, 1, 1)
    else:
        hyp = (425 + 510 * torch.rand(1, 1, h, w)) + torch.linspace(-200.0, 200.0, d).reshape(1, d, 1, 1)
    sps = tuple(s.clone() for s in sps)
    for i, s_ in enumerate(sps):
        s_[:, 0, 3] += (-1) ** i * 0.4 * (256 >> (3 - stage)) * 650.0      # ~0.4 map widths of shift at mid range
    good = torch.randn(1, c, d, h, w)
    bad = good.clone()
    bad[:, :, ::2] = float("nan")
    bad[:, :, 1, ::3] = float("inf")
    rbad = _oracle_variance(feats, rp, sps, hyp, bad, torch.float32)
    _, fd = _run_slot(feats, rp, sps, hyp, bad)
    torch.cuda.synchronize()
    for i, (a, r_) in enumerate(zip(fd, rbad["dfeats"])):
        mine, want = torch.isnan(a.grad.cpu()), torch.isnan(r_)
        assert want.any()
        assert torch.equal(mine, want), (i, int(mine.sum()), int(want.sum()), int((mine != want).sum()))
    rgood = _oracle_variance(feats, rp, sps, hyp, good, torch.float32)
    cost, fd = _run_slot(feats, rp, sps, hyp, good)
    assert torch.isfinite(cost).all() and _rel(cost, rgood["cost"]) < 2e-5
    for i, (a, r_) in enumerate(zip(fd, rgood["dfeats"])):
        assert torch.isfinite(a.grad).all() and _rel(a.grad, r_) < 2e-4, f"feature {i}"


# ----------------------------------------------------------------------------------------------- 6. whole model
def _oracle_core(sd, imgs, extr, intr, dr, ndepths=(48, 24, 8)):
    """oracle.mvs_oracle.core_forward(training=True) with variance_aggregate in the aggregation slots (net/core.py:30-78)."""
    def sub(prefix):
        return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    views = torch.unbind(imgs.to(O.WORK), 1)
    feats = [O.fpn_4scales(v, sub("Backbone."), True) for v in views]
    depth = hyp = prob = None
    depths = []
    for st in range(3):
        fea = [f[st] for f in feats]
        ref_proj, src_projs = O.scale_cam(intr, extr, st)
        hyp = O.hypos_by_fit(depth, dr, prob, hyp, ndepths[st], O.CURVES[st], O.THRESH[st], True)
        cost = O.variance_aggregate(fea, ref_proj, src_projs, hyp)
        prob = O.regular(cost, sub(f"Regular.{st}."), True)
        depth = O.depth_regression(prob, hyp)
        depths.append(depth)
    depths.append(O.refine_net2(depth, dr, sub("Refine.")))
    return depths


def _oracle_step(sd32, scene, gt, dtype):
    imgs, extr, intr, dr = scene
    f32 = torch.float32
    sd = {k: (v.to(dtype).clone().requires_grad_(True) if v.dtype == f32 and "running" not in k else (v.to(dtype) if v.dtype == f32 else v.clone()))
          for k, v in sd32.items()}
    with O.precision(dtype):
        depths = _oracle_core(sd, imgs.to(dtype), extr.to(dtype), intr.to(dtype), dr.to(dtype))
        loss = O.mvs_loss(depths, {k: v.to(dtype) for k, v in gt.items()}, dr.to(dtype))
    loss.backward()
    return float(loss), [d_.detach() for d_ in depths], {k: v.grad for k, v in sd.items() if getattr(v, "grad", None) is not None}


def _gt(rng, b, h, w):
    return {str(s): T((425 + 510 * rng.rand(b, h >> s, w >> s)).astype(np.float32)) for s in (3, 2, 1, 0)}


def test_variance_model_training_step_vs_the_oracle():
    """config.build_model(aggregate="variance").train() on the GPU without the rehearsal backend, 160 x 128, 3 views, batch 2,
    seeded weights (peaked prob heads), loss and one backward: the four depths and every parameter gradient at most 1.5 x as far
    (L2) from the float64 oracle as the farthest fp32-oracle run (unperturbed + six one-ulp draws), median ratio <= 1.5."""
    import rehearsal
    from net.loss import Loss
    from oracle.gen_golden import one_ulp
    assert not rehearsal.enabled()
    m = _variance_model()
    sd32 = {k: v.clone() for k, v in m.state_dict().items()}
    assert not any(k.startswith("Homoaggre.") for k in sd32)
    scene = synth.make_scene(160, 128, 3, batch=2, rot_deg=3.0, seed=31)
    gt = _gt(np.random.RandomState(7), 2, 128, 160)
    _, d64, g64 = _oracle_step(sd32, scene, gt, torch.float64)
    first = spread_d = spread_g = None
    for t in range(-1, 6):
        sc, src = scene, sd32
        if t >= 0:
            torch.manual_seed(t)
            sc = (scene[0] * one_ulp(scene[0].shape),) + tuple(scene[1:])
            src = {k: (v * one_ulp(v.shape) if v.dtype == torch.float32 and "running" not in k else v) for k, v in sd32.items()}
        loss32, d32, g32 = _oracle_step(src, sc, gt, torch.float32)
        ed = [_l2(a, b) for a, b in zip(d32, d64)]
        eg = {k: _l2(g32[k], g64[k]) for k in g64}
        if first is None:
            first, loss_ref = (ed, eg), loss32
            spread_d, spread_g = list(ed), dict(eg)
        spread_d = [max(a, b) for a, b in zip(spread_d, ed)]
        spread_g = {k: max(spread_g[k], eg[k]) for k in eg}
    m.train().to(DEV)
    imgs, extr, intr, dr = scene
    ops.count_begin()
    out = m(imgs.to(DEV), extr.to(DEV), intr.to(DEV), dr.to(DEV))
    loss = Loss()(out, {k: v.to(DEV) for k, v in gt.items()}, dr.to(DEV))
    loss.backward()
    calls = ops.count_end()
    assert calls.get("mdf_warp_aggregate_var_fwd") == 3 and calls.get("mdf_warp_aggregate_var_bwd") == 3, calls
    print(f"\nloss HIP {float(loss):.6f} fp32 oracle {loss_ref:.6f}")
    bad = []
    for i, d_ in enumerate(out["depth"]):
        e = _l2(d_, d64[i])
        print(f"depth{i}: L2 vs float64: HIP {e:.2e} | fp32 oracle {first[0][i]:.2e} | worst of 7 {spread_d[i]:.2e}")
        bad += [("depth", i, e, spread_d[i])] if e > 1.5 * spread_d[i] else []
    rows = []
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
        e = _l2(p.grad, g64[k])
        rows.append((e / max(spread_g[k], 1e-30), e, first[1][k], spread_g[k], k))
    rows.sort(reverse=True)
    med = float(np.median([e / max(f_, 1e-30) for _, e, f_, _, _ in rows]))
    print("parameter gradients, L2 vs float64 -- worst HIP / fp32-spread:",
          [(f"{q:.2f}", f"HIP {e:.1e}", f"oracle {f_:.1e}", f"spread {s_:.1e}", k) for q, e, f_, s_, k in rows[:6]],
          f"; median HIP / fp32 oracle {med:.2f} over {len(rows)} tensors")
    bad += [r for r in rows if r[0] > 1.5]
    assert not bad, bad[:6]
    assert med <= 1.5, med


# ----------------------------------------------------------------------------------------------- 7. recorded step
def test_variance_model_replayed_step_equals_the_eager_step():
    """The same model through graphstep.GraphedTrainStep at learning rate 0: a replayed step on inputs the recording has never
    seen gives the eager step's loss (2e-5 relative) and gradients (finite, L2 < 1e-3) -- the bars of
    tests/test_train_graph_gpu.py::test_replayed_step_follows_its_inputs."""
    from mdfnet_hip.graphstep import GraphedTrainStep
    from mdfnet_hip.optim import FlatAdam
    from net.loss import Loss
    W, H, V = 192, 128, 3

    def scene(k):
        imgs, extr, intr, dr = synth.make_scene(W, H, V, batch=1, rot_deg=2.0 + k, seed=11 + 5 * k)
        dr = dr * (1.0 + 0.03 * k)
        rng = np.random.RandomState(100 + k)
        lo, hi = float(dr[0, 0]), float(dr[0, 1])
        gt = {str(s): T((lo - 20 + (hi - lo + 20) * rng.rand(1, H >> s, W >> s)).astype(np.float32)) for s in (3, 2, 1, 0)}
        return imgs, extr, intr, dr, gt

    crit = Loss().to(DEV)
    me, mg = _variance_model().train().to(DEV), _variance_model().train().to(DEV)
    be, bg = ddp.FlatBucket(me), ddp.FlatBucket(mg)
    oe, og = FlatAdam(be, lr=0.0), FlatAdam(bg, lr=0.0)
    s0 = scene(0)
    step = GraphedTrainStep(mg, crit, bg, og, tuple(t.to(DEV) for t in s0[:4]) + ({k: v.to(DEV) for k, v in s0[4].items()},), warmup=2)
    for k in (1, 2, 0, 3):
        imgs, extr, intr, dr, gt = scene(k)
        out = me(imgs.to(DEV), extr.to(DEV), intr.to(DEV), dr.to(DEV))
        loss = crit(out, {n: v.to(DEV) for n, v in gt.items()}, dr.to(DEV))
        be.zero_grad()
        loss.backward()
        be.allreduce_gradients()
        oe.step()
        le, lg = float(loss), float(step(imgs, extr, intr, dr, gt))
        print(f"\nscene {k}: loss eager {le:.6f} graph {lg:.6f}; gradient L2 rel {_l2(bg.flat, be.flat):.2e}")
        assert abs(lg - le) <= 2e-5 * abs(le)
        assert torch.isfinite(bg.flat).all() and _l2(bg.flat, be.flat) < 1e-3


# ----------------------------------------------------------------------------------------------- 8. slots without a training kernel
def test_foreign_aggregation_slot_is_refused_when_the_training_forward_starts():
    from net.unit.homoaggregate import homo_aggregate_by_variance

    class Foreign(torch.nn.Module):
        def forward(self, features, ref_proj, src_projs, depth_hypos):
            return homo_aggregate_by_variance(features, ref_proj, src_projs, depth_hypos)

    m = _variance_model().train().to(DEV)
    m.Homoaggre[1] = Foreign()
    imgs, extr, intr, dr = synth.make_scene(160, 128, 3, batch=1, rot_deg=2.0, seed=3)
    ops.count_begin()
    try:
        with pytest.raises(RuntimeError, match=r"Homoaggre\[1\] \(Foreign\)"):
            m(imgs.to(DEV), extr.to(DEV), intr.to(DEV), dr.to(DEV))
    finally:
        calls = ops.count_end()
    assert not calls, calls                     # refused before any kernel of the library was launched
    m.eval()                                    # eval keeps accepting any slot
    with torch.no_grad():
        out = m(imgs.to(DEV), extr.to(DEV), intr.to(DEV), dr.to(DEV))
    assert torch.isfinite(out["depth"]).all()


# ----------------------------------------------------------------------------------------------- the regularisers' new first layers
@pytest.mark.parametrize("cin,cout", [(64, 16), (32, 8), (16, 8)])
def test_first_regulariser_layers_behind_a_variance_cost_volume(cin, cout):
    """The variance cost volume has the C feature channels, so the regularisers start with 64 -> 16, 32 -> 8, 16 -> 8 (stride 1):
    eval forward (Conv3d + folded BatchNorm + ReLU) at a small volume and at one above the LDS kernels' threshold, input gradient
    (the pairs 16 -> 64, 8 -> 32, 8 -> 16 on re-packed weights) and weight gradient, against torch on the CPU -- the bars of
    tests/test_train_gpu.py::test_conv3d_input_and_weight_gradients."""
    import torch.nn as nn
    from mdfnet_hip import train_ops
    from net.unit.base import ConvBNReLU3D
    torch.manual_seed(cin + cout)
    blk = ConvBNReLU3D(cin, cout)
    with torch.no_grad():
        blk.bn.weight.uniform_(0.5, 1.5); blk.bn.bias.uniform_(-0.3, 0.3)
        blk.bn.running_mean.normal_(0, 0.2); blk.bn.running_var.uniform_(0.5, 2.0)
    blk.eval()
    for d, h, w in ((4, 6, 22), (8, 140, 150)):
        x = torch.randn(1, cin, d, h, w)
        with torch.no_grad():
            want = blk.relu(blk.bn(blk.conv(x)))
            blk.to(DEV)
            got = blk(x.to(DEV))
            blk.to("cpu")
        assert _rel(got, want) < 2e-5, (d, h, w)
    conv = nn.Conv3d(cin, cout, 3, stride=1, padding=1, bias=False)
    x = torch.randn(2, cin, 4, 6, 22, requires_grad=True)
    y = conv(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    convd = conv.to(DEV)
    xd, dyd = ops.to_ndhwc(x.detach().to(DEV)), ops.to_ndhwc(dy.to(DEV))
    assert _rel(ops.from_ndhwc(train_ops.conv3d_dgrad(convd, False, dyd)), x.grad) < 2e-5
    assert _rel(train_ops.conv3d_wgrad(dyd, xd, 1, tuple(conv.weight.shape)), conv.weight.grad.cpu()) < 3e-5
