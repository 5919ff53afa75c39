"""GPU: the depth-preserving (1,2,2) sampling layers (conv3d_hw_kernel, mdf_conv3d_hw2_fwd) against torch on the CPU, and the
RegularNet_4Scales composed with them against its own stock-module forward (the reference's forward, line for line)."""
import contextlib
import copy
import ctypes
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mdfnet_hip
from mdfnet_hip import ops, synth

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
EARG, EUNSUP = -1, -2

DOWN = [(8, 16), (16, 32), (32, 64)]
UP = [(64, 32), (32, 16), (16, 8)]
PAIRS = [(ci, co, False) for ci, co in DOWN] + [(ci, co, True) for ci, co in UP]
SHAPES = [(1, 1, 9, 37),     # a single plane: only kd = 1 exists; odd H and W: the last output row and column read the zero halo
          (2, 2, 7, 33),     # two planes, batch 2: the depth mask must not leak across items
          (2, 3, 5, 21),     # three planes, fewer rows than a tile
          (1, 4, 6, 8),      # even extents: no halo on the far side of the down mode
          (1, 8, 20, 36),    # stage-2 depth, several m-tiles, a ragged last tile
          (1, 5, 37, 53)]    # D not a multiple of anything, more tiles than one block per class


def _build(**kw):
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        return config.build_model(**kw)


def _layer_case(cin, cout, tr, shape):
    b, d, h, w = shape
    rng = np.random.RandomState(cin * 131 + cout + d * 7 + w)
    x = T(rng.randn(b, cin, d, h, w).astype(np.float32))
    wt = T((rng.randn(*((cin, cout) if tr else (cout, cin)), 3, 3, 3) / np.sqrt(27 * cin)).astype(np.float32))
    alpha = T(rng.uniform(0.5, 1.5, cout).astype(np.float32))
    beta = T(rng.uniform(-0.2, 0.2, cout).astype(np.float32))
    ref = F.conv_transpose3d(x, wt, None, (1, 2, 2), 1, (0, 1, 1)) if tr else F.conv3d(x, wt, None, (1, 2, 2), 1)
    assert tuple(ref.shape) == ((b, cout, d, 2 * h, 2 * w) if tr else (b, cout, d, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    res = T(rng.randn(*ref.shape).astype(np.float32))
    exp = F.relu(ref * alpha.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)) + res
    return x, wt, alpha, beta, res, ref, exp


def _check_layer(cin, cout, tr, shape, monkeypatch):
    x, wt, alpha, beta, res, ref, exp = _layer_case(cin, cout, tr, shape)
    wp = ops.pack_conv3d_weight(wt.to(DEV), tr)
    xd, rd, al, be = ops.to_ndhwc(x.to(DEV)), ops.to_ndhwc(res.to(DEV)), alpha.to(DEV), beta.to(DEV)
    ops.count_begin()
    y = ops.conv3d_ndhwc(xd, wp, cin, cout, (1, 2, 2), tr, al, be, True, rd)
    y2 = ops.conv3d_ndhwc(xd, wp, cin, cout, (1, 2, 2), tr)
    assert ops.count_end() == {"mdf_conv3d_hw2_fwd": 2}
    got = ops.from_ndhwc(y).cpu()
    assert got.shape == exp.shape
    print(f"{cin}->{cout} {'up' if tr else 'down'} {shape}: max |err| epilogue {(got - exp).abs().max():.3e}, raw {(ops.from_ndhwc(y2).cpu() - ref).abs().max():.3e}")
    # fp32 fma chain over K = 27*cin terms, different summation order than oneDNN (the family's bar, test_regular_gpu.py:42)
    np.testing.assert_allclose(got.numpy(), exp.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(ops.from_ndhwc(y2).cpu().numpy(), ref.numpy(), rtol=1e-4, atol=2e-5)
    # the launch rule's routes (one tile per wave, the largest wave tile, split-K where built) agree at the re-association level
    for route in ("1", "2", "3"):
        monkeypatch.setenv("MDF_CONV3D_HW_ROUTE", route)
        yr = ops.conv3d_ndhwc(xd, wp, cin, cout, (1, 2, 2), tr, al, be, True, rd)
        assert (yr - y).abs().max().item() < 2e-5, route
    monkeypatch.delenv("MDF_CONV3D_HW_ROUTE")
    # shallow volumes: with and without the skipped depth taps (they contributed exact zeros)
    if shape[1] <= 3:
        monkeypatch.setenv("MDF_CONV3D_KDSKIP", "0")
        y0 = ops.conv3d_ndhwc(xd, wp, cin, cout, (1, 2, 2), tr, al, be, True, rd)
        assert (y0 - y).abs().max().item() < 2e-5
        monkeypatch.delenv("MDF_CONV3D_KDSKIP")


@pytest.mark.parametrize("cin,cout,tr", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_hw_layer(cin, cout, tr, shape, monkeypatch):
    _check_layer(cin, cout, tr, shape, monkeypatch)


@pytest.mark.parametrize("cin,cout,tr", [(32, 64, False), (64, 32, True)])
def test_hw_layer_innermost_level_routes(cin, cout, tr, monkeypatch):
    """The innermost pair at a volume of the (2,2,2) stage-0 U-Net's bottom: few tiles and a deep K, where the rule splits the taps
    over a block's four waves."""
    _check_layer(cin, cout, tr, (1, 12, 37, 50), monkeypatch)


@pytest.mark.parametrize("cin,cout,tr,shape", [(8, 16, False, (1, 8, 240, 242)), (16, 8, True, (1, 4, 120, 121))])
def test_hw_layer_largest_wave_tile_by_rule(cin, cout, tr, shape, monkeypatch):
    """Just above the volume from which the rule itself takes the largest wave tile (448 blocks of 4 waves x 4 m-tiles x 16 voxels, per
    h-parity class in the up mode), with a ragged last block."""
    b, d, h, w = shape
    vox = b * d * h * w * 2 if tr else b * d * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
    assert 448 <= vox // 256 < 460 and vox % 256 != 0
    _check_layer(cin, cout, tr, shape, monkeypatch)


# ---------------------------------------------------------------------------------------------------- the whole regulariser
def _stock(mod, x):
    """mod._stock_forward(x) on the CPU, eval mode (running BatchNorm statistics).  The product's dispatch refuses CPU tensors; its
    stock-op route is the rehearsal backend, taken by a ConvBNReLU3D in eval mode when autograd is wanted of its input."""
    import rehearsal
    with rehearsal.mode(), torch.enable_grad():
        return mod._stock_forward(x.clone().requires_grad_(True)).detach()


def _compare_with_stock(mod_gpu, mod_cpu, cost, hyp, what):
    """mod_gpu(cost, hyp) on the HIP kernels against mod_cpu._stock_forward(cost) (+ the reference's soft-argmin) on the CPU, under the
    bars of test_regulariser_vs_reference_golden; the fp32-stock-to-float64 distance is printed beside the measured one."""
    exp_p = _stock(mod_cpu, cost)
    exp_d = torch.sum(exp_p * hyp, 1)
    p64 = _stock(copy.deepcopy(mod_cpu).double(), cost.double())
    d64 = torch.sum(p64 * hyp.double(), 1)
    with torch.no_grad():
        prob, depth = mod_gpu(cost.to(DEV), hyp.to(DEV))
    assert tuple(prob.shape) == tuple(exp_p.shape) and tuple(depth.shape) == tuple(exp_d.shape)
    rel = lambda a, b: float(((a - b).abs() / (b.abs() + 1e-30)).max())      # noqa: E731
    print(f"{what}: prob |hip - stock| max {float((prob.cpu() - exp_p).abs().max()):.3e} (rel {rel(prob.cpu().double(), exp_p.double()):.3e}), "
          f"|stock - f64| max {float((exp_p.double() - p64).abs().max()):.3e} (rel {rel(exp_p.double(), p64):.3e}); "
          f"depth |hip - stock| {float((depth.cpu() - exp_d).abs().max()):.3e}, |stock - f64| {float((exp_d.double() - d64).abs().max()):.3e}")
    np.testing.assert_allclose(prob.cpu().numpy(), exp_p.numpy(), rtol=2e-3, atol=2e-6)
    np.testing.assert_allclose(depth.cpu().numpy(), exp_d.numpy(), rtol=0, atol=5e-3)
    return prob, depth


@pytest.fixture(scope="module")
def hw_model(seeded_sd):
    model = _build(regular_stride=(1, 2, 2))
    model.load_state_dict(seeded_sd, strict=True)
    model.eval()
    return copy.deepcopy(model), model.to(DEV)      # (CPU copy for the stock forward, GPU model)


@pytest.mark.parametrize("stage", [1, 2])
def test_regulariser_vs_stock_forward(golden, hw_model, stage):
    """The (1,2,2) stage-1 / stage-2 regularisers on the golden cost volumes.  Measured on an MI355X: prob |hip - stock| 2.1e-6 (stage 1) /
    4.4e-6 (stage 2) beside |stock - float64| 1.8e-6 / 3.5e-6; depth 4.9e-4 / 3.1e-4 mm beside 3.3e-4 / 3.0e-4 -- the bars hold as they are."""
    g = golden("ops.npz")
    cpu, gpu = hw_model
    cost, hyp = T(g[f"agg{stage}_cost"]), T(g[f"agg{stage}_hyp"])
    ops.count_begin()
    prob, depth = _compare_with_stock(gpu.Regular[stage], cpu.Regular[stage], cost, hyp, f"stage {stage}")
    assert ops.count_end().get("mdf_conv3d_hw2_fwd", 0) == 6
    assert torch.equal(gpu.Regular[stage](cost.to(DEV)), prob)
    # the fused soft-argmin == the standalone Regress slot on the same prob, bit for bit
    assert torch.equal(gpu.Depth_regress(prob, hyp.to(DEV)), depth)


@pytest.mark.parametrize("shape", [(1, 8, 5, 16, 24), (2, 8, 1, 8, 16)])
def test_regulariser_runs_at_any_depth(shape):
    from net.unit.regular import RegularNet_4Scales
    torch.manual_seed(shape[2])
    mod = RegularNet_4Scales(8, 8, (1, 2, 2), (0, 1, 1)).eval()
    for m in mod.modules():                      # BatchNorm statistics away from the identity
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.uniform_(-0.1, 0.1); m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5); m.bias.data.uniform_(-0.1, 0.1)
    cost = torch.randn(*shape)
    b, _, d, h, w = shape
    hyp = torch.sort(torch.rand(b, d, h, w) * 500 + 400, dim=1)[0]
    _compare_with_stock(copy.deepcopy(mod).to(DEV), mod, cost, hyp, f"cost {shape}")


# ---------------------------------------------------------------------------------------------------- routing
def test_default_model_launches_nothing_new_and_hw_model_twelve(golden, seeded_sd, hw_model):
    w, h, v, b, rot, seed = golden("e2e_tiny.npz")["cfg"]
    scene = [t.to(DEV) for t in synth.make_scene(int(w), int(h), int(v), batch=int(b), rot_deg=float(rot), seed=int(seed))]
    default = _build()
    default.load_state_dict(seeded_sd)
    default.eval().to(DEV)
    outs = []
    for model, n in ((default, 0), (hw_model[1], 12)):
        ops.count_begin()
        with torch.no_grad():
            out = model(*scene)
        counts = ops.count_end()
        assert counts.get("mdf_conv3d_hw2_fwd", 0) == n, counts
        outs.append(out)
    for k in ("depth", "confidence"):
        assert outs[1][k].shape == outs[0][k].shape and bool(torch.isfinite(outs[1][k]).all())
    ops.count_begin()
    with torch.no_grad():
        default.Regular[1](torch.randn(1, 16, 8, 16, 24, device=DEV))
    assert ops.count_end().get("mdf_conv3d_hw2_fwd", 0) == 0


def test_training_mode_is_refused_before_any_launch():
    from net.unit.regular import RegularNet_4Scales
    mod = RegularNet_4Scales(8, 8, (1, 2, 2), (0, 1, 1)).to(DEV).train()
    x = torch.randn(1, 8, 8, 16, 16, device=DEV)
    ops.count_begin()
    try:
        with pytest.raises(NotImplementedError, match=r"\(2,2,2\)") as ei:
            mod(x)
    finally:
        counts = ops.count_end()
    assert counts == {}
    assert "rehearsal.enable(on_gpu=True)" in str(ei.value) and "reference" in str(ei.value)


# ---------------------------------------------------------------------------------------------------- ABI errors
def test_abi_errors_of_the_new_entry():
    lib = mdfnet_hip.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    x = torch.zeros(1, 2, 4, 4, 32, device=DEV)
    y = torch.zeros(1, 2, 8, 8, 64, device=DEV)
    w = torch.zeros(1 << 17, device=DEV)
    a = torch.ones(64, device=DEV)
    assert lib.mdf_conv3d_hw2_fwd(None, ptr(w), None, None, None, ptr(y), 1, 2, 4, 4, 8, 16, 0, 0, st) == EARG
    assert b"null" in lib.mdf_last_error()
    assert lib.mdf_conv3d_hw2_fwd(ptr(x), ptr(w), ptr(a), None, None, ptr(y), 1, 2, 4, 4, 8, 16, 0, 0, st) == EARG
    assert lib.mdf_conv3d_hw2_fwd(ptr(x), ptr(w), None, None, None, ptr(y), 1, 0, 4, 4, 8, 16, 0, 0, st) == EARG
    assert lib.mdf_conv3d_hw2_fwd(ptr(x), ptr(w), None, None, None, ptr(y), 1 << 10, 1 << 10, 1 << 10, 4, 8, 16, 0, 0, st) == EARG
    assert b"32-bit" in lib.mdf_last_error()
    assert lib.mdf_conv3d_hw2_fwd(ptr(x), ptr(w), None, None, None, ptr(y), 1, 2, 4, 4, 24, 16, 0, 0, st) == EUNSUP
    assert b"not built" in lib.mdf_last_error()
    assert lib.mdf_conv3d_hw2_fwd(ptr(x), ptr(w), None, None, None, ptr(y), 1, 2, 4, 4, 8, 16, 1, 0, st) == EUNSUP      # 8 -> 16 is a down pair
    # ... and the library still works
    wt = torch.ones(16, 8, 3, 3, 3, device=DEV)
    out = ops.conv3d_ndhwc(torch.ones(1, 3, 5, 5, 8, device=DEV), ops.pack_conv3d_weight(wt, False), 8, 16, (1, 2, 2))
    assert tuple(out.shape) == (1, 3, 3, 3, 16) and float(out[0, 1, 1, 1, 0]) == 8 * 27
    torch.cuda.synchronize()
