"""CPU: the float64 references of tests/conv_mirror.py against torch.nn.functional in float64 and the network's modules, the exactness
condition of the exact generator for every case of the table, the proof that a correct fp32 Winograd kernel meets the random bar and
that the bars catch deliberate errors, and the table's reach over the rows of conv_lds.hip.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_mirror as M  # noqa: E402

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
cl2 = lambda t: t.permute(0, 2, 3, 1).numpy()             # [B,C,H,W] -> channels-last
cl3 = lambda t: t.permute(0, 2, 3, 4, 1).numpy()


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


# ---------------------------------------------------------------------------------------------------------------- reference vs torch
SHAPES2D = [(3, 7, 9), (1, 1, 13), (2, 12, 1), (1, 1, 1), (2, 6, 8)]          # odd extents, batch 3, one row, one column, one pixel, even
SHAPES3D = [(3, 3, 7, 9), (1, 1, 5, 7), (2, 2, 1, 6), (1, 4, 6, 1), (1, 5, 6, 8)]


@pytest.mark.parametrize("k,stride", [(1, 1), (3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("shape", SHAPES2D)
def test_conv2d_reference_equals_torch_float64(k, stride, shape):
    b, h, w = shape
    rs = M.rng(k, stride, *shape)
    o = M.random_operands(rs, "normal", (b, 1, h, w, 5), (6, 5, 1, k, k), (1, stride, stride))
    x, wt = o["x"][:, 0], o["w"][:, :, 0]
    y, a = M.conv2d_ref(x, wt, stride)
    xt, wtt = T64(x).permute(0, 3, 1, 2), T64(wt)
    assert close(y, cl2(F.conv2d(xt, wtt, None, stride, (k - 1) // 2)))
    assert close(a, cl2(F.conv2d(xt.abs(), wtt.abs(), None, stride, (k - 1) // 2)))
    # the planar image layout is the same layer on a permuted tensor
    assert np.array_equal(M.conv2d_ref(np.ascontiguousarray(x.transpose(0, 3, 1, 2)).transpose(0, 2, 3, 1), wt, stride)[0], y)


@pytest.mark.parametrize("stride,transposed", [(1, False), (2, False), ((1, 2, 2), False), (2, True), ((1, 2, 2), True)])
@pytest.mark.parametrize("shape", SHAPES3D)
def test_conv3d_reference_equals_torch_float64(stride, transposed, shape):
    b, d, h, w = shape
    rs = M.rng(transposed, *M._triple(stride), *shape)
    wshape = (5, 6, 3, 3, 3) if transposed else (6, 5, 3, 3, 3)
    o = M.random_operands(rs, "normal", (b, d, h, w, 5), wshape, stride, transposed)
    y, a = M.conv_ref(o["x"], o["w"], stride, transposed)
    xt, wt = T64(o["x"]).permute(0, 4, 1, 2, 3), T64(o["w"])
    s3 = M._triple(stride)
    f = (lambda x_, w_: F.conv_transpose3d(x_, w_, None, s3, 1, tuple(s - 1 for s in s3))) if transposed else (lambda x_, w_: F.conv3d(x_, w_, None, s3, 1))
    assert close(y, cl3(f(xt, wt))) and close(a, cl3(f(xt.abs(), wt.abs())))
    assert y.shape == o["res"].shape
    # the fp32 chain is the same operation: a few u of A from it
    c = M.chain32(o["x"], o["w"], stride, transposed)
    assert M.metrics(c, y, a)["perA"] < 16 * M.U


def test_epilogue_equals_the_modules():
    """ConvBNReLU / ConvBNReLU3D in eval mode (net/unit/base.py), F.interpolate + lateral (backbone.py:58-66), the Res block and
    conv2 = conv -> PixelShuffle(2) -> conv of RefineNet2 (refine.py:18-44), all in float64."""
    from mdfnet_hip import ops
    from net.unit.base import ConvBNReLU, ConvBNReLU3D, Res
    from net.unit.refine import RefineNet2
    torch.manual_seed(3)
    for mod, x in ((ConvBNReLU(5, 8, 3, 1), torch.randn(3, 5, 7, 9)), (ConvBNReLU(5, 8, 5, 2), torch.randn(2, 5, 7, 10)),
                   (ConvBNReLU3D(5, 8, 3, 2), torch.randn(2, 5, 3, 7, 9))):
        mod = mod.double().eval()
        mod.bn.running_mean.normal_(), mod.bn.running_var.uniform_(0.5, 2), mod.bn.weight.data.normal_(), mod.bn.bias.data.normal_()
        x = x.double()
        with torch.no_grad():
            want = F.relu(mod.bn(mod.conv(x)))
        invstd = 1.0 / torch.sqrt(mod.bn.running_var + mod.bn.eps)
        alpha = (mod.bn.weight * invstd).detach().numpy()
        beta = (mod.bn.bias - mod.bn.running_mean * mod.bn.weight * invstd).detach().numpy()
        wt = mod.conv.weight.detach().numpy()
        if x.dim() == 4:
            acc, want = M.taps(cl2(x)[:, None], wt[:, :, None], (1,) + tuple(mod.conv.stride))[:, 0], cl2(want)
        else:
            acc, want = M.taps(cl3(x), wt, tuple(mod.conv.stride)), cl3(want)
        assert close(M.epilogue(acc, alpha, beta, True), want, 1e-11)
    # up + lat(x): F.interpolate(top, scale_factor=2, bilinear) + conv1x1 with bias; odd and even extents, one row
    for b, h, w in ((2, 6, 10), (1, 7, 9), (3, 2, 2), (1, 1, 4)):
        top, lat, x = torch.randn(b, 4, max(h // 2, 1), max(w // 2, 1)).double(), nn.Conv2d(5, 4, 1, bias=True).double(), torch.randn(b, 5, h, w).double()
        if h % 2 or w % 2 or h < 2:
            # odd extents, one row: torch's own rule (source = (o + 0.5) / 2 - 0.5 clamped at 0, the second tap clamped to the last row /
            # column of the [h / 2, w / 2] map) written out pixel by pixel in float64
            up, t = M.bilinear_up2(cl2(top), h, w, np.float64), cl2(top)
            hh, wh = t.shape[1:3]
            for oy in range(h):
                sy = max((oy + 0.5) * 0.5 - 0.5, 0.0)
                y0 = min(int(sy), hh - 1)
                y1, fy = min(y0 + 1, hh - 1), sy - int(sy)
                for ox in range(w):
                    sx = max((ox + 0.5) * 0.5 - 0.5, 0.0)
                    x0 = min(int(sx), wh - 1)
                    x1, fx = min(x0 + 1, wh - 1), sx - int(sx)
                    want = (1 - fy) * ((1 - fx) * t[:, y0, x0] + fx * t[:, y0, x1]) + fy * ((1 - fx) * t[:, y1, x0] + fx * t[:, y1, x1])
                    assert close(up[:, oy, ox], want), (h, w, oy, ox)
            continue
        with torch.no_grad():
            want = F.interpolate(top, scale_factor=2, mode="bilinear", align_corners=False) + lat(x)
        got = M.heads_ref(cl2(x), [(lat.weight.detach().numpy(), lat.bias.detach().numpy())], [cl2(top)])[0][0]
        assert close(got, cl2(want), 1e-11)
    # Res block and the refinement tail and head
    res, ref = Res(8).double(), RefineNet2().double()
    x = torch.randn(3, 8, 5, 7).double()
    with torch.no_grad():
        want_res = res(x)
        want_tail = ref.conv2(x)
    got, _, _ = M.res_pair_ref(cl2(x), res.conv[0].weight.detach().numpy(), res.conv[2].weight.detach().numpy(), 0.1)
    assert close(got, cl2(want_res), 1e-6)                      # (the mirror takes the kernel's fp32 0.1)
    got, _, _ = M.res_pair_ref(cl2(x), res.conv[0].weight.detach().numpy(), res.conv[2].weight.detach().numpy(), 0.5)
    with torch.no_grad():
        assert close(got, cl2(x + 0.5 * res.conv(x)))
    lo, span = np.array([1.0, 2.0, 3.0]), np.array([0.5, 2.0, 4.0])
    got, _, _ = M.refine_tail_ref(cl2(x), ref.conv2[0].weight.detach().numpy(), ref.conv2[2].weight.detach().numpy(), lo, span)
    assert close(got, (T64(lo).view(3, 1, 1, 1) + want_tail * T64(span).view(3, 1, 1, 1)).squeeze(1).numpy())
    # the shuffled store is PixelShuffle(2) of the layer whose rows ops.shuffle2_rows reordered
    w1 = ref.conv2[0].weight.detach()
    conv_rows = M.conv2d_ref(cl2(x), ops.shuffle2_rows(w1).numpy())[0]
    with torch.no_grad():
        assert close(M.shuffle2_store(conv_rows), cl2(F.pixel_shuffle(F.conv2d(x, w1, None, 1, 1), 2)))
    depth = torch.randn(3, 5, 7).double()
    with torch.no_grad():
        want = ref.conv0((depth.unsqueeze(1) - T64(lo).view(3, 1, 1, 1)) / T64(span).view(3, 1, 1, 1))
    assert close(M.refine_head_ref(depth.numpy(), lo, span, ref.conv0.weight.detach().numpy())[0], cl2(want))
    # the pair of the feature pyramid: conv01 of FPN_4Scales
    c1, c2 = ConvBNReLU(3, 8, 3, 1).double().eval(), ConvBNReLU(8, 8, 3, 1).double().eval()
    img = torch.randn(2, 3, 6, 7).double()
    fold = lambda m: ((m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)).detach().numpy(),
                      (m.bn.bias - m.bn.running_mean * m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)).detach().numpy())
    for m in (c1, c2):
        m.bn.running_mean.normal_(), m.bn.running_var.uniform_(0.5, 2)
    with torch.no_grad():
        want = F.relu(c2.bn(c2.conv(F.relu(c1.bn(c1.conv(img))))))
    got = M.pair_planar_ref(img.numpy(), c1.conv.weight.detach().numpy(), *fold(c1), c2.conv.weight.detach().numpy(), *fold(c2))[0]
    assert close(got, cl2(want), 1e-11)


# ---------------------------------------------------------------------------------------------------------------- exactness
def _k_of(family, key):
    """(taps * cin of the deepest sum, Winograd (kd * cin) or 0, |x| bound of that sum's input) of a table case."""
    if family == "lds":
        _, kind, args, _ = key
        if kind == "3d":
            return 27 * args[0], 3 * args[0], 4
        cin, _, k, s = args[:4]
        return k * k * cin, (cin if k == 3 else 4 * cin), 4              # k5 s2 as a 3x3 layer over the four parity images
    if family == "digest":
        fn, args = key
        if fn == "lds2d_digests":
            return args[2] * args[2] * args[0], 4 * args[0], 4
        if fn == "tr_digests":
            import test_conv3d_digests_gpu as T
            return 27 * T.TR_ROUTES[args[0]][0], 0, 4
        return 27 * args[0], 3 * args[0], 4
    if family in ("hw", "strip"):
        return 27 * key[0], 3 * key[0], 4
    if family == "pair":
        return 72, 0, 2 * 4 * 27 + 2                                      # the second layer reads relu(alpha * conv + beta), |alpha| <= 2, |beta| <= 2
    if family in ("res_pair", "refine_tail"):
        return 72, 0, 4 * 72
    if family == "refine_head":
        return 9, 0, 4
    return 32, 0, 4                                                       # heads: 1x1 over 32 channels


def test_exactness_condition_holds_for_every_case_of_the_table():
    """Bounds from the generator's ranges alone: A <= xmax * 1 * K, A_w <= (9/4) * 4 xmax * (kd cin); the epilogue multiplies by at
    most 2 and adds at most 2 + 4 + 4 (beta, up, res); the unit is 2^-6.  Holds at the three scales (2^-130: the unit is then 2^-136)."""
    for name, (family, key) in M.table().items():
        k, kw, xmax = _k_of(family, key)
        a, a_w = float(xmax * k), 2.25 * 4 * xmax * kw
        for scale in (1.0, 2.0 ** 100, 2.0 ** -130):
            assert M.exact_condition(2 * max(a, a_w) + 10, unit=2.0 ** -6, scale=scale), name
        assert 2.0 ** 100 * (2 * max(a, a_w) + 10) * 4 * 72 < 2.0 ** 127, name      # no overflow, through a fused second layer too


LAYERS3D = [(8, 8), (16, 8), (16, 16), (32, 16), (32, 32), (16, 32), (8, 16), (64, 64)]
LAYERS2D = [(3, 8), (8, 8), (16, 16), (32, 32), (64, 64), (16, 32), (32, 64)]


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 100, 2.0 ** -130])
@pytest.mark.parametrize("cin,cout,kd", [(ci, co, 3) for ci, co in LAYERS3D] + [(ci, co, 1) for ci, co in LAYERS2D])
def test_exact_operands_make_every_order_exact(cin, cout, kd, scale):
    """The measured A and A_w stay below the analytic bounds, y64 is an fp32 tensor, and the serial fp32 chain, the fp32 Winograd
    restatement and both epilogues give it bit for bit."""
    shape = (2, 3, 7, 9) if kd == 3 else (2, 1, 9, 13)
    o = M.exact_operands(M.rng(cin, cout, kd), shape + (cin,), (cout, cin, kd, 3, 3), scale=scale)
    y64, a = M.conv_ref(o["x"], o["w"])
    assert a.max() <= scale * 4 * 9 * kd * cin and M.wino_bounds(o["x"], o["w"]) <= scale * 2.25 * 16 * kd * cin
    assert M.exact_condition(a.max() / scale, M.wino_bounds(o["x"], o["w"]) / scale, scale=scale) and M.is_f32(y64)
    assert abs(float((o["x"] == 0).mean()) - 0.30) < 0.06
    c, wg = M.chain32(o["x"], o["w"]), M.wino32(o["x"], o["w"])
    assert np.array_equal(c.astype(np.float64), y64) and np.array_equal(wg.astype(np.float64), y64)
    for kw in (dict(relu=True, res=o["res"]), dict(relu=True, res=o["res"], res_scale=o["res_scale"]), dict(relu=False)):
        e64 = M.epilogue(y64, o["alpha"], o["beta"], dtype=np.float64, **kw)
        e32 = M.epilogue(wg, o["alpha"], o["beta"], dtype=np.float32, **kw)
        assert M.is_f32(e64) and np.array_equal(e32.astype(np.float64), e64)
    if kd == 1:
        e64 = M.epilogue(y64[:, 0], o["alpha"], o["beta"], res_up=o["res_up"], dtype=np.float64)
        e32 = M.epilogue(wg[:, 0], o["alpha"], o["beta"], res_up=o["res_up"], dtype=np.float32)
        assert np.array_equal(e32.astype(np.float64), e64)


def test_exact_operands_of_the_other_modes_and_the_fused_pairs():
    for stride, tr in ((2, False), ((1, 2, 2), False), (2, True), ((1, 2, 2), True)):
        o = M.exact_operands(M.rng(7, tr), (2, 3, 7, 9, 16), (16, 8, 3, 3, 3) if tr else (8, 16, 3, 3, 3), stride, tr)
        y64, _ = M.conv_ref(o["x"], o["w"], stride, tr)
        assert np.array_equal(M.chain32(o["x"], o["w"], stride, tr).astype(np.float64), y64)
    rs = M.rng(11)
    o1 = M.exact_operands(rs, (2, 1, 13, 37, 3), (8, 3, 1, 3, 3))
    o2 = M.exact_operands(rs, (2, 1, 13, 37, 8), (8, 8, 1, 3, 3))
    xp = np.ascontiguousarray(o1["x"][:, 0].transpose(0, 3, 1, 2))
    args = (xp, o1["w"][:, :, 0], o1["alpha"], o1["beta"], o2["w"][:, :, 0], o2["alpha"], o2["beta"])
    y64, a, amid = M.pair_planar_ref(*args)
    assert M.exact_condition(max(a.max(), amid.max())) and np.array_equal(M.pair_planar_ref(*args, dtype=np.float32)[0].astype(np.float64), y64)
    y64, a, amid = M.res_pair_ref(o2["x"][:, 0], o2["w"][:, :, 0], o2["w"][::-1, :, 0], 0.5)
    assert M.exact_condition(max(a.max(), amid.max()))
    assert np.array_equal(M.res_pair_ref(o2["x"][:, 0], o2["w"][:, :, 0], o2["w"][::-1, :, 0], 0.5, dtype=np.float32)[0].astype(np.float64), y64)


# ---------------------------------------------------------------------------------------------------------------- the bar
RANDOM_LAYERS = [(16, 16, 3, (2, 3, 7, 9)), (32, 32, 3, (2, 5, 6, 11)), (64, 64, 1, (2, 1, 9, 13)), (16, 32, 1, (2, 1, 19, 33))]


def _errors(o, acc32, y64, a, **fault):
    """The three metrics of raw and of the epilogue (ReLU, residual, res_scale) against float64."""
    kw = dict(relu=True, res=o["res"], res_scale=o["res_scale"])
    e64 = M.epilogue(y64, o["alpha"], o["beta"], **kw)
    ae = M.epilogue_scale(a, o["alpha"], o["beta"], o["res"], o["res_scale"])
    return M.metrics(acc32, y64, a), M.metrics(M.epilogue(acc32, o["alpha"], o["beta"], dtype=np.float32, **kw, **fault), e64, ae)


@pytest.mark.parametrize("cls", M.CLASSES)
@pytest.mark.parametrize("cin,cout,kd,shape", RANDOM_LAYERS)
def test_a_correct_fp32_winograd_meets_the_random_bar(cin, cout, kd, shape, cls):
    o = M.random_operands(M.rng(cin, cout, kd, M.CLASSES.index(cls)), cls, shape + (cin,), (cout, cin, kd, 3, 3))
    y64, a = M.conv_ref(o["x"], o["w"])
    c_raw, c_epi = _errors(o, M.chain32(o["x"], o["w"]), y64, a)
    w_raw, w_epi = _errors(o, M.wino32(o["x"], o["w"]), y64, a)
    for what, got, yard in (("raw", w_raw, c_raw), ("epi", w_epi, c_epi)):
        r = M.bar_ratios(got, yard)
        print(f"{cin}->{cout} kd{kd} {cls} {what}: e_32 perA {yard['perA'] / M.U:.2f} u, Winograd / (1.5 e_32) " + " ".join(f"{k} {v:.2f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, (what, r)
        assert 0.25 * M.U < yard["perA"] < 8 * M.U           # the yardstick is a few u of A


def _spliced_last_column(o, faulty):
    good = M.wino32(o["x"], o["w"])
    good[:, :, :, -1] = faulty[:, :, :, -1]
    return good


def _restatement_with(fault, o):
    """(accumulator, epilogue fault) of the Winograd restatement with one deliberate error."""
    x, w = o["x"], o["w"]
    if fault == "tap dropped in the last column":
        w0 = w.copy()
        w0[:, :, -1, 1, 0] = 0
        return _spliced_last_column(o, M.wino32(x, w0)), {}
    if fault == "right halo reads the next row":
        return M.wino32(x, w, faults=("right_halo",)), {}
    if fault == "depth halo reads the next batch item":
        return M.wino32(x, w, faults=("depth_halo",)), {}
    if fault == "G entry off by 2^-20":
        g = M.G.copy()
        g[1, 1] = np.float32(0.5 * (1 + 2.0 ** -20))
        return M.wino32(x, w, g), {}
    if fault == "res_scale on res":
        return M.wino32(x, w), {"scale_res_instead": True}
    return M.wino32(x, w), {}


FAULTS = ["tap dropped in the last column", "right halo reads the next row", "depth halo reads the next batch item", "alpha and beta swapped",
          "res_scale on res", "G entry off by 2^-20"]


@pytest.mark.parametrize("fault", FAULTS)
def test_the_bars_catch_a_deliberate_error(fault):
    """On the ragged batch-2 case, 16 -> 16 3-D: the random bar (every class) and the exact bar must both break; the exact bar may
    miss the 2^-20 error of G (its products stay below the fp32 grid of the exact sums or round away), the random bar must not."""
    cin, cout, shape = 16, 16, (2, 3, 7, 9)

    def swapped(o):
        if fault == "alpha and beta swapped":
            o = dict(o)
            al, be = o["alpha"].copy(), o["beta"].copy()
            al[3], be[3] = o["beta"][3], o["alpha"][3]
            o["alpha"], o["beta"] = al, be
        return o
    for cls in M.CLASSES:
        o = M.random_operands(M.rng(cin, cout, 3, M.CLASSES.index(cls)), cls, shape + (cin,), (cout, cin, 3, 3, 3))
        y64, a = M.conv_ref(o["x"], o["w"])
        _, yard = _errors(o, M.chain32(o["x"], o["w"]), y64, a)
        acc, epi_fault = _restatement_with(fault, o)
        got_ref = M.epilogue(y64, o["alpha"], o["beta"], relu=True, res=o["res"], res_scale=o["res_scale"])
        wrong = M.epilogue(acc, swapped(o)["alpha"], swapped(o)["beta"], relu=True, res=o["res"], res_scale=o["res_scale"], dtype=np.float32, **epi_fault)
        got = M.metrics(wrong, got_ref, M.epilogue_scale(a, o["alpha"], o["beta"], o["res"], o["res_scale"]))
        assert max(M.bar_ratios(got, yard).values()) > 1.0, (cls, M.bar_ratios(got, yard))
    o = M.exact_operands(M.rng(cin, cout, 99), shape + (cin,), (cout, cin, 3, 3, 3))
    y64, _ = M.conv_ref(o["x"], o["w"])
    acc, epi_fault = _restatement_with(fault, o)
    so = swapped(o)
    wrong = M.epilogue(acc, so["alpha"], so["beta"], relu=True, res=o["res"], res_scale=o["res_scale"], dtype=np.float32, **epi_fault)
    right = M.epilogue(y64, o["alpha"], o["beta"], relu=True, res=o["res"], res_scale=o["res_scale"])
    if fault != "G entry off by 2^-20":
        assert not np.array_equal(wrong.astype(np.float64), right)


def test_a_fused_multiply_add_in_the_epilogue_changes_bits():
    """acc * alpha + beta as one fma stays inside any error bar; the bit-exact epilogue check of the GPU suite (the mirror's fp32
    epilogue applied to the kernel's own raw output) is what catches it."""
    o = M.random_operands(M.rng(5), "normal", (2, 3, 7, 9, 16), (16, 16, 3, 3, 3))
    raw = M.chain32(o["x"], o["w"])
    two = M.epilogue(raw, o["alpha"], o["beta"], True, dtype=np.float32)
    one = M.epilogue(raw, o["alpha"], o["beta"], True, dtype=np.float32, fuse_mul_add=True)
    assert not np.array_equal(one, two) and np.abs(one.astype(np.float64) - two).max() <= 2 * M.U * np.abs(two).max()


# ---------------------------------------------------------------------------------------------------------------- reach
def test_the_table_reaches_every_row_and_every_case_of_the_digest_suites():
    import test_conv3d_digests_gpu as T
    import test_conv_lds_routes_gpu as R
    tab = M.table()
    with open(R.GOLDEN) as f:
        golden = json.load(f)["settings"]
    seen = set()
    for setting in R.SETTINGS:
        names = {f"lds {setting}: {c[0]}" for c in R.cases(setting)}
        assert names <= set(tab)
        for c in R.cases(setting):
            seen |= {l.split(" grid ")[0] for l in golden[setting][c[0]]["lds"]}
    assert seen == R.EXPECTED_KERNELS and len(R.EXPECTED_KERNELS) == sum(3 if st else 1 for _, st in R.ROWS)
    assert {f"digest {n}" for n in T.CASES} <= set(tab)
    fams = {f for f, _ in tab.values()}
    assert fams == {"lds", "digest", "hw", "strip", "pair", "res_pair", "refine_tail", "refine_head", "heads"}
