"""CPU: the float64 references of tests/stream_mirror.py against independent formulations, the preconditions of the exact generator for
every table case, and the tables' reach over the launch branches.  No GPU."""
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

import stream_mirror as M  # noqa: E402

SMALL_BN = [c for c in M.BN_CASES if c[0] * c[1] * c[2] <= 1 << 17]


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------------- BatchNorm + ReLU
@pytest.mark.parametrize("case", [c for c in SMALL_BN if c[0] > 1], ids=M.bn_id)
@pytest.mark.parametrize("mode", ["momentum", "cumulative", "untracked"])
def test_bn_mirrors_equal_batchnorm3d_relu_autograd(case, mode):
    """finalize + apply + backward-reduce + backward against nn.BatchNorm3d(train).double() -> ReLU (+ residual), one module call per
    group in order (running statistics, num_batches_tracked) and the parameter gradients summed over the calls."""
    n, c, groups, _, has_res, _ = case
    y, dz, res, gamma, beta = M.bn_randn_inputs(case)
    bn = nn.BatchNorm3d(c, eps=float(np.float32(M.BN_EPS)), momentum=None if mode == "cumulative" else float(np.float32(M.BN_MOMENTUM)),
                        track_running_stats=mode != "untracked").double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        if mode != "untracked":
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
            bn.num_batches_tracked.fill_(3)
    running = None if mode == "untracked" else (bn.running_mean.clone(), bn.running_var.clone())
    aux, _, run, _, nbt = M.bn_finalize_ref(M.bn_stats_ref(y), gamma, beta, M.BN_EPS, n, None if mode == "cumulative" else M.BN_MOMENTUM,
                                            running, 3)
    yr = y.clone().requires_grad_(True)
    zs = []
    for g in range(groups):
        z = F.relu(bn(yr[g].t().reshape(1, c, n, 1, 1))).reshape(c, n).t()
        zs.append(z if res is None else z + res[g])
    zr = torch.stack(zs)
    zr.backward(dz)
    assert close(M.bn_apply_ref(y, aux, res), zr)
    if mode != "untracked":
        assert close(run[0], bn.running_mean) and close(run[1], bn.running_var)
        assert nbt == int(bn.num_batches_tracked) == 3 + groups
    dy, dgamma, dbeta, _ = M.bn_bwd_ref(dz, y, aux, M.bn_bwd_reduce_ref(dz, y, aux), gamma)
    assert close(dy, yr.grad, 1e-10) and close(dgamma, bn.weight.grad, 1e-10) and close(dbeta, bn.bias.grad, 1e-10)


def test_bn_one_voxel_per_group_has_zero_variance():
    case = M.BN_CASES[0]
    y, _, _, _, gamma, beta = M.bn_exact_inputs(case)
    aux, _, run, _, _ = M.bn_finalize_ref(M.bn_stats_ref(y), gamma, beta, M.BN_EPS, 1, M.BN_MOMENTUM, (torch.zeros(8), torch.ones(8)))
    assert torch.equal(aux[0, 2], y[0, 0]) and close(aux[0, 3], torch.full((8,), float(np.float32(M.BN_EPS)) ** -0.5, dtype=torch.float64))
    assert close(run[1], torch.full((8,), 1.0 - float(np.float32(0.1)), dtype=torch.float64))           # the biased variance (0) where N = 1


@pytest.mark.parametrize("case", M.BN_CASES, ids=M.bn_id)
def test_bn_exact_generator_preconditions(case):
    for name, bound, grid in M.bn_worst(case):
        assert M.fits32(bound, grid), (name, bound, grid)
    n, c, groups, nslices = case[:4]
    red = M.bn_handmade_red(case)
    q = red / n
    assert M.on_grid(q, 0.25) and float(q.abs().max()) <= 2 and bool((q == 0).any())
    inv_n = 1.0 / float(n)                                                       # the kernel's fp64 1/N and its fp32 (S * 1/N)
    assert np.array_equal((red.numpy() * inv_n).astype(np.float32).astype(np.float64), q.numpy())
    sl = M.spread_over_slices(red, nslices)
    assert torch.equal(sl.sum(0), red) and M.on_grid(sl, 0.25)
    if nslices > 1:
        later = sl[1:].flatten()
        nz = later[later != 0]
        assert bool((later == 0).any()) and nz.unique().numel() == nz.numel()
    tot = red.sum(0)
    assert torch.equal(tot.float().double(), tot)                                # dgamma, dbeta are fp32 values


@pytest.mark.parametrize("case", SMALL_BN, ids=M.bn_id)
def test_bn_exact_generator_data_is_on_its_grids(case):
    y, dz, res, aux, gamma, beta = M.bn_exact_inputs(case)
    n, c, groups = case[:3]
    assert float(y.abs().max()) <= M.Y_MAX and M.on_grid(y, 1.0) and M.on_grid(dz, 1.0)
    assert M.on_grid(aux[:, 0], 0.125) and M.on_grid(aux[:, 1], 0.125) and float(aux[:, 1].abs().max()) <= 21 and M.on_grid(aux[:, 2], 1.0) and M.on_grid(aux[:, 3], 0.25)
    pre = y * aux[:, 0:1] + aux[:, 1:2]
    assert bool((pre == 0).any()) or n < 16                         # the closed side of the ReLU decision is in the data
    if groups > 1:
        assert not torch.equal(y[0].mean(0).round(), y[1].mean(0).round())       # groups differ by their offsets
    for t, grid in ((M.bn_apply_ref(y, aux, res), 1 / 8), (M.bn_bwd_reduce_ref(dz, y, aux), 0.25)):
        assert M.on_grid(t, grid) and torch.equal(t.float().double(), t)
    dy, _, _, _ = M.bn_bwd_ref(dz, y, aux, M.bn_handmade_red(case), gamma)
    assert M.on_grid(dy, 1 / 256) and torch.equal(dy.float().double(), dy)


def test_bn_table_reaches_every_branch():
    cs = M.BN_CASES
    assert {c[1] for c in cs} == M.BN_CHANNELS and {c[2] for c in cs} >= M.BN_GROUPS and {c[3] for c in cs} == M.BN_SLICES
    assert {c[4] for c in cs} == {True, False} and {c[5] for c in cs} == {True, False}
    assert any(c[0] == 1 for c in cs) and any(c[0] % 2 == 1 and c[0] > 1 for c in cs)
    n4 = [M.bn_n4(c) for c in cs]
    assert any(v < 256 for v in n4) and any(v % 256 == 254 for v in n4) and any(v % 256 == 2 and v > 256 for v in n4)
    for rule, per_block in ((M.grid_for_reduce, 1024), (M.grid_for, 256)):
        for groups in (1, 40):
            mine = [c for c in cs if c[2] == groups]
            capped = [c for c in mine if -(-M.bn_n4(c) // per_block) > rule(M.bn_n4(c), groups)]
            assert capped and len(capped) < len(mine), (rule.__name__, groups)
    assert M.grid_for_reduce(10 ** 9, 1) == 512 and M.grid_for(10 ** 9, 1) == 2048
    assert M.grid_for_reduce(10 ** 9, 40) == 32 and M.grid_for(10 ** 9, 40) == 64
    assert M.grid_for_reduce(1, 1) == 1 and M.grid_for(257, 1) == 2 and M.grid_for_reduce(1025, 5) == 2
    assert any(M.bn_n4(c) > 524288 and c[2] == 1 for c in cs)
    big40 = [c for c in cs if c[2] == 40 and M.bn_n4(c) > 32 * 1024]
    assert big40 and all(M.per_thread(M.bn_n4(c), 32) > 4 for c in big40)


def test_variance_bound_has_room_for_the_summation_form():
    """The kernels' statistics: fp32 partials of m elements per thread (sum y, sum y^2), the rest in fp64.  Emulated here with
    sequential fp32 partials of m = 12 elements; the relative error of the variance stays under (m+1) 2^-24 (1 + (mean/std)^2)."""
    g = torch.Generator().manual_seed(5)
    m, parts = 12, 4096
    for ratio in (0.0, 3.0, 30.0):
        y = (torch.randn(parts, m, generator=g) * 2 + 2 * ratio).float()
        s1, s2 = torch.zeros(parts), torch.zeros(parts)
        for k in range(m):
            s1 = s1 + y[:, k]
            s2 = torch.from_numpy(np.float32(y[:, k].double().numpy() * y[:, k].double().numpy() + s2.double().numpy()))     # fmaf
        n = parts * m
        mean = s1.double().sum() / n
        var = s2.double().sum() / n - mean * mean
        ref = y.double().var(unbiased=False)
        assert abs(float(var - ref)) / float(ref) <= (m + 1) * M.U * (1 + ratio ** 2), ratio


# ---------------------------------------------------------------------------------------------------------------- softmax / regress backward
@pytest.mark.parametrize("case", [c for c in M.SOFTMAX_CASES if c[0] * c[2] * c[3] < 4096], ids=M.softmax_id)
def test_softmax_mirror_equals_autograd(case):
    B, D, h, w, pp = case
    g = M._gen(11, *case)
    logit = torch.randn(B, D, h, w, generator=g).double().requires_grad_(True)
    _, hyp, dd, dp = M.softmax_randn_inputs(case)
    prob = F.softmax(logit, 1)
    depth = torch.sum(prob * hyp, 1)
    for form, (use_dd, use_dp) in zip(M.SOFTMAX_FORMS, ((True, True), (True, False), (False, True), (False, True))):
        logit.grad = None
        ((depth * dd).sum() * float(use_dd) + (prob * dp).sum() * float(use_dp)).backward(retain_graph=True)
        ref = M.softmax_regress_bwd_ref(prob.detach(), None if form == "dprob-nohypos" else hyp, dd if use_dd else None, dp if use_dp else None)
        assert close(ref, logit.grad, 1e-9), form


@pytest.mark.parametrize("case", M.SOFTMAX_CASES, ids=M.softmax_id)
def test_softmax_exact_generator_preconditions(case):
    for name, bound, grid in M.softmax_worst():
        assert M.fits32(bound, grid), name
    if case[0] * case[2] * case[3] * case[1] > 1 << 20:
        return
    prob, hyp, dd, dp = M.softmax_exact_inputs(case)
    assert M.on_grid(prob, 1 / 16) and bool((prob.sum(1) == 1.0).all())
    assert M.on_grid(hyp, 1.0) and 400 <= float(hyp.min()) and float(hyp.max()) <= 1000
    assert M.on_grid(dd, 1.0) and M.on_grid(dp, 1 / 8) and float(dp.abs().max()) <= 2
    # the kernel's formula in fp32, operation by operation, equals it in float64
    m = (prob * hyp).sum(1, keepdim=True)
    c = (prob * (hyp - m)).sum(1, keepdim=True)
    mp = (prob * dp).sum(1, keepdim=True)
    gg = dd.unsqueeze(1) * ((hyp - m) - c) + (dp - mp)
    for t in (m, c, mp, gg, prob * gg):
        assert torch.equal(t.float().double(), t)
    assert torch.equal(prob * gg, M.softmax_regress_bwd_ref(prob, hyp, dd, dp))


def test_softmax_table_reaches_every_split():
    cs = M.SOFTMAX_CASES
    assert {M.softmax_split(*c[:4]) for c in cs} == {1, 2, 4, 8}
    assert {c[1] for c in cs} == M.SOFTMAX_D and {c[4] for c in cs} == {0, 1}
    cut = {(M.softmax_split(*c[:4]), M.split_cut_by(*c[:4])) for c in cs}
    assert (2, "planes") in cut and (4, "planes") in cut and (4, "pixels") in cut and (1, "pixels") in cut and (1, "planes") in cut
    assert any(c[1] % M.softmax_split(*c[:4]) for c in cs)
    assert any(c[0] > 1 and c[4] == 0 for c in cs) and any(c[0] > 1 and c[4] == 1 for c in cs)
    px = [(c[0] * c[2] * c[3], 256 // M.softmax_split(*c[:4])) for c in cs]
    assert any(n == 1 for n, _ in px) and any(n >= 262144 and n % 256 for n, _ in px)
    for S in (2, 4, 8):
        mine = [n % ppb for n, ppb in px if ppb == 256 // S]
        assert (256 // S - 1) in mine and 1 in mine, S


# ---------------------------------------------------------------------------------------------------------------- prob conv dgrad
@pytest.mark.parametrize("case", [c for c in M.DGRAD_CASES if M.dgrad_voxels(c) < 1 << 16], ids=M.dgrad_id)
def test_dgrad_mirror_equals_conv3d_autograd(case):
    B, D, H, W, C, _ = case
    dlogit, w, y, aux = M.dgrad_randn_inputs(case)
    x = torch.zeros(B, C, D, H, W, dtype=torch.float64, requires_grad=True)
    F.conv3d(x, w, padding=1).backward(dlogit.unsqueeze(1))
    dx = M.prob_conv_dgrad_ref(dlogit, w)
    assert close(dx, x.grad.permute(0, 2, 3, 4, 1))
    dr = torch.where(y * aux[0] + aux[1] > 0, dx.reshape(-1, C), torch.zeros(1, dtype=torch.float64))
    assert close(M.dgrad_stat_ref(dx, y, aux), torch.cat([dr.sum(0), (dr * (y - aux[2]) * aux[3]).sum(0)]))


@pytest.mark.parametrize("case", M.DGRAD_CASES, ids=M.dgrad_id)
def test_dgrad_exact_generator_preconditions(case):
    for name, bound, grid in M.dgrad_worst(case):
        assert M.fits32(bound, grid), name
    n = M.dgrad_voxels(case)
    assert n < 2 ** 31
    if n < 1 << 16:
        dlogit, w, y, aux = M.dgrad_exact_inputs(case)
        dx = M.prob_conv_dgrad_ref(dlogit, w)
        assert M.on_grid(dx, 1.0) and float(dx.abs().max()) <= 243 and M.on_grid(M.dgrad_stat_ref(dx, y, aux), 0.25)


def test_dgrad_table_reaches_every_branch():
    cs = M.DGRAD_CASES
    assert {c[4] for c in cs} == {8, 16} and {c[5] for c in cs} == M.DGRAD_SLICES
    assert any(-(-M.dgrad_voxels(c) // 256) > 4096 for c in cs) and any(M.dgrad_voxels(c) == 1 for c in cs)
    assert M.grid_4096(M.dgrad_voxels(cs[-1])) == 4096 and M.per_thread(M.dgrad_voxels(cs[-1]), 4096) == 2


# ---------------------------------------------------------------------------------------------------------------- upsample adjoint
@pytest.mark.parametrize("case", M.UP_CASES[:-1], ids=M.up_id)
def test_upsample_mirror_equals_interpolate_autograd(case):
    B, h, w, C = case
    dfine, before = M.up_exact_inputs(case)
    x = torch.zeros(B, C, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False).backward(dfine.permute(0, 3, 1, 2))
    ref = M.upsample2_bwd_ref(dfine)
    assert torch.equal(ref, x.grad.permute(0, 2, 3, 1))                          # integer cotangents, taps on 1/16: exact in float64
    assert M.on_grid(ref, 1 / 16) and float(ref.abs().max()) <= 12
    assert torch.equal(M.upsample2_bwd_ref(dfine, before), ref + before)
    assert torch.equal((ref + before).float().double(), ref + before)


def test_upsample_table_reaches_every_branch():
    cs = M.UP_CASES
    assert any(c[1] == 1 and c[2] == 1 for c in cs) and any(c[1] == 1 and c[2] > 1 for c in cs) and any(c[2] == 1 and c[1] > 1 for c in cs)
    assert any(c[1] == 2 for c in cs) and any(c[0] > 1 for c in cs)
    assert any(-(-M.up_float4(c) // 256) > 4096 for c in cs) and any(M.up_float4(c) < 256 for c in cs)
    assert M.fits32(12.0 + 50, 1 / 16)


# ---------------------------------------------------------------------------------------------------------------- loss
def _net_loss(pairs, fl):
    from net import loss as loss_mod
    ests = [e.clone().requires_grad_(True) for e, _ in pairs]
    rng = torch.stack([fl, fl + 500], 1)
    out = loss_mod.Loss()({"depth": [e.view(e.shape[0], 1, -1) for e in ests]}, {i: g.view(g.shape[0], 1, -1) for i, (_, g) in enumerate(pairs)}, rng)
    out.backward()
    return out.detach(), [e.grad for e in ests]


@pytest.mark.parametrize("case", M.LOSS_CASES, ids=M.loss_id)
@pytest.mark.parametrize("gen", ["exact", "randn"])
def test_loss_mirror_equals_net_loss(case, gen):
    """The mirror's route (reduce -> finalize -> backward) against net/loss.py on the CPU, float64 -- value, gradients, the valid mask,
    and a scale without a valid pixel (NaN loss, zero gradient there, the other scales' gradients untouched)."""
    ns, B, form, _, empty, dloss = case
    pairs = M.loss_exact_inputs(case) if gen == "exact" else M.loss_randn_inputs(case)
    _, fl = M.loss_floor(case)
    ref, grads = _net_loss([(e.double(), g.double()) for e, g in pairs], fl)
    acc = [v for e, g in pairs for v in M.loss_reduce_ref(e, g, fl)]
    acc64 = [v for e, g in pairs for v in M.loss_reduce_f64(e, g, fl)]
    loss, inv = M.loss_finalize_ref(acc)
    counts = acc[1::2]
    assert counts == acc64[1::2]
    if gen == "exact":
        assert acc == acc64                                                      # every fp32 per-pixel value is the float64 one
        assert (empty is not None) == bool(np.isnan(loss)) == bool(torch.isnan(ref))
    if not np.isnan(loss):
        assert abs(float(loss) - float(ref)) <= 4 * ns * M.U * abs(float(ref))
    for s, (e, g) in enumerate(pairs):
        de = M.loss_bwd_ref(e, g, fl, dloss, inv[s])
        assert torch.equal(de != 0, grads[s] != 0) or gen == "randn"
        if counts[s] == 0:
            assert s == empty and not bool(de.any()) and not bool(grads[s].any()) and np.isinf(inv[s])
        else:
            assert close(de, dloss * grads[s], 4 * M.U) and close(M.loss_bwd_f64(e, g, fl, dloss, counts[s]), dloss * grads[s])


@pytest.mark.parametrize("case", M.LOSS_CASES, ids=M.loss_id)
def test_loss_exact_generator_preconditions(case):
    """Every per-pixel value is a multiple of 2^-26 and their absolute sum stays below 2^26: any order of fp64 adds is exact."""
    _, fl = M.loss_floor(case)
    for e, g in M.loss_exact_inputs(case):
        d = e.double() - g.double()
        assert torch.equal((e - g).double(), d) and float(d.abs().max()) <= 4
        a = np.abs((e - g).numpy())
        v = np.where(a < 1, (np.float32(0.5) * (e - g).numpy()) * (e - g).numpy(), a - np.float32(0.5)).astype(np.float64)
        assert np.array_equal(np.round(v * 2.0 ** 26), v * 2.0 ** 26) and v.sum() < 2.0 ** 26
        regular = (d * 8 == torch.round(d * 8))
        assert int((~regular).sum()) <= 6 * e.shape[0]


def test_loss_table_reaches_every_branch():
    cs = M.LOSS_CASES
    assert {c[0] for c in cs} == {1, 4, 8} and {c[1] for c in cs} == {1, 3}
    assert {c[2] for c in cs} == set(M.LOSS_FLOORS) and any(c[2].endswith("stride2") for c in cs)
    assert any(c[3] is not None and 0 < c[3] < c[0] - 1 for c in cs) and any(c[4] is not None for c in cs) and any(c[5] != 1.0 for c in cs)
    px = M.LOSS_PIXELS
    assert px[0] > 262144 and M.grid_x(px[0]) == 256 and -(-px[0] // 1024) > 256 and {1, 255, 257, 72 * 96} <= set(px[:5]) and len(px) == 9
    assert M.grid_x(1) == 1 and M.grid_x(1025) == 2
    # the boundary values are in the data: the floor itself (invalid), the next fp32 (valid), |d| = 1 and one ulp either side
    case = next(c for c in cs if c[2] == "f32-0dim")
    _, fl = M.loss_floor(case)
    e, g = M.loss_exact_inputs(case)[0]
    d = (e - g).double()[0]
    for want in (1.0, -1.0, 1 + 2.0 ** -23, 1 - 2.0 ** -24, -(1 + 2.0 ** -23), -(1 - 2.0 ** -24)):
        assert bool((d == want).any()), want
    for c in cs:
        _, flc = M.loss_floor(c)
        e, g = M.loss_exact_inputs(c)[0]
        f32 = np.float32(flc[0].item())
        assert float(g[0, 0]) == float(f32) and not float(g[0, 0]) > float(flc[0])
        assert float(g[0, 1]) == float(np.nextafter(f32, np.float32(np.inf))) and float(g[0, 1]) > float(flc[0])
    assert any(abs(float(M.loss_floor(c)[1][-1]) - (300 + 1e-7)) < 1e-9 or M.LOSS_FLOORS[c[2]][1:2] == [300 + 1e-7] for c in cs)
