"""GPU parity of the training step's stream kernels (csrc/bn_train.hip, prob_bwd.hip, upsample_bwd.hip, the loss part of loss.hip) with
the float64 references of tests/stream_mirror.py, through the C ABI, at edge shapes, group / slice layouts and every launch-rule branch.

Exact generator: the kernels owe the reference BIT FOR BIT (torch.equal); the conditions are asserted in tests/test_stream_mirror_cpu.py.
Random generator: the bars the kernels' tests in tests/test_train_gpu.py hold; the worst value per entry is printed.  Where neither
applies (the finalize kernels, dy from sums the kernels reduced) the bar is the fp32 ulp bound derived in the mirror's docstring.

Every output is filled with NaN before the call, every reduction buffer is zeroed as the callers do and carries a NaN canary behind
its last slice, and accumulating outputs start from integers."""
import ctypes
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
from mdfnet_hip import check, lib, ops, train_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
EPS32, MOM32 = float(np.float32(M.BN_EPS)), float(np.float32(M.BN_MOMENTUM))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    check(getattr(lib(), name)(*args, _stream()), name)


def dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def zeroed_with_canary(n):
    """n zeroed doubles (as the callers hand them over) and two NaNs behind them."""
    buf = torch.zeros(n + 2, device=DEV, dtype=torch.float64)
    buf[n:] = NAN
    return buf


def with_canary(t):
    flat = t.reshape(-1).to(torch.float64)
    return torch.cat([flat, torch.full((2,), NAN, dtype=torch.float64)]).to(DEV)


def canary_intact(buf, n):
    return bool(buf[n:].isnan().all()) and not bool(buf[:n].isnan().any())


def exact(got, ref, what):
    """got (fp32 or fp64, device) equals the float64 reference bit for bit."""
    g = got.detach().cpu()
    assert g.dtype in (torch.float32, torch.float64)
    g = g.double().reshape(ref.shape)
    if not torch.equal(g, ref):
        bad = (g != ref).nonzero()
        first = ", ".join(f"{tuple(i.tolist())}: got {float(g[tuple(i)])} ref {float(ref[tuple(i)])}" for i in bad[:4])
        raise AssertionError(f"{what}: {len(bad)} of {ref.numel()} elements differ; {first}")


def within(got, ref, bound, what):
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    over = err > bound
    assert not bool(over.any()) and not bool(err.isnan().any()), f"{what}: {int(over.sum())} elements past the bound, worst {float((err / bound.clamp(min=1e-300)).max()):.3f} x"


_WORST = {}


def bar(name, got, ref, limit):
    e = M.rel_err(got, ref)
    _WORST[name] = max(_WORST.get(name, 0.0), e)
    print(f"{name}: {e:.3e} (worst so far {_WORST[name]:.3e}, bar {limit:g})")
    assert e < limit, (name, e)


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def test_mirror_constants_are_the_packages():
    assert ops.STAT_SLICES == M.STAT_SLICES


# ==================================================================================================================== BatchNorm + ReLU
def bn_exact(case):
    return cached(("bn", case), lambda: M.bn_exact_inputs(case))


def bn_call_stats(y, case):
    n, c, groups = case[:3]
    buf = zeroed_with_canary(groups * 2 * c)
    call("mdf_bn_stats_fwd", y.data_ptr(), n, c, groups, buf.data_ptr())
    return buf


def bn_call_reduce(dz, y, aux, case):
    n, c, groups = case[:3]
    buf = zeroed_with_canary(groups * 2 * c)
    call("mdf_bn_relu_bwd_reduce", dz.data_ptr(), y.data_ptr(), aux.data_ptr(), n, c, groups, buf.data_ptr())
    return buf


def bn_call_apply(y, aux, res, case):
    n, c, groups = case[:3]
    z = nans(groups, n, c)
    call("mdf_bn_relu_apply_fwd", y.data_ptr(), aux.data_ptr(), ptr(res), z.data_ptr(), n, c, groups)
    return z


def bn_call_bwd(dz, y, aux, red, gamma, case, nslices):
    n, c, groups = case[:3]
    dy, dgamma, dbeta = nans(groups, n, c), nans(c), nans(c)
    call("mdf_bn_relu_bwd", dz.data_ptr(), y.data_ptr(), aux.data_ptr(), red.data_ptr(), gamma.data_ptr(), n, c, groups, dy.data_ptr(),
         dgamma.data_ptr(), dbeta.data_ptr(), nslices)
    return dy, dgamma, dbeta


def bn_running(case):
    c = case[1]
    g = M._gen(21, *case[:4])
    return torch.randn(c, generator=g), torch.rand(c, generator=g) * 1.5 + 0.5


@pytest.mark.parametrize("case", M.BN_CASES, ids=M.bn_id)
def test_bn_reductions_and_apply_exact(case):
    n, c, groups = case[:3]
    y, dz, res, aux, _, _ = bn_exact(case)
    yd, dzd, auxd = dev(y), dev(dz), dev(aux)
    k = groups * 2 * c
    buf = bn_call_stats(yd, case)
    exact(buf[:k], M.bn_stats_ref(y), "mdf_bn_stats_fwd")
    assert canary_intact(buf, k)
    buf = bn_call_reduce(dzd, yd, auxd, case)
    exact(buf[:k], M.bn_bwd_reduce_ref(dz, y, aux), "mdf_bn_relu_bwd_reduce")
    assert canary_intact(buf, k)
    exact(bn_call_apply(yd, auxd, dev(res), case), M.bn_apply_ref(y, aux, res), "mdf_bn_relu_apply_fwd")
    if res is not None:
        exact(bn_call_apply(yd, auxd, None, case), M.bn_apply_ref(y, aux, None), "mdf_bn_relu_apply_fwd without residual")


@pytest.mark.parametrize("case", M.BN_CASES, ids=M.bn_id)
def test_bn_backward_exact_with_handmade_slices(case):
    """red = [slice][group][2C] hand-made: distinct entries, exact zeros, totals N q.  dy, dgamma, dbeta bit for bit."""
    n, c, groups, nslices = case[:4]
    y, dz, _, aux, gamma, _ = bn_exact(case)
    tot = M.bn_handmade_red(case)
    red = with_canary(M.spread_over_slices(tot, nslices))
    dy, dgamma, dbeta = bn_call_bwd(dev(dz), dev(y), dev(aux), red, dev(gamma), case, nslices)
    rdy, rdg, rdb, _ = M.bn_bwd_ref(dz, y, aux, tot, gamma)
    exact(dy, rdy, "dy")
    exact(dgamma, rdg, "dgamma")
    exact(dbeta, rdb, "dbeta")
    assert bool(red[nslices * groups * 2 * c:].isnan().all())


@pytest.mark.parametrize("case", [c for c in M.BN_CASES if c[3] == 1 or c[0] > 10000], ids=M.bn_id)
def test_bn_backward_from_reduced_sums_within_ulp_bound(case):
    """The sums as mdf_bn_relu_bwd_reduce left them (exact), N not a power of two: dy within the derived bound of float64."""
    n, c, groups = case[:3]
    y, dz, _, aux, gamma, _ = bn_exact(case)
    yd, dzd, auxd = dev(y), dev(dz), dev(aux)
    red = bn_call_reduce(dzd, yd, auxd, case)
    dy, dgamma, dbeta = bn_call_bwd(dzd, yd, auxd, red, dev(gamma), case, 1)
    tot = M.bn_bwd_reduce_ref(dz, y, aux)
    rdy, rdg, rdb, bound = M.bn_bwd_ref(dz, y, aux, tot, gamma)
    within(dy, rdy, bound, "dy")
    within(dgamma, rdg, M.U * M.SLACK * rdg.abs(), "dgamma")
    within(dbeta, rdb, M.U * M.SLACK * rdb.abs(), "dbeta")


def _finalize_inputs(case):
    n, c, groups, nslices, _, has_run = case
    y = bn_exact(case)[0]
    _, _, _, gamma, beta = M.bn_randn_inputs((4, c, 1, 1, False, False))
    tot = M.bn_stats_ref(y)
    sums = with_canary(M.spread_over_slices(tot, nslices, salt=3))
    run = bn_running(case) if has_run else None
    return y, gamma.float().double(), beta.float().double(), tot, sums, run


def _check_finalize(case, aux, rm, rv, nbt, gamma, beta, tot, run, what):
    n, c, groups = case[:3]
    raux, baux, rrun, brun, rnbt = M.bn_finalize_ref(tot, gamma, beta, M.BN_EPS, n, M.BN_MOMENTUM,
                                                     None if run is None else (run[0].double(), run[1].double()), 3)
    within(aux, raux, baux, what + " aux")
    if run is not None:
        within(rm, rrun[0], brun[0], what + " running_mean")
        within(rv, rrun[1], brun[1], what + " running_var")
        assert int(nbt) == rnbt == 3 + groups


@pytest.mark.parametrize("case", M.BN_CASES, ids=M.bn_id)
def test_bn_finalize_within_ulp_bound(case):
    n, c, groups, nslices, _, has_run = case
    _, gamma, beta, tot, sums, run = _finalize_inputs(case)
    aux = nans(groups, 4, c)
    rm, rv = (dev(run[0]), dev(run[1])) if run else (None, None)
    nbt = torch.full((), 3, device=DEV, dtype=torch.int64) if run else None
    gd, bd = dev(gamma), dev(beta)
    call("mdf_bn_finalize_fwd", sums.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS32, MOM32, n, c, groups, aux.data_ptr(), ptr(rm), ptr(rv), ptr(nbt),
         nslices)
    _check_finalize(case, aux, rm, rv, nbt, gamma, beta, tot, run, "mdf_bn_finalize_fwd")


@pytest.mark.parametrize("case", M.BN_CASES, ids=M.bn_id)
def test_bn_finalize_apply_aux_bound_and_z_exact(case):
    """Two assertions that together pin the fused entry: the aux it publishes is within the bound of float64, and z is, bit for bit,
    the apply formula with THAT aux (y an integer: y a is exact in float64, and the sum with b is checked to be, so one rounding to
    fp32 is the kernel's fmaf)."""
    n, c, groups, nslices, has_res, has_run = case
    y, gamma, beta, tot, sums, run = _finalize_inputs(case)
    res = bn_exact(case)[2]
    aux, z = nans(groups, 4, c), nans(groups, n, c)
    rm, rv = (dev(run[0]), dev(run[1])) if run else (None, None)
    nbt = torch.full((), 3, device=DEV, dtype=torch.int64) if run else None
    yd, gd, bd, rd = dev(y), dev(gamma), dev(beta), dev(res)
    call("mdf_bn_finalize_apply_fwd", yd.data_ptr(), sums.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS32, MOM32, ptr(rd), z.data_ptr(), aux.data_ptr(),
         ptr(rm), ptr(rv), ptr(nbt), n, c, groups, nslices)
    _check_finalize(case, aux, rm, rv, nbt, gamma, beta, tot, run, "mdf_bn_finalize_apply_fwd")
    a64 = aux.cpu().double()
    p, b = y * a64[:, 0:1], a64[:, 1:2].expand_as(y)
    s = p + b
    bb = s - p
    assert not bool(((p - (s - bb)) + (b - bb)).any()), "y a + b is not exact in float64 for this aux"
    pre = torch.clamp(s.float(), min=0.0).double()
    exact(z, pre if res is None else (pre + res).float().double(), "z of mdf_bn_finalize_apply_fwd")


@pytest.mark.parametrize("case", M.BN_CASES, ids=M.bn_id)
def test_bn_chain_randn_at_the_existing_bars(case):
    n, c, groups, _, has_res, _ = case
    y, dz, res, gamma, beta = cached(("bnr", case), lambda: M.bn_randn_inputs(case))
    yd, dzd, gd, bd = dev(y), dev(dz), dev(gamma), dev(beta)
    sums = bn_call_stats(yd, case)
    aux = nans(groups, 4, c)
    call("mdf_bn_finalize_fwd", sums.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS32, MOM32, n, c, groups, aux.data_ptr(), None, None, None, 1)
    z = bn_call_apply(yd, aux, dev(res), case)
    red = bn_call_reduce(dzd, yd, aux, case)
    dy, dgamma, dbeta = bn_call_bwd(dzd, yd, aux, red, gd, case, 1)
    y32, dz32 = y.float().double(), dz.float().double()
    g32, b32 = gamma.float().double(), beta.float().double()
    raux = M.bn_finalize_ref(M.bn_stats_ref(y32), g32, b32, M.BN_EPS, n)[0]
    bar("bn sums", sums[:-2].cpu(), M.bn_stats_ref(y32).reshape(-1), M.BN_BAR_FWD)
    if n > 1:
        # (N = 1: var = 0 and invstd = eps^-1/2 = 316, so z = b + y a cancels two numbers 316 x the size of y and carries 316 u of
        #  it -- a property of the formula in fp32, whichever code evaluates it.  The one-voxel cases are held by the exact pass and by
        #  the ulp bounds of the finalize tests instead.)
        bar("bn z", z, M.bn_apply_ref(y32, raux, None if res is None else res.float().double()), M.BN_BAR_FWD)
        rdy, rdg, rdb, _ = M.bn_bwd_ref(dz32, y32, raux, M.bn_bwd_reduce_ref(dz32, y32, raux), g32)
        bar("bn dy", dy, rdy, M.BN_BAR_BWD)
        bar("bn dgamma", dgamma, rdg, M.BN_BAR_BWD)
        bar("bn dbeta", dbeta, rdb, M.BN_BAR_BWD)


def test_bn_variance_of_offset_data_within_the_summation_bound():
    """Per-channel mean/std of 0, 3 and 30: the variance the kernel's sums give is within (m+1) 2^-24 (1 + (mean/std)^2) of float64,
    m the per-thread element count of the reduction grid."""
    case = (3001, 16, 1, 1, False, False)
    ratios = (0.0, 3.0, 30.0)
    y = M.bn_randn_inputs(case, ratios)[0].float()
    sums = bn_call_stats(dev(y), case)[:32].cpu()
    n, c = case[0], case[1]
    m = M.per_thread(M.bn_n4(case), M.grid_for_reduce(M.bn_n4(case), 1))
    mean = sums[:c] / n
    var = sums[c:] / n - mean * mean
    ref = y.double()[0].var(0, unbiased=False)
    rel = (var - ref).abs() / ref
    for ch in range(c):
        r = ratios[ch % 3]
        print(f"channel {ch} mean/std {r}: {float(rel[ch]):.3e}")
        assert float(rel[ch]) <= (m + 1) * M.U * (1 + r * r), (ch, r)


def test_bn_wrappers_with_groups_pool_and_given_sums():
    case = (513, 16, 5, 3, True, True)
    n, c, groups, nslices = case[:4]
    y, dz, res, aux, gamma, _ = bn_exact(case)
    yd, dzd, auxd = dev(y), dev(dz), dev(aux)
    pool = train_ops.ZeroPool(DEV, 4096)
    exact(train_ops.bn_stats(yd, n, c, groups, pool=pool), M.bn_stats_ref(y), "bn_stats(pool=)")
    exact(train_ops.bn_stats(yd, n, c, groups), M.bn_stats_ref(y), "bn_stats")
    exact(train_ops.bn_relu_apply(yd, auxd, dev(res), n, c, groups), M.bn_apply_ref(y, aux, res), "bn_relu_apply")
    tot = M.bn_handmade_red(case)
    rdy, rdg, rdb, _ = M.bn_bwd_ref(dz, y, aux, tot, gamma)
    red = dev(M.spread_over_slices(tot, nslices), torch.float64).reshape(-1)
    for got, ref, what in zip(train_ops.bn_relu_backward(dzd, yd, auxd, dev(gamma), n, c, groups, red=red), (rdy, rdg, rdb), ("dy", "dgamma", "dbeta")):
        exact(got, ref, f"bn_relu_backward(red=) {what}")
    tot = M.bn_bwd_reduce_ref(dz, y, aux)
    rdy, rdg, rdb, bound = M.bn_bwd_ref(dz, y, aux, tot, gamma)
    for kw in ({"pool": pool}, {}):
        dy, dg, db = train_ops.bn_relu_backward(dzd, yd, auxd, dev(gamma), n, c, groups, **kw)
        within(dy, rdy, bound, "bn_relu_backward dy")
        within(dg, rdg, M.U * M.SLACK * rdg.abs(), "dgamma")
        within(db, rdb, M.U * M.SLACK * rdb.abs(), "dbeta")
    for fused in (False, True):
        bn = nn.BatchNorm3d(c, eps=M.BN_EPS, momentum=M.BN_MOMENTUM)
        run = bn_running(case)
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
            bn.running_mean.copy_(run[0])
            bn.running_var.copy_(run[1])
            bn.num_batches_tracked.fill_(3)
        g64, b64 = bn.weight.detach().double(), bn.bias.detach().double()
        bn = bn.to(DEV)
        sums = dev(M.spread_over_slices(M.bn_stats_ref(y), nslices), torch.float64).reshape(-1)
        if fused:
            z, got = train_ops.bn_finalize_apply(sums, bn, yd, dev(res), n, c, groups)
            assert not bool(z.isnan().any())
        else:
            got = train_ops.bn_finalize(sums, bn, n, c, groups)
        _check_finalize(case, got.view(groups, 4, c), bn.running_mean, bn.running_var, bn.num_batches_tracked, g64, b64, M.bn_stats_ref(y), run,
                        "bn_finalize_apply" if fused else "bn_finalize")


# ==================================================================================================================== softmax / regress backward
def softmax_call(prob, hyp, pp, dd, dp, case):
    B, D, h, w, _ = case
    out = nans(B, D, h, w)
    call("mdf_prob_softmax_regress_bwd", prob.data_ptr(), ptr(hyp), pp, ptr(dd), ptr(dp), out.data_ptr(), B, D, h, w)
    return out


def test_softmax_split_query_and_the_tables_reach():
    L = lib()
    got = {c: L.mdf_prob_softmax_regress_bwd_split(*c[:4]) for c in M.SOFTMAX_CASES}
    assert all(got[c] == M.softmax_split(*c[:4]) for c in M.SOFTMAX_CASES), got
    assert set(got.values()) == {1, 2, 4, 8}
    cut = {(got[c], M.split_cut_by(*c[:4])) for c in M.SOFTMAX_CASES}
    assert any(why == "planes" and s in (2, 4) for s, why in cut) and any(why == "pixels" and s in (2, 4) for s, why in cut)
    assert any(c[1] % got[c] for c in M.SOFTMAX_CASES)
    for b, d, h, w in ((0, 8, 4, 4), (1, 0, 4, 4), (1, 8, 0, 4), (1, 8, 4, -1)):
        assert L.mdf_prob_softmax_regress_bwd_split(b, d, h, w) == -1 and b"bad shape" in L.mdf_last_error()


@pytest.mark.parametrize("case", M.SOFTMAX_CASES, ids=M.softmax_id)
@pytest.mark.parametrize("form", M.SOFTMAX_FORMS)
def test_softmax_regress_backward(case, form):
    """The four (ddepth, dprob) forms; 'dprob-nohypos' passes hypos = NULL, which the kernel must not touch without ddepth."""
    B, D, h, w, pp = case
    use_dd, use_dp, use_h = form.startswith("ddepth"), form.endswith("dprob") or form == "dprob-nohypos", form != "dprob-nohypos"
    for gen, inputs in (("exact", M.softmax_exact_inputs), ("randn", M.softmax_randn_inputs)):
        prob, hyp, dd, dp = cached(("sm", gen, case), lambda: inputs(case))
        hd = dev(hyp if pp else hyp.reshape(B, D)) if use_h else None
        got = softmax_call(dev(prob), hd, pp, dev(dd) if use_dd else None, dev(dp) if use_dp else None, case)
        p32, h32 = prob.float().double(), hyp.float().double()
        ref = M.softmax_regress_bwd_ref(p32, h32, dd.float().double() if use_dd else None, dp.float().double() if use_dp else None)
        if gen == "exact":
            exact(got, ref, f"dlogit ({form})")
        else:
            bar(f"softmax dlogit {form}", got, ref, M.PROB_BAR)


# ==================================================================================================================== prob conv dgrad
def dgrad_call(dlogit, w, case, stat=None):
    B, D, H, W, C, nslices = case
    dx = nans(B, D, H, W, C)
    if stat is None:
        call("mdf_prob_conv_dgrad", dlogit.data_ptr(), w.data_ptr(), dx.data_ptr(), B, D, H, W, C)
        return dx, None
    red = zeroed_with_canary(nslices * 2 * C)
    call("mdf_prob_conv_dgrad_stat", dlogit.data_ptr(), w.data_ptr(), dx.data_ptr(), B, D, H, W, C, stat[0].data_ptr(), stat[1].data_ptr(),
         red.data_ptr(), nslices)
    return dx, red


@pytest.mark.parametrize("case", M.DGRAD_CASES, ids=M.dgrad_id)
def test_prob_conv_dgrad_and_stat_epilogue(case):
    B, D, H, W, C, nslices = case
    k = nslices * 2 * C
    for gen, inputs in (("exact", M.dgrad_exact_inputs), ("randn", M.dgrad_randn_inputs)):
        dlogit, w, y, aux = inputs(case)
        dl, wd = dev(dlogit), dev(w)
        dx, _ = dgrad_call(dl, wd, case)
        dxs, red = dgrad_call(dl, wd, case, (dev(y), dev(aux)))
        assert torch.equal(dx, dxs), "dx differs with the stat epilogue"
        assert canary_intact(red, k)
        tot = red[:k].view(nslices, 2 * C).sum(0)
        ref = M.prob_conv_dgrad_ref(dlogit.float().double(), w.float().double())
        if gen == "exact":
            exact(dx, ref, "dx")
            exact(tot, M.dgrad_stat_ref(ref, y, aux), "sum over slices of (sum dr, sum dr xhat)")
            if M.grid_4096(M.dgrad_voxels(case)) >= nslices > 1:
                assert bool(red[:k].view(nslices, 2 * C).abs().sum(1).gt(0).all()), "a slice received nothing"
        else:
            bar("prob dgrad dx", dx, ref, M.PROB_BAR)
            # the sums of the kernel's OWN dx (the ReLU decisions and xhat are functions of y, aux alone)
            bar("prob dgrad sums", tot, M.dgrad_stat_ref(dx.cpu().double(), y.float().double(), aux.float().double()), M.PROB_BAR)


# ==================================================================================================================== upsample adjoint
@pytest.mark.parametrize("case", M.UP_CASES, ids=M.up_id)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_upsample_adjoint(case, accumulate):
    B, h, w, C = case
    for gen, inputs in (("exact", M.up_exact_inputs), ("randn", M.up_randn_inputs)):
        def make():
            dfine, before = inputs(case)
            f32, b32 = dfine.float().double(), before.float().double()
            return f32, b32, M.upsample2_bwd_ref(f32), None if gen == "exact" else M.upsample2_bwd_ref(f32.abs())
        f32, b32, ref, mag = cached(("up", gen, case), make)
        out = dev(b32) if accumulate else nans(B, h, w, C)          # accumulate = 0 must overwrite whatever the output held
        fine = dev(f32)
        call("mdf_upsample2_bilinear_bwd", fine.data_ptr(), out.data_ptr(), B, h, w, C, accumulate)
        if gen == "exact":
            exact(out, ref + b32 if accumulate else ref, "dcoarse")
        else:
            # 16 fmaf and one add, each one rounding of a partial sum bounded by the sum of magnitudes
            within(out, ref + b32 if accumulate else ref, 17 * M.U * M.SLACK * (mag + b32.abs()), "dcoarse (randn)")


def test_upsample_wrapper_with_and_without_dcoarse():
    case = (3, 7, 9, 32)
    dfine, before = M.up_exact_inputs(case)
    exact(train_ops.upsample2_backward(dev(dfine)), M.upsample2_bwd_ref(dfine), "upsample2_backward")
    acc = dev(before)
    out = train_ops.upsample2_backward(dev(dfine), acc)
    assert out.data_ptr() == acc.data_ptr()
    exact(out, M.upsample2_bwd_ref(dfine, before), "upsample2_backward(dcoarse=)")


# ==================================================================================================================== loss
def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def loss_run(case, pairs, route):
    """-> acc (2 ns doubles, cpu), loss, inv_count [ns], [de or None]; route 'multi' or 'single'."""
    ns, B, form, null, _, dloss = case
    ft, _ = M.loss_floor(case)
    fd = ft.to(DEV)
    f64, fstride = int(ft.dtype == torch.float64), (ft.stride(0) if ft.dim() else 0) * (2 if form.endswith("stride2") else 1)
    es, gs = [dev(e) for e, _ in pairs], [dev(g) for _, g in pairs]
    pb = [e.shape[1] for e, _ in pairs]
    acc = zeroed_with_canary(2 * ns)
    des = [None if s == null else nans(B, pb[s]) for s in range(ns)]
    dl = torch.tensor(dloss, device=DEV, dtype=torch.float32)
    loss, inv = nans(1), nans(ns)
    if route == "multi":
        ep, gp, pbs = _arr(ctypes.c_void_p, [e.data_ptr() for e in es]), _arr(ctypes.c_void_p, [g.data_ptr() for g in gs]), _arr(ctypes.c_int64, pb)
        call("mdf_masked_smooth_l1_reduce_multi", ep, gp, pbs, ns, fd.data_ptr(), f64, fstride, B, acc.data_ptr())
        call("mdf_masked_smooth_l1_finalize", acc.data_ptr(), ns, loss.data_ptr(), inv.data_ptr())
        dp = _arr(ctypes.c_void_p, [ptr(d) for d in des])
        call("mdf_masked_smooth_l1_bwd_multi", ep, gp, pbs, ns, fd.data_ptr(), f64, fstride, B, dl.data_ptr(), inv.data_ptr(), dp)
    else:
        for s in range(ns):
            call("mdf_masked_smooth_l1_reduce", es[s].data_ptr(), gs[s].data_ptr(), fd.data_ptr(), f64, fstride, B, pb[s], acc[2 * s:].data_ptr())
        call("mdf_masked_smooth_l1_finalize", acc.data_ptr(), ns, loss.data_ptr(), inv.data_ptr())
        for s in range(ns):
            if des[s] is not None:
                call("mdf_masked_smooth_l1_bwd", es[s].data_ptr(), gs[s].data_ptr(), fd.data_ptr(), f64, fstride, B, pb[s], dl.data_ptr(),
                     inv[s:].data_ptr(), des[s].data_ptr())
    torch.cuda.synchronize()
    assert bool(acc[2 * ns:].isnan().all())
    return acc[:2 * ns].cpu(), loss.cpu(), inv.cpu(), [None if d is None else d.cpu() for d in des]


def same_bits(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    assert a.dtype == b.dtype == torch.float32, (a.dtype, b.dtype)
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", M.LOSS_CASES, ids=M.loss_id)
def test_loss_exact_both_routes_equal_the_mirror(case):
    ns, B, form, null, empty, dloss = case
    pairs = M.loss_exact_inputs(case)
    _, fl = M.loss_floor(case)
    racc = torch.tensor([v for e, g in pairs for v in M.loss_reduce_ref(e, g, fl)], dtype=torch.float64)
    rloss, rinv = M.loss_finalize_ref(racc.numpy())
    assert bool(np.isnan(rloss)) == (empty is not None)
    multi, single = loss_run(case, pairs, "multi"), loss_run(case, pairs, "single")
    for name, (acc, loss, inv, des) in (("multi", multi), ("single", single)):
        assert torch.equal(acc, racc), (name, acc, racc)
        assert same_bits(inv, torch.from_numpy(rinv)), (name, inv, rinv)
        assert same_bits(loss, torch.tensor([float(rloss)], dtype=torch.float32)) or (np.isnan(rloss) and bool(loss.isnan().all())), (name, loss, rloss)
        for s, (e, g) in enumerate(pairs):
            if s == null:
                assert des[s] is None
                continue
            ref = M.loss_bwd_ref(e, g, fl, dloss, rinv[s])
            assert torch.equal(des[s], ref), f"{name}: gradient of scale {s} differs in {int((des[s] != ref).sum())} places"
            if s == empty:
                assert not bool(des[s].any())
            else:
                assert torch.equal(des[s] != 0, (g.double() > fl.view(-1, 1)) & (e != g))
    assert torch.equal(multi[0], single[0]) and same_bits(multi[2], single[2])
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(multi[3], single[3]))


@pytest.mark.parametrize("case", [c for c in M.LOSS_CASES if c[4] is None], ids=M.loss_id)
def test_loss_randn_at_the_existing_bar(case):
    ns, B, form, null, _, dloss = case
    pairs = M.loss_randn_inputs(case)
    _, fl = M.loss_floor(case)
    racc = [M.loss_reduce_f64(e, g, fl) for e, g in pairs]
    rloss = sum(s / c for s, c in racc)
    for route in ("multi", "single"):
        acc, loss, inv, des = loss_run(case, pairs, route)
        assert [float(v) for v in acc[1::2]] == [c for _, c in racc]
        err = abs(float(loss) - rloss) / abs(rloss)
        print(f"loss {route}: {err:.3e}")
        assert err <= M.LOSS_BAR
        for s, (e, g) in enumerate(pairs):
            if des[s] is not None:
                bar(f"loss gradient {route}", des[s], M.loss_bwd_f64(e, g, fl, dloss, racc[s][1]), M.LOSS_BAR)


def test_loss_backward_with_no_gradient_wanted_launches_nothing():
    case = (4, 1, "f32", None, None, 1.0)
    pairs = M.loss_exact_inputs(case)
    es, gs = [dev(e) for e, _ in pairs], [dev(g) for _, g in pairs]
    fd, dl, inv = torch.tensor([425.0], device=DEV), torch.ones(1, device=DEV), torch.ones(4, device=DEV)
    acc = torch.zeros(8, device=DEV, dtype=torch.float64)
    ep, gp = _arr(ctypes.c_void_p, [e.data_ptr() for e in es]), _arr(ctypes.c_void_p, [g.data_ptr() for g in gs])
    pbs = _arr(ctypes.c_int64, [e.shape[1] for e in es])
    call("mdf_masked_smooth_l1_reduce_multi", ep, gp, pbs, 4, fd.data_ptr(), 0, 1, 1, acc.data_ptr())
    before = lib().mdf_last_launch()
    assert b"reduce_multi" in before
    rc = lib().mdf_masked_smooth_l1_bwd_multi(ep, gp, pbs, 4, fd.data_ptr(), 0, 1, 1, dl.data_ptr(), inv.data_ptr(), _arr(ctypes.c_void_p, [None] * 4), _stream())
    assert rc == 0 and lib().mdf_last_launch() == before
    torch.cuda.synchronize()


def test_loss_train_with_nine_scales_takes_the_per_scale_entries():
    """More than 8 scales: train_ops.LossTrainFn goes scale by scale.  Value and gradients equal the mirror's, and the accumulators of
    the 8 + 1 split (the multi entry for the first eight, the single entry for the ninth) finalised together."""
    B, ns = 3, 9
    case8 = (8, B, "f64", None, None, 1.0)
    case9 = (9, B, "f64", None, None, 1.0)
    pairs = M.loss_exact_inputs(case9)
    ft, fl = M.loss_floor(case9)
    racc = [v for e, g in pairs for v in M.loss_reduce_ref(e, g, fl)]
    rloss, rinv = M.loss_finalize_ref(racc)
    ests = [dev(e).requires_grad_(True) for e, _ in pairs]
    counts = {}
    ops._counts, keep = counts, ops._counts
    try:
        loss = train_ops.loss_train(ft.to(DEV), [(e, dev(g)) for e, (_, g) in zip(ests, pairs)])
        (loss * 0.75).backward()
    finally:
        ops._counts = keep
    assert counts.get("mdf_masked_smooth_l1_reduce") == 9 and counts.get("mdf_masked_smooth_l1_bwd") == 9 and "mdf_masked_smooth_l1_reduce_multi" not in counts
    assert same_bits(loss.detach().cpu().reshape(1), torch.tensor([float(rloss)], dtype=torch.float32))
    for s, (e, g) in enumerate(pairs):
        assert torch.equal(ests[s].grad.cpu(), M.loss_bwd_ref(e, g, fl, 0.75, rinv[s])), s
    acc8 = loss_run(case8, pairs[:8], "multi")[0]
    acc1 = torch.zeros(2, device=DEV, dtype=torch.float64)
    e9, g9 = dev(pairs[8][0]), dev(pairs[8][1])
    fd = ft.to(DEV)
    call("mdf_masked_smooth_l1_reduce", e9.data_ptr(), g9.data_ptr(), fd.data_ptr(), 1, 1, B, e9.shape[1], acc1.data_ptr())
    split = torch.cat([acc8, acc1.cpu()])
    assert torch.equal(split, torch.tensor(racc, dtype=torch.float64))
    sloss, _ = M.loss_finalize_ref(split.numpy())
    assert same_bits(loss.detach().cpu().reshape(1), torch.tensor([float(sloss)], dtype=torch.float32))


# ==================================================================================================================== prob head wrapper
@pytest.mark.parametrize("per_pixel", [0, 1])
def test_prob_head_backward_wrapper_in_its_four_forms(per_pixel):
    B, D, h, w, C = 2, 5, 6, 11, 8
    case = (B, D, h, w, per_pixel)
    prob, hyp, dd, dp = M.softmax_randn_inputs(case)
    g = M._gen(31, per_pixel)
    x = torch.randn(B, D, h, w, C, generator=g)
    wt = 0.2 * torch.randn(1, C, 3, 3, 3, generator=g)
    p32, h32, d32, q32 = prob.float().double(), hyp.float().double(), dd.float().double(), dp.float().double()
    for form, (use_dd, use_dp, use_h) in zip(M.SOFTMAX_FORMS, ((1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 1, 0))):
        dx, dw = train_ops.prob_head_backward(dev(prob), dev(hyp) if use_h else None, dev(dd) if use_dd else None, dev(dp) if use_dp else None,
                                              dev(x), dev(wt))
        dlogit = M.softmax_regress_bwd_ref(p32, h32, d32 if use_dd else None, q32 if use_dp else None)
        bar(f"prob_head_backward dx {form}", dx, M.prob_conv_dgrad_ref(dlogit, wt.double()), M.PROB_BAR)
        wr = wt.double().clone().requires_grad_(True)
        F.conv3d(x.double().permute(0, 4, 1, 2, 3), wr, padding=1).backward(dlogit.unsqueeze(1))
        bar(f"prob_head_backward dw {form}", dw, wr.grad, M.PROB_BAR)


# ==================================================================================================================== refusals
def test_refusals_launch_nothing_and_name_the_reason():
    L = lib()
    buf = torch.zeros(1 << 16, device=DEV)
    dbl = torch.zeros(1 << 12, device=DEV, dtype=torch.float64)
    p, d, st = buf.data_ptr(), dbl.data_ptr(), _stream()
    call("mdf_bn_stats_fwd", p, 4, 8, 1, d)
    before = L.mdf_last_launch()
    two = _arr(ctypes.c_void_p, [p, p])
    nine = _arr(ctypes.c_void_p, [p] * 9)
    e, m = EPS32, MOM32
    refused = [
        ("C=12", lambda: L.mdf_bn_stats_fwd(p, 4, 12, 1, d, st), -1, b"C=12"),
        ("C=12 apply", lambda: L.mdf_bn_relu_apply_fwd(p, p, None, p, 4, 12, 1, st), -1, b"C=12"),
        ("N=0", lambda: L.mdf_bn_stats_fwd(p, 0, 8, 1, d, st), -1, b"voxel count"),
        ("N=0 bwd", lambda: L.mdf_bn_relu_bwd(p, p, p, d, p, 0, 8, 1, p, p, p, 1, st), -1, b"voxel count"),
        ("groups=0", lambda: L.mdf_bn_stats_fwd(p, 4, 8, 0, d, st), -1, b"bad argument"),
        ("groups=65536", lambda: L.mdf_bn_stats_fwd(p, 4, 8, 65536, d, st), -1, b"bad argument"),
        ("groups=0 apply", lambda: L.mdf_bn_relu_apply_fwd(p, p, None, p, 4, 8, 0, st), -1, b"bad argument"),
        ("groups=65536 reduce", lambda: L.mdf_bn_relu_bwd_reduce(p, p, p, 4, 8, 65536, d, st), -1, b"bad argument"),
        ("groups=65536 bwd", lambda: L.mdf_bn_relu_bwd(p, p, p, d, p, 4, 8, 65536, p, p, p, 1, st), -1, b"bad argument"),
        ("groups=0 finalize", lambda: L.mdf_bn_finalize_fwd(d, p, p, e, m, 4, 8, 0, p, None, None, None, 1, st), -1, b"bad shape"),
        ("groups=0 finalize_apply", lambda: L.mdf_bn_finalize_apply_fwd(p, d, p, p, e, m, None, p, p, None, None, None, 4, 8, 0, 1, st), -1, b"bad argument"),
        ("mean without var", lambda: L.mdf_bn_finalize_fwd(d, p, p, e, m, 4, 8, 1, p, p, None, None, 1, st), -1, b"go together"),
        ("var without mean", lambda: L.mdf_bn_finalize_apply_fwd(p, d, p, p, e, m, None, p, p, None, p, None, 4, 8, 1, 1, st), -1, b"go together"),
        ("nslices=0 finalize", lambda: L.mdf_bn_finalize_fwd(d, p, p, e, m, 4, 8, 1, p, None, None, None, 0, st), -1, b"bad shape"),
        ("nslices=0 finalize_apply", lambda: L.mdf_bn_finalize_apply_fwd(p, d, p, p, e, m, None, p, p, None, None, None, 4, 8, 1, 0, st), -1, b"bad argument"),
        ("nslices=0 bwd", lambda: L.mdf_bn_relu_bwd(p, p, p, d, p, 4, 8, 1, p, p, p, 0, st), -1, b"bad argument"),
        ("nslices=0 dgrad", lambda: L.mdf_prob_conv_dgrad_stat(p, p, p, 1, 1, 2, 2, 8, p, p, d, 0, st), -1, b"nslices"),
        ("upsample C=6", lambda: L.mdf_upsample2_bilinear_bwd(p, p, 1, 2, 2, 6, 0, st), -1, b"multiple of 4"),
        ("9 scales reduce", lambda: L.mdf_masked_smooth_l1_reduce_multi(nine, nine, _arr(ctypes.c_int64, [4] * 9), 9, p, 0, 1, 1, d, st), -1, b"at most 8"),
        ("9 scales bwd", lambda: L.mdf_masked_smooth_l1_bwd_multi(nine, nine, _arr(ctypes.c_int64, [4] * 9), 9, p, 0, 1, 1, p, p, nine, st), -1, b"at most 8"),
        ("empty scale reduce", lambda: L.mdf_masked_smooth_l1_reduce_multi(two, two, _arr(ctypes.c_int64, [4, 0]), 2, p, 0, 1, 1, d, st), -1, b"empty scale 1"),
        ("empty scale bwd", lambda: L.mdf_masked_smooth_l1_bwd_multi(two, two, _arr(ctypes.c_int64, [0, 4]), 2, p, 0, 1, 1, p, p, two, st), -1, b"empty scale 0"),
        ("dgrad C=32", lambda: L.mdf_prob_conv_dgrad(p, p, p, 1, 1, 2, 2, 32, st), -2, b"C in {8,16}"),
        ("dgrad_stat C=32", lambda: L.mdf_prob_conv_dgrad_stat(p, p, p, 1, 1, 2, 2, 32, p, p, d, 1, st), -2, b"C in {8,16}"),
        ("ddepth without hypos", lambda: L.mdf_prob_softmax_regress_bwd(p, None, 0, p, None, p, 1, 2, 2, 2, st), -1, b"needs the hypotheses"),
    ]
    for what, fn, want, text in refused:
        rc = fn()
        assert rc == want and text in L.mdf_last_error(), (what, rc, L.mdf_last_error())
        assert L.mdf_last_launch() == before, what
    torch.cuda.synchronize()
