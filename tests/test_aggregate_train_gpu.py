"""GPU parity of the training-mode vector aggregation (csrc/warp_aggregate_train.hip, warp_scatter.h, the tap-table helpers of
warp_common.h) with the float64 reference of tests/aggregate_mirror.py, through the C ABI, pass by pass as AggregateTrainFn runs them:
prepare, pass 0 (statistics), finalize, pass 1 (forward), pass 2 (backward reductions), pass 3 (scatter), backward finalize.  Every pass
consumes the previous pass's GPU output and every intermediate is compared, so a failure names its pass.

Outputs are filled with NaN before the call, accumulators are zeroed as AggregateTrainFn zeroes them, and `red`, `par`, `dcw` and the
last `dhalf` carry a two-element NaN canary behind their end.  The bars: exact where the kernels owe exactness; 1 fp32 ulp of the
float64 mirror for agg_finalize_kernel; e_hip <= 1.5 e_32 + t against the float64 reference for everything else (the mirror's docstring
derives t), next to the bars tests/test_train_gpu.py holds against the fp32 oracle.  The case table and the proof that it reaches every
launch route are in the mirror and in tests/test_aggregate_mirror_cpu.py.

Run as a program (`python tests/test_aggregate_train_gpu.py --child`) the file checks the reduced table in a fresh process: the forced
launch geometries sit behind MDF_WARP_TRAIN_TAB / MDF_WARP_BWD_TAB / MDF_WARP_TRAIN_BLOCKS / MDF_WARP_BWD_BLOCKS, which the library
reads once per process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import aggregate_mirror as M  # noqa: E402
from mdfnet_hip import lib, train_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GEOMETRY_ENV = ("MDF_WARP_TRAIN_TAB", "MDF_WARP_BWD_TAB", "MDF_WARP_TRAIN_BLOCKS", "MDF_WARP_BWD_BLOCKS")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rc_of(name, *args):
    return getattr(lib(), name)(*args, _stream())


def call(name, *args):
    rc = rc_of(name, *args)
    assert rc == 0, (name, rc, lib().mdf_last_error().decode("utf-8", "replace"))


def dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[ptr(t) for t in ts])


def filled(n, value, canary=2, dtype=torch.float32):
    """n elements of `value` and `canary` NaNs behind them."""
    buf = torch.full((n + canary,), value, device=DEV, dtype=dtype)
    buf[n:] = NAN
    return buf


def canary_intact(buf, n):
    return bool(buf[n:].isnan().all()) and not bool(buf[:n].isnan().any())


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def refs(cid):
    """(inputs, float64 reference, fp32 restatement, derived t) of a case, computed once."""
    def make():
        inp = M.inputs(cid)
        r64, r32 = M.run(inp, torch.float64), M.run(inp, torch.float32)
        pert = [M.run(inp, torch.float64, perturb=17 + i) for i in range(M.PERTURB_DRAWS)]
        live, cnt = M.live_texels(inp)
        plan = M.plan_train(inp.dims, inp.per_pixel)
        return inp, r64, r32, M.derived_t(inp, r64, pert, plan.dchunk, int(cnt.max())), live
    return cached(("refs", cid), make)


# ==================================================================================================================== the chain
def device_inputs(inp):
    b, c, g, d, h, w, n_src = inp.dims
    nhwc = lambda t: dev(t.permute(0, 2, 3, 1))  # noqa: E731
    return M.NS(ref=nhwc(inp.ref), srcs=[nhwc(s) for s in inp.srcs], proj=dev(inp.proj.reshape(n_src, b, 12)),
                hyp=dev(inp.hyp.reshape(b, d, -1) if inp.per_pixel else inp.hyp.reshape(b, d)), pp=int(inp.per_pixel), cw=dev(inp.cw),
                gamma=dev(inp.gamma), beta=dev(inp.beta), w2=dev(inp.w2), b2=dev(inp.b2), dcost=dev(inp.dcost.permute(0, 2, 3, 4, 1)))


def vec_train(pass_, x, dims, par, red_in=None, dcost=None, cost=None, wsum=None, red_out=None, dref=None, dsrc=None, dcw=None, aux=None,
              srcs=None, override=None):
    b, c, g, d, h, w, n_src = dims
    o = dict(C=c, G=g, h=h, n_src=n_src, pass_=pass_)
    o.update(override or {})
    return rc_of("mdf_warp_aggregate_vec_train", o["pass_"], ptr(x.ref), ptrs(x.srcs if srcs is None else srcs), ptr(x.proj), ptr(x.hyp), x.pp,
                 ptr(par), ptr(red_in), ptr(dcost), ptr(cost), ptr(wsum), ptr(red_out), ptr(dref), None if dsrc is None else ptrs(dsrc), ptr(dcw),
                 ptr(aux), b, o["C"], o["G"], d, o["h"], w, o["n_src"])


def chain(inp, nbt0=5):
    """The seven launches of one forward + backward -> the kernels' outputs on the CPU in float64 (mirror layouts), after the exact
    checks of the control kernels and the canaries."""
    b, c, g, d, h, w, n_src = inp.dims
    n, npar, nhalf, nref = b * d * h * w, g + 4 + 4 * n_src, b * h * w * g, b * h * w * c
    x = device_inputs(inp)

    def ok(rc, what):
        assert rc == 0, (what, rc, lib().mdf_last_error().decode("utf-8", "replace"))

    # ---- prepare: par exact, red zeroed exactly
    par, red0 = filled(npar, NAN), filled(2 * n_src, NAN, dtype=torch.float64)
    call("mdf_aggregate_train_prepare", ptr(x.cw), ptr(x.w2), ptr(x.b2), ptr(x.gamma), n, g, n_src, ptr(par), ptr(red0), 2 * n_src)
    want = torch.cat([inp.cw, inp.w2, inp.b2, inp.gamma, torch.tensor([np.float32(1.0 / n)]), torch.zeros(4 * n_src)])
    assert torch.equal(par[:npar].cpu(), want), "agg_prepare_kernel: par"
    assert bool((red0[:2 * n_src] == 0).all()) and canary_intact(par, npar) and canary_intact(red0, 2 * n_src), "agg_prepare_kernel: red / canaries"

    # ---- pass 0
    ok(vec_train(0, x, inp.dims, par, red_out=red0), "pass 0")
    assert canary_intact(red0, 2 * n_src), "pass 0 wrote behind red"
    assert torch.equal(par[:g + 4].cpu(), want[:g + 4]) and canary_intact(par, npar)

    # ---- finalize: double arithmetic, one rounding
    rmean, rvar, nbt = dev(inp.rmean), dev(inp.rvar), torch.tensor([nbt0], device=DEV, dtype=torch.int64)
    call("mdf_aggregate_train_finalize", ptr(red0), ptr(x.gamma), ptr(x.beta), ctypes.c_float(M.BN_EPS32), ctypes.c_float(M.BN_MOM32), n, g, n_src,
         ptr(par), ptr(rmean), ptr(rvar), ptr(nbt))
    assert canary_intact(par, npar) and int(nbt) == nbt0 + n_src
    consts = par[g + 4:npar].cpu().reshape(n_src, 4)
    c64, rm64, rv64 = M.finalize_mirror(red0[:2 * n_src].cpu(), inp.gamma, inp.beta, n, inp.rmean, inp.rvar)
    within_one_ulp(consts, c64, "agg_finalize_kernel constants")
    within_one_ulp(torch.stack([rmean.cpu()[0], rvar.cpu()[0]]), torch.tensor([rm64, rv64], dtype=torch.float64), "agg_finalize_kernel running statistics")

    # ---- pass 1
    cost, wsum = filled(n * g, NAN, 0), filled(n, NAN, 0)
    ok(vec_train(1, x, inp.dims, par, cost=cost, wsum=wsum), "pass 1")
    cost_b, wsum_b = filled(n * g, NAN, 0), filled(n, NAN, 0)          # the forward has no atomics: a second run gives the same bits
    ok(vec_train(1, x, inp.dims, par, cost=cost_b, wsum=wsum_b), "pass 1 again")
    assert torch.equal(cost, cost_b) and torch.equal(wsum, wsum_b) and not bool(cost.isnan().any()), "pass 1 is not deterministic"

    # ---- pass 2
    red2, aux = filled(2 * n_src + 2, 0.0, dtype=torch.float64), filled(n_src * n * 4, NAN, 0)
    ok(vec_train(2, x, inp.dims, par, dcost=x.dcost, cost=cost, wsum=wsum, red_out=red2, aux=aux), "pass 2")
    assert canary_intact(red2, 2 * n_src + 2), "pass 2 wrote behind red"
    aux4 = aux.reshape(n_src, n, 4)
    assert bool((aux4[..., 3] == 0).all())

    # ---- pass 3
    dhalf, dref_acc, dcw = filled(n_src * nhalf, 0.0), torch.zeros(nref, device=DEV), filled(g, 0.0)
    views = [dhalf[v * nhalf:(v + 1) * nhalf] for v in range(n_src)]
    ok(vec_train(3, x, inp.dims, par, red_in=red2, dcost=x.dcost, cost=cost, wsum=wsum, dref=dref_acc, dsrc=views, dcw=dcw, aux=aux), "pass 3")
    assert canary_intact(dhalf, n_src * nhalf) and canary_intact(dcw, g), "pass 3 wrote behind dhalf / dcw"

    # ---- backward finalize: exact
    dfull, dpar, dref = filled(n_src * nhalf * 2, NAN, 0), filled(4, NAN), filled(nref, NAN, 0)
    call("mdf_aggregate_train_bwd_finalize", ptr(dhalf), ptr(red2), n_src, n_src * nhalf, ptr(dfull), ptr(dpar), ptr(dref_acc), ptr(dref), nref)
    hv = dhalf[:n_src * nhalf]
    assert torch.equal(dfull.reshape(-1, 2), torch.stack([hv, -hv], 1)) and torch.equal(dref, dref_acc), "agg_bwd_finalize_kernel"
    r2 = red2[:2 * n_src + 2].cpu()
    want_dpar = torch.stack([r2[1:2 * n_src:2].sum(), r2[0:2 * n_src:2].sum(), r2[2 * n_src], r2[2 * n_src + 1]]).float()
    assert torch.equal(dpar[:4].cpu(), want_dpar) and canary_intact(dpar, 4), "agg_bwd_finalize_kernel: dpar"

    f64 = lambda t: t.detach().cpu().double()  # noqa: E731
    return M.NS(red0=f64(red0[:2 * n_src]), consts=f64(consts), rmean=float(rmean), rvar=float(rvar), cost=f64(cost).reshape(b, d, h, w, g),
                wsum=f64(wsum).reshape(b, d, h, w), aux=f64(aux4[..., :3]), red2=f64(r2), dref=f64(dref).reshape(b, h, w, c),
                dsrc=f64(dfull).reshape(n_src, b, h, w, c), dcw=f64(dcw[:g]), dpar=f64(dpar[:4]),
                bits=(cost.clone(), wsum.clone()))


def within_one_ulp(got, ref64, what):
    """fp32 `got` equals the float64 `ref64` rounded to fp32, to within one fp32 ulp."""
    g = got.detach().cpu().numpy().astype(np.float32).reshape(-1)
    r = ref64.detach().cpu().numpy().astype(np.float64).reshape(-1)
    r32 = r.astype(np.float32)
    ulps = np.abs(g.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
    assert np.all(np.isfinite(g)) and float(ulps.max()) <= 1.0, (what, float(ulps.max()), g, r32)


# ==================================================================================================================== the bars
_TABLE = {}          # quantity, metric -> (ratio to the bar, e_32, e_hip, t, case): the worst ratio seen
FP32_ORACLE_BARS = {"cost": 2e-5, "dref": 2e-4, "dsrc": 2e-4, "dcw": 5e-4, "dpar": 1e-2}     # the bars of tests/test_train_gpu.py, max|d| / max|ref|


def judge(cid, got, label=""):
    """Assertion 3 for every quantity of one chain, after printing each figure; -> the failures (empty when all hold)."""
    inp, r64, r32, tt, live = refs(cid)
    n_src = inp.dims[6]
    fails = []
    for name in M.QUANTITIES:
        if n_src == 1 and name in M.ZERO_AT_ONE_VIEW:
            bound, val = M.one_view_bounds(r64)[name], M.quantity(got, name)
            worst = float((val.abs() / bound.clamp(min=1e-300)).max())
            print(f"{cid}{label} {name}: zero in exact arithmetic, |kernel| / noise bound = {worst:.3f}")
            if not worst <= 1.0:
                fails.append((name, "noise bound", worst))
            continue
        e_hip, e_32 = M.distances(got, r64, name), M.distances(r32, r64, name)
        for metric, eh in e_hip.items():
            e3, t = e_32[metric], tt[name][metric]
            bar = 1.5 * e3 + t
            ratio = eh / bar if bar > 0 else (0.0 if eh == 0 else float("inf"))
            print(f"{cid}{label} {name:7s} {metric:4s}: e_hip {eh:.2e}  e_32 {e3:.2e}  t {t:.2e}  e_hip / (1.5 e_32 + t) = {ratio:.3f}")
            if ratio > _TABLE.get((name, metric), (-1.0,))[0]:
                _TABLE[(name, metric)] = (ratio, e3, eh, t, cid + label)
            if not ratio <= 1.0:
                fails.append((name, metric, eh, e3, t))
        if name in FP32_ORACLE_BARS:
            a, r = M.quantity(got, name), M.quantity(r32, name)
            e = float((a - r).abs().max() / r.abs().max().clamp(min=1e-300))
            if not e < FP32_ORACLE_BARS[name]:
                fails.append((name, "fp32 oracle bar", e))
    # the scatter writes nothing outside the texels the mirror lists as touched by a live tap
    outside = ~live.unsqueeze(-1).expand_as(got.dsrc)
    if bool((got.dsrc[outside] != 0).any()):
        fails.append(("dsrc", "nonzero outside the live taps' texels", int((got.dsrc[outside] != 0).sum())))
    if not (abs(got.rmean - r64.rmean) <= 4 * M.U * (abs(r64.rmean) + abs(float(inp.rmean))) + 1.5 * abs(r32.rmean - r64.rmean)
            and abs(got.rvar - r64.rvar) <= 4 * M.U * (abs(r64.rvar) + abs(float(inp.rvar))) + 1.5 * abs(r32.rvar - r64.rvar)):
        fails.append(("running statistics", got.rmean, r64.rmean, got.rvar, r64.rvar))
    return fails


def print_table():
    print("\nquantity metric | e_32 | e_hip | t | e_hip / (1.5 e_32 + t) | case")
    for (name, metric), (ratio, e3, eh, t, cid) in sorted(_TABLE.items()):
        print(f"| {name} | {metric} | {e3:.1e} | {eh:.1e} | {t:.1e} | {ratio:.2f} | {cid} |")


# ==================================================================================================================== tests
@pytest.mark.parametrize("cid", list(M.CASES))
def test_chain_against_the_float64_reference(cid):
    """Assertions 1 (the exact ones inside `chain`), 2 and 3 for one case of the table."""
    got = chain(refs(cid)[0])
    fails = judge(cid, got)
    print_table()
    assert not fails, fails
    if cid == "gone":
        assert bool((got.dsrc[1] == 0).all()), "a view without a live tap received a gradient"
        assert bool((got.dsrc[0] != 0).any())


@pytest.mark.parametrize("cid", ["fix4", "gen3", "mag64"])
def test_forward_is_deterministic(cid):
    """Two whole chains: the fp64 atomics of pass 0 may add in another order, so the bits are compared when the fp32 constants came out
    the same (all but always); `chain` itself holds two runs of pass 1 on ONE `par` bit-identical for every case."""
    inp = refs(cid)[0]
    a, b_ = chain(inp), chain(inp)
    if torch.equal(a.consts, b_.consts):        # the fp64 atomics of pass 0 rounded to the same fp32 constants (all but always)
        assert torch.equal(a.bits[0], b_.bits[0]) and torch.equal(a.bits[1], b_.bits[1])
    else:
        assert float((a.consts - b_.consts).abs().max() / a.consts.abs().max()) < 4 * M.U


def _module(inp):
    from net.unit.homoaggregate import VectorAggregate
    b, c, g, d, h, w, n_src = inp.dims
    mod = VectorAggregate(g)
    with torch.no_grad():
        head = mod.depth_weight
        head[0].conv.weight.copy_(inp.cw.reshape(1, g, 1, 1, 1))
        head[0].bn.weight.copy_(inp.gamma)
        head[0].bn.bias.copy_(inp.beta)
        head[0].bn.running_mean.copy_(inp.rmean)
        head[0].bn.running_var.copy_(inp.rvar)
        head[1].weight.copy_(inp.w2.reshape(1, 1, 1, 1, 1))
        head[1].bias.copy_(inp.b2)
    return mod.train().to(DEV)


@pytest.mark.parametrize("cid", ["fix4", "d9"])
def test_per_view_tensors_and_one_view_major_tensor_give_the_same_bits(cid):
    """train_ops.aggregate_train from per-view feature tensors and from the slices of ONE view-major tensor: the same kernels on the
    same values, so cost is bit-identical (given the same fp32 constants) and so is its agreement with the chain."""
    inp = refs(cid)[0]
    b, c, g, d, h, w, n_src = inp.dims
    proj, hyp = dev(inp.proj.reshape(n_src, b, 12)), dev(inp.hyp)
    feats = [dev(f) for f in [inp.ref] + inp.srcs]
    mod = _module(inp)
    cost_a = train_ops.aggregate_train(mod, feats, proj, hyp).clone()
    whole = torch.cat(feats, 0).contiguous(memory_format=torch.channels_last)
    parts = [whole[v * b:(v + 1) * b] for v in range(n_src + 1)]
    for v, t in enumerate(parts):
        t._mdf_parent = (whole, v, n_src + 1)
    mod_b = _module(inp)
    cost_b = train_ops.aggregate_train(mod_b, parts, proj, hyp).clone()
    bn_a, bn_b = mod.depth_weight[0].bn, mod_b.depth_weight[0].bn
    if torch.equal(bn_a.running_var, bn_b.running_var) and torch.equal(bn_a.running_mean, bn_b.running_mean):
        assert torch.equal(cost_a, cost_b)
    assert float((cost_a - cost_b).abs().max()) < 1e-6
    got = chain(inp)
    assert float((cost_a.permute(0, 2, 3, 4, 1).cpu().double() - got.cost).abs().max()) < 1e-6


def test_finalize_kernel_within_one_ulp_of_the_float64_mirror():
    """agg_finalize_kernel on hand-made sums: a view whose variance is exactly zero and one whose variance is negative by rounding (the
    clamp; eps dominates, invstd = 1/sqrt(eps)), ordinary views, n = 1 (the unbiased factor's guard), and without running statistics."""
    for n, reds, gamma, beta in ((12, [6.0, 3.0, 6.0, 3.0 - 1e-9, 7.25, 31.5, -3.0, 40.0], 1.3, -0.2),
                                 (1, [0.75, 0.5625], -0.7, 0.4),
                                 (5001, [1234.5, 9999.0, -77.0, 3.0, 0.0, 1e-12], 0.9, 0.1)):
        n_src, g = len(reds) // 2, 8
        red = torch.tensor(reds, dtype=torch.float64, device=DEV)
        gm, bt = torch.tensor([gamma], device=DEV), torch.tensor([beta], device=DEV)
        for track in (True, False):
            par = filled(g + 4 + 4 * n_src, NAN)
            rmean, rvar, nbt = torch.tensor([0.3], device=DEV), torch.tensor([1.7], device=DEV), torch.tensor([41], device=DEV, dtype=torch.int64)
            call("mdf_aggregate_train_finalize", ptr(red), ptr(gm), ptr(bt), ctypes.c_float(M.BN_EPS32), ctypes.c_float(M.BN_MOM32), n, g, n_src,
                 ptr(par), ptr(rmean) if track else None, ptr(rvar) if track else None, ptr(nbt) if track else None)
            c64, rm, rv = M.finalize_mirror(reds, gm.cpu(), bt.cpu(), n, rmean.new_tensor([0.3]).cpu(), rvar.new_tensor([1.7]).cpu())
            within_one_ulp(par[g + 4:g + 4 + 4 * n_src], c64.reshape(-1), "constants")
            assert bool(par[:g + 4].isnan().all()) and bool(par[g + 4 + 4 * n_src:].isnan().all())
            if track:
                within_one_ulp(torch.stack([rmean[0], rvar[0]]), torch.tensor([rm, rv], dtype=torch.float64), "running statistics")
                assert int(nbt) == 41 + n_src
            else:
                assert float(rmean) == np.float32(0.3) and float(rvar) == np.float32(1.7) and int(nbt) == 41
        if n == 12:
            inv = par[g + 4:g + 4 + 4 * n_src].cpu().reshape(n_src, 4)[:2, 3].double()
            assert bool(((inv - 1.0 / np.sqrt(M.BN_EPS32)).abs() < 1e-4 * inv).all())


@pytest.mark.parametrize("n_half,n_ref,n_src", [(1000, 2000, 3), (1000, 8000, 1), (257, 4, 16), (70000, 130000, 2), (300, 0, 2)])
def test_bwd_finalize_kernel_exact(n_half, n_ref, n_src):
    """Integer-valued inputs: dfull = (v, -v) interleaved, d ref a copy, dpar the fp64 sums rounded once.  n_half no multiple of 256,
    n_ref / 4 below and above n_half, and the form without d ref (n_ref = 0)."""
    gen = torch.Generator().manual_seed(n_half)
    dhalf = torch.randint(-9, 10, (n_half,), generator=gen).float().to(DEV)
    red = torch.randint(-(1 << 30), 1 << 30, (2 * n_src + 2,), generator=gen).double() * 1025.0
    dfull, dpar = filled(2 * n_half, NAN), filled(4, NAN)
    acc = torch.randint(-9, 10, (n_ref,), generator=gen).float().to(DEV) if n_ref else None
    dref = filled(n_ref, NAN) if n_ref else None
    call("mdf_aggregate_train_bwd_finalize", ptr(dhalf), ptr(red.to(DEV)), n_src, n_half, ptr(dfull), ptr(dpar), ptr(acc), ptr(dref), n_ref)
    assert torch.equal(dfull[:2 * n_half].reshape(-1, 2), torch.stack([dhalf, -dhalf], 1)) and canary_intact(dfull, 2 * n_half)
    if n_ref:
        assert torch.equal(dref[:n_ref], acc) and canary_intact(dref, n_ref)
    want = torch.stack([red[1:2 * n_src:2].sum(), red[0:2 * n_src:2].sum(), red[2 * n_src], red[2 * n_src + 1]]).float()
    assert torch.equal(dpar[:4].cpu(), want) and canary_intact(dpar, 4)


@pytest.mark.parametrize("cid", M.COLLISION_CASES)
def test_claim_protocol_against_all_atomic_window_updates(cid, monkeypatch):
    """The non-atomic window update behind the claim protocol against MDF_WARP_BWD_ATOMIC=1 (read per call) where many pixels of one
    wave instruction meet on one texel: bars of test_aggregate_scatter_claim_vs_all_atomics_full_size (2e-5 max, 4e-6 L2), and both
    modes within the bar of the float64 reference."""
    inp = refs(cid)[0]
    monkeypatch.delenv("MDF_WARP_BWD_ATOMIC", raising=False)
    claim = chain(inp)
    monkeypatch.setenv("MDF_WARP_BWD_ATOMIC", "1")
    atomic = chain(inp)
    monkeypatch.delenv("MDF_WARP_BWD_ATOMIC", raising=False)
    fails = judge(cid, claim, " claim") + judge(cid, atomic, " atomic")
    for name in ("dsrc", "dref"):
        a, b_ = M.quantity(claim, name), M.quantity(atomic, name)
        e_max, e_l2 = float((a - b_).abs().max() / b_.abs().max()), float((a - b_).norm() / b_.norm())
        print(f"{cid} {name} claim vs atomic: max {e_max:.2e} l2 {e_l2:.2e}")
        if not (e_max < 2e-5 and e_l2 < 4e-6):
            fails.append((name, "claim vs atomic", e_max, e_l2))
    print_table()
    assert not fails, fails


REFUSALS = [
    ("pass 4", dict(pass_=4), 3, "pass=4"),
    ("G * 2 != C", dict(G=7), 1, "C/G == 2"),
    ("C = 8", dict(C=8, G=4), 1, "C in {16,32,64}"),
    ("n_src = 0", dict(n_src=0), 1, "n_src=0"),
    ("n_src = 17", dict(n_src=17), 1, "n_src=17"),
    ("h = 1", dict(h=1), 1, "bad shape"),
    ("null src_feas[1]", "null_src", 1, "src_feas[1] is null"),
    ("null dsrc[1] in pass 3", "null_dsrc", 3, "dsrc[1] is null"),
    ("pass 2 without aux", "no_aux", 2, "aux"),
]


@pytest.mark.parametrize("what,how,pass_,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing_and_name_the_reason(what, how, pass_, text):
    inp = refs("s2")[0]
    b, c, g, d, h, w, n_src = inp.dims
    n, nhalf = b * d * h * w, b * h * w * g
    x = device_inputs(inp)
    par = torch.zeros(g + 4 + 4 * n_src, device=DEV)
    outs = dict(cost=filled(n * g, NAN, 0), wsum=filled(n, NAN, 0), red=filled(2 * n_src + 2, NAN, 0, torch.float64), dref=filled(b * h * w * c, NAN, 0),
                dcw=filled(g, NAN, 0), aux=filled(n_src * n * 4, NAN, 0), dhalf=filled(n_src * nhalf, NAN, 0))
    views = [outs["dhalf"][v * nhalf:(v + 1) * nhalf] for v in range(n_src)]
    srcs = list(x.srcs)
    if how == "null_src":
        srcs[1] = None
    if how == "null_dsrc":
        views[1] = None
    red_in = torch.zeros(2 * n_src + 2, device=DEV, dtype=torch.float64)
    rc = vec_train(pass_, x, inp.dims, par, red_in=red_in, dcost=x.dcost, cost=outs["cost"], wsum=outs["wsum"], red_out=outs["red"],
                   dref=outs["dref"], dsrc=views, dcw=outs["dcw"], aux=None if how == "no_aux" else outs["aux"], srcs=srcs,
                   override=how if isinstance(how, dict) else None)
    torch.cuda.synchronize()
    msg = lib().mdf_last_error().decode("utf-8", "replace")
    assert rc != 0 and text in msg, (rc, msg)
    for k, t in outs.items():
        assert bool(t.isnan().all()), f"{what}: {k} was written"


def test_bwd_finalize_refuses_a_ragged_d_ref():
    dhalf, red = torch.zeros(8, device=DEV), torch.zeros(6, device=DEV, dtype=torch.float64)
    dfull, dpar, acc, dref = filled(16, NAN, 0), filled(4, NAN, 0), torch.zeros(6, device=DEV), filled(6, NAN, 0)
    rc = rc_of("mdf_aggregate_train_bwd_finalize", ptr(dhalf), ptr(red), 2, 8, ptr(dfull), ptr(dpar), ptr(acc), ptr(dref), 6)
    torch.cuda.synchronize()
    assert rc != 0 and "n_ref" in lib().mdf_last_error().decode("utf-8", "replace")
    assert bool(dfull.isnan().all()) and bool(dpar.isnan().all()) and bool(dref.isnan().all())


# ==================================================================================================================== forced geometry
CHILD_SETTINGS = {"one_slice": {"MDF_WARP_TRAIN_TAB": "64", "MDF_WARP_BWD_TAB": "64", "MDF_WARP_TRAIN_BLOCKS": "1", "MDF_WARP_BWD_BLOCKS": "1"},
                  "most_slices": {"MDF_WARP_TRAIN_BLOCKS": "1048576", "MDF_WARP_BWD_BLOCKS": "1048576"}}


def child_main():
    """Assertions 1 and 3 over the reduced table under this process's launch geometry."""
    bad = []
    for cid in M.REDUCED_CASES:
        got = chain(refs(cid)[0])
        bad += [(cid,) + f for f in judge(cid, got, " child")]
    print_table()
    print("child: %d cases, %d failures %s" % (len(M.REDUCED_CASES), len(bad), bad))
    return 1 if bad else 0


@pytest.mark.parametrize("setting", list(CHILD_SETTINGS))
def test_forced_launch_geometry_in_a_fresh_process(setting):
    """One-plane chunks in a single slice (fix4's 48 planes with the direct d ref store), and the maximal D/4 slices: the sizes are
    statics the library reads once, hence a fresh process per setting, one after the other."""
    env = dict(os.environ)
    for k in GEOMETRY_ENV + ("MDF_WARP_BWD_ATOMIC",):
        env.pop(k, None)
    env.update(CHILD_SETTINGS[setting])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, timeout=120, capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
    assert "child: %d cases, 0 failures" % len(M.REDUCED_CASES) in r.stdout


if __name__ == "__main__":
    sys.exit(child_main() if "--child" in sys.argv else 2)
