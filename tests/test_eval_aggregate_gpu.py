"""GPU parity of the eval plane-sweep kernels (csrc/warp_aggregate.hip, the helpers of csrc/warp_common.h) with the float64 reference of
tests/eval_aggregate_mirror.py, through the torch-facing wrappers: the vector aggregation under its four routes (8 channels per lane,
4 channels per lane, 8 forced at C = 16, the LDS-window form), the pair-difference aggregation under both lane mappings, the variance
aggregation, the plain warp and the corner indices, in both output layouts.

The bars: e_hip <= 1.5 e_32 + t against the float64 reference over the finite voxels (the mirror's docstring derives t), NaN masks equal
to the reference's exactly, the sibling routes and the two layouts bit-identical, the warp bit-equal to oracle.homo_warping_explicit.
The case table and the proof that it reaches every launch route and FixedPairs form are in the mirror and in
tests/test_eval_aggregate_mirror_cpu.py.  mdf_last_launch gives a kernel's name, not its template arguments: the route is asserted by
name, the instantiation (channels, groups per lane, fixed or generic fill) follows from the plan the CPU suite holds against the sources.

`python tests/test_eval_aggregate_gpu.py` prints the table of measured distances (profiles/eval_aggregate_parity.md)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import eval_aggregate_mirror as E  # noqa: E402
import mdfnet_hip  # noqa: E402
from mdfnet_hip import lib, ops  # noqa: E402
from oracle import mvs_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MIN = -2 ** 31
ROUTE_ENV = ("MDF_WARP_VEC8", "MDF_WARP_WINDOW", "MDF_PAIRDIFF_GPL", "MDF_WARP_DCHUNK", "MDF_WARP_POOL_KB")
VEC_ROUTES = {"default": ({}, dict(vec8=1)), "vec8=0": ({"MDF_WARP_VEC8": "0"}, dict(vec8=0)), "vec8=2": ({"MDF_WARP_VEC8": "2"}, dict(vec8=2)),
              "window": ({"MDF_WARP_WINDOW": "1"}, dict(vec8=1, window=True))}
_CACHE = {}
MEASURED = []         # (case, mode, route, metric, e_hip, e_32, t)


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def refs(cid, mode):
    """(inputs, float64 reference, e_32, t) of a case and mode, computed once and left unchanged."""
    def make():
        inp = cached(("inp", cid), lambda: E.inputs(cid))
        r64, r32 = E.run_eval(inp, mode, torch.float64), E.run_eval(inp, mode, torch.float32)
        return inp, r64, E.distances_eval(r32, r64, mode), E.derived_t(inp, mode, r64, E.perturbed_runs(inp, mode))
    return cached(("refs", cid, mode), make)


def device_inputs(inp):
    def make():
        b, c, g, d, h, w, n_src = inp.dims
        return E.NS(feats=[t.to(DEV) for t in [inp.ref] + inp.srcs], diffs=[t.to(DEV) for t in [inp.dref] + inp.dsrcs],
                    proj=inp.proj.reshape(n_src, b, 12).to(DEV), hyp=inp.hyp.to(DEV), wpar=inp.wpar.to(DEV))
    return cached(("dev", inp.id), make)


def clean_env(monkeypatch, env=None):
    for k in ROUTE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def last_launch():
    return lib().mdf_last_launch().decode()


def ndhwc(cost):
    """logical [B,X,D,h,w] -> [B,D,h,w,X] (the mirror's layout)."""
    return cost.permute(0, 2, 3, 4, 1).contiguous()


def hold_to_the_bar(cid, mode, route, got, fails):
    """Prints every figure, then collects the misses of e_hip <= 1.5 e_32 + t and of the NaN mask."""
    inp, r64, e_32, t = refs(cid, mode)
    name = E.QUANTITY[mode]
    res = E.NS(**{name: got.detach().cpu().double()})
    if not torch.equal(E.nan_mask(res, mode), E.nan_mask(r64, mode)):
        fails.append((mode, route, "NaN mask", int(E.nan_mask(res, mode).sum()), int(E.nan_mask(r64, mode).sum())))
        return
    e_hip = E.distances_eval(res, r64, mode)
    for k, eh in e_hip.items():
        bar = 1.5 * e_32[k] + t[k]
        print(f"{cid} {mode:8s} {route:8s} {k:4s}: e_hip {eh:.2e}  e_32 {e_32[k]:.2e}  t {t[k]:.2e}  e_hip / (1.5 e_32 + t) = {eh / bar:.3f}")
        MEASURED.append((cid, mode, route, k, eh, e_32[k], t[k]))
    fails += [(mode, route) + f for f in E.judge(e_hip, e_32, t)]


# ==================================================================================================================== vec
@pytest.mark.parametrize("cid", list(E.CASES))
def test_vector_aggregate_routes_layouts_and_bar(cid, monkeypatch):
    inp, r64, _, _ = refs(cid, "vec")
    x, g = device_inputs(inp), inp.dims[2]
    out, fails = {}, []
    for route, (env, rule) in VEC_ROUTES.items():
        clean_env(monkeypatch, env)
        plan = E.vec_route(inp.dims, **rule)
        for cl in (True, False):
            cost = ops.warp_aggregate_vec(x.feats, x.proj, x.hyp, x.wpar, g, channels_last=cl)
            assert last_launch() == plan.launch, (route, last_launch(), plan.launch)
            assert cost.shape == (inp.dims[0], g, inp.dims[3], inp.dims[4], inp.dims[5]) and cost.is_contiguous() != cl
            out[route, cl] = ndhwc(cost)
    base = out["default", True]
    hold_to_the_bar(cid, "vec", "default", base, fails)
    assert not fails, fails
    same_nan = lambda a, b_: torch.equal(torch.isnan(a), torch.isnan(b_)) and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b_, nan=7.0))  # noqa: E731
    for key, val in out.items():                 # the four routes and the two layouts: one cost volume, bit for bit
        assert same_nan(val, base), key
    if not bool(torch.isnan(base).any()):
        assert all(torch.equal(val, base) for val in out.values())


# ==================================================================================================================== pairdiff
@pytest.mark.parametrize("cid", list(E.CASES))
def test_pair_difference_aggregate_lane_mappings_layouts_and_bar(cid, monkeypatch):
    """GPL 4 against GPL 8: the kernel states one operand order for both, so the two are held bit-identical (observed to hold on the
    whole table on the first GPU run), next to the bar each meets on its own."""
    inp, r64, _, _ = refs(cid, "pairdiff")
    x = device_inputs(inp)
    out, fails = {}, []
    for gpl in (4, 8):
        clean_env(monkeypatch, {"MDF_PAIRDIFF_GPL": str(gpl)})
        plan = E.pairdiff_route(inp.dims, gpl)
        for cl in (True, False):
            cost = ops.warp_aggregate_pairdiff(x.diffs, x.proj, x.hyp, x.wpar, channels_last=cl)
            assert last_launch() == plan.launch
            out[gpl, cl] = ndhwc(cost)
        hold_to_the_bar(cid, "pairdiff", f"gpl{gpl}", out[gpl, True], fails)
        assert torch.equal(torch.nan_to_num(out[gpl, True], nan=7.0), torch.nan_to_num(out[gpl, False], nan=7.0)), gpl
    assert not fails, fails
    assert torch.equal(torch.nan_to_num(out[4, True], nan=7.0), torch.nan_to_num(out[8, True], nan=7.0)), "GPL 4 and GPL 8 differ"


# ==================================================================================================================== var
@pytest.mark.parametrize("cid", list(E.VAR_CASES))
def test_variance_aggregate_layouts_and_bar(cid, monkeypatch):
    inp, r64, _, _ = refs(cid, "var")
    x = device_inputs(inp)
    clean_env(monkeypatch)
    fails, out = [], {}
    for cl in (True, False):
        var = ops.warp_aggregate_var(x.feats, x.proj, x.hyp, channels_last=cl)
        assert last_launch() == "warp_kernel" and var.is_contiguous() != cl
        out[cl] = ndhwc(var)
    hold_to_the_bar(cid, "var", "default", out[True], fails)
    assert not fails, fails
    assert torch.equal(torch.nan_to_num(out[True], nan=7.0), torch.nan_to_num(out[False], nan=7.0))
    assert torch.equal(torch.isnan(out[True]), torch.isnan(out[False]))


# ==================================================================================================================== warp, corners
@pytest.mark.parametrize("cid", list(E.CASES))
def test_warp_and_corner_indices_are_exact(cid, monkeypatch):
    inp = cached(("inp", cid), lambda: E.inputs(cid))
    b, c, g, d, h, w, n_src = inp.dims
    x = device_inputs(inp)
    clean_env(monkeypatch)
    eye, src4 = E.projections_4x4(inp)
    want = O.homo_warping_explicit(inp.srcs[0], src4[0], eye, inp.hyp)
    got = ops.homo_warp(x.feats[1], x.proj[0], x.hyp)
    assert last_launch() == "warp_kernel"
    assert np.array_equal(got.cpu().numpy(), want.numpy(), equal_nan=True)
    for v in range(n_src):
        ix, iy = O.warp_positions(O.relative_projection(src4[v], eye), inp.hyp, h, w)
        ix, iy = ix.expand(b, d, h * w), iy.expand(b, d, h * w)
        x0, y0, _, _ = O.warp_corners(ix, iy, h, w)
        idx = ops.warp_corner_indices(x.proj[v], x.hyp, h, w).cpu()
        assert last_launch() == "corner_index_kernel"
        exp = torch.stack([x0, y0], -1).reshape(idx.shape)
        fin = (torch.isfinite(ix) & torch.isfinite(iy)).reshape(b, d, h, w)
        assert torch.equal(idx[fin], exp[fin]), v
        assert bool((idx[~fin] == INT32_MIN).all()), v
        if cid == "z0" and v == 0:
            assert bool((~fin)[:, 1].all()) and int((~fin).sum()) == h * w


# ==================================================================================================================== plane independence
@pytest.mark.parametrize("cid", ["fix4c64", "gen3"])
def test_planes_are_independent_across_a_chunk_boundary(cid, monkeypatch):
    """A call on planes [a, b) alone equals the slice of the full call bit for bit; [a, b) starts inside the first chunk of the full call
    and ends in a later one, and the short call walks other chunks altogether: the chunk walk from a second side, with no reference."""
    inp = cached(("inp", cid), lambda: E.inputs(cid))
    x, g = device_inputs(inp), inp.dims[2]

    def check(plan, fn):
        a, b_ = E.straddling_planes(plan)
        hyp = x.hyp[:, a:b_].contiguous()
        full, part = fn(x.hyp), fn(hyp)
        assert part.shape[2] == b_ - a and torch.equal(full[:, :, a:b_], part), (plan.kernel, a, b_)

    for env, rule in (VEC_ROUTES["default"], VEC_ROUTES["vec8=0"], VEC_ROUTES["window"]):
        clean_env(monkeypatch, env)
        check(E.vec_route(inp.dims, **rule), lambda hyp: ops.warp_aggregate_vec(x.feats, x.proj, hyp, x.wpar, g))
    for gpl in (4, 8):
        clean_env(monkeypatch, {"MDF_PAIRDIFF_GPL": str(gpl)})
        check(E.pairdiff_route(inp.dims, gpl), lambda hyp: ops.warp_aggregate_pairdiff(x.diffs, x.proj, hyp, x.wpar))
    clean_env(monkeypatch)
    check(E.plan_eval(inp.dims, "warp_kernel"), lambda hyp: ops.warp_aggregate_var(x.feats, x.proj, hyp))
    check(E.plan_eval(inp.dims, "warp_kernel", n_src=1), lambda hyp: ops.homo_warp(x.feats[1], x.proj[0], hyp))


# ==================================================================================================================== refusals
def test_entry_points_refuse_bad_view_counts_channels_and_rows(monkeypatch):
    """n_src = 0 and 17, C = 12 and h = 1 are refused with a message that names the argument, and nothing is launched: mdf_last_launch
    still names the kernel before, and the census of C-ABI calls shows the one refused call.  (tests/test_abi_errors_gpu.py holds
    n_src = 17 and C = 48 for the vector aggregation at the C ABI, tests/test_pairdiff_gpu.py G = 12.)"""
    clean_env(monkeypatch)
    f = lambda c, h=4, n=3: [torch.randn(1, c, h, 8, device=DEV) for _ in range(n)]  # noqa: E731
    proj = torch.zeros(17, 1, 12, device=DEV)
    hyp = torch.full((1, 2, 1, 1), 500.0, device=DEV)
    ops.warp_corner_indices(proj[0], hyp, 4, 8)
    before = last_launch()
    assert before == "corner_index_kernel"
    vec = lambda feats, g: ops.warp_aggregate_vec(feats, proj, hyp, torch.zeros(g + 4, device=DEV), g)  # noqa: E731
    pdf = lambda feats: ops.warp_aggregate_pairdiff(feats, proj, hyp, torch.zeros(feats[0].shape[1] + 4, device=DEV))  # noqa: E731
    var = lambda feats: ops.warp_aggregate_var(feats, proj, hyp)  # noqa: E731
    refused = [
        ("mdf_warp_aggregate_vec_fwd", lambda: vec(f(16, n=1), 8), "n_src=0"),
        ("mdf_warp_aggregate_vec_fwd", lambda: vec(f(12), 6), "C=12"),
        ("mdf_warp_aggregate_vec_fwd", lambda: vec(f(16, h=1), 8), "h=1"),
        ("mdf_warp_aggregate_pairdiff_fwd", lambda: pdf(f(8, n=1)), "n_src=0"),
        ("mdf_warp_aggregate_pairdiff_fwd", lambda: pdf(f(8, n=18)), "n_src=17"),
        ("mdf_warp_aggregate_pairdiff_fwd", lambda: pdf(f(8, h=1)), "h=1"),
        ("mdf_warp_aggregate_var_fwd", lambda: var(f(16, n=1)), "n_src=0"),
        ("mdf_warp_aggregate_var_fwd", lambda: var(f(16, n=18)), "n_src=17"),
        ("mdf_warp_aggregate_var_fwd", lambda: var(f(12)), "C=12"),
        ("mdf_warp_aggregate_var_fwd", lambda: var(f(16, h=1)), "h=1"),
        ("mdf_homo_warp_fwd", lambda: ops.homo_warp(f(12)[0], proj[0], hyp), "C=12"),
        ("mdf_homo_warp_fwd", lambda: ops.homo_warp(f(16, h=1)[0], proj[0], hyp), "h=1"),
        ("mdf_warp_corner_indices", lambda: ops.warp_corner_indices(proj[0], hyp, 1, 8), "h=1"),
    ]
    for entry, call, names in refused:
        ops.count_begin()
        try:
            with pytest.raises(mdfnet_hip.MdfHipError, match=names):
                call()
        finally:
            counts = ops.count_end()
        assert counts == {entry: 1}, (entry, names, counts)
        assert last_launch() == before, (entry, names, last_launch())
    # ... and the library still works
    assert ops.warp_aggregate_var(f(16), proj, hyp).shape == (1, 16, 2, 4, 8) and last_launch() == "warp_kernel"
    torch.cuda.synchronize()


# ==================================================================================================================== the record
def measured_table():
    lines = ["| case | mode | route | metric | e_hip | e_32 | t | e_hip / (1.5 e_32 + t) |", "|---|---|---|---|---|---|---|---|"]
    for cid, mode, route, k, eh, e3, t in MEASURED:
        lines.append(f"| {cid} | {mode} | {route} | {k} | {eh:.2e} | {e3:.2e} | {t:.2e} | {eh / (1.5 * e3 + t):.2f} |")
    return "\n".join(lines)


if __name__ == "__main__":
    for route_env in ROUTE_ENV:
        os.environ.pop(route_env, None)
    all_fails = []
    for case in E.CASES:
        dims = refs(case, "vec")[0].dims
        xs = device_inputs(refs(case, "vec")[0])
        hold_to_the_bar(case, "vec", "default", ndhwc(ops.warp_aggregate_vec(xs.feats, xs.proj, xs.hyp, xs.wpar, dims[2])), all_fails)
        for lanes in (4, 8):
            os.environ["MDF_PAIRDIFF_GPL"] = str(lanes)
            hold_to_the_bar(case, "pairdiff", f"gpl{lanes}", ndhwc(ops.warp_aggregate_pairdiff(xs.diffs, xs.proj, xs.hyp, xs.wpar)), all_fails)
        os.environ.pop("MDF_PAIRDIFF_GPL")
        if case in E.VAR_CASES:
            hold_to_the_bar(case, "var", "default", ndhwc(ops.warp_aggregate_var(xs.feats, xs.proj, xs.hyp, channels_last=True)), all_fails)
    print(measured_table())
    print("misses:", all_fails)
    sys.exit(1 if all_fails else 0)
