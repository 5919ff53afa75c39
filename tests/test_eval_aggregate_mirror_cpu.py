"""CPU: the conditions tests/test_eval_aggregate_gpu.py relies on -- the mirror's constants against the kernel sources, the case table's
reach over every launch route and FixedPairs form of the eval warp / aggregation kernels, the grid-line margin of every sample, the NaN
masks, the fp32 restatement against the oracle the goldens pin, and that the bar e_hip <= 1.5 e_32 + t of tests/eval_aggregate_mirror.py
trips on deliberate errors.  No GPU.  If a case misses a condition, the case changes."""
import copy
import os
import re
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
import eval_aggregate_mirror as E  # noqa: E402
from oracle import mvs_oracle as O  # noqa: E402

CSRC = os.path.join(ROOT, "mdf-net_amd", "csrc")
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def inp_of(cid):
    return cached(("inp", cid), lambda: E.inputs(cid))


def refs(cid, mode):
    """(float64 reference, fp32 restatement, e_32, t) of a case and mode, computed once."""
    def make():
        inp = inp_of(cid)
        r64, r32 = E.run_eval(inp, mode, torch.float64), E.run_eval(inp, mode, torch.float32)
        return r64, r32, E.distances_eval(r32, r64, mode), E.derived_t(inp, mode, r64, E.perturbed_runs(inp, mode))
    return cached(("refs", cid, mode), make)


def modes_of(cid):
    return ("vec", "pairdiff") + (("var",) if cid in E.VAR_CASES else ())


# ---------------------------------------------------------------------------------------------------------------- constants
def test_constants_are_the_sources():
    rd = lambda n: open(os.path.join(CSRC, n)).read()  # noqa: E731
    common, agg = rd("warp_common.h"), rd("warp_aggregate.hip")
    header = open(os.path.join(ROOT, "include", "mdfnet_hip.h")).read()
    num = lambda pat, s: int(re.search(pat, s).group(1))  # noqa: E731
    assert num(r"constexpr int kThreads = (\d+);", common) == E.K_THREADS
    assert num(r"#define MDF_MAX_SRC_VIEWS (\d+)", header) == E.MAX_SRC_VIEWS
    assert num(r"#define MDF_VEC8_TAB (\d+)", agg) == E.VEC8_TAB
    # launch<MODE> and launch_win: 512 entries; launch_vec8 and launch_pairdiff: MDF_VEC8_TAB; each clamped to [1, D]
    assert [int(x) for x in re.findall(r"int dch = (\d+) / \(p\.n_src \* ppb\);", agg)] == [E.WARP_TAB, E.WARP_TAB]
    assert len(re.findall(r"int dch = MDF_VEC8_TAB / \(p\.n_src \* ppb\);", agg)) == 2
    assert len(re.findall(r"if \(dch < 1\) dch = 1;\s*if \(dch > p\.D\) dch = p\.D;", agg)) == 4
    assert [int(x) * 1024 for x in re.findall(r"if \(lds > (\d+) \* 1024\) return MDF_EUNSUPPORTED;", agg)] == [E.LDS_LIMIT, E.LDS_LIMIT, E.WIN_LDS_LIMIT]
    assert num(r"int pool_kb = (\d+);", agg) == E.WIN_POOL_KB
    # sizeof(TapEntry) == sizeof(TapXY): four ints and four floats, 16-byte aligned
    assert re.search(r"struct __attribute__\(\(aligned\(16\)\)\) TapEntry \{\s*int off\[4\];[^\n]*\n\s*float wt\[4\];[^\n]*\n\};", common)
    assert re.search(r"struct __attribute__\(\(aligned\(16\)\)\) TapXY \{\s*int xa, xb, ya, yb;[^\n]*\n\s*float wt\[4\];\s*\n\};", common)
    assert 4 * 4 + 4 * 4 == E.TAP_ENTRY_BYTES
    assert len(re.findall(r"const size_t lds = \(size_t\)dch \* p\.n_src \* ppb \* sizeof\(TapEntry\);", agg)) == 3
    assert re.search(r"const size_t tab_bytes = \(size_t\)dch \* p\.n_src \* ppb \* sizeof\(TapXY\);\s*const size_t lds = tab_bytes \+ \(size_t\)pool_kb \* 1024;", agg)
    # pixels per block and pairs per thread of every kernel
    assert re.search(r"constexpr int ppb = kThreads / \(C / 8\);", agg) and re.search(r"constexpr int ppb = kThreads / \(G / GPL\);", agg)
    assert len(re.findall(r"constexpr int ppb = kThreads / \(C / 4\);", agg)) == 1 and re.search(r"const int lpp = C / 4, ppb = kThreads / lpp;", agg)
    assert len(re.findall(r"const FixedPairs<1, PPB> fp\(pt, p, b\);", agg)) == 1
    assert len(re.findall(r"const FixedPairs<2, PPB> fp\(pt, p, b(?:, FIXED)?\);", agg)) == 2
    assert re.search(r"return \(kThreads % npair\) == 0 \|\| \(NP == 2 && npair == 2 \* kThreads\);", common)
    assert re.search(r"ngrp = few \? kThreads / npair : 1;", common) and re.search(r"for \(int ed = grp; ed < nd; ed \+= ngrp\)", common)
    # the route rules of the two entry points
    assert re.search(r'env_int\("MDF_WARP_VEC8", 1\)', agg) and re.search(r'env_flag\("MDF_WARP_WINDOW", false\)', agg)
    assert re.search(r"if \(C == 64\) rc = launch_vec8<64>.*\n\s*else if \(C == 32\) rc = launch_vec8<32>.*\n\s*else if \(C == 16 && v8 == 2\) rc = launch_vec8<16>", agg)
    assert re.search(r'env_int\("MDF_PAIRDIFF_GPL", 4\) == 8 \? 8 : 4', agg)


# ---------------------------------------------------------------------------------------------------------------- routes
def test_table_reaches_every_route():
    """Every row of the issue's table yields the route it claims, and over the whole table every form occurs."""
    dims = {c: inp_of(c).dims for c in E.CASES}
    P = lambda cid, k, **kw: E.plan_eval(dims[cid], k, **kw)  # noqa: E731
    is_ = lambda p, form, ngrp=1: p.form == form and p.ngrp == ngrp and not p.refused  # noqa: E731
    # min: a map smaller than every tile, D = 1
    for k in E.KERNELS:
        p = P("min", k)
        assert p.nblk == 1 and p.dead_slots == p.ppb - 4 and p.chunks == [1], k
    # v16c64
    assert is_(P("v16c64", "vec8"), "two") and P("v16c64", "vec8").chunks == [2, 1]
    assert is_(P("v16c64", "warp_kernel"), "few", 1) and is_(P("v16c64", "pairdiff4"), "two")
    assert is_(P("v16c64", "pairdiff8"), "generic") and P("v16c64", "pairdiff8").dchunk == 1
    # v16c16
    assert is_(P("v16c16", "warp_kernel"), "generic") and P("v16c16", "warp_kernel").dchunk == 1
    assert P("v16c16", "vec8").lds == E.LDS_LIMIT and not P("v16c16", "vec8").refused and E.vec_route(dims["v16c16"], 2).kernel == "vec8"
    assert P("v16c16", "pairdiff8").refused and E.pairdiff_route(dims["v16c16"], 8).kernel == "pairdiff4"
    assert E.vec_route(dims["v16c16"], 1).kernel == "warp_kernel"                     # C = 16 takes 8 channels per lane only at VEC8 = 2
    # fix4c64
    p = P("fix4c64", "vec8")
    assert is_(p, "few", 2) and p.dchunk == 8 and p.chunks == [8] * 5 + [5] and p.short_last and p.ragged_groups
    # p4c32
    p = P("p4c32", "vec8")
    assert is_(p, "few", 1) and p.chunks == [4, 3] and p.short_last
    # p4c16
    assert is_(P("p4c16", "warp_kernel"), "few", 1) and is_(P("p4c16", "vec8"), "two") and is_(P("p4c16", "pairdiff4"), "two")
    assert is_(P("p4c16", "pairdiff8"), "generic") and P("p4c16", "pairdiff8").dchunk == 1
    # s2c16
    p = P("s2c16", "warp_kernel")
    assert is_(p, "few", 2) and p.dchunk == 4 and p.chunks == [4, 4, 1] and p.ragged_groups
    # gen3: generic everywhere, batch 2, ragged against every tile
    for k in E.KERNELS:
        assert is_(P("gen3", k), "generic") and P("gen3", k).dead_slots > 0, k
    assert dims["gen3"][0] == 2 and inp_of("gen3").hyp.shape == (2, 24, 13, 11)
    # n8c32, n5c64
    assert is_(P("n8c32", "vec8"), "two")
    assert all(is_(P("n5c64", k), "generic") for k in E.KERNELS)
    hyp = inp_of("n5c64").hyp
    assert hyp.shape == (2, 7, 1, 1) and not torch.equal(hyp[0], hyp[1]) and not inp_of("n5c64").per_pixel
    # the default routes: 8 channels per lane at C = 64 / 32, the 4-channel kernel at 16; the window kernel is never refused here
    for cid, d in dims.items():
        assert E.vec_route(d).kernel == ("warp_kernel" if d[1] == 16 else "vec8"), cid
        assert E.vec_route(d, 0).kernel == "warp_kernel" and E.vec_route(d, 2).kernel == "vec8" and E.vec_route(d, 1, True).kernel == "win", cid
        assert E.pairdiff_route(d, 4).kernel == "pairdiff4", cid
    # homo_warp is warp_kernel with one view: few with 16 / 8 / 4 thread groups
    assert [E.plan_eval(dims[c], "warp_kernel", n_src=1).ngrp for c in ("ident64", "mag32", "ident16")] == [16, 8, 4]
    # every form somewhere
    plans = [P(c, k) for c in E.CASES for k in E.KERNELS]
    plans = [p for p in plans if not p.refused]
    assert any(p.form == "few" and p.ngrp == 1 for p in plans) and any(p.form == "few" and p.ngrp > 1 for p in plans)
    assert any(p.form == "two" for p in plans) and any(p.form == "generic" for p in plans)
    assert any(p.dchunk == 1 and dims_d > 1 for p, dims_d in [(P(c, k), dims[c][3]) for c in E.CASES for k in E.KERNELS])
    assert any(p.short_last for p in plans) and any(p.form == "few" and p.ragged_groups for p in plans)
    assert any(E.plan_eval(d, "pairdiff8").refused for d in dims.values())
    # all three lane counts of softmax_pixel, 1 and 16 source views among the variance cases
    assert {dims[c][1] // 4 for c in E.VAR_CASES} == {4, 8, 16}
    assert {dims[c][6] for c in E.VAR_CASES} >= {1, 2, 3, 16}
    # plane independence straddles a chunk boundary of every kernel it is asked of
    for cid in ("fix4c64", "gen3"):
        for plan in (E.vec_route(dims[cid]), E.vec_route(dims[cid], 0), E.vec_route(dims[cid], 1, True), E.pairdiff_route(dims[cid], 4),
                     E.pairdiff_route(dims[cid], 8), E.plan_eval(dims[cid], "warp_kernel"), E.plan_eval(dims[cid], "warp_kernel", n_src=1)):
            a, b_ = E.straddling_planes(plan)
            assert 0 <= a < plan.dchunk < b_ < dims[cid][3] and a // plan.dchunk != (b_ - 1) // plan.dchunk, (cid, plan.kernel)
    # nothing is wider than 33 pixels
    assert all(max(d[4], d[5]) <= 33 for d in dims.values())


def test_exact_cases_sit_on_texels_and_half_texels():
    for ix, iy in E.positions(inp_of("ident64")):
        assert bool((ix == torch.round(ix)).all()) and bool((iy == torch.round(iy)).all())
    (ix0, iy0), (ix1, iy1) = E.positions(inp_of("half16"))
    assert bool(((ix0 - torch.floor(ix0)) == 0.5).all()) and bool((iy0 == torch.round(iy0)).all())
    assert bool(((ix1 - torch.floor(ix1)) == 0.5).all()) and bool(((iy1 - torch.floor(iy1)) == 0.5).all())
    assert float(ix0.max()) == 15.5 and float(ix1.min()) == -0.5 and float(iy1.min()) == -0.5      # out of frame by exactly one tap


@pytest.mark.parametrize("cid", list(E.CASES))
def test_no_sample_near_a_grid_line(cid):
    inp = inp_of(cid)
    if cid in E.EXACT_LINE_CASES:
        for ix, iy in E.positions(inp):
            for t in (ix, iy):
                assert bool(((t * 2) == torch.round(t * 2)).all())
        return
    assert not bool(E._near_lines(inp, E.GRID_MARGIN).any())
    assert M.grid_line_distance(inp) > E.GRID_MARGIN


@pytest.mark.parametrize("cid", list(E.CASES))
def test_the_head_is_live(cid):
    """Both branches of the head's ReLU occur and the per-view weights differ, so alpha, beta, w2, b2 and cw all reach the cost."""
    inp, r = inp_of(cid), refs(cid, "vec")[0]
    g, n_src = inp.dims[2], inp.dims[6]
    ok = ~torch.isnan(r.z)
    on = float((r.z[ok] * float(inp.wpar[g]) + float(inp.wpar[g + 1]) > 0).double().mean())
    spread = float(r.wv[ok].max() - r.wv[ok].min())
    print(f"{cid}: ReLU on for {on:.2f} of the samples, view weights spread {spread:.3f}, wpar tail {inp.wpar[g:].tolist()}")
    lo, hi, sp = E.HEAD_LIVE
    assert lo <= on <= hi
    assert spread >= sp or n_src == 1           # (one view: cost = sim whatever the weight)
    assert abs(float(inp.wpar[g])) > 0.05 and abs(float(inp.wpar[g + 2])) > 0.05 and bool((inp.wpar[g:].abs() < 4).all())   # O(1) factors


def test_nan_masks():
    """z0: exactly the z == 0 plane is NaN, in every mode and precision; `gone` (a view wholly out of frame) has none and a finite cost."""
    for mode in ("vec", "pairdiff", "var", "warp"):
        r64 = E.run_eval(inp_of("z0"), mode) if mode == "warp" else refs("z0", mode)[0]
        r32 = E.run_eval(inp_of("z0"), mode, torch.float32) if mode == "warp" else refs("z0", mode)[1]
        m = E.nan_mask(r64, mode)
        assert bool(m.any()) and not bool(m.all()) and torch.equal(m, E.nan_mask(r32, mode)), mode
        plane = m.reshape(1, -1, 5, 12, 20)[:, :, 1] if mode == "warp" else m[:, 1]
        assert bool(plane.all()) and int(m.sum()) == plane.numel(), mode
        if mode != "warp":
            assert not bool(E.nan_mask(refs("gone", mode)[0], mode).any()), mode
    g = E.run_eval(inp_of("gone"), "warp", torch.float32)
    assert bool(torch.isfinite(g.warp).all())
    inp = inp_of("gone")
    src1 = E.sample(inp.srcs[1], *E.positions(inp)[1])
    assert bool((src1 == 0).all())                                                      # zeros warped in
    # z < 0 planes (500: z = -100) give finite mirrored samples; the half-in-frame view has taps in and out of the frame
    ix, iy = E.positions(inp_of("z0"))[1]
    inside = (ix > 0) & (ix < 19) & (iy > 0) & (iy < 11)
    assert bool(inside.any()) and not bool(inside.all())


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("cid", E.REAL_CAMERA_CASES)
def test_fp32_restatement_against_the_oracle(cid):
    """run_eval(float32) against oracle.vector_aggregate / variance_aggregate over oracle.homo_warping_explicit, max |d| <= 1e-6: a sanity
    bound that ties the mirror to the oracle the goldens pin (both sides are fp32 CPU evaluations of one formula; the folded BatchNorm and
    the pair-difference blend round differently), no bar on any kernel."""
    inp = inp_of(cid)
    rp, sps = inp.cam
    feats = [inp.ref] + inp.srcs
    g = inp.dims[2]
    want = O.vector_aggregate(feats, rp, sps, inp.hyp, g, inp.head, warp=O.homo_warping_explicit).double().permute(0, 2, 3, 4, 1)
    for mode in ("vec", "pairdiff"):
        e = float((refs(cid, mode)[1].cost - want).abs().max())
        print(f"{cid} {mode} fp32 restatement vs fp32 oracle: {e:.2e}")
        assert e <= 1e-6, (mode, e)
    if cid in E.VAR_CASES:
        want = O.variance_aggregate(feats, rp, sps, inp.hyp, warp=O.homo_warping_explicit).double().permute(0, 2, 3, 4, 1)
        e = float((refs(cid, "var")[1].var - want).abs().max())
        print(f"{cid} var fp32 restatement vs fp32 oracle: {e:.2e}")
        assert e <= 1e-6, e


@pytest.mark.parametrize("cid", list(E.CASES))
def test_warp_restatement_is_the_explicit_warp_bit_for_bit(cid):
    """The reference the GPU test holds ops.homo_warp to, NaN positions included, is the mirror's own fp32 sample."""
    inp = inp_of(cid)
    eye, src4 = E.projections_4x4(inp)
    assert torch.equal(O.relative_projection(src4[0], eye)[:, :3, :4], inp.proj[0])
    want = O.homo_warping_explicit(inp.srcs[0], src4[0], eye, inp.hyp)
    got = E.run_eval(inp, "warp", torch.float32).warp
    assert np.array_equal(got.float().numpy(), want.numpy(), equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- the bar
def _with_wpar(inp, fn):
    out = copy.copy(inp)
    out.wpar = inp.wpar.clone()
    fn(out.wpar, inp.dims[2])
    return out


def _swap_ne_sw(monkeypatch):
    real = O.warp_corners

    def swapped(ix, iy, h, w):
        x0, y0, wts, masks = real(ix, iy, h, w)
        return x0, y0, (wts[0], wts[2], wts[1], wts[3]), masks
    monkeypatch.setattr(O, "warp_corners", swapped)


def _alpha_for_w2(wpar, g):
    wpar[g + 2] = wpar[g]


def _last_cw_zero(wpar, g):
    wpar[g - 1] = 0.0


FAULTS = ("ne_sw_swapped", "alpha_for_w2", "wsum_skips_a_view", "var_divisor", "last_cw_zero")


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("cid", ["gen3", "fix4c64"])
def test_the_bar_trips_on_a_deliberate_error(cid, fault, monkeypatch):
    """Each error, put into the fp32 restatement, exceeds 1.5 e_32 + t in at least one metric.  A bar that passes one is too loose."""
    inp = inp_of(cid)
    mode = "var" if fault == "var_divisor" else "vec"
    r64, _, e_32, t = refs(cid, mode)
    if fault == "ne_sw_swapped":
        _swap_ne_sw(monkeypatch)
        bad = E.run_eval(inp, mode, torch.float32)
    elif fault in ("alpha_for_w2", "last_cw_zero"):
        bad = E.run_eval(_with_wpar(inp, _alpha_for_w2 if fault == "alpha_for_w2" else _last_cw_zero), mode, torch.float32)
    else:
        bad = E.run_eval(inp, mode, torch.float32, fault=fault)
    e_bad = E.distances_eval(bad, r64, mode)
    fails = E.judge(e_bad, e_32, t)
    print(f"{cid} {fault}: " + ", ".join(f"{k} {v:.2e} (bar {1.5 * e_32[k] + t[k]:.2e})" for k, v in e_bad.items()))
    assert fails, (cid, fault, e_bad)
    assert torch.equal(E.nan_mask(bad, mode), E.nan_mask(r64, mode))


@pytest.mark.parametrize("cid", list(E.CASES))
def test_the_restatement_passes_and_the_bar_is_no_looser_than_2e_6(cid):
    """The unmodified restatement holds its own bar, and on the cases with real cameras e_32 + t < 2e-6 in the max metric: the bar is
    never looser than the atol the golden tests hold next to it."""
    for mode in modes_of(cid):
        r64, r32, e_32, t = refs(cid, mode)
        assert not E.judge(e_32, e_32, t)
        assert torch.equal(E.nan_mask(r32, mode), E.nan_mask(r64, mode))
        print(f"{cid} {mode}: " + ", ".join(f"{k}: e_32 {e_32[k]:.2e} t {t[k]:.2e}" for k in e_32))
        assert all(v > 0 for v in t.values())
        if cid in E.REAL_CAMERA_CASES:
            assert e_32["max"] + t["max"] < 2e-6, (mode, e_32["max"], t["max"])
