"""CPU: the conditions tests/test_aggregate_train_gpu.py relies on -- the references of tests/aggregate_mirror.py against the oracle's
autograd runs (oracle/train_check.py), the case table's reach over every launch route of the training aggregation, the grid-line margin
of every sample, and the mirror's constants against the kernel sources.  No GPU.  If a case misses a condition, the case changes."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import aggregate_mirror as M  # noqa: E402
from oracle import train_check as TC  # noqa: E402

CSRC = os.path.join(ROOT, "mdf-net_amd", "csrc")
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def inp_of(cid):
    return cached(("inp", cid), lambda: M.inputs(cid))


def routes_of(cid):
    return cached(("routes", cid), lambda: M.scatter_routes(inp_of(cid)))


def plans_of(cid):
    inp = inp_of(cid)
    return M.plan_train(inp.dims, inp.per_pixel), M.plan_bwd(inp.dims, inp.per_pixel)


def _oracle(cid, dtype):
    inp = inp_of(cid)
    b, c, g, d, h, w, n_src = inp.dims
    sd = {"depth_weight.0.conv.weight": inp.cw.reshape(1, g, 1, 1, 1), "depth_weight.0.bn.weight": inp.gamma, "depth_weight.0.bn.bias": inp.beta,
          "depth_weight.0.bn.running_mean": inp.rmean, "depth_weight.0.bn.running_var": inp.rvar,
          "depth_weight.0.bn.num_batches_tracked": torch.zeros((), dtype=torch.int64),
          "depth_weight.1.weight": inp.w2.reshape(1, 1, 1, 1, 1), "depth_weight.1.bias": inp.b2}
    rp, sps = inp.cam
    r = TC.aggregate(sd, g, [inp.ref] + inp.srcs, rp, sps, inp.hyp, inp.dcost, dtype)
    nhwc = lambda x: x.detach().double().permute(0, 2, 3, 1).contiguous()  # noqa: E731
    gr = r["grads"]
    return {"cost": r["cost"].double().permute(0, 2, 3, 4, 1).contiguous(), "dref": nhwc(r["dfeats"][0]),
            "dsrc": torch.stack([nhwc(t) for t in r["dfeats"][1:]]), "dcw": gr["depth_weight.0.conv.weight"].double().reshape(-1),
            "dpar": torch.stack([gr["depth_weight.0.bn.weight"].double()[0], gr["depth_weight.0.bn.bias"].double()[0],
                                 gr["depth_weight.1.weight"].double().reshape(-1)[0], gr["depth_weight.1.bias"].double()[0]]),
            "rmean": float(r["buffers"]["depth_weight.0.bn.running_mean"]), "rvar": float(r["buffers"]["depth_weight.0.bn.running_var"])}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


# printed by the two tests below on the development machine (torch 2.x CPU), the worst over the cases with real cameras and more than
# one source view; the bars are these values times 2
RESTATEMENT_FP32 = {"dref": 0.0, "dsrc": 5.5e-7, "dcw": 0.0, "dpar": 0.0}
POSITION_ROUNDING_F64 = {"cost": 4.0e-6, "dref": 3.9e-6, "dsrc": 3.0e-6, "dcw": 5.2e-6, "dpar": 5.8e-6}


@pytest.mark.parametrize("cid", M.REAL_CAMERA_CASES)
def test_fp32_restatement_is_the_fp32_oracle(cid):
    """run(inp, float32) against oracle.train_check.aggregate(..., float32).  Forward: BIT FOR BIT (the explicit warp is bit-identical
    to grid_sample, tests/test_oracle_golden.py, and everything behind it is the same ATen call).  Gradients: summation-order noise
    (grid_sample's backward scatters in another order than gather's): the worst max-rel difference printed here was d src 5.5e-7, and
    0 -- bit for bit -- for d ref, d conv weight and the head scalars, which never pass the scatter (RESTATEMENT_FP32); the bar is twice that."""
    got, want = cached(("r32", cid), lambda: M.run(inp_of(cid), torch.float32)), _oracle(cid, torch.float32)
    inp = inp_of(cid)
    bitwise = all(torch.equal(M.warp_at(s, *pos), M.O.homo_warping(s, sp, inp.cam[0], inp.hyp))
                  for s, pos, sp in zip(inp.srcs, M.positions(inp), inp.cam[1]))
    # a 7-wide map takes the scalar tail of ATen's vectorised grid_sample, which does not contract the unnormalisation into an FMA:
    # its positions are another rounding of the same numbers, and the comparison is the position-rounding one of the float64 test
    assert bitwise or cid == "v16"
    if not bitwise:
        for k, bar in POSITION_ROUNDING_F64.items():
            assert _rel(getattr(got, k), want[k]) <= 2 * bar, k
        return
    assert torch.equal(got.cost, want["cost"]), f"cost differs by {_rel(got.cost, want['cost']):.2e}"
    assert abs(got.rmean - want["rmean"]) <= 1e-6 * abs(want["rmean"]) and abs(got.rvar - want["rvar"]) <= 1e-6 * abs(want["rvar"])
    if inp_of(cid).dims[6] == 1:
        return      # one view: the head's gradients are rounding noise of a zero (aggregate_mirror.one_view_bounds)
    for k, bar in RESTATEMENT_FP32.items():
        e = _rel(getattr(got, k), want[k])
        print(f"{cid} fp32 restatement vs fp32 oracle {k}: {e:.2e}")
        assert e <= 2 * bar, (k, e)


@pytest.mark.parametrize("cid", M.REAL_CAMERA_CASES)
def test_float64_reference_is_the_float64_oracle_up_to_position_rounding(cid):
    """run(inp, float64) samples at the fp32 positions, the oracle's float64 run at float64 positions: they differ by the rounding of
    ix, iy (half an fp32 ulp of a coordinate of a few pixels, ~1e-7, times the feature slope) and nothing else.  Worst printed:
    cost 4.0e-6 (s2), d ref 3.9e-6, d src 3.0e-6, d conv weight 5.2e-6, head scalars 5.8e-6 (POSITION_ROUNDING_F64); the bar is twice that."""
    got, want = cached(("r64", cid), lambda: M.run(inp_of(cid), torch.float64)), _oracle(cid, torch.float64)
    for k, bar in POSITION_ROUNDING_F64.items():
        if inp_of(cid).dims[6] == 1 and k in ("dcw", "dpar"):
            continue
        e = _rel(getattr(got, k), want[k])
        print(f"{cid} float64 reference vs float64 oracle {k}: {e:.2e}")
        assert e <= 2 * bar, (k, e)


def test_reference_is_self_consistent():
    """The reductions the kernels form (S1, S2, d w2, d b2) are autograd's d beta, d gamma, d w2, d b2; A bounds |d|."""
    for cid in ("gen3", "half64", "mag32"):
        r = cached(("r64", cid), lambda: M.run(inp_of(cid), torch.float64))
        n_src = r.dims[6]
        want = torch.stack([r.red2[1:2 * n_src:2].sum(), r.red2[0:2 * n_src:2].sum(), r.red2[2 * n_src], r.red2[2 * n_src + 1]])
        assert _rel(want, r.dpar) < 1e-10
        assert bool((r.dsrc.abs() <= r.a_src * (1 + 1e-12) + 1e-300).all()) and bool((r.dref.abs() <= r.a_ref * (1 + 1e-9) + 1e-12).all())
        assert bool((r.dcw.abs() <= r.a_dcw * (1 + 1e-12)).all())
        live, _ = M.live_texels(inp_of(cid))
        assert bool((r.a_src[~live.unsqueeze(-1).expand_as(r.a_src)] == 0).all())
        c64, _, _ = M.finalize_mirror(r.red0, inp_of(cid).gamma, inp_of(cid).beta, r.n, inp_of(cid).rmean, inp_of(cid).rvar)
        assert _rel(c64, r.consts) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- routes
def test_table_reaches_every_route():
    ids = list(M.CASES)
    dims = {c: inp_of(c).dims for c in ids}                        # (b, c, g, d, h, w, n_src)
    pt = {c: plans_of(c)[0] for c in ids}
    pb = {c: plans_of(c)[1] for c in ids}
    rec = {c: routes_of(c) for c in ids}
    # tiles with dead slots; C = 16 (64 pixels per tile) on a map smaller than a tile
    assert pt["min"].dead_slots == 12 and pt["min"].ppb == 16
    assert pt["v16"].ppb == 64 and dims["v16"][4] * dims["v16"][5] == 35 and pt["v16"].grid[0] == 1
    # (f) 1 and 16 source views; at 16: nred = KMAX = 34, all 64 threads fill bb and prepare, one plane per chunk
    assert dims["min"][6] == 1 and dims["v16"][6] == M.MAX_SRC_VIEWS
    assert pt["v16"].nred[1] == 2 * M.MAX_SRC_VIEWS + 2 == 34 and pt["v16"].bb_threads == 64 and pt["v16"].dchunk == 1 and pb["v16"].dchunk == 1
    # (e) fixed-pair fill with more thread groups than planes, exactly as many, one group; the generic fill
    assert pt["ident64"].fixed and pt["ident64"].ngrp == 8 and set(pt["ident64"].chunks) == {5}          # ngrp > nd
    assert pt["min"].fixed and pt["min"].ngrp == 16 and pt["min"].chunks == [1]                          # ngrp > nd
    assert pt["fix4"].fixed and pt["fix4"].ngrp == 4 and set(pt["fix4"].chunks) == {4}                   # ngrp == nd
    assert pt["s2"].fixed and pt["s2"].ngrp == 2 and set(pt["s2"].chunks) == {4}                         # 2 groups, ngrp < nd
    assert pt["grp1"].fixed and pt["grp1"].ngrp == 1                                                      # ngrp == 1
    assert not pt["gen3"].fixed and not pt["v16"].fixed and not pt["d9"].fixed                           # generic fill
    assert dims["gen3"][1:] == dims["d9"][1:3] + (24,) + dims["d9"][4:]                                  # ... at the same shape but D
    # (d) depth slices: gridDim.z == 1 and > 1 for both launchers, a ragged last slice
    for plan in (pt, pb):
        assert plan["d7"].grid[2] == 1 and plan["min"].grid[2] == 1
        assert plan["fix4"].grid[2] == 12 and plan["fix4"].dslice == 4 and plan["gen3"].grid[2] == 6
        assert plan["d9"].grid[2] == 2 and plan["d9"].dslice == 5 and plan["d9"].ragged                  # 5 + 4
    assert not pt["fix4"].ragged
    # hypothesis layouts at batch 2
    assert dims["fix4"][0] == 2 and not inp_of("fix4").per_pixel and inp_of("fix4").hyp.shape == (2, 48, 1, 1)
    assert dims["gen3"][0] == 2 and inp_of("gen3").per_pixel and inp_of("gen3").hyp.shape == (2, 24, 13, 11)
    assert not torch.equal(inp_of("fix4").hyp[0], inp_of("fix4").hyp[1])
    # per-view tap tables (per-pixel hypotheses) and per-chunk ones
    assert pb["gen3"].nv == 1 and pb["gen3"].dstep == 12 and pb["fix4"].nv == 4
    # s2: the last tile column of the scatter has one live pixel column
    assert dims["s2"][5] % pb["s2"].tw == 1 and dims["s2"][5] % pt["s2"].ppb != 0
    # (a) window tiles and direct-to-memory tiles in ONE launch, per C
    for cid, c in (("mag64", 64), ("mag32", 32), ("mag16", 16)):
        assert dims[cid][1] == c and pb[cid].win_texels == 8192 // c
        assert any(r.window for r in rec[cid]) and any(r.any and not r.window for r in rec[cid]), cid
    # (b) >= 8 pixels of a tile on one (xa, ya) in one plane; exactly 2
    assert max(r.share for r in rec["mini16"]) >= 8 and max(r.share for r in rec["mini64"]) >= 8
    assert max(r.share for r in rec["mag64"]) == 2
    # (c) a view without a live tap anywhere next to a view with live taps, in one call
    assert all(not r.any for r in rec["gone"] if r.view == 1) and any(r.window for r in rec["gone"] if r.view == 0)
    assert not M.live_texels(inp_of("gone"))[0][1].any()
    # clamped corner sets (the atomic branch), in-bounds taps of weight exactly 0, a pixel's planes all on one corner set
    for cid in ("ident16", "ident64", "half16", "half64"):
        assert any(r.clamped for r in rec[cid]) and any(r.zero_w for r in rec[cid]) and all(r.one_flush for r in rec[cid]), cid
        assert all(r.window for r in rec[cid])
    assert all(r.one_flush for r in rec["mini64"])
    # ident: every sample exactly on a texel; half: exactly +-0.5
    for ix, iy in M.positions(inp_of("ident16")):
        assert bool((ix == torch.round(ix)).all()) and bool((iy == torch.round(iy)).all())
    (ix0, iy0), (ix1, iy1) = M.positions(inp_of("half64"))
    assert bool(((ix0 - torch.floor(ix0)) == 0.5).all()) and bool((iy0 == torch.round(iy0)).all())
    assert bool(((ix1 - torch.floor(ix1)) == 0.5).all()) and bool(((iy1 - torch.floor(iy1)) == 0.5).all())
    assert float(ix0.max()) == 15.5 and float(ix1.min()) == -0.5                                         # xa clamped at either border
    # nothing is larger than 23 x 23 texels per map side ... except s2's 33-wide row, which the issue's table sets
    assert all(max(d[4], d[5]) <= 23 or c in ("s2", "gone") for c, d in dims.items())


def test_forced_geometry_of_the_children():
    """MDF_WARP_*_TAB=64 with *_BLOCKS=1: one-plane chunks and ONE slice (fix4's 48 planes included: the direct d ref store);
    *_BLOCKS=1048576: D/4 slices."""
    for cid in M.REDUCED_CASES:
        inp = inp_of(cid)
        d = inp.dims[3]
        a, b_ = M.plan_train(inp.dims, inp.per_pixel, tab=64, target=1), M.plan_bwd(inp.dims, inp.per_pixel, tab=64, target=1)
        one = 1 if cid != "mag64" else 2                 # 64 table entries: one plane of n_src x PPB pairs (mag64: 2 x 16 pairs, two)
        assert a.grid[2] == 1 and b_.grid[2] == 1 and a.dchunk == one and b_.dchunk == one, cid
        a, b_ = M.plan_train(inp.dims, inp.per_pixel, target=1 << 20), M.plan_bwd(inp.dims, inp.per_pixel, target=1 << 20)
        assert a.grid[2] == b_.grid[2] == max(1, d // 4) and a.dslice == b_.dslice == (4 if d % 4 == 0 else 5), cid


@pytest.mark.parametrize("cid", list(M.CASES))
def test_no_sample_near_a_grid_line(cid):
    """Index-like decisions (floor) must not hinge on the last bit: every sample with a tap in the frame keeps GRID_MARGIN from the
    pixel-grid lines, except in the cases that put samples exactly on lines on purpose (and there every coordinate is exact)."""
    inp = inp_of(cid)
    if cid in M.EXACT_LINE_CASES:
        for ix, iy in M.positions(inp):
            for t in (ix, iy):
                assert bool(((t * 2) == torch.round(t * 2)).all())
        return
    assert M.grid_line_distance(inp) > M.GRID_MARGIN


def test_constants_are_the_sources():
    rd = lambda n: open(os.path.join(CSRC, n)).read()  # noqa: E731
    common, scatter, train = rd("warp_common.h"), rd("warp_scatter.h"), rd("warp_aggregate_train.hip")
    header = open(os.path.join(ROOT, "include", "mdfnet_hip.h")).read()
    num = lambda pat, s: int(re.search(pat, s).group(1))  # noqa: E731
    assert num(r"constexpr int kThreads = (\d+);", common) == M.K_THREADS
    assert num(r"#define MDF_BWD_WIN_FLOATS (\d+)", scatter) == M.WIN_FLOATS
    assert num(r"#define MDF_MAX_SRC_VIEWS (\d+)", header) == M.MAX_SRC_VIEWS
    assert num(r"using BwdTile = PixTile<kThreads / \(C / 4\), (\d+)>;", scatter) == M.SCATTER_TILE_ROWS
    assert num(r"if \(nz > p\.D / (\d+)\) nz = p\.D / \1;", scatter) == M.MIN_PLANES_PER_SLICE
    assert num(r'env_pos\("MDF_WARP_TRAIN_TAB", (\d+)\)', train) == M.TRAIN_TAB
    pair = lambda pat: tuple(int(x) for x in re.search(pat, train).groups())  # noqa: E731
    assert pair(r"tab_env \? tab_env : \(p\.hypos_per_pixel \? (\d+) : (\d+)\)") == (M.BWD_TAB[True], M.BWD_TAB[False])
    targets = re.findall(r"target_env \? target_env : \(p\.hypos_per_pixel \? (\d+) : (\d+)\)", train)
    assert [tuple(int(x) for x in t) for t in targets] == [(M.BWD_TARGET[True], M.BWD_TARGET[False]), (M.TRAIN_TARGET[True], M.TRAIN_TARGET[False])]
    assert re.search(r"use = any && \(\(long long\)ww \* wh \* T <= kWinFloats\);", scatter)
    assert re.search(r"return \(kThreads % npair\) == 0 \|\| \(NP == 2 && npair == 2 \* kThreads\);", common)
    assert re.search(r"constexpr int KMAX = 2 \* MDF_MAX_SRC_VIEWS \+ 2;", train)
    assert re.search(r"sizeof\(TapXY\) \+ \(size_t\)kWinFloats \* sizeof\(float\)", train)
