"""GPU parity of the weight-gradient family (csrc/wgrad.hip, csrc/wgrad_lds.hip) with the float64 reference of tests/wgrad_mirror.py,
through the C ABI, at edge shapes and tile walks.

Exact arithmetic.  The inputs of the first pass are fp32 integers of {-3 .. 3}: every product and every partial sum is an fp32 value
(9 * voxels < 2^24, asserted in tests/test_wgrad_mirror_cpu.py), whatever the order -- MFMA chains, LDS partial sums, slabs, fp32 atomics.
The kernels owe the reference BIT FOR BIT: one dropped, duplicated or misplaced voxel changes an integer.  A second pass runs the same
cases with randn inputs against the same reference at the bar the family's tests hold (max|got - ref| / max|ref| < 3e-5) and prints
the worst value per layer kind.

Every call fills the workspace and dw with NaN first: an unwritten slab element or an un-cleared gradient shows up.

Routes.  mdf_wgrad_last_plan tells which kernel form and tiling a shape took; test_table_reaches_every_route asserts that the table
still holds a case for every path it was chosen for, so that a retune of the host code cannot move the shapes off them unnoticed.

Run as a program (`python tests/test_wgrad_gpu.py --child`) the file checks the reduced table in a fresh process: the direct forms sit
behind MDF_WGRAD_LDS=0 / MDF_WGRAD_PACK=0, which the library reads once per process."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import wgrad_mirror as M  # noqa: E402
from mdfnet_hip import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FIELDS = ("form", "R", "TH", "tv", "n_tiles", "gx", "gy", "gz", "split")
LDS, DIRECT3D, A1_MFMA, A1_VALU, DIRECT2D = 0, 1, 2, 3, 4


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_plan():
    out = (ctypes.c_int * len(FIELDS))()
    assert lib().mdf_wgrad_last_plan(out, len(FIELDS)) == len(FIELDS)
    return dict(zip(FIELDS, out))


def _dims(case):
    """(entry suffix, n = dw.numel(), workspace floats, the ints between the pointers and the trailing arguments)"""
    three_d, kind, a, bc, shape = case
    s, k = M.stride_ksize(three_d, kind)
    L = lib()
    if three_d:
        return "conv3d", a * bc * 27, L.mdf_conv3d_wgrad_workspace(*shape, a, bc), tuple(shape) + (a, bc, s)
    return "conv2d", a * bc * k * k, L.mdf_conv2d_wgrad_workspace(*shape, a, bc, k), tuple(shape) + (a, bc, k, s)


def dw_shape(case):
    three_d, kind, a, bc, _ = case
    _, k = M.stride_ksize(three_d, kind)
    return (a, bc) + (k,) * (3 if three_d else 2)


def call_partial(case, small, big):
    """mdf_conv*_wgrad_partial on NaN-filled workspace and dw -> (workspace, dw, nslab, n).  Asynchronous (or only recorded)."""
    name, n, nwork, ints = _dims(case)
    assert nwork >= n
    work = torch.full((nwork,), NAN, device=DEV)
    dw = torch.full((n,), NAN, device=DEV)
    ns = ctypes.c_int(0)
    entry = f"mdf_{name}_wgrad_partial"
    check(getattr(lib(), entry)(small.data_ptr(), big.data_ptr(), dw.data_ptr(), work.data_ptr(), *ints, ctypes.byref(ns), _stream()), entry)
    assert 1 <= ns.value and ns.value * n <= nwork, (ns.value, n, nwork)
    return work, dw, ns.value, n


def slab_sum(case, work, dw, nslab, n):
    """The three checks of a partial call; returns the slab sum in torch's weight layout (CPU, fp32)."""
    assert not bool(dw.any()) and not bool(dw.isnan().any()), f"{M.case_id(case)}: dw is not cleared"
    slabs = work[:nslab * n].view(nslab, n)
    bad = int(slabs.isnan().sum())
    assert bad == 0, f"{M.case_id(case)}: {bad} of {nslab} x {n} slab elements were never written"
    return slabs.sum(0).reshape(dw_shape(case)).cpu()


def run_partial(case, small, big):
    small, big = small.to(DEV), big.to(DEV)
    work, dw, nslab, n = call_partial(case, small, big)
    plan = last_plan()
    torch.cuda.synchronize()
    assert plan["gx"] == nslab
    return slab_sum(case, work, dw, nslab, n), plan


def exact_mismatch(case, got, ref):
    """'' when got equals ref bit for bit, else a description of the first differing elements."""
    if got.dtype == torch.float32 and torch.equal(got.double(), ref):
        return ""
    bad = (got.double() != ref).nonzero()
    first = ", ".join(f"{tuple(i.tolist())}: got {float(got[tuple(i)])} ref {float(ref[tuple(i)])}" for i in bad[:4])
    return f"{M.case_id(case)}: {len(bad)} of {ref.numel()} elements differ; {first}"


def randn_error(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- the table
_RESULTS = {}


def result(case):
    """Both passes of one table case, run once per process: (plan, mismatch text of the integer pass, randn error)."""
    if case not in _RESULTS:
        small, big = M.int_inputs(case)
        got, plan = run_partial(case, small, big)
        bad = exact_mismatch(case, got, M.ref_of(case, small, big))
        small, big = M.randn_inputs(case)
        got, plan_r = run_partial(case, small, big)
        assert plan_r == plan
        _RESULTS[case] = (plan, bad, randn_error(got, M.ref_of(case, small, big)))
    return _RESULTS[case]


def kind_of(case):
    return f"{'3d' if case[0] else '2d'}-{case[1]}"


@pytest.mark.parametrize("case", M.all_cases(), ids=M.case_id)
def test_partial_tiles_sum_to_the_reference(case):
    plan, bad, err = result(case)
    print(f"{M.case_id(case)}: {plan} randn max|d|/max|ref| = {err:.2e}")
    assert not bad, (bad, plan)
    assert err < M.RANDN_BAR, (err, plan)


def test_table_reaches_every_route():
    """Existence over the table, from what the host code decided -- not from what the table was written for.

    The last condition of the sweep reads `W one voxel past a tile boundary` (W % tv == 1, W > tv: the row's last tile holds a single
    voxel).  The literal `W == tv + 1` cannot be had from the dispatch: it picks the tile width that wastes the fewest voxels, and for
    a row of tv + 1 voxels a narrower tile always wins (no width from 1 to 700 gives it for any sweep kind)."""
    plans = [(c, result(c)[0]) for c in M.all_cases()]
    lds3 = [(c, p) for c, p in plans if c[0] and p["form"] == LDS]
    lds2 = [(c, p) for c, p in plans if not c[0] and p["form"] == LDS]
    assert any(p["TH"] == 2 and c[4][2] % 2 == 1 and c[4][2] > 1 for c, p in lds3), "two-row tiles with an odd height"
    assert any(p["TH"] == 1 and M.stride_ksize(True, c[1])[0] == 2 for c, p in lds3), "one-row tiles in 3-D (stride 2)"
    for r in (0, 1, 2):
        assert any(p["R"] == r for _, p in lds3), f"tap packing R = {r} in 3-D"
        assert any(p["R"] == r for _, p in lds2), f"tap packing R = {r} in 2-D"
    for split in (1, 2, 4):
        assert any(p["split"] == split for _, p in lds3 + lds2), f"wave split {split}"
    assert any(p["n_tiles"] > p["gx"] and p["n_tiles"] % p["gx"] != 0 and c[4][0] > 1 and c[4][1] >= 3 for c, p in lds3), \
        "a tile walk across images and dead kd planes"
    for form in (A1_MFMA, A1_VALU, DIRECT2D):
        assert any(p["form"] == form for _, p in plans), f"kernel form {form}"
    sweep = [(c[4][-1], result(c)[0]) for c in M.sweep_cases()]
    assert all(p["form"] == LDS for _, p in sweep)
    assert any(w % p["tv"] == 0 for w, p in sweep), "a row that is a whole number of tiles"
    assert any(w % p["tv"] == 1 and w > p["tv"] for w, p in sweep), "a row one voxel past a tile boundary"
    assert any(w < p["tv"] for w, p in sweep), "a row narrower than a tile"
    # every plan is self-consistent: the blocks cover the tiles, the slabs fit the workspace
    for c, p in plans:
        assert 1 <= p["gx"] and p["gz"] in (1, 3, 5) and p["split"] in (1, 2, 4) and p["n_tiles"] >= 1, (c, p)
        if p["form"] == LDS:
            assert p["tv"] % 16 == 0 and p["TH"] in (1, 2) and p["gx"] <= p["n_tiles"], (c, p)


def test_worst_randn_error_per_layer_kind():
    worst = {}
    for c in M.all_cases():
        err = result(c)[2]
        if err > worst.get(kind_of(c), (-1.0, None))[0]:
            worst[kind_of(c)] = (err, c)
    for k, (err, c) in sorted(worst.items()):
        print(f"worst randn max|got - ref| / max|ref|, {k}: {err:.2e} at {M.case_id(c)}")
        assert err < M.RANDN_BAR


# ---------------------------------------------------------------------------------------------------------------- complete entries
FULL_CASES = [(True, "conv_s1", 64, 64, (2, 5, 9, 20)), (True, "conv_s2", 32, 16, (2, 3, 5, 17)), (True, "prob_s1", 1, 8, (2, 3, 5, 17)),
              (False, "k3_s1", 8, 8, (3, 9, 70)), (False, "k5_s2", 32, 16, (2, 5, 17)), (False, "k1", 64, 32, (1, 7, 33))]


@pytest.mark.parametrize("case", FULL_CASES, ids=M.case_id)
def test_complete_entries_overwrite_and_accumulate(case):
    """mdf_conv3d_wgrad / mdf_conv2d_wgrad (kernel + slab sum): accumulate = 0 overwrites a NaN-filled dw, accumulate = 1 adds to an
    integer-filled one.  Exact: |old + ref| <= 3 + 9 * voxels < 2^24."""
    name, n, nwork, ints = _dims(case)
    small, big = M.int_inputs(case, salt=5)
    ref = M.ref_of(case, small, big)
    small, big = small.to(DEV), big.to(DEV)
    entry = getattr(lib(), f"mdf_{name}_wgrad")
    g = torch.Generator().manual_seed(n)
    old = torch.randint(-3, 4, (n,), generator=g).float()
    for accumulate, start, want in ((0, torch.full((n,), NAN), ref), (1, old, old.double().reshape(ref.shape) + ref)):
        work = torch.full((nwork,), NAN, device=DEV)
        dw = start.to(DEV)
        check(entry(small.data_ptr(), big.data_ptr(), dw.data_ptr(), work.data_ptr(), *ints, accumulate, _stream()), f"mdf_{name}_wgrad")
        torch.cuda.synchronize()
        bad = exact_mismatch(case, dw.reshape(dw_shape(case)).cpu(), want)
        assert not bad, (accumulate, bad, last_plan())


# ---------------------------------------------------------------------------------------------------------------- slab sums
def test_sum_batch_across_the_launch_boundary():
    """mdf_wgrad_sum_batch on synthetic integer slabs: 100 jobs in one call (a launch takes 96), slab counts on both sides of every
    slice count (gys = nslab / 8 clamped to 1 .. 32) with odd and even trips of the two-accumulator loop, element counts around the
    256-element chunk.  Outputs start as integers, so the += is visible.  |sums| <= 3 + 3 * 300: exact."""
    nslabs_of = [1, 7, 8, 9, 15, 16, 17, 300]
    ns_of = [1, 255, 256, 257, 27 * 64 * 64]
    njobs = 100
    torch.manual_seed(11)
    slabs, outs, olds, nslab, n = [], [], [], [], []
    for j in range(njobs):
        nslab.append(nslabs_of[j % 8])
        n.append(ns_of[(j // 8 + j) % 5])
        slabs.append(torch.randint(-3, 4, (nslab[-1], n[-1]), device=DEV, dtype=torch.int32))
        olds.append(torch.randint(-3, 4, (n[-1],), device=DEV, dtype=torch.int32))
        outs.append(olds[-1].float())
    assert {(a, b) for a, b in zip(nslab, n)} == {(a, b) for a in nslabs_of for b in ns_of}          # every pairing
    fslabs = [s.float() for s in slabs]
    ptr = lambda ts: (ctypes.c_void_p * njobs)(*[t.data_ptr() for t in ts])
    ints = lambda v: (ctypes.c_int * njobs)(*v)
    check(lib().mdf_wgrad_sum_batch(ptr(fslabs), ptr(outs), ints(nslab), ints(n), njobs, _stream()), "mdf_wgrad_sum_batch")
    torch.cuda.synchronize()
    for j in range(njobs):
        want = (slabs[j].sum(0, dtype=torch.int64) + olds[j]).double()
        assert torch.equal(outs[j].double(), want), (j, nslab[j], n[j], int((outs[j].double() != want).sum()))


# ---------------------------------------------------------------------------------------------------------------- job-table launch
@pytest.mark.parametrize("zfast", [None, "0"], ids=["zfast_default", "zfast_0"])
@pytest.mark.parametrize("shape,blocks", [((3, 2, 2, 2), "below 8"), ((1, 2, 7, 33), "8"), ((2, 3, 5, 17), "above 8, no multiple")],
                         ids=["3x2x2x2", "1x2x7x33", "2x3x5x17"])
def test_job_table_launch_past_its_capacity(shape, blocks, zfast, monkeypatch):
    """25 same-shape 16 x 16 stride-1 jobs and three jobs of other kernel instantiations between mdf_wgrad_batch_begin and the flush:
    one instantiation takes 22 jobs per launch, so the 23rd to 25th travel in a second one.  gx * gy of the repeated job is below 8,
    8, and above 8 without being a multiple of it (the z-fast renumbering works in groups of 8 blocks plus a tail); with
    MDF_WGRAD_ZFAST unset and 0 (read per flush).  Every job has its own integer data and is exact."""
    if zfast is None:
        monkeypatch.delenv("MDF_WGRAD_ZFAST", raising=False)
    else:
        monkeypatch.setenv("MDF_WGRAD_ZFAST", zfast)
    main = (True, "conv_s1", 16, 16, shape)
    others = [(True, "conv_s1", 8, 8, (2, 3, 5, 17)), (True, "conv_s2", 32, 16, (1, 2, 7, 33)), (False, "k5_s2", 32, 16, (2, 5, 17))]
    cases = [main] * 11 + others[:1] + [main] * 11 + others[1:2] + [main] * 3 + others[2:]
    assert cases.count(main) == 25
    L = lib()
    jobs, plans = [], []
    check(L.mdf_wgrad_batch_begin(), "mdf_wgrad_batch_begin")
    try:
        for j, case in enumerate(cases):
            small, big = M.int_inputs(case, salt=j + 1)
            ds, db = small.to(DEV), big.to(DEV)
            jobs.append((case, small, big, ds, db) + call_partial(case, ds, db))
            plans.append(last_plan())
        torch.cuda.synchronize()
        assert all(bool(j[5].isnan().all()) for j in jobs), "recorded jobs must not have launched"
    finally:
        rc = L.mdf_wgrad_batch_flush(_stream())
    check(rc, "mdf_wgrad_batch_flush")
    torch.cuda.synchronize()
    assert all(p["form"] == LDS for p in plans)
    keys = {(c[0], M.stride_ksize(c[0], c[1])[1], p["R"], p["TH"]) for c, p in zip(cases, plans)}
    assert len(keys) == 4, keys                                      # four kernel instantiations: the 25, and one each
    g = plans[0]["gx"] * plans[0]["gy"]
    assert {"below 8": g < 8, "8": g == 8, "above 8, no multiple": g > 8 and g % 8 != 0}[blocks], plans[0]
    for j, (case, small, big, _, _, work, dw, nslab, n) in enumerate(jobs):
        bad = exact_mismatch(case, slab_sum(case, work, dw, nslab, n), M.ref_of(case, small, big))
        assert not bad, (j, bad, plans[j])


# ---------------------------------------------------------------------------------------------------------------- direct forms
def child_main():
    """The reduced table in this process, under whatever MDF_WGRAD_* the parent set: prints every failure, exit status 1 if any."""
    lds_off = os.environ.get("MDF_WGRAD_LDS") == "0"
    pack_off = os.environ.get("MDF_WGRAD_PACK") == "0"
    failures, forms = [], set()
    for case in M.reduced_cases():
        try:
            plan, bad, err = result(case)
        except Exception as e:  # noqa: BLE001  (an assertion of the three checks, or a failed call)
            failures.append(f"{M.case_id(case)}: {type(e).__name__}: {e}")
            continue
        forms.add(plan["form"])
        if bad:
            failures.append(f"{bad} {plan}")
        if not err < M.RANDN_BAR:
            failures.append(f"{M.case_id(case)}: randn error {err:.2e} {plan}")
        if lds_off and plan["form"] == LDS:
            failures.append(f"{M.case_id(case)}: took the LDS form with MDF_WGRAD_LDS=0 {plan}")
        if pack_off and plan["form"] == LDS and plan["R"] != 0:
            failures.append(f"{M.case_id(case)}: packed taps with MDF_WGRAD_PACK=0 {plan}")
    want = {DIRECT3D, A1_MFMA, A1_VALU, DIRECT2D} if lds_off else {LDS, A1_MFMA, A1_VALU, DIRECT2D}
    if forms != want:
        failures.append(f"kernel forms reached: {sorted(forms)}, expected {sorted(want)}")
    worst = max(v[2] for v in _RESULTS.values()) if _RESULTS else NAN
    print(f"child: {len(_RESULTS)} cases, forms {sorted(forms)}, worst randn error {worst:.2e}, {len(failures)} failures")
    for f in failures:
        print("FAIL", f)
    return 1 if failures else 0


@pytest.mark.parametrize("setting", ["MDF_WGRAD_LDS", "MDF_WGRAD_PACK"])
def test_direct_forms_in_a_fresh_process(setting):
    """wgrad_kernel / wgrad2d_kernel for every kind (MDF_WGRAD_LDS=0) and the unpacked LDS form for the few-channel kinds
    (MDF_WGRAD_PACK=0): every kind at the single-voxel shape and at (2,3,5,17) / (2,5,17), integer pass exact, randn pass at the bar."""
    env = dict(os.environ)
    env.pop("MDF_WGRAD_LDS", None)
    env.pop("MDF_WGRAD_PACK", None)
    env[setting] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, timeout=120, capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
    assert "child: %d cases" % len(M.reduced_cases()) in r.stdout


if __name__ == "__main__":
    sys.exit(child_main() if "--child" in sys.argv else 2)
