"""The weight-gradient family against the commit before its direct kernels were merged into wgrad_direct_body and its host code moved
onto one plan and one instantiation list (csrc/wgrad.hip, wgrad_lds.hip, wgrad_common.h): every partial tile must have the bits that
commit gave, and every dispatch must decide what it decided.  tests/golden/wgrad_digests.json holds, per case, the nine fields of
mdf_wgrad_last_plan and the SHA-256 of the first nslab * n floats of the workspace after mdf_conv*_wgrad_partial, once for
wgrad_mirror.int_inputs and once for randn_inputs; scripts/gen_wgrad_digests.py wrote it with a library built from that commit
(MDF_HIP_LIB) and this module's own functions, so the test needs the JSON and the library only.

The SLABS are digested, not dw: a block writes its slab alone and in a fixed order, while the slab sums meet in dw through unordered
fp32 atomics and are reproducible only for the integer inputs (tests/test_wgrad_gpu.py holds those exactly).

Cases.  In this process: wgrad_mirror.all_cases() (245 small shapes; every LDS instantiation the default switches reach and the two
A = 1 forms).  In fresh child processes: reduced_cases() under MDF_WGRAD_LDS=0 (wgrad_kernel and wgrad2d_kernel<1|3|5>, the direct
body) and under MDF_WGRAD_PACK=0 (the unpacked LDS form for the few-channel kinds) -- the library reads both once per process.
One more test records four LDS-form layers of different instantiations between mdf_wgrad_batch_begin and mdf_wgrad_batch_flush:
the batch kernels must write the slabs of the single launches.

Every call fills workspace and dw with NaN first (test_wgrad_gpu.call_partial)."""
import functools
import hashlib
import json
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
import test_wgrad_gpu as W  # noqa: E402
from mdfnet_hip import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DIGESTS = os.path.join(HERE, "golden", "wgrad_digests.json")
CHILD_SETTINGS = ("MDF_WGRAD_LDS", "MDF_WGRAD_PACK")
INPUTS = {"int": M.int_inputs, "randn": M.randn_inputs}
BATCH_CASES = [(True, "conv_s1", 16, 16, (2, 3, 5, 17)), (True, "conv_s1", 8, 8, (2, 3, 5, 17)), (True, "conv_s2", 32, 16, (1, 2, 7, 33)),
               (False, "k5_s2", 32, 16, (2, 5, 17))]


def slab_sha(work, nslab, n):
    a = work[:nslab * n].cpu().numpy()
    return hashlib.sha256(a.tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def digest(case):
    """{"plan": the nine fields, "int": sha, "randn": sha} of one case under this process's switches."""
    out = {}
    for kind, inputs in INPUTS.items():
        small, big = (t.to(W.DEV) for t in inputs(case))
        work, _, nslab, n = W.call_partial(case, small, big)
        plan = W.last_plan()
        torch.cuda.synchronize()
        assert plan["gx"] == nslab, (plan, nslab)
        plan = [plan[f] for f in W.FIELDS]
        assert out.setdefault("plan", plan) == plan, (M.case_id(case), out["plan"], plan)
        out[kind] = slab_sha(work, nslab, n)
    return out


def table_digests(cases):
    return {M.case_id(c): digest(c) for c in cases}


def child_digests(setting):
    """reduced_cases() in a fresh process with `setting`=0."""
    env = dict(os.environ)
    for k in CHILD_SETTINGS:
        env.pop(k, None)
    env[setting] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.splitlines()[-1])


def all_digests():
    doc = {"default": table_digests(M.all_cases())}
    for setting in CHILD_SETTINGS:
        doc[setting + "=0"] = child_digests(setting)
    return doc


@functools.lru_cache(maxsize=None)
def recorded():
    with open(DIGESTS) as f:
        return json.load(f)


def differences(got, want):
    assert sorted(got) == sorted(want)
    return {k: (got[k], want[k]) for k in got if got[k] != want[k]}


@pytest.mark.parametrize("case", M.all_cases(), ids=M.case_id)
def test_plan_and_partial_tiles_are_the_parents(case):
    want, got = recorded()["default"][M.case_id(case)], digest(case)
    assert got == want, (got, want)


@pytest.mark.parametrize("setting", CHILD_SETTINGS)
def test_direct_and_unpacked_forms_are_the_parents(setting):
    want = recorded()[setting + "=0"]
    assert len(want) == len(M.reduced_cases())
    bad = differences(child_digests(setting), want)
    assert not bad, bad


def test_batch_launch_writes_the_slabs_of_the_single_launches():
    L = lib()
    jobs = []
    check(L.mdf_wgrad_batch_begin(), "mdf_wgrad_batch_begin")
    try:
        for case in BATCH_CASES:
            small, big = (t.to(W.DEV) for t in M.randn_inputs(case))
            jobs.append((small, big) + W.call_partial(case, small, big) + (W.last_plan(),))
    finally:
        rc = L.mdf_wgrad_batch_flush(W._stream())
    check(rc, "mdf_wgrad_batch_flush")
    torch.cuda.synchronize()
    keys = {(c[0], M.stride_ksize(c[0], c[1])[1], j[-1]["R"], j[-1]["TH"]) for c, j in zip(BATCH_CASES, jobs)}
    assert len(keys) == len(BATCH_CASES), keys                       # four kernel instantiations
    for case, (_, _, work, dw, nslab, n, plan) in zip(BATCH_CASES, jobs):
        want = recorded()["default"][M.case_id(case)]
        assert plan["form"] == W.LDS and [plan[f] for f in W.FIELDS] == want["plan"], (M.case_id(case), plan, want)
        assert not bool(dw.any()) and not bool(dw.isnan().any()), f"{M.case_id(case)}: dw is not cleared"
        assert slab_sha(work, nslab, n) == want["randn"], (M.case_id(case), plan)


if __name__ == "__main__":
    if "--child" not in sys.argv:
        sys.exit(2)
    print(json.dumps(table_digests(M.reduced_cases()), sort_keys=True))
