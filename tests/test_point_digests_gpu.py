"""The point-cloud ops against the commit before their kernels were split into csrc/point_*.hip and moved onto shared walk, sort
and scan bodies: every output tensor (leaves-visited counts included), every workspace size and the text of the shared argument
refusals must be the ones that commit gave.  tests/golden/point_digests.json holds them; scripts/gen_point_digests.py wrote it with a
library built from that commit (MDF_HIP_LIB) and this module's own functions, so the test needs the JSON and the library only.

Inputs are seeded numpy clouds.  Index sizes sit around the leaf size (31 / 32 / 33), at the first size with two sort tiles (4097)
and at a non-power-of-two leaf count with empty tree nodes (9000); `dup` draws 1000 points from 250 distinct ones, so equal
distances meet the lowest-input-index tie-break; the fine voxel grid has more than 1024 occupied cells from n = 4097 on (two scan
chunks).  Queries go in both as an array and as a PointIndex."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import mdfnet_hip
from mdfnet_hip import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_digests.json")
SIZES = (0, 1, 31, 32, 33, 1000, 4097, 9000)
CLOUDS = tuple(f"n{n}" for n in SIZES) + ("dup",)
EXTENT = np.array([10.0, 8.0, 6.0])
M = 777                     # queries
CAP = 1.5                   # some queries find nothing within it
BB = [[1.0, 1.0, 0.5], [9.0, 7.5, 5.0]]
KS = (1, 8, 32)
EARG = -1


def cloud(name):
    if name == "dup":
        rs = np.random.RandomState(77)
        return (rs.random_sample((250, 3)) * EXTENT)[rs.randint(0, 250, 1000)].copy()
    n = int(name[1:])
    return np.random.RandomState(1000 + n).random_sample((n, 3)) * EXTENT


def queries(pts):
    """M points of a box a little larger than the cloud's, the first 100 of them copies of cloud points (distance 0, ties)."""
    rs = np.random.RandomState(5)
    q = rs.random_sample((M, 3)) * (EXTENT + 2.0) - 1.0
    if len(pts):
        q[:100] = pts[rs.randint(0, len(pts), 100)]
    return q


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return f"{a.dtype}{list(a.shape)}:" + hashlib.sha256(a.tobytes()).hexdigest()


def _named(prefix, names, tensors):
    return {f"{prefix}.{k}": sha(t) for k, t in zip(names, tensors)}


@functools.lru_cache(maxsize=None)
def output_digests(name):
    """op.output -> digest for one cloud."""
    pts = cloud(name)
    n = len(pts)
    tp = torch.from_numpy(pts).to(DEV)
    index = ops.point_index(tp)
    tq = torch.from_numpy(queries(pts)).to(DEV)
    out = {}
    for qname, q in (("array", tq), ("index", ops.point_index(tq))):
        out.update(_named(f"nn_distance.{qname}", ("dist", "visits"), ops.nn_distance(index, q, cap=CAP, return_visits=True)))
        out.update(_named(f"nn_distance_bb.{qname}", ("dist", "visits"), ops.nn_distance(index, q, bb=BB, cap=CAP, return_visits=True)))
        nn = ops.nn_search(index, q, CAP, return_d2=True, return_visits=True)
        out.update(_named(f"nn_search.{qname}", ("dist", "nearest", "d2", "visits"), nn))
        for k in KS:
            out.update(_named(f"knn_search.k{k}.{qname}", ("nbr", "d2", "visits"), ops.knn_search(index, q, k, return_d2=True, return_visits=True)))
        if qname == "array":
            out["icp_sums"] = sha(ops.icp_sums(tq, tp, nn[1], nn[2], 1.0))
    dirs = torch.from_numpy(np.random.RandomState(9).standard_normal((n, 3)).astype(np.float32)).to(DEV)
    out.update(_named("estimate_normals", ("normals", "cov"), ops.estimate_normals(index, dirs=dirs, k=8, return_cov=True)))
    stats = {}
    keep, rounds = ops.reduce_points(tp, 0.3, np.random.RandomState(3).permutation(n), index=index, stats=stats)
    out["reduce_points.keep"] = sha(keep)
    out["reduce_points.rounds"] = int(rounds)
    out["reduce_points.edges"] = int(stats["edges"])
    attrs = torch.from_numpy(np.random.RandomState(11).random_sample((n, 3))).to(DEV)
    for vname, voxel in (("fine", 0.25), ("coarse", 2.0)):
        vp, va, vc = ops.voxel_downsample(tp, voxel, attrs=attrs, return_counts=True)
        out.update(_named(f"voxel_downsample.{vname}", ("points", "attrs", "counts"), (vp, va, vc)))
        out[f"voxel_downsample.{vname}.m"] = int(vp.shape[0])
    return out


def workspace_sizes():
    lib = mdfnet_hip.lib()
    out = {"mdf_pts_icp_workspace": int(lib.mdf_pts_icp_workspace())}
    for n in SIZES:
        for fn in ("mdf_pts_index_workspace", "mdf_pts_reduce_workspace", "mdf_pts_voxel_workspace"):
            out[f"{fn}.{n}"] = int(getattr(lib, fn)(n))
    return out


SEARCHES = ("mdf_pts_nn_dist", "mdf_pts_nn", "mdf_pts_knn")
REFUSALS = ("both", "neither", "m_negative", "m_too_large", "index_too_small", "index_misaligned", "qindex_too_small", "qindex_misaligned")


def refusals():
    """refusal -> {entry: message}: one bad argument at a time, every other one valid."""
    lib = mdfnet_hip.lib()
    n, m = 100, 40
    index = ops.point_index(torch.from_numpy(cloud("n1000")[:n]).to(DEV))
    q = torch.from_numpy(queries(cloud("n1000"))[:m]).to(DEV)
    qindex = ops.point_index(q)
    outs = [torch.empty(m * 32, device=DEV, dtype=torch.float64) for _ in range(4)]
    o = [x.data_ptr() for x in outs]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ib, qb = index.buf.data_ptr(), qindex.buf.data_ptr()
    cases = {                       # (index, index_bytes, qindex, queries, m, qindex_bytes)
        "both": (ib, index.nbytes, qb, q.data_ptr(), m, qindex.nbytes),
        "neither": (ib, index.nbytes, None, None, m, 0),
        "m_negative": (ib, index.nbytes, None, q.data_ptr(), -1, 0),
        "m_too_large": (ib, index.nbytes, None, q.data_ptr(), 1 << 31, 0),
        "index_too_small": (ib, index.nbytes - 1, None, q.data_ptr(), m, 0),
        "index_misaligned": (ib + 8, index.nbytes, None, q.data_ptr(), m, 0),
        "qindex_too_small": (ib, index.nbytes, qb, None, m, qindex.nbytes - 1),
        "qindex_misaligned": (ib, index.nbytes, qb + 8, None, m, qindex.nbytes),
    }
    assert tuple(cases) == REFUSALS
    tails = {"mdf_pts_nn_dist": (None, ctypes.c_double(CAP), o[0], o[1], st),
             "mdf_pts_nn": (ctypes.c_double(CAP), o[0], o[1], o[2], o[3], st),
             "mdf_pts_knn": (8, o[0], o[1], o[2], st)}
    out = {}
    for what, (i, ibytes, qi, qa, mm, qbytes) in cases.items():
        out[what] = {}
        for fn in SEARCHES:
            rc = getattr(lib, fn)(i, n, ibytes, qi, qa, mm, qbytes, *tails[fn])
            assert rc == EARG, (what, fn, rc)
            out[what][fn] = lib.mdf_last_error().decode()
    torch.cuda.synchronize()
    return out


def all_digests():
    return {"outputs": {name: output_digests(name) for name in CLOUDS}, "workspace": workspace_sizes(), "refusals": refusals()}


@functools.lru_cache(maxsize=None)
def recorded():
    with open(DIGESTS) as f:
        return json.load(f)


@pytest.mark.parametrize("name", CLOUDS)
def test_outputs_are_bit_identical_to_the_parents(name):
    want, got = recorded()["outputs"][name], output_digests(name)
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, bad


def test_workspace_sizes_are_the_parents():
    assert workspace_sizes() == recorded()["workspace"]


def test_shared_refusals_keep_their_text_in_every_search():
    want, got = recorded()["refusals"], refusals()
    assert got == want
    for what in REFUSALS:
        assert len(set(got[what].values())) == 1, (what, got[what])
