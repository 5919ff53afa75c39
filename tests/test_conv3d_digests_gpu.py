"""The 3-D conv family against the commit before its kernels were split into csrc/conv3d.hip, convtr3d.hip and conv_pack.hip and moved
onto the shared voxel walk, epilogue and launcher of conv3d_common.h: every output `y` must have the bits that commit gave.
tests/golden/conv3d_digests.json holds SHA-256 digests; scripts/gen_conv3d_digests.py wrote it with a library built from that commit
(MDF_HIP_LIB) and this module's own functions, so the test needs the JSON and the library only.

Only `y` is digested: the fp64 epilogue sums of the training entries go through unordered atomics and are not bit-reproducible
(tests/test_train_gpu.py holds them to their float64 bounds).  Every launch is pinned to its route with the MDF_* switches and
mdf_last_launch must name the kernel that was meant, so a changed route rule cannot turn a case into a copy of another.
What that does NOT verify: mdf_last_launch gives the kernel's name, not its template arguments, so conv3d_kernel's tile form (MTMAX,
two tiles, one tile, split-K with one or two) is pinned through MDF_CONV3D_MT_MIN_TILES / MT2_MIN_TILES / SK_MT (FORMS, forms_of: the
rules of launch_conv_mt restated) but not confirmed.  Split-K re-associates the sums, so its digests differ from the others'; the MTMAX,
two-tile and one-tile forms of a layer accumulate in one order and give ONE digest, and a changed MDF_CONV3D_MT* rule would turn those
cases into copies of each other unnoticed.

Shapes are INPUT shapes (B, D, H, W).  conv3d_kernel: (1,1,5,7) one plane, 35 voxels, waves without a live lane; (2,3,7,9) batch 2, a
ragged last tile, Di <= 3 with MDF_CONV3D_KDSKIP 1 and 0; (1,5,6,19) Di > 3; (1,5,58,57) -- stride 2: (1,9,115,113) -- the smallest
volume with the 1024 m-tiles the two-tile split-K form asks for.  conv3d_wlds_kernel: (1,2,3,5) has fewer m-tiles than XCDs (empty
chunks), (1,7,67,151) -- stride 2: (1,13,133,301), the same output volume -- more m-tiles than the 4096 waves of the grid.  Transposed
kernels: (1,1,9,17), (2,3,20,70) and (1,6,101,119), more m-tiles than the persistent waves."""
import contextlib
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
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3d_digests.json")

# MDF_CONV_CASE of conv3d_entry
PAIRS = [(32, 16, "s1"), (16, 16, "s1"), (32, 32, "s1"), (64, 64, "s1"), (16, 8, "s1"), (8, 8, "s1"), (8, 16, "s1"), (16, 32, "s1"),
         (64, 16, "s1"), (32, 8, "s1"), (16, 64, "s1"), (8, 32, "s1"), (16, 32, "s2"), (32, 64, "s2"), (8, 16, "s2"),
         (64, 32, "tr"), (32, 16, "tr"), (16, 8, "tr")]
SHAPES = [(1, 1, 5, 7), (2, 3, 7, 9), (1, 5, 6, 19)]
SK2_SHAPE = {"s1": (1, 5, 58, 57), "s2": (1, 9, 115, 113)}
BIG = "1000000000"
# every route switch conv3d_entry and launch_conv_mt read, cleared before a case sets its own
SWITCHES = ("MDF_CONV3D_WLDS", "MDF_CONV3D_WLDS8", "MDF_CONV3D_WLDS_TRAIN", "MDF_CONVTR_ALL_MIN_VOXELS", "MDF_CONVTR_NS", "MDF_CONVTR_CLS",
            "MDF_CONVTR_WLDS", "MDF_CONV_LDS_MIN_VOXELS", "MDF_CONV3D_MT_MIN_TILES", "MDF_CONV3D_MT2_MIN_TILES", "MDF_CONV3D_SK_MT",
            "MDF_CONV3D_KDSKIP")
# conv3d_kernel alone: no weights-in-LDS form, no all-classes transposed form, no LDS-staged planes
PIN_V1 = {"MDF_CONV3D_WLDS": "0", "MDF_CONV3D_WLDS8": "0", "MDF_CONV3D_WLDS_TRAIN": "0", "MDF_CONVTR_ALL_MIN_VOXELS": "-1",
          "MDF_CONV_LDS_MIN_VOXELS": BIG}
# launch_conv_mt's tile forms: <MTMAX, 1>, <2, 1>, <1, 1> or -- 32 and 64 input channels below 4096 tiles -- <1, 4>, and <2, 4>
FORMS = {"mtmax": {"MDF_CONV3D_MT_MIN_TILES": "0", "MDF_CONV3D_MT2_MIN_TILES": "-1"},
         "mt2": {"MDF_CONV3D_MT_MIN_TILES": BIG, "MDF_CONV3D_MT2_MIN_TILES": "0"},
         "mt1": {"MDF_CONV3D_MT_MIN_TILES": BIG, "MDF_CONV3D_MT2_MIN_TILES": "-1", "MDF_CONV3D_SK_MT": "1"},
         "sk2": {"MDF_CONV3D_MT_MIN_TILES": BIG, "MDF_CONV3D_MT2_MIN_TILES": "-1", "MDF_CONV3D_SK_MT": "2"}}


@contextlib.contextmanager
def switches(**env):
    """The route switches are read per call: set for the launches inside, put back after."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def sha(t):
    a = t.detach().cpu().contiguous().numpy()
    return f"{a.dtype}{list(a.shape)}:" + hashlib.sha256(a.tobytes()).hexdigest()


def ran(kernel):
    got = mdfnet_hip.lib().mdf_last_launch().decode()
    assert got == kernel, f"{got} ran where {kernel} was pinned"


def out_shape(shape, mode):
    b, d, h, w = shape
    if mode == "tr":
        return b, 2 * d, 2 * h, 2 * w
    if mode == "s2":
        return b, (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return shape


@functools.lru_cache(maxsize=None)
def layer(cin, cout, mode, shape):
    """Host-seeded operands of one layer at one shape, on the device: x, packed weights, alpha, beta, res, stat_y, stat_aux."""
    rs = np.random.RandomState((cin * 131 + cout) * 7 + sum(shape) + len(mode) * 1000 + ord(mode[1]))
    b, d, h, w = shape
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(DEV)
    x = f(b, d, h, w, cin)
    wt = f(*((cin, cout) if mode == "tr" else (cout, cin)), 3, 3, 3) / float(np.sqrt(27 * cin))
    wp = ops.pack_conv3d_weight(wt, mode == "tr")
    alpha = torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32)).to(DEV)
    beta = torch.from_numpy(rs.uniform(-0.2, 0.2, cout).astype(np.float32)).to(DEV)
    res = f(*out_shape(shape, mode), cout)
    stat_y = f(*out_shape(shape, mode), cout) * 2 + 0.3
    aux = torch.from_numpy(np.concatenate([rs.uniform(0.5, 1.5, cout), rs.standard_normal(cout) * 0.3, rs.standard_normal(cout) * 0.2,
                                           rs.uniform(0.5, 1.5, cout)]).astype(np.float32)).to(DEV)
    return x, wp, alpha, beta, res, stat_y, aux


def fwd(cin, cout, mode, shape, epi, skip):
    x, wp, alpha, beta, res, _, _ = layer(cin, cout, mode, shape)
    return ops.conv3d_ndhwc(x, wp, cin, cout, 1 if mode == "s1" else 2, mode == "tr", alpha if epi else None, beta if epi else None, bool(epi),
                            res if skip else None)


def train(cin, cout, mode, shape, stat_mode, skip):
    x, wp, _, _, res, stat_y, aux = layer(cin, cout, mode, shape)
    sums = torch.zeros(ops.STAT_SLICES, 2 * cout, device=DEV, dtype=torch.float64)
    return ops.conv3d_train(x, wp, cin, cout, 1 if mode == "s1" else 2, mode == "tr", res if skip else None, stat_mode, sums,
                            stat_y if stat_mode == 2 else None, aux if stat_mode == 2 else None)


def forms_of(cin, mode, shape):
    """The tile forms launch_conv_mt can give this layer at this shape (eval)."""
    b, d, h, w = out_shape(shape, mode) if mode != "tr" else shape
    tiles_1 = b * d * h * w // 16
    if mode == "tr":
        return ["mtmax", "mt1"]
    if cin >= 32 and tiles_1 < 4096:               # (two tiles per wave need 16 input channels or fewer at these sizes; one tile is split-K)
        return ["mtmax", "mt1"] + (["sk2"] if tiles_1 >= 1024 else [])
    return ["mtmax", "mt2", "mt1"]


# --------------------------------------------------------------------------- conv3d_kernel
@functools.lru_cache(maxsize=None)
def v1_digests(cin, cout, mode):
    out = {}
    shapes = [(s, k) for s in SHAPES for k in (("1", "0") if s[1] <= 3 and s[0] == 2 else ("1",))]
    if mode != "tr" and cin >= 32:
        shapes.append((SK2_SHAPE[mode], "1"))
    for shape, kdskip in shapes:
        for form in forms_of(cin, mode, shape):
            if shape in SK2_SHAPE.values() and form != "sk2":
                continue
            with switches(MDF_CONV3D_KDSKIP=kdskip, **PIN_V1, **FORMS[form]):
                for epi in (0, 1):
                    for skip in ((0, 1) if mode == "tr" else (epi,)):
                        out[f"fwd {shape} kdskip{kdskip} {form} epi{epi} res{skip}"] = sha(fwd(cin, cout, mode, shape, epi, skip))
                        ran("conv3d_kernel")
                if cout >= 8 and form in ("mtmax", "mt1"):        # the persistent ST form (training entry)
                    for stat_mode in (1, 2):
                        out[f"train {shape} kdskip{kdskip} {form} stat{stat_mode}"] = sha(train(cin, cout, mode, shape, stat_mode, stat_mode == 2))
                        ran("conv3d_kernel")
    return out


# --------------------------------------------------------------------------- conv3d_wlds_kernel
WLDS = [(32, 32, "s1", 0), (16, 32, "s2", 0), (8, 16, "s2", 0), (32, 32, "s1", 1), (16, 16, "s1", 1), (16, 32, "s2", 1), (8, 16, "s2", 1)]
WLDS_SHAPES = {"s1": [(1, 2, 3, 5), (1, 7, 67, 151)], "s2": [(1, 2, 3, 5), (1, 13, 133, 301)]}


@functools.lru_cache(maxsize=None)
def wlds_digests(cin, cout, mode, st, big):
    shape = WLDS_SHAPES[mode][big]
    out = {}
    with switches(MDF_CONV_LDS_MIN_VOXELS=BIG, MDF_CONV3D_KDSKIP="1"):
        if st:
            for stat_mode in (1, 2):
                out[f"train stat{stat_mode}"] = sha(train(cin, cout, mode, shape, stat_mode, stat_mode == 2))
                ran("conv3d_wlds_kernel")
        else:
            for epi in (0, 1):
                out[f"fwd epi{epi} res{epi}"] = sha(fwd(cin, cout, mode, shape, epi, epi))
                ran("conv3d_wlds_kernel")
    return out


# --------------------------------------------------------------------------- convtr_all_kernel / convtr_cls_kernel
TR_ROUTES = [(64, 32, "convtr_all_kernel", {"MDF_CONVTR_NS": ns}) for ns in ("1", "2", "4")] + \
            [(ci, co, "convtr_all_kernel", {"MDF_CONVTR_WLDS": wl}) for ci, co in ((16, 8), (32, 16)) for wl in ("0", "1", "2")] + \
            [(64, 32, "convtr_cls_kernel", {"MDF_CONVTR_CLS": cl}) for cl in ("1", "2")]
TR_SHAPES = [(1, 1, 9, 17), (2, 3, 20, 70), (1, 6, 101, 119)]


@functools.lru_cache(maxsize=None)
def tr_digests(route, shape):
    cin, cout, kernel, env = TR_ROUTES[route]
    out = {}
    with switches(MDF_CONVTR_ALL_MIN_VOXELS="0", **env):
        for epi in (0, 1):
            for skip in (0, 1):
                out[f"fwd epi{epi} res{skip}"] = sha(fwd(cin, cout, "tr", shape, epi, skip))
                ran(kernel)
    return out


# --------------------------------------------------------------------------- the ST conv_lds_kernel, 3-D and 2-D
LDS3D = [(8, 8), (16, 8), (16, 16), (32, 16), (32, 32), (16, 32)]
LDS2D = [(3, 8, 3, 1), (8, 8, 3, 1), (16, 16, 3, 1), (32, 32, 3, 1), (64, 64, 3, 1), (16, 32, 3, 1), (32, 64, 3, 1), (8, 16, 5, 2), (16, 32, 5, 2),
         (32, 64, 5, 2)]
LDS2D_SHAPES = [(2, 19, 33), (4, 5, 70)]


@functools.lru_cache(maxsize=None)
def lds3d_digests(cin, cout):
    out = {}
    with switches(MDF_CONV_LDS_MIN_VOXELS="0"):
        for shape in SHAPES:
            for stat_mode in (1, 2):
                out[f"train {shape} stat{stat_mode}"] = sha(train(cin, cout, "s1", shape, stat_mode, stat_mode == 2))
                ran("conv_lds_kernel")
    return out


@functools.lru_cache(maxsize=None)
def lds2d_digests(cin, cout, k, stride):
    out = {}
    planar = cin < 4
    for shape in LDS2D_SHAPES:
        b, h, w = shape
        rs = np.random.RandomState(cin * 100 + cout * 3 + k + w)
        f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(DEV)
        x = f(b, cin, h, w) if planar else f(b, h, w, cin)
        wp = ops.pack_conv2d_weight(f(cout, cin, k, k) / float(np.sqrt(k * k * cin)))
        pad = (k - 1) // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        for groups in (1, 2):
            stat_y = f(b, ho, wo, cout) * 2 + 0.3
            aux = torch.from_numpy(np.concatenate([np.concatenate([rs.uniform(0.5, 1.5, cout), rs.standard_normal(cout) * 0.3,
                                                                   rs.standard_normal(cout) * 0.2, rs.uniform(0.5, 1.5, cout)])
                                                   for _ in range(groups)]).astype(np.float32)).to(DEV)
            for stat_mode in ((1,) if planar else (1, 2)):      # (the image layer has no layer below it to take a gradient for)
                sums = torch.zeros(ops.STAT_SLICES, groups * 2 * cout, device=DEV, dtype=torch.float64)
                y = ops.conv2d_train(x, wp, cin, cout, k, stride, planar, stat_mode, sums, groups, stat_y if stat_mode == 2 else None,
                                     aux if stat_mode == 2 else None)
                out[f"train {shape} groups{groups} stat{stat_mode}"] = sha(y)
                ran("conv_lds_kernel")
    return out


# --------------------------------------------------------------------------- packed weight sets
def pack_digests():
    """Every (is3d, transposed, source mode, Cin, Cout, taps) job of train_ops.py and ops.py, through the single packers and through
    mdf_pack_batch: tests/test_conv_pack_gpu.py enumerates and packs them."""
    import test_conv_pack_gpu
    return test_conv_pack_gpu.pack_digests()


def case_ids():
    ids = {f"v1 {ci}->{co} {m}": (v1_digests, (ci, co, m)) for ci, co, m in PAIRS}
    ids.update({f"wlds {ci}->{co} {m} st{st} {'big' if big else 'small'}": (wlds_digests, (ci, co, m, st, big))
                for ci, co, m, st in WLDS for big in (0, 1)})
    ids.update({f"tr {r[0]}->{r[1]} {r[3]} {s}": (tr_digests, (i, s)) for i, r in enumerate(TR_ROUTES) for s in TR_SHAPES})
    ids.update({f"lds3d {ci}->{co}": (lds3d_digests, (ci, co)) for ci, co in LDS3D})
    ids.update({f"lds2d {ci}->{co} k{k}s{s}": (lds2d_digests, (ci, co, k, s)) for ci, co, k, s in LDS2D})
    return ids


CASES = case_ids()


def all_digests():
    return {"outputs": {name: fn(*args) for name, (fn, args) in CASES.items()}, "packs": pack_digests()}


@functools.lru_cache(maxsize=None)
def recorded():
    with open(DIGESTS) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_are_bit_identical_to_the_parents(name):
    fn, args = CASES[name]
    want, got = recorded()["outputs"][name], fn(*args)
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, bad


def test_packed_sets_are_byte_identical_to_the_parents():
    want, got = recorded()["packs"], pack_digests()
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, bad
