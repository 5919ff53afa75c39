"""GPU: the forward convolution family against the float64 references of tests/conv_mirror.py, on every route the two digest suites
reach (their tables are imported, not copied) and on the (1,2,2) layers, the wino3d strip shapes and the fused 2-D kernels.

  1. Exact generator, every case and variant: y equals the float64 reference BIT FOR BIT (outputs are NaN before the call; the kernel
     that ran is the one the digest suites pin; the ST variants' fp64 sums meet tests/test_train_gpu.py's reference at its bar).
  2. The exact generator scaled by 2^100 and by 2^-130 (denormal operands, intermediates and results), one ragged batch-2 case per
     kernel form: bit for bit again.
  3. Random operands of three classes (N(0,1); post-ReLU; N(100,1)), one case per kernel form, raw and with the epilogue:
     e_hip <= 1.5 e_32 + 0 against float64 in max, l2 and perA, e_32 the mirror's serial fp32 fma chain.  The ratio is printed.
  4. The epilogue bit for bit: where the raw and the epi / resup variant of a case ran the same kernel, the epi output equals the
     mirror's fp32 epilogue applied on the host to the kernel's own raw output.  The pairs that ran different kernels are LEFT_OUT.
  5. Non-finite locality, one case per kernel form, raw and with the epilogue's ReLU: one NaN, then one +Inf, planted at the volume's
     corner, in the last live column of the ragged last tile, in the first column of the next tile and in the last channel.  Every
     output outside the mask conv_mirror.receptive_mask gives the form is bit-identical to the clean run; without the ReLU the output
     is NaN wherever float64 is.  The direct 3-D kernels that leak nothing give float64's NaN set exactly for a planted NaN.
  6. train_ops.conv3d_dgrad / conv2d_dgrad on every layer kind against float64 autograd, exact operands, bit for bit.

MDF_CONV_WD, MDF_CONV_WINOGRAD and MDF_CONV_RW are read once per process, so the conv_lds cases run as one fresh child process per
setting, as tests/test_conv_lds_routes_gpu.py runs them: one after the other, each under its own time limit, and the first that does not
exit 0 ends the module (no further child starts).  A child ends at the first exception that is not an MDF_EUNSUPPORTED refusal.  It only
launches and saves every output to a directory of the parent's; the float64 references, the fp32 yardstick and every comparison are the
parent's (`judge`), which draws the same operands from the same seeds on the host, so a child takes about the time of its twin in
tests/test_conv_lds_routes_gpu.py per launch, and one run names every wrong case.  `python tests/test_conv_parity_gpu.py child SETTING
DIR` is one child.  Everything else runs in the pytest process, its per-call switches set through `switches()` or monkeypatch."""
import contextlib
import functools
import json
import os
import re
import subprocess
import sys
import time

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "mdf-net_amd"), os.path.join(_root, "tests")]

import numpy as np
import pytest
import torch

import conv_mirror as M
import mdfnet_hip
import test_conv3d_digests_gpu as T
import test_conv_lds_routes_gpu as R
from mdfnet_hip import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHILD_SECONDS = 240
SUMS_BAR = 2e-6                       # tests/test_train_gpu.py: _sums_close(...) < 2e-6
SCALES = (2.0 ** 100, 2.0 ** -130)
STRIDE = {"s1": 1, "s2": 2, "tr": 2, "hw": (1, 2, 2), "hwtr": (1, 2, 2)}

# Check 4: pairs whose two variants ran different kernels (the golden routes record it; test_the_left_out_list_is_what_the_routes_show
# asserts that this is the whole list): res_up is built in the plain form alone, and at even extents the k5 s2 layers take wino2d.hip
# without an epilogue and the direct or s2d form with one.
LEFT_OUT = {
    "default": ["2d 3->8 k3s1 (2, 20, 34) resup", "2d 1->8 k3s1 (2, 20, 34) resup", "2d 8->8 k3s1 (2, 20, 34) resup",
                "2d 16->16 k3s1 (2, 20, 34) resup", "2d 32->32 k3s1 (2, 20, 34) resup", "2d 64->64 k3s1 (2, 20, 34) resup",
                "2d 16->32 k3s1 (2, 20, 34) resup", "2d 32->64 k3s1 (2, 20, 34) resup", "2d 16->4 k3s1 (2, 20, 34) resup",
                "2d 8->4 k3s1 (2, 20, 34) resup", "2d 8->16 k5s2 (2, 20, 34) epi", "2d 8->16 k5s2 (2, 20, 34) epi CONV_K5_WINOGRAD_64=0",
                "2d 16->32 k5s2 (2, 20, 34) epi", "2d 16->32 k5s2 (2, 20, 34) epi CONV_K5_WINOGRAD_64=0", "2d 32->64 k5s2 (2, 20, 34) epi"],
    "wd0": [], "wd1": [], "wd2": [],
    "wg0": ["2d 3->8 k3s1 (2, 20, 34) resup", "2d 1->8 k3s1 (2, 20, 34) resup", "2d 8->8 k3s1 (2, 20, 34) resup",
            "2d 16->4 k3s1 (2, 20, 34) resup", "2d 8->4 k3s1 (2, 20, 34) resup"],
    "wg0rw0": []}

# Checks 2 and 3: one ragged batch-2 case per form of the kernels conv_lds.hip dispatches to, by the raw case's name (its `epi` twin is
# the same name with the variant replaced), the kernel that must take it, and its kind of receptive field (conv_mirror.receptive_mask).
FORMS = {
    "default": [("wino3d_kernel", "3d 16->16 (2, 5, 17, 40) raw", "wino3d_kernel", None, "wino"),
                ("conv_lds Winograd 3-D", "3d 16->16 (2, 5, 17, 40) raw CONV_WINO3D=0", "conv_lds_kernel", "wg1", "wino"),
                ("conv_lds depth-pair", "3d 8->8 (2, 5, 17, 40) raw", "conv_lds_kernel", "wg2", "winodp"),
                ("conv_lds depth-pair streamed", "3d 16->8 (2, 5, 17, 40) raw", "conv_lds_kernel", "wg3", "winodp"),
                ("conv_lds w-phase", "2d 8->8 k3s1 (2, 19, 33) raw", "conv_lds_kernel", "rw2 wg0", "wphase"),
                ("conv_lds plain 2-D", "2d 8->32 k3s1 (2, 19, 33) raw", "conv_lds_kernel", "rw1 wg0", "direct"),
                ("conv_lds Winograd 2-D", "2d 32->32 k3s1 (2, 19, 33) raw CONV_WINO2D=0", "conv_lds_kernel", "wg1", "wino"),
                ("conv_lds s2d", "2d 16->32 k5s2 (2, 20, 34) raw CONV_WINO2D=0", "conv_lds_kernel", "64,64,32,1,3,1,1,rw2 wg1", "s2d"),
                ("conv_lds k5 s2 direct", "2d 16->32 k5s2 (2, 19, 33) raw", "conv_lds_kernel", "1,5,2,2,rw1 wg0", "direct"),
                ("wino2d_kernel s1", "2d 32->32 k3s1 (2, 19, 33) raw", "wino2d_kernel", None, "wino"),
                ("wino2d_kernel S2D", "2d 16->32 k5s2 (2, 20, 34) raw", "wino2d_kernel", None, "s2d"),
                ("conv1x1_kernel", "2d 16->32 k1s1 (2, 19, 33) raw", "conv1x1_kernel", None, "direct"),
                ("conv_lds 1x1", "2d 16->32 k1s1 (2, 19, 33) raw CONV1X1=0", "conv_lds_kernel", "1,1,1,4,rw1 wg0", "direct")],
    "wg0": [("conv_lds plain 3-D", "3d 16->16 (2, 5, 17, 40) raw", "conv_lds_kernel", "rw1 wg0", "direct")],
    "wd0": [], "wd1": [], "wd2": [], "wg0rw0": []}


# --------------------------------------------------------------------------- outputs are NaN before the call
class _NanEmpty:
    """`torch` as mdfnet_hip.ops sees it, with empty / empty_like filled with NaN: an element the kernel does not write stays NaN."""

    def __init__(self):
        self.hits = 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **kw):
        t = torch.empty(*a, **kw)
        self.hits += 1
        return t.fill_(float("nan")) if t.is_floating_point() else t

    def empty_like(self, *a, **kw):
        t = torch.empty_like(*a, **kw)
        self.hits += 1
        return t.fill_(float("nan")) if t.is_floating_point() else t


@contextlib.contextmanager
def nan_outputs():
    """Every output allocated inside is NaN before its kernel runs; a block that allocated none through this proxy is an error (the
    prefill would be a no-op for it).  A refused call allocates before it is refused."""
    proxy = _NanEmpty()
    saved, ops.torch = ops.torch, proxy
    try:
        yield
    finally:
        ops.torch = saved
    assert proxy.hits > 0, "no output of the call was allocated through mdfnet_hip.ops' torch.empty / empty_like"


@contextlib.contextmanager
def captured_sums():
    """The (kind, stat_out, stat_y, stat_aux, groups) of the training entries called inside."""
    calls, saved = [], (ops.conv3d_train, ops.conv2d_train)

    def c3(x, wpack, cin, cout, stride, transposed, res, stat_mode, stat_out, stat_y=None, stat_aux=None):
        calls.append((stat_mode, stat_out, stat_y, stat_aux, 1))
        return saved[0](x, wpack, cin, cout, stride, transposed, res, stat_mode, stat_out, stat_y, stat_aux)

    def c2(x, wpack, cin, cout, ksize, stride, planar_in, stat_mode, stat_out, ngroups, stat_y=None, stat_aux=None):
        calls.append((stat_mode, stat_out, stat_y, stat_aux, ngroups))
        return saved[1](x, wpack, cin, cout, ksize, stride, planar_in, stat_mode, stat_out, ngroups, stat_y, stat_aux)
    ops.conv3d_train, ops.conv2d_train = c3, c2
    try:
        yield calls
    finally:
        ops.conv3d_train, ops.conv2d_train = saved


def sums_error(y, call):
    """The fp64 epilogue sums against tests/test_train_gpu.py's float64 reference, in its metric."""
    from test_train_gpu import _bn_sums_reference, _sums_close
    stat_mode, stat_out, stat_y, stat_aux, groups = call
    ref = _bn_sums_reference(y, stat_y if stat_mode == 2 else None, stat_aux if stat_mode == 2 else None, groups)
    return _sums_close(stat_out.sum(0), ref, y.numel() // y.shape[-1] // groups)


# --------------------------------------------------------------------------- operands of one generator, and their references
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _HostDict(dict):
    def __init__(self, owner):
        super().__init__()
        self.owner = owner

    def __missing__(self, key):
        self[key] = self.owner.host_of(key)
        return self[key]


class Operands:
    """The digest suites' `layer` / `layer2d` with the mirror's operands: gen = ("exact", scale) or ("random", class)."""

    def __init__(self, gen, plant=None):
        """plant = ((b, d, h, w, c), value): x of every layer holds `value` there (2-D layers: d is dropped)."""
        self.gen, self.host, self.device, self.raw, self.plant = gen, _HostDict(self), {}, {}, plant

    def _make(self, key, xshape, wshape, stride, tr):
        rs = M.rng(*[ord(c) for c in repr(key)], M.CLASSES.index(self.gen[1]) if self.gen[0] == "random" else 7)
        if self.gen[0] == "exact":
            return M.exact_operands(rs, xshape, wshape, stride, tr, self.gen[1]), rs
        return M.random_operands(rs, self.gen[1], xshape, wshape, stride, tr), rs

    @staticmethod
    def _stat(rs, oshape, groups):
        """stat_y and aux as the digest suites draw them (they do not enter y)."""
        c = oshape[-1]
        stat_y = (rs.standard_normal(oshape) * 2 + 0.3).astype(np.float32)
        aux = np.concatenate([np.concatenate([rs.uniform(0.5, 1.5, c), rs.standard_normal(c) * 0.3, rs.standard_normal(c) * 0.2, rs.uniform(0.5, 1.5, c)])
                              for _ in range(groups)]).astype(np.float32)
        return {"stat_y": stat_y, "aux": aux}

    def host_of(self, key):
        """The layer's operands on the host (no GPU needed: the parent process draws the same ones as its child)."""
        if key[0] == "3d":
            _, cin, cout, mode, shape = key
            tr = mode in ("tr", "hwtr")
            o, rs = self._make(key, tuple(shape) + (cin,), ((cin, cout) if tr else (cout, cin)) + (3, 3, 3), STRIDE[mode], tr)
            if self.plant:
                o["x"][self.plant[0]] = self.plant[1]
            return dict(o, **self._stat(rs, o["res"].shape, 1))
        _, cin, cout, k, stride, (b, h, w) = key
        o, rs = self._make(key, (b, 1, h, w, cin), (cout, cin, 1, k, k), (1, stride, stride), False)
        o = dict(o, x=o["x"][:, 0], w=o["w"][:, :, 0], res=o["res"][:, 0])
        if self.plant:
            pl = self.plant[0]
            o["x"][(pl[0],) + tuple(pl[2:])] = self.plant[1]
        return dict(o, **self._stat(rs, o["res"].shape, 2))

    def layer(self, cin, cout, mode, shape):
        key = ("3d", cin, cout, mode, tuple(shape))
        if key not in self.device:
            o = self.host[key]
            self.device[key] = (dev(o["x"]), ops.pack_conv3d_weight(dev(o["w"]), mode in ("tr", "hwtr")), dev(o["alpha"]), dev(o["beta"]),
                                dev(o["res"]), dev(o["stat_y"]), dev(o["aux"]))
        return self.device[key]

    def layer2d(self, cin, cout, k, stride, shape):
        key = ("2d", cin, cout, k, stride, tuple(shape))
        if key not in self.device:
            o = self.host[key]
            self.device[key] = (dev(o["x"]), ops.pack_conv2d_weight(dev(o["w"])), dev(o["alpha"]), dev(o["beta"]), dev(o["res"]), dev(o["res_up"]),
                                dev(o["stat_y"]), dev(o["aux"]))
        return self.device[key]

    # ---- references
    def raw_of(self, key):
        """(y64, A) of the bare convolution; under the exact generator y64 is kept as the fp32 tensor it is (asserted) and A is not kept."""
        if key not in self.raw:
            o = self.host[key]
            x, w, stride, tr = (o["x"], o["w"], STRIDE[key[3]], key[3] in ("tr", "hwtr")) if key[0] == "3d" else M.as3d(o["x"], o["w"], key[4]) + (False,)
            y, a = M.conv_ref(x, w, stride, tr, want_a=self.gen[0] != "exact")
            if key[0] == "2d":
                y, a = y[:, 0], (None if a is None else a[:, 0])
            if self.gen[0] == "exact":
                assert M.is_f32(y), key
                y, a = y.astype(np.float32), None
            self.raw[key] = (y, a)
        y, a = self.raw[key]
        return y.astype(np.float64), a

    def ref3d(self, cin, cout, mode, shape, epi, skip, dtype=np.float64, acc=None):
        key = ("3d", cin, cout, mode, tuple(shape))
        o = self.host[key]
        y, a = self.raw_of(key) if acc is None else (acc, None)
        kw = dict(alpha=o["alpha"] if epi else None, beta=o["beta"] if epi else None, relu=bool(epi), res=o["res"] if skip else None)
        return M.epilogue(y, dtype=dtype, **kw), (None if a is None else M.epilogue_scale(a, kw["alpha"], kw["beta"], kw["res"]))

    def ref2d(self, cin, cout, k, stride, shape, variant, dtype=np.float64, acc=None):
        key = ("2d", cin, cout, k, stride, tuple(shape))
        o = self.host[key]
        y, a = self.raw_of(key) if acc is None else (acc, None)
        if variant == "epi":
            kw = dict(alpha=o["alpha"], beta=o["beta"], res=o["res"], res_scale=o["res_scale"])
            return M.epilogue(y, relu=True, dtype=dtype, **kw), (None if a is None else M.epilogue_scale(a, **kw))
        if variant == "resup":
            kw = dict(alpha=o["alpha"], beta=o["beta"], res_up=o["res_up"])
            return M.epilogue(y, dtype=dtype, **kw), (None if a is None else M.epilogue_scale(a, **kw))
        if variant == "shuf":
            return M.shuffle2_store(y), (None if a is None else M.shuffle2_store(a))
        return y, a                                         # raw, nhwc, st*: the bare convolution


@contextlib.contextmanager
def operands(gen):
    """The digest suites' helpers draw from the mirror's generator inside."""
    o = gen if isinstance(gen, Operands) else Operands(gen)
    saved = T.layer, R.layer2d
    T.layer, R.layer2d = o.layer, o.layer2d
    try:
        yield o
    finally:
        T.layer, R.layer2d = saved


def bits_equal(y, ref):
    got = (torch.from_numpy(y) if isinstance(y, np.ndarray) else y.detach().cpu()).double()
    want = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64))
    return got.shape == want.shape and torch.equal(got, want)


def launched():
    return mdfnet_hip.lib().mdf_last_launch().decode()


def chain_of(o, key):
    """The fp32 yardstick's accumulator of a layer."""
    if key[0] == "3d":
        return M.chain32(o["x"], o["w"], STRIDE[key[3]], key[3] in ("tr", "hwtr"))
    return M.chain32(*M.as3d(o["x"], o["w"], key[4]))[:, 0]


# --------------------------------------------------------------------------- one child process: the conv_lds cases of a setting
def _set_case_env(env):
    for k in R.PER_CALL:
        os.environ.pop(k, None)
    os.environ["MDF_CONV_LDS_MIN_VOXELS"] = "0"
    os.environ.update(env)


def _run_case(kind, args, res_scale):
    return R.run3d(*args) if kind == "3d" else R.run2d(*args, res_scale=res_scale)


def _ref_case(o, kind, args, dtype=np.float64, acc=None):
    if kind == "3d":
        cin, cout, shape, variant = args
        return o.ref3d(cin, cout, "s1", shape, variant == "epi", variant in ("epi", "st2"), dtype, acc)
    return o.ref2d(*args, dtype=dtype, acc=acc)


def _key_case(kind, args):
    return ("3d", args[0], args[1], "s1", tuple(args[2])) if kind == "3d" else ("2d",) + tuple(args[:4]) + (tuple(args[4]),)


def _twin(name, variant):
    """The name of a case's raw twin."""
    return name.replace(f" {variant}", " raw", 1)


def child(setting, outdir):
    """The GPU side of a setting: every launch, its output saved under `outdir` for the parent process to judge (the float64
    references, the fp32 yardstick and every comparison are the parent's, so the child holds the GPU no longer than the digest suite's
    child does per launch).  On stderr, around the library's own MDF_CONV_DEBUG lines: `[case PASS|NAME]` before a call and
    `[done] {json}` after it."""
    t0 = time.time()
    table = {c[0]: c for c in R.cases(setting)}
    count = [0]

    def mark(tag, name):
        sys.stderr.write(f"[case {tag}|{name}]\n")
        sys.stderr.flush()

    def done(y=None, **rec):
        if y is not None:
            rec["file"] = f"{count[0]}.npy"
            np.save(os.path.join(outdir, rec["file"]), y.detach().cpu().numpy())
            count[0] += 1
        sys.stderr.write("[done] " + json.dumps(dict(rec, launch=rec.get("launch", launched()))) + "\n")
        sys.stderr.flush()

    def run(tag, name, kind, args, res_scale, nan=True):
        mark(tag, name)
        try:
            with (nan_outputs() if nan else contextlib.nullcontext()), captured_sums() as calls:
                y = _run_case(kind, args, res_scale)
            done(y, sums=sums_error(y, calls[0]) if calls else None)
        except mdfnet_hip.MdfHipError as e:         # an entry's refusal is a route too; anything else ends the child
            if " failed with code -2: " not in str(e):
                raise
            done(launch=f"error: {e}")

    with operands(("exact", 1.0)):                                             # 1. exact operands, every case
        for name, kind, args, env in table.values():
            _set_case_env(env)
            run("exact", name, kind, args, M.RES_SCALE_EXACT)
    with operands(("random", "normal")):                                       # 4. the raw and the epi / resup launch of a pair
        for name, kind, args, env in table.values():
            if args[-1] in ("epi", "resup") and name not in LEFT_OUT[setting]:
                _set_case_env(env)
                run("epiraw", name, kind, tuple(args[:-1]) + ("raw",), M.RES_SCALE_RANDOM, nan=False)
                run("epi", name, kind, args, M.RES_SCALE_RANDOM, nan=False)
    for form, name, _, _, _ in FORMS[setting]:                                 # 2. and 3. one case per kernel form
        _, kind, args, env = table[name]
        _set_case_env(env)
        for variant in ("raw", "epi"):
            vargs = tuple(args[:-1]) + (variant,)
            for scale in SCALES:
                with operands(("exact", scale)):
                    run(f"scale {scale:g} {variant}", name, kind, vargs, M.RES_SCALE_EXACT)
            for cls in M.CLASSES:
                with operands(("random", cls)):
                    run(f"random {cls} {variant}", name, kind, vargs, M.RES_SCALE_RANDOM, nan=False)
    for form, name, _, _, _ in FORMS[setting]:                                 # 5. one NaN, one +Inf, four places
        _, kind, args, env = table[name]
        _set_case_env(env)
        for vi, value in enumerate(PLANTS):
            for pi, place in enumerate(_places(kind, args)):
                with operands(Operands(("exact", 1.0), (place, value))):
                    for variant in ("raw", "epi"):
                        run(f"plant {vi} {pi} {variant}", name, kind, tuple(args[:-1]) + (variant,), M.RES_SCALE_EXACT)
    sys.stderr.write(f"[seconds] {time.time() - t0:.1f}\n")


PLANTS = (float("nan"), float("inf"))


def _places(kind, args):
    shape = tuple(args[2]) if kind == "3d" else (args[4][0], 1) + tuple(args[4][1:])
    return M.plant_places(shape, args[0])


def locality(y, clean, ref, mask, relu, exact_nan_set=False):
    """The failures of one planted run: y and the clean run are arrays, ref the float64 reference of the planted bare convolution (its
    NaN set is the epilogue-free output's), mask conv_mirror.receptive_mask's."""
    out = []
    outside = np.broadcast_to(~mask, y.shape)
    same = (y == clean) | (np.isnan(y) & np.isnan(clean))
    if not same[outside].all():
        bad = np.argwhere(outside & ~same)
        out.append(f"{len(bad)} outputs outside the receptive field changed, first {bad[0].tolist()}, last {bad[-1].tolist()}")
    if not relu:
        if (np.isnan(ref) & ~np.isnan(y)).any():
            out.append("float64 is NaN where the kernel is not")
        if not np.isnan(y).any():
            out.append("no NaN reached the output")
        if exact_nan_set and not np.array_equal(np.isnan(y), np.isnan(ref)):
            out.append("the NaN set is not float64's")
    return out


def judge(setting, recs, outdir):
    """The parent's half: every saved output against the mirror."""
    table = {c[0]: c for c in R.cases(setting)}
    load = lambda r: np.load(os.path.join(outdir, r["file"]))
    exact, normal = Operands(("exact", 1.0)), Operands(("random", "normal"))
    for (tag, name), r in recs.items():
        if "file" not in r:
            continue
        _, kind, args, _ = table[name]
        key = _key_case(kind, args)
        if tag == "exact":
            r["equal"] = bits_equal(load(r), _ref_case(exact, kind, args)[0])
        elif tag == "epi":
            raw = recs["epiraw", name]
            r["equal"] = "file" in raw and bool(np.array_equal(load(r), _ref_case(normal, kind, args, np.float32, load(raw))[0]))
        elif tag.startswith("scale "):
            _, scale, variant = tag.split()
            o = Operands(("exact", [s for s in SCALES if f"{s:g}" == scale][0]))
            r["equal"] = bits_equal(load(r), _ref_case(o, kind, tuple(args[:-1]) + (variant,))[0])
        elif tag.startswith("random "):
            _, cls, variant = tag.split()
            o, vargs = Operands(("random", cls)), tuple(args[:-1]) + (variant,)
            ref, a = _ref_case(o, kind, vargs)
            yard, _ = _ref_case(o, kind, vargs, np.float32, chain_of(o.host[key], key))
            r["ratios"] = M.bar_ratios(M.metrics(load(r), ref, a), M.metrics(yard, ref, a))
        elif tag.startswith("plant "):
            _, vi, pi, variant = tag.split()
            place, mkind = _places(kind, args)[int(pi)], [f[4] for f in FORMS[setting] if f[1] == name][0]
            h = Operands(("exact", 1.0), (place, PLANTS[int(vi)])).host[key]
            x, w, stride = (h["x"], h["w"], 1) if kind == "3d" else M.as3d(h["x"], h["w"], args[3])
            mask = M.receptive_mask(mkind, place, x.shape, w.shape, stride)
            with np.errstate(invalid="ignore"):
                ref = M.conv_ref(x, w, stride, want_a=False)[0]
            if kind == "2d":
                mask, ref = mask[:, 0], ref[:, 0]
            clean = load(recs["exact", name if variant == "raw" else name.replace(" raw", " epi", 1)])
            r["locality"] = locality(load(r), clean, ref, mask, variant == "epi")
    return recs


_child_failed = []


@functools.lru_cache(maxsize=None)
def records(setting):
    """{(pass, case): record + "lds": the conv_lds tuples of the call} of one fresh process, judged."""
    import shutil
    import tempfile
    assert not _child_failed, f"child {_child_failed[0]} did not exit 0: no further child is started"
    env = dict(os.environ, MDF_CONV_DEBUG="1", **R.SETTINGS[setting])
    for k in R.PER_PROCESS + R.PER_CALL + T.SWITCHES:
        if k not in R.SETTINGS[setting]:
            env.pop(k, None)
    outdir = tempfile.mkdtemp(prefix="conv_parity_")
    try:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "child", setting, outdir], env=env,
                           capture_output=True, text=True)
        if r.returncode != 0:
            _child_failed.append(setting)
        assert r.returncode == 0, f"child {setting} exited {r.returncode}; no further child is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        out, case, lds = {}, None, []
        for line in r.stderr.splitlines():
            m = re.match(r"\[case (.*)\|(.*)\]$", line)
            if m:
                case, lds = (m.group(1), m.group(2)), []
                continue
            m = re.match(r"\[conv_lds<([\d,]+,rw\d+ wg\d+ st\d+)>\] .*, grid (\d+), items (\d+)$", line)
            if m and case:
                lds.append(f"{m.group(1)} grid {m.group(2)} items {m.group(3)}")
            if line.startswith("[done] ") and case:
                out[case] = dict(json.loads(line[7:]), lds=lds)
                case = None
            if line.startswith("[seconds] "):
                print(f"child {setting}: {line[10:]} s, {len(out)} records")
        t0 = time.time()
        judge(setting, out, outdir)
        print(f"judged {setting} in {time.time() - t0:.1f} s")
        return out
    finally:
        shutil.rmtree(outdir, ignore_errors=True)


@pytest.mark.parametrize("setting", list(R.SETTINGS))
def test_conv_lds_routes_exact_operands_bit_for_bit(setting):
    got, want = records(setting), R.golden()[setting]
    names = [c[0] for c in R.cases(setting)]
    assert sorted(n for p, n in got if p == "exact") == sorted(names)
    route = {n: ((got["exact", n]["launch"], got["exact", n]["lds"]), (want[n]["launch"], want[n]["lds"])) for n in names}
    bad = {n: r for n, r in route.items() if r[0] != r[1]}
    assert not bad, ("not the kernel and plan the digest suite pins", dict(list(bad.items())[:4]))
    assert all(("file" in got["exact", n]) != got["exact", n]["launch"].startswith("error: ") for n in names)
    wrong = [n for n in names if got["exact", n].get("equal") is False]
    assert not wrong, (len(wrong), wrong[:12])
    sums = {n: got["exact", n]["sums"] for n in names if got["exact", n].get("sums") is not None}
    assert all(" st" in n for n in sums) and len(sums) == sum(" st" in n and "file" in got["exact", n] for n in names)
    assert max(sums.values(), default=0.0) < SUMS_BAR, {n: v for n, v in sums.items() if v >= SUMS_BAR}


@pytest.mark.parametrize("setting", list(R.SETTINGS))
def test_conv_lds_routes_epilogue_bit_for_bit(setting):
    """Check 4.  Every pair that is not LEFT_OUT ran one kernel twice (launch and conv_lds tuple) and its epilogue is the mirror's."""
    got = records(setting)
    pairs = [n for p, n in got if p == "epi"]
    assert sorted(pairs) == sorted(c[0] for c in R.cases(setting) if c[2][-1] in ("epi", "resup") and c[0] not in LEFT_OUT[setting])
    kern = lambda r: (r["launch"], [l.split(" grid ")[0] for l in r["lds"]])
    assert all(kern(got["epiraw", n]) == kern(got["epi", n]) for n in pairs), [n for n in pairs if kern(got["epiraw", n]) != kern(got["epi", n])]
    wrong = [n for n in pairs if got["epi", n].get("equal") is False]
    assert not wrong, (len(wrong), wrong[:12])


def test_the_left_out_list_is_what_the_routes_show():
    kern = lambda r: (r["launch"], [l.split(" grid ")[0] for l in r["lds"]])
    for setting in R.SETTINGS:
        want, names = R.golden()[setting], {c[0]: c for c in R.cases(setting)}
        differ = [n for n, c in names.items() if c[2][-1] in ("epi", "resup") and kern(want[n]) != kern(want[_twin(n, c[2][-1])])]
        assert differ == LEFT_OUT[setting], setting
        assert all(n.endswith(" resup") or "k5s2 (2, 20, 34) epi" in n for n in differ)


@pytest.mark.parametrize("setting", [s for s in R.SETTINGS if FORMS[s]])
def test_conv_lds_kernel_forms_scaled_and_random(setting):
    """Checks 2 and 3 on the forms of FORMS."""
    got = records(setting)
    failures = []
    for form, name, kernel, tup, _ in FORMS[setting]:
        for variant in ("raw", "epi"):
            for p in [f"scale {s:g} {variant}" for s in SCALES] + [f"random {c} {variant}" for c in M.CLASSES]:
                r = got[p, name]
                if variant == "raw":                  # (the epi twin of a raw case may take another kernel: LEFT_OUT)
                    assert r["launch"] == kernel and (tup is None or any(tup in l for l in r["lds"])), (form, p, r)
                if "ratios" in r:
                    print(f"{form:30s} [{r['launch']}] {p:22s} e_hip / (1.5 e_32): " + " ".join(f"{k} {v:.2f}" for k, v in r["ratios"].items()))
                    if max(r["ratios"].values()) > 1.0:
                        failures.append((form, p, r["ratios"]))
                elif not r.get("equal"):
                    failures.append((form, p, "not bit-exact"))
    assert not failures, failures


@pytest.mark.parametrize("setting", [s for s in R.SETTINGS if FORMS[s]])
def test_conv_lds_kernel_forms_nonfinite_locality(setting):
    """Check 5 on the forms of FORMS."""
    got = records(setting)
    failures = []
    for form, name, kernel, tup, _ in FORMS[setting]:
        for vi in range(len(PLANTS)):
            for pi in range(4):
                r = got[f"plant {vi} {pi} raw", name]
                assert r["launch"] == kernel and (tup is None or any(tup in l for l in r["lds"])), (form, r)
                for variant in ("raw", "epi"):
                    bad = got[f"plant {vi} {pi} {variant}", name]["locality"]
                    if bad:
                        failures.append((form, PLANTS[vi], pi, variant, bad))
    assert not failures, failures


# --------------------------------------------------------------------------- the conv3d digest table, in this process
@contextlib.contextmanager
def checked_digest_helpers(o, failures):
    """T.fwd / T.train check every y they return against the float64 reference (and the ST sums against theirs); T.sha does nothing."""
    saved = T.fwd, T.train, T.sha

    def fwd(cin, cout, mode, shape, epi, skip):
        with nan_outputs():
            y = saved[0](cin, cout, mode, shape, epi, skip)
        if not bits_equal(y, o.ref3d(cin, cout, mode, shape, epi, skip)[0]):
            failures.append(f"fwd {cin}->{cout} {mode} {shape} epi{epi} res{skip} [{launched()}] {dict((k, os.environ[k]) for k in T.SWITCHES if k in os.environ)}")
        return y

    def train(cin, cout, mode, shape, stat_mode, skip):
        with nan_outputs(), captured_sums() as calls:
            y = saved[1](cin, cout, mode, shape, stat_mode, skip)
        if not bits_equal(y, o.ref3d(cin, cout, mode, shape, 0, skip)[0]):
            failures.append(f"train {cin}->{cout} {mode} {shape} stat{stat_mode} [{launched()}]")
        err = sums_error(y, calls[0])
        if not err < SUMS_BAR:
            failures.append(f"sums {cin}->{cout} {mode} {shape} stat{stat_mode}: {err:.3e}")
        return y
    T.fwd, T.train, T.sha = fwd, train, (lambda t: "")
    try:
        yield
    finally:
        T.fwd, T.train, T.sha = saved


EXACT = Operands(("exact", 1.0))


@pytest.mark.parametrize("name", sorted(n for n in T.CASES if not n.startswith("lds2d")))
def test_conv3d_digest_table_exact_operands_bit_for_bit(name):
    """Every case of tests/test_conv3d_digests_gpu.py's table, through its own route pinning (`ran` inside), on exact operands."""
    fn, args = T.CASES[name]
    failures = []
    with operands(EXACT) as o, checked_digest_helpers(o, failures):
        fn.__wrapped__(*args)
    assert not failures, failures[:8]


@pytest.mark.parametrize("cin,cout,k,stride", T.LDS2D)
def test_conv2d_training_entries_exact_operands_bit_for_bit(cin, cout, k, stride):
    """T.LDS2D x T.LDS2D_SHAPES x groups x ST mode (lds2d_digests draws its operands in line; the same calls through run2d)."""
    failures = []
    with operands(EXACT) as o:
        for shape in T.LDS2D_SHAPES:
            for groups in (1, 2):
                for mode in ((1,) if cin < 4 else (1, 2)):
                    with nan_outputs(), captured_sums() as calls:
                        y = R.run2d(cin, cout, k, stride, shape, f"st{mode}g{groups}")
                    T.ran("conv_lds_kernel")
                    if not bits_equal(y, o.ref2d(cin, cout, k, stride, shape, "raw")[0]):
                        failures.append((shape, groups, mode))
                    err = sums_error(y, calls[0])
                    if not err < SUMS_BAR:
                        failures.append((shape, groups, mode, err))
    assert not failures, failures


# --------------------------------------------------------------------------- the (1,2,2) layers and the wino3d strip shapes
def _hw(o, cin, cout, tr, shape, epi):
    x, wp, alpha, beta, res, _, _ = o.layer(cin, cout, "hwtr" if tr else "hw", shape)
    with nan_outputs():
        return ops.conv3d_ndhwc(x, wp, cin, cout, (1, 2, 2), tr, alpha if epi else None, beta if epi else None, bool(epi), res if epi else None)


def _hw_table():
    import test_regular_stride_gpu as H
    return H.PAIRS, H.SHAPES


@pytest.mark.parametrize("cin,cout,tr", _hw_table()[0])
def test_hw_layers_exact_operands_bit_for_bit(cin, cout, tr, monkeypatch):
    failures = []
    for shape in _hw_table()[1]:
        for route in (None, "1", "2", "3"):
            for kdskip in (("1", "0") if shape[1] <= 3 else ("1",)):
                monkeypatch.delenv("MDF_CONV3D_HW_ROUTE", raising=False)
                if route:
                    monkeypatch.setenv("MDF_CONV3D_HW_ROUTE", route)
                monkeypatch.setenv("MDF_CONV3D_KDSKIP", kdskip)
                for epi in (0, 1):
                    y = _hw(EXACT, cin, cout, tr, shape, epi)
                    assert launched() == "conv3d_hw_kernel"
                    if not bits_equal(y, EXACT.ref3d(cin, cout, "hwtr" if tr else "hw", shape, epi, epi)[0]):
                        failures.append((shape, route, kdskip, epi))
    assert not failures, failures


def _strip_shapes():
    import test_wino3d_strip_gpu as W
    return W.SHAPES


@pytest.mark.parametrize("cin,cout", [(32, 16), (16, 16)])
def test_wino3d_strip_shapes_exact_operands_bit_for_bit(cin, cout, monkeypatch):
    failures = []
    monkeypatch.setenv("MDF_CONV_LDS_MIN_VOXELS", "0")
    for shape in _strip_shapes():
        for strip in ("default", "0"):
            for k in ("MDF_W3_STRIP", "MDF_W3_WL"):
                monkeypatch.delenv(k, raising=False)
                if strip == "0":
                    monkeypatch.setenv(k, "0")
            for epi, skip in ((0, 0), (1, 0), (1, 1)):
                with operands(EXACT):
                    with nan_outputs():
                        y = T.fwd(cin, cout, "s1", shape, epi, skip)
                assert launched().startswith("wino3d_kernel")
                if not bits_equal(y, EXACT.ref3d(cin, cout, "s1", shape, epi, skip)[0]):
                    failures.append((shape, strip, epi, skip))
    assert not failures, failures


# --------------------------------------------------------------------------- kernel forms outside conv_lds.hip: checks 2, 3 and 4
RAGGED = (2, 3, 7, 9)                 # T.SHAPES[1]: the ragged batch-2 shape of the conv3d_kernel table; T.TR_SHAPES[1] is the transposed routes'
# (form, kernel, layer, shape, switches)
FORMS3D = [("conv3d_kernel", "conv3d_kernel", (32, 16, "s1"), RAGGED, dict(T.PIN_V1, **T.FORMS["mtmax"])),
           ("conv3d_kernel s2", "conv3d_kernel", (16, 32, "s2"), RAGGED, dict(T.PIN_V1, **T.FORMS["mt1"])),
           ("conv3d_kernel transposed", "conv3d_kernel", (32, 16, "tr"), RAGGED, dict(T.PIN_V1, **T.FORMS["mtmax"])),
           ("conv3d_wlds_kernel", "conv3d_wlds_kernel", (32, 32, "s1"), RAGGED, {"MDF_CONV_LDS_MIN_VOXELS": T.BIG}),
           ("convtr_all_kernel", "convtr_all_kernel", (16, 8, "tr"), T.TR_SHAPES[1], {"MDF_CONVTR_ALL_MIN_VOXELS": "0", "MDF_CONVTR_WLDS": "0"}),
           ("convtr_cls_kernel", "convtr_cls_kernel", (64, 32, "tr"), RAGGED, {"MDF_CONVTR_ALL_MIN_VOXELS": "0", "MDF_CONVTR_CLS": "1"}),
           ("conv3d_hw_kernel down", "conv3d_hw_kernel", (8, 16, "hw"), (2, 3, 5, 21), {}),
           ("conv3d_hw_kernel up", "conv3d_hw_kernel", (16, 8, "hwtr"), (2, 3, 5, 21), {})]


def _fwd3(o, cin, cout, mode, shape, epi, skip):
    if mode in ("hw", "hwtr"):
        x, wp, alpha, beta, res, _, _ = o.layer(cin, cout, mode, shape)
        with nan_outputs():
            return ops.conv3d_ndhwc(x, wp, cin, cout, (1, 2, 2), mode == "hwtr", alpha if epi else None, beta if epi else None, bool(epi), res if skip else None)
    with operands(o), nan_outputs():
        return T.fwd(cin, cout, mode, shape, epi, skip)


@pytest.mark.parametrize("form,kernel,layer,shape,env", FORMS3D, ids=[f[0] for f in FORMS3D])
def test_3d_kernel_forms_scaled_random_and_epilogue(form, kernel, layer, shape, env):
    cin, cout, mode = layer
    key = ("3d", cin, cout, mode, tuple(shape))
    failures = []
    with T.switches(**env):
        for scale in SCALES:                                                        # check 2
            o = Operands(("exact", scale))
            for epi in (0, 1):
                y = _fwd3(o, cin, cout, mode, shape, epi, epi)
                assert launched() == kernel, launched()
                if not bits_equal(y, o.ref3d(cin, cout, mode, shape, epi, epi)[0]):
                    failures.append((f"scale {scale:g}", epi, "not bit-exact"))
        for cls in M.CLASSES:                                                       # checks 3 and 4
            o = Operands(("random", cls))
            raw = _fwd3(o, cin, cout, mode, shape, 0, 0)
            epi = _fwd3(o, cin, cout, mode, shape, 1, 1)
            assert launched() == kernel
            if not np.array_equal(epi.cpu().numpy(), o.ref3d(cin, cout, mode, shape, 1, 1, np.float32, raw.cpu().numpy())[0]):
                failures.append((cls, "the epilogue is not the mirror's on the kernel's own raw output"))
            chain = chain_of(o.host[key], key)
            for what, y, e in (("raw", raw, 0), ("epi", epi, 1)):
                ref, a = o.ref3d(cin, cout, mode, shape, e, e)
                ratios = M.bar_ratios(M.metrics(y.cpu().numpy(), ref, a), M.metrics(o.ref3d(cin, cout, mode, shape, e, e, np.float32, chain)[0], ref, a))
                print(f"{form:30s} random {cls:7s} {what} e_hip / (1.5 e_32): " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
                if max(ratios.values()) > 1.0:
                    failures.append((cls, what, ratios))
    assert not failures, failures


@pytest.mark.parametrize("form,kernel,layer,shape,env", FORMS3D, ids=[f[0] for f in FORMS3D])
def test_3d_kernel_forms_nonfinite_locality(form, kernel, layer, shape, env):
    """Check 5 on the direct 3-D kernels.  The transposed layers with 8 output channels take the `tr8` mask (conv_mirror.receptive_mask:
    the zero rows of the offset +1 tap slot); every other form the tap loop's field, and float64's NaN set exactly for a planted NaN
    (for a planted Inf the masked taps' multiply by zero adds NaNs inside the field)."""
    cin, cout, mode = layer
    key = ("3d", cin, cout, mode, tuple(shape))
    tr = mode in ("tr", "hwtr")
    mkind = "tr8" if tr and cout == 8 else "direct"
    failures = []
    with T.switches(**env):
        clean = Operands(("exact", 1.0))
        y_clean = {epi: _fwd3(clean, cin, cout, mode, shape, epi, epi).cpu().numpy() for epi in (0, 1)}
        for value in PLANTS:
            for pi, place in enumerate(M.plant_places(shape, cin)):
                o = Operands(("exact", 1.0), (place, value))
                h = o.host[key]
                mask = M.receptive_mask(mkind, place, h["x"].shape, h["w"].shape, STRIDE[mode], tr)
                with np.errstate(invalid="ignore"):
                    ref = M.conv_ref(h["x"], h["w"], STRIDE[mode], tr, want_a=False)[0]
                for epi in (0, 1):
                    y = _fwd3(o, cin, cout, mode, shape, epi, epi).cpu().numpy()
                    assert launched() == kernel
                    bad = locality(y, y_clean[epi], ref, mask, bool(epi), exact_nan_set=(mkind == "direct" and value != value))
                    if bad:
                        failures.append((value, pi, place, "epi" if epi else "raw", bad))
    assert not failures, failures


# --------------------------------------------------------------------------- the fused 2-D kernels
def _fused_operands(gen, shape):
    """Host operands of the five fused kernels at one (B,H,W): two 3x3 layers 3 -> 8 -> 8 and 8 -> 8 -> 8, the 8 -> 32 -> 1 tail, the
    1 -> 8 head, and the two 1x1 heads 32 -> 32 / 16 (the 1/4-resolution pair of the feature pyramid)."""
    b, h, w = shape
    exact, scale = gen[0] == "exact", (gen[1] if gen[0] == "exact" else 1.0)
    rs = M.rng(*shape, 5 if exact else 11 + M.CLASSES.index(gen[1]))
    mk = (lambda xs, ws: M.exact_operands(rs, xs, ws, scale=scale)) if exact else (lambda xs, ws: M.random_operands(rs, gen[1], xs, ws))
    sq = lambda o: dict(o, x=o["x"][:, 0], w=o["w"][:, :, 0], res=o["res"][:, 0])
    l1, l2, l3 = sq(mk((b, 1, h, w, 3), (8, 3, 1, 3, 3))), sq(mk((b, 1, h, w, 8), (8, 8, 1, 3, 3))), sq(mk((b, 1, h, w, 8), (8, 8, 1, 3, 3)))
    t1, t2 = sq(mk((b, 1, h, w, 8), (32, 8, 1, 3, 3))), sq(mk((b, 1, 2 * h, 2 * w, 8), (1, 8, 1, 3, 3)))
    hd = sq(mk((b, 1, h, w, 1), (8, 1, 1, 3, 3)))
    h1, h2 = sq(mk((b, 1, h, w, 32), (32, 32, 1, 1, 1))), sq(mk((b, 1, h, w, 32), (16, 32, 1, 1, 1)))
    f = np.float32
    if exact:
        lo = rs.randint(-3, 4, b).astype(f) * f(scale)
        span = rs.choice(np.array([0.5, 2.0, 4.0], dtype=f), size=b)
        depth = (lo[:, None, None] + hd["x"][..., 0] * span[:, None, None]).astype(f)              # (depth - lo) / span is the integer map again
    else:
        lo, span = rs.uniform(400, 500, b).astype(f), rs.uniform(300, 600, b).astype(f)
        depth = (lo[:, None, None] + span[:, None, None] * rs.uniform(0, 1, (b, h, w))).astype(f)
    return dict(l1=l1, l2=l2, l3=l3, t1=t1, t2=t2, hd=hd, h1=h1, h2=h2, lo=lo, span=span, depth=depth)


def _run_fused(p, valu, monkeypatch):
    """{name: (y, launch)} of the fused kernels on one operand set."""
    out = {}
    pack = lambda w: ops.pack_conv2d_weight(dev(w))
    l1, l2, l3, t1, t2, hd, h1, h2 = (p[k] for k in ("l1", "l2", "l3", "t1", "t2", "hd", "h1", "h2"))
    with nan_outputs():
        monkeypatch.setenv("MDF_CONV_PAIR_VALU", valu)
        out["pair"] = ops.conv2d_pair_planar(dev(l1["x"].transpose(0, 3, 1, 2)), pack(l1["w"]), dev(l1["alpha"]), dev(l1["beta"]), pack(l2["w"]),
                                             dev(l2["alpha"]), dev(l2["beta"])), launched()
        monkeypatch.delenv("MDF_CONV_PAIR_VALU")
        scale = float(np.float32(l2["res_scale"]))
        out["res_pair"] = ops.conv2d_res_pair(dev(l2["x"]), pack(l2["w"]), pack(l3["w"]), scale), launched()
        out["refine_tail"] = ops.refine_tail(dev(t1["x"]), ops.pack_conv2d_weight(ops.shuffle2_rows(dev(t1["w"]))), dev(t2["w"]), dev(p["lo"]),
                                             dev(p["span"])), launched()
        out["refine_head"] = ops.refine_head(dev(p["depth"]), dev(p["lo"]), dev(p["span"]), dev(hd["w"])), launched()
        b, h, w = p["depth"].shape
        if h % 2 == 0 and w % 2 == 0:
            ru = [h1["res_up"], None]
        else:
            ru = [None, None]
        heads = [(pack(h1["w"]), dev(h1["beta"]), 32, 32), (pack(h2["w"]), None, 32, 16)]
        out["heads"] = ops.conv1x1_heads(dev(h1["x"]), heads, [None if r is None else dev(r) for r in ru]), launched()
    return out, ru


def _ref_fused(p, ru, dtype=np.float64):
    l1, l2, l3, t1, t2, hd, h1, h2 = (p[k] for k in ("l1", "l2", "l3", "t1", "t2", "hd", "h1", "h2"))
    ref = {}
    y, a, _ = M.pair_planar_ref(l1["x"].transpose(0, 3, 1, 2), l1["w"], l1["alpha"], l1["beta"], l2["w"], l2["alpha"], l2["beta"], dtype)
    ref["pair"] = (y, a)
    y, a, _ = M.res_pair_ref(l2["x"], l2["w"], l3["w"], np.float32(l2["res_scale"]), dtype)
    ref["res_pair"] = (y, a)
    y, a, _ = M.refine_tail_ref(t1["x"], t1["w"], t2["w"], p["lo"], p["span"], dtype)
    ref["refine_tail"] = (y, a)
    ref["refine_head"] = M.refine_head_ref(p["depth"], p["lo"], p["span"], hd["w"], dtype)
    ref["heads"] = M.heads_ref(h1["x"], [(h1["w"], h1["beta"]), (h2["w"], None)], ru, dtype)
    return ref


FUSED_KERNELS = {"pair": {"1": "conv_pair_valu_kernel", "0": "conv_pair_kernel"}, "res_pair": "res_pair_kernel", "refine_tail": "refine_tail_kernel",
                 "refine_head": "refine_head_kernel", "heads": "conv1x1_heads_kernel"}


@pytest.mark.parametrize("valu", ["1", "0"])
@pytest.mark.parametrize("shape", M.FUSED_SHAPES)
def test_fused_kernels_exact_operands_bit_for_bit(shape, valu, monkeypatch):
    scales = (1.0,) + (SCALES if shape == (2, 13, 37) else ())                     # check 2 on the ragged batch-2 shape
    failures = []
    for scale in scales:
        p = _fused_operands(("exact", scale), shape)
        got, ru = _run_fused(p, valu, monkeypatch)
        ref = _ref_fused(p, ru)
        for name, (y, launch) in got.items():
            want_kernel = FUSED_KERNELS[name][valu] if name == "pair" else FUSED_KERNELS[name]
            if launch != want_kernel:
                failures.append((name, scale, f"{launch} ran"))
            ys, rs_ = (y, ref[name][0]) if name == "heads" else ([y], [ref[name][0]])
            if not all(bits_equal(a, b) for a, b in zip(ys, rs_)):
                failures.append((name, f"scale {scale:g}", f"not bit-exact [{launch}]"))
    assert not failures, failures


def _fused_fields(p, place):
    """{name: mask} of the fused kernels for a value planted at (b, h, w, c) of every x (depth map: (b, h, w)): the second layer's field
    of the first layer's field (the tail: through the PixelShuffle); a 1x1 head sees its own pixel.  The 3 -> 8 -> 8 pair and the Res
    block run both layers in the w-phase form: conv_mirror.receptive_mask's `wphase` field, columns w - 2 .. w + 2, per layer."""
    b, h, w, _ = place
    one = lambda shape: np.zeros(shape)
    ind = one(p["l2"]["x"].shape[:3] + (1,))[:, None]
    ind[b, 0, h, w, 0] = 1.0
    k3 = np.ones((1, 1, 1, 3, 3))
    f1 = (M.taps(ind, k3) > 0).astype(np.float64)
    k35 = np.ones((1, 1, 1, 3, 5))
    two = M.taps((M.taps(ind, k35) > 0).astype(np.float64), k35)[:, 0] > 0
    up = np.repeat(np.repeat(f1[:, 0], 2, axis=1), 2, axis=2)[:, None]
    return {"pair": two, "res_pair": two, "refine_tail": (M.taps(up, k3)[:, 0] > 0)[..., 0], "refine_head": f1[:, 0] > 0, "heads": ind[:, 0] > 0}


@pytest.mark.parametrize("valu", ["1", "0"])
def test_fused_kernels_nonfinite_locality(valu, monkeypatch):
    """Check 5 on the fused 2-D kernels at the ragged batch-2 shape: a planted NaN / +Inf changes nothing outside the two layers'
    composed field.  (Their inner ReLU is fmaxf, which turns a NaN into 0, so no NaN set is owed.)"""
    shape = (2, 13, 37)
    p0 = _fused_operands(("exact", 1.0), shape)
    clean, _ = _run_fused(p0, valu, monkeypatch)
    failures = []
    for value in PLANTS:
        for pi, pl in enumerate(M.plant_places((shape[0], 1) + shape[1:], 8)):
            place = (pl[0], pl[2], pl[3], pl[4])
            p = {k: (dict(v, x=v["x"].copy()) if isinstance(v, dict) else v.copy()) for k, v in p0.items()}
            for k in ("l1", "l2", "t1", "hd", "h1"):
                p[k]["x"][place[:3] + (min(place[3], p[k]["x"].shape[-1] - 1),)] = value
            p["depth"][place[:3]] = value
            got, _ = _run_fused(p, valu, monkeypatch)
            fields = _fused_fields(p, place)
            for name, (y, launch) in got.items():
                ys, cs = (y, clean[name][0]) if name == "heads" else ([y], [clean[name][0]])
                for a, c in zip(ys, cs):
                    a, c = a.cpu().numpy(), c.cpu().numpy()
                    mask = fields[name]
                    bad = locality(a, c, None, mask.reshape(mask.shape[:3] + (1,) * (a.ndim - 3)), True)
                    if bad:
                        failures.append((name, launch, value, pi, bad))
    assert not failures, failures


@pytest.mark.parametrize("cls", M.CLASSES)
def test_fused_kernels_random_bar(cls, monkeypatch):
    """Check 3 at the ragged batch-2 shape.  The yardstick of a fused pair is both layers' fp32 chains with the intermediate map an
    fp32 tensor; its distance from float64 includes that map's rounding, which any kernel that keeps the map in fp32 shares."""
    p = _fused_operands(("random", cls), (2, 13, 37))
    failures = []
    for valu in ("1", "0"):
        got, ru = _run_fused(p, valu, monkeypatch)
        ref, yard = _ref_fused(p, ru), _ref_fused(p, ru, np.float32)
        for name, (y, launch) in got.items():
            if name == "heads" or (valu == "0" and name != "pair"):      # (the heads: below; only the pair reads MDF_CONV_PAIR_VALU)
                continue
            a = ref[name][1]
            ratios = M.bar_ratios(M.metrics(y.cpu().numpy(), ref[name][0], a), M.metrics(yard[name][0], ref[name][0], a))
            print(f"{name:12s} [{launch}] random {cls:7s} e_hip / (1.5 e_32): " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
            if max(ratios.values()) > 1.0:
                failures.append((name, launch, ratios))
    # the two 1x1 heads without res_up (odd extents) and with it on the first head (even extents)
    for shape in ((2, 13, 37), (2, 64, 62)):
        p = _fused_operands(("random", cls), shape)
        got, ru = _run_fused(p, "1", monkeypatch)
        ref, yard = _ref_fused(p, ru), _ref_fused(p, ru, np.float32)
        ys, launch = got["heads"]
        assert launch == FUSED_KERNELS["heads"] and (ru[0] is not None) == (shape == (2, 64, 62))
        for i, y in enumerate(ys):
            ratios = M.bar_ratios(M.metrics(y.cpu().numpy(), ref["heads"][0][i], ref["heads"][1][i]),
                                  M.metrics(yard["heads"][0][i], ref["heads"][0][i], ref["heads"][1][i]))
            what = f"heads {i}{' +up' if ru[i] is not None else ''}"
            print(f"{what:12s} [{launch}] random {cls:7s} e_hip / (1.5 e_32): " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
            if max(ratios.values()) > 1.0:
                failures.append((what, shape, ratios))
    assert not failures, failures


# --------------------------------------------------------------------------- check 6: the input gradients
DGRAD3D = [(32, 16, 1, False), (16, 16, 1, False), (32, 32, 1, False), (64, 64, 1, False), (16, 8, 1, False), (8, 8, 1, False),
           (16, 32, 2, False), (32, 64, 2, False), (8, 16, 2, False), (64, 32, 2, True), (32, 16, 2, True), (16, 8, 2, True)]
DGRAD2D = [(8, 8, 3, 1), (16, 16, 3, 1), (32, 32, 3, 1), (64, 64, 3, 1), (8, 16, 5, 2), (16, 32, 5, 2), (32, 64, 5, 2)]
WSET = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0], dtype=torch.float64)


def _exact_layer_and_gradient(conv, xshape, g):
    """The module with weights of the exact generator in float64, an integer dy, and float64 autograd's input gradient."""
    conv = conv.double()
    with torch.no_grad():
        conv.weight.copy_(WSET[torch.randint(0, 5, conv.weight.shape, generator=g)])
    x = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
    y = conv(x)
    dy = torch.randint(-4, 5, y.shape, generator=g).double() * (torch.rand(y.shape, generator=g) >= 0.21)
    y.backward(dy)
    return conv, dy, x.grad


def _even(shape, first):
    return tuple(shape[:first]) + tuple(n + n % 2 for n in shape[first:])


@pytest.mark.parametrize("cin,cout,stride,tr", DGRAD3D)
def test_conv3d_dgrad_exact_operands_bit_for_bit(cin, cout, stride, tr):
    """train_ops.conv3d_dgrad on every layer kind of the regularisers against float64 autograd, with and without add_to.
    A stride-2 Conv3d: dgrad_pack maps the layer onto the transposed kernel, whose output is 2 * Do on every axis.  That is the input's
    shape only where its extents are even; at an odd extent it is one plane / row / column more (the gradient of the forward layer's
    zero padding).  Both shapes here have an odd extent: the function refuses them, and a call that does not name the input's shape;
    the values are checked at the same shapes rounded up to even extents."""
    from torch import nn
    from mdfnet_hip import train_ops
    for shape in ((2, 3, 7, 9), (1, 5, 6, 19)):
        s2 = stride == 2 and not tr
        convd = nn.Conv3d(cin, cout, 3, stride=2, padding=1, bias=False).to(DEV) if s2 else None
        if s2:
            b, d, h, w = shape
            dyd = torch.zeros(b, (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout, device=DEV)
            with pytest.raises(ValueError, match="odd input extents are not supported"):
                train_ops.conv3d_dgrad(convd, False, dyd, in_shape=(b, d, h, w, cin))
            with pytest.raises(ValueError, match="needs in_shape"):
                train_ops.conv3d_dgrad(convd, False, dyd)
            shape = _even(shape, 1)
        b, d, h, w = shape
        g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + stride + sum(shape))
        mod = (nn.ConvTranspose3d(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False) if tr
               else nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False))
        conv, dy, want = _exact_layer_and_gradient(mod, (b, cin, d, h, w), g)
        want = want.permute(0, 2, 3, 4, 1)
        convd, dyd = conv.float().to(DEV), ops.to_ndhwc(dy.float().to(DEV))
        with nan_outputs():
            dx = train_ops.conv3d_dgrad(convd, tr, dyd, in_shape=(b, d, h, w, cin))
        assert tuple(dx.shape) == (b, d, h, w, cin) and torch.equal(dx.cpu().double(), want), shape
        extra = torch.randint(-4, 5, dx.shape, generator=g).float()
        with nan_outputs():
            dx2 = train_ops.conv3d_dgrad(convd, tr, dyd, add_to=extra.to(DEV), in_shape=(b, d, h, w, cin))
        assert torch.equal(dx2.cpu().double(), want + extra.double()), shape


@pytest.mark.parametrize("cin,cout,k,stride", DGRAD2D)
def test_conv2d_dgrad_exact_operands_bit_for_bit(cin, cout, k, stride):
    """train_ops.conv2d_dgrad.  k5 s2 returns [2 Ho, 2 Wo]: (2,19,33) has odd H and W and is refused, as is a call that does not name
    the input's shape; its values are checked at (2,20,34)."""
    from torch import nn
    from mdfnet_hip import train_ops
    for shape in ((2, 19, 33), (2, 20, 34)):
        b, h, w = shape
        if k == 5 and (h % 2 or w % 2):
            convd = nn.Conv2d(cin, cout, 5, stride=2, padding=2, bias=False).to(DEV)
            dyd = torch.zeros(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout, device=DEV)
            with pytest.raises(ValueError, match="odd input extents are not supported"):
                train_ops.conv2d_dgrad(convd, dyd, in_shape=(b, h, w, cin))
            with pytest.raises(ValueError, match="needs in_shape"):
                train_ops.conv2d_dgrad(convd, dyd)
            continue
        g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + k + sum(shape))
        conv, dy, want = _exact_layer_and_gradient(nn.Conv2d(cin, cout, k, stride=stride, padding=(k - 1) // 2, bias=False), (b, cin, h, w), g)
        want = want.permute(0, 2, 3, 1)
        convd, dyd = conv.float().to(DEV), ops.to_nhwc(dy.float().to(DEV))
        with nan_outputs():
            dx = train_ops.conv2d_dgrad(convd, dyd, in_shape=(b, h, w, cin))
        assert tuple(dx.shape) == (b, h, w, cin) and torch.equal(dx.cpu().double(), want), shape


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3])
