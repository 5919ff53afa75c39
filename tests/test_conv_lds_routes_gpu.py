"""mdf_conv_lds_dispatch (csrc/conv_lds.hip) against the commit before its route rules became one table and its launch plan one function:
for every case the route (mdf_last_launch), the kernel instantiation and plan (the `conv_lds<...>` tuple, grid and items of the
MDF_CONV_DEBUG line; none where wino2d.hip, wino3d.hip, conv1x1.hip or conv3d.hip took the layer) and the bits of `y` must be what that
commit gave.  tests/golden/conv_lds_routes.json holds them; scripts/gen_conv_lds_routes.py wrote it with a library built from that commit
(MDF_HIP_LIB) and this module's own functions.  Only `y` is digested: the fp64 epilogue sums go through unordered atomics
(tests/test_train_gpu.py holds them to their bounds).

MDF_CONV_WD, MDF_CONV_WINOGRAD and MDF_CONV_RW are read once per process: one child process per setting (SETTINGS), each under its own
time limit, one after the other; the first that does not exit 0 ends the test and no further child starts.  Inside a child the per-call
switches are toggled case by case.  `python tests/test_conv_lds_routes_gpu.py child SETTING` is one child.

Cases that are pruned because their route cannot differ from the default setting's:
  * MDF_CONV_WD is read by the depth-pair forms alone, which take 3-D layers with 8 output channels: the wd0 / wd1 / wd2 children run those;
  * MDF_CONV_RW is read by the w-phase form alone: the wg0rw0 child runs the layers that have a w-phase row (the wg0 child runs them all);
  * every call-out and the s2d form need MDF_CONV_WINOGRAD: the wg0 children do not toggle MDF_CONV_WINO3D / WINO2D / K5_WINOGRAD*.

Shapes are INPUT shapes.  3-D (B,D,H,W): (1,1,5,7) one plane (the depth-pair forms need two), (1,3,9,33), (2,5,17,40) batch 2 and ragged
tiles.  PLAN3D = (1,6,75,400) on 32 -> 32 enters the plan's "lengthen the chunks until one round holds everything" branch: the Winograd
form's 133 KB of LDS give one block per CU, max_grid = 256; its tile is 8 x 32, so 10 x 13 = 130 tiles; D / 3 = 2 chunks of 3 planes are
260 items, between one and three rounds; one chunk of 6 planes is 130 <= 256 items and 10 * (6 + 2) < 9 * 2 * (3 + 2), so dch = 6 and the
line reads "items 130".  (Fewer than 129 tiles never leave the first round at D = 6; D < 6 has one chunk to begin with.)
2-D (B,H,W): (2,19,33), (4,5,70), and the even (2,20,34) for k5 s2 over the parity images and for res_up.  PLAN2D = (2,66,1000) on
8 -> 8: the w-phase kernel's tile is 4 x 64, 2 x 17 x 16 = 544 tiles, tiles / 2 = 272 blocks: above the floor of 256 and below that
kernel's 1024 resident blocks, so the grid is the unclamped quotient ("grid 272")."""
import functools
import json
import os
import re
import subprocess
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "mdf-net_amd"), os.path.join(_root, "tests")]

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_lds_routes.json")

SETTINGS = {"default": {}, "wd0": {"MDF_CONV_WD": "0"}, "wd1": {"MDF_CONV_WD": "1"}, "wd2": {"MDF_CONV_WD": "2"},
            "wg0": {"MDF_CONV_WINOGRAD": "0"}, "wg0rw0": {"MDF_CONV_WINOGRAD": "0", "MDF_CONV_RW": "0"}}
PER_PROCESS = ("MDF_CONV_WD", "MDF_CONV_WINOGRAD", "MDF_CONV_RW")
PER_CALL = ("MDF_CONV_WINO3D", "MDF_CONV_WINO2D", "MDF_CONV_WD_STREAM", "MDF_CONV_K5_WINOGRAD", "MDF_CONV_K5_WINOGRAD_64", "MDF_CONV1X1")
CHILD_SECONDS = 240

SHAPES3D = [(1, 1, 5, 7), (1, 3, 9, 33), (2, 5, 17, 40)]
PLAN3D = (1, 6, 75, 400)
PAIRS3D = [(8, 8), (16, 8), (16, 16), (32, 16), (32, 32), (16, 32), (8, 16), (64, 64)]      # (64, 64) has no row: conv3d.hip's kernel
SHAPES2D = [(2, 19, 33), (4, 5, 70)]
EVEN2D = (2, 20, 34)
PLAN2D = (2, 66, 1000)
K3 = [(3, 8), (1, 8), (8, 8), (16, 16), (32, 32), (64, 64), (16, 32), (32, 64), (8, 32), (8, 1), (32, 8), (16, 4), (8, 4)]
K5 = [(8, 16), (16, 32), (32, 64), (32, 16)]                                                 # (32, 16) k5 s2 is not built: the entry's error
K1 = [(16, 32), (16, 64), (32, 64), (64, 16), (64, 32), (64, 64), (32, 32), (32, 16), (16, 16)]
RW_LAYERS3D = [(16, 8), (8, 8)]
RW_LAYERS2D = [(16, 4), (8, 4), (8, 8), (3, 8), (1, 8)]

# every row of the table in conv_lds.hip, as the tuple of its debug line, and whether its ST 1 / ST 2 kernels are built
ROWS = [("64,64,32,1,3,1,1,rw2 wg1", False),                                                                  # s2d
        ("8,8,8,3,3,1,1,rw2 wg2", True), ("16,16,8,3,3,1,1,rw2 wg3", False), ("16,16,8,3,3,1,1,rw2 wg2", True),      # depth-pair
        ("16,16,16,3,3,1,1,rw2 wg1", True), ("32,32,16,3,3,1,1,rw2 wg1", True), ("32,32,32,3,3,1,1,rw2 wg1", True),
        ("16,16,8,3,3,1,1,rw2 wg1", True), ("16,16,32,3,3,1,1,rw2 wg1", True),                                 # Winograd 3-D
        ("16,16,16,1,3,1,1,rw2 wg1", True), ("32,32,32,1,3,1,1,rw2 wg1", True), ("64,64,64,1,3,1,1,rw2 wg1", True),
        ("16,16,32,1,3,1,1,rw2 wg1", True), ("32,32,64,1,3,1,1,rw2 wg1", True),                                # Winograd 2-D
        ("16,16,8,3,3,1,2,rw2 wg0", True), ("8,8,8,3,3,1,2,rw2 wg0", True), ("16,16,4,1,3,1,1,rw4 wg0", False),
        ("8,8,4,1,3,1,1,rw4 wg0", False), ("8,8,8,1,3,1,2,rw2 wg0", True), ("4,3,8,1,3,1,2,rw2 wg0", True),
        ("4,1,8,1,3,1,2,rw2 wg0", False),                                                                      # w-phase
        ("32,32,16,3,3,1,2,rw1 wg0", False), ("16,16,16,3,3,1,4,rw1 wg0", False), ("16,16,8,3,3,1,4,rw1 wg0", False),
        ("8,8,8,3,3,1,4,rw1 wg0", False), ("32,32,32,3,3,1,2,rw1 wg0", False), ("16,16,32,3,3,1,2,rw1 wg0", False),
        ("8,8,16,3,3,1,4,rw1 wg0", False),                                                                     # plain 3-D
        ("4,3,8,1,3,1,4,rw1 wg0", False), ("8,8,8,1,3,1,4,rw1 wg0", False), ("16,16,16,1,3,1,4,rw1 wg0", False),
        ("32,32,32,1,3,1,2,rw1 wg0", False), ("64,64,64,1,3,1,1,rw1 wg0", False),
        ("8,8,16,1,5,2,2,rw1 wg0", True), ("16,16,32,1,5,2,2,rw1 wg0", True), ("32,32,64,1,5,2,1,rw1 wg0", True),
        ("16,16,32,1,1,1,4,rw1 wg0", False), ("16,16,64,1,1,1,4,rw1 wg0", False), ("32,32,64,1,1,1,2,rw1 wg0", False),
        ("64,64,16,1,1,1,1,rw1 wg0", False), ("64,64,32,1,1,1,1,rw1 wg0", False), ("64,64,64,1,1,1,1,rw1 wg0", False),
        ("32,32,32,1,1,1,2,rw1 wg0", False), ("32,32,16,1,1,1,2,rw1 wg0", False), ("16,16,16,1,1,1,4,rw1 wg0", False),
        ("4,1,8,1,3,1,4,rw1 wg0", False), ("8,8,32,1,3,1,4,rw1 wg0", False), ("8,8,1,1,3,1,4,rw1 wg0", False),
        ("32,32,8,1,3,1,2,rw1 wg0", False), ("16,16,32,1,3,1,2,rw1 wg0", False), ("32,32,64,1,3,1,1,rw1 wg0", False),
        ("16,16,4,1,3,1,4,rw1 wg0", False), ("8,8,4,1,3,1,4,rw1 wg0", False)]                                  # plain 2-D
EXPECTED_KERNELS = {f"{t} st{st}" for t, train in ROWS for st in ((0, 1, 2) if train else (0,))}


# --------------------------------------------------------------------------- the cases of a setting
def cases(setting):
    """[(name, kind, args, per-call switches)]; kind "3d": (cin, cout, shape, variant), "2d": (cin, cout, k, stride, shape, variant)."""
    wg = "MDF_CONV_WINOGRAD" not in SETTINGS[setting]
    out = []

    def add3(cin, cout, shape, variant, **env):
        tag = "".join(f" {k[4:]}={v}" for k, v in sorted(env.items()))
        out.append((f"3d {cin}->{cout} {shape} {variant}{tag}", "3d", (cin, cout, shape, variant), env))

    def add2(cin, cout, k, s, shape, variant, **env):
        tag = "".join(f" {k_[4:]}={v}" for k_, v in sorted(env.items()))
        out.append((f"2d {cin}->{cout} k{k}s{s} {shape} {variant}{tag}", "2d", (cin, cout, k, s, shape, variant), env))

    pairs3 = PAIRS3D if setting in ("default", "wg0") else ([p for p in PAIRS3D if p[1] == 8] if setting.startswith("wd") else RW_LAYERS3D)
    for cin, cout in pairs3:
        for shape in SHAPES3D:
            for variant in ("raw", "epi", "st1", "st2"):
                add3(cin, cout, shape, variant)
            if wg and cout % 16 == 0:                      # wino3d.hip off: the Winograd rows, eval
                add3(cin, cout, shape, "raw", MDF_CONV_WINO3D="0")
                add3(cin, cout, shape, "epi", MDF_CONV_WINO3D="0")
            if wg and (cin, cout) == (16, 8):              # ring of 4 planes, eval
                add3(cin, cout, shape, "raw", MDF_CONV_WD_STREAM="0")
                add3(cin, cout, shape, "epi", MDF_CONV_WD_STREAM="0")
    if setting == "default":
        add3(32, 32, PLAN3D, "raw", MDF_CONV_WINO3D="0")
        add3(32, 32, PLAN3D, "st1")
        add3(16, 16, SHAPES3D[1], "raw", MDF_CONV_LDS_MIN_VOXELS="150000")      # below conv3d.hip's threshold: its own kernels
    if setting.startswith("wd"):
        return out

    full = setting in ("default", "wg0")
    for cin, cout in (K3 if full else RW_LAYERS2D):
        planar = cin < 4
        for shape in SHAPES2D + [EVEN2D]:
            for variant in ("raw", "epi"):
                add2(cin, cout, 3, 1, shape, variant)
                if wg and cin == cout and cin >= 32:       # wino2d.hip off: the Winograd rows, eval
                    add2(cin, cout, 3, 1, shape, variant, MDF_CONV_WINO2D="0")
            if planar:
                add2(cin, cout, 3, 1, shape, "nhwc")       # the image layer from an NHWC tensor (raw / epi take it planar)
            if cout % 4 == 0 and cout >= 8 and shape != EVEN2D:
                for variant in ("st1g1", "st1g2", "st2g1", "st2g2"):
                    add2(cin, cout, 3, 1, shape, variant)
            if cout % 4 == 0 and shape == EVEN2D:
                add2(cin, cout, 3, 1, shape, "resup")
            if cout == 32 or (cin, cout) == (32, 64):
                add2(cin, cout, 3, 1, shape, "shuf")
    if setting == "default":
        add2(8, 8, 3, 1, PLAN2D, "raw")
        add2(8, 8, 3, 1, PLAN2D, "st1g2")
    if not full:
        return out
    for cin, cout in K5:
        for shape in SHAPES2D + [EVEN2D]:
            for variant in ("raw", "epi", "st1g1", "st2g2"):
                add2(cin, cout, 5, 2, shape, variant)
            if wg and shape == EVEN2D:
                for env in ({"MDF_CONV_WINO2D": "0"}, {"MDF_CONV_K5_WINOGRAD": "0"}, {"MDF_CONV_K5_WINOGRAD_64": "0"}):
                    add2(cin, cout, 5, 2, shape, "raw", **env)
                    add2(cin, cout, 5, 2, shape, "epi", **env)
    for cin, cout in K1:
        for shape in (SHAPES2D[0], EVEN2D):
            for variant in ("raw", "epi") + (("resup",) if shape == EVEN2D else ()):
                add2(cin, cout, 1, 1, shape, variant)
                if setting == "default":
                    add2(cin, cout, 1, 1, shape, variant, MDF_CONV1X1="0")
    return out


# --------------------------------------------------------------------------- one child process
@functools.lru_cache(maxsize=None)
def layer2d(cin, cout, k, stride, shape):
    """Host-seeded operands of one 2-D layer at one shape: x (NHWC), packed weights, alpha, beta, res, res_up, stat_y, aux (2 groups)."""
    from mdfnet_hip import ops
    b, h, w = shape
    rs = np.random.RandomState((cin * 131 + cout) * 7 + k * 1000 + stride * 100 + sum(shape))
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(DEV)
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x = f(b, h, w, cin)
    wp = ops.pack_conv2d_weight(f(cout, cin, k, k) / float(np.sqrt(k * k * cin)))
    alpha = torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32)).to(DEV)
    beta = torch.from_numpy(rs.uniform(-0.2, 0.2, cout).astype(np.float32)).to(DEV)
    res, res_up, stat_y = f(b, ho, wo, cout), f(b, max(ho // 2, 1), max(wo // 2, 1), cout), f(b, ho, wo, cout) * 2 + 0.3
    aux = torch.from_numpy(np.concatenate([np.concatenate([rs.uniform(0.5, 1.5, cout), rs.standard_normal(cout) * 0.3,
                                                           rs.standard_normal(cout) * 0.2, rs.uniform(0.5, 1.5, cout)])
                                           for _ in range(2)]).astype(np.float32)).to(DEV)
    return x, wp, alpha, beta, res, res_up, stat_y, aux


def run3d(cin, cout, shape, variant):
    import test_conv3d_digests_gpu as T
    if variant in ("raw", "epi"):
        return T.fwd(cin, cout, "s1", shape, variant == "epi", variant == "epi")
    return T.train(cin, cout, "s1", shape, int(variant[2]), variant == "st2")


def run2d(cin, cout, k, stride, shape, variant, res_scale=0.1):
    from mdfnet_hip import ops
    x, wp, alpha, beta, res, res_up, stat_y, aux = layer2d(cin, cout, k, stride, shape)
    planar = cin < 4 and variant != "nhwc"
    if planar:
        x = x.permute(0, 3, 1, 2).contiguous()
    if variant.startswith("st"):
        mode, groups = int(variant[2]), int(variant[4])
        sums = torch.zeros(ops.STAT_SLICES, groups * 2 * cout, device=DEV, dtype=torch.float64)
        return ops.conv2d_train(x, wp, cin, cout, k, stride, planar, mode, sums, groups, stat_y if mode == 2 else None,
                                aux[:groups * 4 * cout] if mode == 2 else None)
    if variant == "epi":
        return ops.conv2d_nhwc(x, wp, cin, cout, k, stride, alpha, beta, True, res, res_scale, planar_in=planar)
    if variant == "resup":
        return ops.conv2d_nhwc(x, wp, cin, cout, k, stride, alpha, beta, False, res_up=res_up, planar_in=planar)
    return ops.conv2d_nhwc(x, wp, cin, cout, k, stride, planar_in=planar, pixel_shuffle2=(variant == "shuf"))


def child(setting):
    """Every case of the setting; on stderr, around the library's own MDF_CONV_DEBUG lines: `[case NAME]` before the call and
    `[done] {"launch": ..., "y": ...}` after it."""
    import mdfnet_hip
    from test_conv3d_digests_gpu import sha
    for name, kind, args, env in cases(setting):
        for k in PER_CALL:
            os.environ.pop(k, None)
        os.environ["MDF_CONV_LDS_MIN_VOXELS"] = "0"
        os.environ.update(env)
        sys.stderr.write(f"[case {name}]\n")
        sys.stderr.flush()
        try:
            y = (run3d if kind == "3d" else run2d)(*args)
            rec = {"launch": mdfnet_hip.lib().mdf_last_launch().decode(), "y": sha(y)}
        except mdfnet_hip.MdfHipError as e:       # an entry's refusal (MDF_EUNSUPPORTED, -2) is a route too: its message is the record
            if " failed with code -2: " not in str(e):
                raise                                 # anything else, a HIP error included, ends the child: nothing more starts on the GPU
            rec = {"launch": f"error: {e}", "y": None}
        sys.stderr.write("[done] " + json.dumps(rec) + "\n")
        sys.stderr.flush()


_child_failed = []


@functools.lru_cache(maxsize=None)
def records(setting):
    """{case: {"launch", "lds": the conv_lds tuples, grids and items of the call, "y"}} of one fresh process."""
    assert not _child_failed, f"child {_child_failed[0]} did not exit 0: no further child is started"
    env = dict(os.environ, MDF_CONV_DEBUG="1", **SETTINGS[setting])
    for k in PER_PROCESS + PER_CALL:
        if k not in SETTINGS[setting]:
            env.pop(k, None)
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "child", setting], env=env,
                       capture_output=True, text=True)
    if r.returncode != 0:
        _child_failed.append(setting)
    assert r.returncode == 0, f"child {setting} exited {r.returncode}; no further child is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out, case, lds = {}, None, []
    for line in r.stderr.splitlines():
        m = re.match(r"\[case (.*)\]$", line)
        if m:
            case, lds = m.group(1), []
            continue
        m = re.match(r"\[conv_lds<([\d,]+,rw\d+ wg\d+ st\d+)>\] .*, grid (\d+), items (\d+)$", line)
        if m and case:
            lds.append(f"{m.group(1)} grid {m.group(2)} items {m.group(3)}")
        if line.startswith("[done] ") and case:
            out[case] = dict(json.loads(line[7:]), lds=lds)
            case = None
    assert sorted(out) == sorted(c[0] for c in cases(setting)), "a case left no record"
    return out


def all_records():
    return {s: records(s) for s in SETTINGS}


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["settings"]


# --------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_routes_plans_and_bits_are_the_parents(setting):
    want, got = golden()[setting], records(setting)
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, dict(list(bad.items())[:4])


def test_every_row_of_the_table_is_launched():
    """Eval and, where built, ST 1 and ST 2; and nothing launches that the list above does not name."""
    seen = {l.split(" grid ")[0] for recs in all_records().values() for r in recs.values() for l in r["lds"]}
    assert seen == EXPECTED_KERNELS, (sorted(EXPECTED_KERNELS - seen), sorted(seen - EXPECTED_KERNELS))


def test_both_sides_of_every_form_condition():
    d, wg0 = records("default"), records("wg0")
    kern = lambda r: [l.split(" grid ")[0] for l in r["lds"]]
    # depth-pair at D = 1 falls to the next form, at D >= 2 it launches (16 -> 8: streamed in eval, the ring of 4 with sums)
    assert kern(d["3d 8->8 (1, 1, 5, 7) raw"]) == ["8,8,8,3,3,1,2,rw2 wg0 st0"] and kern(d["3d 8->8 (1, 3, 9, 33) raw"]) == ["8,8,8,3,3,1,1,rw2 wg2 st0"]
    assert kern(d["3d 16->8 (1, 1, 5, 7) raw"]) == ["16,16,8,3,3,1,1,rw2 wg1 st0"] and kern(d["3d 16->8 (1, 3, 9, 33) raw"]) == ["16,16,8,3,3,1,1,rw2 wg3 st0"]
    assert kern(d["3d 16->8 (1, 3, 9, 33) st1"]) == ["16,16,8,3,3,1,1,rw2 wg2 st1"]
    assert kern(d["3d 16->8 (1, 3, 9, 33) raw CONV_WD_STREAM=0"]) == ["16,16,8,3,3,1,1,rw2 wg2 st0"]
    # k5 s2: odd H or W on the direct kernel, even on wino2d.hip, or -- without it -- on the s2d form
    assert kern(d["2d 16->32 k5s2 (2, 19, 33) raw"]) == ["16,16,32,1,5,2,2,rw1 wg0 st0"]
    assert d["2d 16->32 k5s2 (2, 20, 34) raw"]["launch"] == "wino2d_kernel" and not d["2d 16->32 k5s2 (2, 20, 34) raw"]["lds"]
    assert kern(d["2d 16->32 k5s2 (2, 20, 34) raw CONV_WINO2D=0"]) == ["64,64,32,1,3,1,1,rw2 wg1 st0"]
    assert kern(d["2d 32->64 k5s2 (2, 20, 34) raw CONV_K5_WINOGRAD_64=0"]) == ["32,32,64,1,5,2,1,rw1 wg0 st0"]
    # res_up: the plain form only
    assert kern(d["2d 16->16 k3s1 (2, 20, 34) raw"]) == ["16,16,16,1,3,1,1,rw2 wg1 st0"] and kern(d["2d 16->16 k3s1 (2, 20, 34) resup"]) == ["16,16,16,1,3,1,4,rw1 wg0 st0"]
    assert kern(d["2d 8->8 k3s1 (2, 20, 34) raw"]) == ["8,8,8,1,3,1,2,rw2 wg0 st0"] and kern(d["2d 8->8 k3s1 (2, 20, 34) resup"]) == ["8,8,8,1,3,1,4,rw1 wg0 st0"]
    # shuffle2: 8 -> 32 has the plain form only; 16 -> 32 and 32 -> 64 the Winograd form, and without it 32 -> 64 is refused
    assert kern(d["2d 8->32 k3s1 (2, 19, 33) shuf"]) == ["8,8,32,1,3,1,4,rw1 wg0 st0"]
    assert kern(d["2d 16->32 k3s1 (2, 19, 33) shuf"]) == ["16,16,32,1,3,1,1,rw2 wg1 st0"] and kern(d["2d 32->64 k3s1 (2, 19, 33) shuf"]) == ["32,32,64,1,3,1,1,rw2 wg1 st0"]
    assert kern(wg0["2d 16->32 k3s1 (2, 19, 33) shuf"]) == ["16,16,32,1,3,1,2,rw1 wg0 st0"]
    assert wg0["2d 32->64 k3s1 (2, 19, 33) shuf"]["launch"].endswith("conv2d Cin=32 Cout=64 k=3 stride=1 is not built")
    # the image layer: planar and NHWC input, Cin_mem 3 and 1
    assert kern(d["2d 3->8 k3s1 (2, 19, 33) raw"]) == kern(d["2d 3->8 k3s1 (2, 19, 33) nhwc"]) == ["4,3,8,1,3,1,2,rw2 wg0 st0"]
    assert kern(d["2d 1->8 k3s1 (2, 19, 33) raw"]) == ["4,1,8,1,3,1,2,rw2 wg0 st0"]
    # a channel pair without a row comes back as conv3d.hip's kernel
    assert not d["3d 64->64 (1, 3, 9, 33) raw"]["lds"] and d["3d 64->64 (1, 3, 9, 33) raw"]["launch"].startswith("conv3d")
    # the two plan shapes (module docstring)
    assert d["3d 32->32 (1, 6, 75, 400) raw CONV_WINO3D=0"]["lds"] == ["32,32,32,3,3,1,1,rw2 wg1 st0 grid 130 items 130"]
    assert d["2d 8->8 k3s1 (2, 66, 1000) raw"]["lds"] == ["8,8,8,1,3,1,2,rw2 wg0 st0 grid 272 items 272"]


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2])
