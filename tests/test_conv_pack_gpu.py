"""Packed conv weight sets (csrc/conv_pack.h): every set the model uses is byte-identical to the one the library packed before
the layout moved into that header, and every segment of a set reaches the kernel that reads it.

`python tests/test_conv_pack_gpu.py golden OUT.json COMMIT` writes the digest file (run it with MDF_HIP_LIB pointing at a library
built from COMMIT); `python tests/test_conv_pack_gpu.py child` is one child process of the segment test."""
import ctypes
import functools
import hashlib
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
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_pack_digests.json")
SRC_DIRECT, SRC_SWAPFLIP, SRC_K5S2, SRC_PROB, SRC_SHUFFLE2, SRC_SWAP = range(6)      # train_ops._SRC_*


# --------------------------------------------------------------------------- 5. packed sets against the parent's digests
@functools.lru_cache(maxsize=None)
def signatures():
    """(is3d, transposed, mode, Cin_mem, Cout, ntaps, a0, a1) of every weight set the model packs: the training step's batched plan,
    and the eval route's per-layer packs (kSrcDirect sets of every conv module, of the prob head's slices and of the composed 1x1 heads
    of the feature pyramid, whose channel pairs are taken over all of {16, 32, 64}^2)."""
    from mdfnet_hip import train_ops
    from modelutil import build_model
    model = build_model().to(DEV).train()
    sigs = {tuple(j[2:]) for j in train_ops.PackPlan(model).jobs}
    for m in model.modules():
        if isinstance(m, nn.ConvTranspose3d):
            sigs.add((1, 1, SRC_DIRECT, m.in_channels, m.out_channels, 27, 0, 0))
        elif isinstance(m, nn.Conv3d) and m.out_channels == 1:
            sigs.add((0, 0, SRC_DIRECT, m.in_channels, 4, 9, 0, 0))              # ops.pack_prob_weight
        elif isinstance(m, nn.Conv3d):
            sigs.add((1, 0, SRC_DIRECT, m.in_channels, m.out_channels, 27, 0, 0))
        elif isinstance(m, nn.Conv2d):
            sigs.add((0, 0, SRC_DIRECT, m.in_channels, m.out_channels, m.kernel_size[0] ** 2, 0, 0))
    sigs |= {(0, 0, SRC_DIRECT, ci, co, 1, 0, 0) for ci in (16, 32, 64) for co in (16, 32, 64)}
    return sorted(sigs)


def source_numel(sig):
    is3d, tr, mode, cin, cout, ntaps, a0, a1 = sig
    if mode == SRC_K5S2:
        return cin * a0 * 25              # Conv2d(k5) weight [Cin_mem = its out_channels][a0 = its in_channels][5][5]
    if mode == SRC_PROB:
        return cin * 27                   # [1][Cin][3][3][3]
    return cin * cout * ntaps


def key_of(sig):
    return "3d%d tr%d mode%d cin%d cout%d taps%d a%d,%d" % sig


def pack_digests():
    """{key: {"size": size query, "batch": sha256 of the set packed through mdf_pack_job_fill + mdf_pack_batch, "single": the same
    through mdf_conv3d_pack_weights / mdf_conv_pack_weights (kSrcDirect sets)}}.  Buffers are zeroed first: a 3-D buffer has the
    size of the larger of the plain and the transposed layout."""
    from mdfnet_hip import lib
    L = lib()
    sigs = signatures()
    nb = int(L.mdf_pack_job_bytes())
    table = (ctypes.c_char * (nb * len(sigs)))()
    srcs, dsts, sizes, block_job, first = [], [], [], [], 0
    for i, sig in enumerate(sigs):
        is3d, tr, mode, cin, cout, ntaps, a0, a1 = sig
        n = source_numel(sig)
        srcs.append(((torch.arange(n) * 37) % 17 - 8).float().to(DEV))      # integers: every Winograd sum of quarter-multiples is exact
        sizes.append(int(L.mdf_conv3d_packed_size(cin, cout) if is3d else L.mdf_conv_packed_size(cin, cout, ntaps)))
        dsts.append(torch.zeros(sizes[-1], device=DEV))
        nblk = int(L.mdf_pack_job_fill(ctypes.addressof(table), i, srcs[-1].data_ptr(), dsts[-1].data_ptr(), is3d, tr, mode, cin, cout, ntaps,
                                       a0, a1, first))
        assert nblk > 0, (sig, L.mdf_last_error().decode())
        block_job += [i] * nblk
        first += nblk
    table_d = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(DEV)
    block_job_d = torch.tensor(block_job, dtype=torch.int32).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.mdf_pack_batch(table_d.data_ptr(), block_job_d.data_ptr(), first, stream) == 0, L.mdf_last_error().decode()
    torch.cuda.synchronize()
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    out = {}
    for sig, src, dst, size in zip(sigs, srcs, dsts, sizes):
        is3d, tr, mode, cin, cout, ntaps, a0, a1 = sig
        out[key_of(sig)] = d = {"size": size, "batch": sha(dst)}
        if mode == SRC_DIRECT:
            one = torch.zeros(size, device=DEV)
            rc = (L.mdf_conv3d_pack_weights(src.data_ptr(), one.data_ptr(), cin, cout, tr, stream) if is3d else
                  L.mdf_conv_pack_weights(src.data_ptr(), one.data_ptr(), cin, cout, ntaps, stream))
            assert rc == 0, (sig, L.mdf_last_error().decode())
            torch.cuda.synchronize()
            d["single"] = sha(one)
    return out


def test_packed_sets_are_byte_identical_to_the_parents():
    with open(DIGESTS) as f:
        golden = json.load(f)["sets"]
    got = pack_digests()
    sigs = {s[:6] for s in signatures()}
    # what the issue names: 3-D 8..64 channels direct / swap-flip / transposed; 2-D k3, k5, k1; the image layers; shuffle2; prob slices; k5-s2 dgrad parts
    for c in (8, 16, 32, 64):
        assert any(s[0] == 1 and c in s[3:5] for s in sigs), c
    for must in [(0, 0, SRC_DIRECT, 3, 8, 9), (0, 0, SRC_DIRECT, 1, 8, 9), (0, 0, SRC_DIRECT, 16, 32, 25), (0, 0, SRC_DIRECT, 32, 64, 25)]:
        assert must in sigs, must
    for is3d, tr, mode in [(1, 0, SRC_DIRECT), (1, 0, SRC_SWAPFLIP), (1, 1, SRC_DIRECT), (0, 0, SRC_SWAPFLIP), (0, 0, SRC_K5S2), (0, 0, SRC_PROB),
                           (0, 0, SRC_SHUFFLE2), (0, 0, SRC_SWAP)]:
        assert any(s[:3] == (is3d, tr, mode) for s in sigs), (is3d, tr, mode)
    assert len({s[7] for s in signatures() if s[2] == SRC_K5S2}) >= 2        # both parts of a split k5-s2 input gradient
    missing = sorted(set(got) - set(golden))
    assert not missing, f"no digest recorded for {missing}"
    bad = [k for k, d in got.items() if d != golden[k]]
    assert not bad, {k: (got[k], golden[k]) for k in bad[:4]}


# --------------------------------------------------------------------------- 6. every segment reaches its reader
ENVS = [{}, {"MDF_CONV_WD": "0"}, {"MDF_CONV_WINOGRAD": "0"}, {"MDF_CONV_WINOGRAD": "0", "MDF_CONV_RW": "0"}]
# the form of each launch, "rw%d wg%d" of the MDF_CONV_DEBUG line: 3-D (16, 8), 3-D (8, 8), 2-D (8, 8) k3.  (Without epilogue sums the
# 16 -> 8 depth-pair form is the streamed one, wg3; the 2-D 8 -> 8 set has a w-phase segment and no Winograd one.)
FORMS = [("rw2 wg3", "rw2 wg2", "rw2 wg0"), ("rw2 wg1", "rw2 wg0", "rw2 wg0"), ("rw2 wg0", "rw2 wg0", "rw2 wg0"), ("rw1 wg0", "rw1 wg0", "rw1 wg0")]
CASES3D = [(cin, cout, shape) for cin, cout in ((16, 8), (8, 8)) for shape in ((1, 3, 9, 33), (2, 5, 17, 40))]
CASE2D = (8, 8, (2, 19, 33))


def child():
    """conv3d_ndhwc / conv2d_nhwc of the cases, raw and with alpha, beta, ReLU and residual, against torch on the CPU."""
    from mdfnet_hip import ops

    def mark(s):
        sys.stderr.write(f"[case {s}]\n")
        sys.stderr.flush()

    for cin, cout, shape in CASES3D + [CASE2D]:
        g = torch.Generator().manual_seed(cin * 100 + cout + shape[-1])
        nd = len(shape) - 1
        x = torch.randn(shape[0], cin, *shape[1:], generator=g)
        wt = torch.randn(cout, cin, *([3] * nd), generator=g) / np.sqrt(3 ** nd * cin)
        alpha, beta = torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) * 0.4 - 0.2
        ref = (F.conv3d if nd == 3 else F.conv2d)(x, wt, None, 1, 1)
        res = torch.randn(ref.shape, generator=g)
        bc = (1, -1) + (1,) * nd
        exp = F.relu(ref * alpha.view(bc) + beta.view(bc)) + res
        if nd == 3:
            wp, xd, rd = ops.pack_conv3d_weight(wt.to(DEV), False), ops.to_ndhwc(x.to(DEV)), ops.to_ndhwc(res.to(DEV))
            mark(f"3d {cin} {cout} raw")
            raw = ops.from_ndhwc(ops.conv3d_ndhwc(xd, wp, cin, cout, 1, False)).cpu()
            mark(f"3d {cin} {cout} epi")
            epi = ops.from_ndhwc(ops.conv3d_ndhwc(xd, wp, cin, cout, 1, False, alpha.to(DEV), beta.to(DEV), True, rd)).cpu()
        else:
            wp, xd, rd = ops.pack_conv2d_weight(wt.to(DEV)), ops.to_nhwc(x.to(DEV)), ops.to_nhwc(res.to(DEV))
            mark(f"2d {cin} {cout} raw")
            raw = ops.from_nhwc(ops.conv2d_nhwc(xd, wp, cin, cout, 3, 1)).cpu()
            mark(f"2d {cin} {cout} epi")
            epi = ops.from_nhwc(ops.conv2d_nhwc(xd, wp, cin, cout, 3, 1, alpha.to(DEV), beta.to(DEV), True, rd)).cpu()
        np.testing.assert_allclose(raw.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(epi.numpy(), exp.numpy(), rtol=1e-4, atol=2e-5)
    mark("end")


def test_every_segment_reaches_the_kernel_that_reads_it():
    """Four fresh processes (MDF_CONV_WD, MDF_CONV_WINOGRAD and MDF_CONV_RW are read once per process), one after the other; the
    first that does not exit 0 ends the test, so nothing more starts on the GPU after a fault or a time limit."""
    for extra, forms in zip(ENVS, FORMS):
        env = dict(os.environ, MDF_CONV_LDS_MIN_VOXELS="0", MDF_CONV_DEBUG="1", **extra)
        for k in ("MDF_CONV_WD", "MDF_CONV_WINOGRAD", "MDF_CONV_RW"):
            if k not in extra:
                env.pop(k, None)
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, f"child {extra} exited {r.returncode}; no further child is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        # the launches of each case: the debug lines between its marker and the next
        launches, case = {}, None
        for line in r.stderr.splitlines():
            m = re.match(r"\[case (.*)\]$", line)
            if m:
                case = m.group(1)
                continue
            m = re.match(r"\[conv_lds<[\d,]+,(rw\d+ wg\d+) st(\d+)>\]", line)
            if m and case:
                assert m.group(2) == "0", line
                launches.setdefault(case, []).append(m.group(1))
        want = {f"3d 16 8 {v}": forms[0] for v in ("raw", "epi")}
        want.update({f"3d 8 8 {v}": forms[1] for v in ("raw", "epi")})
        want.update({f"2d 8 8 {v}": forms[2] for v in ("raw", "epi")})
        for case, form in want.items():
            n = 1 if case.startswith("2d") else 2          # the 3-D cases run at two shapes
            assert launches.get(case) == [form] * n, (extra, case, launches.get(case), form)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child()
    elif sys.argv[1] == "golden":
        sets = pack_digests()
        for k, d in sets.items():
            assert d.get("single", d["batch"]) == d["batch"], k
        with open(sys.argv[2], "w") as f:
            json.dump({"parent": sys.argv[3], "weights": "((arange(n) * 37) % 17 - 8).float()", "sets": sets}, f, indent=1, sort_keys=True)
        print(len(sets), "sets")
