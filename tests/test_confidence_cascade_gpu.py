"""GPU: confidence_cascade_kernel (csrc/regress.hip) through the C ABI, the op, the slot functions and the model.

The kernel is held to the bits of tests/confidence_mirror.py (its operation order written down in numpy fp32), to the bits of the
two kernels it extends (confidence_kernel, confidence_up2_kernel) where it computes the same thing, and to the reference's own code
on .double() inputs (tests/golden/confidence_cascade.npz) with the bars tests/test_confidence_cascade_cpu.py derives: 2e-6 per call,
6e-6 at the end of the three-stage chain.  Shapes: a one-pixel `last` (every tap clamps), one row / one column of `last`, ragged maps,
two batch items, the templated D = 8 and generic D, more than one block, and one DTU last-stage map with the x2 placement."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import confidence_mirror as C  # noqa: E402
import heads_mirror as M  # noqa: E402
import mdfnet_hip  # noqa: E402
from mdfnet_hip import ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
BAR_CALL, BAR_CHAIN = 2e-6, 6e-6

# (B, D, H, W), up2
# (D = 48, 24 and 8 are the kernel's register forms, every other D its generic form: 1, 5 and 17 here, 17 with more than one block)
CASES = [((1, 1, 2, 2), False), ((1, 8, 2, 4), False), ((1, 8, 4, 2), False), ((2, 8, 6, 10), False), ((2, 24, 34, 66), False),
         ((1, 5, 10, 14), False), ((2, 17, 34, 66), False), ((1, 48, 6, 10), False), ((1, 8, 592, 800), True)]
IDS = ["x".join(map(str, s)) + ("-up2" if u else "") for s, u in CASES]


def dev(a):
    return None if a is None else T(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def assert_bits(got, want, what):
    bad = ~M.same_bits(got, want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {i}: kernel {got[i]!r} mirror {want[i]!r}")


def _seed(shape):
    b, d, h, w = shape
    return (b * 1000003 + h * 10007 + w * 101 + d) % (2 ** 31 - 1)


def _volumes(shape):
    """-> [(name, prob)]: heads_mirror's mixed softmax volume (random, peaked, uniform, one-hot pixels, exact zeros, denormals), one
    one-hot volume (the hot plane walks over D, so windows run off both ends) and one all-zero volume."""
    b, d, h, w = shape
    plane = (np.arange(h * w).reshape(1, 1, h, w) + np.arange(b).reshape(b, 1, 1, 1)) % d
    onehot = (np.arange(d).reshape(1, d, 1, 1) == plane).astype(np.float32)
    return [("softmax", M.make_probs(b, d, h, w, _seed(shape))[0]), ("one-hot", onehot), ("zero", np.zeros(shape, np.float32))]


def _last(shape, seed_offset=0):
    """A seeded uniform map in [-0.25, 1.25] (what a cascade confidence can be, and a little more) at half the resolution."""
    b, _, h, w = shape
    return np.random.RandomState(_seed(shape) + 17 + seed_offset).uniform(-0.25, 1.25, (b, h // 2, w // 2)).astype(np.float32)


# --------------------------------------------------------------------------- kernel == mirror, == the kernels it extends
@pytest.mark.parametrize("shape,up2", CASES, ids=IDS)
def test_bits_of_the_mirror_and_of_the_old_kernels(shape, up2):
    last = _last(shape)
    lg = dev(last)
    for name, prob in _volumes(shape):
        pg = dev(prob)
        got = host(ops.confidence_cascade(pg, lg, up2=up2))
        assert mdfnet_hip.lib().mdf_last_launch().decode() == "confidence_cascade_kernel"
        assert got.shape == ((shape[0], 2 * shape[2], 2 * shape[3]) if up2 else (shape[0],) + shape[2:]) and got.dtype == np.float32
        assert_bits(got, C.cascade(prob, last, up2=up2), f"{name}: with last")
        # placement of the x2: every value at its 2x2 pixels
        other = host(ops.confidence_cascade(pg, lg, up2=not up2))
        small, big = (other, got) if up2 else (got, other)
        assert_bits(big, np.repeat(np.repeat(small, 2, axis=1), 2, axis=2), f"{name}: up2 placement")
        # without last, at the default window: the bits of confidence_kernel and of confidence_up2_kernel
        assert_bits(host(ops.confidence_cascade(pg)), host(ops.confidence(pg)), f"{name}: last=None vs confidence_kernel")
        assert_bits(host(ops.confidence_cascade(pg, up2=True)), host(ops.confidence_up2(pg)), f"{name}: last=None, up2 vs confidence_up2_kernel")
        assert_bits(host(ops.confidence_cascade(pg)), C.cascade(prob), f"{name}: last=None vs mirror")
        # other weights are arguments of the entry, not constants of the kernel
        assert_bits(host(ops.confidence_cascade(pg, lg, weights=(0.25, 1.5))), C.cascade(prob, last, weights=(0.25, 1.5)), f"{name}: weights")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (2, 8, 6, 10), (2, 24, 34, 66), (1, 5, 10, 14), (1, 48, 6, 10)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n,pf", [(2, 0), (1, 0), (8, 3), (4, 0), (2, 5)], ids=lambda v: str(v))
def test_other_windows(shape, n, pf):
    """The reference's commented alternative n=2, pad=(0,0,0,0,0,1) and the other window lengths, with and without last."""
    last = _last(shape, 1)
    for name, prob in _volumes(shape):
        assert_bits(host(ops.confidence_cascade(dev(prob), None, n, pf)), C.cascade(prob, None, n, pf), f"{name}: n={n} pf={pf}")
        assert_bits(host(ops.confidence_cascade(dev(prob), dev(last), n, pf, up2=True)), C.cascade(prob, last, n, pf, up2=True),
                    f"{name}: n={n} pf={pf} with last, up2")


def test_other_window_against_the_golden(golden):
    g, o = golden("confidence_cascade.npz"), golden("ops.npz")
    for s in range(3):
        prob = o[f"reg{s}_prob"]
        got = host(ops.confidence_cascade(dev(prob), None, 2, 0))
        assert_bits(got, C.cascade(prob, None, 2, 0), f"stage {s}")
        d = float(np.abs(got.astype(np.float64) - g[f"n2_64_c{s}"]).max())
        print(f"n=2, pad=(0,1), stage {s}: max |kernel - float64| = {d:.3e}")
        assert d <= BAR_CALL


def test_nonfinite_last():
    """A NaN and an inf planted in last: the same non-finite positions (and the same finite bits elsewhere) as the mirror."""
    shape = (2, 8, 12, 20)
    prob = M.make_probs(*shape, 77)[0]
    last = _last(shape)
    last[0, 2, 3], last[1, 0, 0], last[1, 5, 9] = np.nan, np.inf, -np.inf
    got, want = host(ops.confidence_cascade(dev(prob), dev(last))), C.cascade(prob, last)
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isposinf(got) == np.isposinf(want)).all() and (np.isneginf(got) == np.isneginf(want)).all()
    assert np.isnan(want).sum() >= 16 and np.isfinite(want).sum() > 0          # a planted value reaches its 4x4 .. 8x8 outputs only
    assert_bits(got, want, "non-finite last")


# --------------------------------------------------------------------------- the reference in float64
def test_golden_chain(golden):
    g, o = golden("confidence_cascade.npz"), golden("ops.npz")
    probs = [o[f"reg{s}_prob"] for s in range(3)]
    c, devs = None, []
    for s, p in enumerate(probs):
        alone = host(ops.confidence_cascade(dev(p), None if s == 0 else dev(g[f"chain64_c{s - 1}"].astype(np.float32))))
        d_alone = float(np.abs(alone.astype(np.float64) - g[f"chain64_c{s}"]).max())
        c = ops.confidence_cascade(dev(p), c)
        devs.append(float(np.abs(host(c).astype(np.float64) - g[f"chain64_c{s}"]).max()))
        print(f"stage {s}: max |kernel - float64|: this call alone {d_alone:.3e}, along the chain {devs[-1]:.3e}")
        assert d_alone <= BAR_CALL
    assert devs[0] <= BAR_CALL and devs[1] <= BAR_CHAIN and devs[2] <= BAR_CHAIN
    mirror = C.chain(probs)
    assert_bits(host(c), mirror[2], "chain on the GPU vs mirror")
    up = host(ops.confidence_cascade(dev(g["up_prob"]), dev(g["up_last"])))
    d = float(np.abs(up.astype(np.float64) - g["up_64"]).max())
    print(f"[2,5,7] -> [2,10,14]: max |kernel - float64| = {d:.3e}")
    assert d <= BAR_CALL


def test_slot_functions(golden):
    """confidence_regress: the default call keeps its route (mdf_confidence_fwd); anything else is the new kernel; confidence_cascade
    is the new kernel always.  Same arithmetic."""
    from net.unit import regress
    o = golden("ops.npz")
    p1, p2 = dev(o["reg1_prob"]), dev(o["reg2_prob"])
    ops.count_begin()
    c1 = regress.confidence_regress(p1)
    assert ops.count_end() == {"mdf_confidence_fwd": 1}
    ops.count_begin()
    c2 = regress.confidence_regress(p2, c1)
    c2n = regress.confidence_regress(p2, n=2, pad=(0, 0, 0, 0, 0, 1))
    k1 = regress.confidence_cascade(p1)
    k2 = regress.confidence_cascade(p2, last_confidence=k1, up2=True)
    assert ops.count_end() == {"mdf_confidence_cascade_fwd": 4}
    assert torch.equal(c1, k1) and torch.equal(k2, M_up2(c2))
    assert_bits(host(c2), C.cascade(o["reg2_prob"], host(c1)), "confidence_regress(prob, last)")
    assert_bits(host(c2n), C.cascade(o["reg2_prob"], None, 2, 0), "confidence_regress(n=2, pad=(0,1))")


def M_up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


# --------------------------------------------------------------------------- ABI rejections
def test_abi_rejections_launch_nothing():
    lib = mdfnet_hip.lib()
    prob = torch.rand(1, 8, 6, 10, device=DEV)
    last = torch.rand(1, 3, 5, device=DEV)
    out = torch.full((1, 6, 10), -7.0, device=DEV)
    ops.confidence(prob)                                  # so that the last launch is another kernel's
    torch.cuda.synchronize()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())         # noqa: E731
    f = ctypes.c_float
    call = lambda p, l, n, pf, c, H: lib.mdf_confidence_cascade_fwd(p, l, f(0.8), f(0.2), n, pf, 0, c, 1, 8, H, 10, st)   # noqa: E731
    assert call(None, ptr(last), 4, 1, ptr(out), 6) == -1 and "null" in lib.mdf_last_error().decode()
    assert call(ptr(prob), ptr(last), 4, 1, None, 6) == -1 and "null" in lib.mdf_last_error().decode()
    assert call(ptr(prob), ptr(last), 3, 1, ptr(out), 6) == -1 and "n must be 1, 2, 4 or 8" in lib.mdf_last_error().decode() and "3" in lib.mdf_last_error().decode()
    assert call(ptr(prob), ptr(last), 4, -1, ptr(out), 6) == -1 and "pad_front" in lib.mdf_last_error().decode()
    assert call(ptr(prob), ptr(last), 4, 1, ptr(out), 5) == -1 and "even" in lib.mdf_last_error().decode()      # odd H with last given
    assert call(ptr(prob), None, 4, 1, ptr(out), 5) == 0                                                         # ... fine without
    assert lib.mdf_last_launch().decode() == "confidence_cascade_kernel"
    out.fill_(-7.0)
    ops.confidence(prob)
    for args in ((None, ptr(last), 4, 1, ptr(out), 6), (ptr(prob), ptr(last), 3, 1, ptr(out), 6), (ptr(prob), ptr(last), 4, 1, ptr(out), 5)):
        assert call(*args) == -1
    torch.cuda.synchronize()
    assert lib.mdf_last_launch().decode() == "confidence_kernel" and bool((out == -7.0).all())                  # nothing ran, nothing written
    with pytest.raises(mdfnet_hip.MdfHipError, match="n must be 1, 2, 4 or 8"):
        ops.confidence_cascade(prob, last, n=3)
    with pytest.raises(ValueError, match="last confidence"):
        ops.confidence_cascade(prob, torch.rand(1, 6, 10, device=DEV))
    # ... and the library still works
    assert torch.equal(ops.confidence_cascade(prob), ops.confidence(prob))


# --------------------------------------------------------------------------- the model
def _build(confidence, sd):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        m = config.build_model(confidence=confidence)
    m.load_state_dict(sd)
    return m


def _run_hooked(model, scene):
    probs = {}
    hooks = [model.Regular[s].register_forward_hook(lambda m, i, o, s=s: probs.__setitem__(s, (o[0] if isinstance(o, tuple) else o).detach().clone()))
             for s in range(3)]
    try:
        ops.count_begin()
        with torch.no_grad():
            out = model(*[t.to(DEV) for t in scene])
        counts = ops.count_end()
    finally:
        for h in hooks:
            h.remove()
    return out, [probs[s] for s in range(3)], counts


def test_model_cascade_and_default(golden, seeded_sd):
    """The tiny model of the e2e tests (96x64, 3 views), default and cascade, same weights."""
    w, h, v, b, rot, seed = golden("e2e_tiny.npz")["cfg"]
    scene = synth.make_scene(int(w), int(h), int(v), batch=int(b), rot_deg=float(rot), seed=int(seed))
    default, cascade = _build("last", seeded_sd).eval().to(DEV), _build("cascade", seeded_sd).eval().to(DEV)
    out_d, probs_d, counts_d = _run_hooked(default, scene)
    out_c, probs_c, counts_c = _run_hooked(cascade, scene)
    conf = lambda c: {k: n for k, n in c.items() if "confidence" in k}      # noqa: E731
    assert conf(counts_d) == {"mdf_confidence_up2_fwd": 1}                   # the default model launches what it launched
    assert conf(counts_c) == {"mdf_confidence_cascade_fwd": 3}
    assert {k: n for k, n in counts_d.items() if "confidence" not in k} == {k: n for k, n in counts_c.items() if "confidence" not in k}
    assert all(torch.equal(a, b_) for a, b_ in zip(probs_d, probs_c))
    assert torch.equal(out_d["depth"], out_c["depth"])
    assert out_c["confidence"].shape == out_d["confidence"].shape == out_d["depth"].shape
    assert torch.equal(out_d["confidence"], ops.confidence_up2(probs_d[2]))
    assert_bits(host(out_d["confidence"]), M.confidence_up2(host(probs_d[2])), "default confidence vs mirror")
    want = C.chain([host(p) for p in probs_c], up2_last=True)[2]
    assert_bits(host(out_c["confidence"]), want, "cascade confidence vs the mirror's chain")
    assert not torch.equal(out_c["confidence"], out_d["confidence"])
    print(f"cascade confidence range [{want.min():.4f}, {want.max():.4f}], default [{float(out_d['confidence'].min()):.4f}, {float(out_d['confidence'].max()):.4f}]")


def test_model_train_mode_computes_no_confidence(golden, seeded_sd):
    """model.train(): the output is the four depths, and no confidence entry is called -- the same launches as the default model's."""
    w, h, v, b, rot, seed = golden("e2e_tiny.npz")["cfg"]
    scene = [t.to(DEV) for t in synth.make_scene(int(w), int(h), int(v), batch=int(b), rot_deg=float(rot), seed=int(seed))]
    res = []
    for kind in ("last", "cascade"):
        m = _build(kind, seeded_sd).to(DEV).train()
        ops.count_begin()
        out = m(*scene)
        counts = ops.count_end()
        torch.cuda.synchronize()
        assert sorted(out) == ["depth"] and len(out["depth"]) == 4 and not any("confidence" in k for k in counts)
        res.append(([tuple(d.shape) for d in out["depth"]], counts))
    assert res[0] == res[1]
