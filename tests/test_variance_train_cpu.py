"""CPU: the public surface of the variance-aggregation training path -- C ABI entries declared in the header, the binding and
INTEGRATION.md; config.build_model(aggregate="variance") and the unchanged default; the rehearsal route of the driver for the
variance model; the kernel-family registration of the new kernels."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

from mdfnet_hip import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mdf_warp_aggregate_var_bwd", "mdf_homo_warp_bwd")


def _build(**kw):
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        return config.build_model(**kw)


def test_header_binding_and_integration_notes_declare_the_new_entries():
    from mdfnet_hip import SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdfnet_hip.h")).read(), flags=re.S)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in SIGNATURES and name in notes, name
    # (header == exports == binding over ALL entries is tests/test_abi_cpu.py's; here the argument counts of the two new ones)
    for name in NEW_ENTRIES:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len(decl.split(",")) == len(SIGNATURES[name][1]), name


def test_new_entries_follow_the_error_convention_without_a_gpu():
    import ctypes
    import mdfnet_hip
    l = mdfnet_hip.lib()
    rc = l.mdf_warp_aggregate_var_bwd(None, None, None, None, 0, None, None, None, 1, 16, 1, 4, 4, 1, None)
    assert rc == -1 and b"null" in l.mdf_last_error()
    p = ctypes.c_void_p(8)
    rc = l.mdf_homo_warp_bwd(p, 0, p, p, 0, p, 1, 24, 1, 4, 4, None)
    assert rc == -2 and b"C=24" in l.mdf_last_error()
    rc = l.mdf_homo_warp_bwd(p, 0, p, p, 0, p, 1, 16, 1, 1, 4, None)
    assert rc == -1 and b"bad shape" in l.mdf_last_error()


def test_variance_model_composition():
    from net.unit.homoaggregate import homo_aggregate_by_variance
    m = _build(aggregate="variance")
    assert list(m.Homoaggre) == [homo_aggregate_by_variance] * 3
    sd = m.state_dict()
    assert not any(k.startswith("Homoaggre.") for k in sd)
    # the cost volume has the C feature channels: first regulariser layers 64 -> 16, 32 -> 8, 16 -> 8
    assert tuple(sd["Regular.0.conv01.0.conv.weight"].shape) == (16, 64, 3, 3, 3)
    assert tuple(sd["Regular.1.conv01.conv.weight"].shape) == (8, 32, 3, 3, 3)
    assert tuple(sd["Regular.2.conv01.conv.weight"].shape) == (8, 16, 3, 3, 3)
    # everything else is the default model's
    ref = _build().state_dict()
    for k, v in sd.items():
        if not re.fullmatch(r"Regular\.\d\.conv01(\.0)?\.conv\.weight", k):
            assert tuple(v.shape) == tuple(ref[k].shape), k
    assert set(ref) - set(sd) == {k for k in ref if k.startswith("Homoaggre.")}
    with pytest.raises(ValueError, match="aggregate"):
        _build(aggregate="mean")


def test_default_model_is_unchanged_key_for_key():
    meta = np.load(os.path.join(ROOT, "tests", "golden", "state_dict_meta.npz"))
    want = {str(k): tuple(int(x) for x in s.strip("[]").split(",") if x.strip()) for k, s in zip(meta["keys"], meta["shapes"])}
    for m in (_build(), _build(aggregate="vector")):
        got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert list(got) == [str(k) for k in meta["keys"]]
        assert got == want


def test_variance_model_takes_a_training_step_on_the_rehearsal_backend(rehearsal_backend):
    """The driver's rehearsal route (CPU, stock ops) keeps working for the variance composition: one step, every parameter gets a
    finite gradient and moves."""
    from net.loss import Loss
    m = _build(aggregate="variance")
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=1))
    m.train()
    imgs, extr, intr, dr = synth.make_scene(96, 64, 3, batch=2, rot_deg=3.0, seed=31)
    rng = np.random.RandomState(7)
    gt = {str(s): torch.from_numpy((425 + 510 * rng.rand(2, 64 >> s, 96 >> s)).astype(np.float32)) for s in (3, 2, 1, 0)}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in m.parameters()]
    out = m(imgs, extr, intr, dr)
    assert [tuple(d.shape) for d in out["depth"]] == [(2, 8, 12), (2, 16, 24), (2, 32, 48), (2, 64, 96)]
    loss = Loss()(out, gt, dr)
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    opt.step()
    assert all(not torch.equal(p, q) for p, q in zip(m.parameters(), before))


def test_training_slots_without_a_kernel_are_named():
    """The check CoreNet runs when a GPU training forward starts (exercised on the GPU by tests/test_variance_train_gpu.py)."""
    m = _build(aggregate="variance")
    m._check_training_slots()
    _build()._check_training_slots()

    class Foreign(torch.nn.Module):
        def forward(self, x, *a):
            return x

    m.Homoaggre[2] = Foreign()
    m.Regular[0] = Foreign()
    with pytest.raises(RuntimeError, match=r"Homoaggre\[2\] \(Foreign\), Regular\[0\] \(Foreign\), Depth_regress behind the non-fused Regular\[0\]"):
        m._check_training_slots()


def test_new_kernels_have_a_family():
    from mdfnet_hip import kernel_families as kf
    csrc = os.path.join(ROOT, "mdf-net_amd", "csrc")
    new = {k for k, f in kf.globals_in_sources(csrc).items() if f == "warp_variance_train.hip"}
    assert new == {"warp_var_bwd_kernel"}
    for k in new:
        assert kf.KERNEL_FAMILY[k] == kf.WARP_SCATTER
    assert kf.family("void (anonymous namespace)::warp_var_bwd_kernel<64, true>((anonymous namespace)::VarBwdParams)") == kf.WARP_SCATTER
