"""CPU: ties tests/wgrad_mirror.py down.  `wgrad_ref` (slices and one einsum per tap, no conv backward) equals float64 autograd of
F.conv3d, F.conv_transpose3d and F.conv2d for every layer kind of the tables: bit for bit on the integer inputs, to 1e-12 on randn.
The integer generator keeps every partial sum an fp32 value for every case the GPU tests run (asserted, not assumed)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import wgrad_mirror as M  # noqa: E402

TIE_3D = [(2, 3, 5, 17), (1, 2, 3, 5)]
TIE_2D = [(2, 5, 17), (3, 2, 2)]
TIE_CASES = M._table(M.KINDS_3D, TIE_3D, True) + M._table(M.KINDS_2D, TIE_2D, False)


def autograd_dw(case, small, big):
    """float64 weight gradient of the layer the case stands for, by autograd (the weight's value does not matter: conv is linear in it)."""
    three_d, kind, a, bc, _ = case
    s, k = M.stride_ksize(three_d, kind)
    pad = (k - 1) // 2
    cf = (lambda t: t.double().permute(0, 4, 1, 2, 3)) if three_d else (lambda t: t.double().permute(0, 3, 1, 2))      # channels first
    sm, bg = cf(small), cf(big)
    w = torch.zeros((a, bc) + (k,) * (3 if three_d else 2), dtype=torch.float64, requires_grad=True)
    if kind == "convT_s2":               # small = x [.., Cin = A], big = dy [.., Cout = Bc]; weight [Cin, Cout, 3, 3, 3]
        y = F.conv_transpose3d(sm, w, stride=2, padding=1, output_padding=1)
        assert y.shape == bg.shape
        y.backward(bg)
    else:                                # small = dy [.., Cout = A], big = x [.., Cin = Bc]; weight [Cout, Cin, ..]
        y = (F.conv3d if three_d else F.conv2d)(bg, w, stride=s, padding=pad)
        assert y.shape == sm.shape
        y.backward(sm)
    return w.grad


@pytest.mark.parametrize("case", TIE_CASES, ids=M.case_id)
def test_reference_equals_float64_autograd(case):
    small, big = M.int_inputs(case)
    ref = M.ref_of(case, small, big)
    assert ref.dtype == torch.float64 and tuple(ref.shape[:2]) == (case[2], case[3])
    assert torch.equal(ref, autograd_dw(case, small, big))                   # integers: every sum is exact in float64, in any order
    assert float(ref.abs().max()) <= 9 * M.voxels(case[4])
    small, big = M.randn_inputs(case)
    ref, ag = M.ref_of(case, small, big), autograd_dw(case, small, big)
    assert float((ref - ag).abs().max() / ag.abs().max()) < 1e-12


def test_single_voxel_has_only_the_centre_tap():
    for case in [(True, "conv_s1", 16, 16, (1, 1, 1, 1)), (False, "k5_s2", 16, 8, (1, 1, 1))]:
        small, big = M.int_inputs(case)
        ref = M.ref_of(case, small, big)
        if case[0]:
            assert torch.equal(ref[:, :, 1, 1, 1], torch.outer(small.reshape(-1), big.reshape(-1)).double())
            ref[:, :, 1, 1, 1] = 0
        else:       # k5 s2 pad 2: output pixel 0 reads input pixels -2 .. 2, of which 0 and 1 exist (taps 2 and 3)
            assert torch.equal(ref[:, :, 2:4, 2:4], torch.einsum("a,hwb->abhw", small.reshape(-1).double(), big[0].double()))
            ref[:, :, 2:4, 2:4] = 0
        assert not ref.any()


def test_integer_inputs_keep_every_partial_sum_exact():
    cases = M.all_cases() + M.reduced_cases() + TIE_CASES
    assert len(M.all_cases()) == len(M.cases_3d()) + len(M.cases_2d()) + 5 * len(M.SWEEP_W)
    assert len(M.cases_3d()) == 15 * len(M.SHAPES_3D) and len(M.cases_2d()) == 16 * len(M.SHAPES_2D)
    for case in cases:
        assert 9 * M.voxels(case[4]) < 2 ** 24 and M.exact_for(case[4]), case
    assert M.exact_for((1864135,)) and not M.exact_for((1864136,))           # 9 * 1864135 = 2^24 - 1
    for case in cases[::7]:
        for t in M.int_inputs(case) + M.int_inputs(case, salt=3):
            assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= 3
    a, b = M.int_inputs(cases[40]), M.int_inputs(cases[40], salt=1)
    assert torch.equal(a[0], M.int_inputs(cases[40])[0]) and not torch.equal(a[1], b[1])     # deterministic; salted jobs differ


def test_plan_query_reports_a_recorded_dispatch():
    """mdf_wgrad_last_plan on the host alone: between mdf_wgrad_batch_begin and the flush a dispatch of the LDS form is only recorded
    (nothing is launched), and the query returns what it decided."""
    from mdfnet_hip import lib
    L = lib()
    assert L.mdf_wgrad_last_plan(None, 9) == -1 and b"null" in L.mdf_last_error()
    fake = ctypes.c_void_p(256)                    # never dereferenced on the host
    ns = ctypes.c_int(0)
    out = (ctypes.c_int * 9)(*([-7] * 9))
    assert L.mdf_wgrad_batch_begin() == 0
    try:
        assert L.mdf_conv2d_wgrad_partial(fake, fake, fake, fake, 2, 5, 17, 32, 8, 3, 1, ctypes.byref(ns), None) == 0
        assert L.mdf_wgrad_last_plan(out, 9) == 9
    finally:
        L.mdf_wgrad_batch_begin()                  # drops the recorded job ...
        L.mdf_wgrad_batch_flush(None)              # ... and ends the recording: nothing to launch
    form, r, th, tv, n_tiles, gx, gy, gz, split = list(out)
    assert (form, r, th, gz, split, gy) == (0, 1, 1, 3, 2, 1)          # LDS form, `big` shifts packed (Bc = 8), kh in z, 2 pairs
    assert tv % 16 == 0 and 16 <= tv <= 512 and n_tiles == 2 * 5 * ((17 + tv - 1) // tv) and 1 <= gx <= n_tiles and gx == ns.value
    short = (ctypes.c_int * 9)(*([-7] * 9))
    assert L.mdf_wgrad_last_plan(short, 2) == 9 and list(short) == [0, 1] + [-7] * 7
