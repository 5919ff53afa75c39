"""GPU parity of the 5x5 stride-2 layers of the feature pyramid in their Winograd form over the four parity images (wino2d.hip, S2D):
the steps whose transform-domain weights are structurally zero are skipped at compile time (bit-identical to not skipping them,
MDF_WINO2D_SKIP=0), and 32 -> 64 runs there too, its 128 logical channels in two passes (against torch on the CPU and against the direct
25-tap kernel, MDF_CONV_K5_WINOGRAD_64=0).  A tile is TH x 32 outputs, TH = 8 for 8 -> 16 and 4 for the other two."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mdfnet_hip import lib, ops

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"

CHANS = [(8, 16), (16, 32), (32, 64)]
# (b, h, w) of the input, all even (the parity route), and MDF_WINO2D_GRID
CASES = [
    pytest.param((3, 2, 2), None, id="smaller-than-a-tile"),
    pytest.param((1, 8, 64), None, id="one-tile-row"),
    pytest.param((2, 26, 140), None, id="ragged-3-columns-2-images"),       # 13 x 70 outputs
    pytest.param((2, 26, 140), "1", id="ragged-one-block-walks-all-tiles"),  # >= 12 tiles in one block: LDS slots and fragment ring wrap
]


@functools.lru_cache(maxsize=None)
def _layer(cin, cout, shape):
    """Inputs, weights, folded-BN epilogue and the torch-CPU results of one layer (computed once, shared, never modified)."""
    b, h, w = shape
    rng = np.random.RandomState(cin * 7 + cout * 3 + 5 + h)
    x = T(rng.randn(b, cin, h, w).astype(np.float32))
    wt = T((rng.randn(cout, cin, 5, 5) / np.sqrt(25 * cin)).astype(np.float32))
    alpha = T(rng.uniform(0.5, 1.5, cout).astype(np.float32))
    beta = T(rng.uniform(-0.2, 0.2, cout).astype(np.float32))
    raw = F.conv2d(x, wt, None, 2, 2)
    epi = F.relu(raw * alpha.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1))
    return dict(x=ops.to_nhwc(x.to(DEV)), wp=ops.pack_conv2d_weight(wt.to(DEV)), alpha=alpha.to(DEV), beta=beta.to(DEV), raw=raw, epi=epi)


def _run(L, cin, cout, epilogue):
    if epilogue:
        y = ops.conv2d_nhwc(L["x"], L["wp"], cin, cout, 5, 2, L["alpha"], L["beta"], True)
    else:
        y = ops.conv2d_nhwc(L["x"], L["wp"], cin, cout, 5, 2)
    return y, lib().mdf_last_launch().decode()


def _env(monkeypatch, grid, **kw):
    for k in ("MDF_WINO2D_SKIP", "MDF_CONV_K5_WINOGRAD_64", "MDF_CONV_K5_WINOGRAD", "MDF_CONV_WINO2D", "MDF_CONV_WINOGRAD", "MDF_WINO2D_GRID"):
        monkeypatch.delenv(k, raising=False)
    if grid is not None:
        monkeypatch.setenv("MDF_WINO2D_GRID", grid)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("chans", CHANS)
@pytest.mark.parametrize("shape,grid", CASES)
def test_skipping_the_zero_steps_is_bit_identical(chans, shape, grid, monkeypatch):
    """A skipped MFMA adds +0 products to an accumulator that started from +0: skip == no skip, bit for bit, with and without the epilogue.
    (8 -> 16 keeps every step in both settings -- its skipping was measured and dropped -- and stays here as a case of the route.)"""
    cin, cout = chans
    L = _layer(cin, cout, shape)
    for epilogue in (True, False):
        _env(monkeypatch, grid)
        got, launch = _run(L, cin, cout, epilogue)
        assert launch.startswith("wino2d_kernel"), launch
        _env(monkeypatch, grid, MDF_WINO2D_SKIP="0")
        full, launch = _run(L, cin, cout, epilogue)
        assert launch.startswith("wino2d_kernel"), launch
        assert not torch.isnan(got).any()
        assert torch.equal(got, full), (epilogue, float((got - full).abs().max()))


@pytest.mark.parametrize("shape,grid", CASES)
def test_k5s2_32_to_64_in_two_passes(shape, grid, monkeypatch):
    """32 -> 64 over the parity images (two passes of 64 logical channels, accumulators live across both) against torch on the CPU and against
    the direct 25-tap kernel, at the bar of test_conv2d_layer."""
    L = _layer(32, 64, shape)
    for epilogue in (True, False):
        exp = (L["epi"] if epilogue else L["raw"]).numpy()
        _env(monkeypatch, grid)
        got, launch = _run(L, 32, 64, epilogue)
        assert launch.startswith("wino2d_kernel"), launch
        _env(monkeypatch, grid, MDF_CONV_K5_WINOGRAD_64="0")
        direct, launch = _run(L, 32, 64, epilogue)
        assert launch.startswith("conv_lds_kernel"), launch
        got, direct = ops.from_nhwc(got).cpu().numpy(), ops.from_nhwc(direct).cpu().numpy()
        assert got.shape == exp.shape
        print(f"\n32->64 {shape} grid={grid} epilogue={epilogue}: max|d| vs torch {np.abs(got - exp).max():.3e}, vs direct {np.abs(got - direct).max():.3e}")
        np.testing.assert_allclose(got, exp, rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(got, direct, rtol=1e-4, atol=2e-5)


def test_k5s2_32_to_64_odd_sized_input_stays_on_the_direct_kernel(monkeypatch):
    _env(monkeypatch, None)
    L = _layer(32, 64, (1, 9, 21))
    got, launch = _run(L, 32, 64, True)
    assert launch.startswith("conv_lds_kernel"), launch
    np.testing.assert_allclose(ops.from_nhwc(got).cpu().numpy(), L["epi"].numpy(), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("chans", CHANS)
def test_the_zero_fragments_are_where_the_kernel_assumes(chans):
    """The packed transform-domain weights of the parity form: fragment (chunk, ab, nt) holds [lane = q*16 + m][s] = U[a][b] of
    (cout = nt*16 + m, logical cin = chunk*16 + 4q + s), parity (py*2 + px) = logical cin / Cin.  Everything of a py == 1 parity with
    a == 3 and of a px == 1 parity with b == 3 is exactly 0.0, and nothing else is all zero (guards G and the tap placement)."""
    cin, cout = chans
    rng = np.random.RandomState(cin + cout)
    wt = T((rng.randn(cout, cin, 5, 5) / np.sqrt(25 * cin)).astype(np.float32))
    wp = ops.pack_conv2d_weight(wt.to(DEV)).cpu().numpy()
    kpl = 4 if cin >= 16 else 2
    nch_plain, nt = cin // (4 * kpl), cout // 16
    plain = 25 * nch_plain * nt * 64 * kpl                   # the 25 plain taps come first (the dispatch's offset)
    nch = 4 * cin // 16
    assert wp.size == plain + nch * 16 * nt * 256
    seg = wp[plain:].reshape(nch, 16, nt, 4, 16, 4)          # [chunk][ab][nt][q][m][s]
    n_zero = 0
    for ch in range(nch):
        par = (ch * 16 + 4 * np.arange(4)[:, None] + np.arange(4)[None, :]) // cin        # [q][s]
        for ab in range(16):
            a, b = ab >> 2, ab & 3
            for p in np.unique(par):
                py, px = p >> 1, p & 1
                sel = np.broadcast_to((par == p)[None, :, None, :], (nt, 4, 16, 4))
                vals = seg[ch, ab][sel]
                if (py == 1 and a == 3) or (px == 1 and b == 3):
                    assert np.all(vals == 0.0) and not np.any(np.signbit(vals)), (ch, ab, p)
                    n_zero += 1
                else:
                    assert np.any(vals != 0.0), (ch, ab, p)
    assert n_zero == 15 * max(1, cin // 16)        # 0 + 4 + 4 + 7 dead (ab) per parity, in every chunk of the parity: 49 of 64 live
