"""wino3d.hip covers a last tile column of 1..8 live columns (W % 32 in 1..8) with strip tiles of 32 rows x 8 columns instead of
8 x 32 ones (MDF_W3_STRIP, default 1).  Only which lane holds which 2x2 Winograd tile changes: every output is bit-identical to
the same call with MDF_W3_STRIP=0 / MDF_W3_WL=0 (the tiling before), with and without the epilogue's residual, for NaNs too."""
import numpy as np
import pytest
import torch

from mdfnet_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# W: 40 = a full tile column + an 8-wide strip, 33 = strip with one live column, 8 = strip only, 64 = no strip, 48 = remainder 16
# H: 36 = a full 32-row strip + a 4-row one (4.5 ordinary tiles), 8, 2;  D: 1, 3, 5 (kd masks at both ends, stream-K cuts inside a tile)
SHAPES = [(1, 1, 36, 40), (1, 3, 8, 40), (2, 5, 2, 40), (2, 3, 36, 33), (1, 5, 8, 33), (1, 1, 2, 33),
          (1, 5, 36, 8), (2, 1, 8, 8), (1, 3, 2, 8), (1, 3, 36, 64), (2, 1, 8, 64), (1, 5, 36, 48), (2, 3, 2, 48),
          (2, 5, 36, 40),       # 70 steps on 17 blocks: block 12 owns steps 49..52, the ordinary tiles end at step 50
          (1, 7, 36, 40),       # 49 steps on 12 blocks: block 8 owns steps 32..35, the ordinary tiles end at step 35
          (1, 24, 36, 72)]      # 10 ordinary tiles + 2 strips x 24 planes on 72 blocks: several blocks per tile, of either kind


def _layer(cin, cout, shape, seed):
    b, d, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, d, h, w, cin, generator=g).to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) / np.sqrt(27 * cin)).to(DEV)
    alpha, beta = (torch.rand(cout, generator=g) + 0.5).to(DEV), (torch.rand(cout, generator=g) * 0.4 - 0.2).to(DEV)
    res = torch.randn(b, d, h, w, cout, generator=g).to(DEV)
    return x, ops.pack_conv3d_weight(wt, False), alpha, beta, res


def _run(x, wp, cin, cout, alpha, beta, res, relu=True):
    """The layer with BN (+ ReLU), with and without the residual; each call must be one wino3d_kernel launch."""
    out = []
    for r in (res, None):
        ops.count_begin()
        out.append(ops.conv3d_ndhwc(x, wp, cin, cout, 1, False, alpha, beta, relu, r))
        counts = ops.count_end()
        assert sum(counts.values()) == 1, counts
        assert lib().mdf_last_launch().decode().startswith("wino3d_kernel")
    return out


def _both(monkeypatch, *args):
    monkeypatch.setenv("MDF_CONV_LDS_MIN_VOXELS", "0")     # small volumes take the LDS kernels too
    monkeypatch.delenv("MDF_W3_STRIP", raising=False)
    monkeypatch.delenv("MDF_W3_WL", raising=False)
    new = _run(*args)
    monkeypatch.setenv("MDF_W3_STRIP", "0")
    monkeypatch.setenv("MDF_W3_WL", "0")
    old = _run(*args)
    return new, old


@pytest.mark.parametrize("cin,cout", [(32, 16), (16, 16)])
@pytest.mark.parametrize("shape", SHAPES)
def test_strip_tiles_equal_the_ordinary_tiling(cin, cout, shape, monkeypatch):
    x, wp, alpha, beta, res = _layer(cin, cout, shape, cin * 7 + sum(shape))
    new, old = _both(monkeypatch, x, wp, cin, cout, alpha, beta, res)
    for n, o in zip(new, old):
        assert torch.equal(n, o)
        assert not torch.isnan(n).any()


@pytest.mark.parametrize("cin,cout", [(32, 16), (16, 16)])
def test_nan_reaches_the_same_voxels(cin, cout, monkeypatch):
    """NaNs in the strip column, at the volume's corner and in an ordinary tile next to the strip: NaN in exactly the voxels
    that the ordinary tiling gives, nowhere else (a strip tile's halo beyond the volume holds zeros).  The epilogue's ReLU is
    fmaxf(v, 0), which turns a NaN into 0, so the layer also runs without it: there the NaNs must reach the output."""
    shape = (1, 3, 36, 40)
    x, wp, alpha, beta, res = _layer(cin, cout, shape, 99 + cin)
    x[0, 1, 33, 39, 3] = float("nan")
    x[0, 0, 0, 32, 0] = float("nan")
    x[0, 2, 35, 30, cin - 1] = float("nan")
    for relu in (True, False):
        new, old = _both(monkeypatch, x, wp, cin, cout, alpha, beta, res, relu)
        for n, o in zip(new, old):
            assert torch.equal(torch.isnan(n), torch.isnan(o))
            assert relu or (torch.isnan(n).any() and not torch.isnan(n).all())
            assert torch.equal(torch.nan_to_num(n, nan=0.0), torch.nan_to_num(o, nan=0.0))
