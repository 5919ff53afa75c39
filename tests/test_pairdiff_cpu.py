"""CPU: the feature pyramid's pair-difference heads (net/unit/backbone.py:_composed_fp64).  The aggregation with C/G = 2 reads a
feature pair (a, b) only through b - a, so a composed head may emit f[2g+1] - f[2g] directly: its matrix and bias are rows 2g+1
minus rows 2g of the full composed head, formed in fp64 before the one rounding to fp32."""
import torch

from net.unit.backbone import FPN_4Scales, pair_difference_rows

NAMES = ("y4", "a4", "c4", "y3", "c3", "y2")


def _fpn(seed=0):
    torch.manual_seed(seed)
    m = FPN_4Scales()
    with torch.no_grad():
        for mod in (m.out2, m.out3, m.out4, m.lat2, m.lat3):
            mod.weight.normal_(0.0, 0.3)
            if mod.bias is not None:
                mod.bias.normal_(0.0, 0.5)
    return m


def test_difference_heads_are_row_differences_of_the_composed_heads_in_fp64():
    m = _fpn()
    full, diff = m._composed_fp64(False), m._composed_fp64(True)
    assert sorted(full) == sorted(diff) == sorted(NAMES)
    for k in NAMES:
        w, b = full[k]
        dw, db = diff[k]
        assert w.dtype == dw.dtype == torch.float64
        g = w.shape[0] // 2
        assert dw.shape == (g, w.shape[1])
        for i in range(g):
            assert torch.equal(dw[i], w[2 * i + 1] - w[2 * i]), (k, i)
        assert (b is None) == (db is None)
        if b is not None:
            assert db.dtype == torch.float64 and db.shape == (g,)
            for i in range(g):
                assert db[i] == b[2 * i + 1] - b[2 * i], (k, i)


def test_difference_head_channel_counts():
    diff = _fpn(1)._composed_fp64(True)
    # (outputs, inputs): y4, a4, c4 read t4 (64 channels); y3, c3 read t3 (32); y2 reads t2 (16)
    assert {k: tuple(diff[k][0].shape) for k in NAMES} == {"y4": (32, 64), "a4": (16, 64), "c4": (8, 64), "y3": (16, 32), "c3": (8, 32),
                                                           "y2": (8, 16)}
    assert [diff[k][1] is None for k in NAMES] == [True, True, True, False, False, False]


def test_composing_the_differenced_output_rows_gives_the_same_heads():
    """Differencing the rows of out3 / out2 BEFORE composing with the lateral convs is the same matrix up to fp64 rounding."""
    m = _fpn(2)
    diff = m._composed_fp64(True)

    def mat(c):
        return c.weight.detach().double().reshape(c.out_channels, c.in_channels)
    o2d, o3d = pair_difference_rows(mat(m.out2)), pair_difference_rows(mat(m.out3))
    l2, l3 = mat(m.lat2), mat(m.lat3)
    b2, b3 = m.lat2.bias.detach().double(), m.lat3.bias.detach().double()
    for k, (w, b) in {"y3": (o3d @ l3, o3d @ b3), "c3": (o2d @ l3, o2d @ b3), "y2": (o2d @ l2, o2d @ b2)}.items():
        assert (diff[k][0] - w).abs().max() <= 1e-14 and (diff[k][1] - b).abs().max() <= 1e-14, k


def test_difference_pyramid_is_the_differenced_pyramid_in_fp64():
    """The whole head chain (1x1 heads + bilinear x2 upsample-adds, fpn_4scales' last seven lines) is linear: evaluated in fp64 with
    the difference heads it gives f[:, 1::2] - f[:, 0::2] of the full chain."""
    import torch.nn.functional as F
    m = _fpn(3)
    torch.manual_seed(4)
    t2, t3, t4 = torch.randn(1, 16, 16, 24).double(), torch.randn(1, 32, 8, 12).double(), torch.randn(1, 64, 4, 6).double()

    def chain(hd):
        def conv(t, k):
            w, b = hd[k]
            return F.conv2d(t, w.reshape(*w.shape, 1, 1), b)

        def up(t):
            return F.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=False)
        y4 = conv(t4, "y4")
        y3 = up(conv(t4, "a4")) + conv(t3, "y3")
        c3 = up(conv(t4, "c4")) + conv(t3, "c3")
        y2 = up(c3) + conv(t2, "y2")
        return y4, y3, y2
    for f, d in zip(chain(m._composed_fp64(False)), chain(m._composed_fp64(True))):
        assert d.shape[1] * 2 == f.shape[1]
        assert (d - (f[:, 1::2] - f[:, 0::2])).abs().max() <= 1e-12
