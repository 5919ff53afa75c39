"""CPU: the depth-preserving composition of RegularNet_4Scales -- sample_stride (1,2,2), sample_padding (0,1,1), the alternative the
reference names at regular.py:76-77 -- through the constructor, config.build_model, the eval / validate flags and ops' argument check."""
import contextlib
import io

import pytest
import torch

from mdfnet_hip import ops


def _config():
    with contextlib.redirect_stdout(io.StringIO()):
        import config
    return config


def _build(**kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return _config().build_model(**kw)


def test_constructor_accepts_the_two_pairs_and_nothing_else():
    from net.unit.regular import RegularNet_4Scales
    m = RegularNet_4Scales(8, 8, (1, 2, 2), (0, 1, 1))
    assert tuple(m.conv12[0].conv.stride) == (1, 2, 2) and tuple(m.trconv21[0].stride) == (1, 2, 2)
    assert tuple(m.trconv21[0].output_padding) == (0, 1, 1) and tuple(m.trconv21[0].padding) == (1, 1, 1)
    assert tuple(RegularNet_4Scales(8).conv12[0].conv.stride) == (2, 2, 2)
    with pytest.raises(NotImplementedError):
        RegularNet_4Scales(8, 8, (2, 1, 1), (1, 0, 0))
    with pytest.raises(NotImplementedError):
        RegularNet_4Scales(8, 8, (1, 2, 2), (1, 1, 1))


def test_build_model_has_one_parameter_tree_for_both_strides():
    default, hw = _build(), _build(regular_stride=(1, 2, 2))
    sd0, sd1 = default.state_dict(), hw.state_dict()
    assert list(sd0) == list(sd1)
    assert [tuple(v.shape) for v in sd0.values()] == [tuple(v.shape) for v in sd1.values()]
    hw.load_state_dict(sd0, strict=True)
    from net.unit.regular import RegularNet_3Scales
    assert isinstance(hw.Regular[0], RegularNet_3Scales)
    assert [tuple(r.conv12[0].conv.stride) for r in hw.Regular[1:]] == [(1, 2, 2), (1, 2, 2)]
    assert [tuple(r.conv12[0].conv.stride) for r in default.Regular[1:]] == [(2, 2, 2), (2, 2, 2)]
    assert [tuple(r.conv12[0].conv.stride) for r in _config().model.Regular[1:]] == [(2, 2, 2), (2, 2, 2)]      # the singleton stays the default


def test_build_model_rejects_other_strides():
    with pytest.raises(ValueError, match="regular_stride"):
        _build(regular_stride=(3, 2, 2))
    with pytest.raises(ValueError, match="regular_stride"):
        _build(regular_stride=2)


@pytest.mark.parametrize("module", ["eval", "validate"])
def test_parsers_know_the_flag(module):
    import importlib
    with contextlib.redirect_stdout(io.StringIO()):
        parser = importlib.import_module(module).build_parser()
    assert parser.parse_args([]).regular_stride == "2,2,2"
    assert parser.parse_args(["--regular_stride", "1,2,2"]).regular_stride == "1,2,2"
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        parser.parse_args(["--regular_stride", "2,1,1"])
    assert _config().parse_stride("1,2,2") == (1, 2, 2) and _config().parse_stride("2,2,2") == (2, 2, 2)


def test_stock_forward_keeps_every_depth_plane(rehearsal_backend):
    """D = 5: the skip adds of the (2,2,2) composition need D % 8 == 0 (5 -> 3 -> 2 -> 1 comes back as 2, 4, 8).  (CPU tensors: the
    stock-op route of the modules is the rehearsal backend's, taken in eval mode when autograd is wanted of the input.)"""
    from net.unit.regular import RegularNet_4Scales
    torch.manual_seed(3)
    x = torch.randn(1, 8, 5, 16, 24, requires_grad=True)
    m = RegularNet_4Scales(8, 8, (1, 2, 2), (0, 1, 1)).eval()
    prob = m._stock_forward(x).detach()
    assert tuple(prob.shape) == (1, 5, 16, 24)
    assert torch.allclose(prob.sum(1), torch.ones(1, 16, 24), atol=1e-5)
    with pytest.raises(RuntimeError, match="size of tensor"):
        RegularNet_4Scales(8).eval()._stock_forward(x)


def test_conv3d_ndhwc_rejects_other_stride_tuples_before_the_library(monkeypatch):
    import mdfnet_hip

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(mdfnet_hip, "lib", no_lib)
    monkeypatch.setattr(ops, "lib", no_lib, raising=False)
    x = torch.zeros(1, 2, 4, 4, 8)
    with pytest.raises(ValueError, match="stride"):
        ops.conv3d_ndhwc(x, torch.zeros(16), 8, 16, (2, 1, 1))
    with pytest.raises(ValueError, match="stride"):
        ops.conv3d_ndhwc(x, torch.zeros(16), 8, 16, (2, 2, 2))
