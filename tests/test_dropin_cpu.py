"""CPU: the product's `net` package is a drop-in for the reference's (same state_dict contract), and a reference-layout
config.py composes its model out of OUR slots when mdfnet_hip.dropin is installed in front of it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_matches_reference_contract(golden, seeded_sd):
    from modelutil import build_model
    meta = golden("state_dict_meta.npz")
    m = build_model()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in meta["keys"]]            # same keys, same order
    assert [str(list(v.shape)) for v in sd.values()] == [str(s) for s in meta["shapes"]]
    assert sum(p.numel() for p in m.parameters()) == int(meta["nparams"]) == 1206380
    m.load_state_dict(seeded_sd)                                         # strict, as eval.py:17 / train.py:21
    assert not any(k.startswith("Depth_hypos") for k in sd)              # H8: prob_thresh is not a buffer
    assert sd["Backbone.conv01.0.bn.num_batches_tracked"].dtype == torch.int64


def test_slot_signatures_and_mode_dispatch(rehearsal_backend):
    from modelutil import build_model
    from net.unit import regress, scale
    m = build_model()
    assert callable(m.scale) and m.scale is scale.scale_cam
    assert m.Depth_regress is regress.depth_regression and m.Confidence_regress is regress.confidence_regress
    k = torch.eye(3).reshape(1, 1, 3, 3).repeat(1, 3, 1, 1) * 100
    e = torch.eye(4).reshape(1, 1, 4, 4).repeat(1, 3, 1, 1)
    k0 = k.clone()
    rp, sps = m.scale(k, e, 0)
    assert rp.shape == (1, 4, 4) and len(sps) == 2 and torch.equal(k, k0)   # inputs untouched (scale.py:14)
    hyp = m.Depth_hypos[0](None, torch.tensor([[425.0, 935.0]], dtype=torch.float64), None, None, upsample=True)
    assert hyp.shape == (1, 48, 1, 1) and float(hyp[0, 0]) == 425.0 and float(hyp[0, -1]) == 935.0
    m.train()   # training mode on CPU tensors = the rehearsal backend (selected by the fixture)
    cost = m.Homoaggre[0]([torch.randn(1, 64, 4, 4, requires_grad=True) for _ in range(2)], rp, sps[:1], hyp)
    assert cost.shape == (1, 32, 48, 4, 4) and cost.requires_grad
    m.eval()    # inference = hand-written kernels only: CPU tensors are refused
    with pytest.raises(RuntimeError, match="no CPU route"):
        m.Homoaggre[0]([torch.zeros(1, 64, 4, 4)] * 2, rp, sps[:1], hyp)


# A reference-layout tree: a `config.py` that composes the model out of the `net` slots the way the reference's config.py:186-218
# does (the public constructor contract: FPN_4Scales(chs), HyposByFit(ndepths, curve, prob_thresh), VectorAggregate(ngroups), the
# 3-scale / 4-scale regularisers, the two regression functions, RefineNet2), next to a `net/` package of its own that must never be
# imported -- in the reference tree it is the CUDA-era package the drop-in replaces.
STAND_IN_CONFIG = """\
import torch.nn as nn
from net import core
from net.unit import scale, backbone, regress, refine
from net.unit.depthhypos import HyposByFit
from net.unit.homoaggregate import VectorAggregate
from net.unit.regular import RegularNet_4Scales, RegularNet_3Scales
hypos = nn.ModuleList([HyposByFit(n, c, t) for n, c, t in zip((48, 24, 8), (None, "gauss1", "laplace"), (0.0, 0.95, 1e-5))])
aggregate = nn.ModuleList([VectorAggregate(g) for g in (32, 16, 8)])
regular = nn.ModuleList([RegularNet_3Scales(32), RegularNet_4Scales(16), RegularNet_4Scales(8)])
model = core.CoreNet(backbone.FPN_4Scales((8, 16, 32, 64)), hypos, scale.scale_cam, aggregate, regular,
                     [regress.depth_regression, regress.confidence_regress], refine.RefineNet2())
"""


def test_reference_config_builds_on_our_slots(tmp_path):
    ref = tmp_path / "reference"
    (ref / "net" / "unit").mkdir(parents=True)
    (ref / "config.py").write_text(STAND_IN_CONFIG)
    for f in ("net/__init__.py", "net/core.py", "net/unit/__init__.py"):
        (ref / f).write_text("raise ImportError('the reference tree\\'s own net package was imported')\n")
    code = (
        "import sys, io, contextlib; sys.path.insert(0, %r)\n"
        "from mdfnet_hip import dropin; dropin.install(%r)\n"
        "import os; os.chdir(%r)\n"
        "with contextlib.redirect_stdout(io.StringIO()):\n"
        "    import config\n"
        "import net.core, net.unit.regular\n"
        "assert config.__file__.startswith(%r), config.__file__\n"
        "assert net.core.__file__.startswith(%r), net.core.__file__\n"
        "m = config.model\n"
        "assert type(m).__module__ == 'net.core' and type(m.Regular[0]).__module__ == 'net.unit.regular'\n"
        "from mdfnet_hip import ops  # our slots are HIP-backed\n"
        "print(len(m.state_dict()), sum(p.numel() for p in m.parameters()))\n"
    ) % (os.path.join(ROOT, "mdf-net_amd"), str(ref), str(tmp_path), str(ref), os.path.join(ROOT, "mdf-net_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "290 1206380"
