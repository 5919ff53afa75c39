"""CPU: the validation metrics' definitions (tests/depth_metrics_oracle.py) against an independent formulation, the report
arithmetic on a hand-worked example, the accumulator over two gloo ranks, the drivers' arguments and the loaders' validation lists.
(The eval-mode forward has no CPU route -- CoreNet refuses CPU tensors in eval mode and the rehearsal backend covers training only --
so `train.py --val_every` end to end is a GPU test: tests/test_depth_metrics_gpu.py.)"""
import ctypes
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_metrics_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mdf-net_amd")


def _load(name):
    spec = importlib.util.spec_from_file_location("mdf_" + name, os.path.join(PKG, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _seeded_maps(seed, b=2, h=9, w=13, d=5):
    rng = np.random.RandomState(seed)
    gt = (500 + 300 * rng.rand(b, h, w)).astype(np.float32)
    gt[rng.rand(b, h, w) < 0.2] = 0.0
    est = (gt + rng.randn(b, h, w) * 6).astype(np.float32)
    est[0, 0, 1] = np.nan
    est[1, 2, 3] = np.inf
    conf = (rng.rand(b, h, w) * 1.2 - 0.1).astype(np.float32)
    conf[0, 1, 1] = np.nan
    conf[0, 1, 2] = 1.0
    hyp = np.sort((gt[:, None] + rng.randn(b, d, h, w) * 8).astype(np.float32), axis=1)
    flat = np.stack([np.linspace(425, 935, d)] * b).astype(np.float32).reshape(b, d, 1, 1)
    return [{"est": est, "gt": gt, "hypos": hyp}, {"est": est, "gt": gt, "hypos": flat}, {"est": est, "gt": gt, "conf": conf}]


def _independent(maps, floor, thr):
    """The same tables from torch boolean masks and a Python loop over bins (float64 torch sums: compared to a relative 1e-12)."""
    fl = torch.as_tensor(np.asarray(floor)).double()
    thr = torch.as_tensor(thr)
    out = torch.zeros(len(maps), 33, 9, dtype=torch.float64)
    for m, mp in enumerate(maps):
        est, gt = torch.as_tensor(mp["est"]), torch.as_tensor(mp["gt"])
        b = est.shape[0]
        valid = gt.double() > fl.reshape(b, 1, 1)
        fin = torch.isfinite(est)
        if "hypos" in mp:
            hy = torch.as_tensor(mp["hypos"])
            lo, hi = hy[:, 0].expand_as(est), hy[:, -1].expand_as(est)
            fin = fin & torch.isfinite(lo) & torch.isfinite(hi)
        if "conf" in mp:
            cf = torch.as_tensor(mp["conf"])
            fin = fin & torch.isfinite(cf)
        ok = valid & fin
        e = (est - gt).abs()
        rows = [ok]
        if "conf" in mp:
            k = torch.clamp(torch.floor(torch.nan_to_num(cf) * 32.0), 0, 31)
            rows += [ok & (k == i) for i in range(32)]
        for r, sel in enumerate(rows):
            out[m, r, 0] = sel.sum()
            out[m, r, 2] = e[sel].double().sum()
            for t in range(thr.shape[1]):
                out[m, r, 3 + t] = (sel & (e < thr[:, t].reshape(b, 1, 1))).sum()
        out[m, 0, 1] = (valid & ~fin).sum()
        if "hypos" in mp:
            out[m, 0, 7] = (ok & (lo <= gt) & (gt <= hi)).sum()
            out[m, 0, 8] = (hi - lo)[ok].double().sum()
    return out.numpy()


@pytest.mark.parametrize("floor_dtype", [np.float64, np.float32])
def test_mirror_against_independent_formulation(floor_dtype):
    maps = _seeded_maps(3)
    floor = np.array([425.0, 600.0], dtype=floor_dtype)
    thr = np.array([[2, 4, 8], [1.5, 3, 20]], np.float32)
    ref = O.metrics(maps, floor, thr)
    ind = _independent(maps, floor, thr)
    for c in O.COUNT_COLS:
        np.testing.assert_array_equal(ref["table"][..., c], ind[..., c])
    np.testing.assert_allclose(ref["table"][..., O.SUM_E], ind[..., O.SUM_E], rtol=1e-12)
    np.testing.assert_allclose(ref["table"][..., O.SUM_WIDTH], ind[..., O.SUM_WIDTH], rtol=1e-12)
    t = ref["table"]
    assert t[2, 0, O.NONFINITE] >= 1 and t[0, 0, O.N] > 50 and t[2, 1:, O.N].sum() == t[2, 0, O.N]
    assert t[0, 1:].sum() == 0 and t[2, 0, O.COVERED] == 0          # no conf -> no bin rows; no hypos -> no interval columns
    O.check_against(ref["table"], ref)


def test_mirror_edge_values():
    """gt == floor is invalid; e == threshold is not under; gt == lo and gt == hi are covered; confidences of exactly 1, above 1 and
    below 0 land in the end bins."""
    gt = np.array([[[425.0, 500.0, 500.0, 600.0, 700.0, 0.0]]], np.float32)
    est = np.array([[[430.0, 502.0, 501.0, 600.0, 700.0, 1.0]]], np.float32)
    hyp = np.array([500.0, 550.0, 600.0], np.float32).reshape(1, 3, 1, 1)
    conf = np.array([[[0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.3, -0.01, 0.5]]], np.float32)
    ref = O.metrics([{"est": est, "gt": gt, "hypos": hyp, "conf": conf}], np.array([425.0]), np.array([[2.0]], np.float32))["table"][0]
    assert ref[0, O.N] == 4 and ref[0, O.SUM_E] == 3.0 and ref[0, O.UNDER] == 3          # e = 2, 1, 0, 0: 2 is not under 2
    assert ref[0, O.COVERED] == 3 and ref[0, O.SUM_WIDTH] == 400.0                       # 500 (== lo), 500, 600 (== hi); 700 is outside
    assert ref[1 + 31, O.N] == 3 and ref[1 + 0, O.N] == 1 and ref[1:, O.N].sum() == 4


def _six_pixel_table():
    gt = np.array([[[500, 500, 500, 500, 500, 0]]], np.float32)
    est = gt + np.array([[[1, 3, 5, 1, 10, 0]]], np.float32)
    conf = np.array([[[0.99, 0.97, 0.5, 0.51, 0.0, 0.9]]], np.float32)
    hyp = np.array([400.0, 500.0, 600.0], np.float32).reshape(1, 3, 1, 1)
    stage = {"est": est, "gt": gt, "hypos": hyp}
    return O.metrics([stage, stage, stage, {"est": est, "gt": gt, "conf": conf}], np.array([425.0]), np.array([[2.0, 4.0]], np.float32))["table"]


def test_report_on_hand_worked_example():
    from mdfnet_hip import valmetrics
    rep = valmetrics.make_report(_six_pixel_table(), (2.0, 4.0), items=1)
    fin = rep["maps"]["final"]
    assert fin["n"] == 5 and fin["n_nonfinite"] == 0 and fin["mean_abs_err"] == 4.0 and fin["under"] == [0.4, 0.6]
    assert "coverage" not in fin
    s0 = rep["maps"]["stage0"]
    assert s0["coverage"] == 1.0 and s0["mean_width"] == 200.0 and s0["mean_abs_err"] == 4.0
    rows = rep["confidence"]
    assert [r["conf_ge"] for r in rows] == [k / 32 for k in range(31, -1, -1)]
    top = rows[0]                                        # conf >= 31/32: the pixels with e = 1 and 3
    assert top["share"] == 0.4 and top["mean_abs_err"] == 2.0 and top["under"] == [0.5, 1.0]
    assert rows[14] == dict(top, conf_ge=17 / 32)        # nothing between 17/32 and 31/32
    mid = rows[15]                                       # conf >= 16/32: + the pixels with e = 5 and 1
    assert mid["conf_ge"] == 0.5 and mid["share"] == 0.8 and mid["mean_abs_err"] == 2.5 and mid["under"] == [0.5, 0.75]
    low = rows[31]                                       # conf >= 0: everything
    assert low["share"] == 1.0 and low["mean_abs_err"] == 4.0 and low["under"] == [0.4, 0.6]
    text = valmetrics.format_report(rep)
    assert "stage0" in text and "final map by confidence" in text and "world size" in text
    assert json.loads(valmetrics.report_json(rep))["maps"]["final"]["n"] == 5


def test_report_of_no_valid_pixel():
    from mdfnet_hip import valmetrics
    rep = valmetrics.make_report(np.zeros((4, 33, 9)), (2.0, 4.0, 8.0))
    for e in rep["maps"].values():
        assert e["n"] == 0 and math.isnan(e["mean_abs_err"]) and all(math.isnan(u) for u in e["under"])
    assert math.isnan(rep["maps"]["stage1"]["coverage"]) and all(math.isnan(r["share"]) for r in rep["confidence"])
    line = [ln for ln in valmetrics.format_report(rep).splitlines() if ln.startswith("stage1")][0]
    assert line.split()[1:] == ["0", "0", "-", "-", "-", "-", "-", "-"]
    assert json.loads(valmetrics.report_json(rep))["maps"]["final"]["mean_abs_err"] is None          # NaN -> null


WORKER = r'''
import sys, json
sys.path[:0] = [%(pkg)r]
import torch
from mdfnet_hip import shard, valmetrics
rank, world, local = shard.init("gloo")
acc = valmetrics.Accumulator("cpu")
for item in shard.shard_items(5, rank, world):
    t = torch.zeros(4, 33, 9, dtype=torch.float64)
    t[:, :, 0] = item + 1
    t[:, :, 2] = 0.1 * (item + 1)
    acc.add(t)
table, items = acc.reduce()
one = shard.sum_tensor_over_ranks(torch.tensor([1.5, 2.0]))
if rank == 0:
    print(json.dumps({"items": items, "n": table[3, 0, 0].item(), "sum_e": table[0, 32, 2].item(), "one": one.tolist(), "dtype": str(one.dtype)}))
'''


def test_accumulator_over_two_gloo_ranks(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"pkg": PKG})
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29677", str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["items"] == 5 and rec["n"] == 15.0 and abs(rec["sum_e"] - 1.5) < 1e-12
    assert rec["one"] == [3.0, 4.0] and rec["dtype"] == "torch.float64"
    # a single process: the tensor itself, as float64
    from mdfnet_hip import shard, valmetrics
    assert shard.sum_tensor_over_ranks(torch.tensor([1.0, 2.0])).tolist() == [1.0, 2.0]
    acc = valmetrics.Accumulator("cpu")
    assert acc.reduce()[1] == 0


def test_driver_arguments():
    val, train = _load("validate"), _load("train")
    a = val.build_parser().parse_args([])
    assert (a.dataset, a.aggregate, a.curves, a.prob_thresh, a.confidence, a.thresholds, a.relative, a.out, a.pre_model) == \
        ("dtu", "vector", "gauss1,laplace", "0.95,1e-5", "last", None, False, None, None)
    a = val.build_parser().parse_args("-p x.pth -d blendedmvs --confidence cascade --curves gauss0,laplace --thresholds 1,2.5 --relative --out r.json".split())
    assert (a.pre_model, a.dataset, a.confidence, a.out) == ("x.pth", "blendedmvs", "cascade", "r.json")
    assert val.parse_thresholds(None, "dtu", False) == ((2.0, 4.0, 8.0), False)
    assert val.parse_thresholds(None, "blendedmvs", False) == ((1 / 256, 1 / 128, 1 / 64), True)
    assert val.parse_thresholds("1,2.5", "dtu", True) == ((1.0, 2.5), True)
    assert val.parse_thresholds("1/512", "dtu", False) == ((1 / 512,), False)
    with pytest.raises(ValueError):
        val.parse_thresholds("1,2,3,4,5", "dtu", False)
    t = train.build_parser().parse_args([])
    assert t.val_every == 0 and (t.dataset, t.aggregate, t.curves, t.prob_thresh) == ("dtu", "vector", "gauss1,laplace", "0.95,1e-5")
    assert train.build_parser().parse_args(["--val_every", "3"]).val_every == 3


def test_val_every_zero_builds_no_dataset(monkeypatch):
    train = _load("train")
    import validate                                     # (what train.make_val_dataset imports)
    calls = []
    monkeypatch.setattr(validate, "val_dataset", lambda name, nviews=5: calls.append(name) or "dataset")
    assert train.make_val_dataset(train.build_parser().parse_args([]), 5) is None and calls == []
    assert train.make_val_dataset(train.build_parser().parse_args(["--val_every", "2", "-d", "blendedmvs"]), 5) == "dataset"
    assert calls == ["blendedmvs"]


def test_item_thresholds():
    from mdfnet_hip import valmetrics
    dr = np.array([[425.0, 935.0], [1.0, 3.0]])
    rel = valmetrics.item_thresholds(dr, valmetrics.RELATIVE_THRESHOLDS, True)
    assert rel.dtype == torch.float32 and rel.shape == (2, 3)
    np.testing.assert_allclose(rel.numpy(), [[510 / 256, 510 / 128, 510 / 64], [2 / 256, 2 / 128, 2 / 64]], rtol=1e-7)
    assert valmetrics.item_thresholds(dr, valmetrics.DTU_THRESHOLDS, False).tolist() == [[2.0, 4.0, 8.0]] * 2


def test_validation_lists(tmp_path):
    import config
    from load import synthetic
    from load.blendedtrain import LoadDataset
    root = synthetic.write_blendedmvs_set(str(tmp_path / "bl"), scans=("scanA", "scanB"), nviews_total=5)
    with open(os.path.join(root, "validation_list.txt"), "w") as f:
        f.write("scanB\n")
    both, val = LoadDataset(root, nviews=3), LoadDataset(root, nviews=3, listfile="validation_list.txt")
    assert both.listfile.endswith("training_list.txt") and {c[0] for c in both.all_compose} == {"scanA", "scanB"}
    assert {c[0] for c in val.all_compose} == {"scanB"} and 2 * len(val) == len(both)
    item = val[0]
    assert set(item["ref_depths"]) == {"3", "2", "1", "0"} and item["depth_range"].shape == (2,)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        dtu = config.LoadDTU()
    assert dtu.val_label == [3, 5, 17, 21, 28, 35, 37, 38, 40, 43, 56, 59, 66, 67, 82, 86, 106, 117] and dtu.val_lighting_label == [3]
    assert not set(dtu.val_label) & set(dtu.train_label) and len(dtu.train_label) == 79


def test_op_refuses_cpu_tensors():
    from mdfnet_hip import ops
    z = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_metrics([{"est": z, "gt": z}], torch.zeros(1, dtype=torch.float64), torch.ones(1, 3))


def test_abi_entries_and_error_convention():
    import mdfnet_hip
    from mdfnet_hip import kernel_families as KF
    names = ("mdf_depth_metrics_workspace", "mdf_depth_metrics_reduce_multi", "mdf_depth_metrics_finalize")
    header = open(os.path.join(ROOT, "include", "mdfnet_hip.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in names:
        assert n in mdfnet_hip.SIGNATURES and n in header and n in notes
    assert KF.family("void (anonymous namespace)::depth_metrics_reduce_multi_kernel<3>((anonymous namespace)::MetricMaps, void const*, int, int, float const*, double*)") == KF.CONTROL
    assert KF.family("depth_metrics_finalize_kernel") == KF.CONTROL
    l = mdfnet_hip.lib()
    table = 33 * 9 * 8
    per = (ctypes.c_int64 * 4)(20 * 16, 40 * 32, 80 * 64, 160 * 128)
    # the grid is sized for the largest map (20 blocks of 2 x 512 pixels); smaller maps use ceil(pixels / 512) blocks of it at most
    assert l.mdf_depth_metrics_workspace(per, 4, 1) == (1 + 3 + 10 + 20) * table
    assert l.mdf_depth_metrics_workspace(per, 4, 3) == 3 * (1 + 3 + 10 + 20) * table
    one = (ctypes.c_int64 * 1)(592 * 800)
    assert l.mdf_depth_metrics_workspace(one, 1, 1) == 463 * table          # two trips of 512 lanes per block
    assert l.mdf_depth_metrics_workspace((ctypes.c_int64 * 1)(1600 * 1184), 1, 1) == 512 * table          # the cap: more trips
    assert l.mdf_depth_metrics_workspace(one, 9, 1) == -1 and b"bad shape" in l.mdf_last_error()
    assert l.mdf_depth_metrics_workspace((ctypes.c_int64 * 1)(0), 1, 1) == -1
    assert l.mdf_depth_metrics_finalize(None, 0, one, 1, 1, 0, None, None) == -1 and b"null" in l.mdf_last_error()
    p = lambda: (ctypes.c_void_p * 1)(8)
    i = lambda: (ctypes.c_int * 1)(0)
    rc = l.mdf_depth_metrics_reduce_multi(p(), p(), p(), i(), i(), p(), one, 1, ctypes.c_void_p(8), 1, 1, ctypes.c_void_p(8), 5, 1,
                                          ctypes.c_void_p(8), 1 << 30, None)
    assert rc == -1 and b"thresholds" in l.mdf_last_error()
    rc = l.mdf_depth_metrics_reduce_multi(p(), p(), p(), i(), i(), p(), one, 1, ctypes.c_void_p(8), 1, 1, ctypes.c_void_p(8), 3, 1,
                                          ctypes.c_void_p(8), 16, None)
    assert rc == -1 and b"workspace" in l.mdf_last_error()
