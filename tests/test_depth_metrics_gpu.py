"""GPU: the depth-metrics kernels through the C ABI against the numpy mirror (tests/depth_metrics_oracle.py), the stage tap, the
validation drivers end to end and the eval-mode weight packs after training steps.

Acceptance rule of every table: counts (n, n_nonfinite, under, covered, every bin's) EQUAL the mirror's; every float64 sum S
satisfies |S - fsum| <= n * 2^-53 * sum|terms| (the worst case of any float64 summation order over n terms -- derived, not
measured); a second call on the same input gives the same bits."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import depth_metrics_oracle as O
from mdfnet_hip import ddp, ops, synth, valmetrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(maps, floor, thr):
    """maps / floor / thr as numpy -> the device table (checked to be bit-identical on a second call) as numpy."""
    dm = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in m.items()} for m in maps]
    fl, th = torch.from_numpy(np.asarray(floor)).to(DEV), torch.from_numpy(np.asarray(thr, np.float32)).to(DEV)
    t1, view = ops.depth_metrics(dm, fl, th)
    t2, _ = ops.depth_metrics(dm, fl, th)
    assert t1.dtype == torch.float64 and tuple(t1.shape) == (len(maps), 33, 9)
    assert torch.equal(t1.view(torch.int64), t2.view(torch.int64)), "a second call on the same input gave other bits"
    assert torch.equal(view.n, t1[..., 0]) and torch.equal(view.under, t1[..., 3:7]) and torch.equal(view.sum_width, t1[..., 8])
    return t1.cpu().numpy()


def _check(maps, floor, thr):
    got = _run(maps, floor, thr)
    ref = O.metrics(maps, floor, thr)
    O.check_against(got, ref)
    return got, ref


def _random_map(rng, b, h, w, d=4, hypos="pixel", conf=True, holes=0.15):
    gt = (450 + 400 * rng.rand(b, h, w)).astype(np.float32)
    gt[rng.rand(b, h, w) < holes] = 0.0
    est = (gt + rng.randn(b, h, w).astype(np.float32) * 5).astype(np.float32)
    m = {"est": est, "gt": gt}
    if hypos == "pixel":
        m["hypos"] = np.sort((gt[:, None] + rng.randn(b, d, h, w) * 6).astype(np.float32), axis=1)
    elif hypos == "flat":
        m["hypos"] = np.stack([np.linspace(425 + 10 * i, 935 - 10 * i, d) for i in range(b)]).astype(np.float32).reshape(b, d, 1, 1)
    if conf:
        m["conf"] = (rng.rand(b, h, w) * 1.1 - 0.05).astype(np.float32)
    return m


def test_small_and_odd_shapes():
    """One pixel, one lane short of / exactly / one lane past a wave, an odd map, one pixel past 4 * 256."""
    rng = np.random.RandomState(0)
    thr = np.array([[2.0, 4.0, 8.0]], np.float32)
    for h, w in ((1, 1), (1, 63), (1, 64), (1, 65), (7, 37), (1, 4 * 256 + 1)):
        for hypos in ("pixel", "flat"):
            got, _ = _check([_random_map(rng, 1, h, w, hypos=hypos, holes=0.0 if h * w == 1 else 0.15)], np.array([425.0]), thr)
        assert got[0, 0, O.N] >= 1 and got[0, 1:, O.N].sum() == got[0, 0, O.N]


@pytest.mark.parametrize("floor_dtype", [np.float64, np.float32])
def test_batch_items_with_their_own_floor_and_thresholds(floor_dtype):
    rng = np.random.RandomState(1)
    for b in (1, 2, 3):
        floor = np.array([425.0, 600.0, 700.5][:b], dtype=floor_dtype)
        thr = np.array([[2.0, 4.0, 8.0], [0.5, 1.0, 30.0], [3.0, 3.5, 4.0]][:b], np.float32)
        maps = [_random_map(rng, b, 11, 29)]
        maps[0]["gt"][:, 0, :3] = np.float32(floor.reshape(b, 1))            # gt equal to the floor: invalid
        got, ref = _check(maps, floor, thr)
        assert got[0, 0, O.N] > 0
    # the comparison is made in the floor's own precision: float32(425.1) lies above the double 425.1, so a ground truth of
    # float32(425.1) is valid against the float64 floor 425.1 and invalid against the float32 floor; one ulp more is valid for both
    f32 = np.float32(425.1)
    gt = np.array([[[f32, np.nextafter(f32, np.float32(1e9))]]], np.float32)
    got, _ = _check([{"est": gt + 1, "gt": gt}], np.array([425.1], dtype=floor_dtype), np.array([[2.0]], np.float32))
    assert got[0, 0, O.N] == (1 if floor_dtype is np.float32 else 2)


def test_four_maps_in_one_launch_and_one_map():
    rng = np.random.RandomState(2)
    maps = [_random_map(rng, 2, 16, 20, d=48, hypos="flat", conf=False), _random_map(rng, 2, 32, 40, d=24, conf=False),
            _random_map(rng, 2, 64, 80, d=8, conf=False), _random_map(rng, 2, 128, 160, hypos=None, conf=True)]
    floor, thr = np.array([425.0, 500.0]), np.array([[2.0, 4.0, 8.0], [1.0, 2.0, 3.0]], np.float32)
    got, ref = _check(maps, floor, thr)
    assert (got[:3, 1:] == 0).all() and got[3, 0, O.COVERED] == 0 and got[3, 0, O.SUM_WIDTH] == 0      # absent inputs: zero
    for i, m in enumerate(maps):                       # M = 1: every map alone (another grid, so another order of the sums)
        alone, _ = _check([m], floor, thr)
        for c in O.COUNT_COLS:
            assert np.array_equal(alone[0, :, c], got[i, :, c])


@pytest.mark.parametrize("nthr,h,w", [(1, 592, 800), (4, 592, 800), (3, 1, 512 * 1024 + 513)])
def test_large_map_takes_several_trips(nthr, h, w):
    """592 x 800 = 473600 pixels: 463 blocks whose lanes take two pixels (the last trip ragged).  512 * 1024 + 513 pixels: past the
    launch cap of 512 blocks, a third, ragged trip."""
    rng = np.random.RandomState(3)
    thr = np.array([[2.0, 4.0, 8.0, 16.0][:nthr]], np.float32)
    got, ref = _check([_random_map(rng, 1, h, w, d=2)], np.array([425.0]), thr)
    assert got[0, 0, O.N] > 300000 and (got[0, :, O.UNDER + nthr:O.COVERED] == 0).all()


def test_edge_values():
    f = np.float32
    gt = np.array([[[425.0, 0.0, 500.0, 500.0, 600.0, 700.0, 500.0, 500.0, 500.0, 500.0, 500.0, 500.0]]], f)
    est = np.array([[[430.0, 1.0, 502.0, 501.0, 600.0, 700.0, np.nan, np.inf, -np.inf, 500.5, 500.5, 500.5]]], f)
    conf = np.array([[[0.5, 0.5, 1.0, np.nextafter(f(1), f(2)), 1.3, -0.01, 0.5, 0.5, 0.5, np.nan, 0.0, 0.999]]], f)
    hyp = np.array([500.0, 550.0, 600.0], f).reshape(1, 3, 1, 1)
    got, _ = _check([{"est": est, "gt": gt, "hypos": hyp, "conf": conf}], np.array([425.0]), np.array([[2.0, 0.5]], f))
    row = got[0, 0]
    # valid and finite: e = 2, 1, 0, 0, 0.5, 0.5;  e == 2 is not under 2, e == 0.5 is not under 0.5
    assert row[O.N] == 6 and row[O.NONFINITE] == 4 and row[O.SUM_E] == 4.0 and row[O.UNDER] == 5 and row[O.UNDER + 1] == 2
    assert row[O.COVERED] == 5 and row[O.SUM_WIDTH] == 600.0                    # gt == lo, gt == hi covered; 700 is not
    assert got[0, 1 + 31, O.N] == 4 and got[0, 1 + 0, O.N] == 2                 # 1, nextafter(1), 1.3, 0.999 | -0.01, 0
    # lo > hi: nothing is covered, the width is negative; hypotheses per pixel with a NaN plane: non-finite
    rng = np.random.RandomState(4)
    m = _random_map(rng, 1, 5, 70, holes=0.0)
    m["hypos"] = m["hypos"][:, ::-1].copy()
    m["hypos"][0, 0, 0, 0] = np.nan
    got, _ = _check([m], np.array([425.0]), np.array([[2.0]], f))
    assert got[0, 0, O.COVERED] == 0 and got[0, 0, O.SUM_WIDTH] < 0 and got[0, 0, O.NONFINITE] == 1
    # an all-invalid map, and one whose ground truth is all holes
    m = _random_map(rng, 1, 3, 130)
    got, _ = _check([m], np.array([1e6]), np.array([[2.0]], f))
    assert (got == 0).all()
    m["gt"][:] = 0.0
    got, _ = _check([m], np.array([425.0]), np.array([[2.0]], f))
    assert (got == 0).all()


def test_confidence_bin_patterns():
    """Every pixel in one bin (one wave round), and lane i in bin i % 32 (every round of every wave is taken)."""
    rng = np.random.RandomState(5)
    thr = np.array([[2.0, 4.0, 8.0]], np.float32)
    m = _random_map(rng, 1, 9, 300, hypos=None, holes=0.1)
    m["conf"] = np.full_like(m["gt"], 0.4)
    got, _ = _check([m], np.array([425.0]), thr)
    assert got[0, 1 + 12, O.N] == got[0, 0, O.N] > 0 and got[0, 1 + 12, O.SUM_E] != 0
    lanes = np.arange(9 * 300).reshape(1, 9, 300)
    m["conf"] = (((lanes % 32) + 0.5) / 32).astype(np.float32)
    got, _ = _check([m], np.array([425.0]), thr)
    assert (got[0, 1:, O.N] > 0).all()


def test_bad_arguments_are_refused():
    z = torch.zeros(1, 4, 4, device=DEV)
    fl = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="1 to 8 maps"):
        ops.depth_metrics([{"est": z, "gt": z}] * 9, fl, torch.ones(1, 3, device=DEV))
    with pytest.raises(ValueError, match="thresholds"):
        ops.depth_metrics([{"est": z, "gt": z}], fl, torch.ones(1, 5, device=DEV))
    with pytest.raises(ValueError, match="conf"):
        ops.depth_metrics([{"est": z, "gt": z, "conf": torch.zeros(1, 2, 2, device=DEV)}], fl, torch.ones(1, 3, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- the model
def _model(confidence="last", seed=1):
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        m = config.build_model(confidence=confidence)
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=seed))
    return m


@pytest.mark.parametrize("confidence", ["last", "cascade"])
def test_outputs_are_bit_identical_with_and_without_the_tap(confidence):
    model = _model(confidence).eval().to(DEV)
    scene = [t.to(DEV) for t in synth.make_scene(160, 128, 3, batch=1, rot_deg=2.0, seed=3)]
    keys = [("scan", v) for v in range(3)]
    with torch.no_grad():
        plain = model(*scene, feature_cache={}, view_keys=keys)
        cache, taps = {}, []
        tapped = model(*scene, feature_cache=cache, view_keys=keys, stage_tap=taps)
        calls = []
        again = model(*scene, feature_cache=cache, view_keys=keys, stage_tap=lambda rec: calls.append(rec["stage"]))
    for k in ("depth", "confidence"):
        assert torch.equal(plain[k], tapped[k]) and torch.equal(plain[k], again[k]), k
    assert [r["stage"] for r in taps] == [0, 1, 2, "final"] == calls and len(cache) == 3
    assert [tuple(r["depth"].shape) for r in taps] == [(1, 16, 20), (1, 32, 40), (1, 64, 80), (1, 128, 160)]
    assert [tuple(r["hypos"].shape) for r in taps[:3]] == [(1, 48, 1, 1), (1, 24, 32, 40), (1, 8, 64, 80)]
    assert taps[3]["depth"] is tapped["depth"] and taps[3]["confidence"] is tapped["confidence"]
    model.train()
    with pytest.raises(RuntimeError, match="eval-mode hook"):
        model(*scene, stage_tap=[])


def _reference_total(all_taps, dataset, thresholds, relative):
    """The mirror applied to the tapped tensors, item by item, added up."""
    total = None
    for taps, item in zip(all_taps, dataset):
        gt = {k: np.asarray(v)[None] for k, v in item["ref_depths"].items()}
        maps = []
        for rec in taps:
            m = {"est": rec["depth"].cpu().numpy(), "gt": gt[valmetrics.GT_KEYS[-1 if rec["stage"] == "final" else rec["stage"]]]}
            if rec["stage"] == "final":
                m["conf"] = rec["confidence"].cpu().numpy()
            else:
                m["hypos"] = rec["hypos"].cpu().numpy()
            maps.append(m)
        dr = np.asarray(item["depth_range"], np.float64).reshape(1, 2)
        ref = O.metrics(maps, dr[:, 0], valmetrics.item_thresholds(dr, thresholds, relative).numpy())
        total = ref if total is None else {k: total[k] + ref[k] for k in ref}
    return total


def _check_report(rep, table, ref, thresholds):
    O.check_against(table.numpy(), ref)
    want = valmetrics.make_report(table, thresholds, relative=rep["relative"], items=rep["items"])
    assert json.dumps(valmetrics.json_safe(want["maps"])) == json.dumps(valmetrics.json_safe(rep["maps"]))
    for name in ("stage0", "stage1", "stage2"):
        assert 0.0 <= rep["maps"][name]["coverage"] <= 1.0 and rep["maps"][name]["n"] > 0
    assert rep["maps"]["final"]["n"] == int(ref["table"][3, 0, O.N]) and len(rep["confidence"]) == 32
    assert rep["confidence"][-1]["share"] == 1.0


def test_validate_driver_on_dtu(tmp_path, monkeypatch, capsys):
    """`validate.py -d dtu -p CKPT` on a synthetic DTU tree (160 x 128, 2 validation scans): prints both tables, writes the JSON; the
    numbers are the mirror's on the tapped tensors.  (Random weights, synthetic ground truth: no bar on the quality numbers.)"""
    import config
    import validate
    from load import synthetic
    root = tmp_path / "data"
    synthetic.write_dtu_train_set(str(root / "dtu640x512"), scenes=(3, 5), nviews_total=5, lightings=(3,), width=160, height=128)
    monkeypatch.setattr(config, "DATA_ROOT", str(root))
    monkeypatch.setattr(config, "OUTPUT_ROOT", str(tmp_path / "out"))
    monkeypatch.setattr(config.LoadDTU, "show_args", lambda self: None)
    real = config.LoadDTU

    def two_scans():
        a = real()
        a.val_label = [s for s in a.val_label if s in (3, 5)]
        return a
    monkeypatch.setattr(config, "LoadDTU", two_scans)
    model = _model("cascade", seed=2)
    ckpt = str(tmp_path / "ck.pth")
    torch.save({"epoch": 1, "model": model.state_dict()}, ckpt)
    all_taps, results = [], []
    real_run = valmetrics.run_validation

    def recording_run(*a, **k):
        results.append(real_run(*a, taps_out=all_taps, **k))
        return results[-1]
    monkeypatch.setattr(valmetrics, "run_validation", recording_run)
    out = str(tmp_path / "rep" / "val.json")
    rep = validate.main(["-p", ckpt, "-d", "dtu", "--confidence", "cascade", "--out", out])
    text = capsys.readouterr().out
    assert "stage0" in text and "final map by confidence" in text and os.path.exists(out[:-5] + ".txt")
    disk = json.load(open(out))
    assert disk["items"] == 10 and disk["options"]["confidence"] == "cascade" and disk["thresholds"] == [2.0, 4.0, 8.0]
    dataset = validate.val_dataset("dtu", 5)
    assert len(dataset) == 10 and len(all_taps) == 10
    ref = _reference_total(all_taps, dataset, valmetrics.DTU_THRESHOLDS, False)
    _check_report(rep, results[0][1], ref, valmetrics.DTU_THRESHOLDS)
    table = torch.from_numpy(ref["table"])          # counts must match exactly: the report's ratios from the mirror's counts
    assert disk["maps"]["final"]["n"] == int(table[3, 0, O.N]) and disk["maps"]["stage2"]["n"] == int(table[2, 0, O.N])
    for name, i in (("stage0", 0), ("stage1", 1), ("stage2", 2)):
        assert disk["maps"][name]["coverage"] == float(table[i, 0, O.COVERED] / table[i, 0, O.N])
        assert 0.0 <= disk["maps"][name]["coverage"] <= 1.0
    # stage 0 is handed the uniform hypotheses over the whole range: the interval is depth_max - depth_min wide
    assert abs(disk["maps"]["stage0"]["mean_width"] - 510.0) <= 510.0 * 2 ** -20
    mean = ref["table"][3, 0, O.SUM_E] / ref["table"][3, 0, O.N]
    assert abs(disk["maps"]["final"]["mean_abs_err"] - mean) <= 1e-9 * mean


def test_validation_on_blendedmvs_list(tmp_path):
    from load import synthetic
    from load.blendedtrain import LoadDataset
    root = synthetic.write_blendedmvs_set(str(tmp_path / "bl"), scans=("scanA", "scanB"), nviews_total=6, short_pairs=False)
    with open(os.path.join(root, "validation_list.txt"), "w") as f:
        f.write("scanB\n")
    dataset = LoadDataset(root, nviews=5, robust_train=False, listfile="validation_list.txt")
    assert len(dataset) == 6
    model = _model("last").eval().to(DEV)
    all_taps = []
    rep, table = valmetrics.run_validation(model, dataset, torch.device(DEV), valmetrics.RELATIVE_THRESHOLDS, True, taps_out=all_taps)
    assert rep["items"] == 6 and rep["relative"] and not model.training
    ref = _reference_total(all_taps, dataset, valmetrics.RELATIVE_THRESHOLDS, True)
    _check_report(rep, table, ref, valmetrics.RELATIVE_THRESHOLDS)
    width = 941.0 - 421.0                                   # scanB's depth range (load/synthetic.py)
    assert abs(rep["maps"]["stage0"]["mean_width"] - width) <= width * 2 ** -20
    again, table2 = valmetrics.run_validation(model, dataset, torch.device(DEV), valmetrics.RELATIVE_THRESHOLDS, True)
    assert torch.equal(table.view(torch.int64), table2.view(torch.int64))          # run-to-run bit-identical


# ---------------------------------------------------------------------------------------------------- packs after training steps
W, H, V = 192, 128, 3


class _Scenes(torch.utils.data.Dataset):
    """Loader-shaped items made in memory."""

    def __init__(self, seeds):
        self.items = []
        for k in seeds:
            imgs, extr, intr, dr = synth.make_scene(W, H, V, batch=1, rot_deg=2.0 + k, seed=11 + 5 * k)
            rng = np.random.RandomState(100 + k)
            lo, hi = float(dr[0, 0]), float(dr[0, 1])
            gt = {str(s): (lo - 20 + (hi - lo + 20) * rng.rand(H >> s, W >> s)).astype(np.float32) for s in (3, 2, 1, 0)}
            self.items.append({"imgs": imgs[0].numpy(), "extrinsics": extr[0].numpy(), "intrinsics": intr[0].numpy(),
                               "ref_depths": gt, "depth_range": dr[0].double().numpy()})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _batch(ds, i):
    it = ds[i]
    t = lambda a: torch.from_numpy(np.asarray(a))[None]
    return t(it["imgs"]), t(it["extrinsics"]), t(it["intrinsics"]), t(it["depth_range"]), {k: t(v) for k, v in it["ref_depths"].items()}


def _validate_fresh_copy(model, val):
    fresh = _model("last", seed=9)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    return valmetrics.run_validation(fresh.to(DEV), val, torch.device(DEV))[1]


@pytest.mark.parametrize("hipgraph", [False, True])
def test_validation_after_training_steps_sees_the_current_weights(hipgraph):
    """One training step on the HIP kernels, then validate: the eval-mode packs (BatchNorm folded) must be those of the stepped
    weights and running statistics, i.e. the result equals a freshly built model's loaded from the same state_dict.  hipgraph: the
    step replayed from its recording, validation between two replays."""
    from mdfnet_hip.optim import FlatAdam
    from net.loss import Loss
    train, val = _Scenes([0, 1]), _Scenes([2])
    model = _model("last").to(DEV)
    dev = torch.device(DEV)
    before = valmetrics.run_validation(model, val, dev)[1]             # builds the eval-mode packs of the initial weights
    model.train()
    crit = Loss().to(DEV)
    bucket = ddp.FlatBucket(model)
    opt = FlatAdam(bucket, lr=1e-2)
    if hipgraph:
        from mdfnet_hip.graphstep import GraphedTrainStep
        b0 = _batch(train, 0)
        step = GraphedTrainStep(model, crit, bucket, opt, tuple(t.to(DEV) for t in b0[:4]) + ({k: v.to(DEV) for k, v in b0[4].items()},), warmup=1)
        loss = float(step(*_batch(train, 1)))
    else:
        imgs, extr, intr, dr, gt = _batch(train, 0)
        out = model(imgs.to(DEV), extr.to(DEV), intr.to(DEV), dr.to(DEV))
        loss_t = crit(out, {k: v.to(DEV) for k, v in gt.items()}, dr.to(DEV))
        bucket.zero_grad()
        loss_t.backward()
        bucket.allreduce_gradients()
        opt.step()
        loss = float(loss_t)
    assert np.isfinite(loss)
    after = valmetrics.run_validation(model, val, dev)[1]
    assert model.training                                              # back in the mode it came in
    assert not torch.equal(after, before), "the training step changed nothing that validation sees"
    want = _validate_fresh_copy(model, val)
    assert torch.equal(after.view(torch.int64), want.view(torch.int64))
    if hipgraph:
        assert np.isfinite(float(step(*_batch(train, 0))))             # the recording still replays after the eager pass
        after2 = valmetrics.run_validation(model, val, dev)[1]
        assert torch.equal(after2.view(torch.int64), _validate_fresh_copy(model, val).view(torch.int64))


def test_train_driver_val_every(tmp_path):
    """`train.py -d blendedmvs --val_every 1` for one epoch (a fresh process, as a user starts it): epoch_val.txt gets one line, and
    its numbers are those of a freshly built model loaded from the epoch's checkpoint -- which in turn equal the mirror applied to
    the tapped tensors."""
    import subprocess
    import sys
    from load import synthetic
    from load.blendedtrain import LoadDataset
    from tools import data_io
    root = tmp_path / "data" / "blendedmvs768x576"
    synthetic.write_blendedmvs_set(str(root), scans=("scanA", "scanB"), nviews_total=7, width=128, height=96, short_pairs=False)
    with open(str(root / "validation_list.txt"), "w") as f:
        f.write("scanB\n")
    pkg = os.path.dirname(os.path.dirname(data_io.__file__))
    env = dict(os.environ, MDF_DATA_ROOT=str(tmp_path / "data"), MDF_PTH_PATH=str(tmp_path / "pth"), MDF_MAX_EPOCH="1", OMP_NUM_THREADS="2",
               PYTHONPATH=pkg)
    r = subprocess.run([sys.executable, os.path.join(pkg, "train.py"), "-d", "blendedmvs", "--val_every", "1"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = open(str(tmp_path / "pth" / "epoch_val.txt")).read().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["epoch"] == 1 and line["items"] == 7 and line["relative"] and len(line["confidence"]) == 32
    ck = torch.load(str(tmp_path / "pth" / "blendedmvs_1.pth"), map_location="cpu")
    model = _model("last", seed=4)
    model.load_state_dict(ck["model"])
    dataset = LoadDataset(str(root), nviews=5, robust_train=False, listfile="validation_list.txt")
    all_taps = []
    rep, table = valmetrics.run_validation(model.eval().to(DEV), dataset, torch.device(DEV), valmetrics.RELATIVE_THRESHOLDS, True, taps_out=all_taps)
    assert json.dumps(valmetrics.json_safe(rep["maps"])) == json.dumps(line["maps"])
    assert json.dumps(valmetrics.json_safe(rep["confidence"])) == json.dumps(line["confidence"])
    _check_report(rep, table, _reference_total(all_taps, dataset, valmetrics.RELATIVE_THRESHOLDS, True), valmetrics.RELATIVE_THRESHOLDS)
