"""Validation: depth metrics of every stage of the cascade against the loader's ground-truth pyramid, accumulated on the device.

One item = one eval-mode forward with a stage tap (net/core.py) + one ops.depth_metrics call over four maps (stage 0, 1, 2 at 1/8,
1/4, 1/2 of the image and the refined depth at full size).  Per map: mean absolute error and the share of valid pixels under each
threshold; for the three stages how often the true depth lies inside the hypothesis interval the stage was given (the only pixels a
coarse-to-fine cascade can still recover -- what --curves / --prob_thresh control) and how wide that interval is; for the final map a
confidence table (32 bins) from which a filter threshold is read, for --confidence last or cascade alike.

Counts are exact.  The float64 sums are added in item order on every rank and over the ranks by one all_reduce, so their last bits
depend on the world size (not on the run: for a fixed world size the report is bit-identical from run to run)."""
import json
import math

import torch

from . import hostmirror, ops, shard

MAP_NAMES = ("stage0", "stage1", "stage2", "final")
GT_KEYS = ("3", "2", "1", "0")                      # the loader's pyramid: 1/8, 1/4, 1/2, 1/1 (load/dtutrain.py)
DTU_THRESHOLDS = (2.0, 4.0, 8.0)                    # mm
RELATIVE_THRESHOLDS = (1.0 / 256, 1.0 / 128, 1.0 / 64)     # of depth_max - depth_min; at DTU's 510 mm: 1.99, 3.98, 7.97 mm
_N, _NONFINITE, _SUM_E, _UNDER, _COVERED, _SUM_WIDTH = 0, 1, 2, 3, 7, 8


class Accumulator:
    """Sum of the per-item tables [M, 33, 9], kept on the device and added in item order."""

    def __init__(self, device, nmaps=len(MAP_NAMES)):
        self.total = torch.zeros((nmaps, 1 + ops.METRIC_BINS, len(ops.METRIC_COLUMNS)), dtype=torch.float64, device=device)
        self.items = 0

    def add(self, table):
        self.total += table
        self.items += 1

    def reduce(self):
        """-> (table over all ranks as a CPU float64 tensor, items over all ranks): one float64 all_reduce(SUM)."""
        packed = torch.cat([self.total.reshape(-1), torch.tensor([float(self.items)], dtype=torch.float64, device=self.total.device)])
        packed = shard.sum_tensor_over_ranks(packed).cpu()
        return packed[:-1].reshape(self.total.shape), int(packed[-1].item())


def _ratio(a, b):
    return float(a) / float(b) if float(b) > 0 else float("nan")


def make_report(table, thresholds, names=MAP_NAMES, relative=False, items=None, world=1):
    """table [M, 33, 9] (CPU) -> the report as a plain dict.  thresholds: the T labels (mm, or fractions of the depth range when
    relative).  Means over n = 0 pixels are NaN."""
    t = torch.as_tensor(table, dtype=torch.float64)
    nthr = len(thresholds)
    maps = {}
    for m, name in enumerate(names):
        row = t[m, 0]
        n = row[_N].item()
        entry = {"n": int(n), "n_nonfinite": int(row[_NONFINITE].item()), "mean_abs_err": _ratio(row[_SUM_E], n),
                 "under": [_ratio(row[_UNDER + k], n) for k in range(nthr)]}
        if name != "final":
            entry["coverage"] = _ratio(row[_COVERED], n)
            entry["mean_width"] = _ratio(row[_SUM_WIDTH], n)
        maps[name] = entry
    rep = {"thresholds": [float(x) for x in thresholds], "relative": bool(relative), "maps": maps,
           "sums": "counts are exact; the last bits of the float64 sums depend on the world size (%d here)" % world}
    if items is not None:
        rep["items"] = int(items)
    if "final" in names:
        # top-down: row k is "every valid pixel with confidence >= k/32" = bins k .. 31 (bin 31 also holds confidences above 1,
        # bin 0 those below 0)
        bins = t[list(names).index("final"), 1:]
        total = bins[:, _N].sum().item()
        n = se = 0.0
        un = [0.0] * nthr
        rows = []
        for k in range(ops.METRIC_BINS - 1, -1, -1):
            n += bins[k, _N].item()
            se += bins[k, _SUM_E].item()
            for j in range(nthr):
                un[j] += bins[k, _UNDER + j].item()
            rows.append({"conf_ge": k / ops.METRIC_BINS, "share": _ratio(n, total), "mean_abs_err": _ratio(se, n),
                         "under": [_ratio(u, n) for u in un]})
        rep["confidence"] = rows
    return rep


def _fmt(x, spec="{:.4f}"):
    return "-" if (isinstance(x, float) and math.isnan(x)) else spec.format(x)


def format_report(rep):
    """The report as a text table (NaN printed as '-')."""
    unit = "x range" if rep["relative"] else "mm"
    heads = ["<" + "{:g}".format(x) for x in rep["thresholds"]]
    lines = ["validation" + (" ({} items)".format(rep["items"]) if "items" in rep else "") + "; thresholds in " + unit,
             "{:<8}{:>12}{:>10}{:>12}".format("map", "n", "nonfinite", "mean|e|") + "".join("{:>12}".format(h) for h in heads)
             + "{:>10}{:>12}".format("coverage", "width")]
    for name, e in rep["maps"].items():
        lines.append("{:<8}{:>12d}{:>10d}{:>12}".format(name, e["n"], e["n_nonfinite"], _fmt(e["mean_abs_err"]))
                     + "".join("{:>12}".format(_fmt(u)) for u in e["under"])
                     + "{:>10}{:>12}".format(_fmt(e.get("coverage", float("nan"))), _fmt(e.get("mean_width", float("nan")))))
    if "confidence" in rep:
        lines.append("")
        lines.append("final map by confidence")
        lines.append("{:<10}{:>10}{:>12}".format("conf >=", "share", "mean|e|") + "".join("{:>12}".format(h) for h in heads))
        for r in rep["confidence"]:
            lines.append("{:<10}{:>10}{:>12}".format(_fmt(r["conf_ge"], "{:.5f}"), _fmt(r["share"]), _fmt(r["mean_abs_err"]))
                         + "".join("{:>12}".format(_fmt(u)) for u in r["under"]))
    lines.append("")
    lines.append(rep["sums"])
    return "\n".join(lines)


def json_safe(x):
    if isinstance(x, dict):
        return {k: json_safe(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [json_safe(v) for v in x]
    if isinstance(x, float) and not math.isfinite(x):
        return None
    return x


def report_json(rep):
    """NaN (a mean over no pixels) is written as null."""
    return json.dumps(json_safe(rep), indent=1)


def item_thresholds(depth_range_host, thresholds, relative):
    """-> float32 [B, T] on the host: absolute thresholds as given, relative ones times each item's depth_max - depth_min."""
    dr = torch.as_tensor(depth_range_host, dtype=torch.float64).reshape(-1, 2)
    t = torch.tensor([float(x) for x in thresholds], dtype=torch.float64).reshape(1, -1)
    if relative:
        return ((dr[:, 1] - dr[:, 0]).reshape(-1, 1) * t).float().contiguous()
    return t.expand(dr.shape[0], -1).float().contiguous()


def tapped_maps(taps, ref_depths):
    """The stage tap's records + the ground-truth pyramid -> the `maps` argument of ops.depth_metrics (stage 0, 1, 2, final)."""
    maps = []
    for rec in taps:
        if rec["stage"] == "final":
            maps.append({"est": rec["depth"], "gt": ref_depths[GT_KEYS[-1]], "conf": rec["confidence"]})
        else:
            maps.append({"est": rec["depth"], "gt": ref_depths[GT_KEYS[rec["stage"]]], "hypos": rec["hypos"]})
    return maps


def validate_batch(model, batch, thr, taps_out=None, **forward_kw):
    """One eval-mode forward with the stage tap and one metrics call -> table [4, 33, 9] on the device.  batch: the loader's keys on
    the device; thr [B, T] on the device.  taps_out: a list that receives the tapped records (tests)."""
    taps = []
    with torch.no_grad():
        model(batch["imgs"], batch["extrinsics"], batch["intrinsics"], batch["depth_range"], stage_tap=taps, **forward_kw)
        maps = tapped_maps(taps, batch["ref_depths"])
        table, _ = ops.depth_metrics(maps, batch["depth_range"][:, 0], thr)
    if taps_out is not None:
        taps_out.append(taps)
    return table


def run_validation(model, dataset, device, thresholds=DTU_THRESHOLDS, relative=False, rank=0, world=1, nworks=0, log=None,
                   taps_out=None):
    """Shard `dataset` (a training loader built with robust_train=False) over the ranks like eval.py, validate item by item in
    eval mode and reduce over the ranks -> (report dict, table [4,33,9] CPU).  The model is put back into the mode it came in.  Runs
    eagerly (between the replays of a recorded training step too)."""
    from torch.utils.data import DataLoader, Subset
    from torch.autograd import graph as _graph
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("validation runs on the hand-written MI355X kernels (eval-mode forward + ops.depth_metrics); there is no CPU fallback")
    was_training = model.training
    model.eval()
    # BatchNorm statistics are written through raw pointers by the training kernels: make sure the folded eval-mode packs
    # (layers._Folded, keyed on tensor versions) are rebuilt from the current values
    _graph.increment_version([b for b in model.buffers() if b.is_cuda])
    idx = shard.shard_items(len(dataset), rank, world)
    loader = DataLoader(Subset(dataset, idx), batch_size=1, num_workers=nworks, shuffle=False, pin_memory=True, drop_last=False)
    acc = Accumulator(device)
    try:
        for it, data in enumerate(loader):
            batch = {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in data.items() if k != "ref_depths"}
            batch["ref_depths"] = {k: v.to(device, non_blocking=True) for k, v in data["ref_depths"].items()}
            for k in ("extrinsics", "intrinsics", "depth_range"):       # the loader's CPU tensors ARE the host mirrors
                hostmirror.put(batch[k], data[k])
            thr = item_thresholds(data["depth_range"], thresholds, relative).to(device, non_blocking=True)
            acc.add(validate_batch(model, batch, thr, taps_out=taps_out))
            if log is not None:
                log("validation item {}/{}".format(it + 1, len(loader)))
    finally:
        model.train(was_training)
    table, items = acc.reduce()
    return make_report(table, thresholds, relative=relative, items=items, world=world), table
