"""Numpy mirror of the depth-metrics definitions (include/mdfnet_hip.h: mdf_depth_metrics_*), the reference of the validation tests.

  valid      (double)gt > floor[b]                                  (the training loss's mask)
  non-finite a valid pixel whose est (or conf, lo, hi where given) is not finite counts in n_nonfinite and in nothing else
  e          |est - gt| in float32
  per map    n, n_nonfinite, sum_e, under[t] = #(e < thr[b][t]), covered = #(lo <= gt <= hi), sum_width = sum of float32 (hi - lo)
  per bin    bin = min(max(int(floor(conf * 32 in float32)), 0), 31); n, sum_e, under[t]

Counts are integers; every sum is returned as the correctly rounded float64 sum (math.fsum) of the float32 terms together with the
number of terms and the sum of their magnitudes, from which the tests take the worst-case bound of ANY float64 summation order:
|S - fsum| <= n * 2^-53 * sum|terms|."""
import math

import numpy as np

BINS = 32
COLS = ("n", "n_nonfinite", "sum_e", "under0", "under1", "under2", "under3", "covered", "sum_width")
N, NONFINITE, SUM_E, UNDER, COVERED, SUM_WIDTH = 0, 1, 2, 3, 7, 8
COUNT_COLS = (0, 1, 3, 4, 5, 6, 7)
SUM_COLS = (2, 8)


def _np32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def _floor64(floor):
    """float32 floors are widened exactly, float64 floors taken as they are."""
    return np.asarray(floor).astype(np.float64).reshape(-1)


def metrics(maps, floor, thresholds):
    """maps: list of {"est", "gt" [B,h,w], optional "hypos" [B,D,h,w] | [B,D,1,1], optional "conf" [B,h,w]}; floor [B] (float32 or
    float64); thresholds [B,T] float32 -> dict of [M,33,9] arrays: "table" (float64: counts and fsum sums), "nterms" (int64) and
    "abs" (float64 fsum of |terms|) for the two sum columns."""
    fl = _floor64(floor)
    thr = _np32(thresholds)
    nb = thr.shape[0]
    if fl.shape[0] == 1 and nb > 1:
        fl = np.repeat(fl, nb)
    nt = thr.shape[1]
    m_ = len(maps)
    table = np.zeros((m_, 1 + BINS, len(COLS)), np.float64)
    nterms = np.zeros((m_, 1 + BINS, len(COLS)), np.int64)
    mag = np.zeros((m_, 1 + BINS, len(COLS)), np.float64)
    for m, mp in enumerate(maps):
        est, gt = _np32(mp["est"]), _np32(mp["gt"])
        b = est.shape[0]
        assert b == nb
        valid = gt.astype(np.float64) > fl.reshape(b, 1, 1)
        finite = np.isfinite(est)
        lo = hi = conf = None
        if mp.get("hypos") is not None:
            hy = _np32(mp["hypos"])
            lo = np.broadcast_to(hy[:, 0], est.shape)
            hi = np.broadcast_to(hy[:, -1], est.shape)
            finite = finite & np.isfinite(lo) & np.isfinite(hi)
        if mp.get("conf") is not None:
            conf = _np32(mp["conf"])
            finite = finite & np.isfinite(conf)
        ok = valid & finite
        with np.errstate(all="ignore"):
            e = np.abs(est - gt)                                   # float32
            under = [ok & (e < thr[:, t].reshape(b, 1, 1)) for t in range(nt)]

        def fill(row, sel):
            terms = e[sel].astype(np.float64)
            table[m, row, N] = int(sel.sum())
            table[m, row, SUM_E] = math.fsum(terms.tolist())
            nterms[m, row, SUM_E] = terms.size
            mag[m, row, SUM_E] = math.fsum(np.abs(terms).tolist())
            for t in range(nt):
                table[m, row, UNDER + t] = int((under[t] & sel).sum())

        fill(0, ok)
        table[m, 0, NONFINITE] = int((valid & ~finite).sum())
        if lo is not None:
            with np.errstate(all="ignore"):
                table[m, 0, COVERED] = int((ok & (lo <= gt) & (gt <= hi)).sum())
                width = (hi - lo)[ok].astype(np.float64)            # float32 difference, widened
            table[m, 0, SUM_WIDTH] = math.fsum(width.tolist())
            nterms[m, 0, SUM_WIDTH] = width.size
            mag[m, 0, SUM_WIDTH] = math.fsum(np.abs(width).tolist())
        if conf is not None:
            with np.errstate(all="ignore"):
                scaled = np.floor(np.where(ok, conf, np.float32(0)) * np.float32(BINS))     # float32 product, float32 floor
            bins = np.clip(scaled, 0, BINS - 1).astype(np.int64)
            for k in range(BINS):
                fill(1 + k, ok & (bins == k))
    return {"table": table, "nterms": nterms, "abs": mag}


def check_against(got, ref, T=None):
    """The acceptance rule: counts equal, every sum within n * 2^-53 * sum|terms| of the exact sum.  got [M,33,9] float64."""
    got = np.asarray(got, np.float64)
    tab = ref["table"]
    assert got.shape == tab.shape, (got.shape, tab.shape)
    for c in COUNT_COLS:
        np.testing.assert_array_equal(got[..., c], tab[..., c], err_msg=f"count column {COLS[c]}")
    for c in SUM_COLS:
        bound = ref["nterms"][..., c].astype(np.float64) * 2.0 ** -53 * ref["abs"][..., c]
        err = np.abs(got[..., c] - tab[..., c])
        bad = ~(err <= bound)
        # (inf / nan sums -- a ground truth of +inf -- are compared as such)
        same = (got[..., c] == tab[..., c]) | (np.isnan(got[..., c]) & np.isnan(tab[..., c]))
        assert not (bad & ~same).any(), (COLS[c], got[..., c][bad & ~same], tab[..., c][bad & ~same], bound[bad & ~same])
