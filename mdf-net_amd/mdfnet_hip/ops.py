"""Torch-facing wrappers over the C ABI (include/mdfnet_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every operator below is one
(or a few) hand-written HIP kernels.  No fallback: tensors must live on a HIP device.
"""
import ctypes
import os
import threading

import torch

from . import check, lib

FEA_NHWC = 1
VOL_NCDHW, VOL_NDHWC = 0, 1

# Optional per-launch timing (bench.py's roofline pass): when `_prof` is a list, every C-ABI call is bracketed by
# HIP events recorded on the stream the kernel is launched on, with its algorithmic work attached.
_prof = None


def profile_begin():
    global _prof
    _prof = []


def profile_end():
    """-> list of (abi_name, tag, ms, work-dict) for every launch since profile_begin()."""
    global _prof
    recs, _prof = _prof, None
    torch.cuda.synchronize()
    return [(n, tag, e0.elapsed_time(e1), work) for n, tag, e0, e1, work in recs]


_counts = None      # optional census of the C-ABI entries called (tests: "which kernels actually ran in this process")


def count_begin():
    global _counts
    _counts = {}


def count_end():
    global _counts
    c, _counts = _counts, None
    return c


def _abi(name, args, tag="", work=None):
    fn = getattr(lib(), name)
    if _counts is not None:
        _counts[name] = _counts.get(name, 0) + 1
    if _prof is None:
        check(fn(*args), name)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(*args), name)
    e1.record()
    _prof.append((name, tag, e0, e1, dict(work or {}, kernel=lib().mdf_last_launch().decode())))


class _single_thread:
    """Tiny host-side linear algebra (3x3 / 4x4) must not be fanned out over a 256-thread pool: on the GPU box the
    fork/join alone cost 56 ms per call (scripts/profile_forward.py)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        if self.n > 1:
            torch.set_num_threads(1)

    def __exit__(self, *a):
        if self.n > 1:
            torch.set_num_threads(self.n)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    """The current HIP stream of t's device as a raw handle (the private fast getter when this torch has it: ~10x cheaper than
    building a torch.cuda.Stream object per launch, which matters at ~450 launches per training step)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mdfnet_hip ops run on an MI355X only (got a CPU tensor); there is no CPU fallback")


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def nhwc(t):
    """[B,C,h,w] -> same logical tensor whose memory is [B,h,w,C] (no copy when already so)."""
    return t.float().contiguous(memory_format=torch.channels_last)


# --------------------------------------------------------------------------- recorded host values (parity tests)
# The few host-side control-plane computations (4x4 inverse / matmul, the gauss-fit row, log of the threshold) go through
# LAPACK/BLAS/libm, whose code paths differ per x86 host at cond ~1e14.  The e2e goldens therefore carry
# the values the REAL reference computed on the build host (oracle/gen_golden.py:HostValueRecorder); inside
# `recorded_host_values(...)` the host functions below hand those out instead of computing them, so the device path can be
# compared with the golden depth at the metric's own 1e-3 bar on any host.  Never active in the product path.
_recorded = threading.local()


class recorded_host_values:
    def __init__(self, projs=None, fit_row=None, log_thresh=None, cams=None):
        """projs: list (per aggregate call) of [n_src,B,12]; cams: list (per scale call) of [B,V,3,4]; fit_row [B,D];
        log_thresh: {mode: float}."""
        self.v = {"projs": list(projs or []), "cams": list(cams or []), "fit_row": fit_row, "log_thresh": log_thresh or {}}

    def __enter__(self):
        _recorded.v = self.v
        return self

    def __exit__(self, *exc):
        _recorded.v = None


def recorded(kind, key=None):
    v = getattr(_recorded, "v", None)
    if v is None:
        return None
    if kind in ("projs", "cams"):
        return torch.as_tensor(v[kind].pop(0)).float().contiguous() if v[kind] else None
    if kind == "log_thresh":
        return v["log_thresh"].get(key)
    return None if v[kind] is None else torch.as_tensor(v[kind]).float().contiguous()


def relative_projections(ref_proj, src_projs):
    """HOST side of homo_warping (base.py:98): (src_proj @ inverse(ref_proj))[:3,:4] for every source
    view, computed on the CPU with the reference's own torch calls so the kernel consumes the same
    12 floats as the oracle (GPU and CPU `torch.inverse` use different solvers).  -> [n_src,B,12] CPU."""
    pinned = recorded("projs")
    if pinned is not None:
        return pinned
    ref = ref_proj.detach().to("cpu", torch.float32)
    with _single_thread():
        inv = torch.inverse(ref)
        rows = [torch.matmul(sp.detach().to("cpu", torch.float32), inv)[:, :3, :4].reshape(-1, 12) for sp in src_projs]
        return torch.stack(rows, 0).contiguous()


def _hypos_arg(hypos, h, w):
    per_pixel = int(hypos.shape[-1] != 1 or hypos.shape[-2] != 1)
    if per_pixel and (hypos.shape[-2] != h or hypos.shape[-1] != w):
        raise ValueError(f"depth_hypos {tuple(hypos.shape)} does not match feature size {(h, w)}")
    return _f32c(hypos), per_pixel


def homo_warp(src_fea, proj12, depth_hypos):
    """net/unit/base.py:85-126 with proj12 = relative_projections(...)[v] on device -> [B,C,D,h,w]."""
    _need_gpu(src_fea, proj12, depth_hypos)
    b, c, h, w = src_fea.shape
    d = depth_hypos.shape[1]
    fea = nhwc(src_fea)
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    out = torch.empty((b, c, d, h, w), device=src_fea.device, dtype=torch.float32)
    _abi("mdf_homo_warp_fwd", (fea.data_ptr(), FEA_NHWC, _f32c(proj12).data_ptr(), hyp.data_ptr(), pp,
                                  out.data_ptr(), VOL_NCDHW, b, c, d, h, w, _stream(out),))
    return out


def warp_corner_indices(proj12, depth_hypos, h, w):
    """int32 [B,D,h,w,2] = (floor(ix), floor(iy)) of every sample (indexing-parity test hook)."""
    _need_gpu(proj12, depth_hypos)
    b, d = depth_hypos.shape[:2]
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    out = torch.empty((b, d, h, w, 2), device=proj12.device, dtype=torch.int32)
    _abi("mdf_warp_corner_indices", (_f32c(proj12).data_ptr(), hyp.data_ptr(), pp, out.data_ptr(), b, d, h, w,
                                        _stream(out),))
    return out


def _src_array(srcs):
    arr = (ctypes.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    return arr


def warp_aggregate_vec(features, proj, depth_hypos, w_params, ngroups, channels_last=True):
    """Fused VectorAggregate.forward (eval).  features: list of V [B,C,h,w]; proj [n_src,B,12] device;
    w_params [G+4] device.  Returns cost with logical shape [B,G,D,h,w]; memory is NDHWC when
    channels_last (what the 3-D conv kernels consume) else NCDHW."""
    _need_gpu(*features, proj, depth_hypos, w_params)
    feas = [nhwc(f) for f in features]
    b, c, h, w = feas[0].shape
    d = depth_hypos.shape[1]
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    g = ngroups
    dev = feas[0].device
    if channels_last:
        mem = torch.empty((b, d, h, w, g), device=dev, dtype=torch.float32)
        cost = mem.permute(0, 4, 1, 2, 3)
    else:
        mem = cost = torch.empty((b, g, d, h, w), device=dev, dtype=torch.float32)
    srcs = feas[1:]
    _abi("mdf_warp_aggregate_vec_fwd", (feas[0].data_ptr(), _src_array(srcs), FEA_NHWC, _f32c(proj).data_ptr(),
                                           hyp.data_ptr(), pp, _f32c(w_params).data_ptr(), mem.data_ptr(),
                                           VOL_NDHWC if channels_last else VOL_NCDHW, b, c, g, d, h, w, len(srcs),
                                           _stream(mem),), tag=f"C{c}G{g}D{d} {w}x{h} V{len(feas)}",
         work={"bytes": 4.0 * b * (len(feas) * c * h * w + hyp.numel() / b + g * d * h * w),  # feats once +
               "bound": "hbm"})                                                            # hypos once + cost once
    return cost


def warp_aggregate_pairdiff(diffs, proj, depth_hypos, w_params, channels_last=True):
    """warp_aggregate_vec fed pair-difference maps: diffs = list of V [B,G,h,w] with d[:, g] = f[:, 2g+1] - f[:, 2g] (what the
    built-in feature pyramid's difference heads emit).  Same arguments, result layout and sample positions; the cost differs from
    warp_aggregate_vec(features) by the rounding of the bilinear blend only (one blend of a difference instead of the difference
    of two blends)."""
    _need_gpu(*diffs, proj, depth_hypos, w_params)
    feas = [nhwc(f) for f in diffs]
    b, g, h, w = feas[0].shape
    if w_params.numel() != g + 4:
        raise ValueError(f"w_params has {w_params.numel()} entries, expected G + 4 = {g + 4}: are these pair-difference maps?")
    d = depth_hypos.shape[1]
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    dev = feas[0].device
    if channels_last:
        mem = torch.empty((b, d, h, w, g), device=dev, dtype=torch.float32)
        cost = mem.permute(0, 4, 1, 2, 3)
    else:
        mem = cost = torch.empty((b, g, d, h, w), device=dev, dtype=torch.float32)
    srcs = feas[1:]
    _abi("mdf_warp_aggregate_pairdiff_fwd", (feas[0].data_ptr(), _src_array(srcs), FEA_NHWC, _f32c(proj).data_ptr(),
                                             hyp.data_ptr(), pp, _f32c(w_params).data_ptr(), mem.data_ptr(),
                                             VOL_NDHWC if channels_last else VOL_NCDHW, b, g, d, h, w, len(srcs),
                                             _stream(mem),), tag=f"G{g}D{d} {w}x{h} V{len(feas)}",
         work={"bytes": 4.0 * b * (len(feas) * g * h * w + hyp.numel() / b + g * d * h * w),  # difference maps once + hypos once
               "bound": "hbm"})                                                            # + cost once
    return cost


def warp_aggregate_var(features, proj, depth_hypos, channels_last=False):
    """Fused homo_aggregate_by_variance (homoaggregate.py:49-69) -> [B,C,D,h,w]."""
    _need_gpu(*features, proj, depth_hypos)
    feas = [nhwc(f) for f in features]
    b, c, h, w = feas[0].shape
    d = depth_hypos.shape[1]
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    dev = feas[0].device
    if channels_last:
        mem = torch.empty((b, d, h, w, c), device=dev, dtype=torch.float32)
        cost = mem.permute(0, 4, 1, 2, 3)
    else:
        mem = cost = torch.empty((b, c, d, h, w), device=dev, dtype=torch.float32)
    srcs = feas[1:]
    _abi("mdf_warp_aggregate_var_fwd", (feas[0].data_ptr(), _src_array(srcs), FEA_NHWC, _f32c(proj).data_ptr(),
                                           hyp.data_ptr(), pp, mem.data_ptr(),
                                           VOL_NDHWC if channels_last else VOL_NCDHW, b, c, d, h, w, len(srcs),
                                           _stream(mem),))
    return cost


def fold_view_weight(p, ngroups, prefix="depth_weight."):
    """depth_weight head parameters -> device tensor [G+4] = (conv weight[G], alpha, beta, w2, b2) with
    BatchNorm3d(1) folded as ATen does in eval (alpha = gamma/sqrt(var+eps), beta = bias - mean*alpha)."""
    cw = p[prefix + "0.conv.weight"].reshape(ngroups).float()
    invstd = 1.0 / torch.sqrt(p[prefix + "0.bn.running_var"].float() + 1e-5)
    alpha = p[prefix + "0.bn.weight"].float() * invstd
    beta = p[prefix + "0.bn.bias"].float() - p[prefix + "0.bn.running_mean"].float() * alpha
    return torch.cat([cw, alpha.reshape(1), beta.reshape(1), p[prefix + "1.weight"].reshape(1).float(),
                      p[prefix + "1.bias"].reshape(1).float()]).contiguous()


# --------------------------------------------------------------------------- regression heads
def depth_regress(prob, depth_hypos):
    """net/unit/regress.py:5-7."""
    _need_gpu(prob, depth_hypos)
    b, d, h, w = prob.shape
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    prob = _f32c(prob)
    out = torch.empty((b, h, w), device=prob.device, dtype=torch.float32)
    _abi("mdf_depth_regress_fwd", (prob.data_ptr(), hyp.data_ptr(), pp, out.data_ptr(), b, d, h, w, _stream(out),))
    return out


def confidence(prob, return_index=False):
    """net/unit/regress.py:9-25 (n=4, pad=(1,2))."""
    _need_gpu(prob)
    b, d, h, w = prob.shape
    prob = _f32c(prob)
    out = torch.empty((b, h, w), device=prob.device, dtype=torch.float32)
    idx = torch.empty((b, h, w), device=prob.device, dtype=torch.int64) if return_index else None
    _abi("mdf_confidence_fwd", (prob.data_ptr(), out.data_ptr(), idx.data_ptr() if return_index else None,
                                   b, d, h, w, _stream(out),))
    return (out, idx) if return_index else out


def confidence_up2(prob):
    """regress.py:9-25 followed by F.interpolate(scale_factor=2, mode="nearest") (core.py:75-76) as one launch -> [B,2h,2w]."""
    _need_gpu(prob)
    b, d, h, w = prob.shape
    prob = _f32c(prob)
    out = torch.empty((b, 2 * h, 2 * w), device=prob.device, dtype=torch.float32)
    _abi("mdf_confidence_up2_fwd", (prob.data_ptr(), out.data_ptr(), b, d, h, w, _stream(out),))
    return out


def confidence_cascade(prob, last=None, n=4, pad_front=1, weights=(0.8, 0.2), up2=False):
    """regress.py:9-25 with last_confidence: weights[0] * bicubic_x2(last) + weights[1] * sum prob[idx-pad_front .. +n-1], one launch.
    prob [B,D,H,W]; last [B,H/2,W/2] or None (then the plain window sum); up2: the nearest x2 of core.py:76 folded in -> [B,2H,2W]."""
    _need_gpu(prob, last)
    b, d, h, w = prob.shape
    if last is not None and tuple(last.shape) != (b, h // 2, w // 2):
        raise ValueError(f"last confidence of shape {tuple(last.shape)}: expected {(b, h // 2, w // 2)} for a volume {tuple(prob.shape)}")
    prob = _f32c(prob)
    last_c = None if last is None else _f32c(last)      # (a local: a converted copy must outlive the launch's enqueue)
    out = torch.empty((b, 2 * h, 2 * w) if up2 else (b, h, w), device=prob.device, dtype=torch.float32)
    _abi("mdf_confidence_cascade_fwd", (prob.data_ptr(), None if last_c is None else last_c.data_ptr(), float(weights[0]), float(weights[1]),
                                        int(n), int(pad_front), int(bool(up2)), out.data_ptr(), b, d, h, w, _stream(out),))
    return out


def range_affine(x, lo, span, mode):
    """mode 0: (x - lo[b]) / span[b]; mode 1: lo[b] + x * span[b]   (refine.py:29,44), x [B,...]."""
    _need_gpu(x, lo, span)
    x = _f32c(x)
    y = torch.empty_like(x)
    b = x.shape[0]
    lo_c, span_c = _f32c(lo), _f32c(span)      # (locals: a converted copy must outlive the launch's enqueue)
    _abi("mdf_range_affine_fwd", (x.data_ptr(), lo_c.data_ptr(), span_c.data_ptr(), mode, y.data_ptr(), b, x.numel() // b, _stream(y),))
    return y


METRIC_BINS = 32                     # confidence bins of a depth-metrics table (rows 1..32; row 0 is the whole map)
METRIC_COLUMNS = ("n", "n_nonfinite", "sum_e", "under0", "under1", "under2", "under3", "covered", "sum_width")


class MetricView:
    """Named columns of a depth-metrics table [..., 1 + METRIC_BINS, 9] (views, no copies): n, n_nonfinite, sum_e, covered,
    sum_width are [..., 33]; under is [..., 33, 4].  Row 0 is the whole map, rows 1..32 the confidence bins."""

    def __init__(self, table):
        self.table = table
        for i, name in enumerate(METRIC_COLUMNS):
            if not name.startswith("under"):
                setattr(self, name, table[..., i])
        self.under = table[..., 3:7]


def depth_metrics(maps, floor, thresholds):
    """Validation metrics of up to 8 depth maps of different sizes in one reduction launch and one finalize launch
    (include/mdfnet_hip.h: mdf_depth_metrics_*).  maps: list of dicts with "est", "gt" [B,h,w] and optionally "hypos" ([B,D,h,w] or
    [B,D,1,1]: the hypotheses a stage was given, whose first and last plane are the interval the cascade can recover) and "conf"
    [B,h,w].  floor [B]: depth_min per item, float64 or float32 (any stride: depth_range[:, 0] is taken as it is).  thresholds
    [B,T] (or [T], shared by the items), 1 <= T <= 4, absolute.  -> (table, view): table float64 [M, 33, 9] on the device, view
    a MetricView of it.  Nothing synchronises; the workspace is a torch allocation.  Run-to-run bit-identical."""
    if not 1 <= len(maps) <= 8:
        raise ValueError(f"depth_metrics takes 1 to 8 maps, got {len(maps)}")
    first = maps[0]["est"]
    thr = thresholds if isinstance(thresholds, torch.Tensor) else torch.as_tensor(thresholds, dtype=torch.float32, device=first.device)
    _need_gpu(floor, thr, *[t for m in maps for t in (m["est"], m["gt"], m.get("hypos"), m.get("conf"))])
    b = first.shape[0]
    thr = _f32c(thr)
    if thr.dim() == 1:
        thr = thr.reshape(1, -1).expand(b, -1).contiguous()
    if thr.dim() != 2 or thr.shape[0] != b or not 1 <= thr.shape[1] <= 4:
        raise ValueError(f"thresholds of shape {tuple(thr.shape)}: expected [{b}, 1..4]")
    fl = floor.detach()
    if fl.dtype not in (torch.float32, torch.float64):
        fl = fl.float()
    if fl.dim() == 0:
        fl = fl.reshape(1)
    if fl.dim() != 1 or fl.shape[0] not in (1, b):
        raise ValueError(f"floor of shape {tuple(fl.shape)}: expected [{b}]")
    fstride = fl.stride(0) if fl.shape[0] == b else 0
    nm = len(maps)
    keep, est, gt, hyp, hd, hpp, conf, per = [], [], [], [], [], [], [], []
    conf_mask = 0
    for i, m in enumerate(maps):
        e, g = _f32c(m["est"].detach()), _f32c(m["gt"].detach())
        if e.dim() != 3 or e.shape != g.shape or e.shape[0] != b:
            raise ValueError(f"map {i}: est {tuple(e.shape)} and gt {tuple(g.shape)} must both be [{b}, h, w]")
        h, w = e.shape[1:]
        hy, cf = m.get("hypos"), m.get("conf")
        if hy is not None:
            if hy.dim() != 4 or hy.shape[0] != b:
                raise ValueError(f"map {i}: hypos of shape {tuple(hy.shape)}: expected [{b}, D, h, w] or [{b}, D, 1, 1]")
            hy, pp = _hypos_arg(hy.detach(), h, w)
        if cf is not None:
            cf = _f32c(cf.detach())
            if cf.shape != e.shape:
                raise ValueError(f"map {i}: conf of shape {tuple(cf.shape)}: expected {tuple(e.shape)}")
            conf_mask |= 1 << i
        keep.append((e, g, hy, cf))          # (converted copies must outlive the launch's enqueue)
        est.append(e.data_ptr()); gt.append(g.data_ptr())
        hyp.append(None if hy is None else hy.data_ptr()); hd.append(0 if hy is None else hy.shape[1]); hpp.append(0 if hy is None else pp)
        conf.append(None if cf is None else cf.data_ptr())
        per.append(h * w)
    pb = (ctypes.c_int64 * nm)(*per)
    nbytes = lib().mdf_depth_metrics_workspace(pb, nm, b)
    if nbytes < 0:
        check(int(nbytes), "mdf_depth_metrics_workspace")
    dev = first.device
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    table = torch.empty((nm, 1 + METRIC_BINS, len(METRIC_COLUMNS)), device=dev, dtype=torch.float64)
    st = _stream(table)
    arr = lambda vals: (ctypes.c_void_p * nm)(*vals)
    nbytes_in = 4.0 * b * sum(p * (2 + (c is not None) + 2 * (hy is not None and pp_)) for p, c, hy, pp_ in zip(per, conf, hyp, hpp))
    _abi("mdf_depth_metrics_reduce_multi", (arr(est), arr(gt), arr(hyp), (ctypes.c_int * nm)(*hd), (ctypes.c_int * nm)(*hpp), arr(conf), pb, nm,
                                            fl.data_ptr(), int(fl.dtype == torch.float64), fstride, thr.data_ptr(), thr.shape[1], b,
                                            ws.data_ptr(), nbytes, st), tag=f"depth metrics {nm} maps",
         work={"bytes": nbytes_in + nbytes, "bound": "hbm"})
    _abi("mdf_depth_metrics_finalize", (ws.data_ptr(), nbytes, pb, nm, b, conf_mask, table.data_ptr(), st))
    del keep
    return table, MetricView(table)


_fit_row_cache = {}


def gauss1_fit_row(depth_hypos):
    """HOST: row 0 of (X^T X)^-1 X^T for hypotheses [B,D,1,1] shared by every pixel.

    cond(X^T X) ~ 1e14 in fp32, so the *bits* of this row are the reference's behaviour and they
    depend on which BLAS path torch takes, i.e. on the operand shapes/strides.  The row is therefore produced by
    replaying depthhypos.py:191-208 verbatim (repeat -> stack -> permute -> matmul -> inverse -> matmul) on a
    2x2-pixel replica: verified bit-identical to the per-pixel matrices of any larger image, for any batch size
    (a 1x1 replica is NOT: degenerate strides take another path).  Cached by value: the row only depends on the
    hypotheses, i.e. on (depth_min, depth_max, D), which is constant for a whole dataset.  -> [B,D] CPU float32."""
    pinned = recorded("fit_row")
    if pinned is not None:
        return pinned
    hyp = depth_hypos.detach().to("cpu", torch.float32)
    b, d = hyp.shape[:2]
    key = (b, d, hyp.numpy().tobytes())
    row = _fit_row_cache.get(key)
    if row is None:
        with _single_thread():
            rep = hyp.reshape(b, d, 1, 1).repeat(1, 1, 2, 2)
            x = torch.stack([rep ** 2, rep, torch.ones_like(rep)], dim=-1).permute(0, 2, 3, 1, 4)
            xt = x.transpose(-1, -2)
            row = torch.matmul(torch.inverse(torch.matmul(xt, x)), xt)[:, 0, 0, 0, :].contiguous()
        if len(_fit_row_cache) > 256:
            _fit_row_cache.clear()
        _fit_row_cache[key] = row
    return row


def hypos_fit(mode, prob, depth, depth_hypos, fit_row=None):
    """Step 1 of HyposByFit: per-pixel curve parameter s [B,h,w].
      mode 1  gauss1, hypotheses [B,D,1,1] only: needs `fit_row` (gauss1_fit_row); mirrors the reference's fp32 bits
      mode 2  laplace: needs `depth`; hypotheses [B,D,1,1] or [B,D,h,w]
      mode 3  gauss0: needs `depth`; hypotheses of either form
      mode 4  gauss1, hypotheses of either form: needs neither `depth` nor `fit_row`
    Modes 3 and 4 are centred fits held to the reference's code in float64 (its fp32 is noise for per-pixel hypotheses); a pixel
    whose fit is not determined (fewer than 2 distinct (x - depth)^2, fewer than 3 distinct hypotheses) gets NaN."""
    _need_gpu(prob)
    b, d, h, w = prob.shape
    prob = _f32c(prob)
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    out = torch.empty((b, h, w), device=prob.device, dtype=torch.float32)
    # (locals: a converted copy freed before the enqueue hands its block to the next conversion, which then overwrites it)
    depth_c = None if depth is None else _f32c(depth)
    row_c = None if fit_row is None else _f32c(fit_row)
    _abi("mdf_hypos_fit_fwd", (mode, prob.data_ptr(), None if depth_c is None else depth_c.data_ptr(),
                                  hyp.data_ptr(), pp, None if row_c is None else row_c.data_ptr(),
                                  out.data_ptr(), b, d, h, w, _stream(out),))
    return out


def hypos_from_fit(mode, s, depth, depth_range_f32, log_thresh, ndepths, upsample=True):
    """Step 2 of HyposByFit (depthhypos.py:49-76) -> [B,D,2h,2w] (or [B,D,h,w])."""
    _need_gpu(s, depth, depth_range_f32)
    b, h, w = s.shape
    ho, wo = (2 * h, 2 * w) if upsample else (h, w)
    out = torch.empty((b, ndepths, ho, wo), device=s.device, dtype=torch.float32)
    s_c, depth_c, range_c = _f32c(s), _f32c(depth), _f32c(depth_range_f32)      # (locals: as in hypos_fit)
    _abi("mdf_hypos_from_fit_fwd", (mode, s_c.data_ptr(), depth_c.data_ptr(),
                                       range_c.data_ptr(), ctypes.c_float(log_thresh), out.data_ptr(),
                                       b, ndepths, h, w, int(upsample), _stream(out),))
    return out


def atv_spread(prob, depth, depth_hypos, scale=1.5):
    """Step 1 of the "atv" curve: e = scale * sqrt(sum_d prob_d (hypos_d - depth)^2) [B,h,w], UCS-Net's exp_variance (the second
    argument of the reference's atv_hypos, depthhypos.py:218).  Hypotheses [B,D,1,1] or [B,D,h,w]; scale finite and > 0."""
    _need_gpu(prob, depth)
    b, d, h, w = prob.shape
    if tuple(depth.shape) != (b, h, w) or tuple(depth_hypos.shape[:2]) != (b, d):
        raise ValueError(f"atv_spread: prob {tuple(prob.shape)} needs depth [B,h,w] and hypos [B,D,..], got {tuple(depth.shape)}, {tuple(depth_hypos.shape)}")
    prob_c, depth_c = _f32c(prob), _f32c(depth)      # (locals: as in hypos_fit)
    hyp, pp = _hypos_arg(depth_hypos, h, w)
    out = torch.empty((b, h, w), device=prob.device, dtype=torch.float32)
    _abi("mdf_atv_spread_fwd", (prob_c.data_ptr(), depth_c.data_ptr(), hyp.data_ptr(), pp, ctypes.c_float(scale), out.data_ptr(),
                                b, d, h, w, _stream(out),))
    return out


def atv_hypos(spread, depth, ndepths, upsample=True):
    """Step 2 of the "atv" curve (depthhypos.py:239-253) -> [B,D,2h,2w] (or [B,D,h,w]).  Not clamped to the depth range."""
    _need_gpu(spread, depth)
    b, h, w = spread.shape
    if depth.shape != spread.shape:
        raise ValueError(f"atv_hypos: spread {tuple(spread.shape)} and depth {tuple(depth.shape)} must have one shape")
    ho, wo = (2 * h, 2 * w) if upsample else (h, w)
    out = torch.empty((b, max(int(ndepths), 0), ho, wo), device=spread.device, dtype=torch.float32)
    spread_c, depth_c = _f32c(spread), _f32c(depth)
    _abi("mdf_atv_hypos_fwd", (spread_c.data_ptr(), depth_c.data_ptr(), out.data_ptr(), b, ndepths, h, w, int(upsample), _stream(out),))
    return out


# --------------------------------------------------------------------------- 3-D conv layers (NDHWC)
def to_ndhwc(t):
    """logical [B,C,D,H,W] -> contiguous [B,D,H,W,C] tensor (no copy when the memory already is)."""
    cl = t.permute(0, 2, 3, 4, 1)
    return cl if (cl.is_contiguous() and cl.dtype == torch.float32) else cl.float().contiguous()


def from_ndhwc(cl):
    """[B,D,H,W,C] memory -> logical [B,C,D,H,W] view."""
    return cl.permute(0, 4, 1, 2, 3)


def pack_conv3d_weight(w, transposed=False):
    """torch Conv3d [Cout,Cin,3,3,3] / ConvTranspose3d [Cin,Cout,3,3,3] weight -> MFMA fragment order."""
    _need_gpu(w)
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    n = lib().mdf_conv3d_packed_size(cin, cout)
    out = torch.empty((n,), device=w.device, dtype=torch.float32)
    _abi("mdf_conv3d_pack_weights", (_f32c(w.detach()).data_ptr(), out.data_ptr(), cin, cout, int(transposed),
                                        _stream(out),))
    return out


def conv3d_ndhwc(x, wpack, cin, cout, stride=1, transposed=False, alpha=None, beta=None, relu=False, res=None):
    """y = [res +] [relu](conv(x)*alpha + beta).  x [B,D,H,W,Cin] contiguous -> y [B,Do,Ho,Wo,Cout].  stride: 1 or 2 on every
    axis, or the tuple (1,2,2) -- the depth-preserving sampling layers (mdf_conv3d_hw2_fwd): Do = D, Ho, Wo as for stride 2."""
    if not isinstance(stride, int):
        if tuple(stride) != (1, 2, 2):
            raise ValueError(f"conv3d_ndhwc: stride is 1, 2 or the tuple (1,2,2), got {tuple(stride)}")
        return _conv3d_hw2(x, wpack, cin, cout, transposed, alpha, beta, relu, res)
    _need_gpu(x, wpack)
    b, d, h, w, c = x.shape
    assert c == cin and x.is_contiguous()
    if transposed:
        do, ho, wo = 2 * d, 2 * h, 2 * w
    elif stride == 2:
        do, ho, wo = (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    else:
        do, ho, wo = d, h, w
    y = torch.empty((b, do, ho, wo, cout), device=x.device, dtype=torch.float32)
    if res is not None:
        assert res.shape == y.shape and res.is_contiguous()
    _abi("mdf_conv3d_fwd", (x.data_ptr(), wpack.data_ptr(), None if alpha is None else alpha.data_ptr(),
                               None if beta is None else beta.data_ptr(), None if res is None else res.data_ptr(),
                               y.data_ptr(), b, d, h, w, cin, cout, stride, int(transposed), int(relu), _stream(y),),
         tag=f"{cin}->{cout} {'T' if transposed else 's%d' % stride} {d}x{h}x{w}",
         work={"flops": 2.0 * 27 * cin * cout * b * (d * h * w if transposed else do * ho * wo),
               "bytes": 4.0 * (x.numel() + y.numel() * (2 if res is not None else 1)), "bound": "mfma"})
    return y


def _conv3d_hw2(x, wpack, cin, cout, transposed, alpha, beta, relu, res):
    """conv3d_ndhwc with stride (1,2,2): Conv3d(k3, (1,2,2), pad 1), or ConvTranspose3d(k3, (1,2,2), pad 1, output_padding (0,1,1)),
    on the weight set pack_conv3d_weight(w, transposed) made (mdf_conv3d_hw2_fwd)."""
    _need_gpu(x, wpack)
    b, d, h, w, c = x.shape
    assert c == cin and x.is_contiguous()
    ho, wo = (2 * h, 2 * w) if transposed else ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    y = torch.empty((b, d, ho, wo, cout), device=x.device, dtype=torch.float32)
    if res is not None:
        assert res.shape == y.shape and res.is_contiguous()
    _abi("mdf_conv3d_hw2_fwd", (x.data_ptr(), wpack.data_ptr(), None if alpha is None else alpha.data_ptr(),
                                None if beta is None else beta.data_ptr(), None if res is None else res.data_ptr(),
                                y.data_ptr(), b, d, h, w, cin, cout, int(transposed), int(relu), _stream(y),),
         tag=f"{cin}->{cout} {'T' if transposed else 's'}122 {d}x{h}x{w}",
         work={"flops": conv3d_hw2_flops(b, d, h, w, cin, cout, transposed),
               "bytes": 4.0 * (x.numel() + y.numel() * (2 if res is not None else 1)), "bound": "mfma"})
    return y


def conv3d_hw2_flops(b, d, h, w, cin, cout, transposed):
    """Multiply-adds x 2 the (1,2,2) layer needs on a [b,d,h,w] input: 27 taps per output voxel (down); per INPUT voxel the three depth
    taps of all nine (kh, kw) pairs (up: every weight meets every input voxel once, borders aside)."""
    vox = b * d * h * w if transposed else b * d * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
    return 2.0 * 27 * cin * cout * vox


STAT_SLICES = 16      # copies of the epilogue sums a conv launch spreads its blocks over (the BatchNorm kernels add them up)


def conv3d_train(x, wpack, cin, cout, stride, transposed, res, stat_mode, stat_out, stat_y=None, stat_aux=None):
    """Training: y = [res +] conv(x) raw, with per-channel sums of y accumulated into `stat_out` [2*cout] fp64 by the conv's
    epilogue (mdf_conv3d_train_fwd).  stat_mode 1: (sum y, sum y^2); 2: y is dz of the layer whose raw output is stat_y and whose
    BatchNorm constants are stat_aux -> (sum dr, sum dr*xhat)."""
    _need_gpu(x, wpack, stat_out)
    b, d, h, w, c = x.shape
    assert c == cin and x.is_contiguous()
    if transposed:
        do, ho, wo = 2 * d, 2 * h, 2 * w
    elif stride == 2:
        do, ho, wo = (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    else:
        do, ho, wo = d, h, w
    y = torch.empty((b, do, ho, wo, cout), device=x.device, dtype=torch.float32)
    if res is not None:
        assert res.shape == y.shape and res.is_contiguous()
    if stat_mode == 2:
        assert stat_y.shape == y.shape and stat_y.is_contiguous() and stat_aux.numel() == 4 * cout
    nslices = stat_out.numel() // (2 * cout)
    assert stat_out.numel() == nslices * 2 * cout and stat_out.dtype == torch.float64
    _abi("mdf_conv3d_train_fwd", (x.data_ptr(), wpack.data_ptr(), None if res is None else res.data_ptr(), y.data_ptr(), b, d, h, w, cin, cout,
                                  stride, int(transposed), stat_mode, None if stat_y is None else stat_y.data_ptr(),
                                  None if stat_aux is None else stat_aux.data_ptr(), stat_out.data_ptr(), nslices, _stream(y)),
         tag=f"{cin}->{cout} {'T' if transposed else 's%d' % stride} {d}x{h}x{w} +sums{stat_mode}",
         work={"flops": 2.0 * 27 * cin * cout * b * (d * h * w if transposed else do * ho * wo),
               "bytes": 4.0 * (x.numel() + y.numel() * (1 + (res is not None) + (stat_mode == 2))), "bound": "mfma"})
    return y


def conv2d_train(x, wpack, cin, cout, ksize, stride, planar_in, stat_mode, stat_out, ngroups, stat_y=None, stat_aux=None):
    """2-D counterpart (mdf_conv2d_train_fwd): `ngroups` consecutive sets of images are separate BatchNorm groups."""
    _need_gpu(x, wpack, stat_out)
    if planar_in:
        b, c, h, w = x.shape
    else:
        b, h, w, c = x.shape
    assert c == cin and x.is_contiguous() and b % ngroups == 0
    pad = (ksize - 1) // 2
    ho, wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    y = torch.empty((b, ho, wo, cout), device=x.device, dtype=torch.float32)
    if stat_mode == 2:
        assert stat_y.shape == y.shape and stat_y.is_contiguous() and stat_aux.numel() == ngroups * 4 * cout
    nslices = stat_out.numel() // (ngroups * 2 * cout)
    assert stat_out.numel() == nslices * ngroups * 2 * cout and stat_out.dtype == torch.float64
    _abi("mdf_conv2d_train_fwd", (x.data_ptr(), wpack.data_ptr(), y.data_ptr(), b, h, w, cin, cout, ksize, stride, int(planar_in), stat_mode,
                                  None if stat_y is None else stat_y.data_ptr(), None if stat_aux is None else stat_aux.data_ptr(),
                                  stat_out.data_ptr(), nslices, ngroups, _stream(y)),
         tag=f"{cin}->{cout} k{ksize}s{stride} {h}x{w}x{b} +sums{stat_mode}",
         work={"flops": 2.0 * ksize * ksize * cin * cout * b * ho * wo, "bytes": 4.0 * (x.numel() + y.numel() * (1 + (stat_mode == 2))),
               "bound": "mfma"})
    return y


def pack_prob_weight(weight):
    """[1,Cin,3,3,3] `prob` conv weight -> packed 2-D weight whose output channels are the three kd slices (+ one zero
    channel), for the partial-sum route of prob_head."""
    w = weight.detach().float()
    w2 = torch.zeros((4, w.shape[1], 3, 3), device=w.device, dtype=torch.float32)
    w2[:3] = w[0].permute(1, 0, 2, 3)          # [kd, cin, kh, kw]
    return pack_conv2d_weight(w2)


# The one-launch partial-sum route is parallel over pixels only (one block per 4 x 64 tile): used once that fills the chip.
PROB_FUSED = os.environ.get("MDF_PROB_FUSED", "1") != "0"              # dev A/B
PROB_FUSED_MIN_TILES = int(os.environ.get("MDF_PROB_FUSED_MIN_TILES", "400"))


def prob_head(x, weight, depth_hypos=None, direct=False, wpack=None):
    """Conv3d(Cin->1,k3,p1) + softmax over D [+ soft-argmin].  x [B,D,h,w,Cin] -> prob [B,D,h,w] (, depth).
    Default route: per-plane partial sums on the MFMA conv kernel + a light combine/softmax kernel (`wpack` = cached
    pack_prob_weight(weight), packed here when absent) -- as ONE launch that keeps the partials in registers when the map is
    large enough to fill the chip with one block per 4 x 64 pixel tile, otherwise as two; `direct` (or a shape the partial-sum
    kernels are not built for) uses the self-contained direct kernel."""
    _need_gpu(x, weight)
    b, d, h, w, c = x.shape
    prob = torch.empty((b, d, h, w), device=x.device, dtype=torch.float32)
    depth, hyp, pp = None, None, 0
    if depth_hypos is not None:
        hyp, pp = _hypos_arg(depth_hypos, h, w)
        depth = torch.empty((b, h, w), device=x.device, dtype=torch.float32)
    fused_lds = 2 * c * 398 * 4 + d * 1024          # bytes: two plane tiles + the logits of the block's 256 pixels
    if (not direct and c in (8, 16) and x.is_contiguous() and PROB_FUSED and fused_lds <= 160 * 1024
            and b * ((h + 3) // 4) * ((w + 63) // 64) >= PROB_FUSED_MIN_TILES):
        wp = pack_prob_weight(weight) if wpack is None else wpack
        _abi("mdf_prob_fused_fwd", (x.data_ptr(), wp.data_ptr(), None if hyp is None else hyp.data_ptr(), pp, prob.data_ptr(),
                                    None if depth is None else depth.data_ptr(), b, d, h, w, c, _stream(prob),),
             tag=f"{c}->1 {d}x{h}x{w}", work={"flops": 2.0 * 27 * c * b * d * h * w,
                                              "bytes": 4.0 * (x.numel() + prob.numel()), "bound": "hbm"})
        return prob if depth is None else (prob, depth)
    if not direct and c in (8, 16) and d <= 96 and x.is_contiguous():
        part = conv2d_nhwc(x.view(b * d, h, w, c), pack_prob_weight(weight) if wpack is None else wpack, c, 4, 3, 1,
                           useful_cout=3)
        _abi("mdf_prob_from_partials_fwd", (part.data_ptr(), None if hyp is None else hyp.data_ptr(), pp, prob.data_ptr(),
                                            None if depth is None else depth.data_ptr(), b, d, h, w, _stream(prob),),
             tag=f"partials->prob {d}x{h}x{w}", work={"bytes": 4.0 * (part.numel() + prob.numel()), "bound": "hbm"})
        return prob if depth is None else (prob, depth)
    _abi("mdf_prob_softmax_regress_fwd", (x.data_ptr(), _f32c(weight.detach()).data_ptr(),
                                             None if hyp is None else hyp.data_ptr(), pp, prob.data_ptr(),
                                             None if depth is None else depth.data_ptr(), b, d, h, w, c, _stream(prob),),
         tag=f"{c}->1 {d}x{h}x{w}", work={"flops": 2.0 * 27 * c * b * d * h * w,
                                          "bytes": 4.0 * (x.numel() + prob.numel()), "bound": "hbm"})
    return prob if depth is None else (prob, depth)


def refine_tail(x, w1pack, w2, lo=None, span=None):
    """[lo +] Conv2d(8,1,k3)(PixelShuffle(2)(Conv2d(8,32,k3)(x))) [* span] in one launch.  x [B,h,w,8] NHWC; w1pack =
    pack_conv2d_weight(shuffle2_rows(weight)); w2 [1,8,3,3]; lo, span [B] -> [B,2h,2w]."""
    _need_gpu(x, w1pack, w2)
    b, h, w, c = x.shape
    assert c == 8 and x.is_contiguous() and tuple(w2.shape) == (1, 8, 3, 3)
    y = torch.empty((b, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
    w2_c, lo_c, span_c = _f32c(w2.detach()), (None if lo is None else _f32c(lo)), (None if span is None else _f32c(span))
    _abi("mdf_refine_tail_fwd", (x.data_ptr(), w1pack.data_ptr(), w2_c.data_ptr(), None if lo_c is None else lo_c.data_ptr(),
                                 None if span_c is None else span_c.data_ptr(), y.data_ptr(), b, h, w, _stream(y),),
         tag=f"8->32->1 {h}x{w}x{b}", work={"flops": 2.0 * 72 * (32 + 4) * b * h * w, "bytes": 4.0 * (x.numel() + y.numel()), "bound": "mfma"})
    return y


def fold_bn(bn_weight, bn_bias, running_mean, running_var, eps=1e-5):
    """Eval BatchNorm as ATen folds it: alpha = gamma/sqrt(var+eps), beta = bias - mean*alpha."""
    invstd = 1.0 / torch.sqrt(running_var.float() + eps)
    alpha = (bn_weight.float() * invstd).contiguous()
    beta = (bn_bias.float() - running_mean.float() * alpha).contiguous()
    return alpha, beta


# --------------------------------------------------------------------------- 2-D conv layers (NHWC)
def pack_conv2d_weight(w):
    """torch Conv2d weight [Cout,Cin,k,k] -> MFMA fragment order (Cin 1 or 3 is zero-padded to 4)."""
    _need_gpu(w)
    cout, cin, k, _ = w.shape
    n = lib().mdf_conv_packed_size(cin, cout, k * k)
    out = torch.empty((n,), device=w.device, dtype=torch.float32)
    _abi("mdf_conv_pack_weights", (_f32c(w.detach()).data_ptr(), out.data_ptr(), cin, cout, k * k, _stream(out),))
    return out


def conv2d_nhwc(x, wpack, cin, cout, ksize, stride=1, alpha=None, beta=None, relu=False, res=None, res_scale=1.0,
                res_up=None, planar_in=False, useful_cout=None, pixel_shuffle2=False):
    """y = [res + res_scale *] ([up2(res_up) +] [relu](conv(x)*alpha + beta)).  x [B,H,W,Cin] contiguous
    (or planar [B,Cin,H,W] with planar_in=True, Cin < 4).  pixel_shuffle2: y = PixelShuffle(2)(conv(x)) as [B,2Ho,2Wo,Cout/4]
    (Cout = 32; wpack from pack_conv2d_weight(shuffle2_rows(weight)))."""
    _need_gpu(x, wpack)
    if planar_in:
        b, c, h, w = x.shape
    else:
        b, h, w, c = x.shape
    assert c == cin and x.is_contiguous()
    pad = (ksize - 1) // 2
    ho, wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    y = torch.empty((b, 2 * ho, 2 * wo, cout // 4) if pixel_shuffle2 else (b, ho, wo, cout), device=x.device, dtype=torch.float32)
    _abi("mdf_conv2d_fwd", (x.data_ptr(), wpack.data_ptr(), None if alpha is None else alpha.data_ptr(),
                            None if beta is None else beta.data_ptr(), None if res is None else res.data_ptr(),
                            ctypes.c_float(res_scale), None if res_up is None else res_up.data_ptr(), y.data_ptr(),
                            b, h, w, cin, cout, ksize, stride, int(relu), int(planar_in), int(pixel_shuffle2), _stream(y),),
         tag=f"{cin}->{cout} k{ksize}s{stride} {h}x{w}x{b}",
         work={"flops": 2.0 * ksize * ksize * cin * (useful_cout or cout) * b * ho * wo, "bytes": 4.0 * (x.numel() + y.numel()),
               "bound": "mfma"})
    return y


def conv2d_pair_planar(x, w1pack, a1, b1, w2pack, a2, b2):
    """relu(bn(conv3x3(relu(bn(conv3x3(x)))))) for the 3 -> 8 -> 8 head of the feature pyramid as ONE launch (conv_pair.hip).
    x planar [N,3,H,W] -> [N,H,W,8] NHWC.  Bit-identical to two conv2d_nhwc launches."""
    _need_gpu(x, w1pack, w2pack)
    n, c, h, w = x.shape
    assert c == 3 and x.is_contiguous() and x.dtype == torch.float32
    y = torch.empty((n, h, w, 8), device=x.device, dtype=torch.float32)
    _abi("mdf_conv2d_pair_fwd", (x.data_ptr(), w1pack.data_ptr(), a1.data_ptr(), b1.data_ptr(), w2pack.data_ptr(), a2.data_ptr(), b2.data_ptr(),
                                 y.data_ptr(), n, h, w, _stream(y)), tag=f"3->8->8 k3 {h}x{w}x{n}",
         work={"flops": 2.0 * 9 * (3 * 8 + 8 * 8) * n * h * w, "bytes": 4.0 * (x.numel() + y.numel()), "bound": "mfma"})
    return y


def conv1x1_heads(x, heads, res_ups):
    """Several bias-only 1x1 heads over ONE NHWC input in one launch (conv1x1.hip: conv1x1_heads_kernel).  heads: list of
    (wpack, bias or None, cin, cout); res_ups: per head a [B,H/2,W/2,cout] tensor (bilinear x2 upsample-add) or None.
    -> list of [B,H,W,cout].  Every output is bit-identical to conv2d_nhwc(x, wpack, cin, cout, 1, 1, None, bias, False, None, 1.0, res_up)."""
    _need_gpu(x)
    b, h, w, cin = x.shape
    assert x.is_contiguous() and all(hd[2] == cin for hd in heads)
    n = len(heads)
    ys = [torch.empty((b, h, w, hd[3]), device=x.device, dtype=torch.float32) for hd in heads]
    ptr = lambda t: None if t is None else t.data_ptr()
    wp = (ctypes.c_void_p * n)(*[hd[0].data_ptr() for hd in heads])
    bs = (ctypes.c_void_p * n)(*[ptr(hd[1]) for hd in heads])
    ru = (ctypes.c_void_p * n)(*[ptr(r) for r in res_ups])
    yo = (ctypes.c_void_p * n)(*[y.data_ptr() for y in ys])
    co = (ctypes.c_int * n)(*[hd[3] for hd in heads])
    for r, hd in zip(res_ups, heads):
        assert r is None or (tuple(r.shape) == (b, h // 2, w // 2, hd[3]) and r.is_contiguous())
    cout = sum(hd[3] for hd in heads)
    _abi("mdf_conv1x1_heads_fwd", (x.data_ptr(), n, wp, bs, ru, yo, co, b, h, w, cin, _stream(x)),
         tag=f"{cin}->{'/'.join(str(hd[3]) for hd in heads)} k1s1 {h}x{w}x{b}",
         work={"flops": 2.0 * cin * cout * b * h * w, "bytes": 4.0 * (x.numel() + sum(y.numel() for y in ys)), "bound": "mfma"})
    return ys


def refine_head(depth, lo, span, weight):
    """conv0((depth - lo) / span): the range mapping and the refinement net's Conv2d(1, 8, k3) in one launch; depth [B,h,w] -> [B,h,w,8]."""
    _need_gpu(depth, weight)
    b, h, w = depth.shape
    assert tuple(weight.shape) == (8, 1, 3, 3)
    d, wt = _f32c(depth), _f32c(weight.detach())
    y = torch.empty((b, h, w, 8), device=depth.device, dtype=torch.float32)
    lo_c, span_c = (None if lo is None else _f32c(lo)), (None if span is None else _f32c(span))
    _abi("mdf_refine_head_fwd", (d.data_ptr(), None if lo_c is None else lo_c.data_ptr(), None if span_c is None else span_c.data_ptr(),
                                 wt.data_ptr(), y.data_ptr(), b, h, w, _stream(y)), tag=f"range + 1->8 k3 {h}x{w}x{b}",
         work={"bytes": 4.0 * (d.numel() + y.numel()), "bound": "hbm"})
    return y


def conv2d_res_pair(x, wa_pack, wb_pack, scale=0.1):
    """x + scale * conv3x3(relu(conv3x3(x))) for an 8-channel residual block as ONE launch (res_pair.hip); x [N,H,W,8] NHWC.
    Bit-identical to two conv2d_nhwc launches (relu=True; then res=x, res_scale=scale)."""
    _need_gpu(x, wa_pack, wb_pack)
    n, h, w, c = x.shape
    assert c == 8 and x.is_contiguous() and x.dtype == torch.float32
    y = torch.empty_like(x)
    _abi("mdf_conv2d_res_pair_fwd", (x.data_ptr(), wa_pack.data_ptr(), wb_pack.data_ptr(), ctypes.c_float(scale), y.data_ptr(), n, h, w, _stream(y)),
         tag=f"8->8->8 k3 res {h}x{w}x{n}", work={"flops": 2.0 * 9 * 2 * 8 * 8 * n * h * w, "bytes": 4.0 * (x.numel() + y.numel()), "bound": "mfma"})
    return y


def shuffle2_rows(weight):
    """Reorder the output channels of a Conv2d that feeds nn.PixelShuffle(2): torch channel oc*4 + sub -> row sub*Cq + oc
    (Cq = Cout/4), the order mdf_conv2d_fwd(pixel_shuffle2=1) expects."""
    co = weight.shape[0]
    return weight.detach().reshape(co // 4, 4, *weight.shape[1:]).transpose(0, 1).reshape(weight.shape).contiguous()


def to_nhwc(t):
    """logical [B,C,H,W] -> contiguous [B,H,W,C] (no copy when the memory is already channels_last)."""
    cl = t.permute(0, 2, 3, 1)
    return cl if (cl.is_contiguous() and cl.dtype == torch.float32) else cl.float().contiguous()


def from_nhwc(cl):
    return cl.permute(0, 3, 1, 2)


# --------------------------------------------------------------------------- N1: consistency filter / fusion
def consistency_mats(k_ref, e_ref, src_ks, src_es):
    """HOST: the six matrices per source view the fused kernel consumes, with the reference's own torch calls
    (dynamic_filter_gpu.py:205,210,226,229) on the CPU.  -> [n_src, 68] float32.
    The matrices are made row-major first, as the reference's own are (torch.from_numpy of the camera files): torch.inverse factorises
    a transposed-storage matrix along another path, whose result differs in the last bit."""
    def host(m):
        return m.detach().to("cpu", torch.float32).contiguous()
    k_ref, e_ref = host(k_ref), host(e_ref)
    rows = []
    with _single_thread():
        kr_inv, er_inv = torch.inverse(k_ref), torch.inverse(e_ref)
        for k, e in zip(src_ks, src_es):
            k, e = host(k), host(e)
            rows.append(torch.cat([kr_inv.reshape(-1), torch.matmul(e, er_inv).reshape(-1), k.reshape(-1),
                                   torch.inverse(k).reshape(-1), torch.matmul(e_ref, torch.inverse(e)).reshape(-1),
                                   k_ref.reshape(-1)]))
    return torch.stack(rows).contiguous()


def consistency_fuse(depth_ref, conf, k_ref, e_ref, src_depths, src_ks, src_es, photo_threshold=0.8, nconditions=5,
                     thre1=4.0, thre2=1300.0, per_view=False):
    """Fused filter for one reference view.  depth maps / conf: [h,w] GPU tensors; cameras: any device.
    -> dict(depth_avg [h,w], photo_mask, geo_mask, final_mask [h,w] bool[, view_masks [n,9,h,w] bool, rep [n,h,w]])."""
    _need_gpu(depth_ref, conf, *src_depths)
    h, w = depth_ref.shape
    dev = depth_ref.device
    # converted copies are held in locals until the launch is enqueued: a temporary's block goes back to the caching allocator as soon
    # as its data_ptr() is taken, and the next conversion is handed the same block
    depth_ref, conf, srcs = _f32c(depth_ref), _f32c(conf), [_f32c(d) for d in src_depths]
    mats = consistency_mats(k_ref, e_ref, src_ks, src_es).to(dev, non_blocking=True)
    depth_avg = torch.empty((h, w), device=dev, dtype=torch.float32)
    masks = torch.empty((3, h, w), device=dev, dtype=torch.uint8)
    vm = torch.empty((len(srcs), h, w), device=dev, dtype=torch.int16) if per_view else None
    rep = torch.empty((len(srcs), h, w), device=dev, dtype=torch.float32) if per_view else None
    _abi("mdf_consistency_fuse_fwd", (depth_ref.data_ptr(), conf.data_ptr(), _src_array(srcs), mats.data_ptr(),
                                      len(srcs), h, w, ctypes.c_float(photo_threshold), int(nconditions),
                                      ctypes.c_double(thre1), ctypes.c_double(thre2), depth_avg.data_ptr(), masks.data_ptr(),
                                      None if vm is None else vm.data_ptr(), None if rep is None else rep.data_ptr(),
                                      _stream(depth_avg),),
         tag=f"{w}x{h} nsrc{len(srcs)}", work={"bytes": 4.0 * h * w * (len(srcs) + 3) + 3.0 * h * w, "bound": "hbm"})
    mb = masks.view(torch.bool)         # the kernel writes 0 / 1 bytes: a reinterpretation, not three conversion launches per view
    out = {"depth_avg": depth_avg, "photo_mask": mb[0], "geo_mask": mb[1], "final_mask": mb[2]}
    if per_view:
        bits = vm.to(torch.int32) & 0xFFFF
        out["view_masks"] = torch.stack([((bits >> i) & 1).bool() for i in range(9)], dim=1)
        out["rep"] = rep
    return out


# --------------------------------------------------------------------------- DTU fusion: multi-view consensus (gipuma / fusibile)
CONSENSUS_CAM_STRIDE = 32


def consensus_cameras(K, E):
    """HOST: the camera table of mdf_consensus_fuse_fwd from intrinsics K [N,3,3] and extrinsics E [N,4,4] (any array-like).
    P = K E[:3] in float64 rounded to fp32 (what the reference writes as text and fusibile reads back as float);
    M_inv = inv(P[:, :3]) and C = -M_inv P[:, 3] in float64 from that fp32 P, rounded to fp32.  f = K[0][0, 0] of the scan's FIRST
    camera, used for every view.  -> (table [N, 32] float32 numpy, f float32)."""
    import numpy as np
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    E = np.asarray(E, dtype=np.float32).astype(np.float64)
    n = K.shape[0]
    tab = np.zeros((n, CONSENSUS_CAM_STRIDE), dtype=np.float32)
    for v in range(n):
        P = (K[v] @ E[v][:3]).astype(np.float32)
        m_inv = np.linalg.inv(P[:, :3].astype(np.float64))
        tab[v, 0:12] = P.reshape(-1)
        tab[v, 12:21] = m_inv.astype(np.float32).reshape(-1)
        tab[v, 21:24] = (-(m_inv @ P[:, 3].astype(np.float64))).astype(np.float32)
    return tab, np.float32(K[0][0, 0])


def consensus_fuse(depths, images, K, E, disp_thresh, num_consistent):
    """Fuse one scan's depth maps into a point cloud (the reference's DTU protocol: tools/gipuma/main.py -d).
    depths: GPU fp32 [N,H,W] (0 = invalid; apply the probability filter first); images: GPU uint8 [N,H,W,3] RGB;
    K [N,3,3], E [N,4,4]: host arrays.  -> (xyz [M,3] fp32, rgb [M,3] uint8, per-view kept counts [N] int32), all on the GPU,
    points in reference-view then row-major pixel order.  Device memory beyond the inputs: a workspace of 16 B per (view, pixel)
    (1.5 GB for a 49 x 1600 x 1184 DTU scan, ~16 GB for a 509-view Tanks scan at 1920 x 1056) plus 15 B per kept point."""
    _need_gpu(depths, images)
    if depths.dim() != 3 or images.dim() != 4 or tuple(images.shape) != (*depths.shape, 3) or images.dtype != torch.uint8:
        raise ValueError(f"depths [N,H,W] fp32 and images [N,H,W,3] uint8 expected, got {tuple(depths.shape)} and "
                         f"{tuple(images.shape)} {images.dtype}")
    n, h, w = depths.shape
    dev = depths.device
    tab, f = consensus_cameras(K, E)
    cams = torch.from_numpy(tab).to(dev)
    colors = torch.nn.functional.pad(images, (0, 1)).contiguous()          # RGBA8: one 4-byte gather per texel
    depths = _f32c(depths)
    ws = torch.empty(int(lib().mdf_consensus_fuse_workspace(n, h, w)), device=dev, dtype=torch.uint8)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    # two phases: fusion + count scan, then (the kept total read back) the compaction into outputs of exactly that size
    _abi("mdf_consensus_fuse_fwd", (depths.data_ptr(), colors.data_ptr(), cams.data_ptr(), n, h, w, ctypes.c_float(float(f)),
                                    ctypes.c_float(disp_thresh), int(num_consistent), ws.data_ptr(), None, None, 0,
                                    counts.data_ptr(), total.data_ptr(), _stream(depths)),
         tag=f"{w}x{h} n{n}", work={"pairs": float(n) * (n - 1) * h * w, "bound": "valu"})
    m = int(total.item())
    xyz = torch.empty((m, 3), device=dev, dtype=torch.float32)
    rgb = torch.empty((m, 3), device=dev, dtype=torch.uint8)
    if m:
        _abi("mdf_consensus_compact", (ws.data_ptr(), n, h, w, xyz.data_ptr(), rgb.data_ptr(), m, _stream(depths)),
             tag=f"{w}x{h} n{n}", work={"bytes": 16.0 * n * h * w + 15.0 * m, "bound": "hbm"})
    return xyz, rgb, counts


# --------------------------------------------------------------------------- point-cloud fusion (tools/pcd: visibility + small segments)
PCD_CAM_STRIDE = 64
PCD_STEPS = ("prob", "vis1", "vis_fusion", "vis2", "ave", "vis3", "seg")   # index k of a step == its MDF_PCD_STEP_* (prob: 0)
PCD_MAX_SOURCES = 64
PCD_PROB_THRESHOLD = 0.8
PCD_NORMAL_KNN = 30            # Open3D's estimate_normals() default: KDTreeSearchParamKNN(knn=30)


def pcd_cameras(K, E):
    """HOST: the camera table of mdf_pcd_fuse_fwd from intrinsics K [N,3,3] and extrinsics E [N,4,4] (any array-like):
    K, K^-1, E, E^-1 and the camera centre -R^T t, the last three in float64 from the fp32 K and E, rounded to fp32.
    -> float32 numpy [N, 64]."""
    import numpy as np
    K = np.asarray(K, dtype=np.float32)
    E = np.asarray(E, dtype=np.float32)
    tab = np.zeros((K.shape[0], PCD_CAM_STRIDE), dtype=np.float32)
    for v in range(K.shape[0]):
        k64, e64 = K[v].astype(np.float64), E[v].astype(np.float64)
        tab[v, 0:9] = K[v].ravel()
        tab[v, 9:18] = np.linalg.inv(k64).astype(np.float32).ravel()
        tab[v, 18:34] = E[v].ravel()
        tab[v, 34:50] = np.linalg.inv(e64).astype(np.float32).ravel()
        tab[v, 50:53] = (-(e64[:3, :3].T @ e64[:3, 3])).astype(np.float32)
    return tab


def pcd_sources(src_table, n, view):
    """HOST: [[source view indices of view i, best first] ...] (or an int array, -1 = none) -> int32 numpy [n, view]: the first
    `view` entries of each list, padded with -1."""
    import numpy as np
    t = np.full((n, view), -1, dtype=np.int32)
    for i in range(n):
        s = [int(x) for x in list(src_table[i]) if int(x) >= 0][:view]
        if any(x >= n for x in s):
            raise ValueError(f"view {i}: source index out of range in {s}")
        t[i, :len(s)] = s
    return t


def pcd_steps(depths, masks, cams, srcs, need, first, last):
    """Steps first..last (1..6, see PCD_STEPS) of the fusion pipeline in place on depths [N,H,W] fp32 / masks [N,H,W] uint8
    (GPU); cams [N,64] and srcs [N,V] int32 on the GPU.  -> (workspace, per-view mask-true counts [N] int32, total int)."""
    n, h, w = depths.shape
    v = srcs.shape[1]
    dev = depths.device
    ws = torch.empty(int(lib().mdf_pcd_fuse_workspace(n, h, w, v)), device=dev, dtype=torch.uint8)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    _abi("mdf_pcd_fuse_fwd", (depths.data_ptr(), masks.data_ptr(), cams.data_ptr(), srcs.data_ptr() if v else None, n, h, w, v,
                              int(need), int(first), int(last), ws.data_ptr(), counts.data_ptr(), total.data_ptr(),
                              _stream(depths)),
         tag=f"{w}x{h} n{n} v{v} steps{first}-{last}", work={"candidates": float(n) * (v + 1) * h * w, "bound": "valu"})
    return ws, counts, int(total.item())


def pcd_fuse(depths, probs, images, K, E, src_table, view=10, vthresh=4, normals=False, downsample=None, stages=None):
    """Fuse one scan's depth maps into a point cloud (the reference's tools/pcd/fusion.py:get_cloud, stages 1-8).
    depths, probs: GPU fp32 [N,H,W]; images: GPU uint8 [N,H,W,3] RGB; K [N,3,3], E [N,4,4]: host arrays; src_table: per view
    the list of its source view indices (pair.txt order, already restricted to views of the scan), of which the first `view`
    are used.  stages: None runs the whole pipeline; k in 1..7 stops after step PCD_STEPS[k-1] and returns that state only.
    -> dict(depths [N,H,W] fp32, masks [N,H,W] bool, counts [N] int32, and with the whole pipeline xyz [M,3] fp32,
    rgb [M,3] uint8, dirs [M,3] fp32 (camera centre - point)), all on the GPU, points in view then row-major pixel order.
    normals=True (stage 7) adds normals [M,3] fp64: estimate_normals over the points with k = PCD_NORMAL_KNN neighbours, oriented
    towards the camera by dirs.  downsample=d (stage 8) replaces the points by the means of a voxel grid of side d (d = -1: the
    90th percentile of nn_spacing, numpy's linear rule; needs M >= 2 and a positive result): xyz is the cell means rounded to
    fp32, rgb = uint8(round_half_away(clamp(mean of fp32(u8) / fp32(255), 0, 1) * 255)), normals the cell means (not
    renormalised), cells in ascending (x, y, z) cell order; `voxel` = the side used is added and dirs is dropped.
    Without either the result is what stages 1-6 give.  Neither Open3D call has been compared with an Open3D build.
    Device memory beyond the inputs: mdf_pcd_fuse_workspace (13 B per view-pixel + 8 (view + 3) B per pixel of one view)
    plus 27 B per point; stage 7 adds the fp64 points, the index (point_index: 52 B a point + 96 B a leaf slot) and the
    normals, 100 B a point in all, and no neighbour list; stage 8 adds 8 B a point for the spacing and its sorted copy, the
    attribute columns (24 or 48 B a point), mdf_pts_voxel_workspace (32 B a point + the sort tables) and the worst-case outputs
    (28 B + 8 B per attribute column a point)."""
    import math
    import numpy as np
    if downsample is not None:
        downsample = float(downsample)
        if downsample != -1.0 and not (math.isfinite(downsample) and downsample > 0):
            raise ValueError(f"pcd_fuse: downsample={downsample} must be finite and > 0, or -1 for the 90th percentile of the "
                             "nearest-neighbour spacing")
        if stages is not None:
            raise ValueError("pcd_fuse: downsample needs the whole pipeline (stages=None)")
    if normals and stages is not None:
        raise ValueError("pcd_fuse: normals need the whole pipeline (stages=None)")
    _need_gpu(depths, probs, images)
    if depths.dim() != 3 or tuple(probs.shape) != tuple(depths.shape) or tuple(images.shape) != (*depths.shape, 3) \
            or images.dtype != torch.uint8:
        raise ValueError(f"depths / probs [N,H,W] fp32 and images [N,H,W,3] uint8 expected, got {tuple(depths.shape)}, "
                         f"{tuple(probs.shape)} and {tuple(images.shape)} {images.dtype}")
    if not 0 <= view <= PCD_MAX_SOURCES:
        raise ValueError(f"view={view} out of range [0, {PCD_MAX_SOURCES}]")
    n, h, w = depths.shape
    dev = depths.device
    nsteps = len(PCD_STEPS) if stages is None else int(stages)
    if not 1 <= nsteps <= len(PCD_STEPS):
        raise ValueError(f"stages={stages} out of range [1, {len(PCD_STEPS)}]")
    cams = torch.from_numpy(pcd_cameras(K, E)).to(dev)
    srcs = torch.from_numpy(pcd_sources(src_table, n, view)).to(dev)
    need = int(np.ceil(np.float32(vthresh - 1.1)))
    # step 1 (probability filter) in torch: mask = prob > 0.8; depth *= mask
    masks = (probs > PCD_PROB_THRESHOLD).to(torch.uint8).contiguous()
    depths = (_f32c(depths) * masks).contiguous()
    ws, counts, m = pcd_steps(depths, masks, cams, srcs, need, 1, nsteps - 1) if nsteps > 1 else \
        pcd_steps(depths, masks, cams, srcs, need, 1, 0)
    out = {"depths": depths, "masks": masks.bool(), "counts": counts}
    if stages is not None:
        return out
    xyz = torch.empty((m, 3), device=dev, dtype=torch.float32)
    rgb = torch.empty((m, 3), device=dev, dtype=torch.uint8)
    dirs = torch.empty((m, 3), device=dev, dtype=torch.float32)
    if m:
        images = images.contiguous()
        _abi("mdf_pcd_compact", (depths.data_ptr(), masks.data_ptr(), images.data_ptr(), cams.data_ptr(), n, h, w,
                                 view, ws.data_ptr(), xyz.data_ptr(), rgb.data_ptr(), dirs.data_ptr(), m, _stream(depths)),
             tag=f"{w}x{h} n{n}", work={"bytes": 5.0 * n * h * w + 27.0 * m, "bound": "hbm"})
    out.update(xyz=xyz, rgb=rgb, dirs=dirs)
    if not normals and downsample is None:
        return out
    xyz64 = xyz.double()
    index = point_index(xyz64)
    if normals:
        out["normals"] = estimate_normals(index, dirs=dirs, k=PCD_NORMAL_KNN)
    if downsample is not None:
        voxel = pcd_voxel_size(index) if downsample == -1.0 else downsample
        attrs = (rgb.float() / 255.0).double()               # fp32(u8) / fp32(255), widened
        if normals:
            attrs = torch.cat([attrs, out["normals"]], 1)
        vxyz, vattrs = voxel_downsample(xyz64, voxel, attrs=attrs)
        c = vattrs[:, :3].clamp(0.0, 1.0) * 255.0
        r = torch.floor(c)
        out.update(xyz=vxyz.float(), rgb=(r + ((c - r) >= 0.5).double()).to(torch.uint8), voxel=voxel)
        if normals:
            out["normals"] = vattrs[:, 3:6].contiguous()
        del out["dirs"]
    return out


def pcd_voxel_size(index):
    """The voxel side of pcd_fuse(downsample=-1): numpy.percentile(nn_spacing(index), 90) with its linear interpolation at
    position 0.9 (M - 1), from one torch.sort on the GPU and the two values around that position."""
    m = index.n
    if m < 2:
        raise ValueError(f"pcd_fuse: downsample=-1 needs at least 2 points, got {m}")
    s, _ = torch.sort(nn_spacing(index))
    pos = (m - 1) * (90 / 100)                                 # numpy's virtual index of the linear method
    lo = int(pos // 1)
    t = pos - lo
    lo, hi = min(max(lo, 0), m - 1), min(max(lo + 1, 0), m - 1)
    a, b = (float(v) for v in s[[lo, hi]].tolist())
    d = b - a
    voxel = b - d * (1 - t) if t >= 0.5 else a + d * t       # numpy's two-sided lerp
    if not (voxel > 0 and voxel < float("inf")):
        raise ValueError(f"pcd_fuse: the 90th percentile of the nearest-neighbour spacing is {voxel}; a positive voxel size is needed")
    return voxel


# --------------------------------------------------------------------------- DTU point-cloud evaluation (the MATLAB scorer)
DTU_MAX_DIST_CP = 60.0         # PointCompareMain.m: MaxDist of MaxDistCP (cube size and distance cap)
DTU_OUTLIER = 20.0             # BaseEvalMain_web.m / ComputeStat_web.m: MaxDist of the statistics
DTU_MARGIN = 10                # the ObsMask{scan}_10.mat margin
REDUCE_ROUNDS_PER_CALL = 32


class PointIndex:
    """A spatial index over n fp64 points on the GPU (mdf_pts_index_build): `buf` holds the points in Morton order, the
    permutation back to the input order and the tree.  Build with point_index(pts)."""

    def __init__(self, buf, n, device):
        self.buf, self.n, self.device = buf, int(n), device

    @property
    def nbytes(self):
        return int(self.buf.numel())


def _pts64(pts, device=None):
    """[n,3] array-like or tensor -> contiguous fp64 GPU tensor (host data is copied to `device`, default cuda:current)."""
    if not torch.is_tensor(pts):
        import numpy as np
        pts = torch.from_numpy(np.ascontiguousarray(np.asarray(pts, dtype=np.float64)))
    if not pts.is_cuda:
        if device is None:
            raise RuntimeError("mdfnet_hip ops run on an MI355X only (got a CPU tensor); there is no CPU fallback")
        pts = pts.to(device)
    pts = pts.to(torch.float64).reshape(-1, 3).contiguous() if pts.numel() else pts.new_zeros((0, 3), dtype=torch.float64)
    return pts


def point_index(pts):
    """Spatial index over pts: GPU [n,3] (any float dtype; computed in fp64).  -> PointIndex.
    Device memory: 52 B a point + 96 B a leaf slot (the tree over leaves of 32 points, rounded up to a power of two)."""
    _need_gpu(pts)
    pts = _pts64(pts)
    n = pts.shape[0]
    nbytes = int(lib().mdf_pts_index_workspace(n))
    if nbytes <= 0 and n:
        raise ValueError(f"point_index: {n} points are too many")
    buf = torch.empty(max(nbytes, 16), device=pts.device, dtype=torch.uint8)
    _abi("mdf_pts_index_build", (pts.data_ptr() if n else None, n, buf.data_ptr(), buf.numel(), _stream(buf)), tag=f"n{n}",
         work={"points": float(n), "bound": "hbm"})
    return PointIndex(buf, n, pts.device)


def _host_doubles(vals, k):
    import numpy as np
    a = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).reshape(-1))
    if a.size != k:
        raise ValueError(f"{k} values expected, got {a.size}")
    return (ctypes.c_double * k)(*a.tolist())


def _queries_arg(queries):
    """queries of a search, a PointIndex or GPU [m,3] -> (m, the index's pointer or None, the fp64 array or None, the index's bytes)."""
    if isinstance(queries, PointIndex):
        return queries.n, queries.buf.data_ptr(), None, queries.nbytes
    _need_gpu(queries)
    q = _pts64(queries)
    return q.shape[0], None, q, 0


def nn_distance(index, queries, bb=None, cap=DTU_MAX_DIST_CP, return_visits=False):
    """MaxDistCP(Qto = index's points, Qfrom = queries, BB, cap) of the DTU scorer (MaxDistCP.m): for every query the exact
    nearest-neighbour distance if it is < cap and the query lies in BB's cubes of side cap, else cap.  queries: GPU [m,3] (fp64)
    or a PointIndex (its points are walked in Morton order, so the lanes of a wave follow nearby paths); bb: [[x,y,z],[x,y,z]]
    (BB(1,:), BB(2,:)) or None for no region.  -> dist [m] fp64 GPU (and the leaves visited per query, int32, with
    return_visits)."""
    if not isinstance(index, PointIndex):
        raise TypeError("nn_distance: index must come from point_index()")
    m, qidx, q, qbytes = _queries_arg(queries)
    dev = index.device
    dist = torch.empty(m, device=dev, dtype=torch.float64)
    visits = torch.empty(m, device=dev, dtype=torch.int32) if return_visits else None
    bbh = _host_doubles(bb, 6) if bb is not None else None
    if m:
        qpts = q.data_ptr() if q is not None else None
        _abi("mdf_pts_nn_dist", (index.buf.data_ptr(), index.n, index.nbytes, qidx, qpts, m, qbytes, bbh, float(cap), dist.data_ptr(),
                                 visits.data_ptr() if visits is not None else None, _stream(dist)),
             tag=f"n{index.n} m{m}", work={"queries": float(m), "bound": "valu"})
    return (dist, visits) if return_visits else dist


def reduce_points(pts, dst, order, index=None, stats=None):
    """reducePts_haa(pts, dst) for the visiting order `order` (a permutation of 0..n-1, first visited first): a point is kept iff
    no kept point visited before it lies within distance <= dst -- the sequential greedy result, computed in parallel rounds.
    pts: GPU [n,3]; order: int array-like or tensor; index: a PointIndex over pts to reuse.  -> (keep [n] bool GPU, rounds int).
    With a dict `stats`, its "edges" (pairs of a point and an earlier neighbour) and "rounds" are filled in."""
    import numpy as np
    _need_gpu(pts)
    pts = _pts64(pts)
    n = pts.shape[0]
    dev = pts.device
    if not (float(dst) > 0 and np.isfinite(float(dst))):
        raise ValueError(f"dst={dst} must be finite and > 0")
    order = torch.as_tensor(np.asarray(order) if not torch.is_tensor(order) else order).to(dev, torch.int64).reshape(-1)
    if order.numel() != n:
        raise ValueError(f"order has {order.numel()} entries for {n} points")
    rank = torch.empty(n, device=dev, dtype=torch.int32)
    if n:
        if bool(((order < 0) | (order >= n)).any()) or int(torch.bincount(order, minlength=n).max()) != 1:
            raise ValueError("order must be a permutation of 0..n-1")
        rank[order] = torch.arange(n, device=dev, dtype=torch.int32)
    index = index if index is not None else point_index(pts)
    if index.n != n:
        raise ValueError(f"index over {index.n} points for {n} points")
    ws = torch.empty(max(int(lib().mdf_pts_reduce_workspace(n)), 16), device=dev, dtype=torch.uint8)
    edges = torch.zeros(1, device=dev, dtype=torch.int64)
    args = (index.buf.data_ptr(), n, index.nbytes, rank.data_ptr() if n else None, ctypes.c_double(float(dst)), ws.data_ptr(), ws.numel())
    _abi("mdf_pts_reduce_count", args + (edges.data_ptr(), _stream(ws)), tag=f"n{n}", work={"points": float(n), "bound": "valu"})
    ne = int(edges.item())
    csr = torch.empty(max(ne, 1), device=dev, dtype=torch.int32)
    keep = torch.empty(max(n, 1), device=dev, dtype=torch.uint8)
    state = torch.zeros(3, device=dev, dtype=torch.int32)
    resume = 0
    while True:
        _abi("mdf_pts_reduce", args + (csr.data_ptr(), ne, resume, REDUCE_ROUNDS_PER_CALL, keep.data_ptr(), state.data_ptr(),
                                       _stream(ws)), tag=f"n{n} e{ne}", work={"edges": float(ne), "bound": "latency"})
        rounds, undecided, overflow = (int(x) for x in state.tolist())
        if overflow:
            raise RuntimeError(f"reduce_points: the neighbour lists did not fit ({ne} edges)")
        if undecided == 0:
            break
        resume = 1
    if stats is not None:
        stats.update(edges=ne, rounds=rounds)
    return keep[:n].bool(), rounds


def dtu_masks(qdata, obs_mask, bb, res, qstl, plane):
    """DataInMask and StlAbovePlane of PointCompareMain.m.  qdata [n,3], qstl [m,3]: GPU; obs_mask: the ObsMask array (MATLAB
    dimension order [s1,s2,s3], as read_mat returns it), host or GPU; bb [2,3], res, plane [4]: host values.
    -> (in_mask [n] bool, above [m] bool) on the GPU."""
    import numpy as np
    _need_gpu(qdata, qstl)
    q, s = _pts64(qdata), _pts64(qstl)
    dev = q.device
    if torch.is_tensor(obs_mask):
        dims = tuple(obs_mask.shape)
        om = obs_mask.to(dev).permute(*reversed(range(obs_mask.dim()))).contiguous().reshape(-1).to(torch.uint8)
    else:
        a = np.asarray(obs_mask)
        dims = a.shape
        om = torch.from_numpy(np.ascontiguousarray(a.reshape(-1, order="F")).astype(np.uint8)).to(dev)
    dims = tuple(dims) + (1,) * (3 - len(dims))
    if len(dims) != 3:
        raise ValueError(f"ObsMask must be 3-D, got shape {dims}")
    n, m = q.shape[0], s.shape[0]
    in_mask = torch.empty(max(n, 1), device=dev, dtype=torch.uint8)
    above = torch.empty(max(m, 1), device=dev, dtype=torch.uint8)
    om = om if om.numel() else torch.zeros(1, device=dev, dtype=torch.uint8)
    _abi("mdf_dtu_masks", (q.data_ptr(), n, om.data_ptr(), int(dims[0]), int(dims[1]), int(dims[2]), _host_doubles(bb, 6),
                           ctypes.c_double(float(res)), in_mask.data_ptr(), s.data_ptr(), m, _host_doubles(plane, 4), above.data_ptr(),
                           _stream(q)), tag=f"n{n} m{m}", work={"points": float(n + m), "bound": "hbm"})
    return in_mask[:n].bool(), above[:m].bool()


def dtu_stats(d):
    """ComputeStat_web.m on one filtered distance array (host): (count, mean, variance (n-1), median); NaN for an empty array
    (MATLAB's mean / var / median of []), variance 0 for one value."""
    import numpy as np
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    if d.size == 0:
        return 0, float("nan"), float("nan"), float("nan")
    return int(d.size), float(np.mean(d)), float(np.var(d, ddof=1)) if d.size > 1 else 0.0, float(np.median(d))


def dtu_scan_stats(ev, max_dist=DTU_OUTLIER):
    """The per-scan statistics of BaseEvalMain_web.m / ComputeStat_web.m from a BaseEval dict (Ddata, DataInMask, Dstl,
    StlAbovePlane): accuracy from Ddata[DataInMask & Ddata < max_dist], completeness from Dstl[StlAbovePlane & Dstl < max_dist]."""
    import numpy as np
    dd = np.asarray(ev["Ddata"], dtype=np.float64).reshape(-1)
    ds = np.asarray(ev["Dstl"], dtype=np.float64).reshape(-1)
    dd = dd[np.asarray(ev["DataInMask"], dtype=bool).reshape(-1)]
    ds = ds[np.asarray(ev["StlAbovePlane"], dtype=bool).reshape(-1)]
    nd, md, vd, medd = dtu_stats(dd[dd < max_dist])
    ns, ms, vs, meds = dtu_stats(ds[ds < max_dist])
    return {"nData": nd, "MeanData": md, "VarData": vd, "MedData": medd, "nStl": ns, "MeanStl": ms, "VarStl": vs, "MedStl": meds}


def dtu_eval_scan(qdata, qstl, obs_mask, bb, res, plane, dst=0.2, seed=0, max_dist=DTU_OUTLIER, device=None):
    """PointCompareMain.m + the statistics of one scan on the GPU.  qdata [N,3] (the method's points), qstl [M,3] (the STL
    points), host arrays or GPU tensors; obs_mask, bb [2,3], res, plane [4] as stored in ObsMask{scan}_10.mat / Plane{scan}.mat.
    Qdata is reduced to a minimum spacing of dst in the visiting order numpy.random.RandomState(seed).permutation(N) (MATLAB's
    randperm stream cannot be reproduced), then Ddata = MaxDistCP(Qstl, Qdata, BB, 60), Dstl = MaxDistCP(Qdata, Qstl, BB, 60)
    and the two masks.  -> dict with BaseEval's fields as host numpy (Qdata 3xN reduced, Ddata, Qstl 3xM, Dstl, DataInMask,
    StlAbovePlane, GroundPlane, dst, Margin), the statistics of dtu_scan_stats, and Rounds / Edges of the reduction."""
    import numpy as np
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    q = _pts64(qdata, dev)
    s = _pts64(qstl, dev)
    n = q.shape[0]
    order = np.random.RandomState(seed).permutation(n)
    stats = {}
    keep, _ = reduce_points(q, dst, order, stats=stats)
    qr = q[keep].contiguous()
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    stl_index = point_index(s)
    data_index = point_index(qr)
    ddata = nn_distance(stl_index, data_index, bb=bb, cap=DTU_MAX_DIST_CP)
    dstl = nn_distance(data_index, stl_index, bb=bb, cap=DTU_MAX_DIST_CP)
    in_mask, above = dtu_masks(qr, obs_mask, bb, res, s, plane)
    ev = {"Qdata": qr.cpu().numpy().T.copy(), "Ddata": ddata.cpu().numpy(), "Qstl": s.cpu().numpy().T.copy(), "Dstl": dstl.cpu().numpy(),
          "DataInMask": in_mask.cpu().numpy(), "StlAbovePlane": above.cpu().numpy(),
          "GroundPlane": np.asarray(plane, dtype=np.float64).reshape(4, 1), "dst": float(dst), "Margin": DTU_MARGIN,
          "Rounds": stats["rounds"], "Edges": stats["edges"]}
    ev.update(dtu_scan_stats(ev, max_dist))
    return ev


# --------------------------------------------------------------------------- Tanks and Temples F-score evaluation
# The training scenes' offline protocol: initial alignment from the camera centres, crop volume, voxel-grid
# downsampling, three rounds of point-to-point ICP, precision / recall / F at the scene's distance tau.  Everything fp64.
TANKS_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
             "Truck": 0.005}
TANKS_ICP_ITERS = 20
TANKS_ICP_REL = 1e-6                    # stop when fitness and inlier RMSE both change by less than this, relatively
TANKS_STAGE_C_POINTS = 4e6              # stage C keeps every k-th cropped point, k = max(round(n / 4e6), 1)
TANKS_HIST_BINS, TANKS_HIST_STRETCH = 100, 5
VOXEL_MAX_ATTRS = 6


def _mat4(T):
    import numpy as np
    T = np.ascontiguousarray(np.asarray(T.cpu() if torch.is_tensor(T) else T, dtype=np.float64))
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("a finite 4x4 matrix is expected")
    return T


def nn_search(index, queries, cap, return_d2=False, return_visits=False):
    """Exact nearest neighbour of every query among the index's points (mdf_pts_nn): -> (dist [m] fp64, nearest [m] int32) on the
    GPU, nearest = the point's position in the array the index was built from, or -1 (and dist = cap) when no point lies within
    d < cap; ties on d^2 go to the lowest position.  queries: GPU [m,3] or a PointIndex (walked in Morton order, results at the
    input positions).  return_d2 appends d^2 (+inf when none), return_visits the leaves visited per query."""
    if not isinstance(index, PointIndex):
        raise TypeError("nn_search: index must come from point_index()")
    m, qidx, q, qbytes = _queries_arg(queries)
    dev = index.device
    dist = torch.empty(m, device=dev, dtype=torch.float64)
    d2 = torch.empty(m, device=dev, dtype=torch.float64) if return_d2 else None
    nearest = torch.empty(m, device=dev, dtype=torch.int32)
    visits = torch.empty(m, device=dev, dtype=torch.int32) if return_visits else None
    if m:
        qpts = q.data_ptr() if q is not None else None
        _abi("mdf_pts_nn", (index.buf.data_ptr(), index.n, index.nbytes, qidx, qpts, m, qbytes, ctypes.c_double(float(cap)),
                            dist.data_ptr(), d2.data_ptr() if return_d2 else None, nearest.data_ptr(),
                            visits.data_ptr() if return_visits else None, _stream(dist)),
             tag=f"n{index.n} m{m}", work={"queries": float(m), "bound": "valu"})
    return (dist, nearest) + ((d2,) if return_d2 else ()) + ((visits,) if return_visits else ())


KNN_MAX = 32                   # MDF_PTS_KNN_MAX


def knn_search(index, queries, k, return_d2=False, return_visits=False):
    """Exact k nearest neighbours of every query among the index's points (mdf_pts_knn), 1 <= k <= 32: -> nbr [m,k] int32 on the
    GPU, row i = the positions (in the array the index was built from) of query i's min(k, n) nearest points in ascending
    (d^2, position) order, so ties on d^2 go to the lowest position and a point identical to the query counts like any other;
    slots past min(k, n) hold -1.  queries: GPU [m,3] or a PointIndex (walked in Morton order, results at the input positions).
    return_d2 appends d^2 [m,k] (+inf in the empty slots), return_visits the leaves visited per query."""
    if not isinstance(index, PointIndex):
        raise TypeError("knn_search: index must come from point_index()")
    m, qidx, q, qbytes = _queries_arg(queries)
    k = int(k)
    dev = index.device
    nbr = torch.empty((m, max(k, 0)), device=dev, dtype=torch.int32)
    d2 = torch.empty((m, max(k, 0)), device=dev, dtype=torch.float64) if return_d2 else None
    visits = torch.empty(m, device=dev, dtype=torch.int32) if return_visits else None
    _abi("mdf_pts_knn", (index.buf.data_ptr(), index.n, index.nbytes, qidx, q.data_ptr() if q is not None and m else None, m, qbytes, k,
                         nbr.data_ptr() if m else None, d2.data_ptr() if return_d2 and m else None,
                         visits.data_ptr() if return_visits and m else None, _stream(nbr)),
         tag=f"n{index.n} m{m} k{k}", work={"queries": float(m), "bound": "valu"})
    return nbr if not (return_d2 or return_visits) else (nbr,) + ((d2,) if return_d2 else ()) + ((visits,) if return_visits else ())


def estimate_normals(pts_or_index, dirs=None, k=30, return_cov=False):
    """Normals of a point cloud from its k nearest neighbours (mdf_pts_normals; the point itself is one of them): -> normals [n,3]
    fp64 on the GPU in input order, the unit eigenvector of the neighbours' covariance for its smallest eigenvalue, (0, 0, 1)
    when min(k, n) < 3.  dirs [n,3] (fp32) orients them: a normal n is kept when ((nx*dx) + ny*dy) + nz*dz > 0 and negated
    otherwise.  pts_or_index: GPU [n,3] or a PointIndex.  return_cov appends the covariance [n,6] (xx, xy, xz, yy, yz, zz), whose
    sums run over the neighbours in knn_search's order.  The neighbour lists are never stored."""
    index = pts_or_index if isinstance(pts_or_index, PointIndex) else point_index(pts_or_index)
    n, dev = index.n, index.device
    if dirs is not None:
        _need_gpu(dirs)
        dirs = _f32c(dirs).reshape(-1, 3)
        if dirs.shape[0] != n:
            raise ValueError(f"estimate_normals: {dirs.shape[0]} dirs for {n} points")
    nrm = torch.empty((n, 3), device=dev, dtype=torch.float64)
    cov = torch.empty((n, 6), device=dev, dtype=torch.float64) if return_cov else None
    _abi("mdf_pts_normals", (index.buf.data_ptr(), n, index.nbytes, int(k), dirs.data_ptr() if dirs is not None and n else None,
                             nrm.data_ptr() if n else None, cov.data_ptr() if return_cov and n else None, _stream(nrm)),
         tag=f"n{n} k{int(k)}", work={"queries": float(n), "bound": "valu"})
    return (nrm, cov) if return_cov else nrm


def nn_spacing(index):
    """The distance from every point of the index to its nearest other point (Open3D's compute_nearest_neighbor_distance): the
    square root of the second entry of a k = 2 self-query, so 0 for a duplicated point (and +inf for a lone point).  -> [n] fp64."""
    if not isinstance(index, PointIndex):
        raise TypeError("nn_spacing: index must come from point_index()")
    _, d2 = knn_search(index, index, 2, return_d2=True)
    return torch.sqrt(d2[:, 1])


def transform_points(pts, T):
    """p' = T p for a host 4x4 matrix (rows 0..2 are applied): x' = ((t00 x + t01 y) + t02 z) + t03.  pts GPU [n,3] -> [n,3] fp64."""
    _need_gpu(pts)
    pts = _pts64(pts)
    n = pts.shape[0]
    out = torch.empty_like(pts)
    _abi("mdf_pts_transform", (out.data_ptr() if n else None, pts.data_ptr() if n else None, n, _host_doubles(_mat4(T), 16),
                               _stream(pts)), tag=f"n{n}", work={"bytes": 48.0 * n, "bound": "hbm"})
    return out


def crop_volume(pts, axis, axis_min, axis_max, polygon):
    """The crop-volume test (mdf_pts_crop): keep [n] bool GPU, True iff axis_min <= p[axis] <= axis_max and the point's other two
    coordinates (u, v) = (y, z) / (x, z) / (x, y) for axis 0 / 1 / 2 lie inside `polygon` [k,2] (3 <= k <= 64) by the even-odd
    rule of include/mdfnet_hip.h."""
    import numpy as np
    _need_gpu(pts)
    pts = _pts64(pts)
    n = pts.shape[0]
    poly = np.ascontiguousarray(np.asarray(polygon, dtype=np.float64))
    if poly.ndim != 2 or poly.shape[1] != 2:
        raise ValueError(f"polygon must be [k,2], got {poly.shape}")
    k = poly.shape[0]
    keep = torch.empty(max(n, 1), device=pts.device, dtype=torch.uint8)
    _abi("mdf_pts_crop", (pts.data_ptr() if n else None, n, int(axis), ctypes.c_double(float(axis_min)), ctypes.c_double(float(axis_max)),
                          _host_doubles(poly, 2 * k) if k else None, k, keep.data_ptr(), _stream(pts)), tag=f"n{n} k{k}",
         work={"points": float(n), "bound": "valu"})
    return keep[:n].bool()


def voxel_downsample(pts, voxel, attrs=None, return_counts=False):
    """Voxel-grid downsampling (mdf_pts_voxel_downsample): one point per occupied cell of side `voxel`, the mean of the cell's
    points summed in input order, cells in ascending (x, y, z) cell order with the grid's origin at min(pts) - voxel/2.
    attrs: up to 6 fp64 columns [n,k] (colours, normals) averaged the same way.
    -> pts [m,3] (, attrs [m,k] when given) (, counts [m] int32 with return_counts), on the GPU."""
    _need_gpu(pts, attrs)
    pts = _pts64(pts)
    n = pts.shape[0]
    dev = pts.device
    voxel = float(voxel)
    if not (voxel > 0 and voxel < float("inf")):
        raise ValueError(f"voxel={voxel} must be finite and > 0")
    k = 0
    if attrs is not None:
        k = attrs.shape[-1] if attrs.dim() > 1 else 1
        attrs = attrs.to(torch.float64).reshape(n, k).contiguous()
        if k > VOXEL_MAX_ATTRS:
            raise ValueError(f"{k} attribute columns: at most {VOXEL_MAX_ATTRS}")
    nbytes = int(lib().mdf_pts_voxel_workspace(n))
    if nbytes <= 0 and n:
        raise ValueError(f"voxel_downsample: {n} points are too many")
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    out = torch.empty((max(n, 1), 3), device=dev, dtype=torch.float64)
    oat = torch.empty((max(n, 1), max(k, 1)), device=dev, dtype=torch.float64)
    cnt = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    m = torch.zeros(1, device=dev, dtype=torch.int64)
    _abi("mdf_pts_voxel_downsample", (pts.data_ptr() if n else None, attrs.data_ptr() if k and n else None, k, n, ctypes.c_double(voxel),
                                      ws.data_ptr(), ws.numel(), out.data_ptr(), oat.data_ptr(), cnt.data_ptr(), m.data_ptr(),
                                      _stream(pts)), tag=f"n{n} a{k}", work={"points": float(n), "bound": "hbm"})
    m = int(m.item())
    if m < 0:
        raise ValueError(f"voxel_downsample: voxel={voxel} needs more than 2^21 cells on an axis")
    res = (out[:m].clone(),)
    if attrs is not None:
        res += (oat[:m, :k].clone(),)
    if return_counts:
        res += (cnt[:m].clone(),)
    return res[0] if len(res) == 1 else res


VIEW_STATUS = {1: "an image index outside [0, n_img)", 2: "a track whose image indices do not ascend strictly",
               4: "track offsets outside [0, n_obs] or descending", 8: "a record count that does not match the tracks"}


def _view_inputs(rot, trans, pts, track_off, track_img):
    """The scene of the view-selection entries as contiguous GPU tensors -> (rot [N,9], trans [N,3], pts [P,3], track_off [P+1] int64,
    track_img [T] int32, n_rec = the sum over tracks of t(t-1)/2, computed from the offsets)."""
    _need_gpu(rot, trans, pts, track_off, track_img)
    rot = rot.to(torch.float64).reshape(-1, 9).contiguous()
    trans = trans.to(torch.float64).reshape(-1, 3).contiguous()
    pts = _pts64(pts)
    track_off = track_off.to(torch.int64).reshape(-1).contiguous()
    track_img = track_img.to(torch.int32).reshape(-1).contiguous()
    if trans.shape[0] != rot.shape[0]:
        raise ValueError(f"{rot.shape[0]} rotations, {trans.shape[0]} translations")
    if track_off.numel() != pts.shape[0] + 1:
        raise ValueError(f"track_off has {track_off.numel()} entries for {pts.shape[0]} points ({pts.shape[0] + 1} expected)")
    t = (track_off[1:] - track_off[:-1]).clamp(min=0, max=1 << 20)       # (a bad offset is the kernel's to report)
    n_rec = int((t * (t - 1) // 2).sum().item())
    return rot, trans, pts, track_off, track_img, n_rec


def _view_workspace(n, p, t, n_rec, dev, what):
    nbytes = int(lib().mdf_view_workspace(n, p, t, n_rec))
    if nbytes <= 0:
        raise ValueError(f"{what}: {n} images, {p} points, {t} observations and {n_rec} pair records are too many")
    return torch.empty(nbytes, device=dev, dtype=torch.uint8)


def _view_status(status, what):
    bits = int(status[0].item())
    if bits:
        raise ValueError(f"{what}: the tracks hold " + "; ".join(m for b, m in VIEW_STATUS.items() if bits & b))


def view_depth_ranges(rot, trans, pts, track_off, track_img, quantiles=(0.01, 0.99)):
    """Per-image depth range from a sparse model (mdf_view_depth_ranges): the depths z = r2 . p + t2 of every image's observations
    in ascending order, range[i] = the elements min(int(q * n_i), n_i - 1) for the two quantiles.  rot [N,3,3], trans [N,3]
    world -> camera, pts [P,3]; tracks as a CSR by point (track_off [P+1], track_img [T], strictly ascending inside a track).
    -> range [N,2] fp64 (NaN for an image without observations), count [N] int32, on the GPU."""
    rot, trans, pts, track_off, track_img, _ = _view_inputs(rot, trans, pts, track_off, track_img)
    n, p, t, dev = rot.shape[0], pts.shape[0], track_img.numel(), pts.device
    q_lo, q_hi = float(quantiles[0]), float(quantiles[1])
    if not (0.0 <= q_lo <= q_hi <= 1.0):
        raise ValueError(f"quantiles {quantiles} must satisfy 0 <= q_lo <= q_hi <= 1")
    ws = _view_workspace(n, p, t, 0, dev, "view_depth_ranges")
    rng = torch.empty((max(n, 1), 2), device=dev, dtype=torch.float64)
    cnt = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    status = torch.zeros(4, device=dev, dtype=torch.int32)
    _abi("mdf_view_depth_ranges", (rot.data_ptr() if n else None, trans.data_ptr() if n else None, n, pts.data_ptr() if p else None, p,
                                   track_off.data_ptr(), track_img.data_ptr() if t else None, t, ctypes.c_double(q_lo),
                                   ctypes.c_double(q_hi), ws.data_ptr(), ws.numel(), rng.data_ptr(), cnt.data_ptr(), status.data_ptr(),
                                   _stream(pts)), tag=f"n{n} t{t}", work={"points": float(t), "bound": "hbm"})
    _view_status(status, "view_depth_ranges")
    return rng[:n], cnt[:n]


def view_scores(rot, trans, pts, track_off, track_img, theta0=5.0, sigma1=1.0, sigma2=10.0, return_centres=False):
    """View-selection score of every image pair (mdf_view_scores): over the points both images see, in ascending point index, the sum
    of exp(-(theta - theta0)^2 / (2 sigma^2)) with theta the triangulation angle in degrees (atan2 of the cross and dot products of
    the rays to the two camera centres) and sigma = sigma1 up to theta0, sigma2 beyond.  Inputs as for view_depth_ranges.
    -> score [N,N] fp64 (symmetric, zero diagonal), shared [N,N] int32 (points in common) (, centres [N,3] fp64), on the GPU."""
    rot, trans, pts, track_off, track_img, n_rec = _view_inputs(rot, trans, pts, track_off, track_img)
    n, p, t, dev = rot.shape[0], pts.shape[0], track_img.numel(), pts.device
    theta0, sigma1, sigma2 = float(theta0), float(sigma1), float(sigma2)
    if not (sigma1 > 0 and sigma2 > 0 and sigma1 < float("inf") and sigma2 < float("inf") and abs(theta0) < float("inf")):
        raise ValueError(f"theta0={theta0}, sigma1={sigma1}, sigma2={sigma2}: theta0 finite and both sigmas finite and > 0 are needed")
    ws = _view_workspace(n, p, t, n_rec, dev, "view_scores")
    score = torch.empty((max(n, 1), max(n, 1)), device=dev, dtype=torch.float64)
    shared = torch.empty((max(n, 1), max(n, 1)), device=dev, dtype=torch.int32)
    status = torch.zeros(4, device=dev, dtype=torch.int32)
    _abi("mdf_view_scores", (rot.data_ptr() if n else None, trans.data_ptr() if n else None, n, pts.data_ptr() if p else None, p,
                             track_off.data_ptr(), track_img.data_ptr() if t else None, t, n_rec, ctypes.c_double(theta0),
                             ctypes.c_double(sigma1), ctypes.c_double(sigma2), ws.data_ptr(), ws.numel(), score.data_ptr(),
                             shared.data_ptr(), status.data_ptr(), _stream(pts)), tag=f"n{n} r{n_rec}",
         work={"points": float(n_rec), "bound": "hbm"})
    _view_status(status, "view_scores")
    res = (score[:n, :n], shared[:n, :n])
    if return_centres:
        res += (ws[:n * 24].clone().view(torch.float64).reshape(n, 3),)
    return res


UNDISTORT_KINDS = {"rational": 0, "fisheye": 1}
UNDISTORT_MAX_NSUB = 16


def undistort_images(src, kind, coeffs, fx, fy, cx, cy, out_hw, zoom=1.0, scale=1.0, nsub=1, want_valid=False):
    """Photographs of one distorted camera resampled to the pinhole camera [[zoom fx scale, 0, cx scale], [0, zoom fy scale, cy scale]]
    (mdf_image_undistort; include/mdfnet_hip.h states the map, the bilinear taps and the nsub x nsub sample mean, all fp64).
    src [B,H,W,3] uint8, contiguous, on the GPU; kind "rational" (coeffs k1, k2, p1, p2, k3, k4, k5, k6) or "fisheye" (k1..k4), coeffs up
    to 12 values (the rest zero); out_hw = (Hd, Wd).  -> dst [B,Hd,Wd,3] uint8 (, valid [B,Hd,Wd] uint8: 1 where no sample of the
    pixel fell outside the photograph), on the GPU."""
    import math
    import numpy as np
    if not torch.is_tensor(src):
        raise ValueError("undistort_images: src must be a tensor")
    if not src.is_cuda:
        raise ValueError("undistort_images: src must live on the GPU (there is no CPU fallback)")
    if src.dtype != torch.uint8:
        raise ValueError(f"undistort_images: src must be uint8, got {src.dtype}")
    if src.dim() != 4 or src.shape[-1] != 3:
        raise ValueError(f"undistort_images: src must be [B,H,W,3] (interleaved RGB), got {tuple(src.shape)}")
    if not src.is_contiguous():
        raise ValueError("undistort_images: src must be contiguous")
    if kind not in UNDISTORT_KINDS:
        raise ValueError(f"undistort_images: kind {kind!r} not in {sorted(UNDISTORT_KINDS)}")
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1)
    if c.size > 12 or not np.isfinite(c).all():
        raise ValueError(f"undistort_images: at most 12 finite coefficients, got {c.tolist()}")
    c = np.concatenate([c, np.zeros(12 - c.size)])
    b, hs, ws = (int(v) for v in src.shape[:3])
    hd, wd = int(out_hw[0]), int(out_hw[1])
    fx, fy, cx, cy, zoom, scale, nsub = float(fx), float(fy), float(cx), float(cy), float(zoom), float(scale), int(nsub)
    if min(b, hs, ws, hd, wd) <= 0:
        raise ValueError(f"undistort_images: empty sizes (source {tuple(src.shape)}, output {hd} x {wd})")
    if 3 * b * max(hs * ws, hd * wd) > 2 ** 31 - 1:
        raise ValueError(f"undistort_images: {b} images of {hs} x {ws} -> {hd} x {wd} exceed int32 indexing; pass fewer per call")
    if not 1 <= nsub <= UNDISTORT_MAX_NSUB:
        raise ValueError(f"undistort_images: nsub={nsub} out of range [1,{UNDISTORT_MAX_NSUB}]")
    if not all(math.isfinite(v) and v > 0 for v in (fx, fy, zoom, scale)) or not (math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"undistort_images: fx={fx}, fy={fy}, zoom={zoom}, scale={scale} must be finite and > 0, cx={cx}, cy={cy} finite")
    dst = torch.empty((b, hd, wd, 3), device=src.device, dtype=torch.uint8)
    valid = torch.empty((b, hd, wd), device=src.device, dtype=torch.uint8) if want_valid else None
    d = ctypes.c_double
    _abi("mdf_image_undistort", (src.data_ptr(), dst.data_ptr(), valid.data_ptr() if want_valid else None, b, hs, ws, hd, wd,
                                 UNDISTORT_KINDS[kind], _host_doubles(c, 12), d(fx), d(fy), d(cx), d(cy), d(zoom), d(scale), nsub,
                                 _stream(src)), tag=f"b{b} {ws}x{hs}->{wd}x{hd} n{nsub} {kind}",
         work={"points": float(b * hd * wd * nsub * nsub), "bound": "hbm"})
    return (dst, valid) if want_valid else dst


def icp_sums(src, tgt, nearest, d2, threshold):
    """The sums of one point-to-point ICP step (mdf_pts_icp_sums) over the pairs (src[i], tgt[nearest[i]]) with nearest[i] >= 0 and
    sqrt(d2[i]) < threshold -> host numpy [17]: inlier count, sum of d^2, source centroid, target centroid, H (3x3 row-major,
    H[a][b] = sum (s_a - cs_a)(t_b - ct_b))."""
    _need_gpu(src, tgt, nearest, d2)
    src, tgt = _pts64(src), _pts64(tgt)
    n, nt = src.shape[0], tgt.shape[0]
    nearest = nearest.to(torch.int32).contiguous()
    d2 = d2.to(torch.float64).contiguous()
    if nearest.numel() != n or d2.numel() != n:
        raise ValueError(f"{nearest.numel()} matches / {d2.numel()} distances for {n} source points")
    ws = torch.empty(int(lib().mdf_pts_icp_workspace()), device=src.device, dtype=torch.uint8)
    out = torch.zeros(17, device=src.device, dtype=torch.float64)
    _abi("mdf_pts_icp_sums", (src.data_ptr() if n else None, n, tgt.data_ptr() if nt else None, nt, nearest.data_ptr() if n else None,
                              d2.data_ptr() if n else None, ctypes.c_double(float(threshold)), ws.data_ptr(), ws.numel(), out.data_ptr(),
                              _stream(src)), tag=f"n{n}", work={"points": float(n), "bound": "latency"})
    return out.cpu().numpy()


def icp_rigid_update(sums):
    """The rigid motion that best maps the inlier source points onto their matches (host, numpy): from the centroids and the
    cross-covariance H of icp_sums, R = V diag(1, 1, det(V U^T)) U^T with H = U S V^T, t = ct - R cs.  -> 4x4."""
    import numpy as np
    cs, ct, H = sums[2:5], sums[5:8], np.asarray(sums[8:17], dtype=np.float64).reshape(3, 3)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = ct - R @ cs
    return T


def _rel_small(a, b, tol):
    return abs(a - b) < tol * max(abs(b), 1e-300)


def icp_point_to_point(source, target, threshold, init=None, max_iter=TANKS_ICP_ITERS, rel_tol=TANKS_ICP_REL, target_index=None):
    """Point-to-point ICP without scale.  The source under T is matched to its exact nearest target points with d < threshold;
    fitness = inliers / source points, rmse = sqrt(mean d^2 over inliers).  Then, up to max_iter times: T <- dT T with dT the
    rigid update of the matches (icp_rigid_update), match again, and stop once fitness and rmse both changed by less than rel_tol
    relatively (or no inlier is left).  source, target: GPU [n,3]; target_index: a PointIndex over target to reuse.
    -> (T 4x4 host numpy, fitness, rmse, iterations = updates applied)."""
    import numpy as np
    _need_gpu(source, target)
    src, tgt = _pts64(source), _pts64(target)
    index = target_index if target_index is not None else point_index(tgt)
    if index.n != tgt.shape[0]:
        raise ValueError(f"index over {index.n} points for {tgt.shape[0]} target points")
    n = src.shape[0]
    T = np.eye(4) if init is None else _mat4(init).copy()

    def evaluate(T):
        cur = transform_points(src, T)
        _, nearest, d2 = nn_search(index, cur, threshold, return_d2=True)
        s = icp_sums(cur, tgt, nearest, d2, threshold)
        cnt = s[0]
        return s, (cnt / n if n else 0.0), (float(np.sqrt(s[1] / cnt)) if cnt > 0 else 0.0)

    sums, fitness, rmse = evaluate(T)
    it = 0
    while it < max_iter and sums[0] > 0:
        T = icp_rigid_update(sums) @ T
        it += 1
        pf, pr = fitness, rmse
        sums, fitness, rmse = evaluate(T)
        if _rel_small(fitness, pf, rel_tol) and _rel_small(rmse, pr, rel_tol):
            break
    return T, float(fitness), float(rmse), it


def umeyama(src, dst, with_scale=True):
    """The least-squares similarity (Umeyama 1991) mapping src [n,3] onto dst [n,3] (host): -> 4x4 with c R and t."""
    import numpy as np
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    if len(src) != len(dst) or len(src) < 3:
        raise ValueError(f"umeyama: {len(src)} and {len(dst)} points (equal counts, at least 3)")
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    cov = b.T @ a / len(src)
    U, S, Vt = np.linalg.svd(cov)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ D @ Vt
    c = float((S * np.diag(D)).sum() / (a * a).sum() * len(src)) if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = md - c * R @ ms
    return T


def tanks_initial_alignment(est_poses, ref_poses, trans):
    """Step 1 of the protocol (host): the similarity that maps the camera centres of the estimate's trajectory onto those of the
    reference trajectory after `trans`, least squares over all cameras.  est_poses, ref_poses: [n,4,4] camera-to-world."""
    import numpy as np
    est = np.asarray(est_poses, dtype=np.float64).reshape(-1, 4, 4)
    ref = np.asarray(ref_poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(est) != len(ref):
        raise ValueError(f"the estimate's trajectory has {len(est)} cameras, the reference {len(ref)}")
    trans = _mat4(trans)
    ref_c = ref[:, :3, 3] @ trans[:3, :3].T + trans[:3, 3]
    return umeyama(est[:, :3, 3], ref_c, with_scale=True)


def tanks_fscore(d_est, d_gt, tau):
    """Step 6's numbers from the two distance arrays (host): precision, recall, F and the two cumulative histograms."""
    import numpy as np
    d_est, d_gt = np.asarray(d_est, dtype=np.float64), np.asarray(d_gt, dtype=np.float64)
    p = float((d_est < tau).mean()) if d_est.size else 0.0
    r = float((d_gt < tau).mean()) if d_gt.size else 0.0
    f = 2 * p * r / (p + r) if p + r > 0 else 0.0
    top = TANKS_HIST_STRETCH * tau
    hists = []
    for d in (d_est, d_gt):
        h, edges = np.histogram(d, bins=TANKS_HIST_BINS, range=(0.0, top))
        hists.append(np.cumsum(h).astype(np.float64) / max(d.size, 1))
    return p, r, f, hists[0], hists[1], edges


def tanks_eval_scene(est, gt, crop, tau, init, device=None):
    """The Tanks and Temples F-score of one scene on the GPU.  est [N,3], gt [M,3]: host arrays or GPU tensors; crop: dict with
    axis (0/1/2), axis_min, axis_max, polygon [k,2] (tools/data_io.py:read_crop_json); tau: the scene's distance; init: the 4x4
    of step 1.  Stages A, B (voxel tau, tau/2; ICP threshold 80 tau, 20 tau) and C (every k-th cropped point; 2 tau) refine T
    against the whole ground truth; then both clouds are cropped, downsampled at tau/2 and compared.
    -> dict: precision, recall, fscore, tau, T, T_init, stage_T [3,4,4], stage_fitness / stage_rmse / stage_iterations [3],
    hist_est, hist_gt [100] (cumulative, over [0, 5 tau]), hist_edges [101] and the point counts n_*."""
    import numpy as np
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    e, g = _pts64(est, dev), _pts64(gt, dev)
    tau = float(tau)
    if not (tau > 0 and np.isfinite(tau)):
        raise ValueError(f"tau={tau} must be finite and > 0")
    T = _mat4(init).copy()
    res = {"tau": tau, "T_init": T.copy(), "n_est": e.shape[0], "n_gt": g.shape[0]}

    def cropped(pts):
        return pts[crop_volume(pts, crop["axis"], crop["axis_min"], crop["axis_max"], crop["polygon"])].contiguous()

    gidx = point_index(g)
    stage_T, stage_f, stage_r, stage_i = [], [], [], []
    for name, vox, thr in (("A", tau, 80 * tau), ("B", tau / 2, 20 * tau), ("C", None, 2 * tau)):
        s = cropped(transform_points(e, T))
        res[f"n_crop_{name}"] = s.shape[0]
        if vox is not None:
            s = voxel_downsample(s, vox)
        else:
            k = max(int(round(s.shape[0] / TANKS_STAGE_C_POINTS)), 1)
            s = s[::k].contiguous()
        res[f"n_down_{name}"] = s.shape[0]
        dT, fit, rmse, its = icp_point_to_point(s, g, thr, target_index=gidx)
        T = dT @ T
        stage_T.append(T.copy()); stage_f.append(fit); stage_r.append(rmse); stage_i.append(its)
    del gidx
    ec = cropped(transform_points(e, T))
    gc = cropped(g)
    ed, gd = voxel_downsample(ec, tau / 2), voxel_downsample(gc, tau / 2)
    res.update(n_est_crop=ec.shape[0], n_gt_crop=gc.shape[0], n_est_down=ed.shape[0], n_gt_down=gd.shape[0])
    cap = 2 * TANKS_HIST_STRETCH * tau                    # past the histograms' range: a capped distance lands in no bin
    eidx, gdx = point_index(ed), point_index(gd)
    d1 = nn_search(gdx, eidx, cap)[0].cpu().numpy()
    d2 = nn_search(eidx, gdx, cap)[0].cpu().numpy()
    p, r, f, h1, h2, edges = tanks_fscore(d1, d2, tau)
    res.update(precision=p, recall=r, fscore=f, T=T, stage_T=np.stack(stage_T), stage_fitness=np.array(stage_f),
               stage_rmse=np.array(stage_r), stage_iterations=np.array(stage_i, dtype=np.int64), hist_est=h1, hist_gt=h2,
               hist_edges=edges, dist_est=d1, dist_gt=d2)
    return res


# --------------------------------------------------------------------------- meshing: TSDF fusion, marching tetrahedra, vertex colour
TSDF_CHUNK = 16                # MDF_TSDF_CHUNK: views per launch
TSDF_CAM_FLOATS = 20           # MDF_TSDF_CAM_FLOATS
MESH_CHUNK = 1024              # MDF_MESH_CHUNK


def tsdf_cameras(K, E, dmax=None):
    """HOST: the camera table of mdf_tsdf_integrate / mdf_mesh_colour from intrinsics K [V,3,3] and extrinsics E [V,4,4] (any
    array-like), rounded to fp32: R row-major, t, fx, fy, cx, cy (no skew), dmax (the largest valid depth of the view's map)."""
    import numpy as np
    K = np.asarray(torch.as_tensor(K).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 3, 3)
    E = np.asarray(torch.as_tensor(E).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 4, 4)
    if len(K) != len(E):
        raise ValueError(f"{len(K)} intrinsics for {len(E)} extrinsics")
    t = np.zeros((len(K), TSDF_CAM_FLOATS), np.float32)
    t[:, 0:9] = E[:, :3, :3].reshape(-1, 9)
    t[:, 9:12] = E[:, :3, 3]
    t[:, 12], t[:, 13], t[:, 14], t[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    if dmax is not None:
        t[:, 16] = np.asarray(dmax, np.float32)
    return np.ascontiguousarray(t)


def _tsdf_views(depths, what="depths", dtype=torch.float32, tail=()):
    """[V,h,w(,3)] tensor or list of V same-shaped maps -> list of contiguous maps of `dtype` (no copy when already so)."""
    maps = list(depths) if not torch.is_tensor(depths) else [depths[v] for v in range(depths.shape[0])]
    if not maps:
        raise ValueError(f"{what}: at least one view is needed")
    _need_gpu(*maps)
    shape = tuple(maps[0].shape)
    if len(shape) != 2 + len(tail) or shape[2:] != tuple(tail) or any(tuple(m.shape) != shape for m in maps):
        raise ValueError(f"{what}: every view needs the same [h,w{',3' if tail else ''}] shape, got {[tuple(m.shape) for m in maps][:4]}")
    return [m if (m.dtype == dtype and m.is_contiguous()) else m.to(dtype).contiguous() for m in maps]


def _volume_args(origin, voxel, dims):
    import numpy as np
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3:
        raise ValueError(f"dims={dims}: (nx, ny, nz) is expected")
    o = (ctypes.c_float * 3)(*[float(x) for x in np.asarray(torch.as_tensor(origin).cpu().numpy(), np.float32).reshape(3)])
    return (ctypes.c_int * 3)(*dims), o, ctypes.c_float(float(np.float32(voxel))), dims


def tsdf_integrate(depths, K, E, origin, voxel, dims, trunc, state=None, chunk=None):
    """Integrate V depth maps ([V,h,w] GPU tensor or list of [h,w]; 0 / non-finite = no depth) into a truncated signed distance
    volume of dims = (nx, ny, nz) lattice points at origin + voxel * (i,j,k); trunc in world units.  -> (D, W) [nz,ny,nx] fp32:
    every point's running mean of min(1, (d - z) / trunc) over the views that see it, in the order given, and their number.
    state = (D, W) continues an earlier call (the tensors are updated in place and returned); chunk = views per launch
    (<= TSDF_CHUNK, the default).  The result does not depend on chunk or on where a sequence of calls was split."""
    import numpy as np
    maps = _tsdf_views(depths)
    h, w = maps[0].shape
    cdims, corigin, cvoxel, dims = _volume_args(origin, voxel, dims)
    dev = maps[0].device
    if state is None:
        D = torch.zeros((dims[2], dims[1], dims[0]), device=dev, dtype=torch.float32) if min(dims) > 0 else None
        W = torch.zeros_like(D) if D is not None else None
    else:
        D, W = state
        _need_gpu(D, W)
        if tuple(D.shape) != dims[::-1] or tuple(W.shape) != dims[::-1] or D.dtype != torch.float32 or W.dtype != torch.float32 \
                or not D.is_contiguous() or not W.is_contiguous():
            raise ValueError(f"state: two contiguous fp32 tensors of shape {dims[::-1]} are expected")
    # the largest valid depth of every view, for the brick culling (torch.aminmax over the map with invalid texels at -inf)
    stack = torch.stack(maps).flatten(1)
    valid = torch.isfinite(stack) & (stack > 0)
    dmax = torch.aminmax(torch.where(valid, stack, torch.full_like(stack, float("-inf"))), dim=1).max.cpu().numpy()
    cams = tsdf_cameras(K, E, dmax)
    if len(cams) != len(maps):
        raise ValueError(f"{len(maps)} depth maps for {len(cams)} cameras")
    n = dims[0] * dims[1] * dims[2]
    _abi("mdf_tsdf_integrate", (None if D is None else D.data_ptr(), None if W is None else W.data_ptr(), cdims, corigin, cvoxel,
                                ctypes.c_float(float(np.float32(trunc))), _src_array(maps), cams.ctypes.data_as(ctypes.c_void_p),
                                len(maps), h, w, 0 if chunk is None else int(chunk), _stream(maps[0])),
         tag=f"{dims[0]}x{dims[1]}x{dims[2]} V{len(maps)} {w}x{h}",
         work={"bytes": (8.0 * 2 * -(-len(maps) // (chunk or TSDF_CHUNK)) + 4.0 * len(maps)) * n, "bound": "hbm"})
    return D, W


def mesh_workspace_bytes(n):
    return 18 * n + 24 * ((n + MESH_CHUNK - 1) // MESH_CHUNK) + 256      # MDF_MESH_WORKSPACE_BYTES


def tsdf_mesh(D, W, origin, voxel, min_weight=1):
    """Marching tetrahedra over the Kuhn split of the cells of a TSDF volume (D, W [nz,ny,nx] from tsdf_integrate) whose 8 corners
    have W >= min_weight; a corner is inside where D < 0.  -> (vertices [N,3] fp32, triangles [M,3] int32), vertices in increasing
    (lattice index, edge direction), triangles in increasing (cell, tetrahedron, triangle), normals towards free space."""
    _need_gpu(D, W)
    if D.dim() != 3 or D.shape != W.shape:
        raise ValueError(f"D {tuple(D.shape)} and W {tuple(W.shape)}: two [nz,ny,nx] volumes are expected")
    D, W = _f32c(D), _f32c(W)
    dev = D.device
    cdims, corigin, cvoxel, dims = _volume_args(origin, voxel, tuple(D.shape)[::-1])
    n = D.numel()
    nbytes = mesh_workspace_bytes(n)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    totals = torch.zeros(2, device=dev, dtype=torch.int64)
    mw = ctypes.c_float(float(min_weight))
    _abi("mdf_mesh_count", (D.data_ptr(), W.data_ptr(), cdims, corigin, cvoxel, mw, ws.data_ptr(), nbytes, totals.data_ptr(),
                            _stream(D)), tag=f"{dims[0]}x{dims[1]}x{dims[2]}", work={"bytes": 8.0 * n + 46.0 * n, "bound": "hbm"})
    nv, nt = (int(x) for x in totals.tolist())
    vertices = torch.empty((nv if nt else 0, 3), device=dev, dtype=torch.float32)
    triangles = torch.empty((nt if nv else 0, 3), device=dev, dtype=torch.int32)
    if nv and nt:
        _abi("mdf_mesh_emit", (D.data_ptr(), W.data_ptr(), cdims, corigin, cvoxel, mw, ws.data_ptr(), nbytes, nv, nt,
                               vertices.data_ptr(), triangles.data_ptr(), _stream(D)), tag=f"{dims[0]}x{dims[1]}x{dims[2]}",
             work={"bytes": 2.0 * n + 12.0 * nv + 12.0 * nt, "bound": "hbm"})
    return vertices, triangles


def mesh_colour(vertices, depths, images, K, E, trunc):
    """Colour of mesh vertices [N,3] from V views: depths as for tsdf_integrate, images [V,h,w,3] uint8 (or a list).  A view counts
    for a vertex that lands on its map with a valid depth d and |d - z| <= trunc; the colour is the mean of the nearest texels over
    those views (in the order given), rounded half up; (128,128,128) where no view counts.  -> uint8 [N,3]."""
    import numpy as np
    _need_gpu(vertices)
    maps = _tsdf_views(depths)
    imgs = _tsdf_views(images, "images", torch.uint8, (3,))
    h, w = maps[0].shape
    if tuple(imgs[0].shape[:2]) != (h, w) or len(imgs) != len(maps):
        raise ValueError(f"{len(imgs)} images {tuple(imgs[0].shape)} for {len(maps)} depth maps {(h, w)}")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices {tuple(vertices.shape)}: [N,3] is expected")
    vtx = _f32c(vertices)
    n = vtx.shape[0]
    rgb = torch.empty((n, 3), device=vtx.device, dtype=torch.uint8)
    cams = tsdf_cameras(K, E)
    if len(cams) != len(maps):
        raise ValueError(f"{len(maps)} depth maps for {len(cams)} cameras")
    if n == 0:
        return rgb
    acc = torch.empty((n, 4), device=vtx.device, dtype=torch.float32)
    _abi("mdf_mesh_colour", (vtx.data_ptr(), n, _src_array(maps), _src_array(imgs), cams.ctypes.data_as(ctypes.c_void_p), len(maps),
                             h, w, ctypes.c_float(float(np.float32(trunc))), acc.data_ptr(), rgb.data_ptr(), _stream(vtx)),
         tag=f"N{n} V{len(maps)} {w}x{h}", work={"bytes": (12.0 + 7.0 * len(maps) + 3.0) * n, "bound": "hbm"})
    return rgb
