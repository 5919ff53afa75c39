"""Depth-hypothesis slot (reference: net/unit/depthhypos.py:10-253)."""
import torch
import torch.nn as nn

from mdfnet_hip import controlplane, hostmirror, layers, ops

CURVES = ("gauss0", "gauss1", "laplace", "atv")
_STEP2 = {"gauss0": 1, "gauss1": 1, "laplace": 2}     # mdf_hypos_from_fit_fwd: sqrt(-s ln thr) for both Gaussians, |s ln thr|


def fit_mode(curve, per_pixel):
    """mdf_hypos_fit_fwd mode of a curve: gauss1 on hypotheses shared by all pixels keeps the path that mirrors the reference's
    bits (mode 1, host-prepared fit row); gauss0 and per-pixel gauss1 are the centred device fits (modes 3, 4)."""
    if curve == "gauss0":
        return 3
    if curve == "gauss1":
        return 4 if per_pixel else 1
    if curve == "laplace":
        return 2
    if curve == "atv":
        return None                                   # no fit: the spread kernel (mdf_atv_spread_fwd) takes its place
    raise NotImplementedError(f"HyposByFit curve '{curve}' is not built ({', '.join(CURVES)} are)")


class HyposByFit(nn.Module):
    """HyposByFit(ndepths, curve_calss, prob_thresh); no parameters or buffers (contributes nothing to
    the state_dict, like the reference whose prob_thresh is a plain tensor attribute).

    curve_calss "atv" is the reference's atv_hypos (depthhypos.py:218-253) in this slot: the range is the spread
    atv_scale * sqrt(sum_d p_d (x_d - depth)^2) of the previous stage's distribution (UCS-Net's exp_variance with lamb = atv_scale)
    on either side of the depth, not a curve fit; prob_thresh is ignored, nothing comes from the host, and the hypotheses are not
    clamped to the depth range (the reference has no clamp; every hypothesis is >= 1e-12).

    ops.recorded("log_thresh", step-2 mode) hands out the logarithms recorded for the pinned goldens of the default composition.
    It is keyed by the step-2 mode, which two Gaussian stages with different thresholds would share, so only a slot with one of
    the default composition's (curve, threshold) pairs consults it; every other takes log(prob_thresh)."""

    def __init__(self, ndepths: int = 16, curve_calss: str = "gauss1", prob_thresh: float = 0.95, atv_scale: float = 1.5) -> None:
        super().__init__()
        self.ndepths, self.curve_calss, self.atv_scale = ndepths, curve_calss, float(atv_scale)
        self.prob_thresh = torch.tensor(prob_thresh)
        self.default_curve = (curve_calss, float(prob_thresh)) in (("gauss1", 0.95), ("laplace", 1e-5))     # config.py:147-148

    def uniform_host(self, depth_range):
        """depthhypos.py:31-38 on the host (B*D floats; GPU `tensor / int` rounds differently) -> [B,D,1,1] CPU."""
        dr = hostmirror.get(depth_range)
        b = dr.shape[0]
        lo = dr[:, 0].float().reshape(b, 1)
        step = (dr[:, 1].float().reshape(b, 1) - lo) / (self.ndepths - 1)
        return (lo + torch.arange(0, self.ndepths).reshape(1, -1) * step).reshape(b, self.ndepths, 1, 1).contiguous()

    def _uniform(self, depth_range):
        plan = controlplane.for_range(depth_range)
        if plan is not None and plan.hyp0 is not None and plan.hyp0.shape[1] == self.ndepths:
            return plan.hyp0                                  # uploaded with the rest of the forward's control plane
        host = self.uniform_host(depth_range)
        if depth_range.is_cuda:
            return hostmirror.put(host.to(depth_range.device, non_blocking=True), host)
        return host

    def forward(self, depth, depth_range, prob_volume, depth_hypos, upsample=False):
        if depth is None:
            return self._uniform(depth_range)
        mode = fit_mode(self.curve_calss, depth_hypos.shape[-1] != 1 or depth_hypos.shape[-2] != 1)
        on_gpu = depth.is_cuda and prob_volume.is_cuda      # no gradient flows here (depthhypos.py:40): same kernels in training
        if not on_gpu and not layers.use_hip(self, depth.detach(), prob_volume.detach()):
            if self.curve_calss == "atv":
                return layers.stock().hypos_by_atv(self.atv_scale, self.ndepths, depth.detach(), prob_volume.detach(),
                                                   depth_hypos.detach(), upsample)
            return layers.stock().hypos_by_fit(self.curve_calss, self.prob_thresh, self.ndepths, depth.detach(), depth_range,
                                         prob_volume.detach(), depth_hypos.detach(), upsample)
        if self.curve_calss == "atv":
            with torch.no_grad():
                e = ops.atv_spread(prob_volume, depth, depth_hypos, self.atv_scale)
                return ops.atv_hypos(e, depth, self.ndepths, bool(upsample))
        step2 = _STEP2[self.curve_calss]
        with torch.no_grad():
            row = None
            plan = controlplane.for_range(depth_range)
            if mode == 1:
                if plan is not None and plan.fit_row is not None and depth_hypos is plan.hyp0:
                    row = plan.fit_row
                else:
                    row = ops.gauss1_fit_row(hostmirror.get(depth_hypos)).to(depth.device, non_blocking=True)
            s = ops.hypos_fit(mode, prob_volume, depth, depth_hypos, row)
            rng = plan.rng if plan is not None else hostmirror.get(depth_range).float().contiguous().to(depth.device, non_blocking=True)
            log_thr = ops.recorded("log_thresh", step2) if self.default_curve else None
            if log_thr is None:
                log_thr = float(torch.log(self.prob_thresh))
            return ops.hypos_from_fit(step2, s, depth, rng, log_thr, self.ndepths, bool(upsample))
