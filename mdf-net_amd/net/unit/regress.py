"""Regress slot: soft-argmin depth and photometric confidence (reference: net/unit/regress.py)."""
from mdfnet_hip import layers, ops


def depth_regression(prob_volume, depth_hypos):
    """regress.py:5-7: sum_d prob * hypos.  prob [B,D,h,w]; hypos [B,D,1,1] | [B,D,h,w] -> [B,h,w]."""
    if not layers.use_hip(None, prob_volume, depth_hypos):
        return layers.stock().depth_regression(prob_volume, depth_hypos)   # rehearsal backend only
    return ops.depth_regress(prob_volume, depth_hypos)


depth_regression.mdf_builtin = True   # lets CoreNet fuse it into the regulariser's last kernel

_DEFAULT_PAD = (0, 0, 0, 0, 1, 2)
_BLEND = (0.8, 0.2)     # regress.py:23: 0.8 * upsampled last confidence + 0.2 * this stage's


def _window(prob_volume, last_confidence, n, pad):
    """Checks the arguments of confidence_regress (on any device, before a GPU is asked for) -> the window's front pad."""
    if prob_volume.dim() != 4:
        raise ValueError(f"prob_volume of shape {tuple(prob_volume.shape)}: expected [B,D,H,W]")
    if n not in (1, 2, 4, 8):
        # the reference computes n * avg_pool3d over the window: exactly the window's sum only where 1/n is a power of two
        raise ValueError(f"n={n!r}: the window length must be 1, 2, 4 or 8")
    pad = tuple(pad)
    if len(pad) != 6 or any(not isinstance(v, int) for v in pad) or pad[:4] != (0, 0, 0, 0) or pad[4] < 0 or pad[5] < 0:
        raise ValueError(f"pad={pad!r}: expected (0, 0, 0, 0, front, back), padding on the depth axis only")
    if pad[4] + pad[5] < n - 1:
        raise ValueError(f"pad={pad!r}: front + back must be at least n - 1 = {n - 1} (the pooled volume keeps every depth index)")
    if last_confidence is not None:
        b, _, h, w = prob_volume.shape
        if tuple(last_confidence.shape) != (b, h // 2, w // 2) or h % 2 or w % 2:
            raise ValueError(f"last_confidence of shape {tuple(last_confidence.shape)}: expected [B,H/2,W/2] = "
                             f"{(b, h // 2, w // 2)} for a volume {tuple(prob_volume.shape)} with even H and W")
    return pad[4]


def confidence_regress(prob_volume, last_confidence=None, n=4, pad=(0, 0, 0, 0, 1, 2)):
    """regress.py:9-25: the sum of the n probabilities around trunc(E[d]) (window idx-front .. idx-front+n-1, zero outside the
    volume); with last_confidence [B,H/2,W/2]: 0.8 * bicubic x2 of it + 0.2 * that sum."""
    if last_confidence is None and n == 4 and tuple(pad) == _DEFAULT_PAD:
        _window(prob_volume, None, n, pad)
        return ops.confidence(prob_volume.detach())
    return confidence_cascade(prob_volume, last_confidence, n, pad)


confidence_regress.mdf_builtin = True   # lets CoreNet fold the nearest x2 upsampling of core.py:76 into the same launch


def confidence_cascade(prob_volume, last_confidence=None, n=4, pad=(0, 0, 0, 0, 1, 2), up2=False):
    """confidence_regress for a Confidence_regress slot that CoreNet calls after EVERY stage with the previous stage's result
    (stage 0: None), so the confidence accumulates over the cascade: c0 = f(p0), c1 = f(p1, c0), c2 = f(p2, c1).  Same
    arithmetic as confidence_regress; every call is one launch of confidence_cascade_kernel.  up2 (the last stage's call): with
    the nearest x2 of core.py:76 in the same launch."""
    front = _window(prob_volume, last_confidence, n, pad)
    last = None if last_confidence is None else last_confidence.detach()
    return ops.confidence_cascade(prob_volume.detach(), last, n, front, _BLEND, up2)


confidence_cascade.mdf_builtin = True
confidence_cascade.mdf_cascade = True   # CoreNet (eval): conf = slot(prob, last_confidence=conf) after each stage
