"""Stage orchestrator (reference: net/core.py:4-78): same constructor slots, forward signature, output
dicts and state_dict keys; the stage loop runs on one HIP stream with the hot operators as fused kernels."""
import torch

from mdfnet_hip import controlplane, hostmirror, layers, ops


import contextlib
import os as _os

_STAGE_STREAMS = bool(int(_os.environ.get("MDF_TRAIN_STAGE_STREAMS", "1")))      # dev A/B: 0 = the whole training step on one stream
_SIDE = {}


def _stage_streams(device, n):
    key = (device.index if device.index is not None else torch.cuda.current_device(), n)
    if key not in _SIDE:
        _SIDE[key] = [torch.cuda.Stream(device) for _ in range(n)]
    return _SIDE[key]


@contextlib.contextmanager
def _on_stage_stream(side, stage, main, feats):
    """Issue the body on side[stage]: forked from `main` before, joined into it after (inside a hipGraph recording both edges are
    recorded).  The feature maps were allocated on `main` and are read on the stage's stream."""
    if not side:
        yield
        return
    st = side[stage]
    st.wait_stream(main)
    for f in feats:
        base = getattr(f, "_mdf_parent", None)
        (base[0] if base is not None else f).record_stream(st)
    with torch.cuda.stream(st):
        yield
    main.wait_stream(st)


def _cut_features(feats, cuts):
    """One stage's per-view feature maps -> detached copies that require grad (leaves of the stage's backward chain), noted in
    `cuts`.  The views of one view-major tensor (FPN_4Scales.forward_views) stay slices of ONE cut tensor, so the aggregation slot
    still takes it -- and returns its gradient -- whole."""
    parents = [getattr(f, "_mdf_parent", None) for f in feats]
    pairs = []
    if all(p is not None and p[0] is parents[0][0] and p[1] == i and p[2] == len(feats) for i, p in enumerate(parents)):
        y = parents[0][0]
        yc = y.detach().requires_grad_(True)
        b = y.shape[0] // len(feats)
        out = [yc[g * b:(g + 1) * b] for g in range(len(feats))]
        for g, t in enumerate(out):
            t._mdf_parent = (yc, g, len(feats))
        pairs.append((y, yc))
    else:
        out = [f.detach().requires_grad_(True) for f in feats]
        pairs.extend(zip(feats, out))
    cuts.feat.append(pairs)
    return out


def _cached_form(cache, key):
    """None: no pyramid under `key`; else whether the cached pyramid holds pair-difference maps.  (Looks without touching the
    recency order of an LRU cache.)"""
    if key not in cache:
        return None
    entry = dict.get(cache, key) if isinstance(cache, dict) else cache[key]
    return bool(entry[2]) if len(entry) > 2 else False


class CoreNet(torch.nn.Module):
    def __init__(self, Backbone, Depth_hypos, scale, Homoaggre, Regular, Regress, Refine):
        """Backbone: img -> 3 feature maps; Depth_hypos/Homoaggre/Regular: ModuleLists (one per stage);
        scale: callable(K, E, stage); Regress: [depth_regression, confidence_regress]; Refine: module."""
        super().__init__()
        self.Backbone, self.Depth_hypos, self.scale = Backbone, Depth_hypos, scale
        self.Homoaggre, self.Regular, self.Refine = Homoaggre, Regular, Refine
        self.Depth_regress, self.Confidence_regress = Regress
        print("{} parameters: {}".format(self._get_name(), sum(p.data.nelement() for p in self.parameters())))

    def forward(self, origin_imgs, extrinsics, intrinsics, depth_range, feature_cache=None, view_keys=None, stage_tap=None):
        """Same call as the reference (net/core.py:30).  Optional, for whole-scan evaluation: a dict
        `feature_cache` and per-view hashable `view_keys` [V] (batch 1) -- feature pyramids are then computed once per
        image and reused while it serves as a source view of other items; results are identical.
        `stage_tap` (eval mode only; validation, mdfnet_hip/valmetrics.py): a list or a callable that is handed, after every stage,
        {"stage": s, "hypos": the hypotheses the stage was given, "depth": its depth} and, after the refinement net,
        {"stage": "final", "depth": ..., "confidence": ...} -- the tensors the forward holds anyway, nothing is computed for it."""
        if self.training and origin_imgs.is_cuda and layers.hip_train(self, origin_imgs):
            self._check_training_slots()
        with layers.model_mode(self.training):
            plan = None
            if origin_imgs.is_cuda:
                # one device->host hop for the control-plane tensors (cameras, range) when the caller has not registered host
                # mirrors; then every slot's few dozen host-computed floats go up in ONE packed copy (mdfnet_hip/controlplane.py)
                hostmirror.ensure((extrinsics, intrinsics, depth_range))
                plan = controlplane.prepare(self, intrinsics, extrinsics, depth_range)
            with controlplane.active(plan):
                return self._forward(origin_imgs, extrinsics, intrinsics, depth_range, feature_cache, view_keys, stage_tap)

    def _pair_diff_route(self, imgs):
        """True when this forward runs on pair-difference pyramids: eval on a GPU, the built-in FPN_4Scales with the (8,16,32,64)
        pyramid, and EVERY aggregation slot the built-in VectorAggregate with C/G = 2 -- the aggregation then reads a feature pair
        (a, b) only through b - a, and nothing else reads the pyramid (the refinement net takes depth and range).  Any foreign
        slot, variance aggregation or training: full features, as ever."""
        from .unit import backbone as _bb
        from .unit.homoaggregate import VectorAggregate
        bb = self.Backbone
        if not _bb._PAIR_DIFF or self.training or not imgs.is_cuda or type(bb) is not _bb.FPN_4Scales:
            return False
        chans = (bb.out4.out_channels, bb.out3.out_channels, bb.out2.out_channels)
        if chans != (64, 32, 16) or (bb.out4.in_channels, bb.lat3.in_channels, bb.lat2.in_channels) != (64, 32, 16):
            return False
        slots = list(self.Homoaggre)
        return len(slots) == 3 and all(type(a) is VectorAggregate and 2 * a.ngroups == c for a, c in zip(slots, chans))

    def _check_training_slots(self):
        """Training on the GPU runs every stage slot on a hand-written training kernel; a slot that has none (a foreign module
        or function) is refused HERE, when the training forward starts and before anything is launched, by name -- not halfway
        through stage 0 by whichever kernel-less call comes first.  (The stock-op route for such compositions is the rehearsal
        backend, `rehearsal.enable(on_gpu=True)`, under which this check is not reached.)"""
        from .unit.homoaggregate import VectorAggregate, homo_aggregate_by_variance
        from .unit.regular import RegularNet_3Scales, RegularNet_4Scales
        bad = []
        for s, a in enumerate(self.Homoaggre):
            if type(a) is not VectorAggregate and a is not homo_aggregate_by_variance:
                bad.append(f"Homoaggre[{s}] ({getattr(a, '__name__', type(a).__name__)})")
        for s, r in enumerate(self.Regular):
            if type(r) not in (RegularNet_3Scales, RegularNet_4Scales):
                bad.append(f"Regular[{s}] ({type(r).__name__})")
                if getattr(self.Depth_regress, "mdf_builtin", False):
                    bad.append(f"Depth_regress behind the non-fused Regular[{s}] (stand-alone depth_regression)")
        if bad:
            raise RuntimeError("CoreNet.train() on a GPU: no hand-written training kernel for slot(s) " + ", ".join(bad) + "; built-in "
                               "choices are VectorAggregate or homo_aggregate_by_variance, RegularNet_3Scales / RegularNet_4Scales with "
                               "depth_regression.  The stock-op route is the rehearsal backend: `import rehearsal; "
                               "rehearsal.enable(on_gpu=True)`")

    def _pyramids(self, imgs, feature_cache, view_keys, pair_diff=False):
        nb, nv = imgs.shape[:2]
        backbone = (lambda x: self.Backbone(x, pair_diff=True)) if pair_diff else self.Backbone
        if feature_cache is not None and view_keys is not None and nb == 1 and not self.training:
            if hasattr(feature_cache, "pin"):
                feature_cache.pin(view_keys)                             # a bounded cache must keep this item's views
            # (an entry carries the form of its pyramid: one of the other form -- the development switch flipped -- counts as missing)
            missing = [v for v in range(nv) if _cached_form(feature_cache, view_keys[v]) is not pair_diff]
            if missing:
                f = backbone(imgs[0, missing])                           # only the images not seen yet, batched
                ev = torch.cuda.Event()
                ev.record()                                              # on the stream that produced them
                for j, v in enumerate(missing):
                    feature_cache[view_keys[v]] = (tuple(lv[j:j + 1] for lv in f), ev, pair_diff)
            cur = torch.cuda.current_stream(imgs.device)
            out = []
            for v in range(nv):
                pyr, ev = feature_cache[view_keys[v]][:2]
                cur.wait_event(ev)                                       # another item in flight may have produced it
                for t in pyr:
                    t.record_stream(cur)
                out.append(pyr)
            return out
        if self.training and imgs.is_cuda and hasattr(self.Backbone, "forward_views") and layers.hip_train(self.Backbone, imgs):
            return self.Backbone.forward_views(imgs)          # all views in one pass, BatchNorm statistics per view
        if getattr(self.Backbone, "batch_views", False) and not self.training:
            # eval BatchNorm is per-sample: one batched pass over the B*V images == V separate calls (core.py:42)
            f = backbone(imgs.reshape(nb * nv, *imgs.shape[2:]))
            return [tuple(lv.reshape(nb, nv, *lv.shape[1:])[:, v] for lv in f) for v in range(nv)]
        return [backbone(v) for v in torch.unbind(imgs, 1)]

    def _forward(self, origin_imgs, extrinsics, intrinsics, depth_range, feature_cache=None, view_keys=None, stage_tap=None):
        """imgs [B,V,3,H,W] (view 0 = reference), E [B,V,4,4], K [B,V,3,3], range [B,2]
        -> train: {"depth": [1/8, 1/4, 1/2, 1/1]};  eval: {"depth": [B,H,W], "confidence": [B,H,W]}."""
        if not self.training and not origin_imgs.is_cuda:
            raise RuntimeError("CoreNet inference runs on hand-written MI355X kernels only: move the model and inputs to a "
                               "GPU (there is no CPU fallback; model.train() on a GPU runs the hand-written training kernels)")
        if origin_imgs.is_cuda:
            # one device->host hop for the control-plane tensors (cameras, range); the slots then find host
            # mirrors and never synchronise again
            hostmirror.ensure((extrinsics, intrinsics, depth_range))
        if self.training and origin_imgs.is_cuda and layers.hip_train(self, origin_imgs):
            # this step's weight packs (the optimizer has just changed every weight): one batched launch
            from mdfnet_hip import train_ops
            with torch.no_grad():
                train_ops.prepack(self)
        tap = None
        if stage_tap is not None:
            if self.training:
                raise RuntimeError("CoreNet.forward(stage_tap=...) is an eval-mode hook (validation); call model.eval() first")
            tap = stage_tap.append if isinstance(stage_tap, list) else stage_tap
        pair_diff = self._pair_diff_route(origin_imgs)
        pyramids = self._pyramids(origin_imgs.float(), feature_cache, view_keys, pair_diff)
        depth = hypos = prob = None
        depths = []
        # a Confidence_regress slot marked mdf_cascade (regress.confidence_cascade) is called after every stage with the previous
        # stage's confidence (regress.py:20-23); eval only: training computes no confidence
        cascade = not self.training and origin_imgs.is_cuda and getattr(self.Confidence_regress, "mdf_cascade", False)
        conf = None
        last_stage = len(self.Regular) - 1
        # Training on the HIP kernels: every stage's aggregation + regulariser is issued on a stream of its own.  The forward pass
        # gains nothing (stage s+1 needs stage s's depth: the streams are chained by events), but autograd runs a node's backward
        # on the stream of its forward, and the three stages' backward chains do not depend on each other -- the hypotheses are
        # built under no_grad (depthhypos.py:40,188) and the refinement net detaches its input (refine.py:29) -- so they run side
        # by side until they meet at the feature pyramid: the small-volume launches of one stage fill the CUs another leaves idle.
        side = cuts = None
        if self.training and origin_imgs.is_cuda and torch.is_grad_enabled() and layers.hip_train(self, origin_imgs):
            cuts = layers.active_cuts()      # a recorded step that takes the backward pass in pieces (layers.StageCuts)
            # (a hipGraph with parallel branches is replayed node by node by the host -- 6.5 ms per cfg3 step --, so a recording
            #  keeps one stream unless it cuts the stage chains out into graphs of their own)
            if cuts is not None or (_STAGE_STREAMS and not torch.cuda.is_current_stream_capturing()):
                side = _stage_streams(origin_imgs.device, len(self.Regular))
                main = torch.cuda.current_stream(origin_imgs.device)
                if cuts is not None:
                    cuts.streams = side
        for stage, (make_hypos, aggregate, regular) in enumerate(zip(self.Depth_hypos, self.Homoaggre, self.Regular)):
            feats = [p[stage] for p in pyramids]
            if cuts is not None:
                feats = _cut_features(feats, cuts)
            ref_proj, src_projs = self.scale(intrinsics, extrinsics, stage)
            with _on_stage_stream(side, stage, main if side else None, feats):
                hypos = make_hypos(depth, depth_range, prob, hypos, upsample=True)
                # (pair_diff: the pyramids hold f[2g+1] - f[2g]; said explicitly, not inferred from the channel count)
                cost = aggregate(feats, ref_proj, src_projs, hypos, pair_diff=True) if pair_diff else aggregate(feats, ref_proj, src_projs, hypos)
                if ((not self.training or cost.is_cuda) and getattr(regular, "fused_regress", False)
                        and getattr(self.Depth_regress, "mdf_builtin", False)):
                    # both slots are the built-in ones: the soft-argmin (core.py:64) rides in the regulariser's softmax kernel
                    # (same arithmetic as the standalone slot, asserted equal in tests/test_regular_gpu.py)
                    prob, depth = regular(cost, hypos)
                else:
                    prob = regular(cost)
                    depth = self.Depth_regress(prob, hypos)
            if side:
                # produced on the stage's stream; read by the next stage's stream and by the caller's (loss, refinement net)
                for t in (hypos, prob, depth):
                    t.record_stream(main)
                    if stage + 1 < len(side):
                        t.record_stream(side[stage + 1])
            if cuts is not None:
                cut = depth.detach().requires_grad_(True)
                cuts.depth.append((depth, cut))
                depth = cut
            depths.append(depth)
            if tap is not None:
                tap({"stage": stage, "hypos": hypos, "depth": depth})
            if cascade:
                # (the last stage's call carries the nearest x2 of core.py:76: one launch, as on the default path)
                conf = self.Confidence_regress(prob, last_confidence=conf, up2=stage == last_stage)
        depth = self.Refine(depth, depth_range)
        if cuts is not None and depth.requires_grad:
            cut = depth.detach().requires_grad_(True)       # the refinement net's backward (parameters only: refine.py:29 detaches
            cuts.refine = (depth, cut)                      # its input) is a piece of its own, replayed beside the stage chains
            depth = cut
        depths.append(depth)
        if self.training:
            return {"depth": depths}
        if cascade:
            if tap is not None:
                tap({"stage": "final", "depth": depth, "confidence": conf})
            return {"depth": depth, "confidence": conf}
        if getattr(self.Confidence_regress, "mdf_builtin", False) and prob.is_cuda:
            conf = ops.confidence_up2(prob.detach())          # regress.py:9-25 + the nearest x2 of core.py:76 in one launch
        else:
            conf = self.Confidence_regress(prob)
            conf = torch.nn.functional.interpolate(conf.unsqueeze(1), scale_factor=2, mode="nearest").squeeze(1)
        if tap is not None:
            tap({"stage": "final", "depth": depth, "confidence": conf})
        return {"depth": depth, "confidence": conf}
