"""Configuration + model composition (counterpart of the reference's config.py, which cannot travel).

Same public names (Args classes, LoadDTU/LoadBlendedMVS/LoadTanks, `model`) and the same composition as
config.py:186-218, so a reference-style `train.py` / `eval.py` keeps working.  Differences, all deliberate:
  * dataset / output roots come from the environment (MDF_DATA_ROOT, MDF_OUTPUT_ROOT) instead of /hy-tmp;
  * the visible-device list is left to the launcher (one process per GPU) instead of being forced to 0..7;
  * `build_model()` is exposed so callers can build further instances; the module-level singleton `model`
    is kept (train.py:13, eval.py:12 use it).
"""
import logging
import os
import random
import warnings

import numpy
import torch
import torch.nn as nn

warnings.filterwarnings("ignore")
logging.basicConfig(level=logging.INFO, format="%(asctime)s-%(levelname)s: %(message)s")

seed_id = 1
random.seed(seed_id)
numpy.random.seed(seed_id)
torch.manual_seed(seed_id)

DATA_ROOT = os.environ.get("MDF_DATA_ROOT", "/hy-tmp")
OUTPUT_ROOT = os.environ.get("MDF_OUTPUT_ROOT", os.path.join(DATA_ROOT, "outputs"))


class Args:
    def show_args(self):
        print(self.__class__.__name__ + ":")
        for k, v in self.__dict__.items():
            print("\t" + k, ":", v)

    def get_device(self, parallel):
        """One process per GPU: the device is this rank's (LOCAL_RANK), never a device list."""
        if torch.cuda.is_available():
            torch.cuda.manual_seed(seed_id)
            # (MDF_SHARE_GPU: rehearsal knob for a 1-GPU box -- every rank on card 0; never set in production)
            return torch.device("cuda", 0 if os.environ.get("MDF_SHARE_GPU") else int(os.environ.get("LOCAL_RANK", "0")))
        return torch.device("cpu")


class _TrainBase(Args):
    def __init__(self, batch_size, nworks):
        self.nviews, self.robust = 5, True
        self.start_epoch, self.max_epoch = 1, int(os.environ.get("MDF_MAX_EPOCH", "30"))
        self.batch_size, self.nworks = batch_size, nworks
        self.lr, self.factor = 1e-3, 0.9
        self.pth_path = os.environ.get("MDF_PTH_PATH", "pth")
        os.makedirs(self.pth_path, exist_ok=True)
        self.parallel = True   # data parallel = one process per GPU + RCCL all-reduce (not nn.DataParallel)
        self.DEVICE = self.get_device(self.parallel)
        self.show_args()


class TrainArgs(_TrainBase):          # config.py:47-66
    def __init__(self):
        super().__init__(batch_size=4, nworks=2)


class BlendedMVSArgs(_TrainBase):     # config.py:72-89
    def __init__(self):
        super().__init__(batch_size=6, nworks=3)


class EvalArgs(Args):                 # config.py:95-101
    def __init__(self):
        self.output_path = OUTPUT_ROOT
        os.makedirs(self.output_path, exist_ok=True)
        self.parallel = False
        self.DEVICE = self.get_device(self.parallel)


class EvalDTU(EvalArgs):              # config.py:104-111
    def __init__(self):
        super().__init__()
        self.batch_size, self.nworks, self.nviews = 1, 1, 5
        self.show_args()


class EvalTanks(EvalArgs):            # config.py:114-121
    def __init__(self):
        super().__init__()
        self.batch_size, self.nworks, self.nviews = 1, 1, 11
        self.show_args()


def _scan_ids(spec):
    """ "2 6-8 14" -> [2, 6, 7, 8, 14] """
    out = []
    for tok in spec.split():
        lo, _, hi = tok.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


class DatasetsArgs(Args):
    def __init__(self):
        self.root_dir = DATA_ROOT


class LoadDTU(DatasetsArgs):          # config.py:131-152
    def __init__(self):
        super().__init__()
        self.train_root = os.path.join(self.root_dir, "dtu640x512")
        self.train_pair = os.path.join(self.train_root, "Cameras", "pair.txt")
        self.train_label = _scan_ids("2 6-8 14 16 18-20 22 30-31 36 39 41-42 44-47 50-53 55 57-58 60-61 63-65 68-72 74 76 83-85 87-105 107-109 111-113 115-116 119-128")   # the 79 DTU training scans
        self.train_lighting_label = list(range(7))
        self.train_robust = True
        self.val_label = _scan_ids("3 5 17 21 28 35 37 38 40 43 56 59 66 67 82 86 106 117")   # the 18 DTU validation scans (validate.py, train.py --val_every)
        self.val_lighting_label = [3]
        self.eval_root = os.path.join(self.root_dir, "dtu1600x1200")
        self.eval_pair = os.path.join(self.eval_root, "pair.txt")
        self.eval_label = [int(s) for s in os.environ.get("MDF_DTU_SCANS", "11").split(",")]
        self.show_args()


class LoadBlendedMVS(DatasetsArgs):   # config.py:158-163
    def __init__(self):
        super().__init__()
        self.train_root = os.path.join(self.root_dir, "blendedmvs768x576")
        self.show_args()


class LoadTanks(DatasetsArgs):        # config.py:169-180
    def __init__(self, tanks_set="intermediate"):
        super().__init__()
        self.eval_root = os.path.join(self.root_dir, "TankandTemples", tanks_set)
        self.scenelist = {"intermediate": ["Family", "Francis", "Horse", "Lighthouse", "M60", "Panther", "Playground",
                                           "Train"],
                          "advanced": ["Auditorium", "Ballroom", "Courtroom", "Museum", "Temple", "Palace"]}[tanks_set]
        self.show_args()


class LoadScene(DatasetsArgs):        # imported scenes (tools/colmap/main.py); no reference counterpart
    def __init__(self, scene_root=None, scenes=()):
        super().__init__()
        self.eval_root = scene_root or os.path.join(self.root_dir, "scenes")
        self.scenelist = list(scenes)
        self.show_args()


class EvalScene(EvalArgs):
    def __init__(self, nviews=5):
        super().__init__()
        self.batch_size, self.nworks, self.nviews = 1, 1, nviews
        self.show_args()


# ----------------------------------------------------------------------------- net args (config.py:186-218)
from net import core  # noqa: E402
from net.unit import scale as _scale, backbone, regress, refine  # noqa: E402
from net.unit.depthhypos import HyposByFit  # noqa: E402
from net.unit.homoaggregate import VectorAggregate  # noqa: E402
from net.unit.regular import RegularNet_4Scales, RegularNet_3Scales  # noqa: E402

stages = 4
scale = _scale.scale_cam
chs = (8, 16, 32, 64)
ndepths = (48, 24, 8)
curve_calss = [None, "gauss1", "laplace"]
prob_thresh = (0.0, 0.95, 1e-5)
ngroups = (32, 16, 8)


AGGREGATES = ("vector", "variance")
CURVES = ("gauss0", "gauss1", "laplace", "atv")
atv_scale = (1.5, 1.5)               # UCS-Net's lamb, for a stage whose curve is "atv"
CONFIDENCES = ("last", "cascade")


def parse_pair(text, kind):
    """ "gauss1,laplace" -> ("gauss1", "laplace");  "0.95,1e-5" with kind=float -> (0.95, 1e-05)  (train.py / eval.py flags)."""
    parts = [p.strip() for p in text.split(",")]
    if len(parts) != 2:
        raise ValueError(f"expected two comma-separated values (stage 1, stage 2), got {text!r}")
    return tuple(kind(p) for p in parts)


def _curve_args(curves, thresh):
    """-> per-stage (curve_calss, prob_thresh) lists of the three HyposByFit slots, checked."""
    curves = tuple(curve_calss[1:]) if curves is None else tuple(curves)
    thresh = tuple(prob_thresh[1:]) if thresh is None else tuple(thresh)
    if len(curves) != 2 or any(c not in CURVES for c in curves):
        raise ValueError(f"curves={curves!r}: a pair (stage 1, stage 2) out of {CURVES}")
    if len(thresh) != 2:
        raise ValueError(f"prob_thresh={thresh!r}: a pair (stage 1, stage 2)")
    for c, t in zip(curves, thresh):
        # the hypothesis range is sqrt(-s ln t) (Gaussian) or |s ln t| (Laplace): t must lie inside (0, 1)
        if not 0.0 < float(t) < 1.0:
            raise ValueError(f"prob_thresh={t!r} for curve {c!r}: the threshold must lie in (0, 1)")
    return [None] + list(curves), [0.0] + [float(t) for t in thresh]


def _atv_args(scales):
    """-> per-stage atv_scale list of the three HyposByFit slots, checked (read only by a slot whose curve is "atv")."""
    scales = atv_scale if scales is None else scales
    try:
        scales = tuple(float(v) for v in scales)
    except TypeError:
        raise ValueError(f"atv_scale={scales!r}: a pair (stage 1, stage 2)") from None
    if len(scales) != 2 or not all(0.0 < v < float("inf") for v in scales):
        raise ValueError(f"atv_scale={scales!r}: a pair (stage 1, stage 2) of finite values greater than 0")
    return [1.5] + list(scales)


REGULAR_STRIDES = {(2, 2, 2): (1, 1, 1), (1, 2, 2): (0, 1, 1)}     # sample_stride -> sample_padding of the RegularNet_4Scales slots


def parse_stride(text):
    """ "1,2,2" -> (1, 2, 2)  (the --regular_stride flag of eval.py / validate.py), checked."""
    try:
        stride = tuple(int(p) for p in text.split(","))
    except ValueError:
        stride = None
    if stride not in REGULAR_STRIDES:
        raise ValueError(f"regular_stride={text!r}: choose one of {['%d,%d,%d' % s for s in REGULAR_STRIDES]}")
    return stride


def _regular_stride_args(stride):
    """-> (sample_stride, sample_padding) of the two RegularNet_4Scales slots, checked."""
    try:
        stride = tuple(int(v) for v in stride)
    except (TypeError, ValueError):
        raise ValueError(f"regular_stride={stride!r}: choose one of {tuple(REGULAR_STRIDES)}") from None
    if stride not in REGULAR_STRIDES:
        raise ValueError(f"regular_stride={stride!r}: choose one of {tuple(REGULAR_STRIDES)}")
    return stride, REGULAR_STRIDES[stride]


def build_model(aggregate="vector", curves=None, prob_thresh=None, confidence="last", atv_scale=None, regular_stride=(2, 2, 2)):
    """A fresh CoreNet.  curves: the curve HyposByFit fits before stages 1 and 2, default ("gauss1", "laplace"); prob_thresh: their
    thresholds, default (0.95, 1e-5).  "atv" in a stage is the adaptive-thin-volume range of the reference's atv_hypos instead of a
    curve fit: it reads atv_scale (a pair, default (1.5, 1.5), each finite and > 0) and ignores its prob_thresh (still checked); its
    hypotheses are not clamped to the depth range.  Every choice has the same state_dict (the slot has no parameters), so one checkpoint loads
    into all of them; which curves it was trained with is the caller's to keep.  aggregate="vector" (default): composed exactly like the reference's singleton.  aggregate="variance":
    the classic MVSNet variance cost volume in the Homoaggre slots (homo_aggregate_by_variance, homoaggregate.py:49-69), whose
    cost volume has the C = 2 G feature channels, so the regularisers' first layers are 64->16, 32->8, 16->8.  That model has no
    `Homoaggre.*` parameters and differently shaped `Regular.{0,1,2}.conv01` first layers: reference checkpoints (and those of
    the vector model) do not load into it.  confidence="last" (default): the confidence map comes from the last stage's probability
    volume alone, as the reference's config composes it.  confidence="cascade": regress.confidence_cascade in the slot -- every stage
    blends 0.8 * bicubic x2 of the previous stage's confidence with 0.2 of its own (regress.py:20-23), eval only; the slot has no
    parameters, so the state_dict is the same.  regular_stride=(2,2,2) (default): the reference's composition.  regular_stride=(1,2,2):
    both RegularNet_4Scales slots (stages 1 and 2) are composed with sample_stride (1,2,2), sample_padding (0,1,1) -- the alternative
    the reference names at regular.py:76-77: the U-Net halves H and W and keeps every depth plane.  Same state_dict (3x3x3 kernels
    either way): a checkpoint trained with the reference's (1,2,2) composition loads strictly; one trained for (2,2,2) loads too but
    was not trained for it.  Eval only on the GPU.  RegularNet_3Scales (stage 0) has no such option in the reference."""
    if aggregate not in AGGREGATES:
        raise ValueError(f"aggregate={aggregate!r}: choose one of {AGGREGATES}")
    if confidence not in CONFIDENCES:
        raise ValueError(f"confidence={confidence!r}: choose one of {CONFIDENCES}")
    cv, th = _curve_args(curves, prob_thresh)
    sc = _atv_args(atv_scale)
    rs, rp = _regular_stride_args(regular_stride)
    hypos = nn.ModuleList([HyposByFit(ndepths[i], cv[i], th[i], atv_scale=sc[i]) for i in range(stages - 1)])
    if aggregate == "variance":
        from net.unit.homoaggregate import homo_aggregate_by_variance
        aggre = [homo_aggregate_by_variance] * (stages - 1)
        in_chs = tuple(2 * g for g in ngroups)          # (64, 32, 16): the feature channels of the three stages
    else:
        aggre = nn.ModuleList([VectorAggregate(ngroups[i]) for i in range(stages - 1)])
        in_chs = ngroups
    regular = nn.ModuleList([RegularNet_3Scales(in_chs[0])] + [RegularNet_4Scales(c, sample_stride=rs, sample_padding=rp) for c in in_chs[1:]])
    return core.CoreNet(backbone.FPN_4Scales(chs), hypos, scale, aggre, regular,
                        [regress.depth_regression, regress.confidence_cascade if confidence == "cascade" else regress.confidence_regress],
                        refine.RefineNet2())


model = build_model()
