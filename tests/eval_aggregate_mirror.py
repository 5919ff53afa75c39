"""TEST INFRASTRUCTURE (CPU, torch float64): the reference, the launch-route mirror and the case table of the EVAL plane-sweep kernels
(csrc/warp_aggregate.hip: warp_kernel<C, kWarp|kVec|kVar>, warp_vec8_kernel, warp_pairdiff_kernel<G,GPL,FIXED>, warp_vec_win_kernel,
corner_index_kernel; the fill_taps / FixedPairs / softmax helpers of csrc/warp_common.h).  The training twin is tests/aggregate_mirror.py,
whose sample positions, gather, special-function model and metrics are imported here, not copied.
tests/test_eval_aggregate_mirror_cpu.py asserts the preconditions on the CPU, tests/test_eval_aggregate_gpu.py compares the kernels.

REFERENCE.  `run_eval(inp, mode, dtype)` evaluates one of the four operators AT THE KERNELS' fp32 SAMPLE POSITIONS (aggregate_mirror.positions,
cast to `dtype`); everything behind the positions follows in `dtype`.  A sample whose position is not finite (a z == 0 plane) is NaN in
every channel, as grid_sample and the kernels make it (a NaN / inf coordinate gives NaN weights, and NaN * 0 stays NaN).
  vec       VectorAggregate in eval mode (homoaggregate.py:25-46) with the BatchNorm folded as ops.fold_view_weight folds it:
            sim = sum_pair softmax(ref) softmax(warped), z = sum_g cw_g sim_g, u = relu(z alpha + beta) w2 + b2, wv = sigmoid(u),
            cost = sum_v wv sim / sum_v wv.
  pairdiff  the same fed pair-difference maps d = f[:,1::2] - f[:,0::2] (formed ONCE in fp32 and handed to kernel and mirror alike as
            data): p0 = 1 / (1 + exp(blend(d))).
  var       homo_aggregate_by_variance (homoaggregate.py:49-69): s1 = ref + sum_v p_v, s2 = ref^2 + sum_v p_v^2 with p_v = softmax over
            all C channels of the warped sample, n = n_src + 1, var = s2 / n - (s1 / n)^2.
  warp      the blended sample of view 0 (no bar: the kernel owes the bits of oracle.homo_warping_explicit).
dtype = float32 is the "fp32 restatement": what fp32 arithmetic owes at the case.

THE BAR.  e_hip <= 1.5 e_32 + t per quantity and metric (max|d| / max|ref| and relative L2 over the finite voxels; for `var` also
max |d| / A per element), e_x = the distance of x from the float64 run, t derived from the float64 reference alone:
  t_special  2 x the largest displacement over PERTURB_DRAWS float64 re-runs with every v_exp_f32 / v_rcp_f32 moved by 1 ulp and the
             log2(e) product by u (aggregate_mirror._Perturb); for `var` the C-wide softmax uses expf, modelled at 1 ulp, and an IEEE divide
             (the restatement's own, not perturbed).
  t_order    0 for vec and pairdiff: the forward has no sums beyond the groups of a pixel and the views (aggregate_mirror's docstring).
  var        E[p^2] - mean^2 cancels: acc and acc2 are n_src + 1 terms added in fp32 (n_src roundings each), the two quotients, the
             square and the difference one rounding each: at most (n_src + 3) u (E[p^2] + mean^2) =: (n_src + 3) u A per element.  The
             term enters the max and L2 metrics scaled by max A / max|ref| and |A| / |ref|, and every element is also judged against
             its own A (the perA metric of aggregate_mirror.ACCUMULATED).

ROUTES.  `plan_eval(dims, kernel)` restates the launchers' host arithmetic: pixels per block, planes per chunk, LDS bytes, refused
(-> the fallback of the entry point), the FixedPairs form (few / two / generic) with its thread groups, and the chunk walk.
The constants are compared with the sources by tests/test_eval_aggregate_mirror_cpu.py.
"""
import math
import os
import sys
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import aggregate_mirror as M  # noqa: E402
from aggregate_mirror import (PERTURB_DRAWS, U, ULP, _clear_grid_lines, _exact_projection, _near_lines, _Perturb, distances,  # noqa: E402,F401
                              fixed_pairs_usable, positions, warp_at)
from oracle import mvs_oracle as O  # noqa: E402

# ---- constants of the eval launchers (held against the sources by test_constants_are_the_sources)
K_THREADS = M.K_THREADS
MAX_SRC_VIEWS = M.MAX_SRC_VIEWS
WARP_TAB = 512                 # launch<MODE> and launch_win: 512 / (n_src * ppb) planes per chunk
VEC8_TAB = 1024                # MDF_VEC8_TAB: launch_vec8 and launch_pairdiff
TAP_ENTRY_BYTES = 32           # sizeof(TapEntry) == sizeof(TapXY)
LDS_LIMIT = 64 * 1024          # launch_vec8 / launch_pairdiff refuse beyond it
WIN_LDS_LIMIT = 150 * 1024     # launch_win
WIN_POOL_KB = 64
KERNELS = ("warp_kernel", "vec8", "pairdiff4", "pairdiff8", "win")
LAUNCH_NAME = {"warp_kernel": "warp_kernel", "vec8": "warp_vec8_kernel", "pairdiff4": "warp_pairdiff_kernel", "pairdiff8": "warp_pairdiff_kernel",
               "win": "warp_vec_win_kernel"}

# ==================================================================================================================== case table
# id -> (h, w, C, n_src, D, B, per_pixel, cameras): the issue's table, no shape adjusted (test_table_reaches_every_route holds every row)
CASES = {
    "min": (2, 2, 64, 1, 1, 1, False, "real"),
    "v16c64": (5, 7, 64, 16, 3, 1, True, "real"),
    "v16c16": (5, 7, 16, 16, 3, 2, True, "real"),
    "fix4c64": (7, 9, 64, 4, 45, 2, False, "real"),
    "p4c32": (9, 31, 32, 4, 7, 2, True, "real"),
    "p4c16": (6, 33, 16, 4, 8, 1, True, "real"),
    "s2c16": (6, 33, 16, 2, 9, 1, False, "real"),
    "gen3": (13, 11, 32, 3, 24, 2, True, "real"),
    "n8c32": (5, 7, 32, 8, 5, 1, False, "real"),
    "n5c64": (9, 31, 64, 5, 7, 2, False, "real"),
    "ident16": (8, 16, 16, 2, 5, 1, False, "ident"),
    "ident64": (8, 16, 64, 2, 5, 1, False, "ident"),
    "half16": (8, 16, 16, 2, 5, 1, False, "half"),
    "half64": (8, 16, 64, 2, 5, 1, False, "half"),
    "mag32": (17, 17, 32, 2, 5, 1, True, "mag"),
    "gone": (6, 33, 16, 2, 8, 1, True, "gone"),
    "z0": (12, 20, 32, 2, 5, 1, False, "z0"),
}
# seeds chosen so that (a) _clear_grid_lines clears every real / gone / mag case (test_no_sample_near_a_grid_line) and (b) the head is
# LIVE (test_the_head_is_live): sim stays near 0.5, so z = sum cw sim varies little and with most draws of the head parameters the
# ReLU is on for every sample or for none -- and a dead ReLU hides alpha, beta, w2 and cw from the cost altogether (at seed 1 the bar
# did not notice alpha used for w2 on fix4c64).  Each seed is the first at which both ReLU branches occur and the view weights spread.
SEEDS = {"min": 5, "v16c64": 10, "v16c16": 6, "fix4c64": 21, "p4c32": 2, "p4c16": 3, "s2c16": 26, "gen3": 3, "n8c32": 60, "n5c64": 6,
         "ident16": 1, "ident64": 17, "half16": 59, "half64": 2, "mag32": 117, "gone": 52, "z0": 41}
HEAD_LIVE = (0.05, 0.95, 0.04)     # the ReLU is on for this share of the samples at least / at most; max - min of the view weights at least
REAL_CAMERA_CASES = [k for k, c in CASES.items() if c[7] == "real"]
EXACT_LINE_CASES = ("ident16", "ident64", "half16", "half64")
VAR_CASES = ("min", "v16c64", "v16c16", "gen3", "p4c32", "s2c16", "half16", "gone", "z0")
MODES = ("vec", "pairdiff", "var", "warp")
QUANTITY = {"vec": "cost", "pairdiff": "cost", "var": "var", "warp": "warp"}
GRID_MARGIN = M.GRID_MARGIN


def _gen(case_id):
    return torch.Generator().manual_seed(7000 + 1000 * SEEDS[case_id] + sorted(CASES).index(case_id))


def inputs(case_id):
    """The fp32 inputs of a case, by the training mirror's conventions: features randn, cw = kaiming-uniform + 0.3 randn, the head's
    BatchNorm / conv parameters = the module's initial values + 0.3 randn (the running variance U(0.5, 1.5)), folded into
    wpar = (cw[G], alpha, beta, w2, b2) by ops.fold_view_weight -- O(1) constants, so that an error anywhere in the head moves the cost."""
    from mdfnet_hip import ops
    h, w, c, n_src, d, b, per_pixel, cams = CASES[case_id]
    g = c // 2
    gen = _gen(case_id)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    ur = lambda *s: torch.rand(*s, generator=gen) * 2 - 1  # noqa: E731
    ref = rn(b, c, h, w)
    srcs = [rn(b, c, h, w) for _ in range(n_src)]
    cw = ur(g) / math.sqrt(g) + 0.3 * rn(g)                      # nn.Conv3d(G, 1, 1): kaiming_uniform(a = sqrt 5) = U(+-1/sqrt(fan_in))
    head = {"depth_weight.0.conv.weight": cw.reshape(1, g, 1, 1, 1), "depth_weight.0.bn.weight": 1.0 + 0.3 * rn(1),
            "depth_weight.0.bn.bias": 0.3 * rn(1), "depth_weight.0.bn.running_mean": 0.3 * rn(1),
            "depth_weight.0.bn.running_var": torch.rand(1, generator=gen) + 0.5,
            "depth_weight.0.bn.num_batches_tracked": torch.zeros((), dtype=torch.int64),
            "depth_weight.1.weight": (ur(1) + 0.3 * rn(1)).reshape(1, 1, 1, 1, 1), "depth_weight.1.bias": ur(1) + 0.3 * rn(1)}
    wpar = ops.fold_view_weight(head, g)
    cam = None
    if cams in ("real", "gone"):
        from mdfnet_hip import synth
        intr, extr, _ = synth.make_cameras(w, h, n_src + 1, batch=b, rot_deg=2.0, seed=SEEDS[case_id] + 7)
        rp, sps = O.scale_cam(intr, extr, 3)
        proj = torch.stack([O.relative_projection(sp, rp)[:, :3, :4] for sp in sps]).contiguous()
        if per_pixel:
            hyp = (425 + 510 * torch.rand(b, 1, h, w, generator=gen)) + torch.linspace(-20, 20, d).reshape(1, d, 1, 1)
        else:
            hyp = torch.stack([torch.linspace(425 + 9 * i, 935 - 5 * i, d) for i in range(b)]).reshape(b, d, 1, 1)
        if cams == "gone":
            proj[1, :, 0, 3] += 1.0e6                            # view 1: ~1000 pixels off the frame at every plane
        else:
            cam = (rp, sps)
    elif cams == "mag":                                          # aggregate_mirror's: many pixels on one texel, small window boxes
        proj = torch.eye(4)[:3].repeat(2, 1, 1, 1)
        proj[0, 0, :, 3] = torch.tensor([0.0, 0.0, -420.0])
        proj[1, 0, :, 3] = torch.tensor([10.0, -5.0, -400.0])
        hyp = 500 + 300 * torch.rand(b, d, h, w, generator=gen)
    elif cams == "z0":
        # the cameras of tests/test_pairdiff_gpu.py:test_kernel_out_of_frame_and_degenerate_planes (reference projection = identity).
        # View 0: z = depth - 600, zero on the 600 plane (NaN) and negative below it, x runs out of frame; view 1: z = depth - 300, half in frame
        proj = torch.eye(4)[:3].repeat(2, 1, 1, 1)
        proj[0, 0, :, 3] = torch.tensor([3.0, -2.0, -600.0])
        proj[1, 0, :, 3] = torch.tensor([-100.0, 50.0, -300.0])
        hyp = torch.tensor([500.0, 600.0, 700.0, 650.0, 610.0]).reshape(1, 5, 1, 1)
    else:
        shifts = {"ident": [(0.0, 0.0), (0.0, 0.0)], "half": [(0.5, 0.0), (-0.5, -0.5)]}[cams]
        proj = torch.stack([_exact_projection(h, w, sx, sy) for sx, sy in shifts]).unsqueeze(1).contiguous()
        hyp = torch.linspace(512, 1024, d).reshape(1, d, 1, 1)
    pd = lambda f: (f[:, 1::2] - f[:, 0::2]).contiguous()  # noqa: E731
    inp = NS(id=case_id, ref=ref, srcs=srcs, dref=pd(ref), dsrcs=[pd(s) for s in srcs], proj=proj.float().contiguous(),
             hyp=hyp.float().contiguous(), per_pixel=per_pixel, head=head, wpar=wpar, cam=cam, dims=(b, c, g, d, h, w, n_src))
    if cams in ("real", "gone", "mag", "z0"):                    # (z0: the NaN plane has no sample near anything and stays at 600)
        _clear_grid_lines(inp)
    return inp


def projections_4x4(inp):
    """(ref_proj, [src_proj]) whose oracle.relative_projection is inp.proj exactly: the identity and the 3 x 4 rows under (0,0,0,1)."""
    b = inp.dims[0]
    eye = torch.eye(4).repeat(b, 1, 1)
    out = []
    for v in range(inp.dims[6]):
        m = eye.clone()
        m[:, :3, :4] = inp.proj[v]
        out.append(m)
    return eye, out


# ==================================================================================================================== the reference
class _PerturbEval(_Perturb):
    """aggregate_mirror._Perturb plus the C-wide softmax of softmax_pixel: expf at 1 ulp, exact maximum, an IEEE divide."""

    def softmax_all(self, x, dim):
        e = torch.exp(x - x.amax(dim, keepdim=True))
        e = e * (1 + ULP * self.sign(e))
        return e / e.sum(dim, keepdim=True)


def sample(src_fea, ix, iy):
    """aggregate_mirror.warp_at, with NaN in every channel where the position is not finite."""
    b, c, h, w = src_fea.shape
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    off = torch.full_like(ix, -8.0)                              # anywhere out of frame: the value is replaced below
    vol = warp_at(src_fea, torch.where(fin, ix, off), torch.where(fin, iy, off))
    nan = torch.full((), float("nan"), dtype=vol.dtype)
    return torch.where(fin.reshape(b, 1, ix.shape[1], h, w), vol, nan)


def run_eval(inp, mode, dtype=torch.float64, perturb=None, fault=None):
    """One operator at the kernels' positions in `dtype` -> float64 on the CPU in the kernels' layouts: cost [B,D,h,w,G] / var [B,D,h,w,C]
    (NDHWC) / warp [B,C,D,h,w], and the per-sample intermediates sim [n_src,B,D,h,w,G], z, u, wv [n_src,B,D,h,w], wsum [B,D,h,w].
    perturb = a seed: the special-function model (float64 only).  fault: a deliberate error for the sensitivity test of the CPU suite
    ("wsum_skips_a_view": the last view's weight is left out of wsum; "var_divisor": n_src instead of n_src + 1)."""
    b, c, g, d, h, w, n_src = inp.dims
    pos = positions(inp)
    pt = _PerturbEval(perturb) if perturb is not None else None
    assert pt is None or dtype == torch.float64
    assert mode in MODES and fault in (None, "wsum_skips_a_view", "var_divisor")
    cast = lambda t: t.detach().to(dtype)  # noqa: E731
    f64 = lambda x: x.detach().double()  # noqa: E731
    ndhwc = lambda x: f64(x).permute(0, 2, 3, 4, 1).contiguous()  # noqa: E731
    out = NS(dims=inp.dims, mode=mode)
    with O.precision(dtype), torch.no_grad():
        xy = [(ix.to(dtype), iy.to(dtype)) for ix, iy in pos]
        if mode == "warp":
            out.warp = f64(sample(cast(inp.srcs[0]), *xy[0]))
            return out
        if mode == "var":
            ref = cast(inp.ref).unsqueeze(2)
            s1, s2 = ref, ref ** 2
            for v in range(n_src):
                vol = sample(cast(inp.srcs[v]), *xy[v])
                p = pt.softmax_all(vol, 1) if pt else F.softmax(vol, dim=1)
                s1 = s1 + p
                s2 = s2 + p ** 2
            n = n_src if fault == "var_divisor" else n_src + 1
            out.var = ndhwc(s2 / n - (s1 / n) ** 2)
            out.var_mag = ndhwc(s2 / n + (s1 / n) ** 2)          # A = E[p^2] + mean^2: what the difference cancels
            return out
        wpar = cast(inp.wpar)
        cw, alpha, beta, w2, b2 = wpar[:g], wpar[g], wpar[g + 1], wpar[g + 2], wpar[g + 3]
        if mode == "vec":
            refp = cast(inp.ref).reshape(b, g, 2, 1, h, w)
            r0 = (pt.softmax_pair(refp, 2) if pt else F.softmax(refp, dim=2))
        else:
            x = cast(inp.dref).reshape(b, g, 1, h, w)
            r0 = pt.logistic(-x) if pt else 1 / (1 + torch.exp(x))
        num, den = 0.0, 0.0
        sims, zs, us, wvs = [], [], [], []
        for v in range(n_src):
            if mode == "vec":
                volp = sample(cast(inp.srcs[v]), *xy[v]).reshape(b, g, 2, d, h, w)
                q = pt.softmax_pair(volp, 2) if pt else F.softmax(volp, dim=2)
                sim = (q * r0).sum(dim=2)
            else:
                dv = sample(cast(inp.dsrcs[v]), *xy[v])
                p0 = pt.logistic(-dv) if pt else 1 / (1 + torch.exp(dv))
                sim = p0 * r0 + (1 - p0) * (1 - r0)
            z = F.conv3d(sim, cw.reshape(1, g, 1, 1, 1))
            u = F.relu(z * alpha + beta) * w2 + b2
            wv = pt.logistic(u) if pt else torch.sigmoid(u)
            if not (fault == "wsum_skips_a_view" and v == n_src - 1):
                den = den + wv
            num = num + wv * sim
            sims.append(ndhwc(sim))
            zs.append(f64(z).reshape(b, d, h, w))
            us.append(f64(u).reshape(b, d, h, w))
            wvs.append(f64(wv).reshape(b, d, h, w))
        out.cost = ndhwc(num / den)
        out.wsum = f64(den).reshape(b, d, h, w)
        out.sim, out.z, out.u, out.wv = torch.stack(sims), torch.stack(zs), torch.stack(us), torch.stack(wvs)
    return out


def nan_mask(res, mode):
    return torch.isnan(getattr(res, QUANTITY[mode]))


def distances_eval(got, ref64, mode):
    """{metric: value} of `got` (a run_eval result, or NS(<quantity>=kernel output in the same layout)) from the float64 reference over
    the voxels where the reference is finite (the NaN masks are compared separately, exactly).  aggregate_mirror.distances' max and L2
    metrics; for `var` also perA = max |d| / A per element."""
    name = QUANTITY[mode]
    r = getattr(ref64, name)
    ok = ~torch.isnan(r)
    a = getattr(got, name).double()
    out = distances(NS(**{name: a[ok]}), NS(**{name: r[ok]}), name)
    if mode == "var":
        out["perA"] = float(((a[ok] - r[ok]).abs() / ref64.var_mag[ok]).max())
    return out


def perturbed_runs(inp, mode):
    return [run_eval(inp, mode, torch.float64, perturb=17 + i) for i in range(PERTURB_DRAWS)]


def derived_t(inp, mode, ref64, perturbed):
    """{metric: t} of the mode's quantity (module docstring), from the float64 reference and its perturbed re-runs alone."""
    n_src = inp.dims[6]
    t = {}
    for pr in perturbed:
        for k, v in distances_eval(pr, ref64, mode).items():
            t[k] = max(t.get(k, 0.0), 2.0 * v)
    if mode == "var":
        r, mag = ref64.var, ref64.var_mag
        ok = ~torch.isnan(r)
        rel = (n_src + 3) * U
        t["max"] += rel * float(mag[ok].max() / r[ok].abs().max().clamp(min=1e-300))
        t["l2"] += rel * float(mag[ok].norm() / r[ok].norm().clamp(min=1e-300))
        t["perA"] += rel
    return t


def judge(e_hip, e_32, t):
    """-> [(metric, e_hip, e_32, t, ratio)] of the metrics that miss e_hip <= 1.5 e_32 + t."""
    fails = []
    for k, eh in e_hip.items():
        bar = 1.5 * e_32[k] + t[k]
        if not eh <= bar:
            fails.append((k, eh, e_32[k], t[k], eh / bar if bar > 0 else float("inf")))
    return fails


# ==================================================================================================================== routes
def plan_eval(dims, kernel, n_src=None):
    """The host arithmetic of one launcher of warp_aggregate.hip.  kernel: "warp_kernel" (launch<MODE>: kVec, kVar, and kWarp with
    n_src = 1), "vec8" (launch_vec8), "pairdiff4" / "pairdiff8" (launch_pairdiff<G, GPL>), "win" (launch_win).
    -> ppb, lpp, nblk, dchunk, lds, refused (the launcher returns MDF_EUNSUPPORTED and the entry point falls back), form
    ("few" / "two" / "generic") and ngrp of FixedPairs, chunks (nd of every chunk), nchunks, short_last, ragged_groups (some chunk's nd
    is no multiple of ngrp), dead_slots."""
    b, c, g, d, h, w, ns = dims
    ns = ns if n_src is None else n_src
    assert kernel in KERNELS
    if kernel in ("warp_kernel", "win"):
        lpp, tab, np_, limit = c // 4, WARP_TAB, 1, None
    elif kernel == "vec8":
        lpp, tab, np_, limit = c // 8, VEC8_TAB, 2, LDS_LIMIT
    else:
        gpl = int(kernel[-1])
        lpp, tab, np_, limit = g // gpl, VEC8_TAB, 2, LDS_LIMIT
    ppb = K_THREADS // lpp
    nblk = (h * w + ppb - 1) // ppb
    dch = min(max(1, tab // (ns * ppb)), d)
    lds = dch * ns * ppb * TAP_ENTRY_BYTES
    if kernel == "win":
        lds += WIN_POOL_KB * 1024
        limit = WIN_LDS_LIMIT
    refused = limit is not None and lds > limit
    npair = ppb * ns
    few = K_THREADS % npair == 0
    two = np_ == 2 and npair == 2 * K_THREADS
    assert (few or two) == ((fixed_pairs_usable(ppb, ns)) or two)
    form = "generic" if kernel == "win" or not (few or two) else ("few" if few else "two")
    ngrp = K_THREADS // npair if form == "few" else 1
    chunks = [min(dch, d - d0) for d0 in range(0, d, dch)]
    return NS(kernel=kernel, launch=LAUNCH_NAME[kernel], ppb=ppb, lpp=lpp, nblk=nblk, dchunk=dch, lds=lds, refused=refused, form=form, ngrp=ngrp,
              chunks=chunks, nchunks=len(chunks), short_last=chunks[-1] < dch, ragged_groups=any(nd % ngrp for nd in chunks),
              dead_slots=nblk * ppb - h * w)


def vec_route(dims, vec8=1, window=False):
    """The kernel mdf_warp_aggregate_vec_fwd launches under MDF_WARP_VEC8 = `vec8` and MDF_WARP_WINDOW = `window` -> its plan."""
    c = dims[1]
    if window:
        p = plan_eval(dims, "win")
        if not p.refused:
            return p
    if vec8 != 0 and (c in (64, 32) or (c == 16 and vec8 == 2)):
        p = plan_eval(dims, "vec8")
        if not p.refused:
            return p
    return plan_eval(dims, "warp_kernel")


def pairdiff_route(dims, gpl=4):
    """The plan mdf_warp_aggregate_pairdiff_fwd launches under MDF_PAIRDIFF_GPL = `gpl` (8 falls back to 4 when its table outgrows LDS)."""
    if gpl == 8:
        p = plan_eval(dims, "pairdiff8")
        if not p.refused:
            return p
    p = plan_eval(dims, "pairdiff4")
    assert not p.refused
    return p


def straddling_planes(plan):
    """[a, b) that starts inside the first chunk of `plan` and ends inside a later one, the third where there is one (plane
    independence across a chunk boundary); never the whole depth range."""
    d = sum(plan.chunks)
    assert plan.nchunks >= 2
    return max(plan.dchunk - 2, 0), min(d - 1, 2 * plan.dchunk + 1)
