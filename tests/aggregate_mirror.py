"""TEST INFRASTRUCTURE (CPU, torch float64): the reference, the launch-route mirror and the case table of the training-mode vector
aggregation (csrc/warp_aggregate_train.hip, csrc/warp_scatter.h, the fill_taps / FixedPairs / PixTile helpers of csrc/warp_common.h).
tests/test_aggregate_mirror_cpu.py asserts the preconditions on the CPU, tests/test_aggregate_train_gpu.py compares the kernels.

REFERENCE.  `run(inp, dtype)` is VectorAggregate in training mode (homoaggregate.py:16-46) AT THE KERNELS' SAMPLE POSITIONS: ix, iy come
from oracle.mvs_oracle.warp_positions in fp32 (bit-identical to the kernels', tests/test_oracle_golden.py) and are then cast to `dtype`;
bilinear weights, the zero of out-of-bounds taps, the gather-based warp (the body of oracle.homo_warping_explicit), pair softmax,
similarity, Conv3d(G->1) / BatchNorm(batch statistics) / ReLU / Conv3d(1->1) / sigmoid per source view and sum(w sim) / sum(w) follow in
`dtype`, and autograd differentiates them.  The oracle's own float64 run rounds the sampling GRID in float64, samples somewhere else by
up to ~1e-4 on large maps and cannot resolve what this suite is after.  dtype = float32 is the "fp32 restatement": what fp32 arithmetic
owes.  The projections are the relative ones of the C ABI ([n_src,B,3,4], pixel units), so synthetic cameras need no intrinsics.

MAGNITUDE SUMS.  Every accumulated gradient element is judged against A = the sum of the absolute values of the terms added into it:
d src: the gradient of sum(warped * |d warped|.detach()) w.r.t. the source map (the bilinear weights are non-negative, so this is exactly
sum w_tap |g|); d ref: sum_{v,d} |d sim| |2 q0 - 1| p0 p1; d conv weight: sum |d t| sim; the fp64 reductions: sum |t|, sum t^2,
sum |dz|, sum |dz xhat|, sum |du relu|, sum |du|.

THE BAR.  e_hip <= 1.5 e_32 + t per quantity and metric (max|d| / max|ref|, relative L2, and max |d| / A for the accumulated
gradients), with e_x the distance of x from the float64 reference.  1.5 is the project's standing rule for an fp32 implementation next
to its fp32 oracle.  t covers what the kernels do differently BY DESIGN and is derived from the float64 reference alone, never from a
kernel's output.  With u = 2^-24 (fp32 unit roundoff) and ulp = 2 u:

  t = t_special + t_order

  t_special: v_exp_f32 and v_rcp_f32 are 1-ulp instructions (libm's expf and the IEEE divide of the restatement are 0.5 ulp), and the
    argument of the exponential is multiplied by log2(e) first (a relative error u of an argument x is a relative error |x| u of e^x).
    Every pair softmax 1 / (1 + exp2((b - a) log2e)) and every sigmoid carries one of each.  On the path of one sample there are the
    reference softmax (2 operations), the source softmax (2) and, for everything behind the view weights, the sigmoid (2), and every
    quantity behind the BatchNorm sees those of ALL samples through the batch statistics -- so the operations are not counted by hand:
    the float64 reference is RE-RUN with every such operation moved by its bound, e -> e (1 + s1 ulp) with the argument x -> x (1 + s0 u),
    1/(1+e) -> (1 + s2 ulp) / (1 + e), s = +-1 independent per element and operation (distinct elements' errors are independent; the
    alignment of 10^4 signs is no implementation's behaviour), and the displacement of every quantity is measured in the quantity's own
    metric.  t_special = 2 x the largest displacement of PERTURB_DRAWS = 3 draws (the factor covers the draw-to-draw spread of a
    maximum norm).  This is first-order error propagation evaluated numerically: it sees the cancellations (d t = gamma invstd (dz -
    mean dz - xhat mean(dz xhat)), d sim = dN w + dt cw) and the amplification |w2 alpha| sum|cw| of the head that a count alone misses.
  t_order: the kernels add in another order than torch does, in fp32: per lane over the planes of a chunk, then over the wave, then fp64
    atomics (reductions: <= dchunk + 6 fp32 additions, worst-case bound (dchunk + 6) u sum|terms|); fp32 fma chains per lane, the LDS
    window and fp32 atomics for the gradients (n terms in an order that changes from run to run: the rounding errors of n additions in
    random order grow as sqrt(n), bound 2 sqrt(n) u sum|terms| = 2 sqrt(n) u A with n = the number of terms of the element: live taps
    of the texel for d src, D n_src for d ref, B D h w n_src for d conv weight).  In the max / L2 metrics the term is scaled by
    max A / max|ref| and |A| / |ref|.
  The forward (cost, wsum, the per-sample scalars) has no sums beyond the 32 groups of a pixel and the n_src views: t_order = 0 there.

ROUTES.  `plan_train` / `plan_bwd` restate the launchers' host arithmetic (tile shapes, block counts, depth_slices, equal_chunks, table
sizes, slice targets, FixedPairs::usable) and `scatter_routes` the block-level decisions of warp_bwd_kernel from the float64 tap weights
per (tile, batch, slice, chunk, view): the bounding box of the live taps, window or direct to memory, clamped corner sets, and how many
pixels of a tile share one (xa, ya) within a plane.  The constants are compared with the sources by tests/test_aggregate_mirror_cpu.py.
"""
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import mvs_oracle as O  # noqa: E402

U = 2.0 ** -24
ULP = 2.0 ** -23
PERTURB_DRAWS = 3
BN_EPS32 = float(np.float32(1e-5))
BN_MOM32 = float(np.float32(0.1))

# ---- constants of the kernels' launchers (held against the sources by test_constants_are_the_sources)
K_THREADS = 256
WIN_FLOATS = 4096
MAX_SRC_VIEWS = 16
SCATTER_TILE_ROWS = 4
MIN_PLANES_PER_SLICE = 4
TRAIN_TAB = 512
BWD_TAB = {True: 512, False: 1024}            # per-pixel hypotheses: True
TRAIN_TARGET = {True: 1024, False: 2048}
BWD_TARGET = {True: 768, False: 1024}


# ==================================================================================================================== case table
# id -> (h, w, C, n_src, D, B, per_pixel, cameras)
CASES = {
    "min": (2, 2, 64, 1, 1, 1, False, "real"),
    "v16": (5, 7, 16, 16, 3, 1, True, "real"),
    "fix4": (7, 9, 64, 4, 48, 2, False, "real"),
    "gen3": (13, 11, 32, 3, 24, 2, True, "real"),
    "s2": (6, 33, 16, 2, 8, 1, True, "real"),
    "d9": (13, 11, 32, 3, 9, 1, True, "real"),
    "d7": (13, 11, 32, 3, 7, 1, True, "real"),
    # exact positions need a map whose (w-1)/w and (h-1)/h are dyadic: base.py:117 normalises by (w-1)/2 and grid_sample
    # (align_corners=False) unnormalises by w/2, so ix = px w/(w-1) - 0.5, and at 6 x 10 no fp32 projection lands on the texels
    "ident16": (8, 16, 16, 2, 5, 1, False, "ident"),
    "ident64": (8, 16, 64, 2, 5, 1, False, "ident"),
    "half16": (8, 16, 16, 2, 5, 1, False, "half"),
    "half64": (8, 16, 64, 2, 5, 1, False, "half"),
    "mini16": (8, 16, 16, 2, 4, 1, False, "mini"),
    "mini64": (8, 16, 64, 2, 4, 1, False, "mini"),
    "mag64": (13, 15, 64, 2, 5, 1, True, "mag"),
    "mag32": (17, 17, 32, 2, 5, 1, True, "mag"),
    "mag16": (23, 23, 16, 2, 5, 1, True, "mag"),
    "gone": (6, 33, 16, 2, 8, 1, True, "gone"),
    # one thread group of fixed pairs (PPB n_src = 256), which no case of the issue's table has
    "grp1": (6, 9, 32, 8, 4, 1, False, "real"),
}
# seeds chosen so that no sample lies within GRID_MARGIN of a pixel-grid line (test_no_sample_near_a_grid_line)
SEEDS = {k: 1 for k in CASES}
REAL_CAMERA_CASES = [k for k, c in CASES.items() if c[7] == "real"]
COLLISION_CASES = ["mini16", "mini64", "ident16", "ident64", "half16", "half64", "mag64", "mag32", "mag16"]
REDUCED_CASES = ["fix4", "gen3", "s2", "mag64"]
EXACT_LINE_CASES = ("ident16", "ident64", "half16", "half64")      # put samples on grid lines on purpose
GRID_MARGIN = 1e-4


def _gen(case_id):
    return torch.Generator().manual_seed(1000 * SEEDS[case_id] + sorted(CASES).index(case_id))


def _exact_projection(h, w, sx, sy):
    """[3,4] whose sample positions are EXACTLY (x + sx, y + sy) at every plane (power-of-two map sides, hypotheses with few bits):
    px = (x + sx + 0.5)(w-1)/w, and ix = fma(px / ((w-1)/2), w/2, -0.5) retraces it without a rounding."""
    assert w & (w - 1) == 0 and h & (h - 1) == 0
    m = torch.zeros(3, 4)
    m[0, 0], m[0, 2] = (w - 1) / w, (sx + 0.5) * (w - 1) / w
    m[1, 1], m[1, 2] = (h - 1) / h, (sy + 0.5) * (h - 1) / h
    m[2, 2] = 1.0
    return m


def inputs(case_id):
    """The fp32 inputs of a case: features randn, head parameters = the module's initial values + 0.3 randn, dcost randn."""
    h, w, c, n_src, d, b, per_pixel, cams = CASES[case_id]
    g = c // 2
    gen = _gen(case_id)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    ref = rn(b, c, h, w)
    srcs = [rn(b, c, h, w) for _ in range(n_src)]
    bound = 1.0 / math.sqrt(g)                                   # nn.Conv3d(G, 1, 1): kaiming_uniform(a = sqrt 5) = U(+-1/sqrt(fan_in))
    cw = (torch.rand(g, generator=gen) * 2 - 1) * bound + 0.3 * rn(g)
    gamma, beta = 1.0 + 0.3 * rn(1), 0.3 * rn(1)
    w2, b2 = (torch.rand(1, generator=gen) * 2 - 1) + 0.3 * rn(1), (torch.rand(1, generator=gen) * 2 - 1) + 0.3 * rn(1)
    dcost = rn(b, g, d, h, w)
    rmean, rvar = rn(1), torch.rand(1, generator=gen) + 0.5
    if cams in ("real", "gone"):
        from mdfnet_hip import synth
        intr, extr, _ = synth.make_cameras(w, h, n_src + 1, batch=b, rot_deg=2.0, seed=SEEDS[case_id] + 7)
        rp, sps = O.scale_cam(intr, extr, 3)
        proj = torch.stack([O.relative_projection(sp, rp)[:, :3, :4] for sp in sps]).contiguous()
        if per_pixel:
            hyp = (425 + 510 * torch.rand(b, 1, h, w, generator=gen)) + torch.linspace(-20, 20, d).reshape(1, d, 1, 1)
        else:
            hyp = torch.stack([torch.linspace(425 + 9 * i, 935 - 5 * i, d) for i in range(b)]).reshape(b, d, 1, 1)
        cam = (rp, sps)
        if cams == "gone":
            proj[1, :, 0, 3] += 1.0e6                            # view 1: ~1000 pixels off the frame at every plane
            cam = None
    else:
        cam = None
        if cams == "mag":                                        # the cameras of test_vector_aggregate_scatter_window_and_direct_to_memory_paths
            proj = torch.eye(4)[:3].repeat(2, 1, 1, 1)
            # (C = 16: a window holds 512 of the 23 x 23 = 529 texels, so the origin tile has to reach all 23 rows: 8x at d = 500)
            proj[0, 0, :, 3] = torch.tensor([0.0, 0.0, -440.0 if c == 16 else -420.0])
            proj[1, 0, :, 3] = torch.tensor([10.0, -5.0, -400.0])
            hyp = 500 + 300 * torch.rand(b, d, h, w, generator=gen)
        else:
            shifts = {"ident": [(0.0, 0.0), (0.0, 0.0)], "half": [(0.5, 0.0), (-0.5, -0.5)]}.get(cams)
            if cams == "mini":                                   # x' = x/4, y' = y/4 at every plane: Z = 4 d
                m = torch.eye(4)[:3].clone()
                m[2, 2] = 4.0
                proj = torch.stack([m, m]).unsqueeze(1).contiguous()
                proj[1, 0, 0, 2] = 0.3                           # view 1: x' = (x + 0.3)/4
            else:
                proj = torch.stack([_exact_projection(h, w, sx, sy) for sx, sy in shifts]).unsqueeze(1).contiguous()
            hyp = torch.linspace(512, 1024, d).reshape(1, d, 1, 1)
    inp = NS(id=case_id, ref=ref, srcs=srcs, proj=proj.float().contiguous(), hyp=hyp.float().contiguous(), per_pixel=per_pixel, cw=cw,
             gamma=gamma, beta=beta, w2=w2, b2=b2, dcost=dcost, rmean=rmean, rvar=rvar, cam=cam, dims=(b, c, g, d, h, w, n_src))
    if cams in ("real", "gone", "mag"):
        _clear_grid_lines(inp)
    return inp


def _near_lines(inp, margin):
    """bool [B,D,hw]: a sample of some view with a tap in the frame lies within `margin` of a pixel-grid line."""
    b, c, g, d, h, w, n_src = inp.dims
    bad = torch.zeros(b, d, h * w, dtype=torch.bool)
    for ix, iy in positions(inp):
        ix, iy = ix.double(), iy.double()
        near = (ix > -1) & (ix < w) & (iy > -1) & (iy < h)
        bad |= near & (((ix - torch.round(ix)).abs() < margin) | ((iy - torch.round(iy)).abs() < margin))
    return bad


def _clear_grid_lines(inp):
    """Random hypotheses put a few of the ~10^4 samples of a case next to a grid line, where floor() of the fp32 restatement and of a
    kernel may differ for reasons that are the inputs', not the kernel's: those hypotheses (the plane's, when they are uniform) are
    moved in steps of 0.61 until every sample keeps 2 GRID_MARGIN.  Deterministic; a case it cannot clear fails the CPU suite."""
    for _ in range(60):
        bad = _near_lines(inp, 2 * GRID_MARGIN)
        if not bool(bad.any()):
            return
        if inp.per_pixel:
            inp.hyp += 0.61 * bad.reshape(inp.hyp.shape).float()
        else:
            inp.hyp += 0.61 * bad.any(dim=2).reshape(inp.hyp.shape).float()


# ==================================================================================================================== the reference
def positions(inp):
    """[(ix, iy)] per source view, fp32 [B,D,h*w]: the kernels' sample positions."""
    b, c, g, d, h, w, n_src = inp.dims
    assert O.WORK == torch.float32
    out = []
    for v in range(n_src):
        ix, iy = O.warp_positions(inp.proj[v], inp.hyp, h, w)
        out.append((ix.expand(b, d, h * w).contiguous(), iy.expand(b, d, h * w).contiguous()))
    return out


def warp_at(src_fea, ix, iy):
    """The body of oracle.homo_warping_explicit behind its positions, in the working precision: torch.gather, autograd-able."""
    b, c, h, w = src_fea.shape
    d = ix.shape[1]
    x0f, y0f = torch.floor(ix), torch.floor(iy)
    _, _, wts, masks = O.warp_corners(ix, iy, h, w)
    flat = src_fea.reshape(b, c, 1, h * w).expand(b, c, d, h * w)

    def tap(xf, yf, m):
        xi = xf.clamp(0, w - 1).long()
        yi = yf.clamp(0, h - 1).long()
        idx = (yi * w + xi).unsqueeze(1).expand(b, c, d, h * w)
        return torch.gather(flat, 3, idx) * m.unsqueeze(1)

    taps = (tap(x0f, y0f, masks[0]), tap(x0f + 1, y0f, masks[1]), tap(x0f, y0f + 1, masks[2]), tap(x0f + 1, y0f + 1, masks[3]))
    ws = [wt.unsqueeze(1).expand(b, c, d, h * w) for wt in wts]
    acc = taps[0] * ws[0]
    for k in (1, 2, 3):
        acc = O._fma(taps[k], ws[k], acc)
    return acc.reshape(b, c, d, h, w)


class _Perturb:
    """The 1-ulp model of v_exp_f32 / v_rcp_f32 and of the log2(e) product (module docstring), float64 only."""

    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)

    def sign(self, x):
        return (torch.randint(0, 2, x.shape, generator=self.gen) * 2 - 1).to(x.dtype)

    def logistic(self, x):
        """1 / (1 + e^-x) through the modelled instructions."""
        e = torch.exp(-x * (1 + U * self.sign(x))) * (1 + ULP * self.sign(x))
        return (1 + ULP * self.sign(x)) / (1 + e)

    def softmax_pair(self, x, dim):
        a, b_ = x.unbind(dim)
        p0 = self.logistic(a - b_)
        return torch.stack((p0, 1 - p0), dim)


def finalize_mirror(red, gamma, beta, n, rmean, rvar, eps=BN_EPS32, momentum=BN_MOM32):
    """agg_finalize_kernel in float64: red [2 n_src] -> consts [n_src,4] (alpha, shift, mean, invstd), running mean / var after n_src
    chained updates.  eps and momentum are the fp32 values widened, as the entry point passes them."""
    red = [float(x) for x in red]
    gamma, beta, n = float(gamma), float(beta), float(n)
    rm, rv = float(rmean), float(rvar)
    rows = []
    for v in range(len(red) // 2):
        mean = red[2 * v] / n
        var = max(red[2 * v + 1] / n - mean * mean, 0.0)
        invstd = 1.0 / math.sqrt(var + eps)
        alpha = gamma * invstd
        rows.append([alpha, beta - mean * alpha, mean, invstd])
        rm = (1.0 - momentum) * rm + momentum * mean
        rv = (1.0 - momentum) * rv + momentum * var * (n / (n - 1.0 if n > 1.0 else 1.0))
    return torch.tensor(rows, dtype=torch.float64), rm, rv


def run(inp, dtype=torch.float64, perturb=None):
    """Forward and backward of the slot at the kernels' positions in `dtype` -> every intermediate in the KERNELS' layouts, float64 on
    the CPU.  perturb = a seed: the special-function model of the module docstring (float64 only)."""
    b, c, g, d, h, w, n_src = inp.dims
    pos = positions(inp)
    pt = _Perturb(perturb) if perturb is not None else None
    assert pt is None or dtype == torch.float64
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)  # noqa: E731
    ref, srcs = leaf(inp.ref), [leaf(s) for s in inp.srcs]
    cw, gamma, beta, w2, b2 = (leaf(t) for t in (inp.cw, inp.gamma, inp.beta, inp.w2, inp.b2))
    dcost = inp.dcost.to(dtype)
    n = b * d * h * w
    views = []
    with O.precision(dtype):
        refp = ref.reshape(b, g, 2, 1, h, w)
        ref_unit = pt.softmax_pair(refp, 2) if pt else F.softmax(refp, dim=2)
        num, den = 0.0, 0.0
        for v in range(n_src):
            ix, iy = (t.to(dtype) for t in pos[v])
            vol = warp_at(srcs[v], ix, iy)
            vol.retain_grad()
            volp = vol.reshape(b, g, 2, d, h, w)
            q = pt.softmax_pair(volp, 2) if pt else F.softmax(volp, dim=2)
            sim = (q * ref_unit).sum(dim=2)
            sim.retain_grad()
            t = F.conv3d(sim, cw.reshape(1, g, 1, 1, 1))
            z = F.batch_norm(t, None, None, gamma, beta, True, 0.1, BN_EPS32)
            rl = F.relu(z)
            uu = F.conv3d(rl, w2.reshape(1, 1, 1, 1, 1), b2)
            wv = pt.logistic(uu) if pt else torch.sigmoid(uu)
            for x in (t, z, uu):
                x.retain_grad()
            den = den + wv
            num = num + wv * sim
            views.append(NS(vol=vol, q=q, sim=sim, t=t, z=z, rl=rl, u=uu, w=wv))
        cost = num / den
    cost.backward(dcost)

    f64 = lambda x: x.detach().double()  # noqa: E731
    nhwc = lambda x: f64(x).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    out = NS(dims=inp.dims, n=n)
    out.cost = f64(cost).permute(0, 2, 3, 4, 1).contiguous()                     # [B,D,h,w,G]
    out.wsum = f64(den).reshape(b, d, h, w)
    red0, red0_abs, red2, red2_abs, aux, consts = [], [], [], [], [], []
    rm, rv = float(inp.rmean), float(inp.rvar)
    a_dcw = torch.zeros(g, dtype=torch.float64)
    a_ref = torch.zeros(b, g, h, w, dtype=torch.float64)
    p0, p1 = f64(ref_unit)[:, :, 0], f64(ref_unit)[:, :, 1]                      # [B,G,1,h,w]
    for vw in views:
        t = f64(vw.t)
        red0 += [t.sum(), (t * t).sum()]
        red0_abs += [t.abs().sum(), (t * t).sum()]
        mean, var = t.mean(), t.var(unbiased=False)
        invstd = 1.0 / torch.sqrt(var + BN_EPS32)
        alpha = f64(gamma)[0] * invstd
        consts.append(torch.stack([alpha, f64(beta)[0] - mean * alpha, mean, invstd]))
        rm = (1.0 - BN_MOM32) * rm + BN_MOM32 * float(mean)
        rv = (1.0 - BN_MOM32) * rv + BN_MOM32 * float(var) * (n / (n - 1.0 if n > 1 else 1.0))
        dz, du, xh = f64(vw.z.grad), f64(vw.u.grad), (t - mean) * invstd
        red2 += [dz.sum(), (dz * xh).sum()]
        red2_abs += [dz.abs().sum(), (dz * xh).abs().sum()]
        aux.append(torch.stack([f64(vw.w).reshape(-1), dz.reshape(-1), t.reshape(-1)], 1))
        a_dcw += (f64(vw.t.grad) * f64(vw.sim)).abs().sum(dim=(0, 2, 3, 4))
        a_ref += (f64(vw.sim.grad).abs() * (2 * f64(vw.q)[:, :, 0] - 1).abs() * p0 * p1).sum(dim=2)
    # one source view: cost = w sim / w = sim, so everything behind d w is ZERO in exact arithmetic and rounding noise in fp32.  Its scale:
    # d w = sum_g (dc_g / den) sim_g - sum_g dc_g cost_g / den, two dot products over the G groups with sum |terms| = mag_dw
    dc, cst = f64(dcost), f64(cost)
    out.mag_dz, out.xh, out.rl, out.sim = [], [], [], []
    for vw in views:
        mag_dw = ((dc.abs() * (f64(vw.sim).abs() + cst.abs())).sum(1, keepdim=True) / f64(den))
        wv = f64(vw.w)
        out.mag_dz.append((f64(w2).abs() * wv * (1 - wv) * mag_dw * (f64(vw.z) > 0)).reshape(-1))
        t = f64(vw.t)
        out.xh.append(((t - t.mean()) / torch.sqrt(t.var(unbiased=False) + BN_EPS32)).reshape(-1))
        out.rl.append(f64(vw.rl).reshape(-1))
        out.sim.append(f64(vw.sim))
    out.w2 = float(w2.detach())
    du_rl = [f64(vw.u.grad) * f64(vw.rl) for vw in views]
    out.red0, out.red0_abs = torch.stack(red0), torch.stack(red0_abs)
    out.red2 = torch.stack(red2 + [sum(x.sum() for x in du_rl), sum(f64(vw.u.grad).sum() for vw in views)])
    out.red2_abs = torch.stack(red2_abs + [sum(x.abs().sum() for x in du_rl), sum(f64(vw.u.grad).abs().sum() for vw in views)])
    out.consts, out.rmean, out.rvar = torch.stack(consts), rm, rv
    out.aux = torch.stack(aux)                                                   # [n_src, B*D*h*w, 3]
    out.dref = nhwc(ref.grad)                                                    # [B,h,w,C]
    out.dsrc = torch.stack([nhwc(s.grad) for s in srcs])                         # [n_src,B,h,w,C]
    out.dcw = f64(cw.grad)
    out.dpar = torch.stack([f64(gamma.grad)[0], f64(beta.grad)[0], f64(w2.grad)[0], f64(b2.grad)[0]])
    out.a_dcw = a_dcw
    out.a_ref = a_ref.permute(0, 2, 3, 1).repeat_interleave(2, dim=3).contiguous()   # [B,h,w,C]: both channels of a pair
    # A of d src: the warp is linear in the source map, so this gradient is sum w_tap |g| exactly
    a_src = []
    with O.precision(dtype):
        for v in range(n_src):
            s2 = leaf(inp.srcs[v])
            ix, iy = (t.to(dtype) for t in pos[v])
            (warp_at(s2, ix, iy) * views[v].vol.grad.abs().detach()).sum().backward()
            a_src.append(nhwc(s2.grad))
    out.a_src = torch.stack(a_src)
    return out


QUANTITIES = ("red0", "consts", "cost", "wsum", "aux_w", "aux_dz", "aux_t", "red2", "dref", "dsrc", "dcw", "dpar")
ACCUMULATED = {"dref": "a_ref", "dsrc": "a_src", "dcw": "a_dcw", "red0": "red0_abs", "red2": "red2_abs"}


def quantity(res, name):
    if name.startswith("aux_"):
        return res.aux[..., ("w", "dz", "t").index(name[4:])]
    return getattr(res, name)


def distances(got, ref64, name):
    """{metric: value} of `got` (a result of run, or kernel outputs in the same layout) from the float64 reference."""
    a, r = quantity(got, name).double(), quantity(ref64, name)
    dif = (a - r).abs()
    out = {"max": float(dif.max() / r.abs().max().clamp(min=1e-300)), "l2": float(dif.norm() / r.norm().clamp(min=1e-300))}
    if name in ACCUMULATED:
        mag = getattr(ref64, ACCUMULATED[name])
        live = mag > 1e-12 * mag.max()          # (A = 0: no term at all, e.g. a pixel whose samples all leave the frame; the max metric holds those)
        out["perA"] = float((dif[live] / mag[live]).max()) if bool(live.any()) else 0.0
    return out


ZERO_AT_ONE_VIEW = ("aux_dz", "red2", "dcw", "dpar")


def one_view_bounds(ref64):
    """n_src = 1: absolute bounds of the quantities that are zero in exact arithmetic (run: mag_dz).  A dot product of G fp32 terms
    errs by at most G u sum|terms|, the stored cost by 2 u (product and quotient), the two quotients by u each: (G + 4) u mag_dz per
    sample, propagated linearly through the sums and the BatchNorm backward."""
    b, c, g, d, h, w, n_src = ref64.dims
    assert n_src == 1
    bdz = (g + 4) * U * ref64.mag_dz[0]
    xh, rl = ref64.xh[0].abs(), ref64.rl[0]
    s1, s2 = bdz.sum(), (bdz * xh).sum()
    dw2, db2 = (bdz * rl).sum() / abs(ref64.w2), bdz.sum() / abs(ref64.w2)
    gi = (ref64.consts[0, 0]).abs()                                   # |gamma invstd|
    bdt = gi * (bdz + bdz.mean() + xh * (bdz * xh).mean())
    dcw = (bdt.reshape(b, 1, d, h, w) * ref64.sim[0].abs()).sum(dim=(0, 2, 3, 4))
    return {"aux_dz": bdz.reshape(1, -1), "red2": torch.stack([s1, s2, dw2, db2]), "dcw": dcw, "dpar": torch.stack([s2, s1, dw2, db2])}


def derived_t(inp, ref64, perturbed, dchunk_train, taps_per_texel):
    """{quantity: {metric: t}} (module docstring).  perturbed: the PERTURB_DRAWS perturbed float64 runs; dchunk_train: planes per chunk
    of passes 0 and 2; taps_per_texel: the largest number of live taps on one texel of a source map (scatter_routes)."""
    b, c, g, d, h, w, n_src = inp.dims
    n_terms = {"dref": d * n_src, "dsrc": max(1, taps_per_texel), "dcw": b * d * h * w * n_src}
    out = {}
    for name in QUANTITIES:
        t = {}
        for pr in perturbed:
            for k, v in distances(pr, ref64, name).items():
                t[k] = max(t.get(k, 0.0), 2.0 * v)
        if name in ACCUMULATED:
            mag, r = getattr(ref64, ACCUMULATED[name]), quantity(ref64, name)
            rel = (dchunk_train + 6) * U if name.startswith("red") else 2.0 * math.sqrt(n_terms[name]) * U
            t["max"] += rel * float(mag.max() / r.abs().max().clamp(min=1e-300))
            t["l2"] += rel * float(mag.norm() / r.norm().clamp(min=1e-300))
            t["perA"] += rel
        if name == "consts":
            # CORRECTED after the first GPU run (every case failed `consts` and nothing else, e_hip up to 1.6e-5 at v16): the derivation
            # above had left out that agg_finalize_kernel forms var = E[t^2] - mean^2 from the two sums, so the fp32 partial sums of
            # pass 0 (relative error k u of sum t^2 and of sum |t|, k = dchunk + 6, the t_order of red0) reach the constants amplified by
            # mean^2 / var, where torch's BatchNorm (two passes over the centred values) and the perturbed runs are not:
            #   d var <= k u (E t^2 + 2 |mean| E|t|), d mean <= k u E|t|, d invstd / invstd = d alpha / alpha = d var / (2 (var + eps)),
            #   d shift <= |alpha| d mean + |mean| d alpha
            k = (dchunk_train + 6) * U
            rows = []
            for v in range(n_src):
                alpha, _, mean, invstd = (float(x) for x in ref64.consts[v])
                et2, eabs = float(ref64.red0[2 * v + 1]) / ref64.n, float(ref64.red0_abs[2 * v]) / ref64.n
                var_eps = 1.0 / (invstd * invstd)
                dvar, dmean = k * (et2 + 2 * abs(mean) * eabs), k * eabs
                rel = 0.5 * dvar / var_eps
                rows.append([abs(alpha) * rel, abs(alpha) * dmean + abs(mean) * abs(alpha) * rel, dmean, invstd * rel])
            bound = torch.tensor(rows, dtype=torch.float64)
            t["max"] += float(bound.max() / ref64.consts.abs().max())
            t["l2"] += float(bound.norm() / ref64.consts.norm())
        if name == "dpar":       # (d gamma, d beta, d w2, d b2) = the fp64 reductions of pass 2, summed over the views in fp64
            r2, a2 = ref64.red2, ref64.red2_abs
            rel = (dchunk_train + 6) * U
            mags = torch.stack([a2[1:2 * n_src:2].sum(), a2[0:2 * n_src:2].sum(), a2[2 * n_src], a2[2 * n_src + 1]])
            t["max"] += rel * float(mags.max() / ref64.dpar.abs().max().clamp(min=1e-300))
            t["l2"] += rel * float(mags.norm() / ref64.dpar.norm().clamp(min=1e-300))
        out[name] = t
    return out


# ==================================================================================================================== routes
def depth_slices(nblk_x, b, d, dch, target):
    """warp_scatter.h:depth_slices -> (gridDim.z, dslice, dch clamped)."""
    blocks = nblk_x * b
    nz = (target + blocks - 1) // blocks
    nz = max(1, min(nz, d // MIN_PLANES_PER_SLICE))
    dslice = (d + nz - 1) // nz
    nz = (d + dslice - 1) // dslice
    return nz, dslice, min(dch, dslice)


def equal_chunks(dslice, dch):
    nch = (dslice + dch - 1) // dch
    return (dslice + nch - 1) // nch


def fixed_pairs_usable(ppb, n_src):
    return K_THREADS % (ppb * n_src) == 0


def plan_train(dims, per_pixel, tab=TRAIN_TAB, target=0):
    """launch_train (passes 0 to 2): tiles are runs of PPB pixels in row-major order."""
    b, c, g, d, h, w, n_src = dims
    ppb = K_THREADS // (c // 4)
    nblk_x = (h * w + ppb - 1) // ppb
    dch = max(1, tab // (n_src * ppb))
    nz, dslice, dch = depth_slices(nblk_x, b, d, dch, target or TRAIN_TARGET[bool(per_pixel)])
    dchunk = equal_chunks(dslice, dch)
    fixed = fixed_pairs_usable(ppb, n_src)
    ngrp = K_THREADS // (ppb * n_src) if fixed else 0
    chunks = []                         # nd of every chunk of every slice
    for z in range(nz):
        dlo, dhi = z * dslice, min(d, (z + 1) * dslice)
        chunks += [min(dchunk, dhi - d0) for d0 in range(dlo, dhi, dchunk)]
    return NS(ppb=ppb, nblk_x=nblk_x, grid=(nblk_x, b, nz), dslice=dslice, dchunk=dchunk, fixed=fixed, ngrp=ngrp, chunks=chunks,
              lds=dchunk * n_src * ppb * 32, dead_slots=nblk_x * ppb - h * w, nred=(2 * n_src, 2 * n_src + 2),
              ragged=d % dslice != 0, bb_threads=4 * n_src)


def plan_bwd(dims, per_pixel, tab=0, target=0):
    """launch_bwd (pass 3): tiles are (PPB/4) x 4 rectangles."""
    b, c, g, d, h, w, n_src = dims
    ppb = K_THREADS // (c // 4)
    tw, th = ppb // SCATTER_TILE_ROWS, SCATTER_TILE_ROWS
    tiles_x, tiles_y = (w + tw - 1) // tw, (h + th - 1) // th
    nblk_x = tiles_x * tiles_y
    dch = max(1, (tab or BWD_TAB[bool(per_pixel)]) // (n_src * ppb))
    nz, dslice, dch = depth_slices(nblk_x, b, d, dch, target or BWD_TARGET[bool(per_pixel)])
    dchunk = equal_chunks(dslice, dch)
    nv = 1 if per_pixel else n_src
    dstep = dchunk * n_src if per_pixel else dchunk
    return NS(ppb=ppb, tw=tw, th=th, tiles_x=tiles_x, nblk_x=nblk_x, grid=(nblk_x, b, nz), dslice=dslice, dchunk=dchunk, nv=nv, dstep=dstep,
              lds=dchunk * n_src * ppb * 32 + WIN_FLOATS * 4, ragged=d % dslice != 0, win_texels=WIN_FLOATS // g)


def taps64(inp):
    """Per view: float64 tap weights [4,B,D,hw] (0 out of bounds) and the kernels' clamped corners xa, xb, ya, yb (int64 [B,D,hw])."""
    b, c, g, d, h, w, n_src = inp.dims
    out = []
    for ix, iy in positions(inp):
        ix, iy = ix.double(), iy.double()
        x0, y0 = torch.floor(ix), torch.floor(iy)
        fw, fn = ix - x0, iy - y0
        wts = [(1 - fn) * (1 - fw), (1 - fn) * fw, fn * (1 - fw), fn * fw]
        inb = lambda v, m: (v >= 0) & (v <= m)  # noqa: E731
        bx0, bx1, by0, by1 = inb(x0, w - 1), inb(x0 + 1, w - 1), inb(y0, h - 1), inb(y0 + 1, h - 1)
        msk = [bx0 & by0, bx1 & by0, bx0 & by1, bx1 & by1]
        wts = torch.stack([wt * m for wt, m in zip(wts, msk)])
        xi, yi = x0.clamp(-2, w).long(), y0.clamp(-2, h).long()
        xa, xb = xi.clamp(0, w - 1), (xi + 1).clamp(0, w - 1)
        ya, yb = yi.clamp(0, h - 1), (yi + 1).clamp(0, h - 1)
        out.append(NS(wt=wts, xa=xa, xb=xb, ya=ya, yb=yb, ix=ix, iy=iy))
    return out


def live_texels(inp):
    """[n_src,B,h,w] bool: the texels some live tap (weight != 0) of the view touches, and [n_src,B,h,w] the count of such taps."""
    b, c, g, d, h, w, n_src = inp.dims
    cnt = torch.zeros(n_src, b, h * w, dtype=torch.int64)
    for v, t in enumerate(taps64(inp)):
        for k in range(4):
            tx, ty = (t.xb if k & 1 else t.xa), (t.yb if k & 2 else t.ya)
            idx = (ty * w + tx).reshape(b, -1)
            cnt[v].scatter_add_(1, idx, (t.wt[k] != 0).reshape(b, -1).long())
    cnt = cnt.reshape(n_src, b, h, w)
    return cnt > 0, cnt


def scatter_routes(inp, plan=None):
    """The block-level decisions of warp_bwd_kernel, one record per (tile, batch, slice, chunk, view):
    any (a live tap exists), window (ScatterWin::use), box (ww, wh), clamped (a live pixel has xb == xa or yb == ya), share (the most
    pixels of the tile on one (xa, ya) within one plane, among pixels with a live tap), one_flush (every live pixel's corner set is the
    same over all planes of the record), zero_w (an in-bounds tap of weight exactly 0 next to a live one)."""
    b, c, g, d, h, w, n_src = inp.dims
    plan = plan or plan_bwd(inp.dims, inp.per_pixel)
    taps = taps64(inp)
    # pixel ids of every tile (live slots only)
    tiles = []
    for tl in range(plan.nblk_x):
        y0, x0 = (tl // plan.tiles_x) * plan.th, (tl % plan.tiles_x) * plan.tw
        tiles.append(torch.tensor([y * w + x for y in range(y0, min(y0 + plan.th, h)) for x in range(x0, min(x0 + plan.tw, w))]))
    recs = []
    for z in range(plan.grid[2]):
        dlo, dhi = z * plan.dslice, min(d, (z + 1) * plan.dslice)
        for v in range(n_src):
            t = taps[v]
            for d0 in range(dlo, dhi, plan.dstep):
                nd = min(plan.dstep, dhi - d0)
                for bi in range(b):
                    for tl, pix in enumerate(tiles):
                        sl = (bi, slice(d0, d0 + nd), pix)
                        wt = t.wt[(slice(None),) + sl]                                       # [4,nd,npix]
                        xa, xb, ya, yb = t.xa[sl], t.xb[sl], t.ya[sl], t.yb[sl]
                        lv = wt != 0
                        pix_live = lv.any(0)
                        rec = NS(tile=tl, b=bi, z=z, d0=d0, nd=nd, view=v, any=bool(pix_live.any()), window=False, box=(0, 0), clamped=False,
                                 share=0, one_flush=False, zero_w=False)
                        if rec.any:
                            xs = torch.cat([(xb if k & 1 else xa)[lv[k]] for k in range(4)])
                            ys = torch.cat([(yb if k & 2 else ya)[lv[k]] for k in range(4)])
                            ww, wh = int(xs.max() - xs.min()) + 1, int(ys.max() - ys.min()) + 1
                            rec.box = (ww, wh)
                            rec.window = ww * wh * g <= WIN_FLOATS
                            rec.clamped = bool((((xb == xa) | (yb == ya)) & pix_live).any())
                            for dd in range(nd):
                                key = (ya[dd] * w + xa[dd])[pix_live[dd]]
                                if key.numel():
                                    rec.share = max(rec.share, int(torch.bincount(key).max()))
                            same = (xa == xa[:1]) & (ya == ya[:1]) & (xb == xb[:1]) & (yb == yb[:1])
                            rec.one_flush = nd > 1 and bool(same.all())
                            inb = ((t.ix[sl] >= 0) & (t.ix[sl] <= w - 2) & (t.iy[sl] >= 0) & (t.iy[sl] <= h - 2)).unsqueeze(0)
                            rec.zero_w = bool(((wt == 0) & inb & pix_live.unsqueeze(0)).any())
                        recs.append(rec)
    return recs


def grid_line_distance(inp):
    """The smallest distance of a sample coordinate from a pixel-grid line (an integer), over the samples with a tap in the frame."""
    b, c, g, d, h, w, n_src = inp.dims
    worst = float("inf")
    for ix, iy in positions(inp):
        ix, iy = ix.double(), iy.double()
        near = (ix > -1) & (ix < w) & (iy > -1) & (iy < h)
        for t in (ix, iy):
            dist = (t - torch.round(t)).abs()[near]
            if dist.numel():
                worst = min(worst, float(dist.min()))
    return worst
