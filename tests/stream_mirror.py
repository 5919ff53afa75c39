"""Float64 references of the training step's stream kernels and the case tables of their tests
(mdf-net_amd/csrc/bn_train.hip, prob_bwd.hip, upsample_bwd.hip, the loss part of loss.hip).

Every reference restates the FORMULA of its entry (the kernels' header comments; net/loss.py, net/unit/base.py:50-68, backbone.py:60-62)
with whole-tensor numpy / torch float64 expressions.  None walks a grid, a tile or a thread's share, so none shares code or structure with
the kernels; tests/test_stream_mirror_cpu.py ties each of them to an independent formulation (nn.BatchNorm3d + ReLU, F.interpolate,
softmax -> sum(prob * hyp), F.conv3d, net/loss.py's Loss, all float64 with autograd).

Two input generators per family.

Exact generator.  Values for which every product and every partial sum is representable in the type the kernel holds it in, whatever the
order of the fp32 per-thread partials, the LDS adds, the fp64 atomics and the FMAs.  The kernel then owes the reference BIT FOR BIT: one
dropped tail element, one wrong group or slice stride, one wrong border tap changes an integer.  The conditions (all magnitudes below
2^24 on the value's dyadic grid, with the worst per-thread element count the launch rules allow) are stated by `fits32` and the
`*_worst` functions here and asserted for every table case by the CPU test.

Random generator.  randn-like data, judged at the bar the kernel's existing test holds in tests/test_train_gpu.py (max|got - ref| / max|ref|
against float64): BN_BAR_FWD / BN_BAR_BWD, PROB_BAR, LOSS_BAR.

Where exactness cannot be had the bar is an fp32 ulp bound derived from the kernel's EXPRESSION (never from its output); with
u = 2^-24 the unit roundoff of fp32 and SLACK covering second-order terms and the fp64 operations (a few 2^-53 (1 + mean^2/var), which
at the tables' mean/std <= 30 is below 2^-40):

  bn_finalize (aux of mdf_bn_finalize_fwd and mdf_bn_finalize_apply_fwd), from fp64 mean, var:
    mean32  = fl(mean)                                one rounding              |err| <= u |mean|
    invstd  = fl(1/sqrt(var+eps))                     one rounding              |err| <= u |invstd|
    a       = fl(gamma * invstd)                      invstd's + the product's  |err| <= 2u |a|
    b       = fl(beta - fl(mean32 * a))               mean32's u, a's 2u, the product's u (absent in a fused form), the subtraction's u
                                                                                |err| <= 4u |mean a| + u |b|
  running statistics, per group in call order, r' = fl(fl(k r) + fl(m x32)), k = fl(1 - m) in fp32, x32 = fl(x) the batch value:
    k's u and the product's u on the first term, x32's u and the product's u on the second, the addition's u (a fused form drops one):
                                                      local |err| <= 2u |k r| + 2u |m x| + u |r'|
    and the error carried in from the previous group is scaled by k:  E_g = k E_(g-1) (1 + 3u) + local_g.
  dy of mdf_bn_relu_bwd with sums the kernels reduced (N not a power of two: m1 = fl(S1 * fl64(1/N)) is not a dyadic number):
    dy = fl(gi * fl(fl(dr - m1) - fl(xh * m2))),  gi, dr, xh exact under the exact generator, m1 and m2 one rounding each:
      dr - m1: m1's u |m1| + u |dr - m1|;  xh m2: m2's u |xh m2| + the product's u |xh m2|;  the subtraction u |t|;  the product u |dy|
                                                      |err| <= u |gi| (|m1| + |dr - m1| + 2 |xh m2| + 2 |t|),   t = dr - m1 - xh m2

Nothing here needs a GPU or reads the reference tree."""
import math

import numpy as np
import torch

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -8
BN_BAR_FWD, BN_BAR_BWD, PROB_BAR, LOSS_BAR = 1e-5, 2e-5, 1e-4, 2e-6
KT = 256
STAT_SLICES = 16          # mdfnet_hip.ops.STAT_SLICES (asserted by the GPU test)


def _gen(*key):
    h = 17
    for v in key:
        h = (h * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def ints(shape, g, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def fits32(bound, grid):
    """A value of magnitude <= bound on the dyadic grid `grid` (a power of two) is an fp32 number, and so is every partial sum of it."""
    return math.log2(grid) == int(math.log2(grid)) and bound / grid < 2 ** 24


def on_grid(t, grid):
    t = torch.as_tensor(t, dtype=torch.float64)
    return bool(torch.equal(torch.round(t / grid) * grid, t))


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-300))


# ------------------------------------------------------------------------------------------------------------ launch rules, restated
def _clamp(g, cap):
    return int(max(1, min(g, cap)))


def grid_for_reduce(n4, groups):           # bn_train.hip: reductions, few fat blocks
    return _clamp(-(-n4 // (4 * KT)), max(512 // groups, 32))


def grid_for(n4, groups):                  # bn_train.hip: apply / backward streams
    return _clamp(-(-n4 // KT), max(2048 // groups, 64))


def grid_x(per_batch):                     # loss.hip
    return _clamp(-(-per_batch // (4 * KT)), 256)


def grid_4096(n):                          # prob_conv_dgrad (n voxels), upsample adjoint (n float4 of the coarse map)
    return _clamp(-(-n // KT), 4096)


def per_thread(n, blocks):
    """Most elements one thread of a `blocks` x 256 grid-stride loop over n elements takes."""
    return -(-n // (blocks * KT))


def softmax_split(B, D, h, w):             # prob_bwd.hip: threads that share a pixel
    n, S = B * h * w, 1
    while S < 8 and n * S < 262144 and 2 * S <= D:
        S *= 2
    return S


def split_cut_by(B, D, h, w):
    """What stopped the doubling: 'cap' (S = 8), 'planes' (2S > D) or 'pixels' (n S >= 262144; decided first where both hold)."""
    S, n = softmax_split(B, D, h, w), B * h * w
    return "cap" if S == 8 else ("pixels" if n * S >= 262144 else "planes")


# ==================================================================================================================== BatchNorm + ReLU
# case = (N, C, groups, nslices, res, running)
BN_CASES = [
    (1, 8, 1, 1, True, True),            # one voxel: n4 = 2, var = 0
    (1, 64, 2, 3, False, False),         # one voxel per group, n4 = 16
    (31, 8, 1, 1, False, True),          # n4 = 62 < 256, odd N
    (127, 8, 1, 3, True, False),         # n4 = 254 = 256 - 2   (n4 = N C / 4 is even for C >= 8: +-2 is as near as a block edge gets)
    (129, 8, 1, 16, True, True),         # n4 = 258 = 256 + 2
    (63, 16, 2, 1, True, True),          # n4 = 252
    (65, 16, 2, 16, False, True),        # n4 = 260
    (513, 16, 5, 3, True, True),         # n4 = 2052 = 8 * 256 + 4: a reduce grid of 3 blocks, an apply grid of 9
    (77, 32, 5, 1, False, False),
    (129, 32, 16, 16, True, True),       # caps 32 / 128
    (33, 64, 16, 3, True, False),
    (95, 64, 40, 1, False, True),        # caps 32 / 64, under both
    (16501, 8, 40, 3, True, True),       # n4 = 33002: past 32 x 1024 and 64 x 256 with 40 groups
    (270001, 8, 1, 16, True, True),      # n4 = 540002 > 524288: past 512 x 1024 and 2048 x 256
]
BN_GROUPS, BN_SLICES, BN_CHANNELS = {1, 2, 5, 16, 40}, {1, 3, 16}, {8, 16, 32, 64}
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
Y_OFF = 11                 # |group/channel offset| <= 11, so |y| <= 14
Y_MAX = 3 + Y_OFF


def bn_id(case):
    n, c, g, s, res, run = case
    return f"N{n}-C{c}-g{g}-s{s}-{'res' if res else 'nores'}-{'run' if run else 'norun'}"


def bn_n4(case):
    return case[0] * case[1] // 4


def _gc(groups, c):
    return torch.arange(groups).view(groups, 1), torch.arange(c).view(1, c)


def bn_exact_inputs(case):
    """y, dz, res [G,N,C] (res None where the case has none), aux [G,4,C], gamma, beta [C]; all float64 holding fp32 values.
    y = integers of {-3..3} plus an integer offset that differs per group and per channel; aux hand-made (a, b, invstd small dyadics,
    mean an integer; b a multiple of 1/8 of at most 21) and NOT consistent with y: a kernel that reads a of another group, or b where mean belongs, changes integers."""
    n, c, groups, _, has_res, _ = case
    g = _gen(1, *case[:4])
    gi, ci = _gc(groups, c)
    off = ((7 * gi + 3 * ci) % 23 - Y_OFF).double()
    y = ints((groups, n, c), g) + off.view(groups, 1, c)
    dz = ints((groups, n, c), g)
    res = ints((groups, n, c), g) if has_res else None
    a = torch.tensor([0.5, -0.25, 1.0, 0.75, -1.5, 0.125], dtype=torch.float64)[(gi + ci) % 6]
    b = -a * (off + ((gi + ci) % 7 - 3).double())      # y a + b is exactly 0 at one of the channel's seven values: the closed side of `> 0`
    mean = ((gi + 2 * ci) % 5 - 2).double()
    invstd = torch.tensor([0.5, 1.0, 2.0, 0.25], dtype=torch.float64)[(gi + ci) % 4]
    aux = torch.stack([a, b, mean, invstd], 1)
    gamma = torch.tensor([0.5, 1.0, 1.5, -0.75], dtype=torch.float64)[torch.arange(c) % 4]
    beta = ((torch.arange(c) % 7) - 3).double() / 4
    return y, dz, res, aux, gamma, beta


def bn_randn_inputs(case, ratios=(0.0,)):
    """randn-like data; channel c has mean/std = ratios[c % len]."""
    n, c, groups, _, has_res, _ = case
    g = _gen(2, *case[:4])
    r = torch.tensor(ratios, dtype=torch.float32)[torch.arange(c) % len(ratios)]
    y = torch.randn(groups, n, c, generator=g) * 2 + 2 * r
    dz = torch.randn(groups, n, c, generator=g)
    res = torch.randn(groups, n, c, generator=g) if has_res else None
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.rand(c, generator=g) * 0.6 - 0.3
    return y.double(), dz.double(), None if res is None else res.double(), gamma.double(), beta.double()


def bn_stats_ref(y):
    """[G,N,C] -> [G,2C]: sum y | sum y^2."""
    return torch.cat([y.sum(1), (y * y).sum(1)], 1)


def bn_apply_ref(y, aux, res):
    z = torch.clamp(y * aux[:, 0:1] + aux[:, 1:2], min=0.0)
    return z if res is None else z + res


def _dr_xhat(dz, y, aux):
    dr = torch.where(y * aux[:, 0:1] + aux[:, 1:2] > 0, dz, torch.zeros_like(dz))
    return dr, (y - aux[:, 2:3]) * aux[:, 3:4]


def bn_bwd_reduce_ref(dz, y, aux):
    """-> [G,2C]: sum dr | sum dr * xhat."""
    dr, xh = _dr_xhat(dz, y, aux)
    return torch.cat([dr.sum(1), (dr * xh).sum(1)], 1)


def bn_bwd_ref(dz, y, aux, tot, gamma):
    """tot [G,2C] = the totals over the slices -> dy [G,N,C], dgamma [C], dbeta [C], and the ulp bound of dy (module docstring)."""
    n, c = y.shape[1], y.shape[2]
    dr, xh = _dr_xhat(dz, y, aux)
    m1, m2 = (tot[:, :c] / n).unsqueeze(1), (tot[:, c:] / n).unsqueeze(1)
    gi = (gamma.view(1, c) * aux[:, 3]).unsqueeze(1)
    t = dr - m1 - xh * m2
    bound = U * SLACK * gi.abs() * (m1.abs() + (dr - m1).abs() + 2 * (xh * m2).abs() + 2 * t.abs())
    return gi * t, tot[:, c:].sum(0), tot[:, :c].sum(0), bound


def bn_finalize_ref(tot, gamma, beta, eps, n, momentum=BN_MOMENTUM, running=None, nbt=0):
    """tot [G,2C] fp64 totals -> aux [G,4,C] and its bound; running = (mean, var) updated as by G successive calls, with its bounds.
    momentum None = nn.BatchNorm's cumulative average (factor 1/num_batches_tracked).  eps, momentum: the fp32 values the kernel is passed."""
    groups, c = tot.shape[0], tot.shape[1] // 2
    mean = tot[:, :c] / n
    var = torch.clamp(tot[:, c:] / n - mean * mean, min=0.0)
    invstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    a = gamma.view(1, c) * invstd
    b = beta.view(1, c) - mean * a
    aux = torch.stack([a, b, mean, invstd], 1)
    bound = U * SLACK * torch.stack([2 * a.abs(), 4 * (mean * a).abs() + b.abs(), mean.abs(), invstd.abs()], 1)
    if running is None:
        return aux, bound, None, None, nbt
    unb = var * n / (n - 1.0) if n > 1 else var
    rm, rv = running[0].clone().double(), running[1].clone().double()
    em, ev = torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    for g in range(groups):
        nbt += 1
        m = 1.0 / nbt if momentum is None else float(np.float32(momentum))
        k = 1.0 - m
        for r, e, x in ((rm, em, mean[g]), (rv, ev, unb[g])):
            new = k * r + m * x
            e.copy_(k * e * (1 + 3 * U) + U * SLACK * (2 * (k * r).abs() + 2 * (m * x).abs() + new.abs()))
            r.copy_(new)
    return aux, bound, (rm, rv), (em, ev), nbt


def spread_over_slices(tot, nslices, salt=0):
    """[G,K] totals -> [nslices,G,K] hand-made copies that add up to them exactly: every entry of the later slices is a distinct
    non-zero multiple of 1/4, except a fifth of them which are exactly 0.0 (the kernels skip zeros); slice 0 holds the rest."""
    groups, k = tot.shape
    out = torch.zeros(nslices, groups, k, dtype=torch.float64)
    idx = torch.arange((nslices - 1) * groups * k).view(nslices - 1, groups, k)
    v = (idx + 1 + salt).double() / 4 * torch.where(idx % 2 == 0, 1.0, -1.0)
    out[1:] = torch.where(idx % 5 == 3, torch.zeros_like(v), v)
    out[0] = tot - out[1:].sum(0)
    return out


def bn_handmade_red(case):
    """Backward sums [G,2C] = N * q with q a multiple of 1/4 of [-2, 2], distinct neighbours, some exactly 0: S/N is then q for ANY N
    (fl32(N q * fl64(1/N)) = q: the fp64 error is far below half an fp32 ulp of q), and dy is exact under the exact generator."""
    n, c, groups = case[0], case[1], case[2]
    gi, ei = torch.arange(groups).view(groups, 1), torch.arange(2 * c).view(1, 2 * c)
    return ((7 * gi + 3 * ei) % 17 - 8).double() / 4 * n


def bn_worst(case):
    """(name, magnitude bound, grid) of every fp32 quantity the BN kernels form under the exact generator."""
    n4, groups = bn_n4(case), case[2]
    m = per_thread(n4, grid_for_reduce(n4, groups))
    xh = (Y_MAX + 2) * 2.0                       # |y - mean| * invstd, on 1/4
    return [("sum y", m * Y_MAX, 1.0), ("sum y^2", m * Y_MAX ** 2, 1.0), ("y a + b", Y_MAX * 1.5 * 2, 1 / 8),
            ("sum dr", m * 3, 1.0), ("sum dr xhat", m * 3 * xh, 0.25), ("z", Y_MAX * 1.5 * 2 + 3, 1 / 8),
            ("dr - m1 - xh m2", 3 + 2 + xh * 2, 1 / 16), ("dy", 1.5 * 2 * (5 + xh * 2), 1 / 256),
            ("dgamma, dbeta", case[0] * groups * 2.0, 0.25)]


# ==================================================================================================================== softmax / regress backward
# case = (B, D, h, w, per_pixel)
SOFTMAX_CASES = [
    (1, 1, 1, 1, 0),           # S = 1 by the planes; one pixel
    (2, 1, 3, 5, 1),
    (1, 2, 1, 127, 1),         # S = 2; 127 = 128 - 1
    (3, 3, 1, 43, 0),          # S = 2, D % S != 0; 129 = 128 + 1
    (1, 5, 7, 9, 1),           # S = 4, D % S != 0; 63 = 64 - 1
    (5, 5, 1, 13, 0),          # 65 = 64 + 1
    (1, 8, 3, 11, 0),          # S = 8; 33 = 32 + 1
    (1, 9, 1, 31, 1),          # S = 8, D % S != 0; 31 = 32 - 1
    (3, 24, 5, 7, 1),
    (2, 48, 4, 8, 0),
    (1, 8, 250, 280, 1),       # 70000 pixels: S = 4, cut by the pixel count although D allows 8
    (1, 3, 511, 515, 0),       # 263165 pixels >= 262144: S = 1 although D allows 2; not a multiple of 256
]
SOFTMAX_FORMS = ("ddepth+dprob", "ddepth", "dprob", "dprob-nohypos")
SOFTMAX_D = {1, 2, 3, 5, 8, 9, 24, 48}


def softmax_id(case):
    return "B{}-D{}-{}x{}-pp{}".format(*case)


def softmax_exact_inputs(case):
    """prob multiples of 1/16 that add up to exactly 1 per pixel (sixteen sixteenths thrown at random planes: not a real softmax, but the
    kernel's bracket (h - m) - sum p (h - m) is the header's h - M only where sum p = 1), hypos integers of [400, 1000], ddepth integers
    of {-3..3}, dprob multiples of 1/8 of [-2, 2]."""
    B, D, h, w, pp = case
    g = _gen(3, *case)
    k = torch.zeros(B, D, h, w, dtype=torch.int64)
    k.scatter_add_(1, torch.randint(0, D, (B, 16, h, w), generator=g), torch.ones(B, 16, h, w, dtype=torch.int64))
    prob = k.double() / 16
    hyp = ints((B, D, h, w) if pp else (B, D, 1, 1), g, 400, 1000)
    return prob, hyp, ints((B, h, w), g), ints((B, D, h, w), g, -16, 16) / 8


def softmax_randn_inputs(case):
    B, D, h, w, pp = case
    g = _gen(4, *case)
    prob = torch.softmax(2 * torch.randn(B, D, h, w, generator=g), 1)
    hyp = 425 + 500 * torch.rand((B, D, h, w) if pp else (B, D, 1, 1), generator=g)
    return prob.double(), hyp.double(), torch.randn(B, h, w, generator=g).double(), 0.1 * torch.randn(B, D, h, w, generator=g).double()


def softmax_regress_bwd_ref(prob, hyp, ddepth, dprob):
    """dlogit[d] = p[d] (g[d] - sum_k p[k] g[k]),  g = ddepth * hyp (+ dprob); a missing cotangent contributes nothing."""
    g = torch.zeros_like(prob)
    if ddepth is not None:
        g = g + ddepth.unsqueeze(1) * hyp
    if dprob is not None:
        g = g + dprob
    return prob * (g - (prob * g).sum(1, keepdim=True))


def softmax_worst():
    """The kernel's own expression, dlogit = p (dd ((h - m) - c) + (dp - mp)), m = sum p h, c = sum p (h - m), mp = sum p dp, under the
    exact generator (p = k/16, sum p = 1, so m lies among the hypotheses and c = 0; a thread's partial sums are bounded by the sums of
    magnitudes): (name, magnitude bound, grid).  dlogit = (k/16) g: k g <= 16 |g| is on g's grid, the division only shifts the exponent."""
    return [("m", 1000.0, 1 / 16), ("h - m", 600.0, 1 / 16), ("c", 600.0, 1 / 256), ("(h - m) - c", 1200.0, 1 / 256),
            ("mp", 2.0, 1 / 128), ("dp - mp", 4.0, 1 / 128), ("g", 3 * 1200.0 + 4, 1 / 256), ("16 dlogit", 16 * 3604.0, 1 / 256)]


# ==================================================================================================================== prob conv dgrad
# case = (B, D, H, W, C, nslices)
DGRAD_CASES = [
    (1, 1, 1, 1, 8, 1), (1, 1, 1, 1, 16, 3),               # only the centre tap lands inside
    (1, 1, 3, 5, 8, 16), (1, 1, 3, 5, 16, 1),
    (3, 2, 2, 2, 8, 3), (3, 2, 2, 2, 16, 16),              # more slices than blocks
    (2, 5, 13, 37, 8, 16), (2, 5, 13, 37, 16, 3), (2, 5, 13, 37, 8, 1),      # 19 blocks over 16, 3 and 1 slices
    (1, 9, 350, 340, 8, 16),       # 1,071,000 voxels: past 4096 x 256, the stride loop runs
]
DGRAD_SLICES = {1, 3, 16}


def dgrad_id(case):
    return "{}x{}x{}x{}-C{}-s{}".format(*case)


def dgrad_voxels(case):
    return case[0] * case[1] * case[2] * case[3]


def dgrad_exact_inputs(case):
    """dlogit [B,D,H,W], w [1,C,3,3,3] integers of {-3..3}; stat_y [n,C] as the BN generator's y, stat_aux [4,C] hand-made."""
    B, D, H, W, C, _ = case
    g = _gen(5, *case)
    gi, ci = _gc(1, C)
    y = ints((dgrad_voxels(case), C), g) + ((3 * ci) % 23 - Y_OFF).double()
    aux = bn_exact_inputs((1, C, 1, 1, False, False))[3][0]
    return ints((B, D, H, W), g), ints((1, C, 3, 3, 3), g), y, aux


def dgrad_randn_inputs(case):
    B, D, H, W, C, _ = case
    g = _gen(6, *case)
    y = torch.randn(dgrad_voxels(case), C, generator=g).double()
    aux = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2,
                       torch.rand(C, generator=g) + 0.5]).float().double()
    return torch.randn(B, D, H, W, generator=g).double(), (0.2 * torch.randn(1, C, 3, 3, 3, generator=g)).double(), y, aux


def prob_conv_dgrad_ref(dlogit, w):
    """dx[o][c] = sum_tap dlogit[o - tap + 1] W[c][tap] (zero outside the volume) -> [B,D,H,W,C]: one shifted product per tap."""
    B, D, H, W = dlogit.shape
    C = w.shape[1]
    pad = torch.zeros(B, D + 2, H + 2, W + 2, dtype=torch.float64)
    pad[:, 1:-1, 1:-1, 1:-1] = dlogit
    dx = torch.zeros(B, D, H, W, C, dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                sl = pad[:, 2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]
                dx += sl.unsqueeze(-1) * w[0, :, kd, kh, kw]
    return dx


def dgrad_stat_ref(dx, y, aux):
    """The backward sums of the layer dx is the complete dz of -> [2C]."""
    c = y.shape[1]
    return bn_bwd_reduce_ref(dx.reshape(1, -1, c), y.view(1, -1, c), aux.view(1, 4, c))[0]


def dgrad_worst(case):
    m = per_thread(dgrad_voxels(case), grid_4096(dgrad_voxels(case)))
    xh = (Y_MAX + 2) * 2.0
    return [("dx", 27 * 9.0, 1.0), ("row sum dr", 16 * m * 243.0, 1.0), ("row sum dr xhat", 16 * m * 243.0 * xh, 0.25)]


# ==================================================================================================================== upsample adjoint
# case = (B, h, w, C) of the COARSE map
UP_CASES = [(1, 1, 1, 4), (2, 1, 5, 8), (1, 5, 1, 4), (1, 2, 2, 16), (3, 7, 9, 32), (1, 37, 50, 64),
            (1, 260, 257, 64)]     # 1,069,120 float4 > 4096 x 256


def up_id(case):
    return "{}x{}x{}x{}".format(*case)


def up_float4(case):
    return case[0] * case[1] * case[2] * case[3] // 4


def up_exact_inputs(case):
    B, h, w, C = case
    g = _gen(7, *case)
    return ints((B, 2 * h, 2 * w, C), g), ints((B, h, w, C), g, -50, 50)       # dfine, what dcoarse holds before an accumulating call


def up_randn_inputs(case):
    B, h, w, C = case
    g = _gen(8, *case)
    return torch.randn(B, 2 * h, 2 * w, C, generator=g).double(), torch.randn(B, h, w, C, generator=g).double()


def up_matrix(n):
    """[2n, n]: fine[2j] = 0.25 c[j-1] + 0.75 c[j], fine[2j+1] = 0.75 c[j] + 0.25 c[j+1], indices clamped at the border."""
    m = torch.zeros(2 * n, n, dtype=torch.float64)
    for j in range(n):
        m[2 * j, max(j - 1, 0)] += 0.25
        m[2 * j, j] += 0.75
        m[2 * j + 1, j] += 0.75
        m[2 * j + 1, min(j + 1, n - 1)] += 0.25
    return m


def upsample2_bwd_ref(dfine, before=None):
    """dcoarse = up^T dfine (+ what dcoarse held, for an accumulating call)."""
    _, h2, w2, _ = dfine.shape
    out = torch.einsum("iy,bijc,jx->byxc", up_matrix(h2 // 2), dfine, up_matrix(w2 // 2))
    return out if before is None else out + before


# ==================================================================================================================== loss
# per-batch pixel counts of the scales, in order: a case with k scales takes the first k
LOSS_PIXELS = [263001, 1, 255, 72 * 96, 257, 255, 1, 300, 77]
# case = (scales, B, floor form, null scale or None, empty scale or None, dloss)
LOSS_CASES = [
    (1, 1, "f64", None, None, 1.0),
    (4, 3, "f32", None, None, 1.0),
    (8, 3, "f64-stride2", 3, None, 0.75),
    (4, 1, "f32-0dim", 1, None, -2.5),
    (8, 1, "f64", None, 2, 1.0),          # scale 2 has no valid pixel
    (4, 3, "f64-0dim", None, 1, 0.75),
]
LOSS_FLOORS = {"f64": [425.0, 300.0 + 1e-7, 512.5], "f32": [425.0, 300.0, 512.5], "f64-stride2": [425.0, 300.0 + 1e-7, 512.5],
               "f32-0dim": [0.0], "f64-0dim": [300.0 + 1e-7]}


def loss_id(case):
    return "s{}-B{}-{}-null{}-empty{}-dl{}".format(*case)


def loss_floor(case):
    """-> (the tensor the entries get, floor per batch element as float64 [B]).  0-dim forms serve every batch element (stride 0);
    the strided form is every second element of a longer vector."""
    _, B, form, _, _, _ = case
    dt = torch.float64 if form.startswith("f64") else torch.float32
    vals = LOSS_FLOORS[form]
    if form.endswith("0dim"):
        t = torch.tensor(vals[0], dtype=dt)
        return t, t.double().expand(B).clone()
    if form.endswith("stride2"):
        base = torch.full((2 * B,), -1e9, dtype=dt)
        base[0::2] = torch.tensor(vals[:B], dtype=dt)
        return base, base[0::2].double().clone()
    t = torch.tensor(vals[:B], dtype=dt)
    return t, t.double().clone()


def _next_f32(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def loss_exact_inputs(case):
    """-> [(est, gt)] float32 [B, pixels].  gt: multiples of 1/4 above the floor, a third of the pixels 0 or below the floor (invalid),
    and the floor's own boundary values; est - gt: multiples of 1/8 with |d| <= 4, and the smooth-L1 boundary |d| = 1 -+ one ulp where
    the floor is 0 (only there are 1 - 2^-24 and 1 + 2^-23 differences of two fp32 numbers above the floor)."""
    ns, B, form, _, empty, _ = case
    _, fl = loss_floor(case)
    g = _gen(9, ns, B, len(form))
    out = []
    for s in range(ns):
        n = LOSS_PIXELS[s]
        base = torch.ceil(fl).view(B, 1)
        gt = base + torch.randint(1, 1200, (B, n), generator=g).double() / 4
        invalid = torch.randint(0, 3, (B, n), generator=g) == 0
        gt = torch.where(invalid, torch.where(torch.randint(0, 2, (B, n), generator=g) == 0, torch.zeros_like(gt), base - 8.0), gt)
        d = torch.randint(-32, 33, (B, n), generator=g).double() / 8
        if n >= 8:
            for b in range(B):
                f32 = float(np.float32(fl[b].item()))
                gt[b, 0] = f32                              # the floor itself (rounded to fp32): never above the fp32 floor
                gt[b, 1] = _next_f32(f32)                   # the next fp32 above it
                if f32 == 0.0:
                    d[b, 1] = 0.0                           # (a subnormal: est = gt is the only estimate that keeps est - gt exact)
                gt[b, 2], d[b, 2] = base[b, 0] + 1, 1.0
                gt[b, 3], d[b, 3] = base[b, 0] + 1, -1.0
        elif empty != s:
            gt[:, 0] = base[:, 0] + 0.25                    # a one-pixel scale is valid unless it is the empty one
        if empty == s:
            gt = torch.where(torch.randint(0, 2, (B, n), generator=g) == 0, torch.zeros_like(gt), base.expand(B, n) - 8.0)
        est = gt + d
        if form == "f32-0dim" and n >= 16:                  # floor 0
            e1, e2 = 2.0 ** -23, 2.0 ** -24
            for i, (gv, ev) in enumerate([(0.5, 1.5 + e1), (e2, 1.0), (1.5 + e1, 0.5), (1.0, e2), (0.5, 1.5 - e1), (1.5, 0.5 + e2)]):
                gt[:, 8 + i], est[:, 8 + i] = gv, ev
        assert torch.equal(gt.float().double(), gt) and torch.equal(est.float().double(), est)
        out.append((est.float(), gt.float()))
    return out


def loss_randn_inputs(case):
    ns, B = case[0], case[1]
    _, fl = loss_floor(case)
    g = _gen(10, ns, B)
    out = []
    for s in range(ns):
        n = LOSS_PIXELS[s]
        gt = fl.view(B, 1).float() + torch.rand(B, n, generator=g) * 500 - 100
        out.append((gt + torch.randn(B, n, generator=g) * 1.5, gt))
    return out


def loss_reduce_ref(est, gt, fl):
    """-> (sum of smooth-L1 over gt > floor, count) as float64.  The per-pixel value is the kernel's fp32 expression, operation by
    operation: d = e - g; |d| < 1 ? (0.5 d) d : |d| - 0.5; the sum of those fp32 values is taken in float64."""
    e, g = est.numpy().astype(np.float32), gt.numpy().astype(np.float32)
    d = e - g
    a = np.abs(d)
    v = np.where(a < np.float32(1.0), (np.float32(0.5) * d) * d, a - np.float32(0.5)).astype(np.float32)
    valid = g.astype(np.float64) > fl.numpy().reshape(-1, 1)
    return float(np.sum(np.where(valid, v.astype(np.float64), 0.0))), float(valid.sum())


def loss_reduce_f64(est, gt, fl):
    """The same in float64 throughout (the random generator's reference)."""
    d = est.double() - gt.double()
    a = d.abs()
    v = torch.where(a < 1, 0.5 * d * d, a - 0.5)
    valid = gt.double() > fl.view(-1, 1)
    return float(torch.where(valid, v, torch.zeros_like(v)).sum()), float(valid.sum())


def loss_finalize_ref(acc):
    """acc [2 ns] float64 -> (loss, inv_count [ns]) float32, in the kernel's types: an fp64 divide rounded to fp32 per scale, the
    fp32 adds over the scales in order."""
    acc = np.asarray(acc, dtype=np.float64)
    total = np.float32(0.0)
    inv = np.zeros(len(acc) // 2, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(len(inv)):
            total = np.float32(total + np.float32(acc[2 * s] / acc[2 * s + 1]))
            inv[s] = np.float32(np.float64(1.0) / acc[2 * s + 1])
    return total, inv


def loss_bwd_ref(est, gt, fl, dloss, inv_count):
    """de = (dloss * inv_count) * clamp(e - g, -1, 1) on gt > floor, 0 elsewhere: one fp32 multiply for the scale, one per gradient."""
    e, g = est.numpy().astype(np.float32), gt.numpy().astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        scale = np.float32(np.float32(dloss) * np.float32(inv_count))
        valid = g.astype(np.float64) > fl.numpy().reshape(-1, 1)
        de = np.where(valid, scale * np.clip(e - g, np.float32(-1.0), np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(de)


def loss_bwd_f64(est, gt, fl, dloss, count):
    d = torch.clamp(est.double() - gt.double(), -1.0, 1.0)
    return torch.where(gt.double() > fl.view(-1, 1), d * (dloss / count), torch.zeros_like(d))
