"""Float64 reference of the weight-gradient correlation (mdf-net_amd/csrc/wgrad.hip, wgrad_lds.hip) and the case tables of its tests.

The kernels compute one correlation for every layer kind,
    dw[a][b][tap] = sum over voxels o of  small[o][a] * big[s*o + tap - pad][b]          (zero outside `big`)
with Conv3d / Conv2d: small = dy, big = x; ConvTranspose3d(k3,s2,p1,op1): small = x, big = dy (twice the size), s = 2.
`wgrad_ref` writes that sum out with slices and one einsum per tap; it calls no conv backward, so it shares no code with what
tests/test_wgrad_mirror_cpu.py ties it to (float64 autograd of F.conv3d, F.conv_transpose3d and F.conv2d).

Why integers.  With fp32 inputs that hold integers of {-3 .. 3}, every product is an integer of magnitude <= 9 and every partial sum of
at most `voxels` products is an integer of magnitude <= 9 * voxels: below 2^24 all of them are fp32 values, so the sums are exact in ANY
order -- through the MFMA chains, the LDS partial sums, the slabs and the fp32 atomics of the slab sums.  The kernels then owe the
float64 reference bit for bit; one dropped, duplicated or misplaced voxel changes an integer.  `exact_for` is the condition.

Nothing here needs a GPU or reads the reference tree."""
import torch
import torch.nn.functional as F

INT_LO, INT_HI = -3, 3
RANDN_BAR = 3e-5          # max|got - ref| / max|ref| of the randn pass: the bar the kernels' existing tests hold (tests/test_train_gpu.py)


def wgrad_ref(small, big, stride, ksize, three_d):
    """small [B,(Ds,)Hs,Ws,A], big [B,(s*Ds,)s*Hs,s*Ws,Bc] channels-last -> float64 dw [A,Bc,(k,)k,k] (torch's weight layout)."""
    s, k = int(stride), int(ksize)
    pad = (k - 1) // 2
    sm, bg = small.double(), big.double()
    if not three_d:
        sm, bg = sm.unsqueeze(1), bg.unsqueeze(1)
    _, Ds, Hs, Ws, A = sm.shape
    Bc = bg.shape[-1]
    pd = pad if three_d else 0
    bp = F.pad(bg, (0, 0, pad, pad, pad, pad, pd, pd))
    nd = k if three_d else 1
    out = torch.zeros(A, Bc, nd, k, k, dtype=torch.float64)
    for kd in range(nd):
        for kh in range(k):
            for kw in range(k):
                sl = bp[:, kd:kd + s * Ds:s, kh:kh + s * Hs:s, kw:kw + s * Ws:s]
                out[:, :, kd, kh, kw] = torch.einsum("ndhwa,ndhwb->ab", sm, sl)
    return out if three_d else out[:, :, 0]


# ---------------------------------------------------------------------------------------------------------------- layer kinds
# kind -> (stride, ksize, [(A, Bc), ..]); A = channels of `small`
KINDS_3D = {
    "conv_s1": (1, 3, [(16, 32), (16, 16), (32, 32), (64, 64), (8, 16), (8, 8)]),
    "conv_s2": (2, 3, [(32, 16), (64, 32), (16, 8)]),
    "convT_s2": (2, 3, [(64, 32), (32, 16), (16, 8)]),          # small = x, big = dy
    "prob_s1": (1, 3, [(1, 8), (1, 16), (1, 4)]),
}
KINDS_2D = {
    "k3_s1": (1, 3, [(8, 4), (8, 8), (16, 16), (32, 32), (64, 64), (32, 8), (1, 8), (8, 1)]),
    "k5_s2": (2, 5, [(16, 8), (32, 16), (64, 32)]),
    "k1": (1, 1, [(64, 64), (64, 32), (32, 64), (64, 16), (16, 64)]),
}

# ---------------------------------------------------------------------------------------------------------------- shapes (of `small`)
SHAPES_3D = [
    (1, 1, 1, 1),        # only the centre tap is non-zero: the kd = 0 and kd = 2 blocks must deliver exact zeros
    (1, 1, 3, 5),        # a single plane, narrower than one 16-voxel chunk
    (3, 2, 2, 2),        # batch 3, two planes
    (2, 3, 5, 17),       # odd height under two-row tiles, one voxel past a chunk
    (1, 2, 7, 33),       # two planes, odd height, one voxel past two chunks
    (2, 5, 9, 20),       # a tile walk: more tiles than blocks for the 64 x 64 kind, across images and dead kd planes
]
SHAPES_2D = [(1, 1, 1), (3, 2, 2), (2, 5, 17), (1, 7, 33), (3, 9, 70)]
SWEEP_W = [15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
SWEEP_3D = [("conv_s1", 16, 16), ("conv_s2", 32, 16), ("convT_s2", 32, 16)]          # one unpacked kind of each stride class
SWEEP_2D = [("k5_s2", 32, 16), ("k1", 64, 32)]
SWEEP_BASE_3D = (1, 4, 3)        # (B, Ds, Hs), W appended
SWEEP_BASE_2D = (2, 3)           # (B, Hs)
# the reduced table of the child processes that run the direct forms: every kind at these two shapes
REDUCED_3D = [(1, 1, 1, 1), (2, 3, 5, 17)]
REDUCED_2D = [(1, 1, 1), (2, 5, 17)]


def _table(kinds, shapes, three_d):
    return [(three_d, kind, a, bc, shape) for kind, (_, _, pairs) in kinds.items() for (a, bc) in pairs for shape in shapes]


def cases_3d():
    return _table(KINDS_3D, SHAPES_3D, True)


def cases_2d():
    return _table(KINDS_2D, SHAPES_2D, False)


def sweep_cases():
    out = [(True, kind, a, bc, SWEEP_BASE_3D + (w,)) for (kind, a, bc) in SWEEP_3D for w in SWEEP_W]
    return out + [(False, kind, a, bc, SWEEP_BASE_2D + (w,)) for (kind, a, bc) in SWEEP_2D for w in SWEEP_W]


def reduced_cases():
    return _table(KINDS_3D, REDUCED_3D, True) + _table(KINDS_2D, REDUCED_2D, False)


def all_cases():
    return cases_3d() + cases_2d() + sweep_cases()


def stride_ksize(three_d, kind):
    s, k, _ = (KINDS_3D if three_d else KINDS_2D)[kind]
    return s, k


def case_id(case):
    three_d, kind, a, bc, shape = case
    return f"{'3d' if three_d else '2d'}-{kind}-{a}x{bc}-" + "x".join(map(str, shape))


def voxels(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def exact_for(shape):
    """Every partial sum of integer inputs of {-3 .. 3} over `shape` voxels is an fp32 value."""
    return max(abs(INT_LO), abs(INT_HI)) ** 2 * voxels(shape) < 2 ** 24


def _seed(case, salt):
    three_d, kind, a, bc, shape = case
    h = 17 + salt
    for v in (int(three_d), sum(map(ord, kind)), a, bc) + tuple(shape):
        h = (h * 1000003 + v) % (2 ** 31 - 1)
    return h


def operand_shapes(case):
    three_d, kind, a, bc, shape = case
    s, _ = stride_ksize(three_d, kind)
    return tuple(shape) + (a,), (shape[0],) + tuple(s * v for v in shape[1:]) + (bc,)


def int_inputs(case, salt=0):
    """fp32 (small, big) holding integers drawn uniformly from {-3 .. 3}; `salt` gives the jobs of one batch their own data."""
    assert exact_for(case[4]), case
    g = torch.Generator().manual_seed(_seed(case, 2 * salt))
    ss, bs = operand_shapes(case)
    return (torch.randint(INT_LO, INT_HI + 1, ss, generator=g).float(), torch.randint(INT_LO, INT_HI + 1, bs, generator=g).float())


def randn_inputs(case):
    g = torch.Generator().manual_seed(_seed(case, 1))          # (odd salts: never the data of an integer case)
    ss, bs = operand_shapes(case)
    return torch.randn(ss, generator=g), torch.randn(bs, generator=g)


def ref_of(case, small, big):
    three_d, kind = case[0], case[1]
    s, k = stride_ksize(three_d, kind)
    return wgrad_ref(small, big, s, k, three_d)
