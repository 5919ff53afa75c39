"""TEST INFRASTRUCTURE (CPU): the float64 reference, the case table and the band tools of the fused depth-map consistency filter
(csrc/consistency.hip, entry mdf_consistency_fuse_fwd, ops.consistency_fuse).  tests/test_filter_mirror_cpu.py asserts the
preconditions on the CPU, tests/test_filter_parity_gpu.py compares the kernel; both import the table from here.

REFERENCE.  `fuse64(scene)` is the whole operation of tools/filter/dynamic_filter_gpu.py (reproject_with_depth,
check_geometric_consistency, the fusion of filter()) in numpy float64 from the fp32 inputs, with its own float64 matrix inverses:
reprojection, zero-padded bilinear sampling at the projected pixel (grid_sample(align_corners=True) of 2x/(w-1)-1 samples AT x),
back-projection, dist, rel, the nine nested masks, the counts, geo >= nconditions, photo = conf > fp32(photo_threshold) and
depth_avg.  It shares no code with oracle/filter_oracle.py.  The thresholds are the exact doubles i / thre.

CASES.  `CASES` holds the shapes, view counts, scene edits, value plants and arguments; `scene(name)` builds one from
oracle.gen_golden.filter_scene (scene synthesis only).  Edits change a camera (or a whole view) AFTER the synthesis, so an edited view
need not agree with the surface any more -- the filter then rejects it, through the paths the edit is there to exercise.
  shift     view 1's camera moves 40 mm in x: a quarter of its projections leave the map (zero-padded taps, clamped corner indices)
  behind    view 1's camera turns 180 degrees about its y axis: every point is behind it (q2 < 0)
  copy      the last view becomes an exact copy of the reference camera and depth map
  kdist     every view gets a K of its own (focal lengths and principal point)
  unit      every K and E is the identity, the reference depth is 1 and view 1's depth is 1 except at 27 pixels holding 1 - t for
            t = each rel threshold fp32(i / thre2) and its two fp32 neighbours.  The pixel projects onto itself and
            depth_reprojected is the source depth, exactly, so rel == t exactly where 1 - t is representable (t >= 0.5, i.e. i >= 4
            at thre2 = 6.1): the only scene whose masks tell thresholds one ulp apart from each other.  3 x 1025 so that (w - 1) / 2
            and (h - 1) / 2 are powers of two and the 27 decisions are under the band's cap
Plants write the six values PLANT_VALUES (0, a negative depth, NaN, +inf, a denormal, 1e30):
  ref       into six pixels of the reference depth
  src       into six pixels of view 1's depth
  border    along all four border rows / columns of view 1's depth, the pixels out-of-map taps are clamped onto
  conf      NaN, fp32(photo_threshold) and its two fp32 neighbours into four pixels of the confidence map
A `copy` case carries no plants: its projections land on integer pixel positions up to rounding, so WHICH neighbour gets the
(near-zero) second weight differs between fp32 and float64 -- next to a NaN / inf / 1e30 pixel that is a NaN on one side only, at any
distance from a threshold.  (The bit-exact checks do not need float64 and a copied view of a planted reference is covered by `ref`.)

BAND.  Decisions (pixel, view, threshold) are compared with float64 outside a relative band around the threshold: a decision is left
out when |dist64 - td| <= BAND td or |rel64 - tr| <= BAND tr.  BAND is 2 x the largest relative distance from a threshold at which a
single comparison (dist < td, rel < tr) of the fp32 explicit oracle disagrees with float64 over the whole table, measured by
tests/test_filter_mirror_cpu.py (which also holds it against the cap: at most 1e-3 of any case's decisions inside the band).
"""
import functools
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import filter_oracle as FO  # noqa: E402

T = torch.from_numpy
MAX_SRC_VIEWS = 16                      # MDF_MAX_SRC_VIEWS
BLOCK = 256                             # threads per block of consistency_fuse_kernel
BAND = 1.0e-4                           # see BAND above: 2 x 4.72e-5 (kdist_17x259_n2), rounded up; test_band_is_twice_the_measured_flip_distance
BAND_CAP = 1e-3                         # share of a case's decisions the band may leave out
PLANT_VALUES = np.array([0.0, -3.5, np.nan, np.inf, 1e-40, 1e30], dtype=np.float32)
UNIT_X0, UNIT_DX = 7, 100               # the `unit` edit plants threshold i (i = 2..10) in column UNIT_X0 + UNIT_DX (i - 2), rows 0..2
THRES = ((4, 1300.0), (3.3, 1234.56), (4.7, 1500.3), (2.9, 6.1))


# ==================================================================================================================== case table
def _case(name, h, w, n_src, edits=(), plants=(), nconditions=5, thre=(4, 1300.0), photo=0.8, seed=5, aten=True):
    assert not ("copy" in edits and plants), "see the module docstring"
    return NS(name=name, h=h, w=w, n_src=n_src, edits=tuple(edits), plants=tuple(plants), nconditions=nconditions, thre1=thre[0],
              thre2=thre[1], photo=photo, seed=seed, aten=aten)


SHAPES = ((2, 2, 1), (15, 17, 1), (16, 16, 2), (13, 21, 3), (17, 259, 2), (31, 33, 16), (61, 67, 10))
ALL_PLANTS = ("ref", "src", "border", "conf")


def _table():
    t = [_case(f"shape_{h}x{w}_n{n}", h, w, n) for h, w, n in SHAPES]
    for h, w, n in ((13, 21, 3), (17, 259, 2)):
        s = f"{h}x{w}_n{n}"
        t += [_case(f"{e}_{s}", h, w, n, edits=(e,)) for e in ("shift", "behind", "copy", "kdist")]
        t += [_case(f"plants_{s}", h, w, n, plants=ALL_PLANTS),
              _case(f"shift_border_{s}", h, w, n, edits=("shift",), plants=("border",)),      # out-of-map taps clamped onto NaN / inf
              _case(f"behind_kdist_plants_{s}", h, w, n, edits=("behind", "kdist"), plants=ALL_PLANTS),
              _case(f"shift_plants_photo0_{s}", h, w, n, edits=("shift",), plants=ALL_PLANTS, photo=0.0)]
        t += [_case(f"thre{i}_{s}", h, w, n, thre=THRES[i], plants=("ref", "src", "conf")) for i in (1, 2, 3)]
    t += [_case("plants_2x2_n1", 2, 2, 1, plants=("conf",), photo=0.0),
          _case("plants_15x17_n1", 15, 17, 1, edits=("shift",), plants=ALL_PLANTS),
          _case("plants_61x67_n10", 61, 67, 10, edits=("shift", "kdist"), plants=ALL_PLANTS),
          _case("copy_31x33_n16", 31, 33, 16, edits=("copy", "kdist"))]
    t += [_case("unit_3x1025_n1", 3, 1025, 1, edits=("unit",), thre=THRES[3])]
    t += [_case(f"ncond{c}_31x33_n16", 31, 33, 16, nconditions=c) for c in (0, 1, 9, 10)]
    t += [_case(f"ncond{c}_61x67_n10", 61, 67, 10, nconditions=c, plants=("ref", "src")) for c in (0, 1, 9, 10)]
    t += [_case(f"thre{i}_61x67_n10", 61, 67, 10, thre=THRES[i], edits=("shift",)) for i in (1, 2, 3)]
    t += [_case(f"thre{i}_31x33_n16", 31, 33, 16, thre=THRES[i], photo=0.0, plants=("conf",)) for i in (1, 3)]
    assert len({c.name for c in t}) == len(t)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def _rot_y_pi():
    r = np.eye(4, dtype=np.float32)
    r[0, 0] = r[2, 2] = -1.0
    return r


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> NS(depths [V,h,w], conf [h,w], K [V,3,3], E [V,4,4]: read-only float32 numpy, view 0 = reference; case)."""
    from oracle.gen_golden import filter_scene
    c = BY_NAME[name]
    d, conf, K, E = (a.copy() for a in filter_scene(h=c.h, w=c.w, nsrc=c.n_src, seed=c.seed))
    rng = np.random.RandomState(1000 + c.seed)
    if "kdist" in c.edits:
        for v in range(c.n_src + 1):
            K[v, 0, 0] *= np.float32(1 + 0.011 * v)
            K[v, 1, 1] *= np.float32(1 - 0.007 * v)
            K[v, 0, 2] += np.float32(0.37 * v)
            K[v, 1, 2] -= np.float32(0.21 * v)
    if "unit" in c.edits:
        K[:], E[:], d[:] = np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32), np.float32(1)
        for j, i in enumerate(range(2, 11)):
            t = np.float32(i / c.thre2)
            for r, tt in enumerate((np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf)))):
                d[1][r, UNIT_X0 + UNIT_DX * j] = np.float32(1) - tt
    if "shift" in c.edits:
        E[1, 0, 3] += np.float32(40.0)
    if "behind" in c.edits:
        E[1] = _rot_y_pi() @ E[1]
    if "copy" in c.edits:
        d[-1], K[-1], E[-1] = d[0], K[0], E[0]
    pick = rng.permutation(c.h * c.w)
    if "ref" in c.plants:
        d[0].reshape(-1)[pick[:6]] = PLANT_VALUES
    if "src" in c.plants:
        d[1].reshape(-1)[pick[6:12]] = PLANT_VALUES
    if "border" in c.plants:
        d[1][0, :] = PLANT_VALUES[np.arange(c.w) % 6]
        d[1][-1, :] = PLANT_VALUES[(np.arange(c.w) + 3) % 6]
        d[1][:, 0] = PLANT_VALUES[(np.arange(c.h) + 1) % 6]
        d[1][:, -1] = PLANT_VALUES[(np.arange(c.h) + 4) % 6]
    if "conf" in c.plants:
        thr = np.float32(c.photo)
        conf.reshape(-1)[pick[-4:]] = [np.nan, thr, np.nextafter(thr, np.float32(np.inf)), np.nextafter(thr, np.float32(-np.inf))]
    for a in (d, conf, K, E):
        a.setflags(write=False)
    return NS(depths=d, conf=conf, K=K, E=E, case=c)


def tensors(sc):
    """The scene as the argument tuple of ops.consistency_fuse / FO.fuse_view (CPU tensors; copies, the scene stays read-only)."""
    n = sc.depths.shape[0]
    t = lambda a: T(a.copy())  # noqa: E731
    return (t(sc.depths[0]), t(sc.conf), t(sc.K[0]), t(sc.E[0]), [t(sc.depths[v]) for v in range(1, n)],
            [t(sc.K[v]) for v in range(1, n)], [t(sc.E[v]) for v in range(1, n)])


# ==================================================================================================================== float64 reference
def _sample64(src, x, y):
    """Zero-padded bilinear sample of src [h,w] (float64) at pixel positions x, y [N]; a tap outside the map contributes 0 whatever the
    map holds, a non-finite position gives NaN."""
    h, w = src.shape
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0
        out = np.zeros_like(x)
        for dx, dy, wt in ((0, 0, (1 - fy) * (1 - fx)), (1, 0, (1 - fy) * fx), (0, 1, fy * (1 - fx)), (1, 1, fy * fx)):
            xt, yt = x0 + dx, y0 + dy
            inside = (xt >= 0) & (xt <= w - 1) & (yt >= 0) & (yt <= h - 1)
            xi = np.where(inside, xt, 0).astype(np.int64)
            yi = np.where(inside, yt, 0).astype(np.int64)
            out = out + np.where(inside, src[yi, xi], 0.0) * wt
    return out


def reproject64(d_ref, k_ref, e_ref, d_src, k_src, e_src):
    """-> depth_reprojected, x_reprojected, y_reprojected, x_src, y_src, z_src (the depth in the source camera)  [h,w] float64."""
    h, w = d_ref.shape
    d_ref, k_ref, e_ref, d_src, k_src, e_src = (np.asarray(a, dtype=np.float64) for a in (d_ref, k_ref, e_ref, d_src, k_src, e_src))
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y, d = xs.ravel(), ys.ravel(), d_ref.ravel()
    one = np.ones_like(x)
    with np.errstate(all="ignore"):
        cam = np.linalg.inv(k_ref) @ np.stack([x * d, y * d, d])
        in_src = ((e_src @ np.linalg.inv(e_ref)) @ np.vstack([cam, one]))[:3]
        q = k_src @ in_src
        x_src, y_src = q[0] / q[2], q[1] / q[2]
        samp = _sample64(d_src, x_src, y_src)
        back = np.linalg.inv(k_src) @ np.stack([x_src * samp, y_src * samp, samp])
        in_ref = ((e_ref @ np.linalg.inv(e_src)) @ np.vstack([back, one]))[:3]
        u = k_ref @ in_ref
        xr, yr = u[0] / u[2], u[1] / u[2]
    return tuple(a.reshape(h, w) for a in (in_ref[2], xr, yr, x_src, y_src, in_src[2]))


def fuse64(sc):
    """The whole operation in float64 -> NS(dist, rel, rep [n,h,w]; td, tr [9]; masks [n,9,h,w]; counts [9,h,w]; nvalid; geo_mask,
    photo_mask, final_mask, depth_avg [h,w])."""
    c = sc.case
    d0 = sc.depths[0].astype(np.float64)
    h, w = d0.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    td = np.array([i / float(c.thre1) for i in range(2, 11)])
    tr = np.array([i / float(c.thre2) for i in range(2, 11)])
    dist, rel, rep, masks = [], [], [], []
    with np.errstate(all="ignore"):
        for v in range(1, c.n_src + 1):
            r, xr, yr, _, _, _ = reproject64(sc.depths[0], sc.K[0], sc.E[0], sc.depths[v], sc.K[v], sc.E[v])
            dv = np.sqrt((xr - xs) ** 2 + (yr - ys) ** 2)
            rv = np.abs(r - d0) / d0
            mv = (dv[None] < td[:, None, None]) & (rv[None] < tr[:, None, None])
            dist.append(dv); rel.append(rv); masks.append(mv); rep.append(np.where(mv[-1], r, 0.0))
        masks = np.stack(masks)
        counts = masks.sum(0)
        nvalid = masks[:, -1].sum(0)
        geo = sum((counts[i - 2] >= i).astype(np.int64) for i in range(2, 11))
        depth_avg = (np.sum(rep, 0) + d0) / (nvalid + 1)
        photo = sc.conf.astype(np.float64) > float(np.float32(c.photo))
    geo_mask = geo >= c.nconditions
    return NS(dist=np.stack(dist), rel=np.stack(rel), rep=np.stack(rep), td=td, tr=tr, masks=masks, counts=counts, nvalid=nvalid,
              geo_mask=geo_mask, photo_mask=photo, final_mask=photo & geo_mask, depth_avg=depth_avg)


@functools.lru_cache(maxsize=None)
def ref64(name):
    return fuse64(scene(name))


# ==================================================================================================================== fp32 oracle runs
FORMS = {"explicit": True, "aten": False, "grid_sample": "grid_sample"}


def oracle32(name, form="explicit"):
    """The fp32 oracle (oracle/filter_oracle.py) on a case, in one of its three forms -> NS(view_masks [n,9,h,w] bool, rep [n,h,w], dist, rel [n,h,w] fp32 (the
    oracle's own two lines on its reprojection), cmp_dist, cmp_rel [n,9,h,w] bool (the single comparisons), geo_mask, photo_mask,
    final_mask, depth_avg): torch CPU tensors.  "aten" is the reference's own calls (grid_sample and torch.matmul, whose
    accumulation order is the host BLAS's); "grid_sample" keeps the explicit products and samples through F.grid_sample."""
    return _oracle32(name, FORMS[form])


@functools.lru_cache(maxsize=None)
def _oracle32(name, explicit):
    sc = scene(name)
    c = sc.case
    d0, conf, k0, e0, ds, ks, es = tensors(sc)
    h, w = d0.shape
    ys, xs = torch.meshgrid(torch.arange(0, h), torch.arange(0, w), indexing="ij")
    fn = FO.REPROJECT[explicit]
    vm, rep, dist, rel, cd, cr = [], [], [], [], [], []
    for d, k, e in zip(ds, ks, es):
        masks, _, r = FO.check_geometric_consistency(d0, k0, e0, d, k, e, c.thre1, c.thre2, explicit=explicit)
        vm.append(torch.stack(masks)[:, 0]); rep.append(r[0])
        dr, xr, yr, _, _ = fn(d0, k0, e0, d, k, e)
        dv = torch.sqrt((xr - xs.unsqueeze(0)) ** 2 + (yr - ys.unsqueeze(0)) ** 2)       # filter_oracle.py: check_geometric_consistency
        rv = torch.abs(dr - d0) / d0
        dist.append(dv[0]); rel.append(rv[0])
        cd.append(torch.stack([dv[0] < i / c.thre1 for i in range(2, 11)]))
        cr.append(torch.stack([rv[0] < i / c.thre2 for i in range(2, 11)]))
        assert torch.equal(vm[-1], cd[-1] & cr[-1])
    f = FO.fuse_view(d0, conf, k0, e0, ds, ks, es, photo_threshold=c.photo, nconditions=c.nconditions, thre1=c.thre1, thre2=c.thre2,
                     explicit=explicit)
    return NS(view_masks=torch.stack(vm), rep=torch.stack(rep), dist=torch.stack(dist), rel=torch.stack(rel), cmp_dist=torch.stack(cd),
              cmp_rel=torch.stack(cr), geo_mask=f["geo_mask"], photo_mask=f["photo_mask"], final_mask=f["final_mask"],
              depth_avg=f["depth_avg"])


def same_bits(a, b):
    """Bit-for-bit equality of two float32 / bool / integer tensors or arrays (NaN payloads and the sign of zero included)."""
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return bool(np.array_equal(a, b))


def same_values(a, b):
    """Equality of two float32 tensors with every NaN equal to every NaN: the same NaN set, the same values elsewhere (+0 == -0)."""
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def forms_agree(name, form="aten"):
    """`form` == the explicit form on this host, for every output of the case: the same NaN set and equal values elsewhere in the
    floats (a NaN's payload and sign come from whichever operand the host's instruction kept, so they are not compared), equal masks.
    -> list of the outputs that differ."""
    a, e = oracle32(name, form), oracle32(name)
    bad = [k for k in ("view_masks", "geo_mask", "photo_mask", "final_mask") if not torch.equal(getattr(a, k), getattr(e, k))]
    return bad + [k for k in ("rep", "depth_avg") if not same_values(getattr(a, k), getattr(e, k))]


def host_products_are_forward_chains(n):
    """Does torch.matmul of a [3,3] and a [4,4] matrix with n columns round like the explicit form's chain (acc = m0 x0, then
    fma(m_j, x_j, acc)) on this host?  It does on the goldens' build host for the n of the table; an AVX-512 BLAS walks the
    three-term products in another order, and the ATen form is then no checker of anything."""
    g = torch.Generator().manual_seed(n)
    for k in (3, 4):
        m, x = torch.randn(k, k, generator=g), torch.randn(k, n, generator=g) * 100
        if not torch.equal(torch.matmul(m, x.unsqueeze(0))[0], torch.stack(FO._mm(m, list(x)))):
            return False
    return True


# ==================================================================================================================== band tools
def in_band(r64, band=BAND):
    """[n,9,h,w] bool: the decisions check 3 leaves out (float64 dist or rel within `band`, relative, of its threshold)."""
    td, tr = r64.td[None, :, None, None], r64.tr[None, :, None, None]
    with np.errstate(invalid="ignore"):
        return (np.abs(r64.dist[:, None] - td) <= band * td) | (np.abs(r64.rel[:, None] - tr) <= band * tr)


def flip_distances(name):
    """The single comparisons of the fp32 explicit oracle that disagree with float64 -> (count, largest relative distance of the
    float64 value from its threshold among them; inf if a disagreement has no such distance, i.e. a NaN on the float64 side)."""
    o, r = oracle32(name), ref64(name)
    worst, count = 0.0, 0
    for c32, v64, t in ((o.cmp_dist.numpy(), r.dist, r.td), (o.cmp_rel.numpy(), r.rel, r.tr)):
        t = t[None, :, None, None]
        with np.errstate(invalid="ignore"):
            flip = c32 != (v64[:, None] < t)
            rd = np.abs(v64[:, None] - t) / t
        if flip.any():
            count += int(flip.sum())
            m = rd[flip]
            worst = max(worst, float("inf") if np.isnan(m).any() else float(m.max()))
    return count, worst


def distances(got, ref, ok):
    """The project's usual pair: max |d| / max |ref| and relative L2, over the pixels `ok`, in float64."""
    g, r = np.asarray(got, dtype=np.float64)[ok], np.asarray(ref, dtype=np.float64)[ok]
    if r.size == 0:
        return {"max": 0.0, "l2": 0.0}
    with np.errstate(over="ignore"):
        return {"max": float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-300)),
                "l2": float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300))}


def judged_pixels(name):
    """[h,w] bool: the pixels whose depth_avg check 3 judges -- float64 finite, no decision of the pixel inside the band, and the fp32
    explicit oracle finite (where it is not, check 1 already pins the kernel to the oracle's bits)."""
    r = ref64(name)
    return np.isfinite(r.depth_avg) & ~in_band(r).any(axis=(0, 1)) & np.isfinite(oracle32(name).depth_avg.numpy())
