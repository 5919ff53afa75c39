"""CPU: the preconditions of tests/test_filter_parity_gpu.py -- the explicit oracle's zero-padded taps are selects (equal to the ATen
form at non-finite border pixels), the float64 reference of tests/filter_mirror.py is pinned to the reference's goldens, the case
table exercises what it names, and the band of check 3 is measured from the fp32 oracle and float64 alone."""
import numpy as np
import pytest
import torch

import filter_mirror as FM
from oracle import filter_oracle as FO

T = torch.from_numpy
EDGE = [n for n in FM.NAMES if "shift" in FM.BY_NAME[n].edits or "border" in FM.BY_NAME[n].plants]


def _pair(name, v=1):
    sc = FM.scene(name)
    return tuple(T(a.copy()) for a in (sc.depths[0], sc.K[0], sc.E[0], sc.depths[v], sc.K[v], sc.E[v]))


def _clamped_onto_nonfinite(name):
    """[h,w] bool: some tap of view 1 lies outside the map and its clamped index is a NaN / inf pixel (where a product-form tap
    gives NaN and grid_sample's zero padding gives 0)."""
    sc = FM.scene(name)
    h, w = sc.depths[0].shape
    _, _, _, xs, ys = FO.reproject_explicit(*_pair(name))
    x0, y0 = torch.floor(xs[0]), torch.floor(ys[0])
    bad = ~torch.isfinite(T(sc.depths[1].copy()))
    hit = torch.zeros(h, w, dtype=torch.bool)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xt, yt = x0 + dx, y0 + dy
        out = ~((xt >= 0) & (xt <= w - 1) & (yt >= 0) & (yt <= h - 1)) & torch.isfinite(xt) & torch.isfinite(yt)
        hit |= out & bad[torch.nan_to_num(yt).clamp(0, h - 1).long(), torch.nan_to_num(xt).clamp(0, w - 1).long()]
    return hit


def test_case_table_covers_what_it_names():
    cs = FM.CASES
    assert {(c.h, c.w, c.n_src) for c in cs} >= set(FM.SHAPES)
    assert all(c.h * c.w < 5000 and 1 <= c.n_src <= FM.MAX_SRC_VIEWS for c in cs)
    sizes = {c.h * c.w for c in cs}
    assert min(sizes) < FM.BLOCK and FM.BLOCK in sizes and FM.BLOCK - 1 in sizes and any(s > FM.BLOCK and s % FM.BLOCK for s in sizes)
    assert {c.n_src for c in cs} >= {1, 2, 3, 10, 16}
    for e in ("shift", "behind", "copy", "kdist"):
        assert {(c.h, c.w) for c in cs if e in c.edits} >= {(13, 21), (17, 259)}, e
    for p in FM.ALL_PLANTS:
        assert {(c.h, c.w) for c in cs if p in c.plants} >= {(13, 21), (17, 259)}, p
    assert {c.nconditions for c in cs} == {0, 1, 5, 9, 10}
    assert {(c.thre1, c.thre2) for c in cs} == set(FM.THRES)
    assert {c.photo for c in cs} == {0.0, 0.8}
    assert np.float32(1e-40) > 0 and np.float32(1e-40) < np.finfo(np.float32).tiny          # the denormal plant is one
    for c in cs:                                                                                # the plants are in the scene
        sc = FM.scene(c.name)
        if "conf" in c.plants:
            thr = np.float32(c.photo)
            vals = sc.conf[np.isnan(sc.conf) | (np.abs(sc.conf - thr) <= np.spacing(thr))]
            assert np.isnan(vals).sum() == 1 and (vals == thr).sum() == 1 and (vals > thr).sum() == 1 and (vals < thr).sum() == 1, c.name
        for k, v in (("ref", 0), ("src", 1)):
            if k in c.plants:
                d = sc.depths[v]
                assert np.isnan(d).any() and np.isposinf(d).any() and (d == 0).any() and (d < 0).any() and (d == np.float32(1e30)).any() \
                    and (d == np.float32(1e-40)).any(), c.name


@pytest.mark.parametrize("name", [n for n in FM.NAMES if FM.BY_NAME[n].edits])
def test_edits_do_what_they_name(name):
    c, sc = FM.BY_NAME[name], FM.scene(name)
    h, w = sc.depths[0].shape
    _, _, _, xs, ys, zs = FM.reproject64(sc.depths[0], sc.K[0], sc.E[0], sc.depths[1], sc.K[1], sc.E[1])
    ok = np.isfinite(xs) & np.isfinite(ys)
    outside = ((np.floor(xs) < 0) | (np.floor(xs) + 1 > w - 1) | (np.floor(ys) < 0) | (np.floor(ys) + 1 > h - 1)) & ok
    if "shift" in c.edits and "behind" not in c.edits:
        assert outside.sum() >= 0.2 * ok.sum(), (name, int(outside.sum()), int(ok.sum()))     # some tap of these is zero-padded
        assert (~outside & ok).sum() >= 0.1 * ok.sum()
    if "behind" in c.edits:
        front = np.isfinite(sc.depths[0]) & (sc.depths[0] > 1)           # every pixel but the planted ones
        assert (zs[front] < 0).all() and front.sum() >= 0.9 * zs.size
    if "copy" in c.edits:
        assert np.array_equal(sc.depths[-1], sc.depths[0]) and np.array_equal(sc.K[-1], sc.K[0]) and np.array_equal(sc.E[-1], sc.E[0])
        o = FM.oracle32(name)
        fin = np.isfinite(sc.depths[0])
        fin[[0, -1], :] = False; fin[:, [0, -1]] = False        # a border pixel samples a hair outside the map, as in the reference
        assert bool(o.view_masks[-1][:, T(fin)].all())
    if "kdist" in c.edits:
        assert len({sc.K[v].tobytes() for v in range(c.n_src + 1)}) == c.n_src + 1 - ("copy" in c.edits)    # the copy has view 0's K


def test_unit_scene_lands_on_the_thresholds():
    """The `unit` case: rel of the fp32 oracle IS the planted value (thresholds i >= 4), so its masks tell the reference's thresholds
    (float)(i / thre) from (float)(i / (float)thre): thresholds taken through a float thre flip decisions of this case."""
    name = "unit_3x1025_n1"
    c, o = FM.BY_NAME[name], FM.oracle32(name)
    assert float(o.dist.max()) < 1e-3          # x * samp / samp at the planted pixels: far below the smallest dist threshold
    flipped = 0
    for j, i in enumerate(range(2, 11)):
        t = np.float32(i / c.thre2)
        x = FM.UNIT_X0 + FM.UNIT_DX * j
        if t >= 0.5:
            got = o.rel[0, :, x].numpy()
            assert np.array_equal(got, [np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf))]), i
            assert o.cmp_rel[0, j, :, x].tolist() == [True, False, False], i
            t_float = np.float32(i / np.float64(np.float32(c.thre2)))
            flipped += int(((got < t_float) != (got < t)).sum())
    assert flipped > 0
    r = FM.ref64(name)
    assert r.masks.mean() > 0.99 and FM.in_band(r).sum() == 27


def _same_nan_set_and_bits(a, e):
    for x, y in zip(a, e):
        assert torch.equal(torch.isnan(x), torch.isnan(y))
        fin = ~torch.isnan(x)
        assert FM.same_bits(x[fin], y[fin])


@pytest.mark.parametrize("name", EDGE)
def test_explicit_taps_are_selects_like_grid_sample(name):
    """The fixed explicit form against grid_sample itself on the shifted and planted-border scenes: the same NaN set and bit-identical
    finite values in all five outputs -- against the grid_sample form on any host, and against the ATen form where the host's
    torch.matmul rounds like the explicit products.  On the shifted scenes with planted borders, pixels exist where an out-of-map tap
    is clamped onto a NaN / inf pixel while grid_sample's result is finite: where a product-form tap gave NaN."""
    c = FM.BY_NAME[name]
    e = FO.reproject_explicit(*_pair(name))
    a = FO.reproject_grid_sample(*_pair(name))
    _same_nan_set_and_bits(a, e)
    if FM.host_products_are_forward_chains(c.h * c.w):
        _same_nan_set_and_bits(FO.reproject_with_depth(*_pair(name)), e)
    if "border" in c.plants and "shift" in c.edits and "behind" not in c.edits:
        hit = _clamped_onto_nonfinite(name)
        assert int((hit & torch.isfinite(a[0][0])).sum()) > 0, name


@pytest.mark.parametrize("name", FM.NAMES)
def test_forms_that_qualify_as_checkers(name):
    """Check 2's references.  The grid_sample form equals the explicit form in every output of every case, on any host.  The ATen
    form's torch.matmul belongs to the host's BLAS: where it rounds like the explicit products (it does on the goldens' build host
    at every size of the table but 2 x 2), the `aten` column of the table says whether the form equals the explicit one."""
    c = FM.BY_NAME[name]
    assert FM.forms_agree(name, "grid_sample") == []
    if FM.host_products_are_forward_chains(c.h * c.w):
        bad = FM.forms_agree(name, "aten")
        assert (not bad) == c.aten, (name, bad)


def test_explicit_form_still_equals_the_reference_golden(golden):
    g = golden("filter.npz")
    d, K, E = g["depths"], g["K"], g["E"]
    n = d.shape[0]
    exp = FO.reproject_explicit(T(d[0]), T(K[0]), T(E[0]), T(d[1]), T(K[1]), T(E[1]))
    assert np.array_equal(torch.stack([o[0] for o in exp]).numpy(), g["reproj1"], equal_nan=True)
    for v in range(1, n):
        m, _, rep = FO.check_geometric_consistency(T(d[0]), T(K[0]), T(E[0]), T(d[v]), T(K[v]), T(E[v]), explicit=True)
        assert np.array_equal(torch.stack(m)[:, 0].numpy(), np.unpackbits(g[f"masks{v}"], axis=0)[:9].astype(bool))
        assert np.array_equal(rep[0].numpy(), g[f"rep{v}"])
    r = FO.fuse_view(T(d[0]), T(g["conf"]), T(K[0]), T(E[0]), [T(d[v]) for v in range(1, n)], [T(K[v]) for v in range(1, n)],
                     [T(E[v]) for v in range(1, n)], explicit=True)
    assert np.array_equal(r["depth_avg"].numpy(), g["depth_avg"])
    for k in ("geo_mask", "photo_mask", "final_mask"):
        assert np.array_equal(r[k].numpy(), g[k]), k


def test_float64_reference_is_pinned_to_the_reference_golden(golden):
    """The float64 reference on filter.npz: every (pixel, view, threshold) decision outside the band equals the golden mask the
    reference's own functions produced, the band leaves out at most the cap, and the fused outputs agree wherever no decision of the
    pixel is inside the band."""
    g = golden("filter.npz")
    d = g["depths"]
    n, h, w = d.shape
    case = FM.NS(n_src=n - 1, thre1=4, thre2=1300.0, photo=0.8, nconditions=5)
    r = FM.fuse64(FM.NS(depths=d, conf=g["conf"], K=g["K"], E=g["E"], case=case))
    gold = np.stack([np.unpackbits(g[f"masks{v}"], axis=0)[:9].astype(bool) for v in range(1, n)])
    ib = FM.in_band(r)
    assert ib.mean() <= FM.BAND_CAP
    assert not ((gold != r.masks) & ~ib).any()
    assert 0.05 < r.masks.mean() < 0.95                       # the decisions go both ways
    clear = ~ib.any(axis=(0, 1))
    assert clear.mean() > 0.99
    for k in ("geo_mask", "photo_mask", "final_mask"):
        assert np.array_equal(getattr(r, k)[clear], g[k][clear]), k
    assert np.array_equal(r.photo_mask, g["photo_mask"])
    e = FM.distances(g["depth_avg"], r.depth_avg, clear)
    assert e["max"] <= 64 * 2.0 ** -24 and e["l2"] <= 8 * 2.0 ** -24, e      # fp32 rounding of a ~40-operation chain, no cancellation


def test_band_is_twice_the_measured_flip_distance():
    """BAND of tests/filter_mirror.py from the fp32 explicit oracle and float64 alone (never the kernel): the largest relative distance
    from a threshold at which one of their single comparisons disagrees, doubled; and the cap -- the band leaves out at most 1e-3 of
    the decisions of any case.  Outside the band every decision of the oracle equals float64's."""
    worst, flips, share = 0.0, 0, {}
    for name in FM.NAMES:
        n, wd = FM.flip_distances(name)
        flips, worst = flips + n, max(worst, wd)
        ib = FM.in_band(FM.ref64(name))
        share[name] = float(ib.mean())
        assert not ((FM.oracle32(name).view_masks.numpy() != FM.ref64(name).masks) & ~ib).any(), name
    top = max(share, key=share.get)
    print(f"\nfp32 oracle vs float64 over {len(FM.NAMES)} cases: {flips} single comparisons flip, the farthest {worst:.3e} (relative) from "
          f"its threshold; BAND {FM.BAND:.1e} leaves out at most {share[top]:.2e} of a case's decisions ({top})")
    assert flips > 0 and 2.0 * worst <= FM.BAND <= 4.0 * worst, worst
    assert share[top] <= FM.BAND_CAP, (top, share[top])


def test_float64_reference_properties():
    """The float64 reference on its own: zero padding is a select (an out-of-map tap on a NaN border contributes 0), a view identical
    to the reference reprojects every interior pixel onto itself, NaN compares false in every mask."""
    src = np.full((4, 4), np.nan)
    src[1:3, 1:3] = 5.0
    got = FM._sample64(src, np.array([1.25, -1.5, 1.0, 3.5]), np.array([1.0, 1.0, -2.0, 1.0]))
    assert got[0] == 5.0 and got[1] == 0.0 and got[2] == 0.0 and np.isnan(got[3])
    src2 = np.full((3, 4), 2.0)
    assert np.array_equal(FM._sample64(src2, np.array([-0.25, 3.5, 1.0, np.nan]), np.array([0.0, 2.5, 2.25, 0.0]))[:3], [1.5, 0.5, 1.5])
    assert np.isnan(FM._sample64(src2, np.array([np.nan, np.inf]), np.array([0.0, 0.0]))).all()
    r = FM.ref64("copy_13x21_n3")
    assert r.dist[-1][1:-1, 1:-1].max() < 1e-9 and r.rel[-1][1:-1, 1:-1].max() < 1e-12
    r = FM.ref64("plants_13x21_n3")
    sc = FM.scene("plants_13x21_n3")
    assert not r.masks[:, :, np.isnan(sc.depths[0])].any() and np.isnan(r.depth_avg[np.isnan(sc.depths[0])]).all()
