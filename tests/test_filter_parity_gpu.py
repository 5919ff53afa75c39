"""GPU parity of the fused consistency filter (csrc/consistency.hip, mdf_consistency_fuse_fwd) over the case table of
tests/filter_mirror.py: edge shapes (smaller than a block, one lane short of a block, exactly a block, ragged last blocks), 1 to 16 source
views, projections outside the map and behind the camera, non-finite / zero / negative / denormal / huge depths, confidences on the
photometric threshold, nconditions 0..10 and thresholds fp32 cannot hold.

Every case is launched ONCE through the ABI into buffers with a guard row on each side, prefilled with a NaN of a payload no
arithmetic produces (floats) and 0xFF (bytes); the four checks share that run.
  check 1  bit for bit against the explicit oracle run on this host: depth_avg and every view's depth_reprojected (the same NaN set,
           the same bits elsewhere), the three masks and every view's nine masks; every pixel written, the guards untouched.
  check 2  the same against grid_sample itself on the cases the table marks `aten`: the grid_sample form of the oracle (its explicit
           products around F.grid_sample) on any host, the ATen form (torch.matmul too) on hosts whose BLAS rounds the products like
           the explicit form (tests/test_filter_mirror_cpu.py holds both against the explicit form, case by case).
  check 3  against float64: every (pixel, view, threshold) decision outside the band equals the float64 decision; depth_avg at most
           1.5 x as far from float64 as the explicit oracle's (max |d| / max |ref| and relative L2) over the pixels that are finite in
           float64 and have no decision inside the band.
           BAND = 1e-4, relative: the fp32 explicit oracle and float64 disagree in 18 single comparisons (dist < td, rel < tr) over the
           47 cases, the farthest 4.72e-5 from its threshold (kdist_17x259_n2), doubled and rounded up.  It leaves out at most 9.8e-4
           of a case's decisions (unit_3x1025_n1: its 27 planted decisions, by construction on the thresholds), 4.5e-4 on the
           synthesised scenes (thre3_61x67_n10), under the cap of 1e-3.  Measured by test_band_is_twice_the_measured_flip_distance on
           the CPU from the oracle and float64 alone.  Ratios printed per case; observed on an MI355X: 1.00 (max and L2) on all 47
           cases, the kernel's depth_avg being the oracle's bit for bit.
  check 4  per_view=False, non-contiguous and fp64 inputs, the driver's check_geometric_consistency with its own thresholds, and the
           refusal of 0 and 17 source views.
"""
import ctypes

import numpy as np
import pytest
import torch

import filter_mirror as FM
import mdfnet_hip
from mdfnet_hip import ops
from oracle import filter_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x7FE5A5A5                     # a quiet NaN whose payload neither the inputs nor the hardware's default NaN carry
_runs = {}


def _filled(n, dtype):
    if dtype == torch.float32:
        return torch.full((n,), FILL, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((n,), -1, dtype=dtype, device=DEV).view(torch.uint8 if dtype == torch.int8 else dtype)


def _launch(sc, n_src=None, per_view=True, thre=None):
    """One call of mdf_consistency_fuse_fwd on a scene -> (rc, NS of the guarded buffers, already on the host).  Every output buffer
    is [guard row | payload | guard row]; the kernel gets the payload's address."""
    c = sc.case
    d0, conf, k0, e0, ds, ks, es = FM.tensors(sc)
    h, w = d0.shape
    n = len(ds) if n_src is None else n_src
    hw = h * w
    keep = [d0.to(DEV), conf.to(DEV)] + [d.to(DEV) for d in ds]
    srcs = [keep[2 + (v % len(ds))] for v in range(max(n, 1))]            # n_src = 17: seventeen valid pointers, in case they are read
    mats = ops.consistency_mats(k0, e0, [ks[v % len(ks)] for v in range(max(n, 1))], [es[v % len(es)] for v in range(max(n, 1))]).to(DEV)
    nv = max(n, 1)
    thre1, thre2 = thre or (c.thre1, c.thre2)
    avg, masks = _filled(hw + 2 * w, torch.float32), _filled(3 * hw + 2 * w, torch.int8)
    vm, rep = _filled(nv * hw + 2 * w, torch.int16), _filled(nv * hw + 2 * w, torch.float32)
    rc = mdfnet_hip.lib().mdf_consistency_fuse_fwd(
        keep[0].data_ptr(), keep[1].data_ptr(), ops._src_array(srcs), mats.data_ptr(), n, h, w, ctypes.c_float(c.photo), int(c.nconditions),
        ctypes.c_double(thre1), ctypes.c_double(thre2), avg.data_ptr() + 4 * w, masks.data_ptr() + w,
        vm.data_ptr() + 2 * w if per_view else None, rep.data_ptr() + 4 * w if per_view else None, ops._stream(avg))
    torch.cuda.synchronize()
    return rc, FM.NS(avg=avg.cpu(), masks=masks.cpu(), vm=vm.cpu(), rep=rep.cpu(), h=h, w=w, n=nv)


def _untouched(t):
    return bool((t.view(torch.int32) == FILL).all()) if t.dtype == torch.float32 else bool((t.view(torch.uint8) == 0xFF).all())


def _unpack(b):
    """The guarded buffers -> NS(depth_avg [h,w], masks [3,h,w] uint8, vm [n,h,w] int32 (the 16 bits), rep [n,h,w]) + guards intact."""
    h, w, n, hw = b.h, b.w, b.n, b.h * b.w
    guards = all(_untouched(t[:w]) and _untouched(t[-w:]) for t in (b.avg, b.masks, b.vm, b.rep))
    return FM.NS(depth_avg=b.avg[w:-w].reshape(h, w), masks=b.masks[w:-w].reshape(3, h, w),
                 vm=(b.vm[w:-w].to(torch.int32) & 0xFFFF).reshape(n, h, w), rep=b.rep[w:-w].reshape(n, h, w), guards=guards)


def run(name):
    if name not in _runs:
        rc, b = _launch(FM.scene(name))
        assert rc == 0, mdfnet_hip.lib().mdf_last_error().decode()
        _runs[name] = _unpack(b)
    return _runs[name]


def _same_float(got, ref):
    """The same NaN set and the same bits elsewhere (a NaN's sign and payload are the producing hardware's, not the operation's)."""
    got, ref = got.numpy(), ref.numpy()
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan)) and bool(np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))


def _pack(view_masks):
    """[n,9,h,w] bool -> [n,h,w] int32, bit i <-> threshold index i: what the kernel writes, the upper seven bits zero."""
    return sum(view_masks[:, i].to(torch.int32) << i for i in range(9))


def _against(name, o):
    g = run(name)
    assert g.guards, "a guard row was written"
    for k, t in (("depth_avg", g.depth_avg), ("rep", g.rep)):
        assert not bool((t.view(torch.int32) == FILL).any()), f"{k}: pixels left unwritten"
    assert _same_float(g.depth_avg, o.depth_avg), "depth_avg"
    for i, k in enumerate(("photo_mask", "geo_mask", "final_mask")):
        assert torch.equal(g.masks[i], getattr(o, k).to(torch.uint8)), k
    bad = (g.vm != _pack(o.view_masks)).flatten(1).sum(1)
    assert int(bad.sum()) == 0, f"per-view masks differ in views {bad.nonzero().flatten().tolist()}"
    for v in range(g.rep.shape[0]):
        assert _same_float(g.rep[v], o.rep[v]), f"depth_reprojected of view {v + 1}"


@pytest.mark.parametrize("name", FM.NAMES)
def test_bit_exact_vs_explicit_oracle(name):
    _against(name, FM.oracle32(name))


@pytest.mark.parametrize("name", [c.name for c in FM.CASES if c.aten])
def test_bit_exact_vs_aten_form(name):
    """Against grid_sample itself: the grid_sample form (the explicit products around F.grid_sample) on any host, and the ATen form
    (torch.matmul too) where this host's BLAS rounds the 3- and 4-term products like the explicit form -- elsewhere that form
    differs from the reference's own goldens and checks nothing."""
    c = FM.BY_NAME[name]
    _against(name, FM.oracle32(name, "grid_sample"))
    if FM.host_products_are_forward_chains(c.h * c.w):
        _against(name, FM.oracle32(name, "aten"))


@pytest.mark.parametrize("name", FM.NAMES)
def test_decisions_and_depth_vs_float64(name):
    """Check 3 of the module docstring (the band, its measurement and the shares it leaves out are written there)."""
    g, r, o = run(name), FM.ref64(name), FM.oracle32(name)
    ib = FM.in_band(r)
    assert ib.mean() <= FM.BAND_CAP
    got = np.stack([((g.vm.numpy() >> i) & 1).astype(bool) for i in range(9)], axis=1)
    wrong = (got != r.masks) & ~ib
    assert not wrong.any(), f"{int(wrong.sum())} decisions outside the band differ from float64"
    ok = FM.judged_pixels(name)
    region = np.isfinite(r.depth_avg) & ~ib.any(axis=(0, 1))              # `ok` = the region less the pixels the fp32 oracle overflows at
    assert np.array_equal(np.isfinite(g.depth_avg.numpy())[region], ok[region]), "finite where the oracle is not, or the reverse"
    e_hip, e_32 = FM.distances(g.depth_avg.numpy(), r.depth_avg, ok), FM.distances(o.depth_avg.numpy(), r.depth_avg, ok)
    ratio = {k: (e_hip[k] / e_32[k] if e_32[k] > 0 else (1.0 if e_hip[k] == 0 else float("inf"))) for k in e_hip}
    print(f"\n{name}: band leaves out {ib.mean():.2e} of {ib.size} decisions; depth_avg over {int(ok.sum())} of {ok.size} pixels: "
          f"max {e_hip['max']:.3e} (oracle {e_32['max']:.3e}, ratio {ratio['max']:.2f}), l2 {e_hip['l2']:.3e} (oracle {e_32['l2']:.3e}, "
          f"ratio {ratio['l2']:.2f})")
    for k in e_hip:
        assert e_hip[k] <= 1.5 * e_32[k], (k, e_hip[k], e_32[k])


def _gpu_args(sc):
    d0, conf, k0, e0, ds, ks, es = FM.tensors(sc)
    return [d0.to(DEV), conf.to(DEV), k0, e0, [d.to(DEV) for d in ds], ks, es]


def _kw(c):
    return dict(photo_threshold=c.photo, nconditions=c.nconditions, thre1=c.thre1, thre2=c.thre2)


def _same_result(r, g, per_view):
    assert _same_float(r["depth_avg"].cpu(), g.depth_avg), f"depth_avg differs at {int((r['depth_avg'].cpu() != g.depth_avg).sum())} pixels (NaNs counted)"
    for i, k in enumerate(("photo_mask", "geo_mask", "final_mask")):
        assert torch.equal(r[k].cpu().to(torch.uint8), g.masks[i]), k
    assert ("view_masks" in r) == per_view and ("rep" in r) == per_view
    if per_view:
        assert torch.equal(_pack(r["view_masks"].cpu()), g.vm) and _same_float(r["rep"].cpu(), g.rep)


@pytest.mark.parametrize("name", FM.NAMES)
def test_per_view_outputs_are_optional(name):
    """ops.consistency_fuse with and without the per-view outputs: depth_avg and the masks of both equal the guarded run's."""
    sc = FM.scene(name)
    for per_view in (False, True):
        _same_result(ops.consistency_fuse(*_gpu_args(sc), per_view=per_view, **_kw(sc.case)), run(name), per_view)


@pytest.mark.parametrize("name", ["plants_13x21_n3", "shift_plants_photo0_17x259_n2", "thre1_31x33_n16"])
def test_strided_and_fp64_inputs(name):
    sc = FM.scene(name)
    d0, conf, k0, e0, ds, ks, es = _gpu_args(sc)
    h, w = d0.shape
    wide = torch.zeros(h, 2 * w + 1, device=DEV)
    wide[:, 1::2] = d0
    pile = torch.stack(ds, dim=-1)                                         # [h,w,n]: every source map a strided slice
    strided = [wide[:, 1::2], conf.t().contiguous().t(), k0.t().contiguous().t(), e0, [pile[..., v] for v in range(len(ds))], ks, es]
    assert not strided[0].is_contiguous() and not strided[1].is_contiguous() and not strided[4][0].is_contiguous()
    _same_result(ops.consistency_fuse(*strided, per_view=True, **_kw(sc.case)), run(name), True)
    fp64 = [d0.double(), conf.double(), k0.double(), e0.double(), [d.double() for d in ds], [k.double() for k in ks], [e.double() for e in es]]
    _same_result(ops.consistency_fuse(*fp64, per_view=True, **_kw(sc.case)), run(name), True)


@pytest.mark.parametrize("name", ["plants_13x21_n3", "shift_border_17x259_n2", "unit_3x1025_n1", "shape_2x2_n1"])
def test_driver_check_geometric_consistency_with_its_own_thresholds(name):
    """The driver's n_src = 1 entry with thresholds fp32 cannot hold, against the oracle's."""
    from tools.filter import dynamic_filter_gpu as filt
    sc = FM.scene(name)
    d0, _, k0, e0, ds, ks, es = FM.tensors(sc)
    for t1, t2 in ((3.3, 1234.56), (2.9, 6.1)):
        masks, last, rep = filt.check_geometric_consistency(d0.to(DEV), k0, e0, ds[0].to(DEV), ks[0], es[0], thre1=t1, thre2=t2)
        om, olast, orep = FO.check_geometric_consistency(d0, k0, e0, ds[0], ks[0], es[0], t1, t2, explicit=True)
        assert len(masks) == 9 and all(torch.equal(m.cpu(), x) for m, x in zip(masks, om)) and torch.equal(last.cpu(), olast)
        assert rep.shape == orep.shape and _same_float(rep.cpu(), orep)


@pytest.mark.parametrize("n_src", [0, FM.MAX_SRC_VIEWS + 1])
def test_view_counts_out_of_range_are_refused(n_src):
    rc, b = _launch(FM.scene("shape_13x21_n3"), n_src=n_src)
    assert rc != 0
    assert f"n_src={n_src} out of range [1,{FM.MAX_SRC_VIEWS}]" in mdfnet_hip.lib().mdf_last_error().decode()
    assert all(_untouched(t) for t in (b.avg, b.masks, b.vm, b.rep)), "a refused call wrote an output"
    if n_src:
        sc = FM.scene("shape_13x21_n3")
        d0, conf, k0, e0, ds, ks, es = _gpu_args(sc)
        with pytest.raises(mdfnet_hip.MdfHipError, match=f"n_src={n_src} out of range"):
            ops.consistency_fuse(d0, conf, k0, e0, (ds * n_src)[:n_src], (ks * n_src)[:n_src], (es * n_src)[:n_src])


def test_thresholds_are_taken_as_doubles():
    """The `unit` case, whose rel values ARE the thresholds and their fp32 neighbours: with thre2 = 6.1 the masks are the oracle's at
    6.1 (check 1), and with the double (float)6.1 -- the value an ABI with float thresholds would receive -- they are the oracle's
    at THAT value, and differ from the former."""
    name = "unit_3x1025_n1"
    sc = FM.scene(name)
    c = sc.case
    t1, t2 = float(np.float32(c.thre1)), float(np.float32(c.thre2))
    assert (t1, t2) != (c.thre1, c.thre2)
    rc, b = _launch(sc, thre=(t1, t2))
    assert rc == 0
    g = _unpack(b)
    d0, _, k0, e0, ds, ks, es = FM.tensors(sc)
    om, _, orep = FO.check_geometric_consistency(d0, k0, e0, ds[0], ks[0], es[0], t1, t2, explicit=True)
    assert g.guards and torch.equal(g.vm, _pack(torch.stack(om)[:, 0].unsqueeze(0))) and _same_float(g.rep[0], orep[0])
    assert int((g.vm != run(name).vm).sum()) > 0


def test_threshold_arguments_are_checked():
    sc = FM.scene("shape_13x21_n3")
    for t1, t2 in ((0.0, 1300.0), (4.0, -1.0), (float("nan"), 1300.0)):
        with pytest.raises(mdfnet_hip.MdfHipError, match="bad shape / thresholds"):
            ops.consistency_fuse(*_gpu_args(sc), thre1=t1, thre2=t2)
