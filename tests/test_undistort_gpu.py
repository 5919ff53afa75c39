"""GPU: mdf_image_undistort / ops.undistort_images against tests/undistort_oracle.py, and the importer with --undistort end to end.

Bars.  Identity (no coefficients, z = s = 1): dst is the source's top-left block byte for byte; no oracle is involved.  Rational
kind (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV): dst and valid are the oracle's bytes -- both sides execute the same correctly
rounded fp64 operations in the order the oracle's docstring fixes.  Fisheye kind: the device's atan may differ from the host's in the
last bits, which moves a coordinate by ~1e-13 pixels and a value by at most 255 times that; every byte q must satisfy
|q - v| <= 0.5 + 1e-6 with v the oracle's unrounded value (1e-6 is an envelope, not a measurement), and valid must agree wherever
the oracle's U, V are farther than 1e-9 from the four blank thresholds (the inputs are chosen so that this excludes no pixel; at most
1 % may be).  The number of fisheye bytes that differ from the oracle's rounding is printed (DESIGN section 7 quotes it)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import undistort_oracle as U  # noqa: E402
import view_select_oracle as O  # noqa: E402
import test_undistort_cpu as C  # noqa: E402  (the model writer, the ramp cases and the fit cases: checked there on the CPU)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (source (w, h), output (w, h), s, n, images, principal point, focal scale)
SHAPES = {"s1": ((96, 64), (96, 64), 1.0, 1, 1), "s05": ((200, 136), (96, 64), 0.5, 2, 1), "s04": ((250, 170), (96, 64), 0.4, 3, 1),
          "batch3": ((35, 33), (32, 32), 1.0, 1, 3)}
# distortion coefficients per model, every one non-zero; FULL_OPENCV's denominator stays inside [0.5, 2] (asserted below)
DIST = {"SIMPLE_RADIAL": [-0.11], "RADIAL": [-0.11, 0.03], "OPENCV": [-0.11, 0.03, 0.002, -0.001],
        "FULL_OPENCV": [-0.11, 0.03, 0.002, -0.001, 0.004, 0.05, -0.02, 0.006], "OPENCV_FISHEYE": [0.05, -0.01, 0.003, -0.001]}
RATIONAL = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")


def camera(model, shape, zoom=None):
    """(model, params) of a camera whose frame spans about +-0.4 x +-0.27 normalised units, principal point off the centre."""
    (w, h), _, _, _, _ = SHAPES[shape]
    f = 1.25 * w
    centre = [w / 2 + 1.5, h / 2 - 2.25]
    focal = [f] if model in ("SIMPLE_RADIAL", "RADIAL") else [f, 0.98 * f]
    return model, focal + centre + DIST[model]


# (model, shape, image, zoom): every model at every shape on both images at z = 1, and one z = 0.6 case per kind (blank bands and
# edge-clamped taps on every side)
CASES = [(m, s, img, 1.0) for m in DIST for s in SHAPES for img in ("smooth", "noise")] + \
        [("OPENCV", "s05", "noise", 0.6), ("OPENCV_FISHEYE", "s05", "noise", 0.6)]


def source(shape, image):
    (w, h), _, _, _, b = SHAPES[shape]
    make = U.smooth_image if image == "smooth" else U.noise_image
    return np.stack([make(h, w, seed=11 + k) for k in range(b)])


@functools.lru_cache(maxsize=None)
def oracle(model, shape, image, zoom):
    _, (ow, oh), s, n, _ = SHAPES[shape]
    kind, c, fx, fy, cx, cy = U.model_coeffs(*camera(model, shape))
    res = U.undistort(source(shape, image), kind, c, fx, fy, cx, cy, (oh, ow), zoom, s, n)
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def kernel(model, shape, image, zoom):
    from mdfnet_hip import ops
    _, (ow, oh), s, n, _ = SHAPES[shape]
    kind, c, fx, fy, cx, cy = U.model_coeffs(*camera(model, shape))
    dst, valid = ops.undistort_images(torch.from_numpy(source(shape, image)).to(DEV), kind, c, fx, fy, cx, cy, (oh, ow), zoom=zoom, scale=s,
                                      nsub=n, want_valid=True)
    return dst.cpu().numpy(), valid.cpu().numpy()


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-z{c[3]}"


# ---------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("sw,sh,ow,oh", [(35, 33, 32, 32), (96, 64, 96, 64)])
def test_identity_copies_the_top_left_block(sw, sh, ow, oh):
    from mdfnet_hip import ops
    src = np.stack([U.noise_image(sh, sw, seed=k) for k in range(2)])
    dst, valid = ops.undistort_images(torch.from_numpy(src).to(DEV), "rational", np.zeros(12), 1.25 * sw, 1.2 * sw, sw / 2 + 1.5, sh / 2 - 2.25,
                                      (oh, ow), want_valid=True)
    assert dst.dtype == torch.uint8 and tuple(dst.shape) == (2, oh, ow, 3) and tuple(valid.shape) == (2, oh, ow)
    assert np.array_equal(dst.cpu().numpy(), src[:, :oh, :ow]) and valid.cpu().numpy().all()
    only = ops.undistort_images(torch.from_numpy(src).to(DEV), "fisheye", [], 1.25 * sw, 1.2 * sw, sw / 2 + 1.5, sh / 2 - 2.25, (oh, ow))
    assert torch.is_tensor(only) and tuple(only.shape) == (2, oh, ow, 3)              # without want_valid: the image alone


# ---------------------------------------------------------------------------------------------------- parity
def test_inputs_hold_the_conditions_the_bars_assume():
    """On the CPU side: FULL_OPENCV's denominator, the blank bands of the z = 0.6 cases, and the fisheye exclusion rule."""
    for shape in SHAPES:
        (w, h), (ow, oh), s, n, _ = SHAPES[shape]
        kind, c, fx, fy, cx, cy = U.model_coeffs(*camera("FULL_OPENCV", shape))
        for z in (1.0, 0.6):
            x = (np.array([0.0, ow / s]) - cx) / (z * fx)
            y = (np.array([0.0, oh / s]) - cy) / (z * fy)
            r2 = np.linspace(0, float(np.max(x ** 2) + np.max(y ** 2)), 200)
            den = 1 + c[5] * r2 + c[6] * r2 ** 2 + c[7] * r2 ** 3
            assert 0.5 <= den.min() and den.max() <= 2.0
    for case in CASES:
        res = oracle(*case)
        (w, h) = SHAPES[case[1]][0]
        blank_px = res["valid"][0] == 0
        if case[3] == 0.6:
            for band in (blank_px[0], blank_px[-1], blank_px[:, 0], blank_px[:, -1]):      # blanks on every side ...
                assert band.all()
            U_, V_ = res["U"], res["V"]
            ok = ~res["blank"]
            assert (ok & (U_ < 0)).any() and (ok & (U_ > w - 1)).any() and (ok & (V_ < 0)).any() and (ok & (V_ > h - 1)).any()   # ... and clamped taps
            assert 0.2 < res["valid"].mean() < 0.8
        if case[0] == "OPENCV_FISHEYE":
            near = (U.threshold_distance(res["U"], res["V"], w, h) <= 1e-9).any(axis=(0, 1))
            assert near.mean() <= 0.01 and not near.any()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in RATIONAL], ids=case_id)
def test_rational_kind_gives_the_oracles_bytes(case):
    dst, valid = kernel(*case)
    want = oracle(*case)
    diff = int((dst != want["bytes"]).sum())
    print(f"{case_id(case)}: {diff} of {dst.size} bytes differ from the oracle, {int((valid != want['valid']).sum())} valid flags")
    assert np.array_equal(valid, want["valid"])
    assert np.array_equal(dst, want["bytes"])


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "OPENCV_FISHEYE"], ids=case_id)
def test_fisheye_kind_within_half_a_level_of_the_oracle(case):
    dst, valid = kernel(*case)
    want = oracle(*case)
    w, h = SHAPES[case[1]][0]
    far = ~(U.threshold_distance(want["U"], want["V"], w, h) <= 1e-9).any(axis=(0, 1))
    assert far.mean() >= 0.99
    diff = int((dst != want["bytes"]).sum())
    dist = float(np.max(np.abs(dst.astype(np.float64) - want["mean"])))
    print(f"{case_id(case)}: {diff} of {dst.size} bytes differ from the oracle's rounding, max |q - v| = {dist!r}")
    assert np.array_equal(valid[:, far], want["valid"][:, far])
    assert dist <= 0.5 + 1e-6


# ---------------------------------------------------------------------------------------------------- coordinate image
@functools.lru_cache(maxsize=None)
def ramp(name):
    return C.ramp_expectation(name)


@pytest.mark.parametrize("name", sorted(C.RAMP_CASES))
def test_ramp_image_reads_back_the_coordinates(name):
    from mdfnet_hip import ops
    model, params, (w, h), (ow, oh), zoom, scale, n = C.RAMP_CASES[name]
    kind, c, fx, fy, cx, cy = U.model_coeffs(model, params)
    _, mu, mv, inner = ramp(name)
    dst = ops.undistort_images(torch.from_numpy(U.ramp_image(h, w)[None]).to(DEV), kind, c, fx, fy, cx, cy, (oh, ow), zoom=zoom, scale=scale,
                               nsub=n).cpu().numpy()[0].astype(np.float64)
    du, dv = np.max(np.abs(dst[:, :, 0][inner] - mu[inner])), np.max(np.abs(dst[:, :, 1][inner] - mv[inner]))
    print(f"{name}: max |R - mean U| = {du!r}, max |G - mean V| = {dv!r} over {int(inner.sum())} pixels")
    assert du <= 0.5 + 1e-6 and dv <= 0.5 + 1e-6
    assert not dst[:, :, 2].any()


# ---------------------------------------------------------------------------------------------------- fit
@pytest.mark.parametrize("name", sorted(C.FIT_CASES))
def test_fitted_zoom_leaves_no_blank_and_a_smaller_one_does(name):
    from mdfnet_hip import ops
    p, (kind, c, fx, fy, cx, cy) = C.fit_case(name)
    src = torch.from_numpy(U.noise_image(64, 96, 1)[None]).to(DEV)
    at = ops.undistort_images(src, kind, c, fx, fy, cx, cy, (64, 96), zoom=p["z"], want_valid=True)[1].cpu().numpy()
    below = ops.undistort_images(src, kind, c, fx, fy, cx, cy, (64, 96), zoom=p["z"] * (1 - 2.0 ** -8), want_valid=True)[1].cpu().numpy()
    assert at.all() and not below.all()


# ---------------------------------------------------------------------------------------------------- ops checks
def test_ops_checks_raise_value_errors():
    from mdfnet_hip import ops
    good = torch.zeros((1, 64, 96, 3), dtype=torch.uint8, device=DEV)
    args = ("rational", [0.1], 100.0, 100.0, 48.0, 32.0, (64, 96))
    assert tuple(ops.undistort_images(good, *args).shape) == (1, 64, 96, 3)
    for bad in (good.cpu(), good.float(), torch.zeros((1, 64, 3, 96), dtype=torch.uint8, device=DEV).permute(0, 1, 3, 2),
                torch.zeros((1, 64, 96, 4), dtype=torch.uint8, device=DEV), good[0]):
        with pytest.raises(ValueError):
            ops.undistort_images(bad, *args)
    for kw in ({"nsub": 0}, {"nsub": 17}, {"zoom": 0.0}, {"scale": float("nan")}):
        with pytest.raises(ValueError):
            ops.undistort_images(good, *args, **kw)
    with pytest.raises(ValueError):
        ops.undistort_images(good, "fov", *args[1:])
    with pytest.raises(ValueError):
        ops.undistort_images(good, "rational", [0.0] * 13, *args[2:])


# ---------------------------------------------------------------------------------------------------- importer end to end
W_, H_ = 200, 136
E2E_CAMERAS = {1: ("SIMPLE_RADIAL", W_, H_, [150.0, W_ / 2 + 1.5, H_ / 2 - 2.25, 0.08]),
               2: ("OPENCV_FISHEYE", W_, H_, [150.0, 148.0, W_ / 2 + 1.5, H_ / 2 - 2.25, 0.05, -0.01, 0.003, -0.001]),
               3: ("PINHOLE", W_, H_, [150.0, 148.0, W_ / 2, H_ / 2])}
E2E_CAMERA_OF_IMAGE = [1, 2, 1, 3, 1]


def _read_K(path):
    rows = open(path).read().split("\n")
    return np.array([[float(v) for v in rows[k].split()] for k in (7, 8, 9)])


def test_import_with_undistort(tmp_path):
    from PIL import Image
    from mdfnet_hip import ops
    from tools.colmap import main as importer, undistort as UD
    n = len(E2E_CAMERA_OF_IMAGE)
    image_dir = tmp_path / "photos"
    image_dir.mkdir()
    names = [f"photo_{i}.jpg" for i in range(n)]
    for k, name in enumerate(names):
        Image.fromarray(U.smooth_image(H_, W_, seed=20 + k)).save(image_dir / name, quality=95)
    dirs = {}
    for tag, cams in (("distorted", E2E_CAMERAS), ("pinhole", {cid: ("PINHOLE", W_, H_, [150.0, 148.0, W_ / 2, H_ / 2]) for cid in E2E_CAMERAS})):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        C.write_model(dirs[tag], cams, binary=(tag == "distorted"), n_img=E2E_CAMERA_OF_IMAGE, names=names, seed=41)
    with pytest.raises(SystemExit, match="or pass --undistort"):
        importer.import_scene(str(dirs["distorted"]), str(image_dir), str(tmp_path / "refused"), nsrc=3, max_dim=100, log=lambda *a: None)
    lines = []
    out = tmp_path / "root" / "toy"
    ops.count_begin()
    res = importer.import_scene(str(dirs["distorted"]), str(image_dir), str(out), nsrc=3, max_dim=100, log=lines.append, undistort=True)
    counts = ops.count_end()
    assert counts["mdf_image_undistort"] == 2                          # the three SIMPLE_RADIAL images share one launch
    ref = importer.import_scene(str(dirs["pinhole"]), str(image_dir), str(tmp_path / "root" / "ref"), nsrc=3, max_dim=100, log=lambda *a: None)
    assert len([ln for ln in lines if "zoom" in ln]) == 2 and any("camera 1 (SIMPLE_RADIAL): 3 images" in ln for ln in lines)
    plans = {cid: UD.plan(E2E_CAMERAS[cid], 100, "inside") for cid in (1, 2)}
    for i, cid in enumerate(E2E_CAMERA_OF_IMAGE):
        with Image.open(out / "images" / ("%08d.jpg" % i)) as im:
            assert im.size == (96, 64) and im.format == "JPEG"
        K = _read_K(out / "cams" / ("%08d_cam.txt" % i))
        if cid == 3:
            assert np.array_equal(K, _read_K(tmp_path / "root" / "ref" / "cams" / ("%08d_cam.txt" % i)))
            assert np.array_equal(K, [[75.0, 0, 50.0], [0, 74.0, 34.0], [0, 0, 1]])
            assert open(out / "images" / ("%08d.jpg" % i), "rb").read() == open(tmp_path / "root" / "ref" / "images" / ("%08d.jpg" % i), "rb").read()
        else:
            assert np.array_equal(K, plans[cid]["K_out"]) and plans[cid]["z"] != 1.0
    assert open(out / "pair.txt").read() == open(tmp_path / "root" / "ref" / "pair.txt").read()
    assert np.array_equal(res["range"], ref["range"]) and np.array_equal(res["sources"], ref["sources"])
    for i in range(n):
        assert open(out / "cams" / ("%08d_cam.txt" % i)).read().split("\n")[11] == open(tmp_path / "root" / "ref" / "cams" / ("%08d_cam.txt" % i)).read().split("\n")[11]
    # one distorted image: the written JPEG decodes to what the kernel's output decodes to after the same encoding
    p = plans[1]
    with Image.open(image_dir / names[2]) as im:
        src = np.asarray(im.convert("RGB"), dtype=np.uint8)
    own = ops.undistort_images(torch.from_numpy(src[None].copy()).to(DEV), p["kind"], p["coeffs"], p["fx"], p["fy"], p["cx"], p["cy"], (64, 96),
                               zoom=p["z"], scale=p["s"], nsub=p["n"]).cpu().numpy()[0]
    Image.fromarray(own).save(tmp_path / "own.jpg", format="JPEG", quality=95)
    with Image.open(tmp_path / "own.jpg") as a, Image.open(out / "images" / "00000002.jpg") as b:
        round_trip, written = np.asarray(a.convert("RGB")), np.asarray(b.convert("RGB"))
    print(f"JPEG codec error on the kernel's output: max |decode(encode(x)) - x| = {int(np.abs(round_trip.astype(int) - own.astype(int)).max())}")
    assert np.array_equal(written, round_trip)
    # --undistort_fit same keeps the focal length and reports what stays black
    lines = []
    importer.import_scene(str(dirs["distorted"]), str(image_dir), str(tmp_path / "root" / "same"), nsrc=3, max_dim=100, log=lines.append,
                          undistort=True, undistort_fit="same")
    assert np.array_equal(_read_K(tmp_path / "root" / "same" / "cams" / "00000000_cam.txt"), [[75.0, 0, 101.5 * 0.5], [0, 75.0, 65.75 * 0.5], [0, 0, 1]])
    assert sum("% of the pixels not covered" in ln for ln in lines) == 2
