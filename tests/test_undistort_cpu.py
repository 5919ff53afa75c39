"""CPU: the host side of scene import with --undistort -- the distorted COLMAP camera models (text and binary), the distortion
formulas of the float64 oracle against values worked by hand, the coordinate map on a ramp image, the zoom fit, the export plan,
the argument errors of mdf_image_undistort that need no GPU, and the command line."""
import ctypes
import math
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import colmap_writer as W  # noqa: E402
import undistort_oracle as U  # noqa: E402
import view_select_oracle as O  # noqa: E402

EXTRA_MODEL_IDS = {"OPENCV_FISHEYE": 5, "FULL_OPENCV": 6, "FOV": 7}          # COLMAP's ids of the models colmap_writer does not know

CAMERAS = {
    1: ("SIMPLE_RADIAL", 640, 480, [500.0, 321.5, 239.25, -0.11]),
    2: ("RADIAL", 640, 480, [500.0, 321.5, 239.25, -0.11, 0.03]),
    3: ("OPENCV", 640, 480, [500.0, 510.0, 321.5, 239.25, -0.11, 0.03, 0.002, -0.001]),
    4: ("FULL_OPENCV", 640, 480, [500.0, 510.0, 321.5, 239.25, -0.11, 0.03, 0.002, -0.001, 0.004, 0.05, -0.02, 0.006]),
    5: ("OPENCV_FISHEYE", 640, 480, [300.0, 305.0, 321.5, 239.25, 0.05, -0.01, 0.003, -0.001]),
    6: ("PINHOLE", 640, 480, [500.0, 510.0, 321.5, 239.25]),
    7: ("SIMPLE_PINHOLE", 640, 480, [500.0, 321.5, 239.25]),
}


def write_model(folder, cameras, binary, n_img=None, names=None, seed=17):
    """A sparse model with one image per camera (or camera_ids given through n_img = list of camera ids).  The camera files are
    written here, because colmap_writer's table lacks FULL_OPENCV and OPENCV_FISHEYE; images and points come from colmap_writer."""
    cam_of_image = list(cameras) if n_img is None else list(n_img)
    n = len(cam_of_image)
    rot, trans, pts, off, img = O.make_scene(n, 60, seed, arc_deg=30.0, window=5, drop=0.1)
    image_ids = list(range(1, n + 1))
    names = names or [f"im{i}.jpg" for i in image_ids]
    tracks = [[int(i) + 1 for i in img[off[p]:off[p + 1]]] for p in range(len(pts))]
    pinhole = {cid: ("PINHOLE", c[1], c[2], [1.0, 1.0, 0.0, 0.0]) for cid, c in cameras.items()}     # stand-ins: overwritten below
    (W.write_binary if binary else W.write_text)(str(folder), pinhole, image_ids, W.rotation_to_quaternion(rot), trans, cam_of_image,
                                                 names, list(range(1, len(pts) + 1)), pts, tracks)
    ids = dict(W.MODEL_IDS, **EXTRA_MODEL_IDS)
    if binary:
        with open(os.path.join(str(folder), "cameras.bin"), "wb") as out:
            out.write(struct.pack("<Q", len(cameras)))
            for cid, (model, w, h, params) in cameras.items():
                out.write(struct.pack("<iiQQ", cid, ids[model], w, h) + struct.pack("<%dd" % len(params), *params))
    else:
        with open(os.path.join(str(folder), "cameras.txt"), "w") as out:
            out.write("# Camera list with one line of data per camera:\n")
            for cid, (model, w, h, params) in cameras.items():
                out.write(f"{cid} {model} {w} {h} " + " ".join(repr(float(v)) for v in params) + "\n")
    return names


# ---------------------------------------------------------------------------------------------------- model parsing
@pytest.mark.parametrize("binary", [False, True])
def test_distorted_models_are_read_only_on_request(tmp_path, binary):
    from tools.colmap import model_io
    write_model(tmp_path, {1: CAMERAS[1]}, binary)
    with pytest.raises(SystemExit, match=r"SIMPLE_RADIAL.*image_undistorter.*or pass --undistort"):
        model_io.read_model(str(tmp_path))
    assert model_io.read_model(str(tmp_path), distorted=True)["camera_models"][1][0] == "SIMPLE_RADIAL"


@pytest.mark.parametrize("binary", [False, True])
def test_all_models_parse_with_their_intrinsics_and_distortion(tmp_path, binary):
    from tools.colmap import model_io
    write_model(tmp_path, CAMERAS, binary)
    m = model_io.read_model(str(tmp_path), distorted=True)
    want = {  # camera -> (fx, fy, kind, the first eight coefficients)
        1: (500.0, 500.0, "rational", [-0.11, 0, 0, 0, 0, 0, 0, 0]),
        2: (500.0, 500.0, "rational", [-0.11, 0.03, 0, 0, 0, 0, 0, 0]),
        3: (500.0, 510.0, "rational", [-0.11, 0.03, 0.002, -0.001, 0, 0, 0, 0]),
        4: (500.0, 510.0, "rational", [-0.11, 0.03, 0.002, -0.001, 0.004, 0.05, -0.02, 0.006]),
        5: (300.0, 305.0, "fisheye", [0.05, -0.01, 0.003, -0.001, 0, 0, 0, 0]),
        6: (500.0, 510.0, "rational", [0] * 8),
        7: (500.0, 500.0, "rational", [0] * 8),
    }
    for cid, (fx, fy, kind, coeffs) in want.items():
        cam = m["camera_models"][cid]
        assert cam[0] == CAMERAS[cid][0] and cam[1:3] == (640, 480) and np.array_equal(cam[3], CAMERAS[cid][3])
        assert np.array_equal(model_io.intrinsics(cam), [[fx, 0, 321.5], [0, fy, 239.25], [0, 0, 1]]), cid
        k, c = model_io.distortion(cam)
        assert k == kind and c.shape == (12,) and c.dtype == np.float64 and np.array_equal(c, coeffs + [0] * 4), cid
        ok, oc, ofx, ofy, ocx, ocy = U.model_coeffs(cam[0], cam[3])                     # the oracle reads the parameters alike
        assert (ok, ofx, ofy, ocx, ocy) == (kind, fx, fy, 321.5, 239.25) and np.array_equal(oc, c)
    s = model_io.scene_arrays(m, log=lambda *a: None)
    assert [c[0] for c in s["cameras"]] == [CAMERAS[i][0] for i in range(1, 8)] and s["camera_ids"].tolist() == list(range(1, 8))
    assert np.array_equal(s["K"][4], [[300, 0, 321.5], [0, 305, 239.25], [0, 0, 1]])


@pytest.mark.parametrize("binary", [False, True])
def test_fov_still_exits_and_names_the_supported_models(tmp_path, binary):
    from tools.colmap import model_io
    write_model(tmp_path, {1: ("FOV", 640, 480, [500.0, 510.0, 320.0, 240.0, 0.9])}, binary)
    for distorted in (False, True):
        with pytest.raises(SystemExit, match="FOV") as e:
            model_io.read_model(str(tmp_path), distorted=distorted)
    for name in ("PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV", "OPENCV_FISHEYE"):
        assert name in str(e.value), name


# ---------------------------------------------------------------------------------------------------- distortion formulas
X0, Y0 = 0.3, -0.2           # r2 = 0.13


def test_distort_matches_values_worked_by_hand():
    """One point per model, every coefficient non-zero, COLMAP's documented formulas written out with plain Python floats."""
    x, y = X0, Y0
    r2 = x * x + y * y
    r4, r6 = r2 ** 2, r2 ** 3
    close = lambda got, want: all(abs(float(g) - w) <= 4e-16 for g, w in zip(got, want))       # a few roundings of values below 1
    k = -0.11
    kind, c, *_ = U.model_coeffs("SIMPLE_RADIAL", [1.0, 0.0, 0.0, k])
    assert close(U.distort(kind, c, x, y), (x + x * (k * r2), y + y * (k * r2)))
    k1, k2 = -0.11, 0.03
    kind, c, *_ = U.model_coeffs("RADIAL", [1.0, 0.0, 0.0, k1, k2])
    assert close(U.distort(kind, c, x, y), (x + x * (k1 * r2 + k2 * r4), y + y * (k1 * r2 + k2 * r4)))
    p1, p2 = 0.002, -0.001
    kind, c, *_ = U.model_coeffs("OPENCV", [1.0, 1.0, 0.0, 0.0, k1, k2, p1, p2])
    want = (x + x * (k1 * r2 + k2 * r4) + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y + y * (k1 * r2 + k2 * r4) + 2 * p2 * x * y + p1 * (r2 + 2 * y * y))
    assert close(U.distort(kind, c, x, y), want)
    k3, k4, k5, k6 = 0.004, 0.05, -0.02, 0.006
    kind, c, *_ = U.model_coeffs("FULL_OPENCV", [1.0, 1.0, 0.0, 0.0, k1, k2, p1, p2, k3, k4, k5, k6])
    rad = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    want = (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y))
    assert close(U.distort(kind, c, x, y), want)
    f1, f2, f3, f4 = 0.05, -0.01, 0.003, -0.001
    kind, c, *_ = U.model_coeffs("OPENCV_FISHEYE", [1.0, 1.0, 0.0, 0.0, f1, f2, f3, f4])
    r = math.sqrt(r2)
    th = math.atan(r)
    thd = th * (1 + f1 * th ** 2 + f2 * th ** 4 + f3 * th ** 6 + f4 * th ** 8)
    assert close(U.distort(kind, c, x, y), (x * thd / r, y * thd / r))
    assert [float(v) for v in U.distort(kind, c, 0.0, 0.0)] == [0.0, 0.0]                  # r = 0: the point itself, no 0 / 0


def test_special_cases_are_bit_identical():
    rng = np.random.RandomState(5)
    x, y = rng.uniform(-0.8, 0.8, 500), rng.uniform(-0.6, 0.6, 500)
    bits = lambda model, params: np.stack(U.distort(*U.model_coeffs(model, params)[:2], x, y)).tobytes()
    assert bits("RADIAL", [1, 0, 0, -0.11, 0.0]) == bits("SIMPLE_RADIAL", [1, 0, 0, -0.11])
    assert bits("OPENCV", [1, 1, 0, 0, -0.11, 0.03, 0.0, 0.0]) == bits("RADIAL", [1, 0, 0, -0.11, 0.03])
    assert bits("FULL_OPENCV", [1, 1, 0, 0, -0.11, 0.03, 0.002, -0.001, 0, 0, 0, 0]) == bits("OPENCV", [1, 1, 0, 0, -0.11, 0.03, 0.002, -0.001])
    assert bits("OPENCV", [1, 1, 0, 0, -0.11, 0.03, 0.002, -0.001]) != bits("RADIAL", [1, 0, 0, -0.11, 0.03])


def test_host_distort_equals_the_oracles():
    """tools/colmap/undistort.py evaluates the zoom fit with its own copy of the map: the same bits as the oracle's."""
    from tools.colmap import undistort as UD
    rng = np.random.RandomState(6)
    x, y = rng.uniform(-0.8, 0.8, 500), rng.uniform(-0.6, 0.6, 500)
    x[0] = y[0] = 0.0
    for cid in (4, 5):
        kind, c = U.model_coeffs(CAMERAS[cid][0], CAMERAS[cid][3])[:2]
        assert np.stack(UD.distort(kind, c, x, y)).tobytes() == np.stack(U.distort(kind, c, x, y)).tobytes()


# ---------------------------------------------------------------------------------------------------- coordinate image
RAMP_CASES = {  # name -> (model, params, source (w, h), output (w, h), zoom, scale, nsub)
    "opencv_n1": ("OPENCV", [150.0, 148.0, 49.5, 31.25, -0.11, 0.03, 0.002, -0.001], (96, 64), (96, 64), 1.0, 1.0, 1),
    "full_n2": ("FULL_OPENCV", [300.0, 296.0, 101.5, 66.25, -0.11, 0.03, 0.002, -0.001, 0.004, 0.05, -0.02, 0.006], (200, 136), (96, 64), 1.0, 0.5, 2),
    "fisheye_n3": ("OPENCV_FISHEYE", [180.0, 178.0, 126.5, 83.25, 0.05, -0.01, 0.003, -0.001], (250, 170), (96, 64), 0.9, 0.4, 3),
    "radial_zoomed_out": ("RADIAL", [150.0, 49.5, 31.25, 0.08, 0.01], (96, 64), (96, 64), 0.6, 1.0, 1),
}


def direct_mean_uv(model, params, out_wh, zoom, scale, n):
    """Mean U and V of every output pixel, straight from the formulas of include/mdfnet_hip.h in plain numpy expressions (one grid of pixels per sub-sample)."""
    kind, c, fx, fy, cx, cy = U.model_coeffs(model, params)
    i, j = np.meshgrid(np.arange(out_wh[1], dtype=np.float64), np.arange(out_wh[0], dtype=np.float64), indexing="ij")
    su, sv = np.zeros_like(i), np.zeros_like(i)
    for b in range(n):
        for a in range(n):
            x = ((j + (a + 0.5) / n) / scale - cx) / (zoom * fx)
            y = ((i + (b + 0.5) / n) / scale - cy) / (zoom * fy)
            xd, yd = U.distort(kind, c, x, y)
            su += fx * xd + cx - 0.5
            sv += fy * yd + cy - 0.5
    return su / (n * n), sv / (n * n)


def ramp_expectation(name):
    """-> (oracle result on the ramp image, mean U, mean V, the pixels whose samples all lie in [0, W-1] x [0, H-1])."""
    model, params, (w, h), out_wh, zoom, scale, n = RAMP_CASES[name]
    kind, c, fx, fy, cx, cy = U.model_coeffs(model, params)
    res = U.undistort(U.ramp_image(h, w)[None], kind, c, fx, fy, cx, cy, (out_wh[1], out_wh[0]), zoom, scale, n)
    mu, mv = direct_mean_uv(model, params, out_wh, zoom, scale, n)
    inner = ((res["U"] >= 0) & (res["U"] <= w - 1) & (res["V"] >= 0) & (res["V"] <= h - 1)).all(axis=(0, 1)) & (res["valid"][0] == 1)
    return res, mu, mv, inner


@pytest.mark.parametrize("name", sorted(RAMP_CASES))
def test_ramp_image_reads_back_the_coordinates(name):
    res, mu, mv, inner = ramp_expectation(name)
    assert inner.sum() >= 0.25 * inner.size               # the assertion below speaks about a real share of the frame (z = 0.6 covers 0.36 of it)
    if name == "radial_zoomed_out":
        assert (res["valid"][0] == 0).any() and not inner.all()
    assert np.max(np.abs(res["mean"][0, :, :, 0][inner] - mu[inner])) <= 1e-9
    assert np.max(np.abs(res["mean"][0, :, :, 1][inner] - mv[inner])) <= 1e-9
    assert not res["mean"][0, :, :, 2].any()


# ---------------------------------------------------------------------------------------------------- zoom fit
# COLMAP's sign: xd = x (1 + k r2), so k < 0 pulls the samples towards the centre (a barrel-distorted photograph).  At z = 1 every
# sample of a k < 0 camera then lies inside the photograph (|xd| <= |x| while 1 + k r2 is in (0, 1]), so the smallest zoom without
# blanks is BELOW 1; with k > 0 the corner samples leave the photograph at z = 1 and the zoom must exceed 1.  The request for this
# feature named the two cases the other way round (barrel z > 1, pincushion z < 1), which contradicts its own formulas; the cases,
# the sizes and the two valid-mask conditions are the request's.  The focal length of the k = -0.2 case is long enough that r (1 + k r2) does not fold over
# (3 |k| r2 < 1) at the smallest zoom the bisection probes, or fit_zoom would refuse the camera.
FIT_CASES = {"barrel": ("SIMPLE_RADIAL", 96, 64, [240.0, 48.0, 32.0, -0.2]), "pincushion": ("SIMPLE_RADIAL", 96, 64, [80.0, 48.0, 32.0, 0.1])}


def fit_case(name):
    from tools.colmap import undistort as UD
    cam = FIT_CASES[name]
    p = UD.plan(cam, 0, "inside")
    kind, c, fx, fy, cx, cy = U.model_coeffs(cam[0], cam[3])
    return p, (kind, c, fx, fy, cx, cy)


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_fit_zoom_is_the_smallest_zoom_without_blanks(name):
    p, args = fit_case(name)
    z = p["z"]
    assert (z < 1.0) if name == "barrel" else (z > 1.0)
    assert 0.2 < z < 5.0 and p["n"] == 1 and p["s"] == 1.0 and p["out_size"] == (96, 64)
    src = U.noise_image(64, 96, 1)[None]
    assert U.undistort(src, *args, (64, 96), z, 1.0, 1)["valid"].all()
    assert (U.undistort(src, *args, (64, 96), z * (1 - 2.0 ** -8), 1.0, 1)["valid"] == 0).any()


def test_fit_zoom_refuses_what_it_cannot_fit():
    from tools.colmap import undistort as UD
    with pytest.raises(SystemExit, match="camera 9"):                 # r (1 + k r2) folds over inside the probed zooms
        UD.plan(("SIMPLE_RADIAL", 96, 64, [80.0, 48.0, 32.0, -0.2]), 0, "inside", what="camera 9")
    with pytest.raises(SystemExit, match="camera 9"):                 # zoom 5 still leaves blanks
        UD.plan(("SIMPLE_RADIAL", 96, 64, [10.0, 48.0, 32.0, 50.0]), 0, "inside", what="camera 9")
    assert UD.plan(("SIMPLE_RADIAL", 96, 64, [80.0, 48.0, 32.0, -0.2]), 0, "same")["z"] == 1.0


# ---------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("w,h,max_dim,s,n,out", [(200, 136, 0, 1.0, 1, (192, 128)), (200, 136, 100, 0.5, 2, (96, 64)), (250, 170, 100, 0.4, 3, (96, 64))])
def test_plan_sizes_and_output_camera(w, h, max_dim, s, n, out):
    from tools.colmap import undistort as UD
    cam = ("OPENCV", w, h, [300.0, 296.0, w / 2 + 1.5, h / 2 - 2.25, 0.05, 0.01, 0.002, -0.001])
    for fit in ("same", "inside"):
        p = UD.plan(cam, max_dim, fit)
        assert (p["s"], p["n"], p["out_size"], p["size"], p["kind"]) == (s, n, out, (w, h), "rational")
        z = p["z"]
        assert (z == 1.0) if fit == "same" else (1.0 < z < 1.2)
        assert np.array_equal(p["K_out"], [[z * 300.0 * s, 0, (w / 2 + 1.5) * s], [0, z * 296.0 * s, (h / 2 - 2.25) * s], [0, 0, 1]])


def test_plan_refuses_more_than_16_samples_a_side():
    from tools.colmap import undistort as UD
    cam = ("SIMPLE_RADIAL", 8000, 6000, [6000.0, 4000.0, 3000.0, 0.01])
    assert UD.plan(cam, 500, "same")["n"] == 16
    with pytest.raises(SystemExit, match="16"):
        UD.plan(cam, 499, "same")
    with pytest.raises(SystemExit, match="undistort_fit"):
        UD.plan(cam, 0, "outside")


def test_a_photograph_of_another_size_than_its_camera_exits(tmp_path):
    from PIL import Image
    from tools.colmap import undistort as UD
    path = str(tmp_path / "a.png")
    Image.fromarray(U.noise_image(64, 96, 3)).save(path)
    assert np.array_equal(UD.load_rgb(path, (96, 64), "camera 4"), U.noise_image(64, 96, 3))
    with pytest.raises(SystemExit, match=r"96 x 64.*camera 4 is 100 x 64"):
        UD.load_rgb(path, (100, 64), "camera 4")


# ---------------------------------------------------------------------------------------------------- ABI and command line
def test_abi_argument_errors_without_gpu():
    """Argument errors come back as -1 with a message and launch nothing (no GPU is needed to see them)."""
    import mdfnet_hip
    l = mdfnet_hip.lib()
    ptr = ctypes.c_void_p(256)                                         # never dereferenced: every check below fails first
    coeffs = (ctypes.c_double * 12)()
    d = ctypes.c_double

    def call(src=ptr, dst=ptr, B=1, hs=64, ws=96, hd=64, wd=96, kind=0, k=coeffs, fx=100.0, fy=100.0, zoom=1.0, scale=1.0, nsub=1):
        return l.mdf_image_undistort(src, dst, None, B, hs, ws, hd, wd, kind, k, d(fx), d(fy), d(48.0), d(32.0), d(zoom), d(scale), nsub, None)

    assert call(src=None) == -1 and b"null" in l.mdf_last_error()
    assert call(dst=None) == -1 and b"null" in l.mdf_last_error()
    assert call(k=None) == -1 and b"null" in l.mdf_last_error()
    assert call(B=0) == -1 and b"positive" in l.mdf_last_error()
    assert call(wd=-32) == -1 and b"positive" in l.mdf_last_error()
    for nsub in (0, 17):
        assert call(nsub=nsub) == -1 and b"nsub" in l.mdf_last_error()
    for fx in (0.0, float("nan"), float("inf"), -5.0):
        assert call(fx=fx) == -1 and b"focal" in l.mdf_last_error()
        assert call(fy=fx) == -1 and b"focal" in l.mdf_last_error()
    for z in (0.0, float("nan")):
        assert call(zoom=z) == -1 and b"zoom" in l.mdf_last_error()
        assert call(scale=z) == -1 and b"scale" in l.mdf_last_error()
    assert call(kind=2) == -1 and b"kind" in l.mdf_last_error()
    assert call(B=8, hs=20000, ws=20000) == -1 and b"int32" in l.mdf_last_error()
    assert call(B=2, hd=1 << 16, wd=1 << 16) == -1 and b"int32" in l.mdf_last_error()
    assert call(B=1 << 30, hs=1 << 30, ws=1 << 30) == -1 and b"int32" in l.mdf_last_error()         # no overflow inside the check
    bad = (ctypes.c_double * 12)(*([0.0] * 5 + [float("nan")] + [0.0] * 6))
    assert call(k=bad) == -1 and b"coeffs[5]" in l.mdf_last_error()


def test_ops_refuse_what_is_not_a_gpu_uint8_image():
    import torch
    from mdfnet_hip import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.undistort_images(torch.zeros((1, 64, 96, 3), dtype=torch.uint8), "rational", [0.0], 100.0, 100.0, 48.0, 32.0, (64, 96))


def test_command_line_flags():
    from tools.colmap import main as importer
    base = ["--model", "m", "--images", "i", "--out", "o"]
    a = importer.build_parser().parse_args(base)
    assert a.undistort is False and a.undistort_fit == "inside"
    a = importer.build_parser().parse_args(base + ["--undistort", "--undistort_fit", "same"])
    assert a.undistort is True and a.undistort_fit == "same"
    with pytest.raises(SystemExit):
        importer.build_parser().parse_args(base + ["--undistort_fit", "outside"])
    with pytest.raises(SystemExit, match="undistort_fit"):
        importer.import_scene("m", "i", "o", undistort=True, undistort_fit="outside")
