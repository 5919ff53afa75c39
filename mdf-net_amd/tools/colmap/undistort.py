"""Scene import with --undistort: the images of a SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV or OPENCV_FISHEYE camera are resampled
to a pinhole camera on the GPU (ops.undistort_images: mdf_image_undistort, include/mdfnet_hip.h states the arithmetic).

Conventions ("Undistortion").  Pixel j covers [j, j + 1), its centre is j + 0.5.  For a camera (fx, fy, cx, cy, W, H)
and the --max_dim scale s, the written image has main.py's size (round(W s), round(H s), cropped to multiples of 32) and the camera
K_out = [[z fx s, 0, cx s], [0, z fy s, cy s], [0, 0, 1]]; every output pixel is the mean of n x n samples, n = 1 at s = 1, else
ceil(1 / s).  z is 1 (--undistort_fit same: pixels the photograph does not cover stay black) or the smallest zoom at which every sample
of the outermost rows and columns falls inside the photograph (inside, the default), found here in float64 by bisection."""
import math

import numpy as np

from tools.colmap import model_io

MULTIPLE = 32
MAX_NSUB = 16
GROUP = 8                          # images per launch
ZOOM_RANGE = (0.2, 5.0)
ZOOM_REL_WIDTH = 2.0 ** -20
FITS = ("same", "inside")


def distort(kind, c, x, y):
    """(x, y) normalised undistorted -> (xd, yd), float64 arrays, in the order the kernel states."""
    xx, yy = x * x, y * y
    r2 = xx + yy
    if kind == "rational":
        r4 = r2 * r2
        r6 = r4 * r2
        rad = (((1.0 + c[0] * r2) + c[1] * r4) + c[4] * r6) / (((1.0 + c[5] * r2) + c[6] * r4) + c[7] * r6)
        q = 2.0 * (x * y)
        return x * rad + (c[2] * q + c[3] * (r2 + 2.0 * xx)), y * rad + (c[3] * q + c[2] * (r2 + 2.0 * yy))
    r = np.sqrt(r2)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.arctan(r)
        t2 = t * t
        t4 = t2 * t2
        sc = (t * ((((1.0 + c[0] * t2) + c[1] * t4) + c[2] * (t4 * t2)) + c[3] * (t4 * t4))) / r
        return np.where(r == 0.0, x, x * sc), np.where(r == 0.0, y, y * sc)


def border_blanks(kind, coeffs, fx, fy, cx, cy, size, out_size, z, s, n):
    """How many samples of the output's rows 0 and ch - 1 and columns 0 and cw - 1 are blank at zoom z (a pixel on two of them
    counts twice: only zero or not, and the order of the counts, matter)."""
    (w, h), (cw, ch) = size, out_size
    sub = (np.arange(n, dtype=np.float64) + 0.5) / n
    xs = ((np.arange(cw, dtype=np.float64)[:, None] + sub[None, :]) / s).reshape(-1)
    ys = ((np.arange(ch, dtype=np.float64)[:, None] + sub[None, :]) / s).reshape(-1)
    edge_x = ((np.array([0.0, cw - 1.0])[:, None] + sub[None, :]) / s).reshape(-1)
    edge_y = ((np.array([0.0, ch - 1.0])[:, None] + sub[None, :]) / s).reshape(-1)
    blanks = 0
    with np.errstate(all="ignore"):
        for X, Y in ((xs[:, None], edge_y[None, :]), (edge_x[:, None], ys[None, :])):
            x, y = np.broadcast_arrays((X - cx) / (z * fx), (Y - cy) / (z * fy))
            xd, yd = distort(kind, coeffs, x, y)
            U, V = (fx * xd + cx) - 0.5, (fy * yd + cy) - 0.5
            inside = (U >= -0.5) & (U <= w - 0.5) & (V >= -0.5) & (V <= h - 0.5)      # a NaN compares false
            blanks += int(inside.size - np.count_nonzero(inside))
    return blanks


def fit_zoom(kind, coeffs, fx, fy, cx, cy, size, out_size, s, n, what="camera"):
    """The smallest zoom in ZOOM_RANGE for which no sample of the outermost output rows and columns is blank: bisection down to a
    relative width of 2^-20, the upper end returned.  Exits when the largest zoom still leaves blanks or the blank count does not
    fall with the zoom at the probes."""
    lo, hi = ZOOM_RANGE
    count = lambda z: border_blanks(kind, coeffs, fx, fy, cx, cy, size, out_size, z, s, n)
    probes = {lo: count(lo), hi: count(hi)}
    if probes[hi] != 0:
        raise SystemExit(f"{what}: at zoom {hi} {probes[hi]} border samples still fall outside the photograph; use --undistort_fit same")
    if probes[lo] == 0:
        return lo
    while (hi - lo) > ZOOM_REL_WIDTH * hi:
        mid = 0.5 * (lo + hi)
        probes[mid] = count(mid)
        if probes[mid] == 0:
            hi = mid
        else:
            lo = mid
    zs = sorted(probes)
    if any(probes[a] < probes[b] for a, b in zip(zs, zs[1:])):
        raise SystemExit(f"{what}: the number of blank border samples does not fall with the zoom (the distortion folds over inside "
                         f"[{ZOOM_RANGE[0]}, {ZOOM_RANGE[1]}]); use --undistort_fit same")
    return hi


def plan(camera, max_dim=0, fit="inside", what="camera"):
    """camera (model, width, height, params) -> dict: kind, coeffs [12], fx, fy, cx, cy, size (W, H), z, s, n, out_size (cw, ch), K_out."""
    if fit not in FITS:
        raise SystemExit(f"--undistort_fit {fit!r}: one of {', '.join(FITS)}")
    _, w, h, _ = camera
    K = model_io.intrinsics(camera)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    kind, coeffs = model_io.distortion(camera)
    s = float(max_dim) / max(w, h) if max_dim > 0 and max(w, h) > max_dim else 1.0
    sw, sh = (max(int(round(w * s)), 1), max(int(round(h * s)), 1)) if s != 1.0 else (w, h)
    cw, ch = sw // MULTIPLE * MULTIPLE, sh // MULTIPLE * MULTIPLE
    if cw == 0 or ch == 0:
        raise SystemExit(f"{what}: {sw} x {sh} pixels leave nothing after the crop to multiples of {MULTIPLE}")
    n = 1 if s == 1.0 else int(math.ceil(1.0 / s))
    if n > MAX_NSUB:
        raise SystemExit(f"{what}: --max_dim {max_dim} scales {w} x {h} down by more than {MAX_NSUB}; scale the photographs first")
    z = 1.0 if fit == "same" else fit_zoom(kind, coeffs, fx, fy, cx, cy, (w, h), (cw, ch), s, n, what)
    K_out = np.array([[z * fx * s, 0, cx * s], [0, z * fy * s, cy * s], [0, 0, 1]], dtype=np.float64)
    return {"kind": kind, "coeffs": coeffs, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "size": (w, h), "z": z, "s": s, "n": n,
            "out_size": (cw, ch), "K_out": K_out, "fit": fit}


def load_rgb(path, size, what):
    """The photograph as [H,W,3] uint8 (EXIF orientation ignored, as COLMAP ignores it); exits unless it has the camera's size."""
    from PIL import Image
    with Image.open(path) as im:
        if im.size != tuple(size):
            raise SystemExit(f"{path}: {im.size[0]} x {im.size[1]} pixels, but {what} is {size[0]} x {size[1]}")
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def save_jpeg(rgb, path):
    from PIL import Image
    Image.fromarray(rgb).save(path, format="JPEG", quality=95)


def undistort_group(paths, p, device, what="camera", want_valid=False):
    """Decode -> upload -> kernel -> download for up to GROUP photographs that share the plan p -> (dst [B,ch,cw,3] uint8 numpy,
    valid [B,ch,cw] or None)."""
    import torch
    from mdfnet_hip import ops
    src = torch.from_numpy(np.stack([load_rgb(path, p["size"], what) for path in paths])).to(device)
    res = ops.undistort_images(src, p["kind"], p["coeffs"], p["fx"], p["fy"], p["cx"], p["cy"], (p["out_size"][1], p["out_size"][0]),
                               zoom=p["z"], scale=p["s"], nsub=p["n"], want_valid=want_valid)
    dst, valid = res if want_valid else (res, None)
    return dst.cpu().numpy(), (valid.cpu().numpy() if want_valid else None)


def export_images(jobs, p, device, what="camera", log=print):
    """jobs: (source path, JPEG path to write) of the images of one distorted camera; written in groups of at most GROUP per launch.
    One line is logged: the zoom and, for fit same, the share of pixels with a blank sample."""
    want_valid = p["fit"] == "same"
    blank, total = 0, 0
    for k in range(0, len(jobs), GROUP):
        part = jobs[k:k + GROUP]
        dst, valid = undistort_group([src for src, _ in part], p, device, what, want_valid)
        for (_, out), img in zip(part, dst):
            save_jpeg(img, out)
        if want_valid:
            blank, total = blank + int(valid.size - np.count_nonzero(valid)), total + valid.size
    line = f"{what}: {len(jobs)} images undistorted to {p['out_size'][0]} x {p['out_size'][1]}, zoom {p['z']!r} ({p['fit']}), {p['n']} x {p['n']} samples a pixel"
    log(line + (f", {100.0 * blank / max(total, 1):.2f} % of the pixels not covered by the photograph (black)" if want_valid else ""))
