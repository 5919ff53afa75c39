"""Reading a COLMAP sparse model, text (cameras.txt, images.txt, points3D.txt) or binary (.bin), and turning it into the arrays the
view-selection kernels take (ops.view_scores / ops.view_depth_ranges): world -> camera rotations from the (qw, qx, qy, qz)
quaternions, translations, intrinsics, the points and their tracks as a CSR by point."""
import os
import struct

import numpy as np

# model id -> (name, number of parameters), COLMAP's camera model table
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
SUPPORTED_MODELS = ("PINHOLE", "SIMPLE_PINHOLE")
# read with distorted=True besides those two (main.py --undistort resamples their images on the GPU: tools/colmap/undistort.py)
DISTORTED_MODELS = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV", "OPENCV_FISHEYE")
ONE_FOCAL_MODELS = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


def _data_lines(path):
    with open(path) as f:
        return [ln.rstrip("\n") for ln in f if not ln.lstrip().startswith("#")]


def _read_text(folder):
    cameras = {}
    for ln in _data_lines(os.path.join(folder, "cameras.txt")):
        tok = ln.split()
        if tok:
            cameras[int(tok[0])] = (tok[1], int(tok[2]), int(tok[3]), np.array([float(x) for x in tok[4:]], dtype=np.float64))
    images = []
    lines = _data_lines(os.path.join(folder, "images.txt"))
    while lines and not lines[-1].strip():
        lines.pop()
    for k in range(0, len(lines), 2):                      # two lines an image; the second (its 2-D points) may be empty
        tok = lines[k].split()
        images.append((int(tok[0]), [float(x) for x in tok[1:5]], [float(x) for x in tok[5:8]], int(tok[8]), " ".join(tok[9:])))
    points = []
    for ln in _data_lines(os.path.join(folder, "points3D.txt")):
        tok = ln.split()
        if tok:
            points.append((int(tok[0]), [float(x) for x in tok[1:4]], [int(x) for x in tok[8::2]]))
    return cameras, images, points


def _unpack(f, fmt):
    return struct.unpack("<" + fmt, f.read(struct.calcsize("<" + fmt)))


def _read_binary(folder):
    cameras, images, points = {}, [], []
    with open(os.path.join(folder, "cameras.bin"), "rb") as f:
        for _ in range(_unpack(f, "Q")[0]):
            cam_id, model_id, w, h = _unpack(f, "iiQQ")
            if model_id not in CAMERA_MODELS:
                raise SystemExit(f"cameras.bin: unknown camera model id {model_id}")
            name, k = CAMERA_MODELS[model_id]
            cameras[cam_id] = (name, int(w), int(h), np.array(_unpack(f, "d" * k), dtype=np.float64))
    with open(os.path.join(folder, "images.bin"), "rb") as f:
        for _ in range(_unpack(f, "Q")[0]):
            v = _unpack(f, "idddddddi")
            name = b""
            while True:
                c = f.read(1)
                if c in (b"\0", b""):
                    break
                name += c
            f.seek(24 * _unpack(f, "Q")[0], 1)              # the 2-D points (x, y, point id): the tracks come from points3D
            images.append((v[0], list(v[1:5]), list(v[5:8]), v[8], name.decode("utf-8")))
    with open(os.path.join(folder, "points3D.bin"), "rb") as f:
        for _ in range(_unpack(f, "Q")[0]):
            v = _unpack(f, "QdddBBBdQ")
            track = np.frombuffer(f.read(8 * v[8]), dtype="<i4").reshape(-1, 2)
            points.append((v[0], list(v[1:4]), track[:, 0].tolist()))
    return cameras, images, points


def read_model(folder, distorted=False):
    """-> dict of arrays, images in ascending COLMAP image id and points in ascending point id:
    camera_models {camera id: (model name, width, height, params)}, image_ids [N] int64, qvec [N,4], tvec [N,3] float64,
    camera_ids [N] int64, names (list), point_ids [P] int64, xyz [P,3] float64, track_off [P+1] int64, track_image_ids [T] int64
    (COLMAP image ids, in file order).  The binary files are used when cameras.bin exists, else the text files.  A camera that is not
    PINHOLE or SIMPLE_PINHOLE exits with the advice; with distorted=True the DISTORTED_MODELS are read as well."""
    cameras, images, points = _read_binary(folder) if os.path.exists(os.path.join(folder, "cameras.bin")) else _read_text(folder)
    for cam_id, (name, _, _, params) in sorted(cameras.items()):
        if distorted and name not in SUPPORTED_MODELS + DISTORTED_MODELS:
            raise SystemExit(f"camera {cam_id} has model {name}: --undistort reads {', '.join(SUPPORTED_MODELS + DISTORTED_MODELS)}. "
                             "Undistort the images first (colmap image_undistorter) and import the undistorted sparse model")
        if not distorted and name not in SUPPORTED_MODELS:
            raise SystemExit(f"camera {cam_id} has model {name}: only {' and '.join(SUPPORTED_MODELS)} are read. Undistort the images first "
                             "(colmap image_undistorter) and import the undistorted sparse model, or pass --undistort")
        want = next(k for n, k in CAMERA_MODELS.values() if n == name)
        if len(params) != want:
            raise SystemExit(f"camera {cam_id} ({name}) has {len(params)} parameters, {want} expected")
    images.sort(key=lambda r: r[0])
    points.sort(key=lambda r: r[0])
    lens = np.array([len(p[2]) for p in points], dtype=np.int64)
    return {"camera_models": cameras,
            "image_ids": np.array([r[0] for r in images], dtype=np.int64),
            "qvec": np.array([r[1] for r in images], dtype=np.float64).reshape(-1, 4),
            "tvec": np.array([r[2] for r in images], dtype=np.float64).reshape(-1, 3),
            "camera_ids": np.array([r[3] for r in images], dtype=np.int64),
            "names": [r[4] for r in images],
            "point_ids": np.array([p[0] for p in points], dtype=np.int64),
            "xyz": np.array([p[1] for p in points], dtype=np.float64).reshape(-1, 3),
            "track_off": np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens)]),
            "track_image_ids": np.array([i for p in points for i in p[2]], dtype=np.int64)}


def quaternion_to_rotation(q):
    """(qw, qx, qy, qz) [N,4] -> rotation matrices [N,3,3] (the quaternion is normalised first)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y,
                     2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                     2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], axis=1).reshape(-1, 3, 3)


def intrinsics(camera):
    """(model, width, height, params) -> K [3,3] float64 (f on both axes for a model with one focal length)."""
    name, _, _, p = camera
    fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if name in ONE_FOCAL_MODELS else (p[0], p[1], p[2], p[3])
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)


def distortion(camera):
    """(model, width, height, params) -> (kind, coeffs [12] float64), the arguments of ops.undistort_images: kind "rational" with
    k1, k2, p1, p2, k3, k4, k5, k6 (SIMPLE_RADIAL, RADIAL, OPENCV and the pinhole models are special cases with zeros) or "fisheye"
    with k1..k4 (OPENCV_FISHEYE); the rest of coeffs is zero."""
    name, _, _, p = camera
    p = np.asarray(p, dtype=np.float64)
    c = np.zeros(12, dtype=np.float64)
    if name == "OPENCV_FISHEYE":
        c[:4] = p[4:8]
        return "fisheye", c
    if name == "SIMPLE_RADIAL":
        c[0] = p[3]
    elif name == "RADIAL":
        c[:2] = p[3:5]
    elif name == "OPENCV":
        c[:4] = p[4:8]
    elif name == "FULL_OPENCV":
        c[:8] = p[4:12]
    elif name not in SUPPORTED_MODELS:
        raise SystemExit(f"camera model {name}: no distortion model here ({', '.join(SUPPORTED_MODELS + DISTORTED_MODELS)})")
    return "rational", c


def tracks_csr(point_index, image_index, n_pts):
    """Observations (point index, image index), in any order and with repeats -> the CSR by point with strictly ascending image
    indices inside a track: track_off [n_pts + 1] int64, track_img [T] int32."""
    pairs = np.unique(np.stack([np.asarray(point_index, dtype=np.int64), np.asarray(image_index, dtype=np.int64)], 1).reshape(-1, 2), axis=0)
    off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.bincount(pairs[:, 0], minlength=n_pts))]).astype(np.int64)
    return off, pairs[:, 1].astype(np.int32)


def scene_arrays(model, log=print):
    """The model as the kernels' inputs.  Points with non-finite coordinates are dropped (their number is reported), observations
    of images the model does not list are dropped, an image without observations is left out (one line each), and the remaining
    images get dense ids 0..N-1 in ascending COLMAP id.
    -> dict: rot [N,3,3], trans [N,3], K [N,3,3], size [N,2] (width, height), colmap_ids [N], names, pts [P,3], track_off [P+1]
    int64, track_img [T] int32, camera_ids [N] (COLMAP camera id per image), cameras (per image its (model, width, height, params))."""
    finite = np.isfinite(model["xyz"]).all(axis=1)
    if not finite.all():
        log(f"dropped {int((~finite).sum())} of {len(finite)} points with non-finite coordinates")
    lens = np.diff(model["track_off"])
    pt_of_obs = np.repeat(np.arange(len(lens)), lens)
    ids = model["image_ids"]
    pos = np.searchsorted(ids, model["track_image_ids"])
    known = (pos < len(ids)) & (ids[np.minimum(pos, max(len(ids) - 1, 0))] == model["track_image_ids"]) if len(ids) else np.zeros(len(pos), bool)
    use = known & finite[pt_of_obs]
    seen = np.zeros(len(ids), dtype=bool)
    seen[pos[use]] = True
    for i in np.flatnonzero(~seen):
        log(f"image {int(ids[i])} ({model['names'][i]}) has no observations: left out")
    dense = np.cumsum(seen) - 1                                   # image position -> dense id
    new_pt = np.cumsum(finite) - 1
    off, img = tracks_csr(new_pt[pt_of_obs[use]], dense[pos[use]], int(finite.sum()))
    keep = np.flatnonzero(seen)
    cams = [model["camera_models"][int(c)] for c in model["camera_ids"][keep]]
    return {"rot": quaternion_to_rotation(model["qvec"][keep]), "trans": np.ascontiguousarray(model["tvec"][keep]),
            "K": np.stack([intrinsics(c) for c in cams]) if cams else np.zeros((0, 3, 3)),
            "size": np.array([[c[1], c[2]] for c in cams], dtype=np.int64).reshape(-1, 2),
            "colmap_ids": ids[keep], "names": [model["names"][i] for i in keep],
            "camera_ids": model["camera_ids"][keep], "cameras": cams,
            "pts": np.ascontiguousarray(model["xyz"][finite]), "track_off": off, "track_img": img}
