"""Host-side file I/O of the eval data plane (counterpart of the reference's tools/data_io.py:6-130).
PFM: 'Pf\\n<w> <h>\\n-1.000000\\n' + bottom-up little-endian float32 rows (data_io.py:44-71)."""
import re
import sys

import numpy as np
import torch


def read_pfm(filename):
    with open(filename, "rb") as f:
        kind = f.readline().decode("utf-8").rstrip()
        if kind not in ("PF", "Pf"):
            raise Exception("Not a PFM file.")
        m = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
        if not m:
            raise Exception("Malformed PFM header.")
        width, height = int(m.group(1)), int(m.group(2))
        scale = float(f.readline().rstrip())
        endian = "<" if scale < 0 else ">"
        data = np.fromfile(f, endian + "f")
    shape = (height, width, 3) if kind == "PF" else (height, width)
    return np.flipud(data.reshape(shape)), abs(scale)


def save_pfm(filename, image, scale=1):
    image = np.flipud(np.asarray(image))
    if image.dtype.name != "float32":
        raise Exception("Image dtype must be float32.")
    if image.ndim == 3 and image.shape[2] == 3:
        header = "PF\n"
    elif image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1):
        header = "Pf\n"
    else:
        raise Exception("Image must have H x W x 3, H x W x 1 or H x W dimensions.")
    if image.dtype.byteorder == "<" or (image.dtype.byteorder == "=" and sys.byteorder == "little"):
        scale = -scale
    with open(filename, "wb") as f:
        f.write(header.encode("utf-8"))
        f.write("{} {}\n".format(image.shape[1], image.shape[0]).encode("utf-8"))
        f.write(("%f\n" % scale).encode("utf-8"))
        image.tofile(f)


def write_depth_img(filename, depth):
    from PIL import Image
    Image.fromarray((depth - 500) / 2).convert("L").save(filename)
    return 1


def read_pairfile(pair_path):
    """-> (num_viewpoint, [[ref_view, [src views sorted by score]], ...])   (data_io.py:79-89)"""
    pairs = []
    with open(pair_path) as f:
        n = int(f.readline())
        for _ in range(n):
            ref = int(f.readline().rstrip())
            srcs = [int(x) for x in f.readline().rstrip().split()[1::2]]
            pairs.append([ref, srcs])
    return n, pairs


def read_cam_file(filename, with_range=False):
    """extrinsic 4x4 on lines 1-4, intrinsic 3x3 on lines 7-9, optional depth range on line 11 (data_io.py:92-101)."""
    with open(filename) as f:
        lines = [ln.rstrip() for ln in f.readlines()]
    extrinsic = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intrinsic = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    if with_range:
        return intrinsic, extrinsic, np.array(lines[11].split(), dtype=np.float32)
    return intrinsic, extrinsic


def resize_nearest(img, size):
    """cv2.resize(img, (w, h), interpolation=cv2.INTER_NEAREST) without OpenCV (absent here; used by load/dtutrain.py:55-57
    and load/blendedtrain.py:48-50 for the 1/8, 1/4, 1/2 ground-truth maps).  OpenCV's nearest neighbour is NOT
    centre-aligned: source index = min(floor(dst_index * (src/dst)), src - 1) with the ratio in double precision
    (resize.cpp, resizeNN).  For the power-of-two factors the loaders use on divisible sizes this is plain striding."""
    w, h = int(size[0]), int(size[1])
    sh, sw = img.shape[:2]
    ys = np.minimum(np.floor(np.arange(h, dtype=np.float64) * (sh / h)).astype(np.int64), sh - 1)
    xs = np.minimum(np.floor(np.arange(w, dtype=np.float64) * (sw / w)).astype(np.int64), sw - 1)
    return np.ascontiguousarray(img[ys][:, xs])


def read_img(filename):
    from PIL import Image
    return np.array(Image.open(filename), dtype=np.float32) / 255.0


def write_ply(path, xyz, rgb, normals=None):
    """Vertices with float x,y,z (15 bytes each) + uchar red,green,blue; binary_little_endian 1.0 (what PlyData([el]).write produces).
    With normals [M,3], float nx,ny,nz follow z (27 bytes a vertex); read them back with read_ply_normals."""
    xyz = np.asarray(xyz, dtype="<f4").reshape(-1, 3)
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        normals = np.asarray(normals, dtype="<f4").reshape(-1, 3)
        if len(normals) != len(xyz):
            raise ValueError(f"{len(normals)} normals for {len(xyz)} points")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    rec = np.empty(len(xyz), dtype=fields + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    nprops = ""
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
        nprops = "property float nx\nproperty float ny\nproperty float nz\n"
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "%sproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % (len(rec), nprops))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        rec.tofile(f)


def read_ply_normals(path):
    """The normals variant of write_ply -> (xyz [M,3] f32, rgb [M,3] u8, normals [M,3] f32)."""
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                n = int(line.split()[-1])
            if line == "end_header":
                break
        rec = np.fromfile(f, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                    ("red", "u1"), ("green", "u1"), ("blue", "u1")], count=n)
    return (np.stack([rec["x"], rec["y"], rec["z"]], 1), np.stack([rec["red"], rec["green"], rec["blue"]], 1),
            np.stack([rec["nx"], rec["ny"], rec["nz"]], 1))


def read_ply(path):
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                n = int(line.split()[-1])
            if line == "end_header":
                break
        rec = np.fromfile(f, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")], count=n)
    return np.stack([rec["x"], rec["y"], rec["z"]], 1), np.stack([rec["red"], rec["green"], rec["blue"]], 1)


_MESH_VERTEX = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
_MESH_FACE = [("n", "u1"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")]


def write_ply_mesh(path, xyz, rgb, faces):
    """A triangle mesh, binary_little_endian 1.0: vertices as write_ply writes them (float x,y,z + uchar red,green,blue, 15 bytes
    each), then `element face` with `property list uchar int vertex_indices` (a count byte 3 and three int32, 13 bytes each)."""
    xyz = np.asarray(xyz, dtype="<f4").reshape(-1, 3)
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    if len(rgb) != len(xyz):
        raise ValueError(f"{len(rgb)} colours for {len(xyz)} vertices")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(xyz)):
        raise ValueError(f"face indices out of range [0,{len(xyz)})")
    vert = np.empty(len(xyz), dtype=_MESH_VERTEX)
    vert["x"], vert["y"], vert["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    vert["red"], vert["green"], vert["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    face = np.empty(len(faces), dtype=_MESH_FACE)
    face["n"] = 3
    face["a"], face["b"], face["c"] = faces[:, 0], faces[:, 1], faces[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (len(vert), len(face)))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        vert.tofile(f)
        face.tofile(f)


def read_ply_mesh(path):
    """What write_ply_mesh wrote -> (xyz [N,3] f32, rgb [N,3] u8, faces [M,3] int32)."""
    with open(path, "rb") as f:
        nv = nf = None
        while True:
            raw = f.readline()
            if not raw:
                raise ValueError(f"{path}: PLY header without end_header")
            line = raw.decode("ascii").strip()
            if line.startswith("element vertex"):
                nv = int(line.split()[-1])
            elif line.startswith("element face"):
                nf = int(line.split()[-1])
            elif line == "end_header":
                break
        if nv is None or nf is None:
            raise ValueError(f"{path}: a vertex and a face element are expected")
        vert = np.fromfile(f, dtype=_MESH_VERTEX, count=nv)
        face = np.fromfile(f, dtype=_MESH_FACE, count=nf)
    if len(vert) != nv or len(face) != nf or (nf and not (face["n"] == 3).all()):
        raise ValueError(f"{path}: truncated, or a face that is not a triangle")
    return (np.stack([vert["x"], vert["y"], vert["z"]], 1), np.stack([vert["red"], vert["green"], vert["blue"]], 1),
            np.stack([face["a"], face["b"], face["c"]], 1).astype(np.int32))


def tocuda(data_batch, device, parallel=False):
    out = {}
    for k, v in data_batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to(device)
        elif isinstance(v, dict):
            out[k] = {k2: v2.to(device) for k2, v2 in v.items()}
    return out


# --------------------------------------------------------------------------- general PLY vertex reader (the DTU scorer's plyread)
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8",
              "float64": "f8"}


def _ply_header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError("PLY header without end_header")
        tok = raw.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], None, (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
        elif tok[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"unknown PLY format {fmt}")
    return fmt, elements


def _ply_binary_rows(f, count, props, end):
    """Rows of an element with list properties, one at a time -> {name: [values]} for the scalar properties."""
    out = {name: [] for name, t, _ in props if t is not None}
    for _ in range(count):
        for name, t, lt in props:
            if t is not None:
                dt = np.dtype(end + t)
                out[name].append(np.frombuffer(f.read(dt.itemsize), dtype=dt)[0])
            else:
                ct, it = np.dtype(end + lt[0]), np.dtype(end + lt[1])
                k = int(np.frombuffer(f.read(ct.itemsize), dtype=ct)[0])
                f.read(k * it.itemsize)
    return out


def read_ply_vertices(path):
    """The x, y, z of a PLY file's vertex element as float64 [N,3], whatever the format (ascii, binary little / big endian), the
    property types, the extra properties or the elements around it (what the DTU scorer's plyread returns as Mesh.vertex)."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f)
        if fmt == "ascii":
            lines = iter(f.read().decode("ascii").split("\n"))
            for name, count, props in elements:
                rows = []
                for _ in range(count):
                    line = next(lines).split()
                    while not line:
                        line = next(lines).split()
                    if name != "vertex":
                        continue
                    vals, k = {}, 0
                    for pname, t, lt in props:
                        if t is not None:
                            vals[pname] = float(line[k])
                            k += 1
                        else:
                            k += 1 + int(line[k])
                    rows.append((vals["x"], vals["y"], vals["z"]))
                if name == "vertex":
                    return np.array(rows, dtype=np.float64).reshape(-1, 3)
            raise ValueError(f"{path}: no vertex element")
        end = "<" if fmt == "binary_little_endian" else ">"
        for name, count, props in elements:
            if all(t is not None for _, t, _ in props):
                dt = np.dtype([(pname, end + t) for pname, t, _ in props])
                if name == "vertex":
                    rec = np.frombuffer(f.read(dt.itemsize * count), dtype=dt, count=count)
                    return np.stack([rec["x"].astype(np.float64), rec["y"].astype(np.float64), rec["z"].astype(np.float64)], 1)
                f.seek(dt.itemsize * count, 1)
            else:
                rows = _ply_binary_rows(f, count, props, end)
                if name == "vertex":
                    return np.stack([np.asarray(rows[a], dtype=np.float64) for a in ("x", "y", "z")], 1).reshape(-1, 3)
        raise ValueError(f"{path}: no vertex element")


# --------------------------------------------------------------------------- MAT-file level 5 (the DTU ObsMask / Plane files)
_MI = {1: "i1", 2: "u1", 3: "i2", 4: "u2", 5: "i4", 6: "u4", 7: "f4", 9: "f8", 12: "i8", 13: "u8"}
_MX = {6: "f8", 7: "f4", 8: "i1", 9: "u1", 10: "i2", 11: "u2", 12: "i4", 13: "u4", 14: "i8", 15: "u8"}
_MI_MATRIX, _MI_COMPRESSED, _MI_INT8 = 14, 15, 1


def _mat_elements(buf, end):
    """(type, payload) of the data elements in buf (small elements: 2-byte type, 2-byte size, 4 bytes of data)."""
    pos = 0
    while pos + 8 <= len(buf):
        t, nb = np.frombuffer(buf, dtype=end + "u4", count=2, offset=pos)
        t, nb = int(t), int(nb)
        if t >> 16:                                 # small data element
            yield t & 0xFFFF, buf[pos + 4:pos + 4 + (t >> 16)]
            pos += 8
            continue
        yield t, buf[pos + 8:pos + 8 + nb]
        pos += 8 + (nb if t == _MI_COMPRESSED else (nb + 7) // 8 * 8)


def _mat_matrix(payload, end):
    sub = list(_mat_elements(payload, end))
    flags = int(np.frombuffer(sub[0][1], dtype=end + "u4", count=1)[0])
    cls, logical, cplx = flags & 0xFF, bool(flags & 0x200), bool(flags & 0x800)
    dims = tuple(int(x) for x in np.frombuffer(sub[1][1], dtype=end + _MI[sub[1][0]]))
    name = bytes(sub[2][1]).decode("ascii")
    if cls not in _MX or cplx:
        return name, None                            # struct / cell / char / sparse / complex: not needed here
    t, data = sub[3]
    arr = np.frombuffer(data, dtype=end + _MI[t]).astype(_MX[cls])
    arr = arr.reshape(dims, order="F")
    return name, (arr.astype(bool) if logical else arr)


def read_mat(path):
    """A MAT-file (level 5) -> {name: numpy array} for its numeric and logical arrays, in MATLAB's dimension order (column-major
    data), compressed elements or not.  Other variables (structs, cells, strings, sparse, complex) are skipped."""
    import zlib
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 128:
        raise ValueError(f"{path}: not a MAT-file")
    end = {b"IM": "<", b"MI": ">"}.get(raw[126:128])
    if end is None or raw[:6] == b"MATLAB" and b"7.3" in raw[:20]:
        raise ValueError(f"{path}: not a level-5 MAT-file")
    out = {}
    for t, payload in _mat_elements(raw[128:], end):
        if t == _MI_COMPRESSED:
            inner = zlib.decompress(bytes(payload))
            t, payload = next(_mat_elements(inner, end))
        if t != _MI_MATRIX:
            continue
        name, arr = _mat_matrix(payload, end)
        if arr is not None:
            out[name] = arr
    return out


_MX_OF = {np.dtype("f8"): (6, 9), np.dtype("f4"): (7, 7), np.dtype("i1"): (8, 1), np.dtype("u1"): (9, 2), np.dtype("i2"): (10, 3),
          np.dtype("u2"): (11, 4), np.dtype("i4"): (12, 5), np.dtype("u4"): (13, 6), np.dtype("i8"): (14, 12), np.dtype("u8"): (15, 13)}


def _mat_el(t, payload):
    pad = (-len(payload)) % 8
    return np.array([t, len(payload)], dtype="<u4").tobytes() + payload + b"\0" * pad


def write_mat(path, arrays):
    """{name: array} -> an uncompressed little-endian MAT-file (level 5).  Numeric and bool arrays; a bool array is written as
    a logical uint8 array, a scalar as 1x1, a vector as a row (1 x n), as MATLAB's save does."""
    body = b""
    for name, a in arrays.items():
        a = np.asarray(a)
        logical = a.dtype == np.bool_
        if logical:
            a = a.astype(np.uint8)
        a = a.astype(a.dtype.newbyteorder("<"))
        if a.ndim == 0:
            a = a.reshape(1, 1)
        elif a.ndim == 1:
            a = a.reshape(1, -1)
        cls, mi = _MX_OF[np.dtype(a.dtype.str[1:])]
        flags = cls | (0x200 if logical else 0)
        sub = _mat_el(6, np.array([flags, 0], dtype="<u4").tobytes())
        sub += _mat_el(5, np.array(a.shape, dtype="<i4").tobytes())
        sub += _mat_el(_MI_INT8, name.encode("ascii"))
        sub += _mat_el(mi, np.asfortranarray(a).tobytes(order="F"))
        body += _mat_el(_MI_MATRIX, sub)
    head = b"MATLAB 5.0 MAT-file, written by mdfnet tools/data_io.py".ljust(116, b" ") + b"\0" * 8 + \
        np.array([0x0100], dtype="<u2").tobytes() + b"IM"
    with open(path, "wb") as f:
        f.write(head + body)


# --------------------------------------------------------------------------- Tanks and Temples evaluation files
_AXES = "XYZ"


def read_trajectory_log(path):
    """A trajectory .log: per camera a line of three integers (`i i 0`) and the 4 rows of its camera-to-world matrix
    -> poses [n,4,4] float64."""
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    if len(rows) % 5:
        raise ValueError(f"{path}: {len(rows)} non-empty lines, not a multiple of 5")
    poses = []
    for c in range(0, len(rows), 5):
        if len(rows[c]) != 3 or any(len(r) != 4 for r in rows[c + 1:c + 5]):
            raise ValueError(f"{path}: malformed camera block at line {c + 1}")
        poses.append([[float(x) for x in r] for r in rows[c + 1:c + 5]])
    return np.array(poses, dtype=np.float64).reshape(-1, 4, 4)


def write_trajectory_log(path, poses):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    with open(path, "w") as f:
        for i, p in enumerate(poses):
            f.write(f"{i} {i} 0\n")
            for r in p:
                f.write(" ".join(repr(float(x)) for x in r) + "\n")


def read_matrix_txt(path):
    """A 4x4 matrix as text (whitespace-separated, 4 rows) -> [4,4] float64."""
    m = np.loadtxt(path, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError(f"{path}: a 4x4 matrix is expected, got {m.shape}")
    return m


def write_matrix_txt(path, m):
    m = np.asarray(m, dtype=np.float64).reshape(4, 4)
    with open(path, "w") as f:
        for r in m:
            f.write(" ".join(repr(float(x)) for x in r) + "\n")


def crop_uv_axes(axis):
    """The two axes the crop polygon lives on, for an orthogonal axis 0 / 1 / 2: (y, z), (x, z), (x, y)."""
    return (1 if axis == 0 else 0), (1 if axis == 2 else 2)


def read_crop_json(path):
    """A crop volume (.json: orthogonal_axis "X"/"Y"/"Z", axis_min, axis_max, bounding_polygon [[x,y,z], ...]) -> dict with
    axis (0/1/2), axis_min, axis_max, polygon [k,2] (the polygon's coordinates on crop_uv_axes(axis)) and polygon3 [k,3]."""
    import json
    with open(path) as f:
        j = json.load(f)
    axis = _AXES.index(str(j["orthogonal_axis"]).upper())
    poly3 = np.asarray(j["bounding_polygon"], dtype=np.float64).reshape(-1, 3)
    iu, iv = crop_uv_axes(axis)
    return {"axis": axis, "axis_min": float(j["axis_min"]), "axis_max": float(j["axis_max"]),
            "polygon": np.ascontiguousarray(poly3[:, [iu, iv]]), "polygon3": poly3}


def write_crop_json(path, axis, axis_min, axis_max, polygon3):
    import json
    poly3 = np.asarray(polygon3, dtype=np.float64).reshape(-1, 3)
    j = {"axis_max": float(axis_max), "axis_min": float(axis_min), "bounding_polygon": [[float(x) for x in p] for p in poly3],
         "class_name": "SelectionPolygonVolume", "orthogonal_axis": _AXES[int(axis)], "version_major": 1, "version_minor": 0}
    with open(path, "w") as f:
        json.dump(j, f, indent=1)
