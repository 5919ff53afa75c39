"""A small writer of COLMAP sparse models, text and binary, for the scene-import tests (the public file formats)."""
import os
import struct

import numpy as np

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}


def rotation_to_quaternion(rot):
    """[N,3,3] -> unit (qw, qx, qy, qz) [N,4], from the largest of the four candidate components (stable for every rotation)."""
    out = []
    for R in np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3):
        t = [1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]]
        k = int(np.argmax(t))
        r = 2 * np.sqrt(t[k])
        q = [[r / 4, (R[2, 1] - R[1, 2]) / r, (R[0, 2] - R[2, 0]) / r, (R[1, 0] - R[0, 1]) / r],
             [(R[2, 1] - R[1, 2]) / r, r / 4, (R[0, 1] + R[1, 0]) / r, (R[0, 2] + R[2, 0]) / r],
             [(R[0, 2] - R[2, 0]) / r, (R[0, 1] + R[1, 0]) / r, r / 4, (R[1, 2] + R[2, 1]) / r],
             [(R[1, 0] - R[0, 1]) / r, (R[0, 2] + R[2, 0]) / r, (R[1, 2] + R[2, 1]) / r, r / 4]][k]
        out.append(q)
    return np.array(out, dtype=np.float64).reshape(-1, 4)


def write_text(folder, cameras, image_ids, qvec, tvec, camera_ids, names, point_ids, xyz, tracks):
    """cameras {id: (model, w, h, params)}; tracks: per point the list of COLMAP image ids."""
    f = lambda x: repr(float(x))
    with open(os.path.join(folder, "cameras.txt"), "w") as out:
        out.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, (model, w, h, params) in cameras.items():
            out.write(f"{cid} {model} {w} {h} " + " ".join(f(p) for p in params) + "\n")
    with open(os.path.join(folder, "images.txt"), "w") as out:
        out.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                  "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for k, iid in enumerate(image_ids):
            out.write(f"{iid} " + " ".join(f(x) for x in qvec[k]) + " " + " ".join(f(x) for x in tvec[k]) + f" {camera_ids[k]} {names[k]}\n")
            obs = [pid for pid, tr in zip(point_ids, tracks) if iid in tr]
            out.write(" ".join(f"{10.5 + j} {20.25} {pid}" for j, pid in enumerate(obs)) + "\n")     # empty for an unobserved image
    with open(os.path.join(folder, "points3D.txt"), "w") as out:
        out.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, p, tr in zip(point_ids, xyz, tracks):
            out.write(f"{pid} {f(p[0])} {f(p[1])} {f(p[2])} 128 128 128 0.5" + "".join(f" {iid} {j}" for j, iid in enumerate(tr)) + "\n")


def write_binary(folder, cameras, image_ids, qvec, tvec, camera_ids, names, point_ids, xyz, tracks):
    with open(os.path.join(folder, "cameras.bin"), "wb") as out:
        out.write(struct.pack("<Q", len(cameras)))
        for cid, (model, w, h, params) in cameras.items():
            out.write(struct.pack("<iiQQ", cid, MODEL_IDS[model], w, h) + struct.pack("<%dd" % len(params), *params))
    with open(os.path.join(folder, "images.bin"), "wb") as out:
        out.write(struct.pack("<Q", len(image_ids)))
        for k, iid in enumerate(image_ids):
            out.write(struct.pack("<i7di", iid, *[float(x) for x in qvec[k]], *[float(x) for x in tvec[k]], camera_ids[k]))
            out.write(names[k].encode("utf-8") + b"\0")
            obs = [pid for pid, tr in zip(point_ids, tracks) if iid in tr]
            out.write(struct.pack("<Q", len(obs)))
            for j, pid in enumerate(obs):
                out.write(struct.pack("<ddq", 10.5 + j, 20.25, pid))
    with open(os.path.join(folder, "points3D.bin"), "wb") as out:
        out.write(struct.pack("<Q", len(point_ids)))
        for pid, p, tr in zip(point_ids, xyz, tracks):
            out.write(struct.pack("<QdddBBBdQ", pid, float(p[0]), float(p[1]), float(p[2]), 128, 128, 128, 0.5, len(tr)))
            for j, iid in enumerate(tr):
                out.write(struct.pack("<ii", iid, j))
