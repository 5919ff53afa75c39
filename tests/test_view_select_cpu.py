"""CPU: the host side of the scene import -- the COLMAP model reader (text and binary), the files the importer writes, the
source-view selection rule, the image export (scale, crop to multiples of 32), the scene loader, and the argument errors of the
C ABI that need no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import colmap_writer as W  # noqa: E402
import view_select_oracle as O  # noqa: E402


def _model_args(model="PINHOLE"):
    rot, trans, pts, off, img = O.make_scene(6, 40, 17)
    params = {"PINHOLE": [500.0, 510.0, 320.0, 240.0], "SIMPLE_PINHOLE": [500.0, 320.0, 240.0], "OPENCV": [500.0, 510.0, 320.0, 240.0, 0.1, 0, 0, 0]}
    image_ids = [3, 4, 7, 9, 12, 20]                                   # COLMAP ids are neither dense nor zero-based
    tracks = [[image_ids[i] for i in img[off[p]:off[p + 1]]] for p in range(len(pts))]
    tracks = [[i for i in tr if i != 12] for tr in tracks]            # image 12 has no observations
    names = [f"sub/img {i}.jpg" if i == 7 else f"img{i}.jpg" for i in image_ids]          # a name with a folder and a blank
    return ({5: (model, 640, 480, params[model]), 2: ("SIMPLE_PINHOLE", 320, 240, [250.0, 160.0, 120.0])}, image_ids,
            W.rotation_to_quaternion(rot), trans, [5, 5, 2, 5, 5, 2], names, list(range(100, 100 + len(pts))), pts, tracks)


def test_text_and_binary_models_parse_to_the_same_arrays(tmp_path):
    from tools.colmap import model_io
    args = _model_args()
    (tmp_path / "txt").mkdir()
    (tmp_path / "bin").mkdir()
    W.write_text(str(tmp_path / "txt"), *args)
    W.write_binary(str(tmp_path / "bin"), *args)
    a, b = model_io.read_model(str(tmp_path / "txt")), model_io.read_model(str(tmp_path / "bin"))
    assert a["names"] == b["names"] == args[5]
    for k in ("image_ids", "qvec", "tvec", "camera_ids", "point_ids", "xyz", "track_off", "track_image_ids"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["qvec"], args[2]) and np.array_equal(a["xyz"], args[7])
    for cid in (2, 5):
        assert a["camera_models"][cid][:3] == b["camera_models"][cid][:3]
        assert np.array_equal(a["camera_models"][cid][3], b["camera_models"][cid][3])
    lines = []
    s = model_io.scene_arrays(a, log=lines.append)
    assert len(s["names"]) == 5 and 12 not in s["colmap_ids"] and any("12" in ln and "left out" in ln for ln in lines)
    assert np.allclose(s["rot"] @ s["rot"].transpose(0, 2, 1), np.eye(3), atol=1e-14)
    rot = O.make_scene(6, 40, 17)[0]
    assert np.allclose(s["rot"], rot[[0, 1, 2, 3, 5]], atol=1e-12)
    assert np.array_equal(s["K"][2], [[250, 0, 160], [0, 250, 120], [0, 0, 1]]) and np.array_equal(s["K"][0], [[500, 0, 320], [0, 510, 240], [0, 0, 1]])
    assert s["track_off"][-1] == len(s["track_img"]) and s["track_img"].max() == 4
    assert O.valid_tracks(s["track_off"], s["track_img"], 5).all()


def test_non_finite_points_are_dropped_and_counted(tmp_path):
    from tools.colmap import model_io
    args = list(_model_args())
    args[7] = np.array(args[7])
    args[7][3, 1] = np.nan
    args[7][8, 0] = np.inf
    W.write_binary(str(tmp_path), *args)
    lines = []
    s = model_io.scene_arrays(model_io.read_model(str(tmp_path)), log=lines.append)
    assert len(s["pts"]) == 38 and np.isfinite(s["pts"]).all() and len(s["track_off"]) == 39
    assert any("dropped 2 of 40 points" in ln for ln in lines)


def test_tracks_csr_sorts_and_removes_repeats():
    from tools.colmap import model_io
    off, img = model_io.tracks_csr([2, 0, 2, 2, 0, 2], [5, 1, 3, 5, 0, 4], 4)
    assert off.tolist() == [0, 2, 2, 5, 5] and img.tolist() == [0, 1, 3, 4, 5] and img.dtype == np.int32 and off.dtype == np.int64


def test_other_camera_models_exit_with_the_advice(tmp_path):
    from tools.colmap import model_io
    W.write_text(str(tmp_path), *_model_args("OPENCV"))
    with pytest.raises(SystemExit, match="[Uu]ndistort"):
        model_io.read_model(str(tmp_path))


def test_cam_and_pair_files_read_back(tmp_path):
    from tools import data_io
    from tools.colmap import main as importer
    from tools.colmap.select import select_views
    rot, trans, _, _, _ = O.make_scene(4, 1, 5)
    K = np.array([[512.25, 0, 300.5], [0, 498.75, 201.125], [0, 0, 1]])
    lo, hi = 3.0999999046325684, 7.3000001907348633                   # float32 values: the reader returns float32
    path = str(tmp_path / "00000002_cam.txt")
    importer.write_cam(path, rot[2], trans[2], K, lo, hi)
    k, e, r = data_io.read_cam_file(path, with_range=True)
    assert np.array_equal(k, K.astype(np.float32)) and np.array_equal(r, np.array([lo, hi], dtype=np.float32))
    assert np.array_equal(e[:3, :3], rot[2].astype(np.float32)) and np.array_equal(e[:3, 3], trans[2].astype(np.float32))
    assert np.array_equal(e[3], [0, 0, 0, 1])
    text = open(path).read().split("\n")
    assert [float(x) for x in text[11].split()] == [lo, hi] and float(text[1].split()[0]) == rot[2][0, 0]       # repr round-trips the doubles
    score = np.random.RandomState(0).uniform(0, 9, (4, 4))
    score = score + score.T
    src = select_views(score, 2)
    importer.write_pairs(str(tmp_path / "pair.txt"), score, src)
    n, pairs = data_io.read_pairfile(str(tmp_path / "pair.txt"))
    assert n == 4 and [p[0] for p in pairs] == [0, 1, 2, 3] and [p[1] for p in pairs] == src.tolist()
    rows = open(tmp_path / "pair.txt").read().split("\n")
    assert float(rows[2].split()[2]) == score[0, src[0, 0]]


def test_select_views_tie_rule():
    from tools.colmap.select import select_views
    s = np.array([[0, 2, 5, 2, 0], [2, 0, 1, 1, 1], [5, 1, 0, 0, 0], [2, 1, 0, 0, 0], [0, 1, 0, 0, 0]], dtype=np.float64)
    assert select_views(s, 3).tolist() == [[2, 1, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [1, 0, 2]]
    assert select_views(s, 10).shape == (5, 4)                          # always min(nsrc, N - 1), zero scores included
    assert select_views(s, 10)[2].tolist() == [0, 1, 3, 4]
    assert select_views(np.zeros((1, 1)), 10).shape == (1, 0)
    assert select_views(np.zeros((3, 3)), 1).tolist() == [[1], [0], [0]]


@pytest.mark.parametrize("w,h,max_dim,fmt", [(96, 64, 0, "JPEG"), (100, 70, 0, "JPEG"), (200, 140, 100, "JPEG"), (96, 64, 0, "PNG"),
                                             (256, 128, 128, "JPEG")])
def test_export_crops_to_multiples_of_32_and_scales_K(tmp_path, w, h, max_dim, fmt):
    from PIL import Image
    from tools.colmap import main as importer
    src, dst = str(tmp_path / ("in." + fmt.lower())), str(tmp_path / "out.jpg")
    Image.fromarray(np.random.RandomState(1).randint(0, 255, (h, w, 3)).astype(np.uint8)).save(src, format=fmt)
    K = np.array([[120.0, 0, w / 2], [0, 118.0, h / 2], [0, 0, 1]])
    K2, size = importer.export_image(src, dst, K, max_dim)
    with Image.open(dst) as im:
        assert im.size == size and im.format == "JPEG" and size[0] % 32 == 0 and size[1] % 32 == 0
    if max_dim and max(w, h) > max_dim:
        s = max_dim / max(w, h)
        assert np.array_equal(K2[:2], K[:2] * s) and np.array_equal(K2[2], [0, 0, 1])
        assert size == (int(round(w * s)) // 32 * 32, int(round(h * s)) // 32 * 32)
    else:
        assert np.array_equal(K2, K)                                    # cropping at the bottom and right leaves K unchanged
        assert size == (w // 32 * 32, h // 32 * 32)
        same = open(src, "rb").read() == open(dst, "rb").read()
        assert same == (fmt == "JPEG" and w % 32 == 0 and h % 32 == 0)  # nothing to do: copied byte for byte


def _write_scene(root, name, n=4, w=96, h=64):
    from PIL import Image
    from tools.colmap import main as importer
    from tools.colmap.select import select_views
    rot, trans, _, _, _ = O.make_scene(n, 1, 9)
    os.makedirs(os.path.join(root, name, "images"))
    os.makedirs(os.path.join(root, name, "cams"))
    rng = np.random.RandomState(2)
    for i in range(n):
        Image.fromarray(rng.randint(0, 255, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, name, "images", "%08d.jpg" % i))
        importer.write_cam(os.path.join(root, name, "cams", "%08d_cam.txt" % i), rot[i], trans[i],
                           [[130.0, 0, w / 2], [0, 130.0, h / 2], [0, 0, 1]], 3.5 + i, 6.5 + i)
    score = rng.uniform(1, 2, (n, n))
    importer.write_pairs(os.path.join(root, name, "pair.txt"), score + score.T, select_views(score + score.T, 3))


def test_scene_loader_yields_the_tanks_loaders_items(tmp_path):
    from load.sceneeval import LoadDataset
    from load.getpath import get_img_path, get_cam_path
    _write_scene(str(tmp_path), "a")
    _write_scene(str(tmp_path), "b", n=3)
    assert get_img_path("R", "a", 3, mode="scene") == os.path.join("R", "a", "images", "00000003.jpg")
    assert get_cam_path("R", "a", 3, mode="scene") == os.path.join("R", "a", "cams", "00000003_cam.txt")
    data = LoadDataset(str(tmp_path), ["a", "b"], nviews=3)
    assert len(data) == 7
    item = data[1]
    assert sorted(item) == ["depth_range", "extrinsics", "filename", "imgs", "intrinsics", "scan", "view_ids"]
    assert item["imgs"].shape == (3, 3, 64, 96) and item["imgs"].dtype == np.float32
    assert item["intrinsics"].shape == (3, 3, 3) and item["extrinsics"].shape == (3, 4, 4)
    assert item["depth_range"].tolist() == [4.5, 7.5] and item["view_ids"][0] == 1 and item["view_ids"].dtype == np.int64
    assert item["scan"] == "a" and item["filename"].format("depth_est", ".pfm") == "a/depth_est/00000001.pfm"
    assert data[5]["imgs"].shape == (3, 3, 64, 96) and data[5]["scan"] == "b"          # 3 images: the reference and both others


def test_config_knows_the_scene_dataset():
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        import config
        a = config.LoadScene("/data/scenes", ["x", "y"])
    assert a.eval_root == "/data/scenes" and a.scenelist == ["x", "y"]
    assert config.LoadScene().eval_root == os.path.join(config.DATA_ROOT, "scenes") and config.LoadScene().scenelist == []


def test_abi_argument_errors_without_gpu():
    """Argument errors come back as -1 with a message and launch nothing (no GPU is needed to see them)."""
    import mdfnet_hip
    l = mdfnet_hip.lib()
    P = ctypes.c_void_p
    ptr = P(256)                                                       # never dereferenced: every check below fails first
    d = ctypes.c_double

    def ranges(rot=ptr, q=(0.01, 0.99), ws=ptr, ws_bytes=1 << 40, status=ptr):
        return l.mdf_view_depth_ranges(rot, ptr, 3, ptr, 10, ptr, ptr, 20, d(q[0]), d(q[1]), ws, ws_bytes, ptr, ptr, status, None)

    def scores(trans=ptr, theta0=5.0, s1=1.0, s2=10.0, ws=ptr, ws_bytes=1 << 40, n_rec=15, score=ptr):
        return l.mdf_view_scores(ptr, trans, 3, ptr, 10, ptr, ptr, 20, n_rec, d(theta0), d(s1), d(s2), ws, ws_bytes, score, ptr, ptr, None)

    assert ranges(rot=None) == -1 and b"null" in l.mdf_last_error()
    assert ranges(status=None) == -1 and b"null" in l.mdf_last_error()
    assert ranges(ws=None) == -1 and b"null" in l.mdf_last_error()
    assert scores(trans=None) == -1 and b"null" in l.mdf_last_error()
    assert scores(score=None) == -1 and b"null" in l.mdf_last_error()
    for q in ((0.6, 0.4), (-0.1, 0.5), (0.5, 1.5), (float("nan"), 0.5)):
        assert ranges(q=q) == -1 and b"quantiles" in l.mdf_last_error()
    for s1, s2 in ((0.0, 10.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        assert scores(s1=s1, s2=s2) == -1 and b"sigma" in l.mdf_last_error()
    assert scores(theta0=float("inf")) == -1 and b"theta0" in l.mdf_last_error()
    need = l.mdf_view_workspace(3, 10, 20, 15)
    assert need > 0 and need % 16 == 0 and l.mdf_view_workspace(3, 10, 20, 0) <= need
    assert ranges(ws_bytes=64) == -1 and b"too small" in l.mdf_last_error()
    assert scores(ws_bytes=need - 16) == -1 and b"too small" in l.mdf_last_error()
    assert ranges(ws=P(264)) == -1 and b"aligned" in l.mdf_last_error()
    # beyond the sort's limit: unsupported, and the message names the record count
    big = (1 << 31) - 4096
    assert scores(n_rec=big) == -2 and str(big).encode() in l.mdf_last_error()
    assert l.mdf_view_workspace(3, 10, 20, big) == 0 and l.mdf_view_workspace(40000, 10, 20, 15) == 0 and l.mdf_view_workspace(-1, 0, 0, 0) == 0


def test_ops_refuse_cpu_tensors():
    import torch
    from mdfnet_hip import ops
    s = [torch.from_numpy(np.array(a)) for a in O.make_scene(3, 10, 1)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_scores(*s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_depth_ranges(*s)


def test_oracle_runs_in_both_precisions_and_ranking_seeds_hold():
    """The condition of the GPU ranking test, checked where the seeds were chosen: the oracle's smallest relative gap between
    compared ranks is far above 1e-9 on the small ring scene, and the float64 oracle sits within 1e-12 of the longdouble one."""
    from tools.colmap.select import select_views
    s = O.make_scene(9, 300, 5)
    a, sh = O.scores(*s, dtype=np.float64)
    b, _ = O.scores(*s, dtype=np.longdouble)
    assert a.dtype == np.float64 and b.dtype == np.longdouble and int(np.triu(sh, 1).sum()) == O.n_records(s[3])
    pos = b > 0
    assert float(np.max(np.abs(a[pos] - b[pos]) / b[pos])) < 1e-12
    assert O.rank_gap(a, select_views(a, 4)) >= 1e-9
    rng, cnt, _ = O.depth_ranges(*s)
    assert cnt.sum() == len(s[4]) and (rng[:, 0] <= rng[:, 1]).all()
