"""CPU: the DTU consensus fusion's semantics on analytic ground truth (tests/consensus_oracle.py, the yardstick of the GPU kernel),
the host camera preparation of ops.consensus_fuse, the PLY layout and the gipuma driver's probability filter and image crop."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import consensus_oracle as CO  # noqa: E402


def plane_z(x, y):
    return 650.0 + 0.15 * x - 0.1 * y


def render_plane(K, E, h, w):
    """Exact depth maps of the world plane z = plane_z(x, y) (float64 ray-plane intersection, rounded to fp32)."""
    nrm = np.array([-0.15, 0.1, 1.0])
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pix = np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
    out = []
    for k, e in zip(np.asarray(K, np.float64), np.asarray(E, np.float64)):
        R, t = e[:3, :3], e[:3, 3]
        ray = np.linalg.inv(k) @ pix
        d = (650.0 + nrm @ R.T @ t) / (nrm @ R.T @ ray)
        out.append(d.reshape(h, w).astype(np.float32))
    return np.stack(out)


def scene(n=5, h=40, w=56, seed=3):
    from oracle.gen_golden import filter_scene
    _, _, K, E = filter_scene(h=h, w=w, nsrc=n - 1, seed=seed)
    depths = render_plane(K, E, h, w)
    rng = np.random.RandomState(seed)
    images = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    return depths, images, K, E


def test_cameras_host_prep_matches_oracle():
    from mdfnet_hip import ops
    _, _, K, E = scene()
    tab, f = ops.consensus_cameras(K, E)
    tab_o, f_o = CO.cameras(K, E)
    assert tab.dtype == np.float32 and tab.shape == (K.shape[0], 32)
    np.testing.assert_array_equal(tab, tab_o)
    assert f == f_o == np.float32(K[0, 0, 0])
    # C is the camera centre: P [C; 1] = 0
    for v in range(K.shape[0]):
        P = tab[v, :12].reshape(3, 4).astype(np.float64)
        assert np.abs(P @ np.append(tab[v, 21:24], 1.0)).max() < 1e-2 * np.abs(P).max()


def test_consistent_views_count_and_surface():
    """On a noise-free plane every view that sees the point agrees: n = k - 1 with k = views that see it, and the fused point
    lies on the plane (up to the pixel truncation of the other views' points)."""
    depths, images, K, E = scene()
    n, h, w = depths.shape
    tab, f = CO.cameras(K, E)
    for r in (0, 3):
        res = CO.fuse_view(r, depths, images, tab, f, 0.25, 0, torch.float32)
        # expected: views whose projection of the exact surface point lands strictly inside (away from the wrapping last row / column)
        d = depths[r].astype(np.float64)
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        Kr, Er = K[r].astype(np.float64), E[r].astype(np.float64)
        cam = (np.linalg.inv(Kr) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])) * d.ravel()
        X = (np.linalg.inv(Er) @ np.vstack([cam, np.ones(h * w)]))[:3]
        seen = np.zeros(h * w, int)
        edge = np.zeros(h * w, bool)
        for v in range(n):
            if v == r:
                continue
            q = K[v].astype(np.float64) @ (E[v].astype(np.float64) @ np.vstack([X, np.ones(h * w)]))[:3]
            px, py = q[0] / q[2], q[1] / q[2]
            inside = (px >= 0) & (px < w - 1) & (py >= 0) & (py < h - 1)
            near = (np.abs(px - (w - 1)) < 1.01) | (np.abs(py - (h - 1)) < 1.01) | (np.abs(px) < 1e-3) | (np.abs(py) < 1e-3)
            seen += inside
            edge |= near
        got = res["n"].numpy().ravel()
        ok = ~edge
        assert ok.sum() > 0.5 * h * w
        np.testing.assert_array_equal(got[ok], seen[ok])
        assert seen[ok].max() >= 2 and (seen[ok] == 0).any()      # the scene has multi-view points and single-view ones
        xyz = res["xyz"].numpy().reshape(-1, 3).astype(np.float64)[ok]
        foot = 650.0 / float(K[0, 0, 0])                          # one pixel at the plane's depth, in mm
        assert np.abs(xyz[:, 2] - plane_z(xyz[:, 0], xyz[:, 1])).max() < 0.5 * foot
        assert res["keep"].numpy().ravel()[ok].all()              # num_consistent 0: every non-zero point is kept


def wrap_scene(h=4, w=8, f=100.0, tx=7.25):
    """Two pinhole cameras, view 1 shifted by tx along x: reference pixel (0, y) at depth 100 lands at pt = (7.25, y) in view 1,
    i.e. in its last column, whose +1 neighbour wraps to column 0."""
    K = np.array([[[f, 0, 0], [0, f, 0], [0, 0, 1]]] * 2, np.float32)
    E = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    E[1, 0, 3] = tx
    depths = np.full((2, h, w), 100.0, np.float32)
    depths[1, :, 0] = 104.0
    images = np.zeros((2, h, w, 3), np.uint8)
    images[0, :, 0] = (10, 20, 30)
    images[1, :, w - 1] = (100, 100, 100)
    images[1, :, 0] = (200, 0, 40)
    return depths, images, K, E


def test_last_column_wraps_to_column_zero():
    depths, images, K, E = wrap_scene()
    tab, f = CO.cameras(K, E)
    res = CO.fuse_view(0, depths, images, tab, f, 0.25, 1, torch.float32)
    # d^ = 0.75 * 100 (column 7) + 0.25 * 104 (column 0, wrapped) = 101: the fused z is (100 + 101) / 2
    assert res["n"][:, 0].tolist() == [1] * 4
    assert res["keep"][1:, 0].all() and not res["keep"][0, 0]      # row 0 lies at world y = 0 exactly: dropped
    assert res["xyz"][:, 0, 2].tolist() == [100.5] * 4
    # colour: (ref texel + 0.75 * col7 + 0.25 * col0) / 2, truncated
    assert res["rgb"][0, 0].tolist() == [int((10 + 75 + 50) / 2), int((20 + 75) / 2), int((30 + 75 + 10) / 2)]
    assert not res["keep"][:, 1:].any()        # every other pixel projects past the right border


def test_zero_depth_pixels_are_not_special():
    """d = 0 lifts a pixel to M_inv (-p4) = the camera centre; nothing else is special about it."""
    depths, images, K, E = scene()
    depths = depths.copy()
    depths[2, 5:9, 7:20] = 0.0
    tab, f = CO.cameras(K, E)
    res = CO.fuse_view(2, depths, images, tab, f, 0.25, 0, torch.float32)
    zero = torch.from_numpy(depths[2] == 0)
    assert (res["n"][zero] == 0).all()                      # no view sees the camera centre at a matching depth
    c = torch.from_numpy(tab[2, 21:24])
    pts = res["xyz"][zero]
    assert torch.allclose(pts, c.expand_as(pts), rtol=0, atol=1e-3 * float(c.abs().max()))
    assert res["keep"][zero].all()                          # num_consistent 0: the centre is emitted (its coordinates are non-zero)
    res1 = CO.fuse_view(2, depths, images, tab, f, 0.25, 1, torch.float32)
    assert not res1["keep"][zero].any()
    # in the wrap scene camera 0 sits at the origin: its d = 0 points are exactly 0 and are dropped even at num_consistent 0
    d2, im2, K2, E2 = wrap_scene()
    d2[0] = 0.0
    t2, f2 = CO.cameras(K2, E2)
    r2 = CO.fuse_view(0, d2, im2, t2, f2, 0.25, 0, torch.float32)
    assert (r2["xyz"] == 0).all() and not r2["keep"].any()


def test_float64_variant_agrees_on_clean_plane():
    depths, images, K, E = scene(n=4, h=24, w=32)
    tab, f = CO.cameras(K, E)
    a = CO.fuse_view(1, depths, images, tab, f, 0.25, 1, torch.float32)
    b = CO.fuse_view(1, depths, images, tab, f, 0.25, 1, torch.float64)
    flips = (a["keep"] != b["keep"])
    assert (b["margin"][flips] < 1e-4).all()
    both = a["keep"] & b["keep"]
    assert both.sum() > 100
    # fp32 cancellation in M_inv (d*x - p4): a few ulp of the coordinates' scale
    scale = float(b["xyz"][both].abs().max())
    assert float((a["xyz"][both].double() - b["xyz"][both]).abs().max()) < 1e-6 * scale


def test_ply_layout(tmp_path):
    from tools.data_io import write_ply, read_ply
    rng = np.random.RandomState(0)
    xyz = rng.randn(37, 3).astype(np.float32)
    rgb = rng.randint(0, 256, (37, 3)).astype(np.uint8)
    p = str(tmp_path / "a.ply")
    write_ply(p, xyz, rgb)
    raw = open(p, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and "element vertex 37" in lines
    assert [l for l in lines if l.startswith("property")] == ["property float x", "property float y", "property float z",
                                                               "property uchar red", "property uchar green", "property uchar blue"]
    assert len(body) == 15 * 37
    rec = np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    np.testing.assert_array_equal(rec["xyz"], xyz)
    np.testing.assert_array_equal(rec["rgb"], rgb)
    a, b = read_ply(p)
    np.testing.assert_array_equal(a, xyz)
    np.testing.assert_array_equal(b, rgb)
    # the filter driver writes through the same function (its bytes are unchanged)
    from tools.filter import dynamic_filter_gpu as filt
    assert filt.write_ply is write_ply


def make_tiny_scan(tmp_path, n=3, h=24, w=40, img_h=30, img_w=48, seed=5):
    """A DTU-layout scan on disk: <data>/dtu1600x1200/scan7/{images,cams}, <eval>/scan7/{depth_est,confidence}."""
    from PIL import Image
    from tools.data_io import save_pfm
    from oracle.gen_golden import filter_scene
    depths, _, K, E = filter_scene(h=h, w=w, nsrc=n - 1, seed=seed)
    rng = np.random.RandomState(seed)
    data = tmp_path / "data" / "dtu1600x1200" / "scan7"
    ev = tmp_path / "eval" / "scan7"
    for d in (data / "images", data / "cams", ev / "depth_est", ev / "confidence"):
        d.mkdir(parents=True)
    probs, imgs = [], []
    for v in range(n):
        prob = rng.rand(h, w).astype(np.float32)
        img = rng.randint(0, 256, (img_h, img_w, 3)).astype(np.uint8)
        save_pfm(str(ev / "depth_est" / "{:08d}.pfm".format(v)), depths[v])
        save_pfm(str(ev / "confidence" / "{:08d}.pfm".format(v)), prob)
        Image.fromarray(img).save(str(data / "images" / "{:08d}.jpg".format(v)), quality=100)
        with open(data / "cams" / "{:08d}_cam.txt".format(v), "w") as fcam:
            fcam.write("extrinsic\n")
            for row in E[v]:
                fcam.write(" ".join(repr(float(x)) for x in row) + "\n")
            fcam.write("\nintrinsic\n")
            for row in K[v]:
                fcam.write(" ".join(repr(float(x)) for x in row) + "\n")
            fcam.write("\n425.0 2.5 192 935.0\n")
        probs.append(prob)
        imgs.append(img)
    return {"root": str(tmp_path / "data"), "eval": str(tmp_path / "eval"), "data": str(data), "ev": str(ev),
            "depths": depths, "probs": np.stack(probs), "K": K, "E": E}


def test_driver_filter_and_crop(tmp_path):
    from PIL import Image
    from tools.gipuma import main as G, conf
    s = make_tiny_scan(tmp_path)
    fa = conf.fusion_args("dtu", "scan7")
    assert fa == {"nviewss": 49, "prob_threshold": 0.6, "check_views": 3, "disp_threshold": 0.25}
    views, depths, images, K, E = G.load_scan(s["data"], s["ev"], fa["nviewss"], fa["prob_threshold"])
    assert views == [0, 1, 2]
    want = s["depths"].copy()
    want[s["probs"] < 0.6] = 0
    np.testing.assert_array_equal(depths, want)
    assert 0 < (depths == 0).sum() < depths.size
    assert images.shape == (3, 24, 40, 3) and images.dtype == np.uint8
    full = np.asarray(Image.open(os.path.join(s["data"], "images", "00000001.jpg")).convert("RGB"))
    np.testing.assert_array_equal(images[1], full[:24, :40])
    np.testing.assert_array_equal(K, s["K"])
    np.testing.assert_array_equal(E, s["E"])
    _, d_raw, _, _, _ = G.load_scan(s["data"], s["ev"], 49, 0.6, prob_filter=False)
    np.testing.assert_array_equal(d_raw, s["depths"])
    with pytest.raises(ValueError, match="smaller"):
        G.read_crop_img(os.path.join(s["data"], "images", "00000000.jpg"), 31, 40)
