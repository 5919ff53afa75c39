"""Meshing (ops.tsdf_integrate, ops.tsdf_mesh, ops.mesh_colour: csrc/tsdf_mesh.hip) on a synthetic scan: a sphere in a cubic volume of
--resolution lattice points a side (512, then 256), seen by --views (49) pinhole cameras of --width x --height (1600 x 1184) on a
spiral around it; analytic depth maps with a zero background and random images, both made on the GPU.

Per C-ABI entry (HIP events around the entry itself, ops.profile_begin / profile_end; the median of --repeats after one warm-up)
the time, the algorithmic bytes and their share of the HBM rate a float4 copy reaches on this chip (6.29 TB/s):
  mdf_tsdf_integrate  tsdf_integrate_kernel, ceil(views / 16) launches.  Volume bytes: 8 B per lattice point read and 8 B written by
                      every launch.  Texel bytes: 4 B per (point, view) whose projection lands on the map and whose brick was not
                      culled; the script reports the upper bound (every point and view) and, from the sum of W, the updates made.
                      Timed with the brick culling on (default) and off (MDF_TSDF_CULL=0, read per call).
  mdf_mesh_count      a memset of the edge marks (8 B a point), mesh_count_kernel (D and W of 8 corners: 8 B a point once, the
                      rest cache hits; 1 B written), mesh_scan_kernel x 3 (8 + 1 read, 1 written; the chunk sums; 2 read, 8 written).
  mdf_mesh_emit       mesh_emit_kernel: 2 B a point read, 12 B per vertex and per triangle written.
  mdf_mesh_colour     mesh_colour_kernel: 12 B per vertex read, 3 written, 16 B of sums read and written per launch, and per view
                      that sees the vertex a depth texel and an image texel (7 B).
Nothing was measured before these kernels existed, so there is no pass bar.
  python scripts/bench_tsdf_mesh.py [--resolution 512,256] [--views 49] [--repeats 3] [--out profiles/tsdf_mesh_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mdf-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_COPY_BYTES_PER_S = 6.29e12      # float4 copy on an MI355X (8.0e12 is the specification)
RADIUS, HALF = 0.8, 1.3


def make_scene(views, h, w, dev):
    """Cameras on a spiral of radius 3 around the origin, looking at it; analytic sphere depth, zero background; random images."""
    import numpy as np
    import torch
    Ks, Es, depths = [], [], []
    f = 0.45 * min(h, w) / math.tan(math.asin(RADIUS / 3.0))
    v, u = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
    for n in range(views):
        el = math.asin(-0.9 + 1.8 * (n + 0.5) / views)
        az = 2.399963 * n
        c = 3.0 * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, -R @ c
        K = np.array([[f, 0, (w - 1) / 2 + 0.3], [0, f, (h - 1) / 2 - 0.2], [0, 0, 1]])
        Ks.append(K.astype(np.float32))
        Es.append(E.astype(np.float32))
        K64, E64 = Ks[-1].astype(np.float64), Es[-1].astype(np.float64)
        cam = torch.stack([(u - K64[0, 2]) / K64[0, 0], (v - K64[1, 2]) / K64[1, 1], torch.ones_like(u)], -1)
        dirs = cam @ torch.from_numpy(E64[:3, :3]).to(dev)
        oc = torch.from_numpy(-E64[:3, :3].T @ E64[:3, 3]).to(dev)
        a = (dirs * dirs).sum(-1)
        b = 2.0 * (dirs @ oc)
        disc = b * b - 4 * a * (oc @ oc - RADIUS * RADIUS)
        s = (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a)
        depths.append(torch.where((disc > 0) & (s > 0), s, torch.zeros_like(s)).float())
    g = torch.Generator(device=dev).manual_seed(5)
    images = torch.randint(0, 256, (views, h, w, 3), device=dev, dtype=torch.uint8, generator=g)
    return torch.stack(depths), images, np.stack(Ks), np.stack(Es)


def run(a):
    import numpy as np
    import torch
    from mdfnet_hip import ops
    dev = torch.device("cuda", 0)
    depths, images, K, E = make_scene(a.views, a.height, a.width, dev)
    launches = -(-a.views // ops.TSDF_CHUNK)
    out = {"views": a.views, "map": f"{a.width}x{a.height}", "repeats": a.repeats, "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S,
           "resolutions": {}}
    for res in a.resolution:
        dims = (res, res, res)
        voxel = np.float32(2 * HALF / (res - 1))
        origin = np.full(3, -HALF, np.float32)
        tau = np.float32(3.0) * voxel
        n = res ** 3
        recs = {}

        def once(cull):
            os.environ["MDF_TSDF_CULL"] = "1" if cull else "0"
            ops.profile_begin()
            D, W = ops.tsdf_integrate(depths, K, E, origin, voxel, dims, tau)
            t_int = ops.profile_end()
            os.environ.pop("MDF_TSDF_CULL")
            if not cull:
                return D, W, t_int, None, None, None
            ops.profile_begin()
            vtx, tri = ops.tsdf_mesh(D, W, origin, voxel)
            rgb = ops.mesh_colour(vtx, depths, images, K, E, tau)
            return D, W, t_int, ops.profile_end(), vtx, tri

        ref = None
        for rep in range(a.repeats + 1):                      # the first pass is the warm-up
            for cull in (True, False):
                D, W, t_int, t_rest, vtx, tri = once(cull)
                if ref is None:
                    ref = (D.clone(), W.clone())
                elif rep == 0:
                    assert torch.equal(D, ref[0]) and torch.equal(W, ref[1]), "culling changed the volume"
                if rep:
                    recs.setdefault("mdf_tsdf_integrate" + ("" if cull else " (MDF_TSDF_CULL=0)"), []).append(t_int[0][2])
                    for name, _, ms, _ in (t_rest or []):
                        recs.setdefault(name, []).append(ms)
                if cull:
                    nv, nt, updates = int(vtx.shape[0]), int(tri.shape[0]), float(W.sum())
                    seen = float((W > 0).sum())
                del D, W
        colour_launches = launches
        algo = {"mdf_tsdf_integrate": 16.0 * n * launches + 4.0 * updates,
                "mdf_tsdf_integrate (MDF_TSDF_CULL=0)": 16.0 * n * launches + 4.0 * updates,
                "mdf_mesh_count": (8.0 + 8.0 + 1.0 + 9.0 + 1.0 + 2.0 + 8.0) * n,
                "mdf_mesh_emit": 2.0 * n + 12.0 * nv + 12.0 * nt,
                "mdf_mesh_colour": (15.0 + 32.0 * colour_launches) * nv}
        rows = {}
        for name, ms in recs.items():
            med = statistics.median(ms)
            rows[name] = {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                          "algorithmic_bytes": algo[name], "bytes_per_s": algo[name] / (med * 1e-3),
                          "share_of_hbm_copy_rate": algo[name] / (med * 1e-3) / HBM_COPY_BYTES_PER_S}
            print(f"{res}^3 {name:40s} {med:9.3f} ms  {algo[name] / 1e9:8.3f} GB  {100 * rows[name]['share_of_hbm_copy_rate']:5.1f} % of the copy rate",
                  flush=True)
        out["resolutions"][str(res)] = {"lattice_points": n, "voxel": float(voxel), "integrate_launches": launches, "vertices": nv,
                                        "triangles": nt, "observed_points": seen, "updates_sum_W": updates,
                                        "texel_bytes_upper_bound": 4.0 * n * a.views, "entries": rows}
        del ref
        torch.cuda.empty_cache()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=lambda s: [int(x) for x in s.split(",")], default=[512, 256])
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1184)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_mesh_bench.json"))
    run(ap.parse_args())


if __name__ == "__main__":
    main()
