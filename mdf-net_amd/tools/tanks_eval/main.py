"""Tanks and Temples evaluation: precision, recall and F-score at the scene's distance tau, for the training scenes, which ship
their ground truth (the reference stops at the PLY and points at the benchmark's website).  The protocol is restated in DESIGN
section 7 and runs on the GPU (ops.tanks_eval_scene): initial alignment from the camera centres, crop volume, voxel-grid
downsampling, three rounds of point-to-point ICP, nearest-neighbour distances both ways.

Per scene it reads {ply_path}/{scene}.ply (what tools/pcd/fusion.py writes), the ground truth {data_path}/{scene}/{scene}.ply,
the crop volume {scene}.json, the alignment {scene}_trans.txt and the reference trajectory {scene}_COLMAP_SfM.log next to it,
and the estimate's trajectory: {traj_path}/{scene}.log, or the cameras {cams_path}/{scene}/cams/*_cam.txt in name order
(camera-to-world = the inverse of the extrinsic).  --init FILE gives the initial 4x4 directly ("{scene}" in it is replaced).
It writes {results_path}/{scene}_Eval.npz and reuses one that exists.  Scenes shard over ranks (no collective); after a
barrier rank 0 prints the table and the mean F.

  python mdf-net_amd/tools/tanks_eval/main.py --data_path TANKS/training --ply_path PLY_DIR --cams_path TANKS/training --scenes Barn,Truck
"""
import argparse
import os
import sys
import time

_TOP = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # mdf-net_amd/
if _TOP not in sys.path:
    sys.path.insert(0, _TOP)

import numpy as np  # noqa: E402

SCENES = ["Barn", "Caterpillar", "Church", "Courthouse", "Ignatius", "Meetingroom", "Truck"]
RESULT_FIELDS = ("precision", "recall", "fscore", "tau", "T", "T_init", "stage_T", "stage_fitness", "stage_rmse", "stage_iterations",
                 "hist_est", "hist_gt", "hist_edges", "n_est", "n_gt", "n_crop_A", "n_down_A", "n_crop_B", "n_down_B", "n_crop_C",
                 "n_down_C", "n_est_crop", "n_est_down", "n_gt_crop", "n_gt_down")


def scene_paths(args, scene):
    d = os.path.join(args.data_path, scene)
    return {"est": os.path.join(args.ply_path, f"{scene}.ply"), "gt": os.path.join(d, f"{scene}.ply"),
            "crop": os.path.join(d, f"{scene}.json"), "trans": os.path.join(d, f"{scene}_trans.txt"),
            "ref_traj": os.path.join(d, f"{scene}_COLMAP_SfM.log"),
            "traj": os.path.join(args.traj_path, f"{scene}.log") if args.traj_path else None,
            "cams": os.path.join(args.cams_path, scene, "cams") if args.cams_path else None,
            "init": args.init.replace("{scene}", scene) if args.init else None,
            "result": os.path.join(args.results_path, f"{scene}_Eval.npz")}


def poses_from_cams(folder):
    """Camera-to-world matrices of a cams folder (*_cam.txt, extrinsic on lines 1-4), in name order -> [n,4,4] float64."""
    names = sorted(f for f in os.listdir(folder) if f.endswith("_cam.txt"))
    if not names:
        raise ValueError(f"{folder}: no *_cam.txt files")
    poses = []
    for name in names:
        with open(os.path.join(folder, name)) as f:
            lines = [ln.rstrip() for ln in f.readlines()]
        poses.append(np.linalg.inv(np.array(" ".join(lines[1:5]).split(), dtype=np.float64).reshape(4, 4)))
    return np.stack(poses)


def initial_alignment(p):
    from mdfnet_hip import ops
    from tools.data_io import read_matrix_txt, read_trajectory_log
    if p["init"]:
        return read_matrix_txt(p["init"])
    est = read_trajectory_log(p["traj"]) if p["traj"] else poses_from_cams(p["cams"])
    return ops.tanks_initial_alignment(est, read_trajectory_log(p["ref_traj"]), read_matrix_txt(p["trans"]))


def eval_scene(args, scene, device=None):
    """One scene -> its result file (computed unless it exists)."""
    from mdfnet_hip import ops
    from tools.data_io import read_crop_json, read_ply_vertices
    p = scene_paths(args, scene)
    if os.path.exists(p["result"]):
        print(f"{scene}: reusing {p['result']}")
        return p["result"]
    tau = args.tau if args.tau is not None else ops.TANKS_TAU.get(scene)
    if tau is None:
        raise ValueError(f"{scene}: no tau in the table, give --tau")
    t0 = time.time()
    est, gt = read_ply_vertices(p["est"]), read_ply_vertices(p["gt"])
    crop = read_crop_json(p["crop"])
    init = initial_alignment(p)
    t1 = time.time()
    ev = ops.tanks_eval_scene(est, gt, crop, tau, init, device=device)
    t2 = time.time()
    os.makedirs(os.path.dirname(os.path.abspath(p["result"])), exist_ok=True)
    tmp = p["result"] + ".tmp.npz"
    np.savez(tmp, scene=scene, **{k: ev[k] for k in RESULT_FIELDS})
    os.replace(tmp, p["result"])
    print(f"{scene}: {len(est)} points ({ev['n_est_crop']} cropped, {ev['n_est_down']} compared) against {len(gt)} "
          f"({ev['n_gt_crop']}, {ev['n_gt_down']}), ICP iterations {ev['stage_iterations'].tolist()} "
          f"(read {t1 - t0:.2f}s, evaluate {t2 - t1:.2f}s) -> {p['result']}")
    return p["result"]


def summary(args, scenes):
    """The table and the mean F from the result files -> (rows, mean F)."""
    rows = []
    print(f"{'scene':<12} {'tau':>7} {'precision':>10} {'recall':>10} {'f-score':>10}")
    for scene in scenes:
        with np.load(scene_paths(args, scene)["result"]) as z:
            row = {"scene": scene, "tau": float(z["tau"]), "precision": float(z["precision"]), "recall": float(z["recall"]),
                   "fscore": float(z["fscore"])}
        rows.append(row)
        print(f"{scene:<12} {row['tau']:>7g} {row['precision']:>10.6f} {row['recall']:>10.6f} {row['fscore']:>10.6f}")
    mean_f = float(np.mean([r["fscore"] for r in rows]))
    print(f"mean f-score over {len(rows)} scenes: {mean_f:.6f}")
    return rows, mean_f


def parse(argv=None):
    import config                       # the project's data root (MDF_DATA_ROOT)
    parser = argparse.ArgumentParser(description="Tanks and Temples F-score evaluation (training scenes) on the GPU")
    parser.add_argument("--data_path", default=os.path.join(config.DATA_ROOT, "tanksandtemples", "training"),
                        help="the folder of the scenes' ground truth ({scene}/{scene}.ply, .json, _trans.txt, _COLMAP_SfM.log)")
    parser.add_argument("--ply_path", required=True, help="the estimated clouds, {scene}.ply")
    parser.add_argument("--traj_path", default=None, help="the estimate's trajectories, {scene}.log")
    parser.add_argument("--cams_path", default=None, help="or the cameras the estimate was made with, {scene}/cams/*_cam.txt")
    parser.add_argument("--init", default=None, help="or a 4x4 text matrix as the initial alignment ('{scene}' is replaced)")
    parser.add_argument("--scenes", default=None, help="comma-separated scene names (default: the seven training scenes)")
    parser.add_argument("--tau", type=float, default=None, help="the distance threshold in metres (default: the scene's own)")
    parser.add_argument("--results_path", default=None, help="where the result files go (default: the ply path)")
    args = parser.parse_args(argv)
    if sum(x is not None for x in (args.traj_path, args.cams_path, args.init)) != 1:
        parser.error("give exactly one of --traj_path, --cams_path and --init")
    args.results_path = args.results_path or args.ply_path
    args.scenes = args.scenes.split(",") if args.scenes else list(SCENES)
    return args


def main(argv=None):
    import torch
    from mdfnet_hip import shard
    args = parse(argv)
    rank, world, local = shard.init()
    device = torch.device("cuda", local)
    for i in shard.shard_items(len(args.scenes), rank, world):      # scenes are independent: shard them, no collective
        eval_scene(args, args.scenes[i], device)
    shard.barrier()
    if rank == 0:
        return summary(args, args.scenes)
    return None


if __name__ == "__main__":
    main()
