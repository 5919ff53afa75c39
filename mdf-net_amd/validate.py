"""Validation driver: depth metrics of a checkpoint on the DTU validation scans or BlendedMVS' validation list, per stage of the
cascade and per confidence bin (mdfnet_hip/valmetrics.py) -- the numbers by which --curves / --prob_thresh / --aggregate /
--confidence choices and checkpoints are told apart without a whole eval + fusion + scoring run.

    python mdf-net_amd/validate.py -p pth/dtu_30.pth -d dtu [--confidence cascade] [--out val.json]
    torchrun --nproc-per-node N mdf-net_amd/validate.py ...        (items sharded over the ranks like eval.py)

Data comes from the training loaders (fixed source views: robust_train=False) at the loader's size; the model runs in eval mode on
the eval kernels.  Prints the per-stage table and the confidence table and writes the report as JSON (--out) next to a .txt copy."""
import argparse
import logging
import os

import torch

from mdfnet_hip import shard, valmetrics


def build_parser():
    import config
    parser = argparse.ArgumentParser(description="validation parameter setting")
    parser.add_argument("-p", "--pre_model", default=None, type=str, help="checkpoint ({'epoch', 'model'})")
    parser.add_argument("-d", "--dataset", default="dtu", type=str, choices=["dtu", "blendedmvs"])
    parser.add_argument("--aggregate", default="vector", type=str, choices=list(config.AGGREGATES),
                        help="cost-volume operator the checkpoint was trained with (train.py --aggregate)")
    parser.add_argument("--curves", default="gauss1,laplace", type=str,
                        help="hypothesis curves fitted before stages 1 and 2: two of gauss0, gauss1, laplace, atv")
    parser.add_argument("--prob_thresh", default="0.95,1e-5", type=str, help="their probability thresholds, each inside (0, 1)")
    parser.add_argument("--atv_scale", default="1.5,1.5", type=str,
                        help="scale of the spread for a stage whose curve is atv (UCS-Net's lamb), each finite and > 0")
    parser.add_argument("--confidence", default="last", type=str, choices=list(config.CONFIDENCES),
                        help="which confidence map the confidence table is made of (eval.py --confidence)")
    parser.add_argument("--regular_stride", default="2,2,2", type=str, choices=["2,2,2", "1,2,2"],
                        help="sample stride of the stage-1/2 regularisers the checkpoint was trained with: 2,2,2 (the reference's composition) "
                             "or 1,2,2 (its depth-preserving alternative: H and W are halved, every depth plane is kept)")
    parser.add_argument("--thresholds", default=None, type=str,
                        help="1 to 4 comma-separated error thresholds; default 2,4,8 (mm) for dtu, 1/256,1/128,1/64 of each item's depth "
                             "range for blendedmvs")
    parser.add_argument("--relative", action="store_true",
                        help="the thresholds are fractions of each item's depth_max - depth_min (the default for blendedmvs)")
    parser.add_argument("--out", default=None, type=str, help="report file (JSON; a .txt table is written beside it); default "
                                                              "<output root>/validation_<dataset>.json")
    return parser


def parse_thresholds(text, dataset, relative):
    """-> (thresholds, relative).  No --thresholds: the dataset's defaults (DTU absolute mm, BlendedMVS relative)."""
    if text is None:
        if dataset == "blendedmvs" or relative:
            return tuple(valmetrics.RELATIVE_THRESHOLDS), True
        return tuple(valmetrics.DTU_THRESHOLDS), False
    vals = []
    for p in text.split(","):
        num, _, den = p.strip().partition("/")
        vals.append(float(num) / float(den) if den else float(num))
    if not 1 <= len(vals) <= 4 or any(not v > 0 for v in vals):
        raise ValueError(f"--thresholds {text!r}: 1 to 4 positive values")
    return tuple(vals), bool(relative)


def val_dataset(name, nviews=5):
    """The validation items of a dataset, from the training loader with fixed source views."""
    import config
    if name == "dtu":
        load_args = config.LoadDTU()
        from load.dtutrain import LoadDataset
        return LoadDataset(datasetpath=load_args.train_root, pairpath=load_args.train_pair, scencelist=load_args.val_label,
                           lighting_label=load_args.val_lighting_label, nviews=nviews, robust_train=False)
    load_args = config.LoadBlendedMVS()
    from load.blendedtrain import LoadDataset
    return LoadDataset(datasetpath=load_args.train_root, nviews=nviews, robust_train=False, listfile="validation_list.txt")


def main(argv=None):
    import config
    args = build_parser().parse_args(argv)
    logging.info(args)
    thresholds, relative = parse_thresholds(args.thresholds, args.dataset, args.relative)
    rank, world, local = shard.init()
    eval_args = config.EvalDTU()
    dataset = val_dataset(args.dataset, eval_args.nviews)
    curves, thresh = config.parse_pair(args.curves, str), config.parse_pair(args.prob_thresh, float)
    atv_scale = config.parse_pair(args.atv_scale, float)
    regular_stride = config.parse_stride(args.regular_stride)
    default = args.aggregate == "vector" and curves == tuple(config.curve_calss[1:]) and thresh == tuple(config.prob_thresh[1:]) \
        and args.confidence == "last" and regular_stride == (2, 2, 2)
    model = config.model if default else config.build_model(aggregate=args.aggregate, curves=curves, prob_thresh=thresh, atv_scale=atv_scale,
                                                            confidence=args.confidence, regular_stride=regular_stride)
    if args.pre_model is not None:
        model.load_state_dict(torch.load(args.pre_model, map_location="cpu")["model"])
    device = eval_args.DEVICE
    model.to(device)
    rep, _ = valmetrics.run_validation(model, dataset, device, thresholds, relative, rank, world, eval_args.nworks)
    if rank == 0:
        rep["options"] = {"dataset": args.dataset, "checkpoint": args.pre_model, "aggregate": args.aggregate, "curves": list(curves),
                          "prob_thresh": list(thresh), "atv_scale": list(atv_scale), "confidence": args.confidence}
        text = valmetrics.format_report(rep)
        print(text)
        out = args.out or os.path.join(eval_args.output_path, "validation_{}.json".format(args.dataset))
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(valmetrics.report_json(rep) + "\n")
        with open(os.path.splitext(out)[0] + ".txt", "w") as f:
            f.write(text + "\n")
        logging.info("validation report: %s", out)
    return rep


if __name__ == "__main__":
    main()
