"""Aggregation kernels at the three cfg2 stage shapes (and cfg4's), HIP-event timed, synthetic DTU-like cameras.
Times the full-feature entry (ops.warp_aggregate_vec) and the pair-difference entry (ops.warp_aggregate_pairdiff) on the same scene.
MDF_WARP_WINDOW=0|1 selects the plain / LDS-window kernel, MDF_PAIRDIFF_GPL=4|8 the groups per lane of the pair-difference kernel
(both read per call).  dev tool"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, R + '/mdf-net_amd']
import torch
from mdfnet_hip import ops, synth
from net.unit.scale import scale_cam
dev = torch.device('cuda', 0)
torch.manual_seed(0)
W, H, V = (int(x) for x in os.environ.get("MDF_SHAPE", "1600,1184,5").split(","))
intr, extr, dr = synth.make_cameras(W, H, V, batch=1, rot_deg=float(os.environ.get("MDF_ROT", "3.0")), seed=101)
tot = {}
for stage, (c, g, d) in enumerate(((64, 32, 48), (32, 16, 24), (16, 8, 8))):
    h, w = H >> (3 - stage), W >> (3 - stage)
    rp, sps = scale_cam(intr, extr, stage)
    proj = ops.relative_projections(rp, list(sps)).to(dev)
    feats = [torch.randn(1, c, h, w, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(V)]
    if stage == 0:
        hyp = torch.linspace(425, 935, d, device=dev).reshape(1, d, 1, 1)
    else:
        span = 40.0 if stage == 1 else 6.0      # per-pixel hypotheses around a smooth depth map, as the cascade produces
        base = 600 + 80 * torch.sin(torch.linspace(0, 6, w, device=dev)).reshape(1, 1, 1, w) + torch.zeros(1, 1, h, w, device=dev)
        hyp = (base + torch.linspace(-span, span, d, device=dev).reshape(1, d, 1, 1)).contiguous()
    wpar = torch.randn(g + 4, device=dev)
    diffs = [(f[:, 1::2] - f[:, 0::2]).contiguous(memory_format=torch.channels_last) for f in feats]
    for name, run, chans in (("vec", lambda: ops.warp_aggregate_vec(feats, proj, hyp, wpar, g), c),
                             ("pairdiff", lambda: ops.warp_aggregate_pairdiff(diffs, proj, hyp, wpar), g)):
        for _ in range(3):
            cost = run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20
        e0.record()
        for _ in range(n):
            cost = run()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        by = 4.0 * (V * chans * h * w + hyp.numel() + g * d * h * w)
        tot[name] = tot.get(name, 0.0) + ms
        print(f"stage {stage} {name:8s} C{c} G{g} D{d} {w}x{h}: {ms*1e3:8.1f} us  {by/ms/1e6:7.0f} GB/s  checksum {float(cost.double().sum()):.6f}", flush=True)
print("total per view: " + ", ".join(f"{k} {v*1e3:.1f} us" for k, v in tot.items())
      + f" (window={os.environ.get('MDF_WARP_WINDOW', '0')}, pairdiff groups per lane={os.environ.get('MDF_PAIRDIFF_GPL', 'per stage')})")
