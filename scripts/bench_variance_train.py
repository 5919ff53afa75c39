"""Training of the variance cost-volume slot at the three cfg3 stage shapes (768x576, 5 views, batch 1), HIP-event timed:
  (a) homo_aggregate_by_variance forward + backward on the hand-written kernels (mdf_warp_aggregate_var_fwd / _bwd),
  (b) the same slot through stock PyTorch-ROCm autograd (rehearsal.mode(on_gpu=True)),
  (c) VectorAggregate's training forward + backward at the same shape,
alternating in one process, every variant warmed up and timed for >= MDF_BENCH_SECONDS (default 1 s) in rounds whose spread is
printed; achieved bytes/s against the algorithmic bytes of the `work=` tags.  Then (MDF_BENCH_STEP=1, default) the cfg3 training
step of the variance model next to the vector model's, eager and recorded.  dev tool"""
import contextlib, io, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, R + '/mdf-net_amd']
import torch
import rehearsal
from mdfnet_hip import ddp, synth
from net.unit.homoaggregate import VectorAggregate, homo_aggregate_by_variance
from net.unit.scale import scale_cam
dev = torch.device('cuda', 0)
torch.manual_seed(0)
W, H, V = (int(x) for x in os.environ.get("MDF_SHAPE", "768,576,5").split(","))
SECONDS = float(os.environ.get("MDF_BENCH_SECONDS", "1.0"))
ROUNDS = 5


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


intr, extr, dr = synth.make_cameras(W, H, V, batch=1, rot_deg=float(os.environ.get("MDF_ROT", "3.0")), seed=101)
for stage, (c, g, d) in enumerate(((64, 32, 48), (32, 16, 24), (16, 8, 8))):
    h, w = H >> (3 - stage), W >> (3 - stage)
    rp, sps = scale_cam(intr, extr, stage)
    rp, sps = rp.to(dev), tuple(s.to(dev) for s in sps)
    feats = [torch.randn(1, c, h, w, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for _ in range(V)]
    if stage == 0:
        hyp = torch.linspace(425, 935, d, device=dev).reshape(1, d, 1, 1)
    else:
        span = 40.0 if stage == 1 else 6.0      # per-pixel hypotheses around a smooth depth map, as the cascade produces
        base = 600 + 80 * torch.sin(torch.linspace(0, 6, w, device=dev)).reshape(1, 1, 1, w) + torch.zeros(1, 1, h, w, device=dev)
        hyp = (base + torch.linspace(-span, span, d, device=dev).reshape(1, d, 1, 1)).contiguous()
    vec = VectorAggregate(g).train().to(dev)
    dvar = torch.randn(1, d, h, w, c, device=dev).permute(0, 4, 1, 2, 3)       # NDHWC memory, as the regulariser hands it back
    dvec = torch.randn(1, d, h, w, g, device=dev).permute(0, 4, 1, 2, 3)

    def run_hip():
        homo_aggregate_by_variance(feats, rp, sps, hyp).backward(dvar)

    def run_stock():
        with rehearsal.mode(on_gpu=True):
            homo_aggregate_by_variance(feats, rp, sps, hyp).backward(dvar)

    def run_vec():
        vec(feats, rp, sps, hyp).backward(dvec)

    variants = (("a: variance, HIP kernels", run_hip), ("b: variance, stock autograd", run_stock), ("c: VectorAggregate, HIP kernels", run_vec))
    reps, times = {}, {k: [] for k, _ in variants}
    for name, fn in variants:                                    # warm-up, and how many calls make a round of SECONDS / ROUNDS
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(3, int(SECONDS / ROUNDS / max(timed(fn, 3) * 1e-3, 1e-6)) + 1)
    for _ in range(ROUNDS):                                      # alternating
        for name, fn in variants:
            times[name].append(timed(fn, reps[name]))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    # algorithmic bytes, forward + backward: features once + cost once | features and their gradients once + d cost once
    by_var = 4.0 * ((V * c * h * w + c * d * h * w) + (2 * V * c * h * w + c * d * h * w))
    by_vec = 4.0 * ((V * c * h * w + g * d * h * w) + (2 * V * c * h * w + g * d * h * w))
    print(f"stage {stage} C{c} D{d} {w}x{h} V{V}:", flush=True)
    for name, _ in variants:
        by = by_vec if name.startswith("c") else by_var
        print(f"   {name:34s} {med[name] * 1e3:9.1f} us  (min {min(times[name]) * 1e3:.1f}, max {max(times[name]) * 1e3:.1f} over {ROUNDS} rounds of "
              f"{reps[name]} calls)  {by / med[name] / 1e6:7.0f} GB/s of algorithmic bytes", flush=True)
    ka, kb, kc = (n for n, _ in variants)
    print(f"   b / a = {med[kb] / med[ka]:.1f} x   a / c = {med[ka] / med[kc]:.2f}", flush=True)
    for f in feats:
        f.grad = None

if os.environ.get("MDF_BENCH_STEP", "1") == "1":
    from mdfnet_hip.graphstep import GraphedTrainStep
    from mdfnet_hip.optim import FlatAdam
    from net import loss as loss_mod
    with contextlib.redirect_stdout(io.StringIO()):
        import config
    crit = loss_mod.Loss().to(dev)
    imgs, extr, intr, dr = (t.to(dev) for t in synth.make_scene(W, H, V, batch=1, rot_deg=2.0, seed=3))
    gt = {str(k): (torch.rand(1, H >> k, W >> k, device=dev) * 400 + 480) for k in (3, 2, 1, 0)}
    steps = {}
    for kind in ("vector", "variance"):
        with contextlib.redirect_stdout(io.StringIO()):
            model = config.build_model(aggregate=kind)
        model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=1))
        model.train().to(dev)
        bucket = ddp.FlatBucket(model)
        opt = FlatAdam(bucket, lr=1e-3)

        def eager():
            out = model(imgs, extr, intr, dr)
            loss = crit(out, gt, dr)
            bucket.zero_grad(); loss.backward(); bucket.allreduce_gradients(); opt.step()
            return loss.detach()
        steps[kind] = [eager, None]
        for _ in range(3):
            eager()
        gstep = GraphedTrainStep(model, crit, bucket, opt, (imgs, extr, intr, dr, gt), warmup=1)
        steps[kind][1] = lambda gstep=gstep: gstep(imgs, extr, intr, dr, gt)
        for _ in range(3):
            steps[kind][1]()
        torch.cuda.synchronize()
    res = {(k, i): [] for k in steps for i in (0, 1)}
    n = int(os.environ.get("MDF_TRAIN_STEPS", "10"))
    for _ in range(3):                                          # alternating rounds, host clock around a device synchronise
        for kind in steps:
            for i in (0, 1):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(n):
                    l = steps[kind][i]()
                torch.cuda.synchronize()
                res[(kind, i)].append((time.perf_counter() - t0) / n)
    for (kind, i), v in res.items():
        print(f"train step {W}x{H}x{V} B=1, {kind:8s} model, {'recorded' if i else 'eager   '}: {sorted(v)[1] * 1e3:7.2f} ms "
              f"(min {min(v) * 1e3:.2f}, max {max(v) * 1e3:.2f} over 3 rounds of {n})", flush=True)
