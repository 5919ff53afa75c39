"""Generate tests/golden/*.npz from the REAL reference (build container only).

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden.py

Imports the reference's python modules from /root/reference (read-only mount; never
copied), loads the deterministic weights of mdfnet_hip.synth.seeded_state_dict into the
reference's `config.model`, runs reference operators / the full model on seeded
synthetic inputs and stores inputs that cannot be regenerated + all expected outputs.
The fixtures are data only; /root/reference does not exist on the GPU box.
"""
import io
import os
import sys
import contextlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MDF_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "mdf-net_amd"))
from mdfnet_hip import synth  # noqa: E402

OUT = os.environ.get("MDF_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))


def load_reference():
    cwd = os.getcwd()
    os.chdir("/tmp")  # reference Args classes makedirs('pth') relative to cwd; keep the repo clean
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import config as ref_config  # builds config.model (config.py:186-218)
    from net.unit import base, homoaggregate, regress, depthhypos, scale  # noqa
    from net import loss as ref_loss
    os.chdir(cwd)
    sys.path.remove(REF)
    return ref_config, base, homoaggregate, regress, depthhypos, scale, ref_loss


def npy(t):
    return t.detach().cpu().numpy()


class HostValueRecorder:
    """Records, while the REAL reference runs, the host-dependent control-plane values it computes through LAPACK/BLAS
    (SURVEY H2/H3): every `torch.matmul` result whose operands are the 4x4 projection pair of base.py:98, the camera product
    of scale.py:16 and the fit matrix of depthhypos.py:206-208.  Stored next to the e2e goldens so that a test can hand the
    product the build host's own values and compare with the golden depth at the metric's 1e-3 bar on any other host."""

    def __enter__(self):
        self.orig = torch.matmul
        self.calls = []

        def wrapped(a, b, *args, **kw):
            r = self.orig(a, b, *args, **kw)
            self.calls.append((tuple(a.shape), tuple(b.shape), r.detach().clone()))
            return r
        torch.matmul = wrapped
        return self

    def __exit__(self, *exc):
        torch.matmul = self.orig

    def values(self, nviews):
        out = {}
        proj = [r for sa, sb, r in self.calls if len(sa) == 3 and sa[1:] == (4, 4) and sb == sa]          # base.py:98
        assert len(proj) == 3 * (nviews - 1), len(proj)
        for st in range(3):
            rows = proj[st * (nviews - 1):(st + 1) * (nviews - 1)]
            out[f"host_proj{st}"] = npy(torch.stack([r[:, :3, :4].reshape(-1, 12) for r in rows]))       # [n_src,B,12]
        cams = [r for sa, sb, r in self.calls if len(sa) == 4 and sa[2:] == (3, 3) and sb[2:] == (3, 4)]  # scale.py:16
        assert len(cams) == 3, len(cams)
        for st in range(3):
            out[f"host_cam{st}"] = npy(cams[st])                                                          # [B,V,3,4]
        fit = [r for sa, sb, r in self.calls if len(sa) == 5 and sa[3:] == (3, 3) and len(sb) == 5 and sb[3] == 3]   # depthhypos.py:208
        assert len(fit) == 1, len(fit)
        assert bool((fit[0] == fit[0][:, :1, :1]).all())           # shared hypotheses: every pixel's matrix is the same
        out["host_fit_row"] = npy(fit[0][:, 0, 0, 0, :])           # [B,D]
        return out


def gen_train(model, sd, ref_loss):
    """Training-mode golden: one forward + Loss + backward of the real reference at 96x64x3, batch 2 (train.py:36-45).  The
    host-side control-plane values of the run (projection products, camera products, the gauss-fit row, the log thresholds)
    are recorded like for the e2e goldens, so that the GPU test can be given the build host's own LAPACK/BLAS results and be
    held to the eval leg's bars."""
    model.train()
    model.load_state_dict(sd)
    model.zero_grad()
    imgs, extr, intr, dr = synth.make_scene(96, 64, 3, batch=2, rot_deg=3.0, seed=31)
    rng = np.random.RandomState(7)
    gt = {k: torch.from_numpy((425 + 510 * rng.rand(2, 64 // s, 96 // s)).astype(np.float32))
          for k, s in (("3", 8), ("2", 4), ("1", 2), ("0", 1))}
    gt["3"][:, :2] = 0.0  # masked-out region (gt <= depth_min)
    with HostValueRecorder() as rec:
        out = model(imgs, extr, intr, dr)
    loss = ref_loss.Loss()(out, gt, dr)
    loss.backward()
    tg = {"loss": npy(loss)}
    tg.update(rec.values(3))
    for st in (1, 2):
        tg[f"host_log_thresh{st}"] = npy(torch.log(model.Depth_hypos[st].prob_thresh))
    for i, d in enumerate(out["depth"]):
        tg[f"depth{i}"] = npy(d)
    params = dict(model.named_parameters())
    for k in TRAIN_GRAD_KEYS:
        tg["grad:" + k] = npy(params[k].grad)
    for k in gt:
        tg["gt" + k] = npy(gt[k])
    np.savez_compressed(os.path.join(OUT, "train_tiny.npz"), **tg)
    print("train loss", float(loss))


TRAIN_GRAD_KEYS = ("Backbone.conv01.0.conv.weight", "Homoaggre.0.depth_weight.0.conv.weight", "Homoaggre.2.depth_weight.1.bias",
                   "Regular.2.prob.weight", "Regular.0.conv01.0.conv.weight", "Refine.conv2.2.weight")


def train_f64(sd32, gt):
    """The training golden's step (same inputs, same weights) through the ORACLE in float64 (oracle.mvs_oracle.precision): loss,
    the four depth maps and every parameter gradient.  The yardstick of the training-parity tests -- an fp32 implementation is judged
    by its distance from THIS relative to the reference's own fp32 distance from it -- not a parity target: the
    reference never computes in float64.  -> (loss, [depth], {name: grad}) as float64 numpy."""
    sys.path.insert(0, ROOT)
    from oracle import mvs_oracle as O
    dt = torch.float64
    imgs, extr, intr, dr = synth.make_scene(96, 64, 3, batch=2, rot_deg=3.0, seed=31)
    sd = {k: (v.to(dt).clone().requires_grad_(True) if v.dtype == torch.float32 and "running" not in k
              else (v.to(dt) if v.dtype == torch.float32 else v.clone())) for k, v in sd32.items()}
    with O.precision(dt):
        out = O.core_forward(sd, imgs.to(dt), extr.to(dt), intr.to(dt), dr.to(dt), training=True)
        loss = O.mvs_loss(out["depth"], {k: torch.as_tensor(v).to(dt) for k, v in gt.items()}, dr.to(dt))
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in sd.items() if getattr(v, "grad", None) is not None}
    return float(loss), [d.detach().numpy() for d in out["depth"]], grads


def one_ulp(shape):
    """A factor 1 +- 2^-23 per element (random sign, torch's global generator): multiplying an fp32 tensor by it moves every element
    by one unit in the last place -- the perturbation model of `fp32_spread` and of the per-operator tests."""
    return 1.0 + (torch.randint(0, 2, tuple(shape)).float() * 2 - 1) * 2.0 ** -23


def fp32_spread(sd32, gt, depths64, grads64, draws=6, metric="l2"):
    """How far from the float64 result does the reference-class fp32 implementation land?  ONE run is one sample of a noisy quantity:
    the peaked softmaxes and ReLU / mask decisions make several gradients (all of Regular.2, the Homoaggre weight nets) move by 3-10x
    their typical error when any rounding changes -- a ReLU unit whose pre-activation is within rounding of zero opens or not, and
    the gradients downstream of it jump by a fixed amount (measured on Regular[0]: the error of dcost takes the values 2.3e-5, 5.2e-4
    or 2.3e-3 depending on which of two such units flip; the HIP path lands on the third, the unperturbed fp32 oracle on the second).
    So: the fp32 oracle on the unperturbed inputs and on `draws` copies whose images AND parameters are moved by one fp32 ulp (relative
    2^-23, random sign, torch seeds 0..draws-1), each compared with the float64 result of the UNPERTURBED inputs.  -> (per stage: max mean |d depth|, per tensor: max distance); distance = L2-relative or max-relative."""
    sys.path.insert(0, ROOT)
    from oracle import mvs_oracle as O
    imgs, extr, intr, dr = synth.make_scene(96, 64, 3, batch=2, rot_deg=3.0, seed=31)
    gtt = {k: torch.as_tensor(v) for k, v in gt.items()}

    def dist(a, r):
        a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
        if metric == "l2":
            return float(np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-30))
        return float(np.abs(a - r).max() / max(np.abs(r).max(), 1e-30))
    dmax, gmax = [0.0] * 4, {k: 0.0 for k in grads64}
    for t in range(-1, draws):
        im, src = imgs, sd32
        if t >= 0:
            torch.manual_seed(t)
            im = imgs * one_ulp(imgs.shape)
            src = {k: (v * one_ulp(v.shape) if v.dtype == torch.float32 and "running" not in k else v) for k, v in sd32.items()}
        sd = {k: (v.clone().requires_grad_(True) if v.dtype == torch.float32 and "running" not in k else v.clone()) for k, v in src.items()}
        out = O.core_forward(sd, im, extr, intr, dr, training=True)
        O.mvs_loss(out["depth"], gtt, dr).backward()
        for i, d in enumerate(out["depth"]):
            dmax[i] = max(dmax[i], float(np.abs(d.detach().numpy() - depths64[i]).mean()))
        for k in gmax:
            gmax[k] = max(gmax[k], dist(sd[k].grad.numpy(), grads64[k]))
    return dmax, gmax


@contextlib.contextmanager
def reference_in_float64():
    """The reference hard-codes fp32 in five places (`origin_imgs.float()` core.py:39, `dtype=torch.float32` base.py:102-103,
    `depth_range[...].float()` depthhypos.py:29,223 / refine.py:31, `dtype=torch.float` regress.py:15), so `config.model.double()`
    alone fails at the first conv.  While this context is active those spellings mean float64: the reference's OWN code then runs
    in double precision, unmodified on disk."""
    f32, fl, tf = torch.float32, torch.float, torch.Tensor.float
    torch.float32 = torch.float64
    torch.float = torch.float64
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.float32, torch.float, torch.Tensor.float = f32, fl, tf


def ref_train_step(model, ref_loss, sd32, gt, dtype, imgs_scale=None):
    """One forward + Loss + backward of the REFERENCE model (train.py:36-45) on the training golden's scene in `dtype`
    -> (loss, [depth], {name: grad}) as numpy."""
    imgs, extr, intr, dr = synth.make_scene(96, 64, 3, batch=2, rot_deg=3.0, seed=31)
    if imgs_scale is not None:
        imgs = imgs * imgs_scale
    model.float()
    model.load_state_dict(sd32)
    model.train()
    model.zero_grad()
    ctx = reference_in_float64() if dtype == torch.float64 else contextlib.nullcontext()
    if dtype == torch.float64:
        model.double()
    with ctx:
        out = model(imgs.to(dtype), extr.to(dtype), intr.to(dtype), dr.to(dtype))
        loss = ref_loss.Loss()(out, {k: torch.as_tensor(v).to(dtype) for k, v in gt.items()}, dr.to(dtype))
        loss.backward()
    res = (float(loss), [npy(d) for d in out["depth"]], {k: npy(p.grad) for k, p in model.named_parameters()})
    model.float()
    return res


def gen_train_f64(model, ref_loss, sd):
    """tests/golden/train_tiny_f64.npz: the training golden's step through the REFERENCE in float64 (the yardstick
    no longer comes from the oracle) and the reference-class fp32 spread around it: the reference in fp32 on the unperturbed inputs
    and on six copies whose images and parameters are moved by one fp32 ulp (`one_ulp`, torch seeds 0..5), each compared with the
    float64 result of the unperturbed inputs.  The oracle's own float64 run is stored as `oracle64:*` distances (they agree to
    ~1e-12: the restatement IS the reference's arithmetic)."""
    g = np.load(os.path.join(OUT, "train_tiny.npz"))
    gt = {k: g["gt" + k] for k in ("3", "2", "1", "0")}
    loss, depths, grads = ref_train_step(model, ref_loss, sd, gt, torch.float64)
    o_loss, o_depths, o_grads = train_f64(sd, gt)
    tg = {"loss": np.float64(loss), "oracle64:loss_absdiff": np.float64(abs(loss - o_loss))}
    for i, d in enumerate(depths):
        tg[f"depth{i}"] = d
        tg[f"oracle64:depth{i}"] = np.float64(np.abs(o_depths[i] - d).max())
        print(f"depth{i}: reference fp32 golden vs reference float64: mean |d| {np.abs(g[f'depth{i}'] - d).mean():.3e}; oracle float64 vs reference float64: max |d| {tg[f'oracle64:depth{i}']:.1e}")
    for k in TRAIN_GRAD_KEYS:
        tg["grad:" + k] = grads[k]
        tg["oracle64:grad:" + k] = np.float64(np.abs(o_grads[k] - grads[k]).max() / np.abs(grads[k]).max())
        print(f"grad:{k}: reference fp32 golden vs float64: max rel {np.abs(g['grad:' + k] - grads[k]).max() / np.abs(grads[k]).max():.2e}; oracle64 vs reference64 {tg['oracle64:grad:' + k]:.1e}")
    dmax, gmax = [0.0] * 4, {k: 0.0 for k in TRAIN_GRAD_KEYS}
    for t in range(-1, 6):
        scale, src = None, sd
        if t >= 0:
            torch.manual_seed(t)
            scale = one_ulp((2, 3, 3, 64, 96))
            src = {k: (v * one_ulp(v.shape) if v.dtype == torch.float32 and "running" not in k else v) for k, v in sd.items()}
        _, d32, g32 = ref_train_step(model, ref_loss, src, gt, torch.float32, scale)
        for i in range(4):
            dmax[i] = max(dmax[i], float(np.abs(d32[i].astype(np.float64) - depths[i]).mean()))
        for k in gmax:
            gmax[k] = max(gmax[k], float(np.abs(g32[k].astype(np.float64) - grads[k]).max() / np.abs(grads[k]).max()))
    for i, v in enumerate(dmax):
        tg[f"spread:depth{i}"] = np.float64(v)
    for k, v in gmax.items():
        tg["spread:grad:" + k] = np.float64(v)
        print(f"spread:grad:{k}: reference fp32, unperturbed + 6 one-ulp draws: max rel distance from float64 up to {v:.2e}")
    np.savez_compressed(os.path.join(OUT, "train_tiny_f64.npz"), **tg)


def gen_io():
    """PFM bytes written by the reference's tools/data_io.py:44-71 for a known array, and its parse of a pair file."""
    import tempfile
    sys.path.insert(0, REF)
    from tools import data_io as ref_io
    sys.path.remove(REF)
    rng = np.random.RandomState(3)
    img = (425 + 510 * rng.rand(5, 7)).astype(np.float32)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "a.pfm")
        ref_io.save_pfm(f, img)
        raw = np.frombuffer(open(f, "rb").read(), dtype=np.uint8)
        back, scale = ref_io.read_pfm(f)
        pair = os.path.join(d, "pair.txt")
        open(pair, "w").write("2\n0\n3 1 9.5 2 8.0 3 7.5\n1\n2 0 9.5 2 6.0\n")
        n, pairs = ref_io.read_pairfile(pair)
    np.savez(os.path.join(OUT, "io.npz"), img=img, pfm_bytes=raw, pfm_back=np.ascontiguousarray(back), pfm_scale=scale,
             pair_n=n, pair_ref=np.array([p[0] for p in pairs]), pair_src0=np.array(pairs[0][1]), pair_src1=np.array(pairs[1][1]))
    print("io.npz written", raw.size, "bytes of PFM")


LOADER_DTU_ITEMS = (0, 5, 13, -1)       # item indices read from each loader (negative: from the end), robust off and on
LOADER_BLENDED_ITEMS = (0, 3, -1)


def array_digest(a):
    """dtype, shape and SHA-256 of an array's bytes: what train_loaders.npz keeps of the images and ground-truth maps (exact equality
    at a few bytes per array)."""
    import hashlib
    a = np.ascontiguousarray(a)
    return "%s|%s|%s" % (a.dtype.str, "x".join(str(n) for n in a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def loader_sets(root):
    """The two small synthetic training sets (DTU and BlendedMVS layout, written by load/synthetic.py from fixed seeds) that
    train_loaders.npz was read from -> (dtu root, dtu pair file, blendedmvs root)."""
    from load import synthetic
    droot = synthetic.write_dtu_train_set(os.path.join(root, "dtu"), scenes=(2, 6), nviews_total=6, lightings=(0, 3), width=96, height=64)
    broot = synthetic.write_blendedmvs_set(os.path.join(root, "bl"), scans=("scanA", "scanB"), nviews_total=5, width=96, height=64)
    return droot, os.path.join(droot, "Cameras", "pair.txt"), broot


def gen_loaders():
    """Items of the reference's own load/dtutrain.py and load/blendedtrain.py on loader_sets(): composition order, robust sampling
    under random.seed(11), padding, ranges.  OpenCV is absent here, so the reference runs (in a subprocess, its `load` package
    would shadow ours) with a stub `cv2` whose `resize` is our data_io.resize_nearest -- the nearest-resize itself is not part of
    this fixture (tests/test_train_data_cpu.py pins it by its formula).  Cameras, ranges and lengths are stored as arrays, the images and
    ground-truth maps as array_digest() strings."""
    import inspect
    import subprocess
    import tempfile
    from tools import data_io
    with tempfile.TemporaryDirectory() as d:
        droot, pair, broot = loader_sets(d)
        stub = os.path.join(d, "stub")
        os.makedirs(stub)
        with open(os.path.join(stub, "cv2.py"), "w") as f:
            f.write("import importlib.util\n"
                    "_s = importlib.util.spec_from_file_location('_mdf_data_io', %r); _m = importlib.util.module_from_spec(_s); "
                    "_s.loader.exec_module(_m)\n"
                    "INTER_NEAREST = 0\n"
                    "def resize(img, size, interpolation=None):\n"
                    "    assert interpolation == INTER_NEAREST\n"
                    "    return _m.resize_nearest(img, size)\n" % os.path.abspath(data_io.__file__))
        code = inspect.getsource(array_digest) + (
            "import sys, random, numpy as np; sys.path[:0] = [%r, %r]\n"
            "from load.dtutrain import LoadDataset as D\n"
            "from load.blendedtrain import LoadDataset as B\n"
            "res = {}\n"
            "def put(tag, it):\n"
            "    for k in ('intrinsics', 'extrinsics', 'depth_range'): res[tag + k] = np.asarray(it[k])\n"
            "    res[tag + 'imgs'] = np.array(array_digest(np.asarray(it['imgs'])))\n"
            "    for k, v in it['ref_depths'].items(): res[tag + 'gt' + k] = np.array(array_digest(v))\n"
            "for robust in (0, 1):\n"
            "    d = D(%r, %r, [2, 6], [0, 3], 3, bool(robust)); b = B(%r, 4, bool(robust))\n"
            "    res['len_d%%d' %% robust] = np.array(len(d)); res['len_b%%d' %% robust] = np.array(len(b))\n"
            "    random.seed(11)\n"
            "    for i in %r: put('d%%d_%%d_' %% (robust, i), d[i %% len(d)])\n"
            "    for i in %r: put('b%%d_%%d_' %% (robust, i), b[i %% len(b)])\n"
            "np.savez_compressed(%r, **res)\n"
            % (REF, stub, droot, pair, broot, LOADER_DTU_ITEMS, LOADER_BLENDED_ITEMS, os.path.join(OUT, "train_loaders.npz")))
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        env.pop("PYTHONPATH", None)
        subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=d)
    print("train_loaders.npz written")


def filter_scene(h=96, w=128, nsrc=10, seed=3):
    """Synthetic multi-view depth maps of a slanted plane + bumps, with per-view noise/outliers, DTU-like cameras.
    Returns float32 numpy arrays: depths [V,h,w], conf [h,w], K [V,3,3], E [V,4,4] (view 0 = reference)."""
    rng = np.random.RandomState(seed)
    intr, extr, _ = synth.make_cameras(w, h, nsrc + 1, batch=1, rot_deg=3.0, seed=seed)
    K, E = intr[0].numpy().astype(np.float64), extr[0].numpy().astype(np.float64)
    # world surface z = f(x, y): intersect each pixel ray iteratively (3 fixed-point steps are plenty for a gentle surface)
    def surface(xw, yw):
        return 650.0 + 0.15 * xw - 0.1 * yw + 12.0 * np.sin(xw / 35.0) * np.cos(yw / 28.0)
    depths = []
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for v in range(nsrc + 1):
        Kinv, Einv = np.linalg.inv(K[v]), np.linalg.inv(E[v])
        d = np.full((h, w), 650.0)
        for _ in range(20):   # additive fixed point: the ray's z-component is ~1
            cam = (Kinv @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])) * d.ravel()
            wld = (Einv @ np.vstack([cam, np.ones(h * w)]))[:3]
            d = d + (surface(wld[0], wld[1]) - wld[2]).reshape(h, w)
        noise = rng.normal(0, 1.0, (h, w)) + (rng.rand(h, w) < 0.08) * rng.normal(0, 25.0, (h, w))
        depths.append((d + noise).astype(np.float32))
    conf = (0.55 + 0.45 * rng.rand(h, w)).astype(np.float32)
    return np.stack(depths), conf, intr[0].numpy(), extr[0].numpy()


def gen_filter():
    """Goldens for the consistency filter from the reference's own functions (tools/filter/dynamic_filter_gpu.py:166-238).
    That module imports `plyfile` (absent here) only to WRITE the .ply at the end of filter(); an empty placeholder
    module object lets the import proceed -- none of the functions called below touches it."""
    import types
    sys.modules.setdefault("plyfile", types.SimpleNamespace(PlyData=None, PlyElement=None))
    fdir = os.path.join(REF, "tools", "filter")
    sys.path.insert(0, fdir)
    env = dict(os.environ)
    import dynamic_filter_gpu as ref_f          # sets CUDA_VISIBLE_DEVICES; irrelevant on this CPU-only box
    os.environ.clear(); os.environ.update(env)
    sys.path.remove(fdir)
    depths, conf, K, E = filter_scene()
    T = torch.from_numpy
    g = {"depths": depths, "conf": conf, "K": K, "E": E}
    nsrc = depths.shape[0] - 1
    counts = [torch.zeros(1, *conf.shape) for _ in range(9)]
    nvalid, acc = 0, 0
    for v in range(1, nsrc + 1):
        masks, last, rep = ref_f.check_geometric_consistency(T(depths[0]), T(K[0]), T(E[0]), T(depths[v]), T(K[v]), T(E[v]), 4, 1300.)
        g[f"masks{v}"] = np.packbits(torch.stack(masks)[:, 0].numpy(), axis=0)       # 9 masks -> 2 bytes per pixel
        g[f"rep{v}"] = rep[0].numpy()
        for i in range(9):
            counts[i] = counts[i] + masks[i].float()
        nvalid = nvalid + last
        acc = acc + rep
    drep, xr, yr, xs_, ys_ = ref_f.reproject_with_depth(T(depths[0]), T(K[0]), T(E[0]), T(depths[1]), T(K[1]), T(E[1]))
    g["reproj1"] = torch.stack([drep[0], xr[0], yr[0], xs_[0], ys_[0]]).numpy()
    # fusion exactly as filter():91-103
    geo = 0
    for i in range(2, 11):
        geo = geo + (counts[i - 2] >= i)
    g["depth_avg"] = ((acc + T(depths[0])) / (nvalid + 1))[0].numpy()
    g["geo_mask"] = (geo >= 5)[0].numpy()
    g["photo_mask"] = (T(conf) > 0.8).numpy()
    g["final_mask"] = np.logical_and(g["photo_mask"], g["geo_mask"])
    np.savez_compressed(os.path.join(OUT, "filter.npz"), **g)
    print("filter.npz: geo", int(g["geo_mask"].sum()), "photo", int(g["photo_mask"].sum()), "final", int(g["final_mask"].sum()),
          "of", conf.size)


def main():
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    if "--only-io" in sys.argv:
        return gen_io()
    if "--only-filter" in sys.argv:
        return gen_filter()
    if "--only-loaders" in sys.argv:
        return gen_loaders()
    cfg, base, agg, regress, dh, scale, ref_loss = load_reference()
    model = cfg.model
    sd = synth.seeded_state_dict(model.state_dict(), seed=1)
    model.load_state_dict(sd)
    model.eval()
    if "--only-train" in sys.argv:
        return gen_train(model, sd, ref_loss)
    if "--only-train-f64" in sys.argv:      # needs train_tiny.npz (its ground-truth maps)
        return gen_train_f64(model, ref_loss, sd)
    meta = {k: list(v.shape) for k, v in model.state_dict().items()}
    np.savez(os.path.join(OUT, "state_dict_meta.npz"),
             keys=np.array(list(meta.keys())), shapes=np.array([str(s) for s in meta.values()]),
             dtypes=np.array([str(v.dtype) for v in model.state_dict().values()]),
             nparams=np.array(sum(p.numel() for p in model.parameters())))

    # ------------------------------------------------------------------ operator level (ops.npz)
    g = {}
    torch.manual_seed(1234)
    W, H, V = 96, 64, 3
    imgs, extr, intr, dr = synth.make_scene(W, H, V, batch=2, rot_deg=4.0, seed=5)
    with torch.no_grad():
        # a2 scale_cam
        for st in range(3):
            rp, sps = scale.scale_cam(intr, extr, st)
            g[f"scale_ref{st}"] = npy(rp)
            g[f"scale_src{st}"] = npy(torch.stack(sps))
        # a4 homo_warping: stage-0-like (shared hypotheses) and stage-1-like (per-pixel hypotheses)
        rp, sps = scale.scale_cam(intr, extr, 0)
        h8, w8 = H // 8, W // 8
        fea0 = torch.randn(2, 64, h8, w8)
        hyp0 = dh.HyposByFit(48, None, 0.0)(None, dr, None, None)
        g["warp0_src"] = npy(fea0)
        g["warp0_hyp"] = npy(hyp0[:, ::4])
        g["warp0_out"] = npy(base.homo_warping(fea0, sps[0], rp, hyp0[:, ::4]))
        rp1, sps1 = scale.scale_cam(intr, extr, 1)
        h4, w4 = H // 4, W // 4
        fea1 = torch.randn(2, 32, h4, w4)
        hyp1 = (425 + 510 * torch.rand(2, 1, h4, w4)) + torch.linspace(-20, 20, 8).reshape(1, 8, 1, 1)
        g["warp1_src"] = npy(fea1)
        g["warp1_hyp"] = npy(hyp1)
        g["warp1_out"] = npy(base.homo_warping(fea1, sps1[1], rp1, hyp1))
        # H4: plane behind the source camera (z<0) and z==0 (kept separate)
        hyp_neg = torch.full((2, 2, 1, 1), -300.0)
        hyp_neg[:, 1] = 0.0
        g["warpneg_hyp"] = npy(hyp_neg)
        g["warpneg_out"] = npy(base.homo_warping(fea0, sps[0], rp, hyp_neg))
        p_zero = rp.clone()
        src_zero = sps[0].clone()
        src_zero[:, 2, :] = 0.0  # forces z == 0 for every pixel -> inf/nan coordinates
        g["warpz0_srcproj"] = npy(src_zero)
        g["warpz0_out"] = npy(base.homo_warping(fea0, src_zero, p_zero, hyp0[:, :3]))
        # a5 VectorAggregate (eval), all three stage shapes, and a5' variance
        feas = [[torch.randn(2, c, H // s, W // s) for _ in range(V)] for c, s in ((64, 8), (32, 4), (16, 2))]
        hyps = [hyp0,
                (425 + 510 * torch.rand(2, 1, h4, w4)) + torch.linspace(-30, 30, 24).reshape(1, 24, 1, 1),
                (425 + 510 * torch.rand(2, 1, H // 2, W // 2)) + torch.linspace(-6, 6, 8).reshape(1, 8, 1, 1)]
        for st in range(3):
            rp_s, sps_s = scale.scale_cam(intr, extr, st)
            g[f"agg{st}_feas"] = npy(torch.stack(feas[st]))
            g[f"agg{st}_hyp"] = npy(hyps[st])
            g[f"agg{st}_cost"] = npy(model.Homoaggre[st](feas[st], rp_s, sps_s, hyps[st]))
        g["var0_cost"] = npy(agg.homo_aggregate_by_variance(feas[0], rp, sps, hyp0[:, ::4]))
        g["var2_cost"] = npy(agg.homo_aggregate_by_variance(feas[2], *scale.scale_cam(intr, extr, 2), hyps[2][:, ::2]))
        # a6/a7 regularisers (on the aggregated costs above) + a9/a10
        for st in range(3):
            cost = torch.from_numpy(g[f"agg{st}_cost"])
            prob = model.Regular[st](cost)
            g[f"reg{st}_prob"] = npy(prob)
            g[f"reg{st}_depth"] = npy(regress.depth_regression(prob, hyps[st]))
        g["conf2"] = npy(regress.confidence_regress(torch.from_numpy(g["reg2_prob"])))
        # a3 HyposByFit: stage-1 module on stage-0 outputs, stage-2 module on stage-1 outputs
        p0, d0 = torch.from_numpy(g["reg0_prob"]), torch.from_numpy(g["reg0_depth"])
        g["hyp1_out"] = npy(model.Depth_hypos[1](d0, dr, p0, hyp0, upsample=True))
        with HostValueRecorder() as rec:
            g["hyp1_s"] = npy(model.Depth_hypos[1]._gauss_fitting1(d0, p0, hyp0))
        fit = [r for sa, sb, r in rec.calls if len(sa) == 5 and sa[3:] == (3, 3) and sb[3] == 3]
        g["hyp1_fit_row"] = npy(fit[0][:, 0, 0, 0, :])     # the build host's row 0 of (X^T X)^-1 X^T (depthhypos.py:206-208)
        p1, d1 = torch.from_numpy(g["reg1_prob"]), torch.from_numpy(g["reg1_depth"])
        g["hyp2_out"] = npy(model.Depth_hypos[2](d1, dr, p1, hyps[1], upsample=True))
        g["hyp2_s"] = npy(model.Depth_hypos[2]._laplace_fitting(d1, p1, hyps[1]))
        # flat probability volume (H3: ill-conditioned gauss fit; recorded, compared loosely)
        pflat = torch.softmax(0.05 * torch.randn(2, 48, h8, w8), 1)
        g["hyp1flat_prob"] = npy(pflat)
        g["hyp1flat_s"] = npy(model.Depth_hypos[1]._gauss_fitting1(d0, pflat, hyp0))
        # a11 backbone, a12 refine
        f8, f4, f2 = model.Backbone(imgs[:, 0])
        g["fpn_f8"], g["fpn_f4"], g["fpn_f2"] = npy(f8), npy(f4), npy(f2)
        g["refine_out"] = npy(model.Refine(torch.from_numpy(g["reg2_depth"]), dr))
    np.savez_compressed(os.path.join(OUT, "ops.npz"), **g)

    # ------------------------------------------------------------------ end-to-end goldens
    def e2e(name, w, h, v, batch, rot, seed, keep):
        imgs, extr, intr, dr = synth.make_scene(w, h, v, batch=batch, rot_deg=rot, seed=seed)
        tr = {}
        hooks = []
        if keep:
            for st in range(3):
                hooks.append(model.Homoaggre[st].register_forward_hook(
                    lambda m, i, o, st=st: tr.__setitem__(f"cost{st}", npy(o))))
                hooks.append(model.Regular[st].register_forward_hook(
                    lambda m, i, o, st=st: tr.__setitem__(f"prob{st}", npy(o))))
                hooks.append(model.Depth_hypos[st].register_forward_hook(
                    lambda m, i, o, st=st: tr.__setitem__(f"hypos{st}", npy(o))))
        with torch.no_grad(), HostValueRecorder() as rec:
            out = model(imgs, extr, intr, dr)
        for hk in hooks:
            hk.remove()
        tr.update(rec.values(v))
        for st in (1, 2):
            tr[f"host_log_thresh{st}"] = npy(torch.log(model.Depth_hypos[st].prob_thresh))
        tr["depth"], tr["confidence"] = npy(out["depth"]), npy(out["confidence"])
        tr["cfg"] = np.array([w, h, v, batch, rot, seed], dtype=np.float64)
        np.savez_compressed(os.path.join(OUT, name), **tr)
        print(name, "depth mean", float(out["depth"].mean()), "conf mean", float(out["confidence"].mean()))

    e2e("e2e_tiny.npz", 96, 64, 3, 1, 3.0, 11, True)
    e2e("e2e_cfg1.npz", 160, 128, 3, 1, 0.0, 0, False)       # BASELINE config 1 shape
    e2e("e2e_5view.npz", 320, 256, 5, 1, 5.0, 21, False)

    gen_train(model, sd, ref_loss)
    gen_train_f64(model, ref_loss, sd)
    gen_io()
    gen_filter()
    gen_loaders()
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)) // 1024, "KiB")


if __name__ == "__main__":
    main()
