import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'mdf-net_amd')]
import torch
from mdfnet_hip import ops, train_ops
dev = torch.device('cuda', 0)
x = torch.randn(1, 4, 8, 16, 16, device=dev)
conv = torch.nn.Conv3d(16, 16, 3, padding=1, bias=False).to(dev)
wp = ops.pack_conv3d_weight(conv.weight)
def t(fn, n=2000):
    for _ in range(20): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    dt = (time.perf_counter() - t0) / n; torch.cuda.synchronize(); return dt * 1e6
print("conv3d_ndhwc host us/call", t(lambda: ops.conv3d_ndhwc(x, wp, 16, 16, 1, False, None, None, False, None)))
# the 2-D entry: a layer early in conv_lds.hip's table (16 -> 16 k3) and the one its last row takes (8 -> 4 k3 with res_up: the longest walk)
x2, x8 = torch.randn(1, 16, 16, 16, device=dev), torch.randn(1, 16, 16, 8, device=dev)
wp2 = ops.pack_conv2d_weight(torch.randn(16, 16, 3, 3, device=dev))
wp8 = ops.pack_conv2d_weight(torch.randn(4, 8, 3, 3, device=dev))
up8 = torch.randn(1, 8, 8, 4, device=dev)
print("conv2d_nhwc 16->16 host us/call", t(lambda: ops.conv2d_nhwc(x2, wp2, 16, 16, 3, 1)))
print("conv2d_nhwc 8->4 res_up (last row) host us/call", t(lambda: ops.conv2d_nhwc(x8, wp8, 8, 4, 3, 1, res_up=up8)))
if os.environ.get("MDF_HOST_OVERHEAD_CONV_ONLY"):
    sys.exit(0)
print("bn_stats", t(lambda: train_ops.bn_stats(x, 4 * 8 * 16, 16)))
print("pack_conv3d_weight", t(lambda: ops.pack_conv3d_weight(conv.weight)))
print("torch.empty", t(lambda: torch.empty((1, 4, 8, 16, 16), device=dev)))
print("torch.zeros(32,f64)", t(lambda: torch.zeros(32, device=dev, dtype=torch.float64)))
print("torch add", t(lambda: x + x))
big = torch.randn(4096, 4096, device=dev)
h = torch.randn(12)
def busy_then(fn):
    def g():
        y = big @ big
        fn()
    return g
print("matmul alone", t(lambda: big @ big, 50))
print("matmul + .to(dev) pageable", t(busy_then(lambda: h.to(dev, non_blocking=True)), 50))
hp = h.pin_memory()
print("matmul + .to(dev) pinned", t(busy_then(lambda: hp.to(dev, non_blocking=True)), 50))
print("matmul + torch.tensor(list, device)", t(busy_then(lambda: torch.tensor([1, 2, 3], device=dev)), 50))
print("matmul + torch.full", t(busy_then(lambda: torch.full((1,), 0.5, device=dev)), 50))
