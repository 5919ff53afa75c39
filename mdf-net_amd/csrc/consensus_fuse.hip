// DTU depth-map fusion by multi-view consensus (the fusibile step of the reference's tools/gipuma/main.py -d, run with
// normal_thresh 360 and view selection off, so normals take no part).  One launch set per scan:
//   1. consensus_fuse_kernel: a thread owns (reference view r, pixel); it lifts the pixel to 3-D with r's depth, projects it
//      into every other view v, samples v's depth bilinearly (wrap addressing), keeps v when the two disparities f*b/z and
//      f*b/d^ agree within disp_thresh, and averages the agreeing views' points and colours.  Dense record per pixel.
//   2. consensus_scan_kernel: exclusive scan of the per-block kept counts (one block), per-view counts, total.
//   3. consensus_compact_kernel: order-preserving compaction (view-major, row-major pixel order) into xyz / rgb.
// No atomics: the output order and every value are run-independent.
//
// Arithmetic order == tests/consensus_oracle.py (torch fp32 elementwise): every matrix-vector product is the left-to-right chain
// ((m0*x0 + m1*x1) + m2*x2) [+ m3]; divides and the square root are IEEE-rounded; no fma (the library builds with
// -ffp-contract=off).  Bilinear weights are exact fp32 (a texture unit quantises them to 8 fractional bits: DESIGN.md 7).
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int kCamStride = 32;   // floats per view in the camera table: P[12] (3x4 row-major), M_inv[9], C[3], pad
constexpr int kBlock = 256;

// Per-view data is read through the CONSTANT address space: the loop index v is wave-uniform, so P / M_inv / C of view v are
// s_load'ed into SGPRs instead of being fetched per lane (consistency.hip explains the measured cost of the alternative).
typedef const __attribute__((address_space(4))) float* cfloat_p;

struct FuseArgs {
  const float* depths;        // [n][h][w]
  const unsigned* colors;     // [n][h][w], RGBA8 (A unused)
  const float* cams;          // [n][kCamStride]
  float4* dense;              // [n][h*w]: x, y, z, bits(rgb | keep << 24)
  int* block_counts;          // [n][nblk]
  float f, disp_thresh;
  int n, h, w, nblk, num_consistent;
};

__device__ __forceinline__ float dot3(cfloat_p m, float x0, float x1, float x2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(m[0], x0), __fmul_rn(m[1], x1)), __fmul_rn(m[2], x2));
}

__device__ __forceinline__ float lerp4(float t00, float t01, float t10, float t11, float w00, float w01, float w10, float w11) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(t00, w00), __fmul_rn(t01, w01)), __fmul_rn(t10, w10)), __fmul_rn(t11, w11));
}

__device__ __forceinline__ float chan(unsigned c, int k) { return (float)((c >> (8 * k)) & 255u); }

__global__ __launch_bounds__(kBlock) void consensus_fuse_kernel(const FuseArgs p) {
  // f * |C_r - C_v| for every v, once per block.  The square root is taken in double and rounded to float: that is the
  // correctly rounded fp32 root (53 >= 2*24 + 2 bits), which v_sqrt_f32 behind __fsqrt_rn is not (1 ulp) -- a 1-ulp baseline
  // moved a handful of disparity decisions per DTU scan against the oracle.
  __shared__ float fb_tab[MDF_MAX_FUSE_VIEWS];
  const int r = blockIdx.y;
  const cfloat_p cams = (cfloat_p)p.cams;
  const cfloat_p cr = cams + kCamStride * r;
  for (int v = threadIdx.x; v < p.n; v += kBlock) {
    const float* cv = p.cams + kCamStride * v;
    const float e0 = __fsub_rn(cr[21], cv[21]), e1 = __fsub_rn(cr[22], cv[22]), e2 = __fsub_rn(cr[23], cv[23]);
    const float ss = __fadd_rn(__fadd_rn(__fmul_rn(e0, e0), __fmul_rn(e1, e1)), __fmul_rn(e2, e2));
    fb_tab[v] = __fmul_rn(p.f, (float)__dsqrt_rn((double)ss));
  }
  __syncthreads();
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  bool keep = false;
  float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pix < hw) {
    const int yi = pix / p.w, xi = pix - yi * p.w;
    const size_t rpix = (size_t)r * hw + pix;
    const float d = p.depths[rpix];
    // X = M_inv_r (d*x - p4.x, d*y - p4.y, d - p4.z)
    const float a0 = __fsub_rn(__fmul_rn(d, (float)xi), cr[3]);
    const float a1 = __fsub_rn(__fmul_rn(d, (float)yi), cr[7]);
    const float a2 = __fsub_rn(d, cr[11]);
    const float X0 = dot3(cr + 12, a0, a1, a2), X1 = dot3(cr + 15, a0, a1, a2), X2 = dot3(cr + 18, a0, a1, a2);
    float s0 = X0, s1 = X1, s2 = X2;
    const unsigned cref = p.colors[rpix];
    float c0 = chan(cref, 0), c1 = chan(cref, 1), c2 = chan(cref, 2);
    int n = 0;
    const float fw = (float)p.w, fh = (float)p.h;
    for (int v = 0; v < p.n; ++v) {
      if (v == r) continue;
      const cfloat_p cv = cams + kCamStride * v;
      const float u = __fadd_rn(dot3(cv, X0, X1, X2), cv[3]);
      const float q = __fadd_rn(dot3(cv + 4, X0, X1, X2), cv[7]);
      const float z = __fadd_rn(dot3(cv + 8, X0, X1, X2), cv[11]);
      const float px = __fdiv_rn(u, z), py = __fdiv_rn(q, z);
      if (!(px >= 0.f && px < fw && py >= 0.f && py < fh)) continue;      // (NaN fails here too)
      const float x0f = floorf(px), y0f = floorf(py);
      const int ix = (int)x0f, iy = (int)y0f;                              // 0 <= ix < w, 0 <= iy < h
      const int ix1 = (ix + 1 == p.w) ? 0 : ix + 1, iy1 = (iy + 1 == p.h) ? 0 : iy + 1;   // wrap addressing
      const float ax = __fsub_rn(px, x0f), ay = __fsub_rn(py, y0f);
      const float bx = __fsub_rn(1.f, ax), by = __fsub_rn(1.f, ay);
      const float w00 = __fmul_rn(bx, by), w01 = __fmul_rn(ax, by), w10 = __fmul_rn(bx, ay), w11 = __fmul_rn(ax, ay);
      const unsigned r0 = (unsigned)(iy * p.w), r1 = (unsigned)(iy1 * p.w);
      const float* dv = p.depths + (size_t)v * hw;
      const float dh = lerp4(dv[r0 + ix], dv[r0 + ix1], dv[r1 + ix], dv[r1 + ix1], w00, w01, w10, w11);
      // disparity test with the baseline of (r, v) and the scan's one focal length
      const float fb = fb_tab[v];
      if (!(fabsf(__fsub_rn(__fdiv_rn(fb, z), __fdiv_rn(fb, dh))) < p.disp_thresh)) continue;
      // v's own point at the truncated pixel with the interpolated depth
      const float b0 = __fsub_rn(__fmul_rn(dh, (float)ix), cv[3]);
      const float b1 = __fsub_rn(__fmul_rn(dh, (float)iy), cv[7]);
      const float b2 = __fsub_rn(dh, cv[11]);
      s0 = __fadd_rn(s0, dot3(cv + 12, b0, b1, b2));
      s1 = __fadd_rn(s1, dot3(cv + 15, b0, b1, b2));
      s2 = __fadd_rn(s2, dot3(cv + 18, b0, b1, b2));
      const unsigned* col = p.colors + (size_t)v * hw;
      const unsigned t00 = col[r0 + ix], t01 = col[r0 + ix1], t10 = col[r1 + ix], t11 = col[r1 + ix1];
      c0 = __fadd_rn(c0, lerp4(chan(t00, 0), chan(t01, 0), chan(t10, 0), chan(t11, 0), w00, w01, w10, w11));
      c1 = __fadd_rn(c1, lerp4(chan(t00, 1), chan(t01, 1), chan(t10, 1), chan(t11, 1), w00, w01, w10, w11));
      c2 = __fadd_rn(c2, lerp4(chan(t00, 2), chan(t01, 2), chan(t10, 2), chan(t11, 2), w00, w01, w10, w11));
      ++n;
    }
    const float cnt = __fadd_rn((float)n, 1.f);
    float x = __fdiv_rn(s0, cnt), y = __fdiv_rn(s1, cnt), zz = __fdiv_rn(s2, cnt);
    // fusibile's host side: a point with any coordinate exactly 0 is not written; a non-finite one is written as the origin
    keep = n >= p.num_consistent && x != 0.f && y != 0.f && zz != 0.f;
    if (!(isfinite(x) && isfinite(y) && isfinite(zz))) x = y = zz = 0.f;
    const unsigned q0 = (unsigned)fminf(__fdiv_rn(c0, cnt), 255.f);
    const unsigned q1 = (unsigned)fminf(__fdiv_rn(c1, cnt), 255.f);
    const unsigned q2 = (unsigned)fminf(__fdiv_rn(c2, cnt), 255.f);
    rec = make_float4(x, y, zz, __uint_as_float(q0 | (q1 << 8) | (q2 << 16) | ((keep ? 1u : 0u) << 24)));
    p.dense[rpix] = rec;
  }
  const int kept = __syncthreads_count(keep ? 1 : 0);
  if (threadIdx.x == 0) p.block_counts[r * p.nblk + blockIdx.x] = kept;
}

// Exclusive scan of the nitems block counts, per-view counts and the total, in one block.
__global__ __launch_bounds__(mdf::kScanThreads) void consensus_scan_kernel(const int* __restrict__ counts, long long* __restrict__ offsets,
                                                                      int nitems, int nblk, int n, int* __restrict__ view_counts,
                                                                      long long* __restrict__ total) {
  mdf::block_exclusive_scan<int, true>(counts, nitems, offsets, total, nblk, n, view_counts);
}

__global__ __launch_bounds__(kBlock) void consensus_compact_kernel(const float4* __restrict__ dense, const long long* __restrict__ offsets,
                                                                   int hw, int nblk, long long capacity, float* __restrict__ xyz,
                                                                   unsigned char* __restrict__ rgb) {
  __shared__ int wave_base[kBlock / 64];
  const int r = blockIdx.y;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pix < hw) rec = dense[(size_t)r * hw + pix];
  const unsigned bits = __float_as_uint(rec.w);
  const bool keep = pix < hw && (bits >> 24) != 0u;
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wave_base[wave] = __popcll(m);
  __syncthreads();
  int base = 0;
  for (int i = 0; i < wave; ++i) base += wave_base[i];
  if (!keep) return;
  const long long o = offsets[r * nblk + blockIdx.x] + base + before;
  if (o >= capacity) return;
  xyz[3 * o + 0] = rec.x;
  xyz[3 * o + 1] = rec.y;
  xyz[3 * o + 2] = rec.z;
  rgb[3 * o + 0] = (unsigned char)(bits & 255u);
  rgb[3 * o + 1] = (unsigned char)((bits >> 8) & 255u);
  rgb[3 * o + 2] = (unsigned char)((bits >> 16) & 255u);
}

inline int nblocks(int h, int w) { return (h * w + kBlock - 1) / kBlock; }

}  // namespace

extern "C" long long mdf_consensus_fuse_workspace(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  const long long items = (long long)n * nblocks(h, w);
  return (long long)n * h * w * (long long)sizeof(float4) + items * (long long)(sizeof(long long) + sizeof(int));
}

namespace {

// Workspace layout: dense records [n][h*w] float4, then the block offsets [n*nblk] int64, then the block counts [n*nblk] int32.
struct WsLayout {
  float4* dense;
  long long* offsets;
  int* counts;
  int hw, nblk, items;
};

int ws_layout(void* workspace, int n, int h, int w, WsLayout& L) {
  MDF_REQUIRE(n >= 2 && n <= MDF_MAX_FUSE_VIEWS, "n=%d views out of range [2,%d]", n, MDF_MAX_FUSE_VIEWS);
  MDF_REQUIRE(h >= 1 && w >= 1 && (long long)h * w <= (1ll << 30), "bad shape %dx%d", h, w);
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
  L.hw = h * w;
  L.nblk = nblocks(h, w);
  const long long items = (long long)n * L.nblk;
  MDF_REQUIRE(items <= (1ll << 31) - 1, "too many blocks");
  L.items = (int)items;
  char* ws = static_cast<char*>(workspace);
  L.dense = reinterpret_cast<float4*>(ws);
  L.offsets = reinterpret_cast<long long*>(ws + (size_t)n * L.hw * sizeof(float4));
  L.counts = reinterpret_cast<int*>(L.offsets + items);
  return MDF_OK;
}

int launch_compact(const WsLayout& L, int n, float* xyz, unsigned char* rgb, long long capacity, hipStream_t s) {
  hipLaunchKernelGGL(consensus_compact_kernel, dim3(L.nblk, n), dim3(kBlock), 0, s, L.dense, L.offsets, L.hw, L.nblk, capacity,
                     xyz, rgb);
  return mdf::check_launch("consensus_compact_kernel");
}

}  // namespace

extern "C" int mdf_consensus_fuse_fwd(const float* depths, const unsigned char* colors, const float* cams, int n, int h, int w,
                                      float f, float disp_thresh, int num_consistent, void* workspace, float* xyz,
                                      unsigned char* rgb, long long capacity, int* view_counts, long long* total, void* stream) {
  MDF_REQUIRE(depths && colors && cams && workspace && view_counts && total, "null pointer argument");
  MDF_REQUIRE((xyz == nullptr) == (rgb == nullptr), "null pointer argument: xyz and rgb are both given or both null");
  MDF_REQUIRE(capacity >= 0, "negative capacity");
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(colors) % 4 == 0, "colors must be 4-byte aligned");
  WsLayout L;
  if (int rc = ws_layout(workspace, n, h, w, L)) return rc;
  FuseArgs p{};
  p.depths = depths;
  p.colors = reinterpret_cast<const unsigned*>(colors);
  p.cams = cams;
  p.dense = L.dense;
  p.block_counts = L.counts;
  p.f = f; p.disp_thresh = disp_thresh;
  p.n = n; p.h = h; p.w = w; p.nblk = L.nblk; p.num_consistent = num_consistent;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(consensus_fuse_kernel, dim3(L.nblk, n), dim3(kBlock), 0, s, p);
  if (int rc = mdf::check_launch("consensus_fuse_kernel")) return rc;
  hipLaunchKernelGGL(consensus_scan_kernel, dim3(1), dim3(mdf::kScanThreads), 0, s, L.counts, L.offsets, L.items, L.nblk, n,
                     view_counts, total);
  if (int rc = mdf::check_launch("consensus_scan_kernel")) return rc;
  if (xyz == nullptr) return MDF_OK;                 // two-phase use: the caller sizes the output from *total, then compacts
  return launch_compact(L, n, xyz, rgb, capacity, s);
}

extern "C" int mdf_consensus_compact(void* workspace, int n, int h, int w, float* xyz, unsigned char* rgb, long long capacity,
                                     void* stream) {
  MDF_REQUIRE(workspace && xyz && rgb, "null pointer argument");
  MDF_REQUIRE(capacity >= 0, "negative capacity");
  WsLayout L;
  if (int rc = ws_layout(workspace, n, h, w, L)) return rc;
  return launch_compact(L, n, xyz, rgb, capacity, (hipStream_t)stream);
}
