// Validation metrics of depth maps on the device ("Validation metrics"): per map the number of valid
// pixels (gt > depth_min, the training loss's mask), the sum of |est - gt|, the pixels under each of T absolute thresholds,
// how many ground-truth depths lie inside the hypothesis interval [lo, hi] a stage was given and how wide that interval is;
// and the same error columns per confidence bin (K = 32 uniform bins over [0, 1]).
//
// The numbers are compared across epochs and across option choices, so the path is run-to-run bit-identical: no
// floating-point atomics.  Every block writes its partial table to a workspace, a finalize launch folds the block partials
// in block order; inside a block the order is fixed by lane, by trip and by wave.  The result depends on the shapes only.
#include <cmath>
#include "common.h"

namespace {

constexpr int kT = 512;              // threads per block (8 waves: two blocks give a CU 16 waves to hide the shuffle trees behind)
constexpr int kWaves = kT / 64;
constexpr int kMaxMaps = 8;
constexpr int kBins = 32;
constexpr int kMaxThr = 4;
// columns of a table row: n, n_nonfinite, sum_e, under[0..3], covered, sum_width
constexpr int kCols = 9;
constexpr int kRows = 1 + kBins;
constexpr int kTable = kRows * kCols;
enum { cN = 0, cNonfinite = 1, cSumE = 2, cUnder = 3, cCovered = 7, cSumWidth = 8 };

struct MetricMaps {
  const float* est[kMaxMaps];
  const float* gt[kMaxMaps];
  const float* hypos[kMaxMaps];     // NULL: no interval columns.  [B,D,h,w] (per pixel) or [B,D]
  const float* conf[kMaxMaps];      // NULL: no bin rows
  long long per_batch[kMaxMaps];
  long long ws_off[kMaxMaps];       // first partial table of the map, in tables
  int D[kMaxMaps];
  int per_pixel[kMaxMaps];
  int nblk[kMaxMaps];               // blocks per batch item that have pixels of this map
};

__device__ __forceinline__ double load_floor(const void* p, int is_f64, long long i) {
  return is_f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned count(bool p) { return (unsigned)__popcll(__ballot(p)); }

struct BlockTables {
  double bin_sum[kWaves][kBins];
  unsigned bin_cnt[kWaves][kBins][1 + kMaxThr];     // n, under[t]
  double wave_sum[kWaves][2];                       // sum_e, sum_width
  unsigned wave_cnt[kWaves][3 + kMaxThr];           // n, n_nonfinite, covered, under[t]
};

template <int T>
__global__ __launch_bounds__(kT) void depth_metrics_reduce_multi_kernel(MetricMaps mm, const void* __restrict__ floor_, int floor_f64,
                                                                        int floor_stride, const float* __restrict__ thr,
                                                                        double* __restrict__ ws) {
  __shared__ BlockTables sh;
  const int m = blockIdx.z, b = blockIdx.y;
  const long long per = mm.per_batch[m];
  if ((long long)blockIdx.x * kT >= per) return;                   // (the grid is sized for the largest map; whole blocks leave)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ est = mm.est[m] + (long long)b * per;
  const float* __restrict__ gt = mm.gt[m] + (long long)b * per;
  const float* __restrict__ conf = mm.conf[m] ? mm.conf[m] + (long long)b * per : nullptr;
  const float* __restrict__ lo = nullptr;
  const float* __restrict__ hi = nullptr;
  const int pp = mm.per_pixel[m];
  if (mm.hypos[m]) {
    const long long plane = pp ? per : 1;
    lo = mm.hypos[m] + (long long)b * mm.D[m] * plane;
    hi = lo + (long long)(mm.D[m] - 1) * plane;
  }
  const double fl = load_floor(floor_, floor_f64, (long long)b * floor_stride);
  float th[T];
#pragma unroll
  for (int t = 0; t < T; ++t) th[t] = thr[b * T + t];

  if (conf) {
    for (int i = threadIdx.x; i < kWaves * kBins; i += kT) {
      (&sh.bin_sum[0][0])[i] = 0.0;
#pragma unroll
      for (int k = 0; k < 1 + kMaxThr; ++k) (&sh.bin_cnt[0][0][0])[i * (1 + kMaxThr) + k] = 0u;
    }
    __syncthreads();
  }

  double s_e = 0.0, s_w = 0.0;                 // per lane, in trip order
  unsigned c_n = 0, c_nf = 0, c_cov = 0;       // per wave (from ballots: the same in every lane)
  unsigned c_under[T];
#pragma unroll
  for (int t = 0; t < T; ++t) c_under[t] = 0;

  // every lane of the block makes the same number of trips, so that ballots and shuffles see whole waves
  for (long long base = (long long)blockIdx.x * kT; base < per; base += (long long)gridDim.x * kT) {
    const long long i = base + threadIdx.x;
    const bool in = i < per;
    float g = 0.f, e_ = 0.f, cf = 0.f, l = 0.f, h = 0.f;
    if (in) {
      g = gt[i];
      e_ = est[i];
      if (conf) cf = conf[i];
      if (lo) {
        l = pp ? lo[i] : lo[0];
        h = pp ? hi[i] : hi[0];
      }
    }
    const bool valid = in && (double)g > fl;
    const bool finite = isfinite(e_) && isfinite(cf) && isfinite(l) && isfinite(h);
    const bool ok = valid && finite;
    const float e = fabsf(e_ - g);
    c_nf += count(valid && !finite);
    c_n += count(ok);
    bool under[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      under[t] = ok && e < th[t];
      c_under[t] += count(under[t]);
    }
    if (ok) s_e += (double)e;
    if (lo) {
      c_cov += count(ok && l <= g && g <= h);
      if (ok) s_w += (double)(h - l);
    }
    if (conf) {
      // bins, one round per distinct bin among the wave's pixels: the lowest pending lane names the bin, a ballot finds the lanes
      // that share it, their errors are folded by a shuffle tree over the whole wave (other lanes add 0), lane 0 adds the round
      // into the wave's own LDS table.  (The ballot is wave-uniform, so the named lane is read with v_readlane: the first
      // active lane of the pending set.)
      int bin = (int)floorf(cf * (float)kBins);
      bin = bin < 0 ? 0 : (bin > kBins - 1 ? kBins - 1 : bin);
      unsigned long long todo = __ballot(ok);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int b0 = __builtin_amdgcn_readlane(bin, leader);
        const bool mine = ok && bin == b0;
        const unsigned long long same = __ballot(mine);
        const double v = wave_sum(mine ? (double)e : 0.0);
        unsigned u[T];
#pragma unroll
        for (int t = 0; t < T; ++t) u[t] = count(mine && under[t]);
        if (lane == 0) {
          sh.bin_sum[wave][b0] += v;
          sh.bin_cnt[wave][b0][0] += (unsigned)__popcll(same);
#pragma unroll
          for (int t = 0; t < T; ++t) sh.bin_cnt[wave][b0][1 + t] += u[t];
        }
        todo &= ~same;
      }
    }
  }

  s_e = wave_sum(s_e);
  s_w = wave_sum(s_w);
  if (lane == 0) {
    sh.wave_sum[wave][0] = s_e;
    sh.wave_sum[wave][1] = s_w;
    sh.wave_cnt[wave][0] = c_n;
    sh.wave_cnt[wave][1] = c_nf;
    sh.wave_cnt[wave][2] = c_cov;
#pragma unroll
    for (int t = 0; t < T; ++t) sh.wave_cnt[wave][3 + t] = c_under[t];
  }
  __syncthreads();

  // the block's partial table, waves folded in wave order
  double* out = ws + (mm.ws_off[m] + (long long)b * mm.nblk[m] + blockIdx.x) * kTable;
  if (threadIdx.x < kCols) {
    const int c = threadIdx.x;
    double v = 0.0;
    if (c == cSumE || c == cSumWidth) {
      const int k = c == cSumE ? 0 : 1;
      for (int w = 0; w < kWaves; ++w) v += sh.wave_sum[w][k];
    } else {
      const int t = c - cUnder;
      const int k = c == cN ? 0 : c == cNonfinite ? 1 : c == cCovered ? 2 : (t < T ? 3 + t : -1);
      unsigned n = 0;
      if (k >= 0)
        for (int w = 0; w < kWaves; ++w) n += sh.wave_cnt[w][k];
      v = (double)n;
    }
    out[c] = v;
  }
  if (conf) {
    for (int i = threadIdx.x; i < kBins * kCols; i += kT) {
      const int bin = i / kCols, c = i - bin * kCols;
      double v = 0.0;
      if (c == cSumE) {
        for (int w = 0; w < kWaves; ++w) v += sh.bin_sum[w][bin];
      } else if (c == cN || (c >= cUnder && c < cUnder + T)) {
        const int k = c == cN ? 0 : 1 + (c - cUnder);
        unsigned n = 0;
        for (int w = 0; w < kWaves; ++w) n += sh.bin_cnt[w][bin][k];
        v = (double)n;
      }
      out[kCols + i] = v;
    }
  }
}

// tables[m][row][col] = the block partials of map m added in (batch item, block) order; rows a map has no input for are zero
struct MetricFold {
  long long ws_off[kMaxMaps];
  int nparts[kMaxMaps];             // B * nblk
  int has_conf[kMaxMaps];
};

// One block folds 32 entries of one map's table: the partials are cut into 8 contiguous slices, a thread adds one entry over one slice
// in part order, then the slices are added in slice order.  (The cut depends on the number of partials only.)
constexpr int kFoldEntries = 32, kFoldSlices = 8;

__global__ __launch_bounds__(kFoldEntries * kFoldSlices) void depth_metrics_finalize_kernel(MetricFold mf, const double* __restrict__ ws,
                                                                                            double* __restrict__ tables) {
  __shared__ double part[kFoldSlices][kFoldEntries];
  const int m = blockIdx.x, lane = threadIdx.x % kFoldEntries, slice = threadIdx.x / kFoldEntries;
  const int t = blockIdx.y * kFoldEntries + lane;
  double v = 0.0;
  if (t < kTable && (t < kCols || mf.has_conf[m])) {
    const int n = mf.nparts[m], chunk = (n + kFoldSlices - 1) / kFoldSlices;
    const int k0 = slice * chunk, k1 = k0 + chunk < n ? k0 + chunk : n;
    const double* p = ws + mf.ws_off[m] * kTable + t;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) v += p[(long long)k * kTable];
  }
  part[slice][lane] = v;
  __syncthreads();
  if (slice == 0 && t < kTable) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < kFoldSlices; ++j) r += part[j][lane];
    tables[(long long)m * kTable + t] = r;
  }
}

int grid_x(long long per_batch) {
  long long g = (per_batch + 2 * kT - 1) / (2 * kT);
  return (int)(g < 1 ? 1 : (g > 512 ? 512 : g));
}

// the launch geometry of a set of maps: grid x, per map the blocks that do work and the first partial table; returns the tables in all
long long plan(const long long* per_batch, int nmaps, int B, int* gx_out, int* nblk, long long* ws_off) {
  long long big = 0;
  for (int i = 0; i < nmaps; ++i) big = per_batch[i] > big ? per_batch[i] : big;
  const int gx = grid_x(big);
  long long total = 0;
  for (int i = 0; i < nmaps; ++i) {
    const long long need = (per_batch[i] + kT - 1) / kT;
    const int nb = (int)(need < gx ? need : gx);
    if (nblk) nblk[i] = nb;
    if (ws_off) ws_off[i] = total;
    total += (long long)B * nb;
  }
  if (gx_out) *gx_out = gx;
  return total;
}

bool shapes_ok(const long long* per_batch, int nmaps, int B) {
  if (!per_batch || nmaps < 1 || nmaps > kMaxMaps || B < 1 || B > 65535) return false;
  for (int i = 0; i < nmaps; ++i)
    if (per_batch[i] < 1 || per_batch[i] > 0x7fffffffll) return false;
  return true;
}

}  // namespace

extern "C" int64_t mdf_depth_metrics_workspace(const long long* per_batch, int nmaps, int B) {
  if (!shapes_ok(per_batch, nmaps, B)) {
    mdf::set_error("mdf_depth_metrics_workspace: bad shape (1..%d maps of 1..2^31-1 pixels, B in 1..65535)", kMaxMaps);
    return MDF_EARG;
  }
  return (int64_t)plan(per_batch, nmaps, B, nullptr, nullptr, nullptr) * kTable * (int64_t)sizeof(double);
}

extern "C" int mdf_depth_metrics_reduce_multi(const float* const* est, const float* const* gt, const float* const* hypos, const int* hypos_D,
                                              const int* hypos_per_pixel, const float* const* conf, const long long* per_batch, int nmaps,
                                              const void* floor_, int floor_f64, int floor_stride, const float* thr, int T, int B,
                                              void* workspace, long long workspace_bytes, void* stream) {
  MDF_REQUIRE(est && gt && hypos && hypos_D && hypos_per_pixel && conf && per_batch && floor_ && thr && workspace, "null pointer argument");
  MDF_REQUIRE(shapes_ok(per_batch, nmaps, B), "bad shape (1..%d maps of 1..2^31-1 pixels, B in 1..65535)", kMaxMaps);
  MDF_REQUIRE(T >= 1 && T <= kMaxThr && floor_stride >= 0, "bad argument (1..%d thresholds)", kMaxThr);
  MetricMaps mm{};
  int gx = 1;
  const long long total = plan(per_batch, nmaps, B, &gx, mm.nblk, mm.ws_off);
  MDF_REQUIRE(workspace_bytes >= total * kTable * (long long)sizeof(double), "workspace of %lld bytes, need %lld", workspace_bytes,
              total * kTable * (long long)sizeof(double));
  for (int i = 0; i < nmaps; ++i) {
    MDF_REQUIRE(est[i] && gt[i], "null est / gt of map %d", i);
    MDF_REQUIRE(!hypos[i] || hypos_D[i] >= 1, "map %d: hypotheses with D = %d", i, hypos_D[i]);
    mm.est[i] = est[i]; mm.gt[i] = gt[i]; mm.hypos[i] = hypos[i]; mm.conf[i] = conf[i];
    mm.per_batch[i] = per_batch[i];
    mm.D[i] = hypos[i] ? hypos_D[i] : 1;
    mm.per_pixel[i] = hypos[i] ? (hypos_per_pixel[i] != 0) : 0;
  }
  const dim3 grid(gx, B, nmaps), block(kT);
  double* ws = static_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  switch (T) {
    case 1: hipLaunchKernelGGL(depth_metrics_reduce_multi_kernel<1>, grid, block, 0, st, mm, floor_, floor_f64, floor_stride, thr, ws); break;
    case 2: hipLaunchKernelGGL(depth_metrics_reduce_multi_kernel<2>, grid, block, 0, st, mm, floor_, floor_f64, floor_stride, thr, ws); break;
    case 3: hipLaunchKernelGGL(depth_metrics_reduce_multi_kernel<3>, grid, block, 0, st, mm, floor_, floor_f64, floor_stride, thr, ws); break;
    default: hipLaunchKernelGGL(depth_metrics_reduce_multi_kernel<4>, grid, block, 0, st, mm, floor_, floor_f64, floor_stride, thr, ws); break;
  }
  return mdf::check_launch("depth_metrics_reduce_multi_kernel");
}

extern "C" int mdf_depth_metrics_finalize(const void* workspace, long long workspace_bytes, const long long* per_batch, int nmaps, int B,
                                          int conf_mask, double* tables, void* stream) {
  MDF_REQUIRE(workspace && tables, "null pointer argument");
  MDF_REQUIRE(shapes_ok(per_batch, nmaps, B), "bad shape (1..%d maps of 1..2^31-1 pixels, B in 1..65535)", kMaxMaps);
  MetricFold mf{};
  int nblk[kMaxMaps];
  const long long total = plan(per_batch, nmaps, B, nullptr, nblk, mf.ws_off);
  MDF_REQUIRE(workspace_bytes >= total * kTable * (long long)sizeof(double), "workspace of %lld bytes, need %lld", workspace_bytes,
              total * kTable * (long long)sizeof(double));
  for (int i = 0; i < nmaps; ++i) {
    mf.nparts[i] = B * nblk[i];
    mf.has_conf[i] = (conf_mask >> i) & 1;
  }
  hipLaunchKernelGGL(depth_metrics_finalize_kernel, dim3(nmaps, (kTable + kFoldEntries - 1) / kFoldEntries), dim3(kFoldEntries * kFoldSlices), 0,
                     (hipStream_t)stream, mf, static_cast<const double*>(workspace),
                     tables);
  return mdf::check_launch("depth_metrics_finalize_kernel");
}
