// The spatial index of the point-cloud files (point_index.h states its layout), all fp64 and exact, and the sort every one of
// them shares:
//   index      pts_bbox_kernel / pts_bbox_final_kernel (bounding box), pts_morton_kernel (63-bit Morton keys over the box),
//              a stable LSD radix sort (8 passes of 8 bits: pts_sort_hist_kernel, pts_sort_scan_kernel, pts_sort_scatter_kernel;
//              ties keep the input order), pts_gather_kernel (points in key order), pts_leaf_kernel + pts_node_kernel (an implicit
//              binary tree of fp64 AABBs over fixed leaves of kLeaf sorted points, built bottom-up; heap numbering, root 1, leaf
//              l at node P + l, P = leaves rounded up to a power of two, empty nodes hold an inverted box).
//   shared     launch_bbox, sort_pairs and scan_counts launch the bounding-box, sort and scan kernels for the other point files,
//              so each of those kernels exists once.
// No float atomics; the only atomics are the integer counters of the per-block LDS histograms.
#include "point_index.h"

using namespace mdf::pts;

namespace {

// ---------------------------------------------------------------------------------------------------- bounding box
__global__ __launch_bounds__(kBlock) void pts_bbox_kernel(const double* __restrict__ pts, long long n, double* __restrict__ part) {
  __shared__ double red[6][kBlock];
  double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    for (int a = 0; a < 3; ++a) {
      const double x = pts[i * 3 + a];
      v[a] = fmin(v[a], x);
      v[3 + a] = fmax(v[3 + a], x);
    }
  }
  mdf::block_fold(v, red, [](int a, double x, double y) { return a < 3 ? fmin(x, y) : fmax(x, y); });
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void pts_bbox_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ bbox) {
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    double v = a < 3 ? INFINITY : -INFINITY;
    for (int b = 0; b < nparts; ++b) v = a < 3 ? fmin(v, part[b * 6 + a]) : fmax(v, part[b * 6 + a]);
    bbox[a] = v;
  }
}

// ---------------------------------------------------------------------------------------------------- Morton keys
__device__ __forceinline__ unsigned long long spread3(unsigned long long v) {     // 21 bits -> every third bit of 63
  v &= 0x1fffffull;
  v = (v | (v << 32)) & 0x1f00000000ffffull;
  v = (v | (v << 16)) & 0x1f0000ff0000ffull;
  v = (v | (v << 8)) & 0x100f00f00f00f00full;
  v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}

__device__ __forceinline__ unsigned long long quant21(double x, double lo, double hi) {
  const double ext = hi - lo;
  if (!(ext > 0.0)) return 0;
  const double t = (x - lo) / ext * 2097151.0;
  if (!(t > 0.0)) return 0;                         // also NaN
  return t >= 2097151.0 ? 2097151ull : (unsigned long long)t;
}

__global__ __launch_bounds__(kBlock) void pts_morton_kernel(const double* __restrict__ pts, long long n, const double* __restrict__ bbox,
                                                            unsigned long long* __restrict__ keys, int* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned long long qx = quant21(pts[i * 3 + 0], bbox[0], bbox[3]);
  const unsigned long long qy = quant21(pts[i * 3 + 1], bbox[1], bbox[4]);
  const unsigned long long qz = quant21(pts[i * 3 + 2], bbox[2], bbox[5]);
  keys[i] = (spread3(qx) << 2) | (spread3(qy) << 1) | spread3(qz);
  vals[i] = (int)i;
}

// ---------------------------------------------------------------------------------------------------- stable LSD radix sort
// Tile t holds keys [t*kTile, (t+1)*kTile).  hist[d][t] = keys of digit d in tile t; the exclusive scan of hist in that
// (digit-major) order is where tile t's digit-d keys start; the scatter walks each tile in input order, 256 keys at a time.
__global__ __launch_bounds__(kBlock) void pts_sort_hist_kernel(const unsigned long long* __restrict__ keys, long long n, int shift,
                                                               long long ntiles, int* __restrict__ hist) {
  __shared__ int cnt[kRadix];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kTile;
  for (int k = 0; k < kSortItems; ++k) {
    const long long i = base + k * kBlock + threadIdx.x;
    if (i < n) atomicAdd(&cnt[(keys[i] >> shift) & 255u], 1);
  }
  __syncthreads();
  hist[(long long)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(kScanThreads) void pts_sort_scan_kernel(const int* __restrict__ counts, long long nitems,
                                                                     long long* __restrict__ offsets, long long* __restrict__ total) {
  mdf::block_exclusive_scan<long long, false>(counts, nitems, offsets, total);
}

__global__ __launch_bounds__(kBlock) void pts_sort_scatter_kernel(const unsigned long long* __restrict__ kin, const int* __restrict__ vin,
                                                                  long long n, int shift, long long ntiles, const long long* __restrict__ hoff,
                                                                  unsigned long long* __restrict__ kout, int* __restrict__ vout) {
  constexpr int kWaves = kBlock / 64;
  __shared__ long long run[kRadix];
  __shared__ int wcnt[kWaves][kRadix];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  run[t] = hoff[(long long)t * ntiles + blockIdx.x];
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long long base = (long long)blockIdx.x * kTile;
  for (int k = 0; k < kSortItems; ++k) {
    for (int w = 0; w < kWaves; ++w) wcnt[w][t] = 0;
    __syncthreads();
    const long long i = base + k * kBlock + t;
    const bool valid = i < n;
    const unsigned long long key = valid ? kin[i] : 0ull;
    const unsigned d = valid ? (unsigned)((key >> shift) & 255u) : 256u;
    // lanes of this wave with the same digit (invalid lanes match only each other)
    unsigned long long match = __ballot(valid);
    if (!valid) match = ~match;
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bb = __ballot((d >> b) & 1u);
      match &= ((d >> b) & 1u) ? bb : ~bb;
    }
    const int rank = __popcll(match & lt);
    if (valid && (match >> lane) == 1ull) wcnt[wave][d] = __popcll(match);      // highest lane of its group
    __syncthreads();
    if (valid) {
      long long pos = run[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      kout[pos] = key;
      vout[pos] = vin[i];
    }
    __syncthreads();
    int add = 0;
    for (int w = 0; w < kWaves; ++w) add += wcnt[w][t];
    run[t] += add;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void pts_gather_kernel(const double* __restrict__ pts, const int* __restrict__ order, long long n,
                                                            double* __restrict__ out, int* __restrict__ perm) {
  const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  const long long i = order[s];
  out[s * 3 + 0] = pts[i * 3 + 0];
  out[s * 3 + 1] = pts[i * 3 + 1];
  out[s * 3 + 2] = pts[i * 3 + 2];
  perm[s] = (int)i;
}

// ---------------------------------------------------------------------------------------------------- tree
__global__ __launch_bounds__(kBlock) void pts_leaf_kernel(const double* __restrict__ pts, long long n, long long P, double* __restrict__ nodes) {
  const long long l = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (l >= P) return;
  double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const long long lo = l * kLeaf, hi = min(n, lo + kLeaf);
  for (long long j = lo; j < hi; ++j)
    for (int a = 0; a < 3; ++a) {
      v[a] = fmin(v[a], pts[j * 3 + a]);
      v[3 + a] = fmax(v[3 + a], pts[j * 3 + a]);
    }
  double* o = nodes + (P + l) * 6;
  for (int a = 0; a < 6; ++a) o[a] = v[a];
}

// nodes [first, first + count) of one level from their children
__global__ __launch_bounds__(kBlock) void pts_node_kernel(double* __restrict__ nodes, long long first, long long count) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  const long long v = first + k;
  const double* a = nodes + 2 * v * 6;
  const double* b = a + 6;
  double* o = nodes + v * 6;
  for (int c = 0; c < 3; ++c) {
    o[c] = fmin(a[c], b[c]);
    o[3 + c] = fmax(a[3 + c], b[3 + c]);
  }
}

}  // namespace

extern "C" long long mdf_pts_index_workspace(long long n) {
  if (n < 0 || n >= (1ll << 31) - kTile) return 0;
  return index_layout(nullptr, n).bytes;
}

int mdf::pts::launch_bbox(const double* pts, long long n, const SortBuffers& S, hipStream_t s) {
  const int nbb = (int)std::min<long long>(kBboxBlocks, (n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(pts_bbox_kernel, dim3(nbb), dim3(kBlock), 0, s, pts, n, S.bbox_part);
  if (int rc = mdf::check_launch("pts_bbox_kernel")) return rc;
  hipLaunchKernelGGL(pts_bbox_final_kernel, dim3(1), dim3(64), 0, s, S.bbox_part, nbb, S.bbox);
  return mdf::check_launch("pts_bbox_final_kernel");
}

int mdf::pts::scan_counts(const int* counts, long long nitems, long long* offsets, long long* total, hipStream_t s) {
  hipLaunchKernelGGL(pts_sort_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, counts, nitems, offsets, total);
  return mdf::check_launch("pts_sort_scan_kernel");
}

int mdf::pts::sort_pairs(const SortBuffers& S, long long n, long long ntiles, hipStream_t s) {
  unsigned long long *kin = S.key0, *kout = S.key1;
  int *vin = S.val0, *vout = S.val1;
  for (int shift = 0; shift < 64; shift += 8) {
    hipLaunchKernelGGL(pts_sort_hist_kernel, dim3((unsigned)ntiles), dim3(kBlock), 0, s, kin, n, shift, ntiles, S.hist);
    if (int rc = mdf::check_launch("pts_sort_hist_kernel")) return rc;
    if (int rc = scan_counts(S.hist, kRadix * ntiles, S.hoff, nullptr, s)) return rc;
    hipLaunchKernelGGL(pts_sort_scatter_kernel, dim3((unsigned)ntiles), dim3(kBlock), 0, s, kin, vin, n, shift, ntiles, S.hoff, kout, vout);
    if (int rc = mdf::check_launch("pts_sort_scatter_kernel")) return rc;
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
  return MDF_OK;     // an even number of passes: the sorted pairs are in key0 / val0
}

extern "C" int mdf_pts_index_build(const double* pts, long long n, void* index, long long index_bytes, void* stream) {
  MDF_REQUIRE(pts || n == 0, "null pointer argument: pts");
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  const IndexLayout L = index_layout(index, n);
  const SortBuffers& S = L.sort;
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    if (int rc = launch_bbox(pts, n, S, s)) return rc;
    hipLaunchKernelGGL(pts_morton_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, pts, n, S.bbox, S.key0, S.val0);
    if (int rc = mdf::check_launch("pts_morton_kernel")) return rc;
    if (int rc = sort_pairs(S, n, L.ntiles, s)) return rc;
    hipLaunchKernelGGL(pts_gather_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, pts, S.val0, n, L.pts, L.perm);
    if (int rc = mdf::check_launch("pts_gather_kernel")) return rc;
  }
  hipLaunchKernelGGL(pts_leaf_kernel, dim3(grid_of(L.P)), dim3(kBlock), 0, s, L.pts, n, L.P, L.nodes);
  if (int rc = mdf::check_launch("pts_leaf_kernel")) return rc;
  for (long long first = L.P / 2; first >= 1; first /= 2) {
    hipLaunchKernelGGL(pts_node_kernel, dim3(grid_of(first)), dim3(kBlock), 0, s, L.nodes, first, first);
    if (int rc = mdf::check_launch("pts_node_kernel")) return rc;
  }
  return MDF_OK;
}
