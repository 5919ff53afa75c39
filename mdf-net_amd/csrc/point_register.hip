// Registration and F-score: the Tanks and Temples protocol's pieces (crop volume, voxel-grid downsampling, point-to-point ICP,
// F-score), all fp64 and exact, on the index, sort and distance helpers of point_index.h:
//   nn         pts_nn_idx_kernel: nn_walk<true>, pts_nn_kernel's walk without a region, which also reports WHICH point was nearest
//              (its input index; ties on d^2 go to the lowest input index, so a subtree at box distance == best is still walked).
//   transform  pts_transform_kernel: x' = ((r00 x + r01 y) + r02 z) + t0, each operation rounded once.
//   crop       pts_crop_kernel: the axis interval and an even-odd crossing count against the polygon.
//   voxel      launch_bbox, pts_vox_key_kernel (3 x 21-bit cell keys, x major), sort_pairs (stable: a cell's points stay in input
//              order), pts_vox_chunk_sum_kernel + pts_sort_scan_kernel + pts_vox_offsets_kernel (a three-pass exclusive scan of the
//              segment heads over many blocks), pts_vox_mean_kernel (one lane per cell: sum in input order, divide).
//   icp        pts_icp_moment_kernel<false> + pts_icp_final_kernel<false> (inlier count, sum of d^2, the two centroids),
//              pts_icp_moment_kernel<true> + pts_icp_final_kernel<true> (the cross-covariance about them).  Every lane sums a fixed
//              strided subset in order, every block folds its lanes with one fixed tree and one block folds the blocks the same
//              way: the shape depends on n only, so the sums are run-independent.  No atomics.
#include "point_index.h"

using namespace mdf::pts;

namespace {

struct NnIdxArgs {
  const double* pts;       // index points (key order)
  const int* perm;         // key-order position -> input index
  const double* nodes;
  long long n, P;
  const double* q;
  const int* qperm;
  long long m;
  double cap, cap2;
  double* dist;            // nullable
  double* d2;              // nullable
  int* nearest;
  int* visits;             // nullable
};

__global__ __launch_bounds__(kBlock) void pts_nn_idx_kernel(const NnIdxArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.m) return;
  const double qx = a.q[i * 3 + 0], qy = a.q[i * 3 + 1], qz = a.q[i * 3 + 2];
  const long long out = a.qperm ? (long long)a.qperm[i] : i;
  double best = INFINITY;
  int bidx = 0x7fffffff;
  const int visits = a.n > 0 ? nn_walk<true>(a.pts, a.perm, a.nodes, a.n, a.P, qx, qy, qz, a.cap2, best, bidx) : 0;
  const bool found = best < a.cap2;
  if (a.dist) a.dist[out] = found ? sqrt(best) : a.cap;
  if (a.d2) a.d2[out] = found ? best : INFINITY;
  a.nearest[out] = found ? bidx : -1;
  if (a.visits) a.visits[out] = visits;
}

struct Affine { double r[12]; };     // rows of [R | t]

__global__ __launch_bounds__(kBlock) void pts_transform_kernel(double* __restrict__ out, const double* __restrict__ pts, long long n,
                                                               const Affine m) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
  for (int a = 0; a < 3; ++a)
    out[i * 3 + a] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m.r[a * 4 + 0], x), __dmul_rn(m.r[a * 4 + 1], y)), __dmul_rn(m.r[a * 4 + 2], z)),
                               m.r[a * 4 + 3]);
}

constexpr int kMaxPoly = 64;

struct CropArgs {
  const double* pts;
  long long n;
  int axis, iu, iv, k;
  double amin, amax;
  double poly[kMaxPoly][2];
  unsigned char* keep;
};

// Edge (i, i+1) crosses the point's v when exactly one end lies below it (vi < y <= vj or vj < y <= vi); its crossing
// u_i + ((y - v_i) / (v_j - v_i)) * (u_j - u_i) counts when it is < x.  Inside = an odd count.
__global__ __launch_bounds__(kBlock) void pts_crop_kernel(const CropArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const double w = a.pts[i * 3 + a.axis], x = a.pts[i * 3 + a.iu], y = a.pts[i * 3 + a.iv];
  int cnt = 0;
  for (int e = 0; e < a.k; ++e) {
    const int f = e + 1 < a.k ? e + 1 : 0;
    const double ui = a.poly[e][0], vi = a.poly[e][1], uj = a.poly[f][0], vj = a.poly[f][1];
    if ((vi < y && vj >= y) || (vj < y && vi >= y)) {
      const double node = __dadd_rn(ui, __dmul_rn(__ddiv_rn(__dsub_rn(y, vi), __dsub_rn(vj, vi)), __dsub_rn(uj, ui)));
      cnt += node < x ? 1 : 0;
    }
  }
  a.keep[i] = (w >= a.amin && w <= a.amax && (cnt & 1)) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------- voxel grid
constexpr int kVoxPer = 4, kVoxChunk = kBlock * kVoxPer;
constexpr double kVoxMaxCell = 2097151.0;     // 2^21 - 1

struct VoxelLayout {
  long long n, ntiles, nchunks;
  SortBuffers sort;
  int* chunk_sums;         // [nchunks] segment heads per chunk
  long long* chunk_off;    // [nchunks]
  int* seg_start;          // [n] first sorted position of segment g
  long long* total;        // [1] segments
  int* ctl;                // [4] ctl[0] = 1: more than 2^21 cells on an axis
  long long bytes;
};

VoxelLayout voxel_layout(char* base, long long n) {
  VoxelLayout L{};
  L.n = n;
  L.ntiles = (n + kTile - 1) / kTile;
  L.nchunks = (n + kVoxChunk - 1) / kVoxChunk;
  Arena a{base};
  L.sort = take_sort_buffers(a, n, L.ntiles);
  L.chunk_sums = a.take<int>(L.nchunks);
  L.chunk_off = a.take<long long>(L.nchunks);
  L.seg_start = a.take<int>(n);
  L.total = a.take<long long>(1);
  L.ctl = a.take<int>(4);
  L.bytes = a.used;
  return L;
}

__device__ __forceinline__ unsigned long long vox_cell(double x, double origin, double v) {
  const double c = floor(__ddiv_rn(__dsub_rn(x, origin), v));
  if (!(c > 0.0)) return 0;                         // also NaN
  return c >= kVoxMaxCell ? 2097151ull : (unsigned long long)c;
}

__global__ __launch_bounds__(kBlock) void pts_vox_key_kernel(const double* __restrict__ pts, long long n, const double* __restrict__ bbox,
                                                             double v, unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                             int* __restrict__ ctl) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double h = __dmul_rn(v, 0.5);
  const double ox = __dsub_rn(bbox[0], h), oy = __dsub_rn(bbox[1], h), oz = __dsub_rn(bbox[2], h);
  if (i == 0) {
    bool fits = true;
    for (int a = 0; a < 3; ++a) {
      const double top = floor(__ddiv_rn(__dsub_rn(bbox[3 + a], __dsub_rn(bbox[a], h)), v));      // the greatest cell index
      fits = fits && top <= kVoxMaxCell;              // false for NaN too
    }
    ctl[0] = fits ? 0 : 1;
  }
  const unsigned long long cx = vox_cell(pts[i * 3 + 0], ox, v), cy = vox_cell(pts[i * 3 + 1], oy, v), cz = vox_cell(pts[i * 3 + 2], oz, v);
  keys[i] = (cx << 42) | (cy << 21) | cz;
  vals[i] = (int)i;
}

__device__ __forceinline__ int vox_head(const unsigned long long* __restrict__ keys, long long s, long long n) {
  if (s >= n) return 0;
  return (s == 0 || keys[s] != keys[s - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void pts_vox_chunk_sum_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                                   int* __restrict__ sums) {
  const long long base = (long long)blockIdx.x * kVoxChunk + threadIdx.x * kVoxPer;
  int t = 0;
  for (int k = 0; k < kVoxPer; ++k) t += vox_head(keys, base + k, n);
  const int sum = mdf::block_sum(t);
  if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kBlock) void pts_vox_offsets_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                                 const long long* __restrict__ chunk_off, int* __restrict__ seg_start) {
  const long long base = (long long)blockIdx.x * kVoxChunk + threadIdx.x * kVoxPer;
  int c[kVoxPer];
  int t = 0;
  for (int k = 0; k < kVoxPer; ++k) {
    c[k] = vox_head(keys, base + k, n);
    t += c[k];
  }
  long long run = chunk_off[blockIdx.x] + (mdf::block_inclusive_scan(t) - t);
  for (int k = 0; k < kVoxPer; ++k) {
    if (c[k]) seg_start[run] = (int)(base + k);          // run < heads in total <= n
    run += c[k];
  }
}

struct VoxMeanArgs {
  const double* pts;
  const double* attrs;     // [n][nattr] or null
  int nattr;
  long long n;
  const int* order;        // sorted position -> input index
  const int* seg_start;
  const long long* total;
  const int* ctl;
  double* out_pts;
  double* out_attrs;
  int* out_count;
  long long* m;
};

__global__ __launch_bounds__(kBlock) void pts_vox_mean_kernel(const VoxMeanArgs a) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long m = *a.total;
  const bool refused = a.ctl[0] != 0;
  if (g == 0) *a.m = refused ? -1 : m;
  if (refused || g >= m) return;
  const long long lo = a.seg_start[g], hi = g + 1 < m ? (long long)a.seg_start[g + 1] : a.n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long s = lo; s < hi; ++s) {
    const long long i = a.order[s];
    s0 = __dadd_rn(s0, a.pts[i * 3 + 0]);
    s1 = __dadd_rn(s1, a.pts[i * 3 + 1]);
    s2 = __dadd_rn(s2, a.pts[i * 3 + 2]);
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (k < a.nattr) t[k] = __dadd_rn(t[k], a.attrs[i * a.nattr + k]);
  }
  const double cnt = (double)(hi - lo);
  a.out_pts[g * 3 + 0] = __ddiv_rn(s0, cnt);
  a.out_pts[g * 3 + 1] = __ddiv_rn(s1, cnt);
  a.out_pts[g * 3 + 2] = __ddiv_rn(s2, cnt);
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (k < a.nattr) a.out_attrs[g * a.nattr + k] = __ddiv_rn(t[k], cnt);
  a.out_count[g] = (int)(hi - lo);
}

// ---------------------------------------------------------------------------------------------------- ICP sums
constexpr int kIcpBlocks = 1024;
constexpr int kIcpVals = 9;

struct IcpArgs {
  const double* src;       // [n][3] transformed source
  const double* tgt;       // [nt][3] target, input order
  const int* nearest;      // [n] target index or -1
  const double* d2;        // [n]
  long long n, nt;
  double lim2;             // d < threshold <=> d2 < lim2
  double* part;            // [kIcpBlocks][kIcpVals]
  double* out;             // [17]: count, sum d2, source centroid, target centroid, H row-major
};

struct IcpAdd {            // the fold is one fixed tree of rounded additions: the sums are pinned bit for bit
  __device__ double operator()(int, double x, double y) const { return __dadd_rn(x, y); }
};

// kCov = false: v = (count, sum d2, sum s, sum t, 0); kCov = true: v = sum (s - cs)(t - ct)^T with the centroids of out[2..8).
template <bool kCov>
__global__ __launch_bounds__(kBlock) void pts_icp_moment_kernel(const IcpArgs a) {
  __shared__ double red[kIcpVals][kBlock];
  double v[kIcpVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (kCov)
    for (int k = 0; k < 6; ++k) c[k] = a.out[2 + k];
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
    const int j = a.nearest[i];
    const double d2 = a.d2[i];
    if (j < 0 || (long long)j >= a.nt || !(d2 < a.lim2)) continue;
    const double sx = a.src[i * 3 + 0], sy = a.src[i * 3 + 1], sz = a.src[i * 3 + 2];
    const double tx = a.tgt[(long long)j * 3 + 0], ty = a.tgt[(long long)j * 3 + 1], tz = a.tgt[(long long)j * 3 + 2];
    if (!kCov) {
      v[0] = __dadd_rn(v[0], 1.0);
      v[1] = __dadd_rn(v[1], d2);
      v[2] = __dadd_rn(v[2], sx); v[3] = __dadd_rn(v[3], sy); v[4] = __dadd_rn(v[4], sz);
      v[5] = __dadd_rn(v[5], tx); v[6] = __dadd_rn(v[6], ty); v[7] = __dadd_rn(v[7], tz);
    } else {
      const double p[3] = {__dsub_rn(sx, c[0]), __dsub_rn(sy, c[1]), __dsub_rn(sz, c[2])};
      const double q[3] = {__dsub_rn(tx, c[3]), __dsub_rn(ty, c[4]), __dsub_rn(tz, c[5])};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) v[r * 3 + s] = __dadd_rn(v[r * 3 + s], __dmul_rn(p[r], q[s]));
    }
  }
  mdf::block_fold(v, red, IcpAdd{});
  if (threadIdx.x < kIcpVals) a.part[(long long)blockIdx.x * kIcpVals + threadIdx.x] = red[threadIdx.x][0];
}

template <bool kCov>
__global__ __launch_bounds__(kBlock) void pts_icp_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
  __shared__ double red[kIcpVals][kBlock];
  double v[kIcpVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nparts; b += kBlock)
    for (int k = 0; k < kIcpVals; ++k) v[k] = __dadd_rn(v[k], part[(long long)b * kIcpVals + k]);
  mdf::block_fold(v, red, IcpAdd{});
  if (threadIdx.x == 0) {
    if (!kCov) {
      const double cnt = red[0][0];
      out[0] = cnt;
      out[1] = red[1][0];
      for (int k = 0; k < 6; ++k) out[2 + k] = cnt > 0.0 ? __ddiv_rn(red[2 + k][0], cnt) : 0.0;
    } else {
      for (int k = 0; k < 9; ++k) out[8 + k] = red[k][0];
    }
  }
}

}  // namespace

extern "C" int mdf_pts_nn(const void* index, long long n, long long index_bytes, const void* qindex, const double* queries, long long m,
                          long long qindex_bytes, double cap, double* dist, double* dist2_out, int* nearest, int* visits, void* stream) {
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  MDF_REQUIRE(nearest || m == 0, "null pointer argument: nearest");
  Queries Q{};
  if (int rc = resolve_queries(qindex, queries, m, qindex_bytes, &cap, &Q)) return rc;
  if (m == 0) return MDF_OK;
  const IndexLayout L = index_layout(index, n);
  NnIdxArgs a{};
  a.pts = L.pts; a.perm = L.perm; a.nodes = L.nodes; a.n = n; a.P = L.P; a.m = m;
  a.q = Q.q;
  a.qperm = Q.qperm;
  a.cap = cap;
  a.cap2 = sqrt_ge_bound(cap);
  a.dist = dist; a.d2 = dist2_out; a.nearest = nearest; a.visits = visits;
  hipLaunchKernelGGL(pts_nn_idx_kernel, dim3(grid_of(m)), dim3(kBlock), 0, (hipStream_t)stream, a);
  return mdf::check_launch("pts_nn_idx_kernel");
}

extern "C" int mdf_pts_transform(double* out, const double* pts, long long n, const double* matrix, void* stream) {
  MDF_REQUIRE(n >= 0 && n < (1ll << 40), "n=%lld points out of range", n);
  MDF_REQUIRE((out && pts) || n == 0, "null pointer argument");
  MDF_REQUIRE(matrix, "null pointer argument: matrix");
  Affine m{};
  for (int k = 0; k < 12; ++k) {
    MDF_REQUIRE(std::isfinite(matrix[k]), "matrix entry %d is not finite", k);
    m.r[k] = matrix[k];
  }
  if (n == 0) return MDF_OK;
  hipLaunchKernelGGL(pts_transform_kernel, dim3(grid_of(n)), dim3(kBlock), 0, (hipStream_t)stream, out, pts, n, m);
  return mdf::check_launch("pts_transform_kernel");
}

extern "C" int mdf_pts_crop(const double* pts, long long n, int axis, double axis_min, double axis_max, const double* polygon, int k,
                            unsigned char* keep, void* stream) {
  MDF_REQUIRE(n >= 0 && n < (1ll << 40), "n=%lld points out of range", n);
  MDF_REQUIRE((pts && keep) || n == 0, "null pointer argument");
  MDF_REQUIRE(axis >= 0 && axis <= 2, "axis=%d must be 0, 1 or 2", axis);
  MDF_REQUIRE(k >= 3 && k <= kMaxPoly, "polygon of k=%d vertices: 3 <= k <= %d", k, kMaxPoly);
  MDF_REQUIRE(polygon, "null pointer argument: polygon");
  MDF_REQUIRE(!std::isnan(axis_min) && !std::isnan(axis_max), "axis_min / axis_max is NaN");
  CropArgs a{};
  a.pts = pts; a.n = n; a.axis = axis; a.k = k; a.amin = axis_min; a.amax = axis_max; a.keep = keep;
  a.iu = axis == 0 ? 1 : 0;
  a.iv = axis == 2 ? 1 : 2;
  for (int e = 0; e < k; ++e) {
    MDF_REQUIRE(std::isfinite(polygon[e * 2]) && std::isfinite(polygon[e * 2 + 1]), "polygon vertex %d is not finite", e);
    a.poly[e][0] = polygon[e * 2];
    a.poly[e][1] = polygon[e * 2 + 1];
  }
  if (n == 0) return MDF_OK;
  hipLaunchKernelGGL(pts_crop_kernel, dim3(grid_of(n)), dim3(kBlock), 0, (hipStream_t)stream, a);
  return mdf::check_launch("pts_crop_kernel");
}

extern "C" long long mdf_pts_voxel_workspace(long long n) {
  if (n < 0 || n >= (1ll << 31) - kTile) return 0;
  return voxel_layout(nullptr, n).bytes;
}

extern "C" int mdf_pts_voxel_downsample(const double* pts, const double* attrs, int nattr, long long n, double voxel, void* workspace,
                                        long long ws_bytes, double* out_pts, double* out_attrs, int* out_count, long long* m,
                                        void* stream) {
  MDF_REQUIRE(n >= 0 && n < (1ll << 31) - kTile, "n=%lld points out of range", n);
  MDF_REQUIRE(std::isfinite(voxel) && voxel > 0, "voxel=%g must be finite and > 0", voxel);
  MDF_REQUIRE(nattr >= 0 && nattr <= 6, "nattr=%d attribute columns: 0..6", nattr);
  MDF_REQUIRE(m, "null pointer argument: m");
  MDF_REQUIRE((pts && out_pts && out_count) || n == 0, "null pointer argument");
  MDF_REQUIRE((attrs && out_attrs) || nattr == 0 || n == 0, "null pointer argument: attrs");
  MDF_REQUIRE(workspace, "null pointer argument: workspace");
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
  const long long need = voxel_layout(nullptr, n).bytes;
  MDF_REQUIRE(ws_bytes >= need, "workspace too small: %lld bytes, %lld needed", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (hipMemsetAsync(m, 0, 8, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemsetAsync failed");
    return MDF_OK;
  }
  const VoxelLayout L = voxel_layout(static_cast<char*>(workspace), n);
  const SortBuffers& S = L.sort;
  if (int rc = launch_bbox(pts, n, S, s)) return rc;
  hipLaunchKernelGGL(pts_vox_key_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, pts, n, S.bbox, voxel, S.key0, S.val0, L.ctl);
  if (int rc = mdf::check_launch("pts_vox_key_kernel")) return rc;
  if (int rc = sort_pairs(S, n, L.ntiles, s)) return rc;
  hipLaunchKernelGGL(pts_vox_chunk_sum_kernel, dim3((unsigned)L.nchunks), dim3(kBlock), 0, s, S.key0, n, L.chunk_sums);
  if (int rc = mdf::check_launch("pts_vox_chunk_sum_kernel")) return rc;
  if (int rc = scan_counts(L.chunk_sums, L.nchunks, L.chunk_off, L.total, s)) return rc;
  hipLaunchKernelGGL(pts_vox_offsets_kernel, dim3((unsigned)L.nchunks), dim3(kBlock), 0, s, S.key0, n, L.chunk_off, L.seg_start);
  if (int rc = mdf::check_launch("pts_vox_offsets_kernel")) return rc;
  VoxMeanArgs a{pts, attrs, nattr, n, S.val0, L.seg_start, L.total, L.ctl, out_pts, out_attrs, out_count, m};
  hipLaunchKernelGGL(pts_vox_mean_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, a);
  return mdf::check_launch("pts_vox_mean_kernel");
}

extern "C" long long mdf_pts_icp_workspace(void) { return align16((long long)kIcpBlocks * kIcpVals * 8); }

extern "C" int mdf_pts_icp_sums(const double* src, long long n, const double* tgt, long long nt, const int* nearest, const double* d2,
                                double threshold, void* workspace, long long ws_bytes, double* out, void* stream) {
  MDF_REQUIRE(n >= 0 && n < (1ll << 40) && nt >= 0 && nt < (1ll << 31), "n=%lld / nt=%lld out of range", n, nt);
  MDF_REQUIRE((src && nearest && d2) || n == 0, "null pointer argument (source side)");
  MDF_REQUIRE(tgt || nt == 0, "null pointer argument: tgt");
  MDF_REQUIRE(out && workspace, "null pointer argument: out / workspace");
  MDF_REQUIRE(std::isfinite(threshold) && threshold > 0, "threshold=%g must be finite and > 0", threshold);
  MDF_REQUIRE(ws_bytes >= mdf_pts_icp_workspace(), "workspace too small: %lld bytes, %lld needed", ws_bytes, mdf_pts_icp_workspace());
  IcpArgs a{src, tgt, nearest, d2, n, nt, sqrt_ge_bound(threshold), static_cast<double*>(workspace), out};
  const int nb = (int)std::max<long long>(1, std::min<long long>(kIcpBlocks, (n + kBlock - 1) / kBlock));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pts_icp_moment_kernel<false>, dim3(nb), dim3(kBlock), 0, s, a);
  if (int rc = mdf::check_launch("pts_icp_moment_kernel")) return rc;
  hipLaunchKernelGGL(pts_icp_final_kernel<false>, dim3(1), dim3(kBlock), 0, s, a.part, nb, out);
  if (int rc = mdf::check_launch("pts_icp_final_kernel")) return rc;
  hipLaunchKernelGGL(pts_icp_moment_kernel<true>, dim3(nb), dim3(kBlock), 0, s, a);
  if (int rc = mdf::check_launch("pts_icp_moment_kernel")) return rc;
  hipLaunchKernelGGL(pts_icp_final_kernel<true>, dim3(1), dim3(kBlock), 0, s, a.part, nb, out);
  return mdf::check_launch("pts_icp_final_kernel");
}
