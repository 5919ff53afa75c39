// DTU point-cloud evaluation (the reference's MATLAB scorer: reducePts_haa.m, MaxDistCP.m and the masks of PointCompareMain.m),
// all fp64 and exact, on the index of point_index.hip:
//   nn         pts_nn_kernel: the region test, then nn_walk<false>: one query per lane, nearest child first, a subtree is skipped
//              when its box distance^2 is >= min(best^2, cap2); cap2 is the least double whose square root is >= cap, so
//              "d < cap" <=> "d^2 < cap2" exactly.
//   reduce     pts_rank_kernel, pts_radius_kernel<false> (earlier neighbours within dst per point: the greatest double whose
//              square root is <= dst bounds d^2, so "d <= dst" is decided exactly), pts_sort_scan_kernel (exclusive scan, int64),
//              pts_radius_kernel<true> (the same walk places the CSR), pts_reduce_init_kernel, then rounds of
//              pts_reduce_round_kernel + pts_reduce_step_kernel: an undecided point becomes OUT when an earlier neighbour is IN and IN when all of them are
//              OUT, reading the statuses of the previous round only (Jacobi), so the round count is run-independent too;
//              pts_reduce_keep_kernel writes the keep mask.  The result is the sequential greedy result of the visiting order.
//   masks      pts_dtu_masks_kernel: the ObsMask lookup (MATLAB round, 1-based column-major) and the ground-plane test.
// Distances: d^2 = ((dx*dx) + dy*dy) + dz*dz, no contraction (the library builds with -ffp-contract=off; point_index.h pins it).
// No float atomics; the only atomic is an integer counter (the undecided count of a round).
#include "point_index.h"

using namespace mdf::pts;

namespace {

constexpr int kCtl = 4;                      // reduce control words: rounds done, undecided after it, accumulator, spare

struct Region {          // MaxDistCP's cubes: on axis a, [fl(lo_a + k*cap), fl(fl(lo_a + k*cap) + cap)) for k = 0..range_a
  int use;
  double lo[3];
  long long range[3];
};

__device__ __forceinline__ bool in_axis(double f, double lo, long long range, double cap) {
  const double k0 = floor(__ddiv_rn(__dsub_rn(f, lo), cap));
  if (!(k0 >= -1.0 && k0 <= (double)range + 1.0)) return false;     // also NaN
  for (long long k = (long long)k0 - 1; k <= (long long)k0 + 1; ++k) {
    if (k < 0 || k > range) continue;
    const double low = __dadd_rn(lo, __dmul_rn((double)k, cap));
    const double high = __dadd_rn(low, cap);
    if (f >= low && f < high) return true;
  }
  return false;
}

struct NnArgs {
  const double* pts;       // index points (key order)
  const double* nodes;
  long long n, P;
  const double* q;         // queries [m][3]
  const int* qperm;        // result position of query i (nullable: i)
  long long m;
  Region reg;
  double cap, cap2;
  double* dist;
  int* visits;             // nullable
};

__global__ __launch_bounds__(kBlock) void pts_nn_kernel(const NnArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.m) return;
  const double qx = a.q[i * 3 + 0], qy = a.q[i * 3 + 1], qz = a.q[i * 3 + 2];
  const long long out = a.qperm ? (long long)a.qperm[i] : i;
  double best = INFINITY;
  int visits = 0, bidx = 0;
  const bool inside = !a.reg.use || (in_axis(qx, a.reg.lo[0], a.reg.range[0], a.cap) && in_axis(qy, a.reg.lo[1], a.reg.range[1], a.cap) &&
                                     in_axis(qz, a.reg.lo[2], a.reg.range[2], a.cap));
  if (inside && a.n > 0) visits = nn_walk<false>(a.pts, nullptr, a.nodes, a.n, a.P, qx, qy, qz, a.cap2, best, bidx);
  a.dist[out] = best < a.cap2 ? sqrt(best) : a.cap;
  if (a.visits) a.visits[out] = visits;
}

// ---------------------------------------------------------------------------------------------------- reduce
struct ReduceLayout {
  int* rank_s;             // [n] rank of key-order point s
  int* count;              // [n] earlier-rank neighbours
  long long* offs;         // [n + 1] CSR offsets (offs[n] = edges)
  unsigned char *st0, *st1;  // [n] statuses: 0 undecided, 1 IN, 2 OUT
  int* cursor;             // [n] CSR entries known OUT so far
  int* ctl;                // [kCtl]
  long long bytes;
};

ReduceLayout reduce_layout(char* base, long long n) {
  ReduceLayout R{};
  Arena a{base};
  R.rank_s = a.take<int>(n);
  R.count = a.take<int>(n);
  R.offs = a.take<long long>(n + 1);
  R.st0 = a.take<unsigned char>(n);
  R.st1 = a.take<unsigned char>(n);
  R.cursor = a.take<int>(n);
  R.ctl = a.take<int>(kCtl);
  R.bytes = a.used;
  return R;
}

__global__ __launch_bounds__(kBlock) void pts_rank_kernel(const int* __restrict__ rank, const int* __restrict__ perm, long long n,
                                                          int* __restrict__ rank_s) {
  const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (s < n) rank_s[s] = rank[perm[s]];
}

struct RadiusArgs {
  const double* pts;
  const double* nodes;
  const int* perm;
  const int* rank_s;
  long long n, P;
  double lim;              // the greatest double whose square root is <= dst
  int* count;
  const long long* offs;   // place pass only
  int* csr;
  long long capacity;
};

// j precedes s in the visiting order: (rank, input index) ordered lexicographically, so any rank array gives a strict order
__device__ __forceinline__ bool earlier(const RadiusArgs& a, long long j, int rs, int ps) {
  const int rj = a.rank_s[j];
  return rj < rs || (rj == rs && a.perm[j] < ps);
}

template <bool kPlace>
__global__ __launch_bounds__(kBlock) void pts_radius_kernel(const RadiusArgs a) {
  const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (s >= a.n) return;
  const double qx = a.pts[s * 3 + 0], qy = a.pts[s * 3 + 1], qz = a.pts[s * 3 + 2];
  const int rs = a.rank_s[s], ps = a.perm[s];
  long long at = kPlace ? a.offs[s] : 0;
  int c = 0;
  int stack[kStack];
  int sp = 0;
  long long node = 1;
  bool have = box_dist2(a.nodes + 6, qx, qy, qz) <= a.lim;
  while (have) {
    if (node >= a.P) {
      const long long lo = (node - a.P) * kLeaf, hi = min(a.n, lo + kLeaf);
      for (long long j = lo; j < hi; ++j) {
        if (j == s) continue;
        const double d2 = dist2(a.pts[j * 3 + 0], a.pts[j * 3 + 1], a.pts[j * 3 + 2], qx, qy, qz);
        if (d2 <= a.lim && earlier(a, j, rs, ps)) {
          if (kPlace) {
            if (at < a.capacity) a.csr[at] = (int)j;
            ++at;
          }
          ++c;
        }
      }
    } else {
      const long long c0 = 2 * node, c1 = c0 + 1;
      const bool v0 = box_dist2(a.nodes + c0 * 6, qx, qy, qz) <= a.lim, v1 = box_dist2(a.nodes + c1 * 6, qx, qy, qz) <= a.lim;
      if (v1 && sp < kStack) stack[sp++] = (int)c1;
      if (v0) { node = c0; continue; }
    }
    have = sp > 0;
    if (have) node = stack[--sp];
  }
  if (!kPlace) a.count[s] = c;
}

// ctl[3] = 1 when the CSR did not fit: no round runs then.
__global__ __launch_bounds__(kBlock) void pts_reduce_init_kernel(unsigned char* __restrict__ st0, int* __restrict__ cursor, long long n,
                                                                 const long long* __restrict__ offs, long long capacity,
                                                                 int* __restrict__ ctl) {
  const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (s < n) {
    st0[s] = 0;
    cursor[s] = 0;
  }
  if (s == 0) {
    const bool fits = offs[n] <= capacity;
    ctl[0] = 0;
    ctl[1] = n > 0 && fits ? 1 : 0;
    ctl[2] = 0;
    ctl[3] = fits ? 0 : 1;
  }
}

// One round: statuses of round ctl[0] in (ctl[0] even ? st0 : st1), the next round's in the other.  A no-op once ctl[1] == 0.
__global__ __launch_bounds__(kBlock) void pts_reduce_round_kernel(unsigned char* __restrict__ st0, unsigned char* __restrict__ st1,
                                                                  const long long* __restrict__ offs, const int* __restrict__ csr,
                                                                  int* __restrict__ cursor, long long n, long long capacity,
                                                                  int* __restrict__ ctl) {
  if (ctl[1] == 0) return;
  const bool even = (ctl[0] & 1) == 0;
  const unsigned char* cur = even ? st0 : st1;
  unsigned char* nxt = even ? st1 : st0;
  const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
  int undecided = 0;
  if (s < n) {
    unsigned char st = cur[s];
    if (st == 0) {
      const long long e = min(offs[s + 1], capacity), b = min(offs[s], e);     // (a no-op clamp after mdf_pts_reduce_count)
      long long k = b + cursor[s];
      bool prefix = true, any_in = false;
      for (long long q = k; q < e; ++q) {
        const int j = csr[q];
        const unsigned char sj = (unsigned)j < (unsigned long long)n ? cur[j] : 0;
        if (sj == 1) { any_in = true; break; }
        if (sj == 2) { if (prefix) k = q + 1; }
        else prefix = false;
      }
      if (any_in) st = 2;
      else if (k == e) st = 1;
      else {
        cursor[s] = (int)(k - b);
        undecided = 1;
      }
    }
    nxt[s] = st;
  }
  const int u = __syncthreads_count(undecided);
  if (threadIdx.x == 0 && u) atomicAdd(&ctl[2], u);
}

__global__ __launch_bounds__(64) void pts_reduce_step_kernel(int* __restrict__ ctl) {
  if (threadIdx.x == 0 && ctl[1] != 0) {
    ctl[0] += 1;
    ctl[1] = ctl[2];
    ctl[2] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void pts_reduce_keep_kernel(const unsigned char* __restrict__ st0, const unsigned char* __restrict__ st1,
                                                                 const int* __restrict__ perm, long long n, const int* __restrict__ ctl,
                                                                 unsigned char* __restrict__ keep, int* __restrict__ state) {
  const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned char* cur = (ctl[0] & 1) == 0 ? st0 : st1;
  if (s < n) keep[perm[s]] = cur[s] == 1 ? 1 : 0;
  if (s == 0 && state) {
    state[0] = ctl[0];
    state[1] = ctl[1];
    state[2] = ctl[3];
  }
}

// ---------------------------------------------------------------------------------------------------- masks
struct MaskArgs {
  const double* q;
  long long n;
  const unsigned char* obs;
  long long s1, s2, s3;
  double bb[3];
  double res;
  unsigned char* in_mask;
  const double* stl;
  long long m;
  double plane[4];
  unsigned char* above;
};

__device__ __forceinline__ double matlab_index(double x, double lo, double res) {
  return round(__dadd_rn(__ddiv_rn(__dsub_rn(x, lo), res), 1.0));      // round(): halves away from zero, as MATLAB's
}

__global__ __launch_bounds__(kBlock) void pts_dtu_masks_kernel(const MaskArgs a) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < a.n) {
    const double v1 = matlab_index(a.q[i * 3 + 0], a.bb[0], a.res);
    const double v2 = matlab_index(a.q[i * 3 + 1], a.bb[1], a.res);
    const double v3 = matlab_index(a.q[i * 3 + 2], a.bb[2], a.res);
    bool in = v1 > 0.0 && v1 <= (double)a.s1 && v2 > 0.0 && v2 <= (double)a.s2 && v3 > 0.0 && v3 <= (double)a.s3;
    if (in) {
      const long long idx = ((long long)v1 - 1) + ((long long)v2 - 1) * a.s1 + ((long long)v3 - 1) * a.s1 * a.s2;
      in = a.obs[idx] != 0;
    }
    a.in_mask[i] = in ? 1 : 0;
  }
  if (i < a.m) {
    const double x = a.stl[i * 3 + 0], y = a.stl[i * 3 + 1], z = a.stl[i * 3 + 2];
    const double p = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.plane[0], x), __dmul_rn(a.plane[1], y)), __dmul_rn(a.plane[2], z)),
                               a.plane[3]);
    a.above[i] = p > 0.0 ? 1 : 0;
  }
}

}  // namespace

extern "C" int mdf_pts_nn_dist(const void* index, long long n, long long index_bytes, const void* qindex, const double* queries, long long m,
                               long long qindex_bytes, const double* bb, double cap, double* dist, int* visits, void* stream) {
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  MDF_REQUIRE(dist || m == 0, "null pointer argument: dist");
  Queries Q{};
  if (int rc = resolve_queries(qindex, queries, m, qindex_bytes, &cap, &Q)) return rc;
  if (m == 0) return MDF_OK;
  const IndexLayout L = index_layout(index, n);
  NnArgs a{};
  a.pts = L.pts; a.nodes = L.nodes; a.n = n; a.P = L.P; a.m = m;
  a.q = Q.q;
  a.qperm = Q.qperm;
  a.reg.use = bb != nullptr;
  if (bb) {
    for (int k = 0; k < 3; ++k) {
      MDF_REQUIRE(std::isfinite(bb[k]) && std::isfinite(bb[3 + k]) && bb[3 + k] >= bb[k], "bad bounding box on axis %d", k);
      const double r = std::floor((bb[3 + k] - bb[k]) / cap);
      MDF_REQUIRE(r < 1e9, "bounding box too large for cap %g", cap);
      a.reg.lo[k] = bb[k];
      a.reg.range[k] = (long long)r;
    }
  }
  a.cap = cap;
  a.cap2 = sqrt_ge_bound(cap);
  a.dist = dist;
  a.visits = visits;
  hipLaunchKernelGGL(pts_nn_kernel, dim3(grid_of(m)), dim3(kBlock), 0, (hipStream_t)stream, a);
  return mdf::check_launch("pts_nn_kernel");
}

extern "C" long long mdf_pts_reduce_workspace(long long n) {
  if (n < 0 || n >= (1ll << 31)) return 0;
  return reduce_layout(nullptr, n).bytes;
}

static int check_reduce_args(const void* index, long long n, long long index_bytes, const int* rank, double dst, const void* workspace,
                             long long ws_bytes) {
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  MDF_REQUIRE(rank || n == 0, "null pointer argument: rank");
  MDF_REQUIRE(workspace, "null pointer argument: workspace");
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
  MDF_REQUIRE(std::isfinite(dst) && dst > 0, "dst=%g must be finite and > 0", dst);
  const long long need = reduce_layout(nullptr, n).bytes;
  MDF_REQUIRE(ws_bytes >= need, "workspace too small: %lld bytes, %lld needed", ws_bytes, need);
  return MDF_OK;
}

extern "C" int mdf_pts_reduce_count(const void* index, long long n, long long index_bytes, const int* rank, double dst, void* workspace,
                                    long long ws_bytes, long long* edges, void* stream) {
  if (int rc = check_reduce_args(index, n, index_bytes, rank, dst, workspace, ws_bytes)) return rc;
  MDF_REQUIRE(edges, "null pointer argument: edges");
  const IndexLayout L = index_layout(index, n);
  const ReduceLayout R = reduce_layout(static_cast<char*>(workspace), n);
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(pts_rank_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, rank, L.perm, n, R.rank_s);
    if (int rc = mdf::check_launch("pts_rank_kernel")) return rc;
    RadiusArgs a{L.pts, L.nodes, L.perm, R.rank_s, n, L.P, sqrt_le_bound(dst), R.count, nullptr, nullptr, 0};
    hipLaunchKernelGGL(pts_radius_kernel<false>, dim3(grid_of(n)), dim3(kBlock), 0, s, a);
    if (int rc = mdf::check_launch("pts_radius_kernel")) return rc;
  }
  if (int rc = scan_counts(R.count, n, R.offs, edges, s)) return rc;
  if (hipMemcpyAsync(R.offs + n, edges, 8, hipMemcpyDeviceToDevice, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemcpyAsync failed");
  return MDF_OK;
}

extern "C" int mdf_pts_reduce(const void* index, long long n, long long index_bytes, const int* rank, double dst, void* workspace,
                              long long ws_bytes, int* csr, long long capacity, int resume, int max_rounds, unsigned char* keep, int* state,
                              void* stream) {
  if (int rc = check_reduce_args(index, n, index_bytes, rank, dst, workspace, ws_bytes)) return rc;
  MDF_REQUIRE(keep || n == 0, "null pointer argument: keep");
  MDF_REQUIRE(csr || capacity == 0, "null pointer argument: csr");
  MDF_REQUIRE(capacity >= 0, "negative capacity");
  MDF_REQUIRE(max_rounds >= 0 && max_rounds <= 1 << 20, "max_rounds=%d out of range", max_rounds);
  const IndexLayout L = index_layout(index, n);
  const ReduceLayout R = reduce_layout(static_cast<char*>(workspace), n);
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = grid_of(std::max(n, 1ll));
  if (!resume) {
    if (n > 0) {
      RadiusArgs a{L.pts, L.nodes, L.perm, R.rank_s, n, L.P, sqrt_le_bound(dst), R.count, R.offs, csr, capacity};
      hipLaunchKernelGGL(pts_radius_kernel<true>, dim3(g), dim3(kBlock), 0, s, a);
      if (int rc = mdf::check_launch("pts_radius_kernel")) return rc;
    }
    hipLaunchKernelGGL(pts_reduce_init_kernel, dim3(g), dim3(kBlock), 0, s, R.st0, R.cursor, n, R.offs, capacity, R.ctl);
    if (int rc = mdf::check_launch("pts_reduce_init_kernel")) return rc;
  }
  for (int r = 0; r < max_rounds; ++r) {
    hipLaunchKernelGGL(pts_reduce_round_kernel, dim3(g), dim3(kBlock), 0, s, R.st0, R.st1, R.offs, csr, R.cursor, n, capacity, R.ctl);
    if (int rc = mdf::check_launch("pts_reduce_round_kernel")) return rc;
    hipLaunchKernelGGL(pts_reduce_step_kernel, dim3(1), dim3(64), 0, s, R.ctl);
    if (int rc = mdf::check_launch("pts_reduce_step_kernel")) return rc;
  }
  hipLaunchKernelGGL(pts_reduce_keep_kernel, dim3(g), dim3(kBlock), 0, s, R.st0, R.st1, L.perm, n, R.ctl, keep, state);
  return mdf::check_launch("pts_reduce_keep_kernel");
}

extern "C" int mdf_dtu_masks(const double* qdata, long long n, const unsigned char* obs_mask, int s1, int s2, int s3, const double* bb,
                             double res, unsigned char* in_mask, const double* qstl, long long m, const double* plane,
                             unsigned char* above, void* stream) {
  MDF_REQUIRE(n >= 0 && m >= 0 && n < (1ll << 40) && m < (1ll << 40), "negative or too large point count");
  MDF_REQUIRE((qdata && in_mask && obs_mask && bb) || n == 0, "null pointer argument (data side)");
  MDF_REQUIRE((qstl && above && plane) || m == 0, "null pointer argument (stl side)");
  MDF_REQUIRE(s1 >= 0 && s2 >= 0 && s3 >= 0, "negative ObsMask size %dx%dx%d", s1, s2, s3);
  MDF_REQUIRE(n == 0 || (std::isfinite(res) && res > 0), "res=%g must be finite and > 0", res);
  const long long k = std::max(n, m);
  if (k == 0) return MDF_OK;
  MaskArgs a{};
  a.q = qdata; a.n = n; a.obs = obs_mask; a.s1 = s1; a.s2 = s2; a.s3 = s3; a.res = res;
  if (n) for (int i = 0; i < 3; ++i) a.bb[i] = bb[i];
  a.in_mask = in_mask; a.stl = qstl; a.m = m; a.above = above;
  if (m) for (int i = 0; i < 4; ++i) a.plane[i] = plane[i];
  hipLaunchKernelGGL(pts_dtu_masks_kernel, dim3(grid_of(k)), dim3(kBlock), 0, (hipStream_t)stream, a);
  return mdf::check_launch("pts_dtu_masks_kernel");
}
