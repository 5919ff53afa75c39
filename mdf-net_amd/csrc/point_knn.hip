// k-NN and normals: point-cloud post-processing (the reference's Open3D stages: estimate_normals,
// compute_nearest_neighbor_distance), all fp64 and exact, on the index and distance helpers of point_index.h:
//   knn        pts_knn_kernel: one query per lane, the k best (d^2, input index) pairs so far in a list in LDS,
//              laid out [slot][lane] (a wave reads one slot from 64 consecutive words: no bank conflict) and sized k * 64 * 12
//              bytes at launch, so the occupancy follows k.  While the tree is walked the list is unordered: a better candidate
//              overwrites the worst entry and the new worst is found by k independent reads (a sorted insert is a chain of
//              dependent LDS reads and writes, which the whole wave pays whenever one lane accepts a point: 1.5x slower at 49 M points);
//              the list is sorted once, after the walk.  It holds the neighbour's key-order position; its input index
//              is read from perm only when two d^2 are equal.  A subtree is walked while box d^2 <= the list's worst d^2 (<=, not
//              <: an equal distance may still win on the index), nearest child first.  The walk keeps no stack: one bit per level
//              says that the sibling is still to be looked at, and the sibling's box distance is taken again on the way up, so
//              nothing is indexed at run time outside LDS and the kernels use no scratch memory.  A leaf is read in batches of
//              16 points (all their loads issued, then the 16 candidates in order): the walk waits on memory, not on arithmetic.
//   normals    pts_normals_kernel: the same walk over the index's own points, then nine sums over the list in its order, the
//              covariance, six cyclic Jacobi sweeps on registers, the column of the smallest diagonal entry, and the sign.
#include "point_index.h"

using namespace mdf::pts;

namespace {

constexpr int kKnnBlock = 64;                // one wave: every lane owns a column of the list, no barrier
constexpr int kJacobiSweeps = 6;
constexpr int kKnnBatch = 16;                // leaf points whose distances are taken before any of them is looked at

extern __shared__ double knn_lds[];          // [k][64] d^2, then [k][64] int key-order positions

struct KnnWalk {
  const double* pts;
  const int* perm;
  const double* nodes;
  long long n, P;
  int k;
};

// NaN for an empty node, so that every "<=" against it is false
__device__ __forceinline__ double knn_box(const double* __restrict__ b, double x, double y, double z) {
  return b[0] > b[3] ? NAN : box_dist2(b, x, y, z);
}

// The greatest (d^2, input index) of the full list: k independent reads, eight in flight at a time; perm is read on equal d^2 only.
__device__ __forceinline__ void knn_worst(const KnnWalk& a, const double* __restrict__ ld, const int* __restrict__ lj, int lane, double& wd,
                                          int& wi, int& ws) {
  double md = -1.0;                          // every d^2 is >= 0
  int ms = 0, mi = -1;                       // mi < 0: the index of slot ms has not been read yet
  for (int s0 = 0; s0 < a.k; s0 += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld[min(s0 + u, a.k - 1) * kKnnBlock + lane];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int s = s0 + u;
      if (s >= a.k) continue;
      if (v[u] > md) { md = v[u]; ms = s; mi = -1; }
      else if (v[u] == md) {
        if (mi < 0) mi = a.perm[lj[ms * kKnnBlock + lane]];
        const int pi = a.perm[lj[s * kKnnBlock + lane]];
        if (pi > mi) { ms = s; mi = pi; }
      }
    }
  }
  wd = md;
  wi = mi < 0 ? a.perm[lj[ms * kKnnBlock + lane]] : mi;
  ws = ms;
}

// Insertion sort of the first cnt entries by ascending (d^2, input index), once per query.
__device__ __forceinline__ void knn_sort(const KnnWalk& a, double* __restrict__ ld, int* __restrict__ lj, int lane, int cnt) {
  for (int t = 1; t < cnt; ++t) {
    const double d2 = ld[t * kKnnBlock + lane];
    const int j = lj[t * kKnnBlock + lane];
    int pj = -1;
    int s = t;
    while (s > 0) {
      const double pd = ld[(s - 1) * kKnnBlock + lane];
      if (pd < d2) break;
      const int pjk = lj[(s - 1) * kKnnBlock + lane];
      if (pd == d2) {
        if (pj < 0) pj = a.perm[j];
        if (a.perm[pjk] < pj) break;
      }
      ld[s * kKnnBlock + lane] = pd;
      lj[s * kKnnBlock + lane] = pjk;
      --s;
    }
    ld[s * kKnnBlock + lane] = d2;
    lj[s * kKnnBlock + lane] = j;
  }
}

// -> entries in the list (min(k, n)); *visits = leaves looked at
__device__ __forceinline__ int knn_walk(const KnnWalk& a, double qx, double qy, double qz, double* __restrict__ ld, int* __restrict__ lj,
                                        int* visits) {
  const int lane = threadIdx.x;
  int cnt = 0, nvis = 0;
  double wd = INFINITY;                      // the worst entry (and its slot) once the list is full; (+inf, max) before
  int wi = 0x7fffffff, ws = 0;
  if (a.n <= 0) { *visits = 0; return 0; }
  unsigned node = 1, pending = 0;
  bool down = true;
  while (true) {
    if (down) {
      if ((long long)node >= a.P) {          // leaf
        ++nvis;
        const long long lo = ((long long)node - a.P) * kLeaf, hi = min(a.n, lo + kLeaf);
        for (long long j0 = lo; j0 < hi; j0 += kKnnBatch) {
          double bd[kKnnBatch];              // a batch of distances first, so the loads of one batch are in flight together
#pragma unroll
          for (int u = 0; u < kKnnBatch; ++u) {
            const long long j = min(j0 + u, hi - 1);
            bd[u] = dist2(a.pts[j * 3 + 0], a.pts[j * 3 + 1], a.pts[j * 3 + 2], qx, qy, qz);
          }
          unsigned todo = 0;                 // the candidates worth a look: wd only shrinks, so this set only loses members
#pragma unroll
          for (int u = 0; u < kKnnBatch; ++u)
            if (j0 + u < hi && bd[u] <= wd) todo |= 1u << u;
          while (todo) {                     // ascending u; bd[u] by a select chain, not by a run-time index
            const int u = __ffs(todo) - 1;
            todo &= todo - 1;
            double d2 = bd[0];
#pragma unroll
            for (int v = 1; v < kKnnBatch; ++v) d2 = u == v ? bd[v] : d2;
            const long long j = j0 + u;
            if (!(d2 <= wd)) continue;
            if (d2 == wd && a.perm[j] >= wi) continue;
            const int slot = cnt < a.k ? cnt : ws;     // a new slot, or the worst entry's
            ld[slot * kKnnBlock + lane] = d2;
            lj[slot * kKnnBlock + lane] = (int)j;
            if (cnt < a.k) ++cnt;
            if (cnt == a.k) knn_worst(a, ld, lj, lane, wd, wi, ws);
          }
        }
        down = false;
      } else {
        const unsigned c0 = 2 * node, c1 = c0 + 1;
        const double d0 = knn_box(a.nodes + (long long)c0 * 6, qx, qy, qz), d1 = knn_box(a.nodes + (long long)c1 * 6, qx, qy, qz);
        const bool right = d1 < d0;          // false when either is NaN: an empty child is always the right one
        const double dn = right ? d1 : d0, df = right ? d0 : d1;
        if (dn <= wd) {
          node = right ? c1 : c0;
          if (df <= wd) pending |= 1u << (31 - __clz(node));       // the level of the children
        } else {
          down = false;
        }
      }
    } else {
      if (node <= 1) break;
      const unsigned bit = 1u << (31 - __clz(node));
      if (pending & bit) {
        pending &= ~bit;
        const unsigned sib = node ^ 1u;
        if (knn_box(a.nodes + (long long)sib * 6, qx, qy, qz) <= wd) {
          node = sib;
          down = true;
          continue;
        }
      }
      node >>= 1;
    }
  }
  knn_sort(a, ld, lj, lane, cnt);
  *visits = nvis;
  return cnt;
}

struct KnnArgs {
  KnnWalk w;
  const double* q;
  const int* qperm;
  long long m;
  int* nbr;                // [m][k]
  double* d2;              // nullable
  int* visits;             // nullable
};

__global__ __launch_bounds__(kKnnBlock) void pts_knn_kernel(const KnnArgs a) {
  const long long i = (long long)blockIdx.x * kKnnBlock + threadIdx.x;
  if (i >= a.m) return;
  const int lane = threadIdx.x, k = a.w.k;
  double* ld = knn_lds;
  int* lj = reinterpret_cast<int*>(knn_lds + k * kKnnBlock);
  const long long out = a.qperm ? (long long)a.qperm[i] : i;
  int visits;
  const int cnt = knn_walk(a.w, a.q[i * 3 + 0], a.q[i * 3 + 1], a.q[i * 3 + 2], ld, lj, &visits);
  for (int s = 0; s < k; ++s) {
    const bool have = s < cnt;
    a.nbr[out * k + s] = have ? a.w.perm[lj[s * kKnnBlock + lane]] : -1;
    if (a.d2) a.d2[out * k + s] = have ? ld[s * kKnnBlock + lane] : INFINITY;
  }
  if (a.visits) a.visits[out] = visits;
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3 matrix; r is the third index.  v*p / v*q: columns p, q of V.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
  const double root = sqrt(__dadd_rn(__dmul_rn(theta, theta), 1.0));
  const double t = __ddiv_rn(theta < 0.0 ? -1.0 : 1.0, __dadd_rn(fabs(theta), root));     // 0 when theta overflows
  const double c = __ddiv_rn(1.0, sqrt(__dadd_rn(__dmul_rn(t, t), 1.0)));
  const double s = __dmul_rn(t, c);
  const double h = __dmul_rn(t, apq);
  app = __dsub_rn(app, h);
  aqq = __dadd_rn(aqq, h);
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = __dsub_rn(__dmul_rn(c, rp), __dmul_rn(s, rq));
  arq = __dadd_rn(__dmul_rn(s, rp), __dmul_rn(c, rq));
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = __dsub_rn(__dmul_rn(c, a0), __dmul_rn(s, b0)); v0q = __dadd_rn(__dmul_rn(s, a0), __dmul_rn(c, b0));
  v1p = __dsub_rn(__dmul_rn(c, a1), __dmul_rn(s, b1)); v1q = __dadd_rn(__dmul_rn(s, a1), __dmul_rn(c, b1));
  v2p = __dsub_rn(__dmul_rn(c, a2), __dmul_rn(s, b2)); v2q = __dadd_rn(__dmul_rn(s, a2), __dmul_rn(c, b2));
}

struct NormalArgs {
  KnnWalk w;
  const float* dirs;       // [n][3] input order, nullable
  double* normals;         // [n][3] input order
  double* cov;             // [n][6] nullable
};

__global__ __launch_bounds__(kKnnBlock) void pts_normals_kernel(const NormalArgs a) {
  const long long i = (long long)blockIdx.x * kKnnBlock + threadIdx.x;
  if (i >= a.w.n) return;
  const int lane = threadIdx.x, k = a.w.k;
  double* ld = knn_lds;
  int* lj = reinterpret_cast<int*>(knn_lds + k * kKnnBlock);
  const long long out = a.w.perm[i];
  int visits;
  const int cnt = knn_walk(a.w, a.w.pts[i * 3 + 0], a.w.pts[i * 3 + 1], a.w.pts[i * 3 + 2], ld, lj, &visits);
  double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  for (int s = 0; s < cnt; ++s) {
    const long long j = lj[s * kKnnBlock + lane];
    const double x = a.w.pts[j * 3 + 0], y = a.w.pts[j * 3 + 1], z = a.w.pts[j * 3 + 2];
    sx = __dadd_rn(sx, x); sy = __dadd_rn(sy, y); sz = __dadd_rn(sz, z);
    sxx = __dadd_rn(sxx, __dmul_rn(x, x)); sxy = __dadd_rn(sxy, __dmul_rn(x, y)); sxz = __dadd_rn(sxz, __dmul_rn(x, z));
    syy = __dadd_rn(syy, __dmul_rn(y, y)); syz = __dadd_rn(syz, __dmul_rn(y, z)); szz = __dadd_rn(szz, __dmul_rn(z, z));
  }
  const double kd = (double)cnt;              // cnt >= 1: the point finds itself
  const double ex = __ddiv_rn(sx, kd), ey = __ddiv_rn(sy, kd), ez = __ddiv_rn(sz, kd);
  double cxx = __dsub_rn(__ddiv_rn(sxx, kd), __dmul_rn(ex, ex)), cxy = __dsub_rn(__ddiv_rn(sxy, kd), __dmul_rn(ex, ey));
  double cxz = __dsub_rn(__ddiv_rn(sxz, kd), __dmul_rn(ex, ez)), cyy = __dsub_rn(__ddiv_rn(syy, kd), __dmul_rn(ey, ey));
  double cyz = __dsub_rn(__ddiv_rn(syz, kd), __dmul_rn(ey, ez)), czz = __dsub_rn(__ddiv_rn(szz, kd), __dmul_rn(ez, ez));
  if (a.cov) {
    double* c = a.cov + out * 6;
    c[0] = cxx; c[1] = cxy; c[2] = cxz; c[3] = cyy; c[4] = cyz; c[5] = czz;
  }
  double nx = 0.0, ny = 0.0, nz = 1.0;
  if (cnt >= 3) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rotate(cxx, cyy, cxy, cxz, cyz, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
      jacobi_rotate(cxx, czz, cxz, cxy, cyz, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
      jacobi_rotate(cyy, czz, cyz, cxy, cxz, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    // the column of the smallest diagonal entry, the first one among equals
    const bool use1 = cyy < cxx;
    const double lam = use1 ? cyy : cxx;
    const bool use2 = czz < lam;
    nx = use2 ? v02 : (use1 ? v01 : v00);
    ny = use2 ? v12 : (use1 ? v11 : v10);
    nz = use2 ? v22 : (use1 ? v21 : v20);
    const double len = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(nx, nx), __dmul_rn(ny, ny)), __dmul_rn(nz, nz)));
    nx = __ddiv_rn(nx, len); ny = __ddiv_rn(ny, len); nz = __ddiv_rn(nz, len);
  }
  if (a.dirs) {
    const double dx = (double)a.dirs[out * 3 + 0], dy = (double)a.dirs[out * 3 + 1], dz = (double)a.dirs[out * 3 + 2];
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(nx, dx), __dmul_rn(ny, dy)), __dmul_rn(nz, dz));
    if (!(s > 0.0)) { nx = -nx; ny = -ny; nz = -nz; }
  }
  a.normals[out * 3 + 0] = nx; a.normals[out * 3 + 1] = ny; a.normals[out * 3 + 2] = nz;
}

inline size_t knn_lds_bytes(int k) { return (size_t)k * kKnnBlock * 12; }

}  // namespace

extern "C" int mdf_pts_knn(const void* index, long long n, long long index_bytes, const void* qindex, const double* queries, long long m,
                           long long qindex_bytes, int k, int* nbr, double* dist2_out, int* visits, void* stream) {
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  MDF_REQUIRE(k >= 1 && k <= MDF_PTS_KNN_MAX, "k=%d neighbours: 1 <= k <= %d", k, MDF_PTS_KNN_MAX);
  MDF_REQUIRE(nbr || m == 0, "null pointer argument: nbr");
  Queries Q{};
  if (int rc = resolve_queries(qindex, queries, m, qindex_bytes, nullptr, &Q)) return rc;
  if (m == 0) return MDF_OK;
  const IndexLayout L = index_layout(index, n);
  KnnArgs a{};
  a.w = KnnWalk{L.pts, L.perm, L.nodes, n, L.P, k};
  a.m = m;
  a.q = Q.q;
  a.qperm = Q.qperm;
  a.nbr = nbr; a.d2 = dist2_out; a.visits = visits;
  const unsigned grid = (unsigned)((m + kKnnBlock - 1) / kKnnBlock);
  hipLaunchKernelGGL(pts_knn_kernel, dim3(grid), dim3(kKnnBlock), knn_lds_bytes(k), (hipStream_t)stream, a);
  return mdf::check_launch("pts_knn_kernel");
}

extern "C" int mdf_pts_normals(const void* index, long long n, long long index_bytes, int k, const float* dirs, double* normals,
                               double* cov, void* stream) {
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  MDF_REQUIRE(k >= 1 && k <= MDF_PTS_KNN_MAX, "k=%d neighbours: 1 <= k <= %d", k, MDF_PTS_KNN_MAX);
  MDF_REQUIRE(normals || n == 0, "null pointer argument: normals");
  if (n == 0) return MDF_OK;
  const IndexLayout L = index_layout(index, n);
  NormalArgs a{};
  a.w = KnnWalk{L.pts, L.perm, L.nodes, n, L.P, k};
  a.dirs = dirs; a.normals = normals; a.cov = cov;
  const unsigned grid = (unsigned)((n + kKnnBlock - 1) / kKnnBlock);
  hipLaunchKernelGGL(pts_normals_kernel, dim3(grid), dim3(kKnnBlock), knn_lds_bytes(k), (hipStream_t)stream, a);
  return mdf::check_launch("pts_normals_kernel");
}
