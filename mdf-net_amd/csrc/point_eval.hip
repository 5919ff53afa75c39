// DTU point-cloud evaluation (the reference's MATLAB scorer: reducePts_haa.m, MaxDistCP.m and the masks of PointCompareMain.m),
// all fp64 and exact:
//   index      pts_bbox_kernel / pts_bbox_final_kernel (bounding box), pts_morton_kernel (63-bit Morton keys over the box),
//              a stable LSD radix sort (8 passes of 8 bits: pts_sort_hist_kernel, pts_sort_scan_kernel, pts_sort_scatter_kernel;
//              ties keep the input order), pts_gather_kernel (points in key order), pts_leaf_kernel + pts_node_kernel (an implicit
//              binary tree of fp64 AABBs over fixed leaves of kLeaf sorted points, built bottom-up; heap numbering, root 1, leaf
//              l at node P + l, P = leaves rounded up to a power of two, empty nodes hold an inverted box).
//   nn         pts_nn_kernel: one query per lane, nearest child first, a subtree is skipped when its box distance^2 is
//              >= min(best^2, cap2); cap2 is the least double whose square root is >= cap, so "d < cap" <=> "d^2 < cap2" exactly.
//   reduce     pts_rank_kernel, pts_radius_kernel<false> (earlier neighbours within dst per point: the greatest double whose
//              square root is <= dst bounds d^2, so "d <= dst" is decided exactly), pts_sort_scan_kernel (exclusive scan, int64),
//              pts_radius_kernel<true> (the same walk places the CSR), pts_reduce_init_kernel, then rounds of
//              pts_reduce_round_kernel + pts_reduce_step_kernel: an undecided point becomes OUT when an earlier neighbour is IN and IN when all of them are
//              OUT, reading the statuses of the previous round only (Jacobi), so the round count is run-independent too;
//              pts_reduce_keep_kernel writes the keep mask.  The result is the sequential greedy result of the visiting order.
//   masks      pts_dtu_masks_kernel: the ObsMask lookup (MATLAB round, 1-based column-major) and the ground-plane test.
// Distances: d^2 = ((dx*dx) + dy*dy) + dz*dz, no contraction (the library builds with -ffp-contract=off; the pragma pins it here).
// No float atomics; the only atomics are integer counters (per-block LDS histograms and the undecided count of a round).
// The second half of the file ("registration and F-score") builds the Tanks and Temples protocol's pieces on the same index, sort
// and distance helpers: nearest point with its index, rigid transform, crop volume, voxel-grid downsampling, ICP sums.
#include <algorithm>
#include <cmath>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kLeaf = 32;                    // sorted points per leaf
constexpr int kStack = 32;                   // traversal stack: one entry per level at most, depth <= 26 for n < 2^31
constexpr int kSortItems = 16;               // keys per thread per tile of the radix sort
constexpr int kTile = kBlock * kSortItems;   // 4096 keys per tile
constexpr int kRadix = 256;
constexpr int kScanThreads = 1024;
constexpr int kBboxBlocks = 1024;
constexpr int kCtl = 4;                      // reduce control words: rounds done, undecided after it, accumulator, spare

__host__ __device__ inline long long align16(long long b) { return (b + 15) & ~15ll; }

// ---------------------------------------------------------------------------------------------------- index layout
struct IndexLayout {
  long long n, nleaves, P, ntiles;
  double* pts;           // [n][3] in key order
  int* perm;             // [n] key-order position -> input index
  double* nodes;         // [2P][6] lo xyz, hi xyz (node 0 unused)
  double* bbox_part;     // [kBboxBlocks][6]
  double* bbox;          // [6]
  unsigned long long *key0, *key1;
  int *val0, *val1;
  int* hist;             // [kRadix][ntiles]
  long long* hoff;       // [kRadix][ntiles]
  long long bytes;
};

IndexLayout index_layout(char* base, long long n) {
  IndexLayout L{};
  L.n = n;
  L.nleaves = (n + kLeaf - 1) / kLeaf;
  L.P = 1;
  while (L.P < L.nleaves) L.P <<= 1;
  L.ntiles = (n + kTile - 1) / kTile;
  long long o = 0;
  auto take = [&](long long bytes) { const long long at = o; o += align16(bytes); return base + at; };
  L.pts = reinterpret_cast<double*>(take(n * 24));
  L.perm = reinterpret_cast<int*>(take(n * 4));
  L.nodes = reinterpret_cast<double*>(take(2 * L.P * 48));
  L.bbox_part = reinterpret_cast<double*>(take(kBboxBlocks * 48));
  L.bbox = reinterpret_cast<double*>(take(48));
  L.key0 = reinterpret_cast<unsigned long long*>(take(n * 8));
  L.key1 = reinterpret_cast<unsigned long long*>(take(n * 8));
  L.val0 = reinterpret_cast<int*>(take(n * 4));
  L.val1 = reinterpret_cast<int*>(take(n * 4));
  L.hist = reinterpret_cast<int*>(take(kRadix * L.ntiles * 4));
  L.hoff = reinterpret_cast<long long*>(take(kRadix * L.ntiles * 8));
  L.bytes = o;
  return L;
}

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
  for (int a = 0; a < 6; ++a) red[a][threadIdx.x] = v[a];
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int a = 0; a < 6; ++a)
        red[a][threadIdx.x] = a < 3 ? fmin(red[a][threadIdx.x], red[a][threadIdx.x + s]) : fmax(red[a][threadIdx.x], red[a][threadIdx.x + s]);
    __syncthreads();
  }
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

// Exclusive scan of nitems int counts into int64 offsets by one block (contiguous chunks, one per thread); *total = the sum.
__global__ __launch_bounds__(kScanThreads) void pts_sort_scan_kernel(const int* __restrict__ counts, long long nitems,
                                                                     long long* __restrict__ offsets, long long* __restrict__ total) {
  __shared__ long long part[kScanThreads];
  const int t = threadIdx.x;
  const long long chunk = (nitems + kScanThreads - 1) / kScanThreads;
  const long long lo = min(nitems, t * chunk), hi = min(nitems, lo + chunk);
  long long s = 0;
  for (long long i = lo; i < hi; ++i) s += counts[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const long long add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long long run = part[t] - s;
  for (long long i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (t == kScanThreads - 1 && total != nullptr) *total = part[t];
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

// ---------------------------------------------------------------------------------------------------- queries
__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Lower bound of dist2 to any point of the box (an inverted box gives +inf).  Each axis term is the same rounded difference the
// point formula takes for the box's extreme coordinate, and rounding is monotonic, so it never exceeds a contained point's d^2.
__device__ __forceinline__ double box_dist2(const double* __restrict__ b, double x, double y, double z) {
  if (b[0] > b[3]) return INFINITY;
  const double dx = x < b[0] ? __dsub_rn(b[0], x) : (x > b[3] ? __dsub_rn(x, b[3]) : 0.0);
  const double dy = y < b[1] ? __dsub_rn(b[1], y) : (y > b[4] ? __dsub_rn(y, b[4]) : 0.0);
  const double dz = z < b[2] ? __dsub_rn(b[2], z) : (z > b[5] ? __dsub_rn(z, b[5]) : 0.0);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

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
  int visits = 0;
  const bool inside = !a.reg.use || (in_axis(qx, a.reg.lo[0], a.reg.range[0], a.cap) && in_axis(qy, a.reg.lo[1], a.reg.range[1], a.cap) &&
                                     in_axis(qz, a.reg.lo[2], a.reg.range[2], a.cap));
  if (inside && a.n > 0) {
    int stack[kStack];
    double sd[kStack];
    int sp = 0;
    long long node = 1;
    double nd = box_dist2(a.nodes + 6, qx, qy, qz);
    bool have = nd < a.cap2;
    while (have) {
      if (node >= a.P) {                         // leaf
        ++visits;
        const long long lo = (node - a.P) * kLeaf, hi = min(a.n, lo + kLeaf);
        for (long long j = lo; j < hi; ++j) {
          const double d2 = dist2(a.pts[j * 3 + 0], a.pts[j * 3 + 1], a.pts[j * 3 + 2], qx, qy, qz);
          best = d2 < best ? d2 : best;
        }
      } else {
        const long long c0 = 2 * node, c1 = c0 + 1;
        const double d0 = box_dist2(a.nodes + c0 * 6, qx, qy, qz), d1 = box_dist2(a.nodes + c1 * 6, qx, qy, qz);
        const double lim = fmin(best, a.cap2);
        const long long nearc = d1 < d0 ? c1 : c0, farc = d1 < d0 ? c0 : c1;
        const double dn = fmin(d0, d1), df = d1 < d0 ? d0 : d1;
        if (df < lim && sp < kStack) { stack[sp] = (int)farc; sd[sp] = df; ++sp; }
        if (dn < lim) { node = nearc; continue; }
      }
      have = false;
      while (sp > 0) {
        --sp;
        if (sd[sp] < fmin(best, a.cap2)) { node = stack[sp]; have = true; break; }
      }
    }
  }
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
  long long o = 0;
  auto take = [&](long long bytes) { const long long at = o; o += align16(bytes); return base + at; };
  R.rank_s = reinterpret_cast<int*>(take(n * 4));
  R.count = reinterpret_cast<int*>(take(n * 4));
  R.offs = reinterpret_cast<long long*>(take((n + 1) * 8));
  R.st0 = reinterpret_cast<unsigned char*>(take(n));
  R.st1 = reinterpret_cast<unsigned char*>(take(n));
  R.cursor = reinterpret_cast<int*>(take(n * 4));
  R.ctl = reinterpret_cast<int*>(take(kCtl * 4));
  R.bytes = o;
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

// ---------------------------------------------------------------------------------------------------- host helpers
unsigned grid_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// least x with sqrt(x) >= c (c > 0): "sqrt(d2) < c" <=> "d2 < x"
double sqrt_ge_bound(double c) {
  double x = c * c;
  while (x > 0 && std::sqrt(x) >= c) x = std::nextafter(x, 0.0);
  while (std::sqrt(x) < c) x = std::nextafter(x, INFINITY);
  return x;
}

// greatest x with sqrt(x) <= c: "sqrt(d2) <= c" <=> "d2 <= x"
double sqrt_le_bound(double c) {
  double x = c * c;
  while (std::sqrt(x) > c) x = std::nextafter(x, 0.0);
  while (std::sqrt(std::nextafter(x, INFINITY)) <= c) x = std::nextafter(x, INFINITY);
  return x;
}

int check_index_args(const void* index, long long n, long long index_bytes) {
  MDF_REQUIRE(index, "null pointer argument: index");
  MDF_REQUIRE(n >= 0 && n < (1ll << 31) - kTile, "n=%lld points out of range", n);
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(index) % 16 == 0, "index must be 16-byte aligned");
  const long long need = index_layout(nullptr, n).bytes;
  MDF_REQUIRE(index_bytes >= need, "index buffer too small: %lld bytes, %lld needed", index_bytes, need);
  return MDF_OK;
}

}  // namespace

extern "C" long long mdf_pts_index_workspace(long long n) {
  if (n < 0 || n >= (1ll << 31) - kTile) return 0;
  return index_layout(nullptr, n).bytes;
}

extern "C" int mdf_pts_index_build(const double* pts, long long n, void* index, long long index_bytes, void* stream) {
  MDF_REQUIRE(pts || n == 0, "null pointer argument: pts");
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  const IndexLayout L = index_layout(static_cast<char*>(index), n);
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    const int nbb = (int)std::min<long long>(kBboxBlocks, (n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pts_bbox_kernel, dim3(nbb), dim3(kBlock), 0, s, pts, n, L.bbox_part);
    if (int rc = mdf::check_launch("pts_bbox_kernel")) return rc;
    hipLaunchKernelGGL(pts_bbox_final_kernel, dim3(1), dim3(64), 0, s, L.bbox_part, nbb, L.bbox);
    if (int rc = mdf::check_launch("pts_bbox_final_kernel")) return rc;
    hipLaunchKernelGGL(pts_morton_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, pts, n, L.bbox, L.key0, L.val0);
    if (int rc = mdf::check_launch("pts_morton_kernel")) return rc;
    unsigned long long *kin = L.key0, *kout = L.key1;
    int *vin = L.val0, *vout = L.val1;
    for (int shift = 0; shift < 64; shift += 8) {
      hipLaunchKernelGGL(pts_sort_hist_kernel, dim3((unsigned)L.ntiles), dim3(kBlock), 0, s, kin, n, shift, L.ntiles, L.hist);
      if (int rc = mdf::check_launch("pts_sort_hist_kernel")) return rc;
      hipLaunchKernelGGL(pts_sort_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, L.hist, kRadix * L.ntiles, L.hoff, nullptr);
      if (int rc = mdf::check_launch("pts_sort_scan_kernel")) return rc;
      hipLaunchKernelGGL(pts_sort_scatter_kernel, dim3((unsigned)L.ntiles), dim3(kBlock), 0, s, kin, vin, n, shift, L.ntiles, L.hoff, kout,
                         vout);
      if (int rc = mdf::check_launch("pts_sort_scatter_kernel")) return rc;
      std::swap(kin, kout);
      std::swap(vin, vout);
    }
    hipLaunchKernelGGL(pts_gather_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, pts, vin, n, L.pts, L.perm);
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

extern "C" int mdf_pts_nn_dist(const void* index, long long n, long long index_bytes, const void* qindex, const double* queries, long long m,
                               long long qindex_bytes, const double* bb, double cap, double* dist, int* visits, void* stream) {
  if (int rc = check_index_args(index, n, index_bytes)) return rc;
  MDF_REQUIRE(dist || m == 0, "null pointer argument: dist");
  MDF_REQUIRE((qindex == nullptr) != (queries == nullptr) || m == 0, "exactly one of qindex and queries must be given");
  MDF_REQUIRE(std::isfinite(cap) && cap > 0, "cap=%g must be finite and > 0", cap);
  if (qindex) {
    if (int rc = check_index_args(qindex, m, qindex_bytes)) return rc;
  } else {
    MDF_REQUIRE(m >= 0 && m < (1ll << 31), "m=%lld queries out of range", m);
  }
  if (m == 0) return MDF_OK;
  const IndexLayout L = index_layout(static_cast<char*>(const_cast<void*>(index)), n);
  NnArgs a{};
  a.pts = L.pts; a.nodes = L.nodes; a.n = n; a.P = L.P; a.m = m;
  if (qindex) {
    const IndexLayout Q = index_layout(static_cast<char*>(const_cast<void*>(qindex)), m);
    a.q = Q.pts;
    a.qperm = Q.perm;
  } else {
    a.q = queries;
    a.qperm = nullptr;
  }
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
  const IndexLayout L = index_layout(static_cast<char*>(const_cast<void*>(index)), n);
  const ReduceLayout R = reduce_layout(static_cast<char*>(workspace), n);
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(pts_rank_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, rank, L.perm, n, R.rank_s);
    if (int rc = mdf::check_launch("pts_rank_kernel")) return rc;
    RadiusArgs a{L.pts, L.nodes, L.perm, R.rank_s, n, L.P, sqrt_le_bound(dst), R.count, nullptr, nullptr, 0};
    hipLaunchKernelGGL(pts_radius_kernel<false>, dim3(grid_of(n)), dim3(kBlock), 0, s, a);
    if (int rc = mdf::check_launch("pts_radius_kernel")) return rc;
  }
  hipLaunchKernelGGL(pts_sort_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, R.count, n, R.offs, edges);
  if (int rc = mdf::check_launch("pts_sort_scan_kernel")) return rc;
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
  const IndexLayout L = index_layout(static_cast<char*>(const_cast<void*>(index)), n);
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

// ==================================================================================================== registration and F-score
// The Tanks and Temples protocol's pieces (crop volume, voxel-grid downsampling, point-to-point ICP, F-score), on the index, sort and
// distance helpers above:
//   nn         pts_nn_idx_kernel: pts_nn_kernel's walk without a region, which also reports WHICH point was nearest (its input
//              index; ties on d^2 go to the lowest input index, so a subtree at box distance == best is still walked).
//   transform  pts_transform_kernel: x' = ((r00 x + r01 y) + r02 z) + t0, each operation rounded once.
//   crop       pts_crop_kernel: the axis interval and an even-odd crossing count against the polygon.
//   voxel      pts_bbox_*, pts_vox_key_kernel (3 x 21-bit cell keys, x major), the stable radix sort (a cell's points stay in input
//              order), pts_vox_chunk_sum_kernel + pts_sort_scan_kernel + pts_vox_offsets_kernel (a three-pass exclusive scan of the
//              segment heads over many blocks), pts_vox_mean_kernel (one lane per cell: sum in input order, divide).
//   icp        pts_icp_moment_kernel<false> + pts_icp_final_kernel<false> (inlier count, sum of d^2, the two centroids),
//              pts_icp_moment_kernel<true> + pts_icp_final_kernel<true> (the cross-covariance about them).  Every lane sums a fixed
//              strided subset in order, every block folds its lanes with one fixed tree and one block folds the blocks the same
//              way: the shape depends on n only, so the sums are run-independent.  No atomics.
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
  int visits = 0;
  if (a.n > 0) {
    int stack[kStack];
    double sd[kStack];
    int sp = 0;
    long long node = 1;
    const double nd = box_dist2(a.nodes + 6, qx, qy, qz);
    bool have = nd < a.cap2;
    while (have) {
      if (node >= a.P) {                         // leaf
        ++visits;
        const long long lo = (node - a.P) * kLeaf, hi = min(a.n, lo + kLeaf);
        for (long long j = lo; j < hi; ++j) {
          const double d2 = dist2(a.pts[j * 3 + 0], a.pts[j * 3 + 1], a.pts[j * 3 + 2], qx, qy, qz);
          if (d2 <= best) {
            const int pj = a.perm[j];
            if (d2 < best || pj < bidx) { best = d2; bidx = pj; }
          }
        }
      } else {
        const long long c0 = 2 * node, c1 = c0 + 1;
        const double d0 = box_dist2(a.nodes + c0 * 6, qx, qy, qz), d1 = box_dist2(a.nodes + c1 * 6, qx, qy, qz);
        const long long nearc = d1 < d0 ? c1 : c0, farc = d1 < d0 ? c0 : c1;
        const double dn = fmin(d0, d1), df = d1 < d0 ? d0 : d1;
        if (df <= best && df < a.cap2 && sp < kStack) { stack[sp] = (int)farc; sd[sp] = df; ++sp; }
        if (dn <= best && dn < a.cap2) { node = nearc; continue; }
      }
      have = false;
      while (sp > 0) {
        --sp;
        if (sd[sp] <= best && sd[sp] < a.cap2) { node = stack[sp]; have = true; break; }
      }
    }
  }
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
  double* bbox_part;
  double* bbox;
  unsigned long long *key0, *key1;
  int *val0, *val1;
  int* hist;
  long long* hoff;
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
  long long o = 0;
  auto take = [&](long long bytes) { const long long at = o; o += align16(bytes); return base + at; };
  L.bbox_part = reinterpret_cast<double*>(take(kBboxBlocks * 48));
  L.bbox = reinterpret_cast<double*>(take(48));
  L.key0 = reinterpret_cast<unsigned long long*>(take(n * 8));
  L.key1 = reinterpret_cast<unsigned long long*>(take(n * 8));
  L.val0 = reinterpret_cast<int*>(take(n * 4));
  L.val1 = reinterpret_cast<int*>(take(n * 4));
  L.hist = reinterpret_cast<int*>(take(kRadix * L.ntiles * 4));
  L.hoff = reinterpret_cast<long long*>(take(kRadix * L.ntiles * 8));
  L.chunk_sums = reinterpret_cast<int*>(take(L.nchunks * 4));
  L.chunk_off = reinterpret_cast<long long*>(take(L.nchunks * 8));
  L.seg_start = reinterpret_cast<int*>(take(n * 4));
  L.total = reinterpret_cast<long long*>(take(8));
  L.ctl = reinterpret_cast<int*>(take(16));
  L.bytes = o;
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
  __shared__ int part[kBlock];
  const long long base = (long long)blockIdx.x * kVoxChunk + threadIdx.x * kVoxPer;
  int t = 0;
  for (int k = 0; k < kVoxPer; ++k) t += vox_head(keys, base + k, n);
  part[threadIdx.x] = t;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(kBlock) void pts_vox_offsets_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                                 const long long* __restrict__ chunk_off, int* __restrict__ seg_start) {
  __shared__ int part[kBlock];
  const long long base = (long long)blockIdx.x * kVoxChunk + threadIdx.x * kVoxPer;
  int c[kVoxPer];
  int t = 0;
  for (int k = 0; k < kVoxPer; ++k) {
    c[k] = vox_head(keys, base + k, n);
    t += c[k];
  }
  part[threadIdx.x] = t;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {           // Hillis-Steele inclusive scan of the thread sums
    const int add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  long long run = chunk_off[blockIdx.x] + (part[threadIdx.x] - t);
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

__device__ __forceinline__ void icp_block_fold(double (&v)[kIcpVals], double (*red)[kBlock]) {
  for (int k = 0; k < kIcpVals; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int k = 0; k < kIcpVals; ++k) red[k][threadIdx.x] = __dadd_rn(red[k][threadIdx.x], red[k][threadIdx.x + s]);
    __syncthreads();
  }
}

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
  icp_block_fold(v, red);
  if (threadIdx.x < kIcpVals) a.part[(long long)blockIdx.x * kIcpVals + threadIdx.x] = red[threadIdx.x][0];
}

template <bool kCov>
__global__ __launch_bounds__(kBlock) void pts_icp_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
  __shared__ double red[kIcpVals][kBlock];
  double v[kIcpVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nparts; b += kBlock)
    for (int k = 0; k < kIcpVals; ++k) v[k] = __dadd_rn(v[k], part[(long long)b * kIcpVals + k]);
  icp_block_fold(v, red);
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
  MDF_REQUIRE((qindex == nullptr) != (queries == nullptr) || m == 0, "exactly one of qindex and queries must be given");
  MDF_REQUIRE(std::isfinite(cap) && cap > 0, "cap=%g must be finite and > 0", cap);
  if (qindex) {
    if (int rc = check_index_args(qindex, m, qindex_bytes)) return rc;
  } else {
    MDF_REQUIRE(m >= 0 && m < (1ll << 31), "m=%lld queries out of range", m);
  }
  if (m == 0) return MDF_OK;
  const IndexLayout L = index_layout(static_cast<char*>(const_cast<void*>(index)), n);
  NnIdxArgs a{};
  a.pts = L.pts; a.perm = L.perm; a.nodes = L.nodes; a.n = n; a.P = L.P; a.m = m;
  if (qindex) {
    const IndexLayout Q = index_layout(static_cast<char*>(const_cast<void*>(qindex)), m);
    a.q = Q.pts;
    a.qperm = Q.perm;
  } else {
    a.q = queries;
    a.qperm = nullptr;
  }
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
  const int nbb = (int)std::min<long long>(kBboxBlocks, (n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(pts_bbox_kernel, dim3(nbb), dim3(kBlock), 0, s, pts, n, L.bbox_part);
  if (int rc = mdf::check_launch("pts_bbox_kernel")) return rc;
  hipLaunchKernelGGL(pts_bbox_final_kernel, dim3(1), dim3(64), 0, s, L.bbox_part, nbb, L.bbox);
  if (int rc = mdf::check_launch("pts_bbox_final_kernel")) return rc;
  hipLaunchKernelGGL(pts_vox_key_kernel, dim3(grid_of(n)), dim3(kBlock), 0, s, pts, n, L.bbox, voxel, L.key0, L.val0, L.ctl);
  if (int rc = mdf::check_launch("pts_vox_key_kernel")) return rc;
  unsigned long long *kin = L.key0, *kout = L.key1;
  int *vin = L.val0, *vout = L.val1;
  for (int shift = 0; shift < 64; shift += 8) {
    hipLaunchKernelGGL(pts_sort_hist_kernel, dim3((unsigned)L.ntiles), dim3(kBlock), 0, s, kin, n, shift, L.ntiles, L.hist);
    if (int rc = mdf::check_launch("pts_sort_hist_kernel")) return rc;
    hipLaunchKernelGGL(pts_sort_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, L.hist, kRadix * L.ntiles, L.hoff, nullptr);
    if (int rc = mdf::check_launch("pts_sort_scan_kernel")) return rc;
    hipLaunchKernelGGL(pts_sort_scatter_kernel, dim3((unsigned)L.ntiles), dim3(kBlock), 0, s, kin, vin, n, shift, L.ntiles, L.hoff, kout,
                       vout);
    if (int rc = mdf::check_launch("pts_sort_scatter_kernel")) return rc;
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
  hipLaunchKernelGGL(pts_vox_chunk_sum_kernel, dim3((unsigned)L.nchunks), dim3(kBlock), 0, s, kin, n, L.chunk_sums);
  if (int rc = mdf::check_launch("pts_vox_chunk_sum_kernel")) return rc;
  hipLaunchKernelGGL(pts_sort_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, L.chunk_sums, L.nchunks, L.chunk_off, L.total);
  if (int rc = mdf::check_launch("pts_sort_scan_kernel")) return rc;
  hipLaunchKernelGGL(pts_vox_offsets_kernel, dim3((unsigned)L.nchunks), dim3(kBlock), 0, s, kin, n, L.chunk_off, L.seg_start);
  if (int rc = mdf::check_launch("pts_vox_offsets_kernel")) return rc;
  VoxMeanArgs a{pts, attrs, nattr, n, vin, L.seg_start, L.total, L.ctl, out_pts, out_attrs, out_count, m};
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

// ==================================================================================================== k-NN and normals
// Point-cloud post-processing (the reference's Open3D stages: estimate_normals, compute_nearest_neighbor_distance), on the same
// index and distance helpers:
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
  MDF_REQUIRE((qindex == nullptr) != (queries == nullptr) || m == 0, "exactly one of qindex and queries must be given");
  if (qindex) {
    if (int rc = check_index_args(qindex, m, qindex_bytes)) return rc;
  } else {
    MDF_REQUIRE(m >= 0 && m < (1ll << 31), "m=%lld queries out of range", m);
  }
  if (m == 0) return MDF_OK;
  const IndexLayout L = index_layout(static_cast<char*>(const_cast<void*>(index)), n);
  KnnArgs a{};
  a.w = KnnWalk{L.pts, L.perm, L.nodes, n, L.P, k};
  a.m = m;
  if (qindex) {
    const IndexLayout Q = index_layout(static_cast<char*>(const_cast<void*>(qindex)), m);
    a.q = Q.pts;
    a.qperm = Q.perm;
  } else {
    a.q = queries;
    a.qperm = nullptr;
  }
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
  const IndexLayout L = index_layout(static_cast<char*>(const_cast<void*>(index)), n);
  NormalArgs a{};
  a.w = KnnWalk{L.pts, L.perm, L.nodes, n, L.P, k};
  a.dirs = dirs; a.normals = normals; a.cov = cov;
  const unsigned grid = (unsigned)((n + kKnnBlock - 1) / kKnnBlock);
  hipLaunchKernelGGL(pts_normals_kernel, dim3(grid), dim3(kKnnBlock), knn_lds_bytes(k), (hipStream_t)stream, a);
  return mdf::check_launch("pts_normals_kernel");
}
