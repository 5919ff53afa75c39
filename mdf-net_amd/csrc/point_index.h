// What the point-cloud files share (point_index.hip, point_eval.hip, point_register.hip, point_knn.hip): the index's layout and
// argument checks, the sort and bounding-box buffers, the exact distance helpers and the nearest-neighbour stack walk.
//   layout     IndexLayout: the points in key (Morton) order, the permutation back to the input order, the tree that
//              point_index.hip builds, then the buffers of the build (SortBuffers, which the voxel grid's workspace embeds too).
//   distances  d^2 = ((dx*dx) + dy*dy) + dz*dz, every operation rounded once (no contraction).  "d < c" and "d <= c" are decided
//              on d^2 exactly, against the bounds of sqrt_ge_bound / sqrt_le_bound.
//   nn_walk    one query per lane, nearest child first, a subtree is skipped when its box distance^2 cannot improve the result.
#pragma once
#include <algorithm>
#include <cmath>
#include "common.h"
#include "scan_common.h"

#pragma clang fp contract(off)     // for every point file: the library builds with -ffp-contract=off, the pragma pins it here

namespace mdf {
namespace pts {

constexpr int kBlock = 256;
constexpr int kLeaf = 32;                    // sorted points per leaf
constexpr int kStack = 32;                   // traversal stack: one entry per level at most, depth <= 26 for n < 2^31
constexpr int kSortItems = 16;               // keys per thread per tile of the radix sort
constexpr int kTile = kBlock * kSortItems;   // 4096 keys per tile
constexpr int kRadix = 256;
constexpr int kBboxBlocks = 1024;
using mdf::kScanThreads;

static_assert(kBlock == kScanBlock, "the block folds and sums of scan_common.h run in the point kernels' blocks");

__host__ __device__ inline long long align16(long long b) { return (b + 15) & ~15ll; }

inline unsigned grid_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// Hands out 16-byte aligned pieces of one buffer (base may be null: sizes only).
struct Arena {
  char* base;
  long long used = 0;
  template <typename T>
  T* take(long long count) {
    char* at = base + used;
    used += align16(count * (long long)sizeof(T));
    return reinterpret_cast<T*>(at);
  }
};

// ---------------------------------------------------------------------------------------------------- layouts
struct SortBuffers {       // what launch_bbox and sort_pairs work in
  double* bbox_part;       // [kBboxBlocks][6]
  double* bbox;            // [6] lo xyz, hi xyz
  unsigned long long *key0, *key1;
  int *val0, *val1;
  int* hist;               // [kRadix][ntiles]
  long long* hoff;         // [kRadix][ntiles]
};

inline SortBuffers take_sort_buffers(Arena& a, long long n, long long ntiles) {
  SortBuffers S{};
  S.bbox_part = a.take<double>(kBboxBlocks * 6);
  S.bbox = a.take<double>(6);
  S.key0 = a.take<unsigned long long>(n);
  S.key1 = a.take<unsigned long long>(n);
  S.val0 = a.take<int>(n);
  S.val1 = a.take<int>(n);
  S.hist = a.take<int>(kRadix * ntiles);
  S.hoff = a.take<long long>(kRadix * ntiles);
  return S;
}

struct IndexLayout {
  long long n, nleaves, P, ntiles;
  double* pts;           // [n][3] in key order
  int* perm;             // [n] key-order position -> input index
  double* nodes;         // [2P][6] lo xyz, hi xyz (node 0 unused)
  SortBuffers sort;
  long long bytes;
};

inline IndexLayout index_layout(const void* index, long long n) {
  IndexLayout L{};
  L.n = n;
  L.nleaves = (n + kLeaf - 1) / kLeaf;
  L.P = 1;
  while (L.P < L.nleaves) L.P <<= 1;
  L.ntiles = (n + kTile - 1) / kTile;
  Arena a{static_cast<char*>(const_cast<void*>(index))};
  L.pts = a.take<double>(n * 3);
  L.perm = a.take<int>(n);
  L.nodes = a.take<double>(2 * L.P * 6);
  L.sort = take_sort_buffers(a, n, L.ntiles);
  L.bytes = a.used;
  return L;
}

inline int check_index_args(const void* index, long long n, long long index_bytes) {
  MDF_REQUIRE(index, "null pointer argument: index");
  MDF_REQUIRE(n >= 0 && n < (1ll << 31) - kTile, "n=%lld points out of range", n);
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(index) % 16 == 0, "index must be 16-byte aligned");
  const long long need = index_layout(nullptr, n).bytes;
  MDF_REQUIRE(index_bytes >= need, "index buffer too small: %lld bytes, %lld needed", index_bytes, need);
  return MDF_OK;
}

// The queries of a search: an array [m][3] (results in its order) or an index over them (walked in key order, results at the
// input positions through qperm).
struct Queries {
  const double* q;
  const int* qperm;        // result position of query i (null: i)
};

// Exactly one of qindex and queries.  cap, where the search has one (nullable), is checked between the two query checks.
inline int resolve_queries(const void* qindex, const double* queries, long long m, long long qindex_bytes, const double* cap,
                           Queries* out) {
  MDF_REQUIRE((qindex == nullptr) != (queries == nullptr) || m == 0, "exactly one of qindex and queries must be given");
  if (cap) MDF_REQUIRE(std::isfinite(*cap) && *cap > 0, "cap=%g must be finite and > 0", *cap);
  if (qindex) {
    if (int rc = check_index_args(qindex, m, qindex_bytes)) return rc;
    const IndexLayout Q = index_layout(qindex, m);
    *out = Queries{Q.pts, Q.perm};
  } else {
    MDF_REQUIRE(m >= 0 && m < (1ll << 31), "m=%lld queries out of range", m);
    *out = Queries{queries, nullptr};
  }
  return MDF_OK;
}

// least x with sqrt(x) >= c (c > 0): "sqrt(d2) < c" <=> "d2 < x"
inline double sqrt_ge_bound(double c) {
  double x = c * c;
  while (x > 0 && std::sqrt(x) >= c) x = std::nextafter(x, 0.0);
  while (std::sqrt(x) < c) x = std::nextafter(x, INFINITY);
  return x;
}

// greatest x with sqrt(x) <= c: "sqrt(d2) <= c" <=> "d2 <= x"
inline double sqrt_le_bound(double c) {
  double x = c * c;
  while (std::sqrt(x) > c) x = std::nextafter(x, 0.0);
  while (std::sqrt(std::nextafter(x, INFINITY)) <= c) x = std::nextafter(x, INFINITY);
  return x;
}

// ---------------------------------------------------------------------------------------------------- point_index.hip
// The bounding box of pts [n][3] (n > 0) into S.bbox.
int launch_bbox(const double* pts, long long n, const SortBuffers& S, hipStream_t stream);
// Stable LSD radix sort of the n (key0, val0) pairs, 8 passes of 8 bits; the result is back in key0 / val0.
int sort_pairs(const SortBuffers& S, long long n, long long ntiles, hipStream_t stream);
// Exclusive scan of nitems int counts into int64 offsets (pts_sort_scan_kernel); *total = the sum (nullable).
int scan_counts(const int* counts, long long nitems, long long* offsets, long long* total, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------- device helpers
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

// The nearest point of a non-empty index (pts in key order, nodes, n > 0, P) to (qx, qy, qz) among those with d^2 < cap2: best = its d^2
// (unchanged, +inf from the caller, when there is none).  -> leaves visited.
//   kIndex = false  a subtree is walked while its box d^2 < min(best, cap2).
//   kIndex = true   bidx = the point's input index (perm); ties on d^2 go to the lowest input index, so a subtree at box
//                   distance == best is still walked: d <= best && d < cap2.
template <bool kIndex>
__device__ __forceinline__ int nn_walk(const double* __restrict__ pts, const int* __restrict__ perm, const double* __restrict__ nodes,
                                       long long n, long long P, double qx, double qy, double qz, double cap2, double& best, int& bidx) {
  int visits = 0;
  auto open = [&](double d) { return kIndex ? (d <= best && d < cap2) : d < fmin(best, cap2); };
  int stack[kStack];
  double sd[kStack];
  int sp = 0;
  long long node = 1;
  bool have = box_dist2(nodes + 6, qx, qy, qz) < cap2;
  while (have) {
    if (node >= P) {                         // leaf
      ++visits;
      const long long lo = (node - P) * kLeaf, hi = min(n, lo + kLeaf);
      for (long long j = lo; j < hi; ++j) {
        const double d2 = dist2(pts[j * 3 + 0], pts[j * 3 + 1], pts[j * 3 + 2], qx, qy, qz);
        if (!kIndex) {
          best = d2 < best ? d2 : best;
        } else if (d2 <= best) {
          const int pj = perm[j];
          if (d2 < best || pj < bidx) { best = d2; bidx = pj; }
        }
      }
    } else {
      const long long c0 = 2 * node, c1 = c0 + 1;
      const double d0 = box_dist2(nodes + c0 * 6, qx, qy, qz), d1 = box_dist2(nodes + c1 * 6, qx, qy, qz);
      const long long nearc = d1 < d0 ? c1 : c0, farc = d1 < d0 ? c0 : c1;
      const double dn = fmin(d0, d1), df = d1 < d0 ? d0 : d1;
      if (open(df) && sp < kStack) { stack[sp] = (int)farc; sd[sp] = df; ++sp; }
      if (open(dn)) { node = nearc; continue; }
    }
    have = false;
    while (sp > 0) {
      --sp;
      if (open(sd[sp])) { node = stack[sp]; have = true; break; }
    }
  }
  return visits;
}

}  // namespace pts
}  // namespace mdf
