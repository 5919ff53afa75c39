// Scene import from a sparse model (include/mdfnet_hip.h states the semantics): per-image depth ranges and the image-pair
// view-selection score, all fp64, every operation rounded once, sums in a stated order.  The sort, the scan and the arena are
// those of the point-cloud files (point_index.h); nothing here sorts on its own.
//   tracks     view_track_kernel: one thread per point checks its track (offsets inside [0, n_obs], image indices inside [0, N)
//              and strictly ascending) and writes the point's record count t(t-1)/2, or 0 and a status bit for a bad track.
//   ranges     view_depth_key_kernel (one thread per point: depth of each observation as orderable bits, the image as value,
//              per-image counts by integer atomics), sort_pairs by depth, view_regroup_kernel (image as key, depth rank as value),
//              sort_pairs by image (stable: depths stay ascending inside an image), scan_counts, view_range_kernel (one thread per
//              image picks its two order statistics).
//   scores     view_centre_kernel, view_fill_kernel (every record slot starts as the sentinel), view_expand_kernel (one thread per
//              point: key i*N + j, value the point), view_term_kernel (one thread per record: the transcendentals),
//              sort_pairs by pair (stable: point order survives), view_sum_kernel (the first record of a pair adds its run).
// No float atomics; the only atomics are the integer counts and the status bits.
#include "point_index.h"

using namespace mdf::pts;

namespace {

constexpr int kMaxImages = 32768;                       // t(t-1)/2 of one track and i*N + j stay far inside their types
constexpr unsigned long long kNoRecord = ~0ull;         // key of a record slot that holds nothing (sorts last)
constexpr double kDegrees = 57.29577951308232;

struct ViewLayout {
  long long nsort, ntiles;
  double* centre;            // [N][3]  (the workspace begins with it: the header says so)
  int* img_count;            // [N + 1] observations per image; slot N collects the observations of skipped tracks
  long long* img_off;        // [N + 1]
  int* rec_count;            // [P] records per point (0 for a skipped track)
  long long* rec_off;        // [P]
  long long* rec_total;      // [1] the records the accepted tracks hold
  unsigned long long* depth; // [n_obs] depth bits in ascending order
  double* term;              // [n_rec] in record order
  SortBuffers sort;
  long long bytes;
};

ViewLayout view_layout(char* base, int n_img, long long n_pts, long long n_obs, long long n_rec) {
  ViewLayout L{};
  L.nsort = std::max(n_obs, n_rec);
  L.ntiles = (L.nsort + kTile - 1) / kTile;
  Arena a{base};
  L.centre = a.take<double>((long long)n_img * 3);
  L.img_count = a.take<int>(n_img + 1);
  L.img_off = a.take<long long>(n_img + 1);
  L.rec_count = a.take<int>(n_pts);
  L.rec_off = a.take<long long>(n_pts);
  L.rec_total = a.take<long long>(1);
  L.depth = a.take<unsigned long long>(n_obs);
  L.term = a.take<double>(n_rec);
  L.sort = take_sort_buffers(a, L.nsort, L.ntiles);
  L.bytes = a.used;
  return L;
}

bool sizes_ok(int n_img, long long n_pts, long long n_obs, long long n_rec) {
  const long long lim = (1ll << 31) - kTile;
  return n_img >= 0 && n_img <= kMaxImages && n_pts >= 0 && n_pts < lim && n_obs >= 0 && n_obs < lim && n_rec >= 0 && n_rec < lim;
}

// The track of point p: first observation and length, or a status bit (then the track is skipped as a whole).
__device__ __forceinline__ int track_of(const long long* __restrict__ off, const int* __restrict__ img, long long p, long long n_obs,
                                        int N, long long& lo, int& t) {
  lo = off[p];
  const long long hi = off[p + 1];
  t = 0;
  if (lo < 0 || hi < lo || hi > n_obs) return MDF_VIEW_BAD_OFFSETS;
  if (hi - lo > N) return MDF_VIEW_NOT_ASCENDING;     // more observations than images cannot ascend strictly
  int prev = -1, bad = 0;
  for (long long o = lo; o < hi; ++o) {
    const int v = img[o];
    if (v < 0 || v >= N) bad |= MDF_VIEW_BAD_IMAGE;
    else if (v <= prev) bad |= MDF_VIEW_NOT_ASCENDING;
    else prev = v;
  }
  if (!bad) t = (int)(hi - lo);
  return bad;
}

__device__ __forceinline__ unsigned long long orderable(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

__device__ __forceinline__ double from_orderable(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__global__ __launch_bounds__(kBlock) void view_centre_kernel(const double* __restrict__ rot, const double* __restrict__ trans, int N,
                                                            double* __restrict__ centre) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const double* R = rot + (long long)i * 9;
  const double* t = trans + (long long)i * 3;
  for (int a = 0; a < 3; ++a)
    centre[(long long)i * 3 + a] = -__dadd_rn(__dadd_rn(__dmul_rn(R[a], t[0]), __dmul_rn(R[3 + a], t[1])), __dmul_rn(R[6 + a], t[2]));
}

__global__ __launch_bounds__(kBlock) void view_track_kernel(const long long* __restrict__ off, const int* __restrict__ img, long long P,
                                                           long long n_obs, int N, int* __restrict__ rec_count, int* __restrict__ status) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  long long lo;
  int t;
  const int bad = track_of(off, img, p, n_obs, N, lo, t);
  if (bad) atomicOr(status, bad);
  rec_count[p] = t * (t - 1) / 2;
}

// ---------------------------------------------------------------------------------------------------- depth ranges
__global__ __launch_bounds__(kBlock) void view_fill_kernel(unsigned long long* __restrict__ keys, int* __restrict__ vals, long long n,
                                                          unsigned long long key, int val) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  keys[r] = key;
  vals[r] = val;
}

__global__ __launch_bounds__(kBlock) void view_depth_key_kernel(const double* __restrict__ rot, const double* __restrict__ trans, int N,
                                                               const double* __restrict__ pts, long long P, const long long* __restrict__ off,
                                                               const int* __restrict__ img, long long n_obs, unsigned long long* __restrict__ keys,
                                                               int* __restrict__ vals, int* __restrict__ img_count, int* __restrict__ status) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  long long lo;
  int t;
  const int bad = track_of(off, img, p, n_obs, N, lo, t);
  if (bad) atomicOr(status, bad);
  const double x = pts[p * 3 + 0], y = pts[p * 3 + 1], z = pts[p * 3 + 2];
  for (int k = 0; k < t; ++k) {                      // lo + k < n_obs and img in [0, N): track_of checked both
    const int i = img[lo + k];
    const double* R = rot + (long long)i * 9;
    const double d = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(R[6], x), __dmul_rn(R[7], y)), __dmul_rn(R[8], z)), trans[(long long)i * 3 + 2]);
    keys[lo + k] = orderable(d);
    vals[lo + k] = i;
    atomicAdd(&img_count[i], 1);
  }
}

// after the depth sort: the depth bits are put aside, the image becomes the key and the depth rank the value
__global__ __launch_bounds__(kBlock) void view_regroup_kernel(unsigned long long* __restrict__ keys, int* __restrict__ vals, long long n,
                                                             unsigned long long* __restrict__ depth) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  depth[r] = keys[r];
  keys[r] = (unsigned long long)(unsigned)vals[r];
  vals[r] = (int)r;
}

__global__ __launch_bounds__(kBlock) void view_range_kernel(const int* __restrict__ img_count, const long long* __restrict__ img_off,
                                                           const int* __restrict__ rank, const unsigned long long* __restrict__ depth,
                                                           long long n_obs, int N, double q_lo, double q_hi, double* __restrict__ range,
                                                           int* __restrict__ count) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const long long n = n_obs > 0 ? img_count[i] : 0, first = n_obs > 0 ? img_off[i] : 0;
  count[i] = (int)n;
  double lo = NAN, hi = NAN;
  if (n > 0 && first >= 0 && first + n <= n_obs) {                       // the counts of valid tracks sum to <= n_obs
    const long long klo = min((long long)__dmul_rn(q_lo, (double)n), n - 1), khi = min((long long)__dmul_rn(q_hi, (double)n), n - 1);
    lo = from_orderable(depth[rank[first + klo]]);                       // rank: a permutation of [0, n_obs)
    hi = from_orderable(depth[rank[first + khi]]);
  }
  range[(long long)i * 2 + 0] = lo;
  range[(long long)i * 2 + 1] = hi;
}

// ---------------------------------------------------------------------------------------------------- pair scores
__global__ __launch_bounds__(kBlock) void view_expand_kernel(const long long* __restrict__ off, const int* __restrict__ img, long long P, int N,
                                                            const int* __restrict__ rec_count, const long long* __restrict__ rec_off,
                                                            const long long* __restrict__ rec_total, long long n_rec,
                                                            unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                            int* __restrict__ status) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  if (p == 0 && *rec_total != n_rec) atomicOr(status, MDF_VIEW_BAD_COUNT);
  const long long cnt = rec_count[p];
  if (cnt == 0) return;                               // a short or a skipped track
  long long r = rec_off[p];
  if (r + cnt > n_rec) return;                        // the caller's n_rec is less than the tracks hold: nothing past it is written
  const long long lo = off[p];
  const int t = (int)(off[p + 1] - lo);               // view_track_kernel accepted this track: cnt = t(t-1)/2
  for (int a = 0; a < t; ++a) {
    const unsigned long long i = (unsigned long long)img[lo + a];
    for (int b = a + 1; b < t; ++b, ++r) {
      keys[r] = i * (unsigned long long)N + (unsigned long long)img[lo + b];
      vals[r] = (int)p;
    }
  }
}

__global__ __launch_bounds__(kBlock) void view_term_kernel(const double* __restrict__ centre, const double* __restrict__ pts, int N,
                                                          const unsigned long long* __restrict__ keys, int* __restrict__ vals, long long n_rec,
                                                          double theta0, double sigma1, double sigma2, double* __restrict__ term) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rec) return;
  const unsigned long long key = keys[r];
  double out = 0.0;
  if (key != kNoRecord) {
    const long long i = (long long)(key / (unsigned long long)N), j = (long long)(key % (unsigned long long)N), p = vals[r];
    const double px = pts[p * 3 + 0], py = pts[p * 3 + 1], pz = pts[p * 3 + 2];
    const double u0 = __dsub_rn(centre[i * 3 + 0], px), u1 = __dsub_rn(centre[i * 3 + 1], py), u2 = __dsub_rn(centre[i * 3 + 2], pz);
    const double v0 = __dsub_rn(centre[j * 3 + 0], px), v1 = __dsub_rn(centre[j * 3 + 1], py), v2 = __dsub_rn(centre[j * 3 + 2], pz);
    const double cx = __dsub_rn(__dmul_rn(u1, v2), __dmul_rn(u2, v1));
    const double cy = __dsub_rn(__dmul_rn(u2, v0), __dmul_rn(u0, v2));
    const double cz = __dsub_rn(__dmul_rn(u0, v1), __dmul_rn(u1, v0));
    const double s = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz)));
    const double d = __dadd_rn(__dadd_rn(__dmul_rn(u0, v0), __dmul_rn(u1, v1)), __dmul_rn(u2, v2));
    const double theta = __dmul_rn(atan2(s, d), kDegrees);
    const double e = __dsub_rn(theta, theta0);
    const double sigma = theta <= theta0 ? sigma1 : sigma2;
    out = exp(__ddiv_rn(-__dmul_rn(e, e), __dmul_rn(__dmul_rn(2.0, sigma), sigma)));
  }
  term[r] = out;
  vals[r] = (int)r;                                  // the sort carries the record's position, the term stays where it is
}

__global__ __launch_bounds__(kBlock) void view_sum_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ vals,
                                                         const double* __restrict__ term, long long n_rec, int N, double* __restrict__ score,
                                                         int* __restrict__ shared) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rec) return;
  const unsigned long long key = keys[r];
  if (key == kNoRecord || (r > 0 && keys[r - 1] == key)) return;        // not the first record of a pair
  double acc = 0.0;
  int cnt = 0;
  for (long long q = r; q < n_rec && keys[q] == key; ++q, ++cnt) acc = __dadd_rn(acc, term[vals[q]]);     // vals: a permutation of [0, n_rec)
  const long long i = (long long)(key / (unsigned long long)N), j = (long long)(key % (unsigned long long)N);    // i < j < N: view_track_kernel
  score[i * N + j] = acc;
  score[j * N + i] = acc;
  shared[i * N + j] = cnt;
  shared[j * N + i] = cnt;
}

int check_common(const double* rot, const double* trans, int n_img, const double* pts, long long n_pts, const long long* track_off,
                 const int* track_img, long long n_obs, long long n_rec, const void* workspace, long long ws_bytes, const int* status) {
  MDF_REQUIRE(n_img >= 0 && n_img <= kMaxImages, "n_img=%d images out of range (0..%d)", n_img, kMaxImages);
  const long long lim = (1ll << 31) - kTile;
  MDF_REQUIRE(n_pts >= 0 && n_pts < lim, "n_pts=%lld points out of range", n_pts);
  MDF_REQUIRE(n_obs >= 0, "n_obs=%lld observations out of range", n_obs);
  MDF_REQUIRE(n_rec >= 0, "n_rec=%lld records out of range", n_rec);
  MDF_REQUIRE((rot && trans) || n_img == 0, "null pointer argument: rot / trans");
  MDF_REQUIRE(pts || n_pts == 0, "null pointer argument: pts");
  MDF_REQUIRE(track_off, "null pointer argument: track_off");
  MDF_REQUIRE(track_img || n_obs == 0, "null pointer argument: track_img");
  MDF_REQUIRE(status, "null pointer argument: status");
  MDF_REQUIRE(workspace, "null pointer argument: workspace");
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
  if (n_obs >= lim) return mdf::fail(MDF_EUNSUPPORTED, "%lld observations: the sort takes fewer than 2^31 - %d", n_obs, kTile);
  if (n_rec >= lim) return mdf::fail(MDF_EUNSUPPORTED, "%lld pair records: the sort takes fewer than 2^31 - %d", n_rec, kTile);
  const long long need = view_layout(nullptr, n_img, n_pts, n_obs, n_rec).bytes;
  MDF_REQUIRE(ws_bytes >= need, "workspace too small: %lld bytes, %lld needed", ws_bytes, need);
  return MDF_OK;
}

int clear(void* p, long long bytes, hipStream_t s) {
  if (bytes > 0 && hipMemsetAsync(p, 0, (size_t)bytes, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemsetAsync failed");
  return MDF_OK;
}

}  // namespace

extern "C" long long mdf_view_workspace(int n_img, long long n_pts, long long n_obs, long long n_rec) {
  if (!sizes_ok(n_img, n_pts, n_obs, n_rec)) return 0;
  return std::max(16ll, view_layout(nullptr, n_img, n_pts, n_obs, n_rec).bytes);
}

extern "C" int mdf_view_depth_ranges(const double* rot, const double* trans, int n_img, const double* pts, long long n_pts,
                                     const long long* track_off, const int* track_img, long long n_obs, double q_lo, double q_hi,
                                     void* workspace, long long ws_bytes, double* range, int* count, int* status, void* stream) {
  MDF_REQUIRE(q_lo >= 0.0 && q_hi <= 1.0 && q_lo <= q_hi, "quantiles (%g, %g) must satisfy 0 <= q_lo <= q_hi <= 1", q_lo, q_hi);
  if (int rc = check_common(rot, trans, n_img, pts, n_pts, track_off, track_img, n_obs, 0, workspace, ws_bytes, status)) return rc;
  MDF_REQUIRE((range && count) || n_img == 0, "null pointer argument: range / count");
  const ViewLayout L = view_layout(static_cast<char*>(workspace), n_img, n_pts, n_obs, 0);
  const SortBuffers& S = L.sort;
  hipStream_t s = (hipStream_t)stream;
  const int N = n_img;
  if (int rc = clear(status, 4 * sizeof(int), s)) return rc;
  if (N == 0) return MDF_OK;
  if (n_obs > 0) {
    if (int rc = clear(L.img_count, (N + 1) * (long long)sizeof(int), s)) return rc;
    hipLaunchKernelGGL(view_fill_kernel, dim3(grid_of(n_obs)), dim3(kBlock), 0, s, S.key0, S.val0, n_obs, 0ull, N);
    if (int rc = mdf::check_launch("view_fill_kernel")) return rc;
    if (n_pts > 0) {
      hipLaunchKernelGGL(view_depth_key_kernel, dim3(grid_of(n_pts)), dim3(kBlock), 0, s, rot, trans, N, pts, n_pts, track_off, track_img,
                         n_obs, S.key0, S.val0, L.img_count, status);
      if (int rc = mdf::check_launch("view_depth_key_kernel")) return rc;
    }
    const long long ntiles = (n_obs + kTile - 1) / kTile;
    if (int rc = sort_pairs(S, n_obs, ntiles, s)) return rc;
    hipLaunchKernelGGL(view_regroup_kernel, dim3(grid_of(n_obs)), dim3(kBlock), 0, s, S.key0, S.val0, n_obs, L.depth);
    if (int rc = mdf::check_launch("view_regroup_kernel")) return rc;
    if (int rc = sort_pairs(S, n_obs, ntiles, s)) return rc;
    if (int rc = scan_counts(L.img_count, N + 1, L.img_off, nullptr, s)) return rc;
  }
  hipLaunchKernelGGL(view_range_kernel, dim3(grid_of(N)), dim3(kBlock), 0, s, L.img_count, L.img_off, S.val0, L.depth, n_obs, N, q_lo, q_hi,
                     range, count);
  return mdf::check_launch("view_range_kernel");
}

extern "C" int mdf_view_scores(const double* rot, const double* trans, int n_img, const double* pts, long long n_pts,
                               const long long* track_off, const int* track_img, long long n_obs, long long n_rec, double theta0,
                               double sigma1, double sigma2, void* workspace, long long ws_bytes, double* score, int* shared, int* status,
                               void* stream) {
  MDF_REQUIRE(std::isfinite(theta0), "theta0=%g must be finite", theta0);
  MDF_REQUIRE(std::isfinite(sigma1) && sigma1 > 0 && std::isfinite(sigma2) && sigma2 > 0, "sigma1=%g, sigma2=%g must be finite and > 0",
              sigma1, sigma2);
  if (int rc = check_common(rot, trans, n_img, pts, n_pts, track_off, track_img, n_obs, n_rec, workspace, ws_bytes, status)) return rc;
  MDF_REQUIRE((score && shared) || n_img == 0, "null pointer argument: score / shared");
  const ViewLayout L = view_layout(static_cast<char*>(workspace), n_img, n_pts, n_obs, n_rec);
  const SortBuffers& S = L.sort;
  hipStream_t s = (hipStream_t)stream;
  const int N = n_img;
  if (int rc = clear(status, 4 * sizeof(int), s)) return rc;
  if (N == 0) return MDF_OK;
  if (int rc = clear(score, (long long)N * N * sizeof(double), s)) return rc;
  if (int rc = clear(shared, (long long)N * N * sizeof(int), s)) return rc;
  hipLaunchKernelGGL(view_centre_kernel, dim3(grid_of(N)), dim3(kBlock), 0, s, rot, trans, N, L.centre);
  if (int rc = mdf::check_launch("view_centre_kernel")) return rc;
  if (n_pts == 0) return MDF_OK;
  hipLaunchKernelGGL(view_track_kernel, dim3(grid_of(n_pts)), dim3(kBlock), 0, s, track_off, track_img, n_pts, n_obs, N, L.rec_count, status);
  if (int rc = mdf::check_launch("view_track_kernel")) return rc;
  if (int rc = scan_counts(L.rec_count, n_pts, L.rec_off, L.rec_total, s)) return rc;
  if (n_rec > 0) {
    hipLaunchKernelGGL(view_fill_kernel, dim3(grid_of(n_rec)), dim3(kBlock), 0, s, S.key0, S.val0, n_rec, kNoRecord, 0);
    if (int rc = mdf::check_launch("view_fill_kernel")) return rc;
  }
  hipLaunchKernelGGL(view_expand_kernel, dim3(grid_of(n_pts)), dim3(kBlock), 0, s, track_off, track_img, n_pts, N, L.rec_count, L.rec_off,
                     L.rec_total, n_rec, S.key0, S.val0, status);      // n_rec = 0: writes nothing, still compares the count
  if (int rc = mdf::check_launch("view_expand_kernel")) return rc;
  if (n_rec == 0) return MDF_OK;
  hipLaunchKernelGGL(view_term_kernel, dim3(grid_of(n_rec)), dim3(kBlock), 0, s, L.centre, pts, N, S.key0, S.val0, n_rec, theta0, sigma1,
                     sigma2, L.term);
  if (int rc = mdf::check_launch("view_term_kernel")) return rc;
  if (int rc = sort_pairs(S, n_rec, (n_rec + kTile - 1) / kTile, s)) return rc;
  hipLaunchKernelGGL(view_sum_kernel, dim3(grid_of(n_rec)), dim3(kBlock), 0, s, S.key0, S.val0, L.term, n_rec, N, score, shared);
  return mdf::check_launch("view_sum_kernel");
}
