// Point-cloud fusion of one scan's depth maps (the reference's tools/pcd/fusion.py:get_cloud, stages 2-6).  Every view is
// resident; each step reads the state before the step and writes a second buffer, which then replaces the state:
//   vis filter   pcd_reproj_kernel (mode kVis): a thread owns (reference view r, pixel); it lifts the pixel centre with r's
//                depth, projects it into each of r's sources, samples the source depth (grid_sample nearest / zeros), lifts that
//                depth again and projects it back into r; a source counts when the pixel distance is < 1 and the relative
//                depth difference < 0.01.  The pixel stays when at least `need` sources count.
//   vis fusion   per reference view: pcd_cand_count_kernel bins every candidate (r's valid pixels and every valid source pixel
//                forward-projected into r) by the pixel it lands on (integer atomics on the bin counts), a three-pass scan
//                (pcd_bin_sum_kernel, pcd_scan_kernel, pcd_bin_offsets_kernel) turns the counts into bin offsets, pcd_cand_place_kernel computes each candidate's violation count and stores
//                (depth, violations) in its bin (slot order inside a bin is arbitrary), pcd_select_kernel applies the
//                reference's rule on the sorted bin -- without sorting: an entry's sorted position is the count of entries
//                that compare less, so the result depends on the bin's multiset only and is run-independent.  Bins of more
//                than kBigBin entries are left to pcd_select_big_kernel, one block per bin (quadratic work split 256 ways).
//   ave fusion   pcd_reproj_kernel (mode kAve): (sum_v reproj_d * mask_v + d) / (sum_v mask_v + 1), sources in table order.
//   small segs   union-find over the 9x9-window graph: pcd_seg_init_kernel, pcd_seg_hook_kernel (the larger root is hooked
//                under the smaller with a CAS, so every root is its component's smallest pixel; finds halve the path),
//                pcd_seg_count_kernel (root + integer-atomic component sizes), pcd_seg_apply_kernel.
//   points       pcd_count_kernel (per-block kept counts), pcd_scan_kernel, pcd_compact_kernel (ordered compaction: view,
//                then row-major pixel; ballot + block prefix, no atomics).
// No float atomics: every output is run-independent.
//
// Arithmetic order == tests/pcd_oracle.py (torch fp32 elementwise): matrix-vector products are the left-to-right chains
// ((m0*x0 + m1*x1) + m2*x2) [+ m3*x3], every divide is IEEE, the reference's +1e-9 denominators are kept, the one square root
// goes through double; the library builds with -ffp-contract=off.
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int kCam = 64;      // floats per view in the camera table: K[9], K^-1[9], E[16], E^-1[16], centre[3], pad
constexpr int kK = 0, kKi = 9, kE = 18, kEi = 34, kCtr = 50;
constexpr int kBlock = mdf::kScanBlock;     // 256: pcd_bin_sum_kernel / pcd_bin_offsets_kernel run scan_common.h's block bodies
constexpr int kVis = 0, kAve = 1;
constexpr int kSegWin = 4;
constexpr int kBigBin = 256;     // bins above this many candidates are ranked by a whole block
constexpr int kBigBlocks = 1024;

// Views are wave-uniform in every loop below: camera entries come through the constant address space (scalar loads).
typedef const __attribute__((address_space(4))) float* cfloat_p;

struct F4 { float x, y, z, w; };
struct F3 { float x, y, z; };

__device__ __forceinline__ float d3(cfloat_p m, float x0, float x1, float x2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(m[0], x0), __fmul_rn(m[1], x1)), __fmul_rn(m[2], x2));
}
__device__ __forceinline__ float d4(cfloat_p m, float x0, float x1, float x2, float x3) {
  return __fadd_rn(d3(m, x0, x1, x2), __fmul_rn(m[3], x3));
}

// utils.idx_img2world: K^-1 (x, y, z), / (c2 + 1e-9) * d, then E^-1 (c, 1), / (w3 + 1e-9)
__device__ __forceinline__ F4 img2world(cfloat_p c, float x, float y, float z, float d) {
  const float c0 = d3(c + kKi, x, y, z), c1 = d3(c + kKi + 3, x, y, z), c2 = d3(c + kKi + 6, x, y, z);
  const float den = __fadd_rn(c2, 1e-9f);
  const float a0 = __fmul_rn(__fdiv_rn(c0, den), d), a1 = __fmul_rn(__fdiv_rn(c1, den), d), a2 = __fmul_rn(__fdiv_rn(c2, den), d);
  const float w0 = d4(c + kEi, a0, a1, a2, 1.f), w1 = d4(c + kEi + 4, a0, a1, a2, 1.f);
  const float w2 = d4(c + kEi + 8, a0, a1, a2, 1.f), w3 = d4(c + kEi + 12, a0, a1, a2, 1.f);
  const float dw = __fadd_rn(w3, 1e-9f);
  return {__fdiv_rn(w0, dw), __fdiv_rn(w1, dw), __fdiv_rn(w2, dw), __fdiv_rn(w3, dw)};
}

// utils.idx_world2cam: E w, / (q3 + 1e-9)
__device__ __forceinline__ F4 world2cam(cfloat_p c, const F4& w) {
  const float q0 = d4(c + kE, w.x, w.y, w.z, w.w), q1 = d4(c + kE + 4, w.x, w.y, w.z, w.w);
  const float q2 = d4(c + kE + 8, w.x, w.y, w.z, w.w), q3 = d4(c + kE + 12, w.x, w.y, w.z, w.w);
  const float dq = __fadd_rn(q3, 1e-9f);
  return {__fdiv_rn(q0, dq), __fdiv_rn(q1, dq), __fdiv_rn(q2, dq), __fdiv_rn(q3, dq)};
}

// utils.idx_cam2img: q[:3] / (q3 + 1e-9), K a, / (i2 + 1e-9)
__device__ __forceinline__ F3 cam2img(cfloat_p c, const F4& q) {
  const float dq = __fadd_rn(q.w, 1e-9f);
  const float a0 = __fdiv_rn(q.x, dq), a1 = __fdiv_rn(q.y, dq), a2 = __fdiv_rn(q.z, dq);
  const float i0 = d3(c + kK, a0, a1, a2), i1 = d3(c + kK + 3, a0, a1, a2), i2 = d3(c + kK + 6, a0, a1, a2);
  const float di = __fadd_rn(i2, 1e-9f);
  return {__fdiv_rn(i0, di), __fdiv_rn(i1, di), __fdiv_rn(i2, di)};
}

__device__ __forceinline__ float clamp11(float g) { return g < -1.1f ? -1.1f : (g > 1.1f ? 1.1f : g); }   // NaN stays NaN

// F.grid_sample(depth, normalize_for_grid_sample(p), 'nearest', 'zeros', align_corners=False); *in_range = get_in_range.
// The source index is (g + 1) * (size / 2) - 0.5, rounded half to even; NaN fails every comparison (zero sample).
__device__ __forceinline__ float sample_nearest(const float* __restrict__ dep, int h, int w, float px, float py, bool* in_range) {
  const float fw = (float)w, fh = (float)h;
  const float gx = clamp11(__fsub_rn(__fmul_rn(__fdiv_rn(px, fw), 2.f), 1.f));
  const float gy = clamp11(__fsub_rn(__fmul_rn(__fdiv_rn(py, fh), 2.f), 1.f));
  *in_range = gx <= 1.f && gx >= -1.f && gy <= 1.f && gy >= -1.f;
  const float rx = rintf(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.f), 0.5f * fw), 0.5f));
  const float ry = rintf(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.f), 0.5f * fh), 0.5f));
  if (!(rx >= 0.f && rx < fw && ry >= 0.f && ry < fh)) return 0.f;
  return dep[(int)ry * w + (int)rx];
}

struct StepArgs {
  const float* dep;             // [n][hw] state before the step
  const unsigned char* mask;    // [n][hw]
  float* dep_out;
  unsigned char* mask_out;
  const float* cams;            // [n][kCam]
  const int* srcs;              // [n][v], -1 = none
  int n, h, w, v, need;
};

template <int MODE>
__global__ __launch_bounds__(kBlock) void pcd_reproj_kernel(const StepArgs p) {
  const int r = blockIdx.y;
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  const cfloat_p cams = (cfloat_p)p.cams;
  const cfloat_p cr = cams + kCam * r;
  const size_t at = (size_t)r * hw + pix;
  const float d = p.dep[at];
  const bool m_in = p.mask[at] != 0;
  const int yi = pix / p.w, xi = pix - yi * p.w;
  const float xs = (float)xi + 0.5f, ys = (float)yi + 0.5f;
  int cnt = 0;
  float sum = 0.f;
  if (d > 1e-9f) {
    const F4 wr = img2world(cr, xs, ys, 1.f, d);
    for (int k = 0; k < p.v; ++k) {
      const int s = p.srcs[r * p.v + k];
      if (s < 0 || s >= p.n) continue;               // -1 = none; an index past the scan is ignored, never read
      const cfloat_p cs = cams + kCam * s;
      const F3 i = cam2img(cs, world2cam(cs, wr));
      bool inr;
      const float g = sample_nearest(p.dep + (size_t)s * hw, p.h, p.w, i.x, i.y, &inr);
      inr = inr && g > 1e-9f;
      const F4 q = world2cam(cr, img2world(cs, i.x, i.y, i.z, g));
      const F3 j = cam2img(cr, q);
      const float rd = q.z;
      const float dx = __fsub_rn(j.x, xs), dy = __fsub_rn(j.y, ys);
      const float dist = (float)__dsqrt_rn((double)__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
      const float lim = __fmul_rn(fmaxf(d, rd), 0.01f);
      const bool m = inr && dist < 1.f && fabsf(__fsub_rn(d, rd)) < lim;
      cnt += m ? 1 : 0;
      if (MODE == kAve) sum = __fadd_rn(sum, __fmul_rn(rd, m ? 1.f : 0.f));
    }
  }
  if (MODE == kVis) {
    const bool keep = m_in && cnt >= p.need;
    p.mask_out[at] = keep ? 1 : 0;
    p.dep_out[at] = __fmul_rn(d, keep ? 1.f : 0.f);
  } else {
    const float ave = __fdiv_rn(__fadd_rn(sum, d), __fadd_rn((float)cnt, 1.f));
    p.mask_out[at] = m_in ? 1 : 0;
    p.dep_out[at] = __fmul_rn(ave, m_in ? 1.f : 0.f);
  }
}

// ---------------------------------------------------------------------------------------------------- visibility fusion
struct FusionArgs {
  const float* dep;             // [n][hw] state before the step
  const unsigned char* mask;
  float* dep_out;
  const float* cams;
  const int* srcs;
  int* bin_count;               // [hw]
  const long long* bin_off;     // [hw]
  int2* entries;                // [(v+1) hw]: (depth bits, violations)
  long long capacity;
  int* big_list;                // [hw] bins too large for one lane, then their count at big_list[hw]
  int r, n, h, w, v;
};

struct Cand { float x, y, z, d; int bin; };

// Candidate j of reference view r at pixel pix: j = 0 is r's own pixel, j = k+1 source k's pixel in r's image.  -> bin, or -1.
__device__ __forceinline__ Cand candidate(const FusionArgs& p, int j, int pix) {
  const int hw = p.h * p.w;
  const cfloat_p cams = (cfloat_p)p.cams;
  const cfloat_p cr = cams + kCam * p.r;
  const int yi = pix / p.w, xi = pix - yi * p.w;
  const float xs = (float)xi + 0.5f, ys = (float)yi + 0.5f;
  Cand c{xs, ys, 1.f, 0.f, -1};
  if (j == 0) {
    c.d = p.dep[(size_t)p.r * hw + pix];
    if (!(c.d > 1e-9f)) return c;
  } else {
    const int s = p.srcs[p.r * p.v + j - 1];
    if (s < 0 || s >= p.n) return c;
    const float ds = p.dep[(size_t)s * hw + pix];
    if (!(ds > 1e-9f)) return c;
    const F4 q = world2cam(cr, img2world(cams + kCam * s, xs, ys, 1.f, ds));
    const F3 i = cam2img(cr, q);
    c.x = i.x; c.y = i.y; c.z = i.z; c.d = q.z;
  }
  // fusion.cpp: int(std::round(xy - .5)) in double, INRANGE, depth > 1e-9 in double, valid[y][x]
  const double tx = (double)c.x - 0.5, ty = (double)c.y - 0.5;
  if (!(tx > -0.5 && tx < p.w - 0.5 && ty > -0.5 && ty < p.h - 0.5 && (double)c.d > 1e-9)) return c;
  const int bx = (int)round(tx), by = (int)round(ty);
  const int bin = by * p.w + bx;
  if (p.dep[(size_t)p.r * hw + bin] > 1e-9f) c.bin = bin;
  return c;
}

__global__ __launch_bounds__(kBlock) void pcd_cand_count_kernel(const FusionArgs p) {
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= p.h * p.w) return;
  const Cand c = candidate(p, blockIdx.y, pix);
  if (c.bin >= 0) atomicAdd(&p.bin_count[c.bin], 1);
}

__global__ __launch_bounds__(kBlock) void pcd_cand_place_kernel(const FusionArgs p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  const Cand c = candidate(p, blockIdx.y, pix);
  if (c.bin < 0) return;
  const cfloat_p cams = (cfloat_p)p.cams;
  const F4 wr = img2world(cams + kCam * p.r, c.x, c.y, c.z, c.d);
  int vio = 0;
  for (int k = 0; k < p.v; ++k) {
    const int s = p.srcs[p.r * p.v + k];
    if (s < 0 || s >= p.n) continue;
    const cfloat_p cs = cams + kCam * s;
    const F4 q = world2cam(cs, wr);
    const F3 i = cam2img(cs, q);
    bool inr;
    const float g = sample_nearest(p.dep + (size_t)s * hw, p.h, p.w, i.x, i.y, &inr);
    vio += g > q.z ? 1 : 0;
  }
  const long long slot = p.bin_off[c.bin] + atomicAdd(&p.bin_count[c.bin], 1);
  if (slot < p.capacity) p.entries[slot] = make_int2(__float_as_int(c.d), vio);
}

__device__ __forceinline__ bool lex_less(float da, int va, float db, int vb) { return da < db || (da == db && va < vb); }

// The bin's output: with the entries sorted by (depth, violations), the first position k with k >= violations[k], else the
// last entry.  An entry group of equal (d, vio) occupies positions [lo, lo + eq); it holds a qualifying position iff
// lo + eq - 1 >= vio, the first being max(lo, vio).  Positions of different groups are disjoint, so the minimum is unique.
__global__ __launch_bounds__(kBlock) void pcd_select_kernel(const FusionArgs p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  const size_t at = (size_t)p.r * hw + pix;
  const int nb = p.bin_count[pix];
  if (nb > kBigBin) {                             // quadratic in one lane is too slow: a block takes it (pcd_select_big_kernel)
    p.big_list[atomicAdd(p.big_list + hw, 1)] = pix;
    return;
  }
  float out = 0.f;
  if (nb > 0) {
    const int2* e = p.entries + p.bin_off[pix];
    int best = 0x7fffffff;
    float best_d = 0.f, max_d = __int_as_float(e[0].x);
    int max_v = e[0].y;
    for (int i = 0; i < nb; ++i) {
      const float di = __int_as_float(e[i].x);
      const int vi = e[i].y;
      if (lex_less(max_d, max_v, di, vi)) { max_d = di; max_v = vi; }
      int lo = 0, eq = 0;
      for (int j = 0; j < nb; ++j) {
        const float dj = __int_as_float(e[j].x);
        const int vj = e[j].y;
        lo += lex_less(dj, vj, di, vi) ? 1 : 0;
        eq += (dj == di && vj == vi) ? 1 : 0;
      }
      if (lo + eq - 1 >= vi) {
        const int pos = max(lo, vi);
        if (pos < best) { best = pos; best_d = di; }
      }
    }
    out = best == 0x7fffffff ? max_d : best_d;
  }
  p.dep_out[at] = __fmul_rn(out, p.mask[at] ? 1.f : 0.f);
}

// The same rule for the bins pcd_select_kernel deferred, one block per bin: each thread ranks a strided share of the entries
// against the whole bin; the first qualifying position (unique, see above) is an LDS atomicMin, and its owner writes the depth.
// With no qualifying position the output is the last entry, the one with lo + eq == nb (all such entries are equal).
__global__ __launch_bounds__(kBlock) void pcd_select_big_kernel(const FusionArgs p) {
  __shared__ int best;
  __shared__ float res;
  const int hw = p.h * p.w;
  const int nbig = p.big_list[hw];
  for (int b = blockIdx.x; b < nbig; b += gridDim.x) {
    const int pix = p.big_list[b];
    const int nb = p.bin_count[pix];
    const int2* e = p.entries + p.bin_off[pix];
    if (threadIdx.x == 0) best = 0x7fffffff;
    __syncthreads();
    int my_pos = 0x7fffffff;
    float my_d = 0.f;
    for (int i = threadIdx.x; i < nb; i += kBlock) {
      const float di = __int_as_float(e[i].x);
      const int vi = e[i].y;
      int lo = 0, eq = 0;
      for (int j = 0; j < nb; ++j) {
        const float dj = __int_as_float(e[j].x);
        const int vj = e[j].y;
        lo += lex_less(dj, vj, di, vi) ? 1 : 0;
        eq += (dj == di && vj == vi) ? 1 : 0;
      }
      if (lo + eq == nb) res = di;                // the last entry (every writer writes the same value)
      if (lo + eq - 1 >= vi && max(lo, vi) < my_pos) { my_pos = max(lo, vi); my_d = di; }
    }
    if (my_pos != 0x7fffffff) atomicMin(&best, my_pos);
    __syncthreads();
    if (my_pos == best && my_pos != 0x7fffffff) res = my_d;     // the one owner of the unique first position
    __syncthreads();
    if (threadIdx.x == 0) {
      const size_t at = (size_t)p.r * hw + pix;
      p.dep_out[at] = __fmul_rn(res, p.mask[at] ? 1.f : 0.f);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- small segments
struct SegArgs {
  float* dep;                   // [n][hw], updated in place by the apply kernel
  unsigned char* mask;
  int* parent;                  // [n][hw] view-local pixel index, -1 = invalid pixel
  int* size;                    // [n][hw] component sizes at the roots
  int h, w, min_size;
  float diff;
};

__device__ __forceinline__ bool seg_valid(float d) { return !((double)d < 1e-9); }   // fusion.cpp: depth < 1e-9 -> FINISH
__device__ __forceinline__ bool seg_link(float a, float b, float diff) {
  return !(fabsf(__fsub_rn(a, b)) >= __fmul_rn(diff, __fadd_rn(a, b)));
}

// Root of x with path halving: x's parent is replaced by its grandparent on the way up.  Parents only ever move to an
// ancestor (a root is hooked under a smaller root, never re-parented otherwise), so the racy halving store is safe.
__device__ __forceinline__ int seg_find(int* par, int x) {
  while (true) {
    const int q = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == x) return x;
    const int g = __hip_atomic_load(par + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g != q) __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

__global__ __launch_bounds__(kBlock) void pcd_seg_init_kernel(const SegArgs p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  const size_t at = (size_t)blockIdx.y * hw + pix;
  p.parent[at] = seg_valid(p.dep[at]) ? pix : -1;
  p.size[at] = 0;
}

__global__ __launch_bounds__(kBlock) void pcd_seg_hook_kernel(const SegArgs p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  const float* dep = p.dep + (size_t)blockIdx.y * hw;
  int* par = p.parent + (size_t)blockIdx.y * hw;
  const float a = dep[pix];
  if (!seg_valid(a)) return;
  const int y = pix / p.w, x = pix - y * p.w;
  for (int dy = 0; dy <= kSegWin; ++dy) {
    const int yy = y + dy;
    if (yy >= p.h) break;
    for (int dx = -kSegWin; dx <= kSegWin; ++dx) {
      if (dy == 0 && dx <= 0) continue;           // each unordered pair once: the later pixel in row-major order
      const int xx = x + dx;
      if (xx < 0 || xx >= p.w) continue;
      const int q = yy * p.w + xx;
      const float b = dep[q];
      if (!seg_valid(b) || !seg_link(a, b, p.diff)) continue;
      int u = pix, v = q;
      while (true) {
        u = seg_find(par, u);
        v = seg_find(par, v);
        if (u == v) break;
        if (u < v) { const int t = u; u = v; v = t; }
        const int old = atomicCAS(par + u, u, v);       // u (the larger root) goes under v
        if (old == u) break;
        u = old;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void pcd_seg_count_kernel(const SegArgs p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  int* par = p.parent + (size_t)blockIdx.y * hw;
  if (par[pix] < 0) return;
  const int root = seg_find(par, pix);
  atomicAdd(p.size + (size_t)blockIdx.y * hw + root, 1);
}

__global__ __launch_bounds__(kBlock) void pcd_seg_apply_kernel(const SegArgs p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  const size_t at = (size_t)blockIdx.y * hw + pix;
  int* par = p.parent + (size_t)blockIdx.y * hw;
  const bool seg = par[pix] >= 0 && p.size[(size_t)blockIdx.y * hw + seg_find(par, pix)] >= p.min_size;
  const bool keep = p.mask[at] != 0 && seg;
  p.mask[at] = keep ? 1 : 0;
  p.dep[at] = __fmul_rn(p.dep[at], keep ? 1.f : 0.f);
}

// ---------------------------------------------------------------------------------------------------- points
__global__ __launch_bounds__(kBlock) void pcd_count_kernel(const unsigned char* __restrict__ mask, int hw, int nblk,
                                                           int* __restrict__ counts) {
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  const bool keep = pix < hw && mask[(size_t)blockIdx.y * hw + pix] != 0;
  const int kept = __syncthreads_count(keep ? 1 : 0);
  if (threadIdx.x == 0) counts[blockIdx.y * nblk + blockIdx.x] = kept;
}

// Exclusive scan of nitems counts in one block.  With nblk > 0, view v's total is the sum of items [v*nblk, (v+1)*nblk).
__global__ __launch_bounds__(mdf::kScanThreads) void pcd_scan_kernel(const int* __restrict__ counts, long long* __restrict__ offsets,
                                                                int nitems, int nblk, int n, int* __restrict__ view_counts,
                                                                long long* __restrict__ total) {
  mdf::block_exclusive_scan<int, true>(counts, nitems, offsets, total, nblk, n, view_counts);
}

// Bin offsets of one reference view, a three-pass scan over many blocks (one block walking 2M counts in sequence took ~4.4 ms
// a view): pcd_bin_sum_kernel sums each kBinChunk-count chunk, pcd_scan_kernel scans the chunk sums, pcd_bin_offsets_kernel
// scans inside each chunk from its offset.
constexpr int kBinPer = 4, kBinChunk = kBlock * kBinPer;

__global__ __launch_bounds__(kBlock) void pcd_bin_sum_kernel(const int* __restrict__ counts, int n, int* __restrict__ sums) {
  const int base = blockIdx.x * kBinChunk + threadIdx.x * kBinPer;
  int t = 0;
  for (int k = 0; k < kBinPer; ++k) t += base + k < n ? counts[base + k] : 0;
  const int sum = mdf::block_sum(t);
  if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kBlock) void pcd_bin_offsets_kernel(const int* __restrict__ counts, int n,
                                                                 const long long* __restrict__ chunk_off,
                                                                 long long* __restrict__ offsets) {
  const int base = blockIdx.x * kBinChunk + threadIdx.x * kBinPer;
  int c[kBinPer];
  int t = 0;
  for (int k = 0; k < kBinPer; ++k) {
    c[k] = base + k < n ? counts[base + k] : 0;
    t += c[k];
  }
  long long run = chunk_off[blockIdx.x] + (mdf::block_inclusive_scan(t) - t);
  for (int k = 0; k < kBinPer; ++k) {
    if (base + k < n) offsets[base + k] = run;
    run += c[k];
  }
}

struct CompactArgs {
  const float* dep;
  const unsigned char* mask;
  const unsigned char* rgb;     // [n][hw][3]
  const float* cams;
  const long long* offsets;     // [n][nblk]
  float* xyz;
  unsigned char* rgb_out;
  float* dirs;
  long long capacity;
  int h, w, nblk;
};

__global__ __launch_bounds__(kBlock) void pcd_compact_kernel(const CompactArgs p) {
  __shared__ int wave_base[kBlock / 64];
  const int r = blockIdx.y;
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  const size_t at = (size_t)r * hw + pix;
  const bool keep = pix < hw && p.mask[at] != 0;
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wave_base[wave] = __popcll(m);
  __syncthreads();
  int base = 0;
  for (int i = 0; i < wave; ++i) base += wave_base[i];
  if (!keep) return;
  const long long o = p.offsets[r * p.nblk + blockIdx.x] + base + before;
  if (o >= p.capacity) return;
  const cfloat_p cr = (cfloat_p)p.cams + kCam * r;
  const int yi = pix / p.w, xi = pix - yi * p.w;
  const F4 w = img2world(cr, (float)xi + 0.5f, (float)yi + 0.5f, 1.f, p.dep[at]);
  p.xyz[3 * o + 0] = w.x;
  p.xyz[3 * o + 1] = w.y;
  p.xyz[3 * o + 2] = w.z;
  p.dirs[3 * o + 0] = __fsub_rn(cr[kCtr + 0], w.x);
  p.dirs[3 * o + 1] = __fsub_rn(cr[kCtr + 1], w.y);
  p.dirs[3 * o + 2] = __fsub_rn(cr[kCtr + 2], w.z);
  p.rgb_out[3 * o + 0] = p.rgb[3 * at + 0];
  p.rgb_out[3 * o + 1] = p.rgb[3 * at + 1];
  p.rgb_out[3 * o + 2] = p.rgb[3 * at + 2];
}

inline int nblocks(long long items) { return (int)((items + kBlock - 1) / kBlock); }
inline long long align16(long long b) { return (b + 15) & ~15ll; }

// Workspace: dep2 [n*hw] f32 | mask2 [n*hw] u8 | parent [n*hw] i32 | size [n*hw] i32 | bin_count [hw] i32 | bin_off [hw] i64 |
// entries [(v+1)*hw] int2 | block counts [n*nblk] i32 | block offsets [n*nblk] i64   (each 16-byte aligned)
struct WsLayout {
  float* dep2;
  unsigned char* mask2;
  int *parent, *size, *bin_count, *block_counts, *big_list, *chunk_sums;
  long long* chunk_off;
  int nchunk;
  long long *bin_off, *block_off;
  int2* entries;
  long long entries_cap;
  int hw, nblk;
  long long bytes;
};

WsLayout ws_layout(char* ws, int n, int h, int w, int v) {
  WsLayout L{};
  const long long hw = (long long)h * w, nhw = n * hw;
  L.hw = (int)hw;
  L.nblk = nblocks(hw);
  L.entries_cap = (v + 1) * hw;
  long long o = 0;
  auto take = [&](long long bytes) { const long long at = o; o += align16(bytes); return ws + at; };
  L.dep2 = reinterpret_cast<float*>(take(nhw * 4));
  L.mask2 = reinterpret_cast<unsigned char*>(take(nhw));
  L.parent = reinterpret_cast<int*>(take(nhw * 4));
  L.size = reinterpret_cast<int*>(take(nhw * 4));
  L.bin_count = reinterpret_cast<int*>(take(hw * 4));
  L.bin_off = reinterpret_cast<long long*>(take(hw * 8));
  L.big_list = reinterpret_cast<int*>(take((hw + 1) * 4));
  L.nchunk = (int)((hw + kBinChunk - 1) / kBinChunk);
  L.chunk_sums = reinterpret_cast<int*>(take((long long)L.nchunk * 4));
  L.chunk_off = reinterpret_cast<long long*>(take((long long)L.nchunk * 8));
  L.entries = reinterpret_cast<int2*>(take(L.entries_cap * 8));
  L.block_counts = reinterpret_cast<int*>(take((long long)n * L.nblk * 4));
  L.block_off = reinterpret_cast<long long*>(take((long long)n * L.nblk * 8));
  L.bytes = o;
  return L;
}

int check_shape(int n, int h, int w, int v) {
  MDF_REQUIRE(n >= 1 && n <= MDF_MAX_FUSE_VIEWS, "n=%d views out of range [1,%d]", n, MDF_MAX_FUSE_VIEWS);
  MDF_REQUIRE(v >= 0 && v <= MDF_PCD_MAX_SOURCES, "v=%d sources out of range [0,%d]", v, MDF_PCD_MAX_SOURCES);
  MDF_REQUIRE(h >= 1 && w >= 1 && (long long)h * w * (v + 1) < (1ll << 31), "bad shape %dx%d with %d sources", h, w, v);
  MDF_REQUIRE((long long)n * ((h * w + kBlock - 1) / kBlock) < (1ll << 31), "too many blocks");
  return MDF_OK;
}

int run_fusion(const StepArgs& sp, const WsLayout& L, hipStream_t s) {
  FusionArgs f{};
  f.dep = sp.dep; f.mask = sp.mask; f.dep_out = sp.dep_out; f.cams = sp.cams; f.srcs = sp.srcs;
  f.bin_count = L.bin_count; f.bin_off = L.bin_off; f.entries = L.entries; f.capacity = L.entries_cap;
  f.big_list = L.big_list;
  f.n = sp.n; f.h = sp.h; f.w = sp.w; f.v = sp.v;
  const dim3 grid(L.nblk, sp.v + 1);
  for (int r = 0; r < sp.n; ++r) {
    f.r = r;
    if (hipMemsetAsync(L.bin_count, 0, (size_t)L.hw * 4, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(pcd_cand_count_kernel, grid, dim3(kBlock), 0, s, f);
    if (int rc = mdf::check_launch("pcd_cand_count_kernel")) return rc;
    hipLaunchKernelGGL(pcd_bin_sum_kernel, dim3(L.nchunk), dim3(kBlock), 0, s, L.bin_count, L.hw, L.chunk_sums);
    if (int rc = mdf::check_launch("pcd_bin_sum_kernel")) return rc;
    hipLaunchKernelGGL(pcd_scan_kernel, dim3(1), dim3(mdf::kScanThreads), 0, s, L.chunk_sums, L.chunk_off, L.nchunk, 0, 0, nullptr, nullptr);
    if (int rc = mdf::check_launch("pcd_scan_kernel")) return rc;
    hipLaunchKernelGGL(pcd_bin_offsets_kernel, dim3(L.nchunk), dim3(kBlock), 0, s, L.bin_count, L.hw, L.chunk_off, L.bin_off);
    if (int rc = mdf::check_launch("pcd_bin_offsets_kernel")) return rc;
    if (hipMemsetAsync(L.bin_count, 0, (size_t)L.hw * 4, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(pcd_cand_place_kernel, grid, dim3(kBlock), 0, s, f);
    if (int rc = mdf::check_launch("pcd_cand_place_kernel")) return rc;
    if (hipMemsetAsync(L.big_list + L.hw, 0, 4, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(pcd_select_kernel, dim3(L.nblk), dim3(kBlock), 0, s, f);
    if (int rc = mdf::check_launch("pcd_select_kernel")) return rc;
    hipLaunchKernelGGL(pcd_select_big_kernel, dim3(kBigBlocks), dim3(kBlock), 0, s, f);
    if (int rc = mdf::check_launch("pcd_select_big_kernel")) return rc;
  }
  return MDF_OK;
}

}  // namespace

extern "C" long long mdf_pcd_fuse_workspace(int n, int h, int w, int v) {
  if (n < 1 || h < 1 || w < 1 || v < 0) return 0;
  return ws_layout(nullptr, n, h, w, v).bytes;
}

extern "C" int mdf_pcd_fuse_fwd(float* depths, unsigned char* masks, const float* cams, const int* srcs, int n, int h, int w,
                                int v, int need, int first_step, int last_step, void* workspace, int* view_counts,
                                long long* total, void* stream) {
  MDF_REQUIRE(depths && masks && cams && workspace && view_counts && total, "null pointer argument");
  MDF_REQUIRE(srcs || v == 0, "null pointer argument: srcs");
  if (int rc = check_shape(n, h, w, v)) return rc;
  MDF_REQUIRE(first_step >= MDF_PCD_STEP_VIS1 && last_step <= MDF_PCD_STEP_SEG, "steps [%d,%d] out of range [%d,%d]", first_step,
              last_step, MDF_PCD_STEP_VIS1, MDF_PCD_STEP_SEG);
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
  const WsLayout L = ws_layout(static_cast<char*>(workspace), n, h, w, v);
  hipStream_t s = (hipStream_t)stream;
  const size_t nhw = (size_t)n * L.hw;
  StepArgs sp{depths, masks, L.dep2, L.mask2, cams, srcs, n, h, w, v, need};
  const dim3 grid(L.nblk, n);
  for (int step = first_step; step <= last_step; ++step) {
    if (step == MDF_PCD_STEP_SEG) {
      SegArgs g{depths, masks, L.parent, L.size, h, w, 10, 1e-3f};
      hipLaunchKernelGGL(pcd_seg_init_kernel, grid, dim3(kBlock), 0, s, g);
      if (int rc = mdf::check_launch("pcd_seg_init_kernel")) return rc;
      hipLaunchKernelGGL(pcd_seg_hook_kernel, grid, dim3(kBlock), 0, s, g);
      if (int rc = mdf::check_launch("pcd_seg_hook_kernel")) return rc;
      hipLaunchKernelGGL(pcd_seg_count_kernel, grid, dim3(kBlock), 0, s, g);
      if (int rc = mdf::check_launch("pcd_seg_count_kernel")) return rc;
      hipLaunchKernelGGL(pcd_seg_apply_kernel, grid, dim3(kBlock), 0, s, g);
      if (int rc = mdf::check_launch("pcd_seg_apply_kernel")) return rc;
      continue;                                            // in place: every pixel reads and writes only itself
    }
    if (step == MDF_PCD_STEP_FUSION) {
      if (hipMemcpyAsync(L.mask2, masks, nhw, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return mdf::fail(MDF_EHIP, "hipMemcpyAsync failed");
      if (int rc = run_fusion(sp, L, s)) return rc;
    } else if (step == MDF_PCD_STEP_AVE) {
      hipLaunchKernelGGL(pcd_reproj_kernel<kAve>, grid, dim3(kBlock), 0, s, sp);
      if (int rc = mdf::check_launch("pcd_reproj_kernel")) return rc;
    } else {
      hipLaunchKernelGGL(pcd_reproj_kernel<kVis>, grid, dim3(kBlock), 0, s, sp);
      if (int rc = mdf::check_launch("pcd_reproj_kernel")) return rc;
    }
    if (hipMemcpyAsync(depths, L.dep2, nhw * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(masks, L.mask2, nhw, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return mdf::fail(MDF_EHIP, "hipMemcpyAsync failed");
  }
  hipLaunchKernelGGL(pcd_count_kernel, grid, dim3(kBlock), 0, s, masks, L.hw, L.nblk, L.block_counts);
  if (int rc = mdf::check_launch("pcd_count_kernel")) return rc;
  hipLaunchKernelGGL(pcd_scan_kernel, dim3(1), dim3(mdf::kScanThreads), 0, s, L.block_counts, L.block_off, n * L.nblk, L.nblk, n,
                     view_counts, total);
  return mdf::check_launch("pcd_scan_kernel");
}

extern "C" int mdf_pcd_compact(const float* depths, const unsigned char* masks, const unsigned char* rgb, const float* cams, int n,
                               int h, int w, int v, void* workspace, float* xyz, unsigned char* rgb_out, float* dirs,
                               long long capacity, void* stream) {
  MDF_REQUIRE(depths && masks && rgb && cams && workspace && xyz && rgb_out && dirs, "null pointer argument");
  MDF_REQUIRE(capacity >= 0, "negative capacity");
  if (int rc = check_shape(n, h, w, v)) return rc;
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
  const WsLayout L = ws_layout(static_cast<char*>(workspace), n, h, w, v);
  CompactArgs c{depths, masks, rgb, cams, L.block_off, xyz, rgb_out, dirs, capacity, h, w, L.nblk};
  hipLaunchKernelGGL(pcd_compact_kernel, dim3(L.nblk, n), dim3(kBlock), 0, (hipStream_t)stream, c);
  return mdf::check_launch("pcd_compact_kernel");
}
