// What the warp kernels share (eval: warp_aggregate.hip; training: warp_aggregate_train.hip, warp_variance_train.hip), each
// piece defined once: sample-position arithmetic (bit-exact w.r.t. torch's CPU path), the bilinear tap table entry and the two
// forms of its fill (phase A), the four-tap gather and blend, DPP reductions over the lanes of a pixel, the soft-maxes, and the
// argument checks of the entry points.  The scatter side of the backward kernels is in warp_scatter.h.
// Compile with -ffp-contract=off: every fused multiply-add below is explicit.
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 256;

// Pixels of a block's tile.  TH = 0: a run of PPB consecutive pixels in row-major order (wraps over row ends); TH > 0: a
// (PPB / TH) x TH rectangle -- the taps of vertically neighbouring pixels share source texels inside ONE block's L1 working set
// instead of across blocks, and a tile's footprint in a source map is a compact box instead of a slanted line.
#ifndef MDF_WARP_TILE_H
#define MDF_WARP_TILE_H 0
#endif
template <int PPB, int TH = MDF_WARP_TILE_H>
struct PixTile {
  static constexpr int TW = (TH > 0) ? PPB / TH : PPB;
  static_assert(TH == 0 || TW * TH == PPB, "tile shape");
  int x0, y0, lin0;
  __device__ __forceinline__ PixTile(int tile, int W) {
    if constexpr (TH > 0) {
      const int tx = (W + TW - 1) / TW;
      y0 = (tile / tx) * TH; x0 = (tile % tx) * TW; lin0 = 0;
    } else {
      x0 = y0 = 0; lin0 = tile * PPB;
    }
  }
  // -> linear pixel index and coordinates (clamped into the map), live = the tile slot is a pixel of the map
  __device__ __forceinline__ int pix(int pl, int W, int H, int& x, int& y, bool& live) const {
    if constexpr (TH > 0) {
      live = (x0 + pl % TW) < W && (y0 + pl / TW) < H;
      y = min(y0 + pl / TW, H - 1); x = min(x0 + pl % TW, W - 1);
      return y * W + x;
    } else {
      live = (lin0 + pl) < W * H;
      const int q = min(lin0 + pl, W * H - 1);
      y = q / W; x = q - y * W;
      return q;
    }
  }
  __device__ __forceinline__ int pix(int pl, int W, int H, bool& live) const {
    int x, y;
    return pix(pl, W, H, x, y, live);
  }
  static int blocks(int W, int H) {
    if constexpr (TH > 0) return ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
    else return (W * H + PPB - 1) / PPB;
  }
};

struct Geom {
  float half_w, half_h;  // f32((w-1)/2), f32((h-1)/2)       base.py:117-118
  float sw, sh;          // f32(w/2), f32(h/2)               ATen unnormalise scale
  int w, h;
};

// Sample position in source pixel units.  Rounding order == torch 2.10 CPU (verified bitwise by
// tests/test_oracle_golden.py against the real reference):
//   rot_xyz_i = fma(r_i2, 1, fma(r_i1, y, r_i0*x))      base.py:110 (MKL sgemm, K = 3)
//   P = rot_xyz*depth ; P += t ; px = Px/Pz ; py = Py/Pz  base.py:112-115 (no z>0 test)
//   xn = px / f32((w-1)/2) - 1                             base.py:117 (true divide)
//   ix = fma(xn + 1, w/2, -0.5)                            grid_sample(align_corners=False), FMA-contracted
// The two halves of warp_position: the part that depends on (pixel, view) only -- rot_xyz and the translation --, and the part per
// depth hypothesis.  A kernel whose threads keep their (pixel, view) pair over the planes computes the first half once.
struct PixelRay {
  float q0, q1, q2, t0, t1, t2;
};
__device__ __forceinline__ PixelRay warp_ray(const float* __restrict__ m, float x, float y) {
  PixelRay r;
  r.q0 = __fadd_rn(m[2], __fmaf_rn(m[1], y, __fmul_rn(m[0], x)));
  r.q1 = __fadd_rn(m[6], __fmaf_rn(m[5], y, __fmul_rn(m[4], x)));
  r.q2 = __fadd_rn(m[10], __fmaf_rn(m[9], y, __fmul_rn(m[8], x)));
  r.t0 = m[3]; r.t1 = m[7]; r.t2 = m[11];
  return r;
}
__device__ __forceinline__ void warp_position_ray(const PixelRay& r, float dep, const Geom& g, float& ix, float& iy) {
  const float X = __fadd_rn(__fmul_rn(r.q0, dep), r.t0);
  const float Y = __fadd_rn(__fmul_rn(r.q1, dep), r.t1);
  const float Z = __fadd_rn(__fmul_rn(r.q2, dep), r.t2);
  const float px = __fdiv_rn(X, Z);
  const float py = __fdiv_rn(Y, Z);
  const float xn = __fsub_rn(__fdiv_rn(px, g.half_w), 1.0f);
  const float yn = __fsub_rn(__fdiv_rn(py, g.half_h), 1.0f);
  ix = __fmaf_rn(__fadd_rn(xn, 1.0f), g.sw, -0.5f);
  iy = __fmaf_rn(__fadd_rn(yn, 1.0f), g.sh, -0.5f);
}

__device__ __forceinline__ void warp_position(const float* __restrict__ m, float x, float y, float dep,
                                              const Geom& g, float& ix, float& iy) {
  const float q0 = __fadd_rn(m[2], __fmaf_rn(m[1], y, __fmul_rn(m[0], x)));
  const float q1 = __fadd_rn(m[6], __fmaf_rn(m[5], y, __fmul_rn(m[4], x)));
  const float q2 = __fadd_rn(m[10], __fmaf_rn(m[9], y, __fmul_rn(m[8], x)));
  const float X = __fadd_rn(__fmul_rn(q0, dep), m[3]);
  const float Y = __fadd_rn(__fmul_rn(q1, dep), m[7]);
  const float Z = __fadd_rn(__fmul_rn(q2, dep), m[11]);
  const float px = __fdiv_rn(X, Z);
  const float py = __fdiv_rn(Y, Z);
  const float xn = __fsub_rn(__fdiv_rn(px, g.half_w), 1.0f);
  const float yn = __fsub_rn(__fdiv_rn(py, g.half_h), 1.0f);
  ix = __fmaf_rn(__fadd_rn(xn, 1.0f), g.sw, -0.5f);
  iy = __fmaf_rn(__fadd_rn(yn, 1.0f), g.sh, -0.5f);
}

struct __attribute__((aligned(16))) TapEntry {
  int off[4];   // float offsets of the nw, ne, sw, se taps inside one [h,w,C] map (clamped in range)
  float wt[4];  // bilinear weights; 0 for out-of-bounds taps, NaN for non-finite positions
};

// Weights (bit-exact w.r.t. ATen's grid_sampler) and clamped integer corners of one bilinear sample.
__device__ __forceinline__ void tap_weights_corners(float ix, float iy, const Geom& g, float* wt, int& xa, int& xb, int& ya, int& yb) {
  const float x0f = floorf(ix), y0f = floorf(iy);
  const float fw = __fsub_rn(ix, x0f), fe = __fsub_rn(1.0f, fw);
  const float fn = __fsub_rn(iy, y0f), fs = __fsub_rn(1.0f, fn);
  const float wnw = __fmul_rn(fs, fe), wne = __fmul_rn(fs, fw), wsw = __fmul_rn(fn, fe), wse = __fmul_rn(fn, fw);
  const float x1f = x0f + 1.0f, y1f = y0f + 1.0f;
  const float mw = (float)(g.w - 1), mh = (float)(g.h - 1);
  const bool bx0 = (x0f >= 0.0f) && (x0f <= mw), bx1 = (x1f >= 0.0f) && (x1f <= mw);
  const bool by0 = (y0f >= 0.0f) && (y0f <= mh), by1 = (y1f >= 0.0f) && (y1f <= mh);
  // out-of-bounds taps read 0 in the reference; w*0 keeps NaN/inf weights NaN (z == 0 planes -> NaN).
  wt[0] = (bx0 && by0) ? wnw : __fmul_rn(wnw, 0.0f);
  wt[1] = (bx1 && by0) ? wne : __fmul_rn(wne, 0.0f);
  wt[2] = (bx0 && by1) ? wsw : __fmul_rn(wsw, 0.0f);
  wt[3] = (bx1 && by1) ? wse : __fmul_rn(wse, 0.0f);
  const int xi = (int)fminf(fmaxf(x0f, -2.0f), (float)g.w);  // NaN -> -2
  const int yi = (int)fminf(fmaxf(y0f, -2.0f), (float)g.h);
  xa = min(max(xi, 0), g.w - 1); xb = min(max(xi + 1, 0), g.w - 1);
  ya = min(max(yi, 0), g.h - 1); yb = min(max(yi + 1, 0), g.h - 1);
}

// `texel` = floats per texel of the map the offsets address (C, or G for pair-difference maps)
__device__ __forceinline__ void make_taps(float ix, float iy, const Geom& g, int texel, TapEntry& t) {
  int xa, xb, ya, yb;
  tap_weights_corners(ix, iy, g, t.wt, xa, xb, ya, yb);
  t.off[0] = (ya * g.w + xa) * texel;
  t.off[1] = (ya * g.w + xb) * texel;
  t.off[2] = (yb * g.w + xa) * texel;
  t.off[3] = (yb * g.w + xb) * texel;
}

// The same sample with its corners kept as coordinates (kernels that address an LDS window of the source map).
struct __attribute__((aligned(16))) TapXY {
  int xa, xb, ya, yb;   // clamped in range
  float wt[4];
};
__device__ __forceinline__ void make_taps(float ix, float iy, const Geom& g, int, TapXY& t) {
  tap_weights_corners(ix, iy, g, t.wt, t.xa, t.xb, t.ya, t.yb);
}

// ---- the four-tap gather and blend of a lane's 4 channels: one blend, two address front-ends.
// ATen tap order: nw*w + ne*w + sw*w + se*w, each step one fma
__device__ __forceinline__ void blend_taps(const float4& nw, const float4& ne, const float4& sw, const float4& se, const float* wt,
                                           float* val) {
  val[0] = __fmaf_rn(se.x, wt[3], __fmaf_rn(sw.x, wt[2], __fmaf_rn(ne.x, wt[1], __fmul_rn(nw.x, wt[0]))));
  val[1] = __fmaf_rn(se.y, wt[3], __fmaf_rn(sw.y, wt[2], __fmaf_rn(ne.y, wt[1], __fmul_rn(nw.y, wt[0]))));
  val[2] = __fmaf_rn(se.z, wt[3], __fmaf_rn(sw.z, wt[2], __fmaf_rn(ne.z, wt[1], __fmul_rn(nw.z, wt[0]))));
  val[3] = __fmaf_rn(se.w, wt[3], __fmaf_rn(sw.w, wt[2], __fmaf_rn(ne.w, wt[1], __fmul_rn(nw.w, wt[0]))));
}
// `sb` = a view's map of this batch element, `lane_b` = byte offset of the lane's 4 channels inside a texel.
// uniform base (SGPR pair) + 32-bit byte offset per lane: `global_load_dwordx4 v, v_off, s[base]`.  With per-lane 64-bit
// pointers the four gathers cost 13 VALU instructions of address arithmetic per (plane, view) -- a fifth of the sample loop,
// which is VALU-bound (r03, ISA of warp_kernel<32,kVec>)
__device__ __forceinline__ void gather_blend_at(const char* sb, unsigned b0, unsigned b1, unsigned b2, unsigned b3, const float* wt,
                                                float* val) {
  const float4 nw = *reinterpret_cast<const float4*>(sb + b0);
  const float4 ne = *reinterpret_cast<const float4*>(sb + b1);
  const float4 sw = *reinterpret_cast<const float4*>(sb + b2);
  const float4 se = *reinterpret_cast<const float4*>(sb + b3);
  blend_taps(nw, ne, sw, se, wt, val);
}
// TapEntry: float offsets, byte stride 4
__device__ __forceinline__ void gather_blend(const char* sb, const TapEntry& t, unsigned lane_b, float* val) {
  gather_blend_at(sb, (unsigned)t.off[0] * 4u + lane_b, (unsigned)t.off[1] * 4u + lane_b, (unsigned)t.off[2] * 4u + lane_b,
                  (unsigned)t.off[3] * 4u + lane_b, t.wt, val);
}
// TapXY: corners of a [h,W,C] map, texel stride 4*C bytes
template <int C>
__device__ __forceinline__ void gather_blend(const char* sb, const TapXY& t, int W, unsigned lane_b, float* val) {
  const int o0 = (t.ya * W + t.xa), o1 = (t.ya * W + t.xb), o2 = (t.yb * W + t.xa), o3 = (t.yb * W + t.xb);
  gather_blend_at(sb, (unsigned)o0 * (4u * C) + lane_b, (unsigned)o1 * (4u * C) + lane_b, (unsigned)o2 * (4u * C) + lane_b,
                  (unsigned)o3 * (4u * C) + lane_b, t.wt, val);
}

// ---- phase A: the tap table of a depth chunk.  P = a kernel's parameter struct (proj, hypos, hypos_per_pixel, g, B, D, n_src).
// The struct and tile references of these helpers are __restrict__: a helper is optimised on its own before it is inlined, and
// without it the parameter loads are not hoisted over the table stores there (warp_pairdiff_kernel<*,4,false>: 96 -> 98 VGPRs,
// 5 -> 4 waves per SIMD).
//
// Depth hypothesis of plane d at a pixel: [B,D] or [B,D,h,w].  One load through a selected ADDRESS, which is what the compiler made
// of the ternary of two loads while it stood inside the kernels.  In a helper the other two spellings cost a wave per SIMD: the
// ternary of loads (warp_train_kernel 92 -> 98 VGPRs, warp_pairdiff_kernel<*,4,false> 96 -> 98: 5 -> 4 waves) and a selected index
// (warp_kernel<32,kVec> 96 -> 98: 5 -> 4 waves).  The address not taken is only computed, never read.
template <class P>
__device__ __forceinline__ float hypo_depth(const P& __restrict__ p, int b, int d, int hw, int pix) {
  const size_t i = (size_t)b * p.D + d;
  const float* u = p.hypos + i;
  const float* q = p.hypos + (i * hw + pix);
  return *(p.hypos_per_pixel ? q : u);
}

// Generic form: entry e of the table is (plane e / (PPB*nv), view v_lo + (e / PPB) % nv, pixel e % PPB) of the planes [d0, d0 + nd),
// one whole sample position per thread and step.  Entry = TapEntry (offsets into maps of `texel` floats per texel) or TapXY;
// Tile maps a tile slot to its pixel (PixTile); seen(view, live, entry) is called for every entry (bounding boxes).
template <int PPB, class Entry, class Tile, class P, class Seen>
__device__ __forceinline__ void fill_taps(Entry* tab, const Tile& __restrict__ pt, const P& __restrict__ p, int b, int d0, int nd, int v_lo, int nv, int texel,
                                          Seen seen) {
  const int hw = p.g.h * p.g.w;
  const int nent = nd * nv * PPB;
  for (int e = threadIdx.x; e < nent; e += kThreads) {
    const int epl = e % PPB;
    const int ev = v_lo + (e / PPB) % nv;
    const int ed = e / (PPB * nv);
    int xx, yy;
    bool elive;
    const int epix = pt.pix(epl, p.g.w, p.g.h, xx, yy, elive);
    float ix, iy;
    warp_position(p.proj + ((size_t)ev * p.B + b) * 12, (float)xx, (float)yy, hypo_depth(p, b, d0 + ed, hw, epix), p.g, ix, iy);
    Entry t;
    make_taps(ix, iy, p.g, texel, t);
    tab[e] = t;
    seen(ev, elive, t);
  }
}
template <int PPB, class Entry, class Tile, class P>
__device__ __forceinline__ void fill_taps(Entry* tab, const Tile& __restrict__ pt, const P& __restrict__ p, int b, int d0, int nd, int texel) {
  fill_taps<PPB>(tab, pt, p, b, d0, nd, 0, p.n_src, texel, [](int, bool, const Entry&) {});
}

// Fixed-pair form: when the (pixel, view) pairs of the tile divide the block (5 views: 4 x PPB = 256 / 128 / 64) or are exactly
// NP = 2 per thread, a thread keeps ITS pair(s) over all planes and chunks, so the pair's index arithmetic, its three 16-byte
// loads of the projection and rot_xyz are done once per kernel instead of once per sample (they were a third of the per-sample
// instructions; the kernel is VALU-bound).  With more threads than pairs the thread groups take the planes of a chunk in turn.
template <int NP, int PPB>
struct FixedPairs {
  PixelRay ray[NP];
  int pl[NP], v[NP], pix[NP];
  int grp, ngrp;
  bool few, two;     // >= 1 thread group per pair set; exactly two pairs per thread
  static bool usable(int n_src) {
    const int npair = PPB * n_src;
    return (kThreads % npair) == 0 || (NP == 2 && npair == 2 * kThreads);
  }
  // `enable` = false (a kernel instantiated without the fixed form): nothing is computed and active() is false
  template <class Tile, class P>
  __device__ __forceinline__ FixedPairs(const Tile& __restrict__ pt, const P& __restrict__ p, int b, bool enable = true)
      : ray{}, pl{}, v{}, pix{}, grp(0), ngrp(1), few(false), two(false) {
    if (!enable) return;
    const int tid = threadIdx.x;
    const int npair = PPB * p.n_src;
    few = (kThreads % npair) == 0;
    two = (NP == 2) && (npair == 2 * kThreads);
    if (!(few || two)) return;       // the pair's projection loads and rot_xyz only where they are used
    ngrp = few ? kThreads / npair : 1; grp = few ? tid / npair : 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int pair = (few ? tid % npair : tid) + k * kThreads;
      pl[k] = pair % PPB; v[k] = min(pair / PPB, p.n_src - 1);
      int xx, yy;
      bool live;
      pix[k] = pt.pix(pl[k], p.g.w, p.g.h, xx, yy, live);
      ray[k] = warp_ray(p.proj + ((size_t)v[k] * p.B + b) * 12, (float)xx, (float)yy);
    }
  }
  __device__ __forceinline__ bool active() const { return few || two; }
  template <class P>
  __device__ __forceinline__ void fill(TapEntry* tab, const P& __restrict__ p, int b, int d0, int nd, int texel) const {
    const int hw = p.g.h * p.g.w;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      if (k == 1 && !two) break;
      for (int ed = grp; ed < nd; ed += ngrp) {
        float ix, iy;
        warp_position_ray(ray[k], hypo_depth(p, b, d0 + ed, hw, pix[k]), p.g, ix, iy);
        TapEntry t;
        make_taps(ix, iy, p.g, texel, t);
        tab[(ed * p.n_src + v[k]) * PPB + pl[k]] = t;
      }
    }
  }
};

// Reductions over the LPP (4/8/16) lanes of one pixel with DPP row operations (full-rate VALU, no LDS-pipe
// permutes): xor-1 and xor-2 inside the quad, then row_half_mirror / row_mirror -- valid because after the quad steps
// all 4 lanes of a quad already hold the same partial result.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int LPP>
__device__ __forceinline__ float pixel_sum(float v) {
  v += dpp_mov<0xB1>(v);                  // quad_perm [1,0,3,2]
  if (LPP >= 4) v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  if (LPP >= 8) v += dpp_mov<0x141>(v);   // row_half_mirror
  if (LPP >= 16) v += dpp_mov<0x140>(v);  // row_mirror
  return v;
}
template <int LPP>
__device__ __forceinline__ float pixel_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  if (LPP >= 8) v = fmaxf(v, dpp_mov<0x141>(v));
  if (LPP >= 16) v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}

constexpr float kLog2e = 1.4426950408889634f;

// softmax over a pair (C/G = 2): p0 = e^a/(e^a+e^b) = 1/(1 + e^(b-a)), p1 = 1 - p0.  One v_exp + one v_rcp, no selects;
// b-a -> +inf gives p0 = 0, NaN propagates.  (|error| ~1e-7 vs ATen's exp(x-max)/sum; tolerance of the cost is 2e-6.)
__device__ __forceinline__ float softmax2_p0(float a, float b) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((b - a) * kLog2e));
}
__device__ __forceinline__ void softmax2(float a, float b, float& p0, float& p1) {
  p0 = softmax2_p0(a, b);
  p1 = 1.0f - p0;
}

// softmax over all C channels of a pixel (C/4 lanes of 4 channels), homoaggregate.py:60.  The eval kernel and the variance backward
// share it: the training gradient is that of the eval forward only while both are this arithmetic.
template <int LPP>
__device__ __forceinline__ void softmax_pixel(const float* val, float* pr) {
  const float mx = pixel_max<LPP>(fmaxf(fmaxf(val[0], val[1]), fmaxf(val[2], val[3])));
  float e[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = expf(val[k] - mx);
  const float den = pixel_sum<LPP>((e[0] + e[1]) + (e[2] + e[3]));
#pragma unroll
  for (int k = 0; k < 4; ++k) pr[k] = e[k] / den;
}

// ---- host side: the argument checks of the entry points
// max_b: the entry points that refuse a batch beyond one launch's gridDim.y say so between the two checks
int check_shape(int B, int D, int h, int w, int texel, int max_b = 0) {
  MDF_REQUIRE(B > 0 && D > 0 && h > 1 && w > 1, "bad shape B=%d D=%d h=%d w=%d", B, D, h, w);
  if (max_b) MDF_REQUIRE(B < max_b, "B=%d too large for one launch", B);
  MDF_REQUIRE((long long)h * w * texel < (1ll << 30), "feature map too large for 32-bit byte offsets");
  return MDF_OK;
}
int check_channels(int C) {
  if (C != 16 && C != 32 && C != 64)
    return mdf::fail(MDF_EUNSUPPORTED, "C=%d not supported (built for 16, 32, 64)", C);
  return MDF_OK;
}
int check_n_src(int n_src) {
  MDF_REQUIRE(n_src >= 1 && n_src <= MDF_MAX_SRC_VIEWS, "n_src=%d out of range [1,%d]", n_src, MDF_MAX_SRC_VIEWS);
  return MDF_OK;
}
// the per-view pointers of an argument array into a parameter struct; `name` = the argument's name
template <class T>
int copy_views(T** dst, T* const* src, int n_src, const char* name) {
  for (int v = 0; v < n_src; ++v) {
    MDF_REQUIRE(src[v], "%s[%d] is null", name, v);
    dst[v] = src[v];
  }
  return MDF_OK;
}

Geom make_geom(int h, int w) {
  Geom g;
  g.w = w;
  g.h = h;
  g.half_w = (float)((double)(w - 1) / 2.0);
  g.half_h = (float)((double)(h - 1) / 2.0);
  g.sw = (float)((double)w / 2.0);
  g.sh = (float)((double)h / 2.0);
  return g;
}

}  // namespace
