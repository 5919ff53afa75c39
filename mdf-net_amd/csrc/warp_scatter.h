// The scatter side of the backward warp kernels (warp_bwd_kernel in warp_aggregate_train.hip, warp_var_bwd_kernel in
// warp_variance_train.hip), each piece defined once: the tile of a block, the tap table with the bounding box of every view's
// live taps, the LDS window the taps are accumulated in and its dense flush, and the depth slicing of the launchers.
//
// The gradient of a bilinear gather is a scatter through the same four taps.  Per (depth chunk, view) the block finds the
// bounding box of its live taps in the source map; when the box fits the LDS window the taps are accumulated there and the
// window is flushed once with DENSE global atomics (whole rows of the window are contiguous in the NHWC gradient map) -- each
// texel is sent to memory once per chunk instead of once per tap; a block whose footprint does not fit (strong rotation, very
// wide depth range) scatters to memory directly.  What differs per kernel: the floats per window texel, how a pending tap sum
// is added to the window, and the walk over the table.
//
// LIVENESS.  Whether a tap is scattered is decided from its WEIGHT (non-zero for some pending plane; NaN weights of z == 0
// planes count as live), never from the pending value: an out-of-bounds tap has weight 0 and lies outside the bounding box
// (built below from the same weight test), but 0 * (non-finite gradient) = NaN would pass a value test and index the window
// out of range.  grid_sample's backward likewise adds nothing for out-of-bounds taps and propagates NaN through the in-bounds
// ones.  Both kernels keep a mask of live taps next to their pending sums for this.
#pragma once
#include "warp_common.h"

namespace {

#ifndef MDF_BWD_WIN_FLOATS
#define MDF_BWD_WIN_FLOATS 4096
#endif
constexpr int kWinFloats = MDF_BWD_WIN_FLOATS;   // 16 KiB: with the tap table (16-32 KiB) four blocks per CU

// Pixels of a scatter tile: 16 x 4 (C = 16), 8 x 4 (C = 32), 4 x 4 (C = 64), not a run of a row: the bounding box of its taps in a
// source map is (TW+1) x (TH+1) texels plus the depth sweep instead of a slanted (PPB+1)-texel line's box -- half the window
// texels to zero and flush, and a window that fits.
template <int C>
using BwdTile = PixTile<kThreads / (C / 4), 4>;

int bwd_tile_blocks(int C, int w, int h) {      // gridDim.x of a scatter launch
  return (C == 64) ? BwdTile<64>::blocks(w, h) : (C == 32) ? BwdTile<32>::blocks(w, h) : BwdTile<16>::blocks(w, h);
}

// LDS float add through an address-space-3 pointer: `ds_add_f32` (with a generic pointer next to the global fallback the
// compiler merges both branches into one `flat_atomic_add_f32` on a selected 64-bit address).
__device__ __forceinline__ void lds_add(float* p, float v) {
  (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) float*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The tap table of the planes [d0, d0 + nd) and views [v_lo, v_lo + nv) (fill_taps), and bb[v] = xmin, xmax, ymin, ymax of view
// v's live taps (see LIVENESS).  Ends with the table and the boxes visible to the block.
template <int PPB, class Tile, class P>
__device__ __forceinline__ void fill_taps_bbox(TapXY* tab, int (*bb)[4], const Tile& __restrict__ pt, const P& __restrict__ p, int b,
                                               int d0, int nd, int v_lo, int nv) {
  const int tid = threadIdx.x;
  if (tid < 4 * p.n_src) bb[tid >> 2][tid & 3] = (tid & 1) ? INT32_MIN : INT32_MAX;
  __syncthreads();
  fill_taps<PPB>(tab, pt, p, b, d0, nd, v_lo, nv, 0, [&](int ev, bool elive, const TapXY& t) {
    if (elive) {
      const bool a = (t.wt[0] != 0.0f) || (t.wt[2] != 0.0f), bq = (t.wt[1] != 0.0f) || (t.wt[3] != 0.0f);   // column xa / xb live
      const bool cq = (t.wt[0] != 0.0f) || (t.wt[1] != 0.0f), dq = (t.wt[2] != 0.0f) || (t.wt[3] != 0.0f);  // row ya / yb live
      if (a || bq) {
        atomicMin(&bb[ev][0], a ? t.xa : t.xb);
        atomicMax(&bb[ev][1], bq ? t.xb : t.xa);
        atomicMin(&bb[ev][2], cq ? t.ya : t.yb);
        atomicMax(&bb[ev][3], dq ? t.yb : t.ya);
      }
    }
  });
  __syncthreads();
}

// The LDS window over one view's bounding box, T floats per texel.  `use` is block-uniform.
template <int T>
struct ScatterWin {
  int xmin, ymin, ww, wh;
  bool use;
  __device__ __forceinline__ explicit ScatterWin(const int* bbv) {
    const int xmax = bbv[1], ymax = bbv[3];
    xmin = bbv[0]; ymin = bbv[2];
    ww = xmax - xmin + 1; wh = ymax - ymin + 1;
    const bool any = (xmax >= xmin) && (ymax >= ymin);
    use = any && ((long long)ww * wh * T <= kWinFloats);
  }
  __device__ __forceinline__ int texel(int tx, int ty) const { return (ty - ymin) * ww + (tx - xmin); }
  __device__ __forceinline__ void zero(float* win) const {
    for (int i = threadIdx.x; i < ww * wh * T; i += kThreads) win[i] = 0.0f;
  }
  // gmap = the [h,W,T] gradient map of this batch element: ww*T contiguous floats per window row
  __device__ __forceinline__ void flush(const float* win, float* gmap, int W) const {
    for (int wy = 0; wy < wh; ++wy) {
      float* grow = gmap + ((size_t)(ymin + wy) * W + xmin) * T;
      const float* wrow = win + wy * ww * T;
      for (int j = threadIdx.x; j < ww * T; j += kThreads) {
        const float val = wrow[j];
        if (val != 0.0f) unsafeAtomicAdd(grow + j, val);     // (NaN != 0: non-finite sums are sent on)
      }
    }
  }
};

// A block walks its pixels over the planes one (plane, view) at a time, each step a dependent gather: with the few blocks of a
// cfg3-sized map (432 at 72x96x64ch) the chip holds < 2 waves per SIMD and the kernel is latency-bound.  Cut the depth range
// into slices (gridDim.z) until there are about `target` blocks; per-pixel results that span the planes (d ref) meet through
// atomics.  Sets p.dslice, clamps the chunk `dch` to a slice, returns gridDim.z.
template <class P>
int depth_slices(P& p, int& dch, int target) {
  const long long blocks = (long long)p.nblk_x * p.B;
  int nz = (int)((target + blocks - 1) / blocks);
  if (nz > p.D / 4) nz = p.D / 4;          // >= 4 planes per slice: a slice re-reads the reference features and the tap setup
  if (nz < 1) nz = 1;
  p.dslice = (p.D + nz - 1) / nz;
  nz = (p.D + p.dslice - 1) / p.dslice;
  if (dch > p.dslice) dch = p.dslice;
  return nz;
}
// equal chunks inside a slice
int equal_chunks(int dslice, int dch) {
  const int nch = (dslice + dch - 1) / dch;
  return (dslice + nch - 1) / nch;
}

}  // namespace
