// Backward of homo_aggregate_by_variance fused with the plane-sweep warp (net/unit/homoaggregate.py:49-69 over
// net/unit/base.py:85-126, whose sampling grid is built under no_grad, base.py:97 -- gradient flows to the features only),
// and of the stand-alone homo_warping: one kernel template, the soft-max stage compiled out for the plain warp.
//
// The operator has no parameters and no BatchNorm, so training is one forward and one backward pass.  The training FORWARD is
// the eval kernel (mdf_warp_aggregate_var_fwd with an NDHWC cost volume): bit-identical to eval by construction.
//
//   x_0 = ref (raw), x_v = softmax_C(warp(src_v)), N = n_src + 1, m = (sum_v x_v)/N, cost = (sum_v x_v^2)/N - m^2
//   g = d cost:   d ref = sum_d (2/N) g (ref - m)                                   (direct store / depth slices meet through atomics)
//                 gp = (2/N) g (x_v - m),  gv = x_v (gp - sum_c x_v gp),  d src_v[tap_k] += wt_k gv      (scatter: transpose of the gather)
//
// m is RECOMPUTED per voxel from the features (a stored sum volume would be as large as the cost volume): per chunk of at most
// kPlanes depth planes a lane first gathers every view and keeps m and (2/N) g of its 4 channels in registers, then walks the
// views again, one at a time, and scatters.  Thread mapping of the eval kernel (a lane owns 4 channels, the C/4 lanes of a pixel
// are neighbours and reduce with DPP row operations); the scatter -- tile shape, tap table with bounding boxes, LDS window, dense
// flush and direct-to-memory fallback -- is warp_scatter.h's, shared with warp_bwd_kernel.  Every channel carries a gradient of
// its own here, so a window texel is C floats and all window updates are LDS float atomics (no claim bytes: the four waves of a
// block hold DIFFERENT pixels of the tile).  The window (kWinFloats, 16 KiB) lies next to a tap table of at most 32 KiB.
//
// Compile with -ffp-contract=off like the other warp kernels: the sample positions are those of warp_position.
#include <cstdlib>
#include "warp_scatter.h"

namespace {

constexpr int kPlanes = 4;                           // depth planes per chunk whose m and g stay in registers (32 VGPRs)

struct VarBwdParams {
  const float* ref;                      // [B,h,w,C]   (variance only)
  const float* src[MDF_MAX_SRC_VIEWS];   // [B,h,w,C]   (variance only)
  const float* proj;                     // [n_src,B,12]
  const float* hypos;                    // [B,D] or [B,D,h,w]
  const float* dout;                     // upstream gradient: [B,D,h,w,C] or [B,C,D,h,w]
  float* dref;                           // [B,h,w,C], zero-initialised (depth slices add)
  float* dsrc[MDF_MAX_SRC_VIEWS];        // [B,h,w,C], zero-initialised
  Geom g;
  int B, D, n_src, hypos_per_pixel, dout_ndhwc, dchunk, dslice, nblk_x;
};

// VAR = true: variance aggregation (ref + n_src views).  VAR = false: homo_warping of one view, gv = g.
template <int C, bool VAR>
__global__ __launch_bounds__(kThreads) void warp_var_bwd_kernel(const VarBwdParams p) {
  constexpr int LPP = C / 4;            // lanes per pixel (neighbours inside one DPP row)
  constexpr int PPB = kThreads / LPP;   // pixels per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TapXY* tab = reinterpret_cast<TapXY*>(smem);
  float* win = reinterpret_cast<float*>(smem + (size_t)p.dchunk * p.n_src * PPB * sizeof(TapXY));
  __shared__ int bb[MDF_MAX_SRC_VIEWS][4];   // xmin, xmax, ymin, ymax of the live taps of one view in this chunk

  const int hw = p.g.h * p.g.w;
  const int W = p.g.w;
  const int b = blockIdx.y;
  const BwdTile<C> pt((int)mdf::xcd_remap(blockIdx.x, p.nblk_x), W);
  const int tid = threadIdx.x;
  const int pl = tid / LPP, sub = tid % LPP;
  bool live;
  const int pix = pt.pix(pl, W, p.g.h, live);

  float r[4] = {0.f, 0.f, 0.f, 0.f};
  if (VAR) {
    const float4 rv = *reinterpret_cast<const float4*>(p.ref + ((size_t)b * hw + pix) * C + 4 * sub);
    r[0] = rv.x; r[1] = rv.y; r[2] = rv.z; r[3] = rv.w;
  }
  const float nviews = (float)(p.n_src + 1);
  const float gscale = VAR ? 2.0f / nviews : 1.0f;
  const size_t map_stride = (size_t)hw * C;
  const unsigned lane_b = 16u * (unsigned)sub;      // byte offset of this lane's 4 channels inside a texel
  float gref[4] = {0.f, 0.f, 0.f, 0.f};

  const int dlo = blockIdx.z * p.dslice, dhi = min(p.D, dlo + p.dslice);
  for (int d0 = dlo; d0 < dhi; d0 += p.dchunk) {
    const int nd = min(p.dchunk, dhi - d0);      // <= kPlanes
    // ---------------- tap table of the chunk, all views, and the bounding box of every view's live taps
    fill_taps_bbox<PPB>(tab, bb, pt, p, b, d0, nd, 0, p.n_src);

    // ---------------- phase 1: (2/N) g and the mean over the views of every plane of the chunk, in registers
    float g2[kPlanes][4], mean[kPlanes][4];
#pragma unroll
    for (int dd = 0; dd < kPlanes; ++dd) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { g2[dd][k] = 0.f; mean[dd][k] = 0.f; }
      if (dd < nd) {
        const int d = d0 + dd;
        if (p.dout_ndhwc) {
          const float4 gv = *reinterpret_cast<const float4*>(p.dout + (((size_t)b * p.D + d) * hw + pix) * C + 4 * sub);
          g2[dd][0] = gscale * gv.x; g2[dd][1] = gscale * gv.y; g2[dd][2] = gscale * gv.z; g2[dd][3] = gscale * gv.w;
        } else {
          const size_t cs = (size_t)p.D * hw;
          const float* gp = p.dout + ((size_t)b * C * p.D + d) * hw + pix;
#pragma unroll
          for (int k = 0; k < 4; ++k) g2[dd][k] = gscale * gp[(size_t)(4 * sub + k) * cs];
        }
        if (VAR) {
          float acc[4] = {r[0], r[1], r[2], r[3]};
          for (int v = 0; v < p.n_src; ++v) {
            const TapXY t = tab[(dd * p.n_src + v) * PPB + pl];
            const char* sb = reinterpret_cast<const char*>(p.src[v] + (size_t)b * map_stride);
            float val[4], pr[4];
            gather_blend<C>(sb, t, W, lane_b, val);
            softmax_pixel<LPP>(val, pr);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += pr[k];
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            mean[dd][k] = acc[k] / nviews;
            gref[k] = fmaf(g2[dd][k], r[k] - mean[dd][k], gref[k]);
          }
        }
      }
    }

    // ---------------- phase 2: one view at a time, the scatter through its window
    for (int v = 0; v < p.n_src; ++v) {
      const ScatterWin<C> w(bb[v]);
      if (w.use) {
        w.zero(win);
        __syncthreads();
      }
      const char* sb = VAR ? reinterpret_cast<const char*>(p.src[v] + (size_t)b * map_stride) : nullptr;
      float* gout = p.dsrc[v] + (size_t)b * map_stride + 4 * sub;
      float pend[4][4];                       // [tap][channel]: pending tap sums of the current corner set
#pragma unroll
      for (int k = 0; k < 4; ++k) { pend[k][0] = 0.f; pend[k][1] = 0.f; pend[k][2] = 0.f; pend[k][3] = 0.f; }
      int cxa = -1, cxb = -1, cya = -1, cyb = -1;
      unsigned lm = 0;    // live taps of the pending sums (warp_scatter.h, LIVENESS)
      auto flush_taps = [&](int xa, int xb, int ya, int yb) {
        const unsigned m = lm;
        lm = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (m & (1u << k)) {
            const int tx = (k & 1) ? xb : xa, ty = (k & 2) ? yb : ya;
            if (w.use) {
              float* o = win + w.texel(tx, ty) * C + 4 * sub;
              lds_add(o, pend[k][0]); lds_add(o + 1, pend[k][1]); lds_add(o + 2, pend[k][2]); lds_add(o + 3, pend[k][3]);
            } else {
              float* o = gout + (size_t)(ty * W + tx) * C;
              unsafeAtomicAdd(o, pend[k][0]); unsafeAtomicAdd(o + 1, pend[k][1]);
              unsafeAtomicAdd(o + 2, pend[k][2]); unsafeAtomicAdd(o + 3, pend[k][3]);
            }
          }
          pend[k][0] = 0.f; pend[k][1] = 0.f; pend[k][2] = 0.f; pend[k][3] = 0.f;
        }
      };
#pragma unroll
      for (int dd = 0; dd < kPlanes; ++dd) {
        if (dd < nd) {
          const TapXY t = tab[(dd * p.n_src + v) * PPB + pl];
          float gv[4];
          if (VAR) {
            float val[4], x[4], gp[4];
            gather_blend<C>(sb, t, W, lane_b, val);
            softmax_pixel<LPP>(val, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) gp[k] = g2[dd][k] * (x[k] - mean[dd][k]);
            const float s = pixel_sum<LPP>((x[0] * gp[0] + x[1] * gp[1]) + (x[2] * gp[2] + x[3] * gp[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k) gv[k] = x[k] * (gp[k] - s);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) gv[k] = g2[dd][k];
          }
          if (live) {
            // neighbouring planes of a pixel mostly hit the same four texels: keep the tap sums in registers while the corners stay
            if (t.xa != cxa || t.ya != cya || t.xb != cxb || t.yb != cyb) {
              flush_taps(cxa, cxb, cya, cyb);
              cxa = t.xa; cxb = t.xb; cya = t.ya; cyb = t.yb;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
              for (int c = 0; c < 4; ++c) pend[k][c] = fmaf(t.wt[k], gv[c], pend[k][c]);
              lm |= (t.wt[k] != 0.0f) ? (1u << k) : 0u;      // NaN weights (z == 0 planes) count as live, as in `bb`
            }
          }
        }
      }
      flush_taps(cxa, cxb, cya, cyb);
      if (w.use) {
        __syncthreads();
        w.flush(win, p.dsrc[v] + (size_t)b * map_stride, W);
        __syncthreads();
      }
    }
    __syncthreads();   // the next chunk overwrites tab and bb
  }

  if (VAR && live) {
    float* o = p.dref + ((size_t)b * hw + pix) * C + 4 * sub;
    if (gridDim.z == 1) {
      *reinterpret_cast<float4*>(o) = make_float4(gref[0], gref[1], gref[2], gref[3]);
    } else {       // the depth slices of a pixel meet here
      unsafeAtomicAdd(o, gref[0]); unsafeAtomicAdd(o + 1, gref[1]); unsafeAtomicAdd(o + 2, gref[2]); unsafeAtomicAdd(o + 3, gref[3]);
    }
  }
}

template <bool VAR>
int launch_var_bwd(VarBwdParams& p, int C, hipStream_t st) {
  const int lpp = C / 4, ppb = kThreads / lpp;
  p.nblk_x = bwd_tile_blocks(C, p.g.w, p.g.h);
  static const int tab_env = mdf::env_pos("MDF_VAR_BWD_TAB", 1024);   // dev A/B
  int dch = tab_env / (p.n_src * ppb);        // tap-table entries (32 B each) per block
  if (dch > kPlanes) dch = kPlanes;
  if (dch < 1) dch = 1;
  // depth slices (gridDim.z): the small maps of the first stage give a few hundred blocks only.  The chunks of a slice are not
  // equalised here (equal_chunks): they are at most kPlanes planes anyway
  static const int target_env = mdf::env_pos("MDF_VAR_BWD_BLOCKS", 1024);   // dev A/B
  const int nz = depth_slices(p, dch, target_env);
  p.dchunk = dch;
  const size_t lds = (size_t)dch * p.n_src * ppb * sizeof(TapXY) + (size_t)kWinFloats * sizeof(float);
  dim3 grid(p.nblk_x, p.B, nz), block(kThreads);
  switch (C) {
    case 64: hipLaunchKernelGGL((warp_var_bwd_kernel<64, VAR>), grid, block, lds, st, p); break;
    case 32: hipLaunchKernelGGL((warp_var_bwd_kernel<32, VAR>), grid, block, lds, st, p); break;
    case 16: hipLaunchKernelGGL((warp_var_bwd_kernel<16, VAR>), grid, block, lds, st, p); break;
    default: return mdf::fail(MDF_EUNSUPPORTED, "warp kernels are built for C in {16,32,64}, got %d", C);
  }
  return mdf::check_launch("warp_var_bwd_kernel");
}

int check_var_bwd(int B, int C, int D, int h, int w) {
  if (int rc = check_shape(B, D, h, w, C, 65536)) return rc;
  return check_channels(C);
}

}  // namespace

extern "C" int mdf_warp_aggregate_var_bwd(const float* ref_fea, const float* const* src_feas, const float* proj, const float* hypos,
                                          int hypos_per_pixel, const float* dcost, float* dref, float* const* dsrc, int B, int C, int D,
                                          int h, int w, int n_src, void* stream) {
  MDF_REQUIRE(ref_fea && src_feas && proj && hypos && dcost && dref && dsrc, "null pointer argument");
  if (int rc = check_var_bwd(B, C, D, h, w)) return rc;
  if (int rc = check_n_src(n_src)) return rc;
  VarBwdParams p{};
  p.ref = ref_fea;
  for (int v = 0; v < n_src; ++v) {     // (one message for both arrays: not copy_views)
    MDF_REQUIRE(src_feas[v] && dsrc[v], "src_feas[%d] or dsrc[%d] is null", v, v);
    p.src[v] = src_feas[v];
    p.dsrc[v] = dsrc[v];
  }
  p.proj = proj; p.hypos = hypos; p.dout = dcost; p.dref = dref;
  p.g = make_geom(h, w);
  p.B = B; p.D = D; p.n_src = n_src; p.hypos_per_pixel = hypos_per_pixel; p.dout_ndhwc = 1;
  return launch_var_bwd<true>(p, C, (hipStream_t)stream);
}

extern "C" int mdf_homo_warp_bwd(const float* dvol, int vol_layout, const float* proj, const float* hypos, int hypos_per_pixel,
                                 float* dsrc, int B, int C, int D, int h, int w, void* stream) {
  MDF_REQUIRE(dvol && proj && hypos && dsrc, "null pointer argument");
  if (int rc = check_var_bwd(B, C, D, h, w)) return rc;
  MDF_REQUIRE(vol_layout == MDF_VOL_NCDHW || vol_layout == MDF_VOL_NDHWC, "vol_layout=%d", vol_layout);
  VarBwdParams p{};
  p.dsrc[0] = dsrc;
  p.proj = proj; p.hypos = hypos; p.dout = dvol;
  p.g = make_geom(h, w);
  p.B = B; p.D = D; p.n_src = 1; p.hypos_per_pixel = hypos_per_pixel; p.dout_ndhwc = (vol_layout == MDF_VOL_NDHWC);
  return launch_var_bwd<false>(p, C, (hipStream_t)stream);
}
