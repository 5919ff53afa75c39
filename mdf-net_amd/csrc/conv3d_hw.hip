// Depth-preserving 3-D sampling layers of RegularNet_4Scales composed with sample_stride (1,2,2) / sample_padding (0,1,1)
// (reference: net/unit/regular.py:76-77): H and W are halved / doubled, every depth plane is kept.
//   down: Conv3d(k3, stride (1,2,2), pad 1)                                 Do = Di, Ho = (Hi-1)/2+1, Wo = (Wi-1)/2+1
//   up:   ConvTranspose3d(k3, stride (1,2,2), pad 1, output_padding (0,1,1)) Do = Di, Ho = 2 Hi,       Wo = 2 Wi
// The implicit GEMM is conv3d_kernel's (conv3d.hip): D[cout][voxel] = W[cout][k] * X[k][voxel] on v_mfma_f32_16x16x4_f32, the same
// lane mapping and fragment order, so the weight sets of mdf_conv3d_pack_weights are consumed as they are -- the plain set
// (transposed = 0: 27 taps) by the down mode, the transposed set (all nine (kd, kh) pairs x two w-offset slots) by the up mode.
//
// down: M walks the output voxels; the base input voxel of output (d, h, w) is (d, 2h, 2w) and tap k reads offset k - 1 on every
//       axis: the stride-2 kernel with a depth stride of 1.
// up:   M walks the INPUT voxels.  Depth is an ordinary stride-1 correlation with the tap flipped (output plane d reads input plane
//       d + 1 - kd, masked at both ends); H and W use the parity scheme of conv3d_kernel<kTr>: parity 0 <- k = 1 on input i, parity 1
//       <- k = 0 on input i + 1 and k = 2 on input i.  One h-parity class per blockIdx.y; both w-parities are GEMM rows [pw][cout] of
//       one wave, so an input voxel stores 2*COUT contiguous floats.  A class has 3 * (1 + ph) * 2 tap slots, none structurally zero
//       (in the slots of w-offset +1 the rows of pw = 0 are: n-tiles made only of them are skipped, as in conv3d_kernel<kTr>).
// Epilogue (fused, conv3d_common.h): y = [res +] [relu]( acc * alpha + beta ).
//
// Eval only: the training kernels (weight gradient with a separate depth stride, epilogue sums) are not built for this stride.
#include <cstdlib>
#include "conv3d_common.h"

namespace {

enum HwMode { kHwDown = 0, kHwUp = 1 };

// Tap validity of the up mode around input voxel (d, h, w): bits 0-2: depth tap kd valid (it reads plane d + 1 - kd); bits 3-5 / 6-8:
// the h / w slots of conv3d_kernel<kTr> (slot 0 <-> offset +1, slots 1, 2 <-> offset 0).
__device__ __forceinline__ unsigned hw_up_mask(int d, int h, int w, int Di, int Hi, int Wi) {
  unsigned vm = tap_mask<true>(d, h, w, Di, Hi, Wi) & ~7u;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (d + 1 - k >= 0 && d + 1 - k < Di) vm |= 1u << k;
  return vm;
}

// SPLITK = 4: the four waves of a block share ONE wave tile and each takes every 4th tap slot; the partial accumulators are summed
// through LDS (as conv3d_kernel).
template <int CIN, int COUT, int MODE, int MT, int SPLITK>
__global__ __launch_bounds__(256) void conv3d_hw_kernel(const ConvParams p) {
  constexpr bool UP = (MODE == kHwUp);
  constexpr int KPL = (CIN >= 16) ? 4 : 2;   // k values per lane per chunk
  constexpr int CK = 4 * KPL;                // cin per chunk
  constexpr int NCH = CIN / CK;
  constexpr int ROWS = UP ? 2 * COUT : COUT;   // up: GEMM rows are [pw][cout]
  constexpr int NT = (ROWS + 15) / 16;
  static_assert(CIN % CK == 0, "CIN must be a multiple of the chunk");

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = lane >> 4;    // k sub-slot / cout quad
  const int n16 = lane & 15;  // voxel inside the m-tile (B operand, C/D column)
  const unsigned tile_blk = mdf::xcd_remap(blockIdx.x, p.nblk);
  const long long m0 = (SPLITK > 1 ? (long long)tile_blk : (long long)tile_blk * 4 + wave) * (MT * 16);
  const int ph = UP ? (int)blockIdx.y : 0;   // up: the h-parity class of this block

  // per-lane voxel bookkeeping for each m-tile
  int in_off[MT];       // float offset of the base input voxel (channel 0)
  long long out_vox[MT];
  unsigned vmask[MT];   // bits 0-2: kd valid, 3-5: kh valid, 6-8: kw valid (up: hw_up_mask)
  bool live[MT];
  // index space dims (output dims for down, input dims for up)
  const int Md = p.Di, Mh = UP ? p.Hi : p.Ho, Mw = UP ? p.Wi : p.Wo;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    long long m = m0 + t * 16 + n16;
    live[t] = m < p.m_total;
    if (!live[t]) m = p.m_total - 1;
    const Voxel v = split_voxel(m, Md, Mh, Mw);
    const int bd = v.d, bh = UP ? v.h : 2 * v.h, bw = UP ? v.w : 2 * v.w;   // base input coordinate
    const unsigned vm = UP ? hw_up_mask(bd, bh, bw, p.Di, p.Hi, p.Wi) : tap_mask(bd, bh, bw, p.Di, p.Hi, p.Wi);
    vmask[t] = live[t] ? vm : 0u;
    in_off[t] = (int)((((long long)v.b * p.Di + bd) * p.Hi + bh) * p.Wi + bw) * CIN;
    if (UP)
      out_vox[t] = (((long long)v.b * p.Do + v.d) * p.Ho + (2 * v.h + ph)) * p.Wo + 2 * v.w;   // pw added in the epilogue
    else
      out_vox[t] = m;
  }

  // Depth taps that NO voxel of this wave's tiles has (volumes 1-3 planes deep: at Di = 1 only kd = 1 exists) are skipped altogether,
  // wave-uniformly (kd_any_of); in both modes kd is the slowest index of the tap order.
  unsigned kd_any = 7u;
  if (p.kd_skip) kd_any = kd_any_of(vmask);

  f32x4 acc[MT][NT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[t][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Epilogue operands are fetched now so that their L2 round trip overlaps the tap loop; the residual only in the up mode (the
  // layers that carry a skip connection), as conv3d_kernel<kTr> does.
  constexpr bool kPrefetchRes = UP;
  float4 ep_al[NT], ep_be[NT], ep_res[kPrefetchRes ? MT : 1][NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r0 = nt * 16 + 4 * q;
    const int c0 = UP ? r0 % COUT : r0;
    fetch_scale_shift(p, r0 < ROWS, c0, ep_al[nt], ep_be[nt]);
    if constexpr (kPrefetchRes) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        ep_res[t][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 < ROWS && p.res && live[t]) {
          const int pw_out = r0 / COUT;
          ep_res[t][nt] = *reinterpret_cast<const float4*>(p.res + (size_t)(out_vox[t] + pw_out) * COUT + c0);
        }
      }
    }
  }

  const float* xq = p.x + KPL * q;                       // this lane's cin slot inside a chunk
  const float* wl = p.wpack + (size_t)lane * KPL;        // this lane's slot inside a packed 64-lane fragment

  // up: tap slot j = (kd * nkh + jh) * 2 + ow with kh = 1 for ph = 0 and kh = 2 jh for ph = 1; along w, offset 0 feeds pw = 0 (kw = 1) and
  // pw = 1 (kw = 2), offset +1 feeds pw = 1 (kw = 0).
  const int nkh = 1 + ph;
  const int ntaps = UP ? 3 * nkh * 2 : 27;
  const int kd_div = UP ? nkh * 2 : 9;                   // slots per depth tap
  struct TapRegs {
    Frag<KPL> bf[NCH][MT], af[NCH][NT];
    int ow;
  };
  auto load_tap = [&](int j, TapRegs& r) {
    int kd, kh, kw, od, oh, ow, tap;
    if (UP) {
      ow = j & 1;
      const int jh = (j >> 1) % nkh;
      kd = (j >> 1) / nkh;
      kh = ph ? 2 * jh : 1;
      od = 1 - kd; oh = (kh == 0);
      kw = ow ? 0 : 1;                  // validity-mask slot of the w offset: bit 0 <-> offset +1, bit 1 <-> offset 0
      tap = (kd * 3 + kh) * 2 + ow;     // slot in the packed transposed set
    } else {
      tap = j;
      kd = tap / 9; kh = (tap / 3) % 3; kw = tap % 3;
      od = kd - 1; oh = kh - 1; ow = kw - 1;
    }
    r.ow = ow;
    const int tapoff = ((od * p.Hi + oh) * p.Wi + ow) * CIN;
    const unsigned need = (1u << kd) | (8u << kh) | (64u << kw);
    const float* wt = wl + (size_t)tap * (NCH * NT * 64 * KPL);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        // branch-free, as conv3d_kernel: an out-of-range tap reads the voxel's own (valid) position and is zeroed by a multiply
        const bool ok = (vmask[t] & need) == need;
        r.bf[ch][t].load(xq + in_off[t] + (ok ? tapoff : 0) + ch * CK);
        r.bf[ch][t].scale(ok ? 1.0f : 0.0f);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) r.af[ch][nt].load(wt + (size_t)(ch * NT + nt) * (64 * KPL));
    }
  };
  auto mul_tap = [&](const TapRegs& r) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int s = 0; s < KPL; ++s)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            // up, offset +1: rows of parity pw = 0 are structurally zero -> skip n-tiles made only of such rows
            if (UP && r.ow == 1 && (nt + 1) * 16 <= COUT) continue;
            acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(r.af[ch][nt].v[s], r.bf[ch][t].v[s], acc[t][nt], 0, 0, 0);
          }
  };
  // The next tap slot of this wave behind j (split-K: every SPLITK-th) whose depth tap some voxel of the wave has.
  constexpr int js = (SPLITK > 1) ? SPLITK : 1;
  auto next_tap = [&](int j) {
    j += js;
    while (j < ntaps && !((kd_any >> (j / kd_div)) & 1u)) j += js;
    return j;
  };
  // Software pipeline over the taps for the one-tile up kernels (the operands of the next slot are requested before the MFMAs of the
  // current one), one tap in flight for the others: the choice conv3d_kernel measured for its transposed / stride-2 layers, carried
  // over and NOT measured for this stride.
  constexpr bool kPipeTaps = (UP && MT == 1);
  {
    int j = next_tap((SPLITK > 1 ? wave : 0) - js);
    if constexpr (kPipeTaps) {
      TapRegs ra, rb;
      if (j < ntaps) load_tap(j, ra);
      while (j < ntaps) {
        int jn = next_tap(j);
        if (jn < ntaps) load_tap(jn, rb);
        __builtin_amdgcn_sched_barrier(0);       // (the requests stay ahead of the MFMAs)
        mul_tap(ra);
        j = jn;
        if (j >= ntaps) break;
        jn = next_tap(j);
        if (jn < ntaps) load_tap(jn, ra);
        __builtin_amdgcn_sched_barrier(0);
        mul_tap(rb);
        j = jn;
      }
    } else {
      if (kd_any == 7u) {                 // (the common case keeps its own loop, as in conv3d_kernel)
        for (; j < ntaps; j += js) {
          TapRegs r;
          load_tap(j, r);
          mul_tap(r);
        }
      } else {
        for (; j < ntaps; j = next_tap(j)) {
          TapRegs r;
          load_tap(j, r);
          mul_tap(r);
        }
      }
    }
  }

  if (SPLITK > 1) {
    // partial sums -> LDS [wave][t*NT+nt][lane]; pair p is finished (summed + epilogue) by wave p % 4
    __shared__ f32x4 part[4][MT * NT][64];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) part[wave][t * NT + nt][lane] = acc[t][nt];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (((t * NT + nt) & 3) == wave) {
          const f32x4 a0 = part[0][t * NT + nt][lane], a1 = part[1][t * NT + nt][lane];
          const f32x4 a2 = part[2][t * NT + nt][lane], a3 = part[3][t * NT + nt][lane];
          acc[t][nt] = (a0 + a1) + (a2 + a3);
        }
      }
  }

  // epilogue: lane owns GEMM rows nt*16 + 4q .. +3 of voxel out_vox[t]
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r0 = nt * 16 + 4 * q;
    if (r0 >= ROWS) continue;
    const int pw_out = UP ? r0 / COUT : 0;
    const int c0 = UP ? r0 % COUT : r0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (!live[t]) continue;
      if (SPLITK > 1 && ((t * NT + nt) & 3) != wave) continue;  // another wave finishes this pair
      float4 o = scale_shift_relu(acc[t][nt], ep_al[nt], ep_be[nt], p.relu);
      const size_t oi = (size_t)(out_vox[t] + pw_out) * COUT + c0;
      add_res_store<kPrefetchRes>(p, oi, o, ep_res[kPrefetchRes ? t : 0][nt]);
    }
  }
}

template <int CIN, int COUT, int MODE, int MT, int SPLITK>
int launch_hw(ConvParams& p, hipStream_t st) {
  const long long per_blk = (SPLITK > 1 ? 1LL : 4LL) * MT * 16;
  p.nblk = (unsigned)((p.m_total + per_blk - 1) / per_blk);
  dim3 grid(p.nblk, MODE == kHwUp ? 2 : 1), block(256);
  hipLaunchKernelGGL((conv3d_hw_kernel<CIN, COUT, MODE, MT, SPLITK>), grid, block, 0, st, p);
  return mdf::check_launch("conv3d_hw_kernel");
}

// The wave tile and split-K by volume, in the spirit of conv3d.hip's launch_conv_mt.  What is measured is the twelve cfg2 launches of
// the stage-1 / stage-2 regularisers (scripts/bench_regular_stride.py --routes, profiles/regular_stride_122.md); every other volume is
// covered by thresholds that are NOT measured there, as the comments beside them say.
//   MDF_CONV3D_HW_ROUTE (dev A/B and the route-equality test, read per call): 0 = the rule, 1 = one tile per wave, 2 = the largest
//   wave tile, 3 = split-K where it is built (elsewhere one tile per wave).
template <int CIN, int COUT, int MODE>
int launch_hw_mt(ConvParams& p, hipStream_t st) {
  constexpr int ROWS = (MODE == kHwUp) ? 2 * COUT : COUT;
  constexpr int MTMAX = (ROWS > 32) ? 2 : 4;
  // split-K is built for the innermost pair of layers, the ones with the fewest voxels and the deepest K: down 32 -> 64
  // (K = 27 * 32 = 864) and up 64 -> 32 (6 / 12 tap slots of 64 channels per class)
  constexpr bool kSplitBuilt = (MODE == kHwDown) ? (CIN >= 32) : (CIN >= 64);
  const int classes = (MODE == kHwUp) ? 2 : 1;
  const int route = (int)mdf::env_int("MDF_CONV3D_HW_ROUTE", 0);
  if (route == 1) return launch_hw<CIN, COUT, MODE, 1, 1>(p, st);
  if (route == 2) return launch_hw<CIN, COUT, MODE, MTMAX, 1>(p, st);
  if constexpr (kSplitBuilt) {
    if (route == 3) return launch_hw<CIN, COUT, MODE, 1, 4>(p, st);
  }
  if (route == 3) return launch_hw<CIN, COUT, MODE, 1, 1>(p, st);
  // The largest wave tile from 448 "big" blocks up.  Measured (us, largest tile / one tile / split-K): 462 blocks (down 32 -> 64 @8x148x200)
  // 70.5 / 76.4 / 75.2; 693 (up 64 -> 32 @24x37x50) 71.3 / 93.1 / 97.2, (down 16 -> 32 @24x148x200) 59.2 / 62.2; 925 (up 64 -> 32 @8x74x100)
  // 85.6 / 126.0 / 126.3; the layers above 1024 blocks 84-134 against 107-180.  Below: 346 blocks (down 32 -> 64 @24x74x100) 68.2 / 58.5 /
  // 56.5 -- the largest tile loses.  448 lies between 346 and 462; where exactly the crossing is, and whether it is the same for every
  // channel pair, is NOT measured (launch_conv_mt's 1024 was measured on the (2,2,2) layers and is too high here).
  const long long tiles_big = p.m_total / (64LL * MTMAX) * classes;
  if (tiles_big >= 448) return launch_hw<CIN, COUT, MODE, MTMAX, 1>(p, st);
  // few tiles and a deep K: the taps split over the block's four waves.  One measured point (346 big blocks, above): 56.5 against 58.5
  // with one tile per wave.  Smaller volumes -- the ones launch_conv_mt's split-K was made for -- are NOT measured for this stride.
  if constexpr (kSplitBuilt) return launch_hw<CIN, COUT, MODE, 1, 4>(p, st);
  return launch_hw<CIN, COUT, MODE, 1, 1>(p, st);
}

}  // namespace

#define MDF_HW_CASE(ci, co, mode) \
  if (Cin == ci && Cout == co && m == mode) return launch_hw_mt<ci, co, mode>(p, (hipStream_t)stream);

// Conv3d(k3, stride (1,2,2), pad 1) / ConvTranspose3d(k3, stride (1,2,2), pad 1, output_padding (0,1,1)) with the fused epilogue of
// mdf_conv3d_fwd.  Never allocates, never synchronises.
extern "C" int mdf_conv3d_hw2_fwd(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res, float* y,
                                  int B, int Di, int Hi, int Wi, int Cin, int Cout, int transposed, int relu, void* stream) {
  MDF_REQUIRE(x && wpack && y, "null pointer argument");
  MDF_REQUIRE((alpha == nullptr) == (beta == nullptr), "alpha and beta must both be given or both be NULL");
  MDF_REQUIRE(B > 0 && Di > 0 && Hi > 0 && Wi > 0, "bad shape");
  MDF_REQUIRE((long long)B * Di * Hi * Wi * Cin < (1ll << 31), "input volume too large for 32-bit offsets");
  const int m = transposed ? kHwUp : kHwDown;
  const int kd_skip = mdf::env_int("MDF_CONV3D_KDSKIP", 1) && Di <= 3;   // dev A/B (read per call), the switch of mdf_conv3d_fwd
  // (the index space and the output dims of conv_params' stride-2 / transposed modes, with the depth kept)
  ConvParams p = conv_params(x, wpack, alpha, beta, res, y, B, Di, Hi, Wi, transposed ? kTr : kS2, relu, kd_skip, nullptr);
  p.Do = Di;
  p.m_total = transposed ? (long long)B * Di * Hi * Wi : (long long)B * p.Do * p.Ho * p.Wo;
  MDF_HW_CASE(8, 16, kHwDown) MDF_HW_CASE(16, 32, kHwDown) MDF_HW_CASE(32, 64, kHwDown)
  MDF_HW_CASE(64, 32, kHwUp) MDF_HW_CASE(32, 16, kHwUp) MDF_HW_CASE(16, 8, kHwUp)
  return mdf::fail(MDF_EUNSUPPORTED, "conv3d stride (1,2,2) Cin=%d Cout=%d transposed=%d is not built", Cin, Cout, transposed);
}
