// 3-D convolution layers of the cost regularisers (net/unit/regular.py:9-133, base.py:50-68) as an
// implicit GEMM on the fp32 matrix cores of gfx950 (v_mfma_f32_16x16x4_f32: exact f32 fma chain, so
// results differ from the reference only by summation order).
//
// Data layout: activations NDHWC (the aggregation kernel writes the cost volume in this layout), so the
// Cin values of one voxel are contiguous and one MFMA B-fragment (16 voxels x 16 cin) is a single
// coalesced 1-KiB wavefront load.  GEMM orientation is  D[cout][voxel] = W[cout][k] * X[k][voxel]:
//   A operand (weights)     lane l holds W[cout = l&15][k = l>>4]
//   B operand (activations) lane l holds X[k = l>>4][voxel = l&15]
//   C/D                     lane l holds couts 4*(l>>4)..+3 of voxel l&15  -> one 16-B store per lane,
//                           the 4 lanes of a voxel write 64 contiguous bytes (NDHWC output).
// K is walked tap by tap; inside a tap the k order is permuted so that lane group q = l>>4 owns cin
// {KPL*q .. KPL*q+KPL-1} of a chunk: a lane fetches its KPL consecutive cin with ONE 8/16-byte load and
// feeds them to KPL successive MFMAs.  Weights are pre-packed on the device into exactly that fragment
// order (conv_pack.hip: mdf_conv3d_pack_weights), so an A fragment is also one coalesced load.
//
// Epilogue (fused): y = [res +] [relu]( acc * alpha + beta )   (BatchNorm3d folded as ATen does in eval).
//
// Modes: stride 1, stride 2, and ConvTranspose3d(k3,s2,p1,op1).  The transposed conv is computed per
// output parity class (blockIdx.y = 0..7): inside a class every output voxel uses the same 1/2/4/8 taps,
// so no MFMA is spent on structurally-zero taps.
//
// Here: conv3d_kernel (every layer), conv3d_wlds_kernel (weight set in LDS) and the 3-D entry with its route rules.  The voxel
// bookkeeping and the epilogue are conv3d_common.h's; the transposed layers' own kernels are convtr3d.hip's.
#include <cstdlib>
#include "conv3d_common.h"
#include "conv_dispatch.h"

namespace {

// SPLITK = 4: the four waves of a block share ONE wave tile and each takes every 4th tap; partial accumulators are summed
// through LDS.  For tiny volumes (a few thousand voxels, 27*64 deep K) this turns ~90 serial-latency-bound blocks into 4x
// as many quarter-length ones.
template <int CIN, int COUT, int MODE, int MT, int SPLITK, int ST = 0>
__global__ __launch_bounds__(256) void conv3d_kernel(const ConvParams p) {
  constexpr int KPL = (CIN >= 16) ? 4 : 2;   // k values per lane per chunk
  constexpr int CK = 4 * KPL;                // cin per chunk
  constexpr int NCH = CIN / CK;
  // transposed: GEMM rows are [pw][cout] (both output w-parities of an input voxel in one wave -> one contiguous
  // 2*COUT store per input voxel, and no padded rows for COUT = 8)
  constexpr int ROWS = (MODE == kTr) ? 2 * COUT : COUT;
  constexpr int NT = (ROWS + 15) / 16;
  static_assert(CIN % CK == 0, "CIN must be a multiple of the chunk");

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = lane >> 4;    // k sub-slot / cout quad
  const int n16 = lane & 15;  // voxel inside the m-tile (B operand, C/D column)
  // ST: block-level fp64 table of the epilogue sums [2][64] + the producing layer's (a, b, mean, invstd) [4][64].  Sending the
  // sums to memory costs 2*COUT same-address fp64 atomics per BLOCK (~10 ns each, serialised at the memory side): a one-tile
  // block per 16-64 voxels made that the most expensive part of the small layers (rocprof: 32->32 split-K 24 -> 52 us).  The ST
  // form therefore (a) is persistent above the number of blocks the chip holds at once (these kernels live on residency: the
  // grid is capped at that, not lower) and (b) spreads the blocks over slices of stat_out (common.h: conv_stat_send).
  __shared__ double st_tab[ST ? 128 : 1];
  __shared__ float st_aux[ST ? 256 : 1];
  if constexpr (ST != 0) {
    if (threadIdx.x < 128) st_tab[threadIdx.x] = 0.0;
    if (p.stat_mode == 2) {
      const int c = threadIdx.x & 63;
      st_aux[threadIdx.x] = (c < COUT) ? p.stat_aux[(threadIdx.x >> 6) * COUT + c] : 0.f;
    }
    __syncthreads();
  }
  for (unsigned vblk = blockIdx.x; vblk < (ST ? p.nblk : blockIdx.x + 1); vblk += gridDim.x) {
  const unsigned tile_blk = mdf::xcd_remap(vblk, p.nblk);
  const long long m0 = (SPLITK > 1 ? (long long)tile_blk : (long long)tile_blk * 4 + wave) * (MT * 16);

  // transposed: parity class of this block
  const int pc = (MODE == kTr) ? blockIdx.y : 0;   // 4 classes: (pd, ph); both pw live in the wave
  const int pd = (pc >> 1) & 1, ph = pc & 1;

  // per-lane voxel bookkeeping for each m-tile
  int in_off[MT];       // float offset of the base input voxel (channel 0)
  long long out_vox[MT];
  unsigned vmask[MT];   // tap_mask: bits 0-2: kd valid, 3-5: kh valid, 6-8: kw valid
  bool live[MT];
  // index space dims (output dims for S1/S2, input dims for Tr)
  const int Md = (MODE == kTr) ? p.Di : p.Do, Mh = (MODE == kTr) ? p.Hi : p.Ho, Mw = (MODE == kTr) ? p.Wi : p.Wo;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    long long m = m0 + t * 16 + n16;
    live[t] = m < p.m_total;
    if (!live[t]) m = p.m_total - 1;
    const Voxel v = split_voxel(m, Md, Mh, Mw);
    constexpr int sd = (MODE == kS2) ? 2 : 1;
    const int bd = sd * v.d, bh = sd * v.h, bw = sd * v.w;  // base input coordinate
    const unsigned vm = tap_mask<MODE == kTr>(bd, bh, bw, p.Di, p.Hi, p.Wi);
    vmask[t] = live[t] ? vm : 0u;
    in_off[t] = (int)((((long long)v.b * p.Di + bd) * p.Hi + bh) * p.Wi + bw) * CIN;
    if (MODE == kTr)
      out_vox[t] = (((long long)v.b * p.Do + (2 * v.d + pd)) * p.Ho + (2 * v.h + ph)) * p.Wo + 2 * v.w;   // pw added in the epilogue
    else
      out_vox[t] = m;
  }

  // Depth taps that NO voxel of this wave's tiles has (the innermost U-Net levels are 1-3 planes deep: at D = 1 only kd = 1 exists,
  // at D = 2 two of three) are skipped altogether -- they contributed exact zeros (operand scaled by 0) for a third to two thirds of
  // the launch's MFMAs and fragment fetches.  Wave-uniform: a wave's tiles are runs of a row and share d except across a plane edge.
  unsigned kd_any = 7u;
  if (MODE != kTr && p.kd_skip) kd_any = kd_any_of(vmask);

  f32x4 acc[MT][NT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[t][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Epilogue operands (folded BN, residual) are fetched NOW so their L2 round trip overlaps the tap loop: a block lives for
  // one wave tile (10-20 us), an exposed ~1 us at its end is 5-10 % of it.
  // (the residual only for the transposed layers -- the ones that carry a skip connection in these networks; holding it for
  // the others costs the big-tile kernels an occupancy step)
  constexpr bool kPrefetchRes = (MODE == kTr);
  float4 ep_al[NT], ep_be[NT], ep_res[kPrefetchRes ? MT : 1][NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r0 = nt * 16 + 4 * q;
    const int c0 = (MODE == kTr) ? r0 % COUT : r0;
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

  // transposed: output parity p uses kernel taps with (k + p) odd: p=0 -> k=1 (input i') ; p=1 -> k=0 (input i'+1),
  // k=2 (input i').  Only the class's valid (kd, kh) pairs are enumerated (1, 2 or 4 of them) x 2 input w-offsets, so a
  // split-K stride hands every wave real work.  Along w: offset 0 feeds pw=0 (kw=1) and pw=1 (kw=2); offset +1 feeds pw=1 (kw=0).
  const int nkh = 1 + ph;
  const int ntaps = (MODE == kTr) ? (1 + pd) * nkh * 2 : 27;
  // Software pipeline over the taps: the operands of tap j+1 (all cin chunks: NCH*(MT+NT) 16-byte fragments) are requested before
  // the MFMAs of tap j.  A block lives for ONE wave tile, so without it every tap exposes an L2 round trip: the small layers
  // (1/8-resolution volumes, the transposed up-sampling layers) were pure latency -- 64->32 T at 1x74x100: 46 us for 0.8 GFLOP.
  struct TapRegs {
    Frag<KPL> bf[NCH][MT], af[NCH][NT];
    int ow;
  };
  auto load_tap = [&](int j, TapRegs& r) {
    int kd, kh, kw, od, oh, ow, tap;
    if (MODE == kTr) {
      ow = j & 1;
      const int jh = (j >> 1) % nkh, jd = (j >> 1) / nkh;
      kd = pd ? 2 * jd : 1;
      kh = ph ? 2 * jh : 1;
      od = (kd == 0); oh = (kh == 0);
      kw = ow ? 0 : 1;                  // validity-mask slot of the w offset: bit 0 <-> offset +1, bit 1 <-> offset 0
      tap = (kd * 3 + kh) * 2 + ow;     // slot in the packed weights
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
        // branch-free: an out-of-range tap reads the voxel's own (valid) position and is zeroed by a multiply.  A predicated
        // load compiles to a branch and a wait per load (s_and_saveexec / s_cbranch_execz), which serialises the fetches of
        // a tap step; a select instead of the multiply lets the compiler sink the load back under the condition.
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
            // transposed, offset +1: rows of parity pw = 0 are structurally zero -> skip n-tiles made only of such rows
            if (MODE == kTr && r.ow == 1 && (nt + 1) * 16 <= COUT) continue;
            acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(r.af[ch][nt].v[s], r.bf[ch][t].v[s], acc[t][nt], 0, 0, 0);
          }
  };
  // (measured per variant: the single-tile transposed kernels gain 1.1-1.9x -- 64->32 T 77 / 44 / 46 -> 53 / 23 / 25 us; the big-tile
  // variants lose the occupancy their HBM-bound layers live on -- 32->16 T 92 -> 125 us, 16->8 T 88 -> 104 --, and the split-K stride-1
  // kernels lose too -- 64->64 65 -> 85: those keep one tap in flight)
  constexpr bool kPipeTaps = (MODE == kTr && MT == 1);
  {
    const int js = (SPLITK > 1) ? SPLITK : 1;
    int j = (SPLITK > 1) ? wave : 0;
    if constexpr (MODE == kTr) {
      // shallow volumes: a class with output parity pd = 1 has the depth taps kd = 0 (input plane d + 1) and kd = 2 (plane d); on the last
      // plane -- the only one at Di = 1 -- the kd = 0 half multiplies zeros.  kd is the slowest tap index: skipping it is a later start.
      if (p.kd_skip && pd && !__any((int)(vmask[0] & 1u))) {
        bool none = true;
#pragma unroll
        for (int t = 1; t < MT; ++t) none = none && !__any((int)(vmask[t] & 1u));
        if (none) j = __builtin_amdgcn_readfirstlane(nkh * 2);
      }
    }
    if constexpr (kPipeTaps) {
      TapRegs ra, rb;
      if (j < ntaps) load_tap(j, ra);
      while (j < ntaps) {
        if (j + js < ntaps) load_tap(j + js, rb);
        __builtin_amdgcn_sched_barrier(0);       // (the requests stay ahead of the MFMAs; hipcc otherwise sinks them to their first use)
        mul_tap(ra);
        j += js;
        if (j >= ntaps) break;
        if (j + js < ntaps) load_tap(j + js, ra);
        __builtin_amdgcn_sched_barrier(0);
        mul_tap(rb);
        j += js;
      }
    } else {
      if (kd_any == 7u) {                 // (the common case keeps its own loop: a test per tap costs the unrolled form 10-25 %, measured)
        for (; j < ntaps; j += js) {
          TapRegs r;
          load_tap(j, r);
          mul_tap(r);
        }
      } else {
        for (; j < ntaps; j += js) {
          if (!((kd_any >> (j / 9)) & 1u)) continue;     // (see kd_any)
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

  // epilogue: lane owns couts nt*16 + 4q .. +3 of voxel out_vox[t]
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r0 = nt * 16 + 4 * q;   // first GEMM row of this lane
    if (r0 >= ROWS) continue;
    const int pw_out = (MODE == kTr) ? r0 / COUT : 0;
    const int c0 = (MODE == kTr) ? r0 % COUT : r0;
    float ps[4] = {0.f, 0.f, 0.f, 0.f}, pq[4] = {0.f, 0.f, 0.f, 0.f};   // ST: this lane's sums over its m-tiles
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (!live[t]) continue;
      if (SPLITK > 1 && ((t * NT + nt) & 3) != wave) continue;  // another wave finishes this pair
      float4 o = scale_shift_relu(acc[t][nt], ep_al[nt], ep_be[nt], p.relu);
      const size_t oi = (size_t)(out_vox[t] + pw_out) * COUT + c0;
      add_res_store<kPrefetchRes>(p, oi, o, ep_res[kPrefetchRes ? t : 0][nt]);      // (prefetched for the transposed layers only, see above)
      if constexpr (ST != 0) {
        const float ov[4] = {o.x, o.y, o.z, o.w};
        stat_accum<0>(p.stat_mode, p.stat_y, st_aux, oi, c0, ov, ps, pq);
      }
    }
    if constexpr (ST != 0) stat_commit(st_tab, c0, n16, ps, pq);
  }
  if constexpr (ST != 0 && SPLITK > 1) __syncthreads();   // the next tile's partial sums overwrite `part`
  }  // tile loop (one tile unless ST)
  if constexpr (ST != 0) {
    __syncthreads();
    mdf::conv_stat_send<COUT>(st_tab, p.stat_out, 2 * COUT, p.stat_slices, blockIdx.y * gridDim.x + blockIdx.x);
  }
}

// ---- small and mid-size stride-1 / stride-2 layers whose whole packed weight set fits LDS (16 -> 32: 55 KB, 32 -> 32: 110 KB) ---------
// conv3d_kernel streams every weight fragment through the vector L1 for ONE 16-voxel tile (a fragment is used by 1-2 MFMAs per m-tile
// and n-tile: 512 B per MFMA at 32 -> 32, the whole L1 rate), and its one-tile blocks come in a ragged 1.3-2.7 rounds.  Here a block is
// the 16 waves one CU holds: the weight set is copied to LDS once per block, every wave walks m-tiles (stride = the grid's waves) and
// reads its A fragments with ds_read_b128; the B fragments of the next tap are requested before the MFMAs of the current one.
// Per accumulator the MFMA order is conv3d_kernel's without split-K (tap, cin chunk, k).  Eval only (no epilogue sums).
template <int CIN, int COUT, int MODE, int MT, int ST>
__global__ __launch_bounds__(1024) void conv3d_wlds_kernel(const ConvParams p) {
  constexpr int KPL = (CIN >= 16) ? 4 : 2, CK = 4 * KPL, NCH = CIN / CK, NT = (COUT + 15) / 16;
  constexpr int TAPF = NCH * NT * 64 * KPL;             // floats per tap in the packed set
  static_assert(MODE == kS1 || MODE == kS2, "stride-1 / stride-2 layers");
  extern __shared__ float wsm[];
  {
    const float4* src = reinterpret_cast<const float4*>(p.wpack);
    float4* dst = reinterpret_cast<float4*>(wsm);
    for (int i = threadIdx.x; i < 27 * TAPF / 4; i += 1024) dst[i] = src[i];
  }
  // ST (training): the block's fp64 table of the epilogue sums and the producing layer's (a, b, mean, invstd), as in conv3d_kernel
  __shared__ double st_tab[ST ? 128 : 1];
  __shared__ float st_aux[ST ? 256 : 1];
  if constexpr (ST != 0) {
    if (threadIdx.x < 128) st_tab[threadIdx.x] = 0.0;
    if (p.stat_mode == 2 && threadIdx.x < 256) {
      const int c = threadIdx.x & 63;
      st_aux[threadIdx.x] = (c < COUT) ? p.stat_aux[(threadIdx.x >> 6) * COUT + c] : 0.f;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, n16 = lane & 15;
  float4 ep_al[NT], ep_be[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r0 = nt * 16 + 4 * q;
    fetch_scale_shift(p, r0 < COUT, r0, ep_al[nt], ep_be[nt]);
  }
  const float* xq = p.x + KPL * q;
  const float* wl = wsm + lane * KPL;
  const int sd = (MODE == kS2) ? 2 : 1;
  // m-tiles: XCD x (= blockIdx.x & 7) owns a contiguous eighth of them (neighbouring tiles' halos meet in one L2); inside it consecutive
  // tiles go to consecutive blocks, so that every CU is busy whatever the tile count (nblk = number of m-tile groups of MT tiles)
  const unsigned bx = blockIdx.x >> 3, nbx = gridDim.x >> 3;
  const mdf::XcdChunk chunk = mdf::xcd_chunk(blockIdx.x, p.nblk);
  for (unsigned l = (unsigned)wave * nbx + bx; l < chunk.len; l += 16u * nbx) {
    const long long m0 = (long long)(chunk.start + l) * (MT * 16);
    int in_off[MT];
    unsigned vmask[MT];                     // tap_mask: bits 0-2: kd valid, 3-5: kh valid, 6-8: kw valid
    long long out_vox[MT];
    bool live[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      long long m = m0 + t * 16 + n16;
      live[t] = m < p.m_total;
      if (!live[t]) m = p.m_total - 1;
      const Voxel v = split_voxel(m, p.Do, p.Ho, p.Wo);
      const int bd = sd * v.d, bh = sd * v.h, bw = sd * v.w;
      const unsigned vm = tap_mask(bd, bh, bw, p.Di, p.Hi, p.Wi);
      vmask[t] = live[t] ? vm : 0u;
      in_off[t] = (int)((((long long)v.b * p.Di + bd) * p.Hi + bh) * p.Wi + bw) * CIN;
      out_vox[t] = m;
    }
    // depth taps no voxel of this wave has (volumes 1-3 planes deep): skipped, as in conv3d_kernel (kd_any)
    unsigned kd_any = 7u;
    if (p.kd_skip) kd_any = kd_any_of(vmask);
    f32x4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[t][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto load_b = [&](int kd, int kh, int kw, Frag<KPL> (&bf)[NCH][MT]) {
      const int tapoff = (((kd - 1) * p.Hi + (kh - 1)) * p.Wi + (kw - 1)) * CIN;
      const unsigned need = (1u << kd) | (8u << kh) | (64u << kw);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int t = 0; t < MT; ++t) {      // (branch-free: see conv3d_kernel)
          const bool ok = (vmask[t] & need) == need;
          bf[ch][t].load(xq + in_off[t] + (ok ? tapoff : 0) + ch * CK);      // (zeroed in mul_tap: a multiply here would wait for the load)
        }
    };
    auto mul_tap = [&](int tap, int kd, int kh, int kw, Frag<KPL> (&bf)[NCH][MT]) {
      const float* wt = wl + tap * TAPF;
      const unsigned need = (1u << kd) | (8u << kh) | (64u << kw);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const float okf = ((vmask[t] & need) == need) ? 1.0f : 0.0f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) bf[ch][t].scale(okf);
      }
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        Frag<KPL> af[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) af[nt].load(wt + (ch * NT + nt) * (64 * KPL));
#pragma unroll
        for (int s = 0; s < KPL; ++s)
#pragma unroll
          for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[nt].v[s], bf[ch][t].v[s], acc[t][nt], 0, 0, 0);
      }
    };
    // groups of RB rows (kd, kh) of three taps; the next group's B fragments are requested before the current group's MFMAs (two register
    // sets).  (8 input channels, 2 registers per fragment: a whole kd plane of 9 taps per group was measured -- 8->16 s2 @24x296x400
    // 44.7 -> 50.0 us, @8x592x800 58.7 -> 64.8: worse)
    constexpr int RB = 1;
    struct RowRegs { Frag<KPL> b[3 * RB][NCH][MT]; };
    auto load_row = [&](int r, RowRegs& rr) {
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int kd = (r + i) / 3, kh = (r + i) - 3 * kd;
        load_b(kd, kh, 0, rr.b[3 * i]);
        load_b(kd, kh, 1, rr.b[3 * i + 1]);
        load_b(kd, kh, 2, rr.b[3 * i + 2]);
      }
    };
    auto mul_row = [&](int r, RowRegs& rr) {
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int kd = (r + i) / 3, kh = (r + i) - 3 * kd;
        mul_tap(3 * (r + i), kd, kh, 0, rr.b[3 * i]);
        mul_tap(3 * (r + i) + 1, kd, kh, 1, rr.b[3 * i + 1]);
        mul_tap(3 * (r + i) + 2, kd, kh, 2, rr.b[3 * i + 2]);
      }
    };
    auto next_row = [&](int r) {
      r += RB;
      while (r < 9 && !((kd_any >> (r / 3)) & 1u)) r += RB;
      return r;
    };
    {
      RowRegs ra, rb;
      int r = next_row(-RB);
      if (r < 9) load_row(r, ra);
      while (r < 9) {
        int rn = next_row(r);
        if (rn < 9) load_row(rn, rb);
        __builtin_amdgcn_sched_barrier(0);       // (the requests stay ahead of the MFMAs)
        mul_row(r, ra);
        r = rn;
        if (r >= 9) break;
        rn = next_row(r);
        if (rn < 9) load_row(rn, ra);
        __builtin_amdgcn_sched_barrier(0);
        mul_row(r, rb);
        r = rn;
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int r0 = nt * 16 + 4 * q;
      if (r0 >= COUT) continue;
      float ps[4] = {0.f, 0.f, 0.f, 0.f}, pq[4] = {0.f, 0.f, 0.f, 0.f};   // ST: this lane's sums over its m-tiles
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (!live[t]) continue;
        float4 o = scale_shift_relu(acc[t][nt], ep_al[nt], ep_be[nt], p.relu);
        const size_t oi = (size_t)out_vox[t] * COUT + r0;
        add_res_store<false>(p, oi, o);      // (no prefetch: these layers carry no skip connection in the networks, as in conv3d_kernel)
        if constexpr (ST != 0) {
          const float ov[4] = {o.x, o.y, o.z, o.w};
          stat_accum<0>(p.stat_mode, p.stat_y, st_aux, oi, r0, ov, ps, pq);
        }
      }
      if constexpr (ST != 0) stat_commit(st_tab, r0, n16, ps, pq);
    }
  }
  if constexpr (ST != 0) {
    __syncthreads();
    mdf::conv_stat_send<COUT>(st_tab, p.stat_out, 2 * COUT, p.stat_slices, blockIdx.x);
  }
}

template <int CIN, int COUT, int MODE, int MT, int ST = 0>
int launch_conv_wlds(ConvParams& p, hipStream_t st) {
  constexpr int KPL = (CIN >= 16) ? 4 : 2, NCH = CIN / (4 * KPL), NT = (COUT + 15) / 16;
  constexpr size_t kLds = (size_t)27 * NCH * NT * 64 * KPL * sizeof(float);
  static_assert(kLds <= 160 * 1024, "the packed weight set must fit LDS");
  if (ST) p.stat_slices = mdf::conv_stat_slices(256, p.stat_slices);
  return launch_lds_weights<&conv3d_wlds_kernel<CIN, COUT, MODE, MT, ST>>(p, (unsigned)((p.m_total + MT * 16 - 1) / (MT * 16)) /* wave tiles */,
                                                                          1024 /* 16 waves */, kLds, st, "conv3d_wlds_kernel");
}

template <int CIN, int COUT, int MODE, int MT, int SPLITK, int ST>
int launch_conv(ConvParams& p, hipStream_t st) {
  const long long per_blk = (SPLITK > 1 ? 1LL : 4LL) * MT * 16;
  p.nblk = (unsigned)((p.m_total + per_blk - 1) / per_blk);
  unsigned gx = p.nblk;
  if (ST) {   // persistent above what the chip holds at once (8 blocks per CU)
    const unsigned cap = (MODE == kTr) ? 512u : 2048u;
    if (gx > cap) gx = cap;
    p.stat_slices = mdf::conv_stat_slices((long long)gx * (MODE == kTr ? 4 : 1), p.stat_slices);
  }
  dim3 grid(gx, MODE == kTr ? 4 : 1), block(256);
  hipLaunchKernelGGL((conv3d_kernel<CIN, COUT, MODE, MT, SPLITK, ST>), grid, block, 0, st, p);
  return mdf::check_launch("conv3d_kernel");
}

template <int CIN, int COUT, int MODE, int ST>
int launch_conv_mt(ConvParams& p, hipStream_t st) {
  constexpr int ROWS = (MODE == kTr) ? 2 * COUT : COUT;
  constexpr int MTMAX = (ROWS > 32) ? 2 : 4;
  // small volumes: shrink the wave tile so the grid still covers the 256 CUs a few times over
  const long long tiles_big = p.m_total / (64LL * MTMAX) * (MODE == kTr ? 4 : 1);
  // (8 -> 16 stride 2 at 24x296x400: 51.5 us with 4 m-tiles per wave, 47.8 with 2, 56.1 with 1; the other stride-2 / transposed layers
  //  are best at their MTMAX or indifferent)
  if (MODE == kS2 && CIN == 8 && ST == 0 && tiles_big >= 1024) return launch_conv<CIN, COUT, MODE, 2, 1, ST>(p, st);
  {   // dev A/B: two m-tiles per wave for the mid-size one-tile layers (half the weight bytes through L1 per voxel)
    // (r05: 16 -> 32 stride 2 at 48x148x200 -- 693 four-tile blocks' worth -- 68.6 -> 62.6 us; below ~500 the grid is too small)
    const long long mt2_min = mdf::env_int("MDF_CONV3D_MT2_MIN_TILES", 512);
    if (ST == 0 && MODE != kTr && mt2_min >= 0 && tiles_big < 1024 && tiles_big >= mt2_min && !(CIN >= 32 && p.m_total / 16 < 4096))
      return launch_conv<CIN, COUT, MODE, 2, 1, ST>(p, st);
  }
  const long long mt_min = mdf::env_int("MDF_CONV3D_MT_MIN_TILES", 1024);   // dev A/B (read per call)
  if (tiles_big >= mt_min) return launch_conv<CIN, COUT, MODE, MTMAX, 1, ST>(p, st);
  // few tiles and a deep K (27*CIN >= 864): split the taps over the block's waves
  const long long tiles_1 = p.m_total / 16 * (MODE == kTr ? 4 : 1);
  if (MODE != kTr && CIN >= 32 && tiles_1 < 4096) {   // (transposed classes have only 2-8 taps)
    // m-tiles per split-K block: with ONE 16-voxel tile a block streams the layer's whole weight set (442 KB at 64 -> 64) through its
    // L1 for 16 voxels -- 1388 blocks x 442 KB = 0.6 GB from the L2s per launch at 12x37x50; two tiles halve that
    // (r05, 64 output channels at ~1400 tiles: 64 -> 64 @12x37x50 62 -> 57 us, 32 -> 64 s2 @24x74x100 35 -> 31; the 32 -> 32 layers and
    //  the volumes under ~500 tiles are indifferent or lose: they keep one tile)
    const int sk_mt = mdf::env_int("MDF_CONV3D_SK_MT", 0);   // dev A/B (read per call): 0 = the rule
    if (ST == 0 && (sk_mt == 2 || (sk_mt == 0 && COUT >= 64)) && tiles_1 >= 1024) return launch_conv<CIN, COUT, MODE, 2, 4, ST>(p, st);
    return launch_conv<CIN, COUT, MODE, 1, 4, ST>(p, st);
  }
  return launch_conv<CIN, COUT, MODE, 1, 1, ST>(p, st);
}

}  // namespace

using mdf::ConvStat;

#define MDF_CONV_CASE(ci, co, mode)                          \
  if (Cin == ci && Cout == co && m == mode)                  \
    return stat ? launch_conv_mt<ci, co, mode, 1>(p, (hipStream_t)stream) : launch_conv_mt<ci, co, mode, 0>(p, (hipStream_t)stream);

static int conv3d_entry(const float* x, const float* wpack, const float* alpha, const float* beta,
                        const float* res, float* y, int B, int Di, int Hi, int Wi, int Cin, int Cout, int stride,
                        int transposed, int relu, void* stream, const ConvStat* stat) {
  MDF_REQUIRE(x && wpack && y, "null pointer argument");
  MDF_REQUIRE((alpha == nullptr) == (beta == nullptr), "alpha and beta must both be given or both be NULL");
  MDF_REQUIRE(B > 0 && Di > 0 && Hi > 0 && Wi > 0, "bad shape");
  MDF_REQUIRE(stride == 1 || stride == 2, "stride must be 1 or 2");
  MDF_REQUIRE(!transposed || stride == 2, "transposed conv is built for stride 2 only");
  MDF_REQUIRE((long long)B * Di * Hi * Wi * Cin < (1ll << 31), "input volume too large for 32-bit offsets");
  const int m = transposed ? kTr : (stride == 2 ? kS2 : kS1);
  const int kd_skip = mdf::env_int("MDF_CONV3D_KDSKIP", 1) && Di <= 3;   // dev A/B (read per call)
  ConvParams p = conv_params(x, wpack, alpha, beta, res, y, B, Di, Hi, Wi, m, relu, kd_skip, stat);
  const long long lds_min = mdf::env_int("MDF_CONV_LDS_MIN_VOXELS", 150000);   // test hook (read per call): 0 forces the LDS kernels at any size
  if (m == kS1 && p.m_total >= lds_min) {  // large stride-1 layers: LDS-staged planes (conv_lds.hip)
    const int rc = mdf_conv_lds_dispatch(x, wpack, alpha, beta, res, 1.0f, nullptr, y, B, Di, Hi, Wi, Cin, Cin, Cout, 3, 3, 1, relu, stream, 0, 0, stat);
    if (rc != MDF_EUNSUPPORTED) return rc;
  }
  if (m == kTr && !stat) {   // transposed layers, eval: the all-classes and class-per-block kernels where their rules apply (convtr3d.hip)
    const int rc = mdf_convtr3d_dispatch(x, wpack, alpha, beta, res, y, B, Di, Hi, Wi, Cin, Cout, relu, kd_skip, stream);
    if (rc != MDF_EUNSUPPORTED) return rc;
  }
  // weights-in-LDS form for the small and mid-size layers whose packed set fits (eval)
  if (stat) {    // training: the same form with the epilogue sums
    const int wlt = mdf::env_int("MDF_CONV3D_WLDS_TRAIN", 1);   // dev A/B (read per call): 0 = off
    if (wlt == 1) {
      if (Cin == 32 && Cout == 32 && m == kS1) return launch_conv_wlds<32, 32, kS1, 1, 1>(p, (hipStream_t)stream);
      if (Cin == 16 && Cout == 16 && m == kS1) return launch_conv_wlds<16, 16, kS1, 1, 1>(p, (hipStream_t)stream);
      if (Cin == 16 && Cout == 32 && m == kS2) return launch_conv_wlds<16, 32, kS2, 1, 1>(p, (hipStream_t)stream);
      if (Cin == 8 && Cout == 16 && m == kS2) return launch_conv_wlds<8, 16, kS2, 2, 1>(p, (hipStream_t)stream);
    }
  }
  if (!stat) {
    const int wl = mdf::env_int("MDF_CONV3D_WLDS", 1);   // dev A/B (read per call): 0 = off
    if (wl == 1) {     // (two m-tiles per wave were measured and lose: 32 -> 32 @6x74x100 35 -> 64 us, 16 -> 32 s2 @48x148x200 61 -> 76)
      if (Cin == 32 && Cout == 32 && m == kS1) return launch_conv_wlds<32, 32, kS1, 1>(p, (hipStream_t)stream);
      if (Cin == 16 && Cout == 32 && m == kS2) return launch_conv_wlds<16, 32, kS2, 1>(p, (hipStream_t)stream);
    }
    const bool wl8 = mdf::env_flag("MDF_CONV3D_WLDS8", true);   // dev A/B and the equality test (read per call): 0 = off
    // (8 -> 16 stride 2, the gather-heavy layers: @24x296x400 50.4 us -> 46.5 / 43.5 / 49.7 with 1 / 2 / 4 m-tiles per wave, @8x592x800 66.0 -> 60.1 / 55.0 / 64.8)
    if (wl8 && Cin == 8 && Cout == 16 && m == kS2) return launch_conv_wlds<8, 16, kS2, 2>(p, (hipStream_t)stream);
  }
  // stride 1 (every Cin x Cout the nets use)
  MDF_CONV_CASE(32, 16, kS1) MDF_CONV_CASE(16, 16, kS1) MDF_CONV_CASE(32, 32, kS1) MDF_CONV_CASE(64, 64, kS1)
  MDF_CONV_CASE(16, 8, kS1) MDF_CONV_CASE(8, 8, kS1) MDF_CONV_CASE(8, 16, kS1) MDF_CONV_CASE(16, 32, kS1)
  // first layers of the regularisers behind the variance cost volume (C, not G, input channels) and their input gradients (training)
  MDF_CONV_CASE(64, 16, kS1) MDF_CONV_CASE(32, 8, kS1) MDF_CONV_CASE(16, 64, kS1) MDF_CONV_CASE(8, 32, kS1)
  // stride 2
  MDF_CONV_CASE(16, 32, kS2) MDF_CONV_CASE(32, 64, kS2) MDF_CONV_CASE(8, 16, kS2)
  // transposed
  MDF_CONV_CASE(64, 32, kTr) MDF_CONV_CASE(32, 16, kTr) MDF_CONV_CASE(16, 8, kTr)
  return mdf::fail(MDF_EUNSUPPORTED, "conv3d Cin=%d Cout=%d stride=%d transposed=%d is not built", Cin, Cout, stride,
                   transposed);
}

extern "C" int mdf_conv3d_fwd(const float* x, const float* wpack, const float* alpha, const float* beta,
                              const float* res, float* y, int B, int Di, int Hi, int Wi, int Cin, int Cout, int stride,
                              int transposed, int relu, void* stream) {
  return conv3d_entry(x, wpack, alpha, beta, res, y, B, Di, Hi, Wi, Cin, Cout, stride, transposed, relu, stream, nullptr);
}

// Training: the RAW 3-D conv / transposed conv ([res +] conv(x), no scale / shift / ReLU) whose epilogue also accumulates
// per-channel sums of its output (ConvParams::stat_mode) into stat_out [nslices][2*Cout] fp64, zero-initialised by the caller.
// stat_mode 1 serves the forward pass (the layer's batch statistics); stat_mode 2 the backward pass, where this launch is the
// input-gradient conv of the NEXT layer and its output (+ res, the skip gradient) is dz of the layer that produced stat_y.
extern "C" int mdf_conv3d_train_fwd(const float* x, const float* wpack, const float* res, float* y, int B, int Di, int Hi, int Wi, int Cin,
                                    int Cout, int stride, int transposed, int stat_mode, const float* stat_y, const float* stat_aux,
                                    double* stat_out, int nslices, void* stream) {
  if (int rc = mdf::check_stat(stat_mode, stat_y, stat_aux, stat_out, nslices, Cout)) return rc;
  const ConvStat st{stat_mode, stat_y, stat_aux, stat_out, 0, nslices};
  return conv3d_entry(x, wpack, nullptr, nullptr, res, y, B, Di, Hi, Wi, Cin, Cout, stride, transposed, 0, stream, &st);
}
