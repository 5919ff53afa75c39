// ConvTranspose3d(k3,s2,p1,op1) layers of the cost regularisers on kernels of their own: all four (pd, ph) output parity classes from
// one pass over the input (convtr_all_kernel), and one class per persistent block with its tap slots in LDS (convtr_cls_kernel).
// conv3d.hip has the GEMM orientation, the data layout and the per-class kernel (conv3d_kernel<kTr>) whose accumulation order both
// keep; conv3d_common.h the shared voxel bookkeeping and epilogue; mdf_convtr3d_dispatch below the route rules.
#include <cstdlib>
#include "conv3d_common.h"
#include "conv_dispatch.h"

namespace {

// ---- ConvTranspose3d(k3,s2,p1,op1) on large volumes: all four (pd, ph) output parity classes from one pass over the input -----
// conv3d_kernel<kTr> runs one block per class: every class walks its own 2-8 taps, and the four together fetch the tile's input
// fragments 18 times (once per class tap).  The classes use only 8 distinct input positions -- (d, h, w) + (od, oh, ow), offsets
// 0/1 -- so here a wave visits the 8 positions once and feeds each fragment to every class that has a tap there (4 + 2 + 2 + 1
// classes per w offset = the same 18 MFMA groups): 8 input fetches instead of 18, four times the MFMAs behind every fetch, and
// the 2 x 2 (d, h) output neighbourhood of a tile written by one block.  Positions run (od, oh) = (1,1), (1,0), (0,1), (0,0), so
// every class accumulates its taps in the order of conv3d_kernel<kTr>: bit-identical results.
// NS > 1 (small volumes: fewer m-tiles than the chip has SIMDs): the n-tiles of an m-tile are dealt out to NS waves (blockIdx.y = first
// n-tile, stride NS), each fetching the input fragments itself -- NS times the waves at 1/NS of the MFMAs and weight bytes each.  With
// NS = 2 and four n-tiles a wave holds one tile of each output w-parity, so the two halves carry the same work.
// WL (r05; = waves per block): the packed weight set (18 tap slots; 72 KB at 32 -> 16, 18 KB at 16 -> 8) in LDS, one 12- or 16-wave block per CU walking the m-tiles
// (XCD-chunked, as conv3d_wlds_kernel): the per-class kernel streams 27 KB (16 -> 8) / 55 KB (32 -> 16) of weight fragments through the
// vector L1 for every 16 input voxels -- 3-6 times the bytes of the skip + output stream those voxels cause in HBM.
template <int CIN, int COUT, int MT, int NS, int WL>
__global__ __launch_bounds__(WL ? WL * 64 : 256) void convtr_all_kernel(const ConvParams p) {
  constexpr int KPL = (CIN >= 16) ? 4 : 2, CK = 4 * KPL, NCH = CIN / CK;
  constexpr int ROWS = 2 * COUT, NTA = (ROWS + 15) / 16, NT = NTA / NS;     // NTA n-tiles in all, NT of them in this wave
  static_assert(NTA % NS == 0, "the n-tiles must divide over the NS waves");
  const int nt0 = (NS > 1) ? (int)blockIdx.y : 0;                          // this wave's n-tiles: nt0 + i * NS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, n16 = lane & 15;
  extern __shared__ float wsm[];
  float4 ep_al[NT], ep_be[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int r0 = (nt0 + nt * NS) * 16 + 4 * q;
    fetch_scale_shift(p, r0 < ROWS, r0 % COUT, ep_al[nt], ep_be[nt]);
  }
  const float* xq = p.x + KPL * q;
  const float* wl = (WL ? wsm : p.wpack) + (size_t)lane * KPL;
  unsigned l_first = 0u, l_end = 1u, l_step = 1u, c_start = 0u;
  if constexpr (WL != 0) {
    static_assert(NS == 1, "the LDS-weights form keeps an m-tile's n-tiles in one wave");
    const float4* src = reinterpret_cast<const float4*>(p.wpack);
    float4* dst = reinterpret_cast<float4*>(wsm);
    for (int i = threadIdx.x; i < 18 * NCH * NTA * 64 * KPL / 4; i += WL * 64) dst[i] = src[i];
    __syncthreads();
    const unsigned bx = blockIdx.x >> 3, nbx = gridDim.x >> 3;
    const mdf::XcdChunk chunk = mdf::xcd_chunk(blockIdx.x, p.nblk);      // (p.nblk = wave tiles here)
    c_start = chunk.start;
    l_first = (unsigned)wave * nbx + bx; l_end = chunk.len; l_step = (unsigned)WL * nbx;
  }
  for (unsigned l = l_first; l < l_end; l += l_step) {
  const long long m0 = WL ? (long long)(c_start + l) * (MT * 16) : ((long long)mdf::xcd_remap(blockIdx.x, p.nblk) * 4 + wave) * (MT * 16);

  int in_off[MT];
  long long out_vox[MT];      // output voxel (2d, 2h, 2w) of the lane's input voxel
  unsigned vmask[MT];         // next_mask: bit 0: d+1 inside, bit 1: h+1 inside, bit 2: w+1 inside, bit 3: live
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    long long m = m0 + t * 16 + n16;
    const bool live = m < p.m_total;
    if (!live) m = p.m_total - 1;
    const Voxel v = split_voxel(m, p.Di, p.Hi, p.Wi);
    vmask[t] = next_mask(live, v, p.Di, p.Hi, p.Wi);
    in_off[t] = (int)((((long long)v.b * p.Di + v.d) * p.Hi + v.h) * p.Wi + v.w) * CIN;
    out_vox[t] = (((long long)v.b * p.Do + 2 * v.d) * p.Ho + 2 * v.h) * p.Wo + 2 * v.w;
  }
  f32x4 acc[4][MT][NT];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[c][t][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // WL: the skip tensor's values are requested now, ahead of the tile's MFMAs (a persistent wave has no neighbour block to hide the
  // epilogue's round trip behind)
  constexpr bool kPreRes = (WL != 0);
  float4 ep_res[kPreRes ? 4 : 1][kPreRes ? MT : 1][kPreRes ? NT : 1];
  if constexpr (kPreRes) {
    if (p.res) {
#pragma unroll
      for (int cls = 0; cls < 4; ++cls)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const int r0 = (nt0 + nt * NS) * 16 + 4 * q;
            const size_t oi = (size_t)(out_vox[t] + ((long long)(cls >> 1) * p.Ho + (cls & 1)) * p.Wo + r0 / COUT) * COUT + r0 % COUT;
            ep_res[cls][t][nt] = (r0 < ROWS && (vmask[t] & 8u)) ? *reinterpret_cast<const float4*>(p.res + oi) : make_float4(0.f, 0.f, 0.f, 0.f);
          }
    }
  }
  bool no_next_plane = false;
  if (p.kd_skip) {
    unsigned m_or = 0u;
#pragma unroll
    for (int t = 0; t < MT; ++t) m_or |= vmask[t];
    no_next_plane = !__any((int)(m_or & 1u));
  }
  // The fragments of PG positions are requested together and zeroed where they are used (one round trip per group instead of one per
  // position: a persistent wave's tiles run back to back, nobody else hides them)
  // (the one-tile 64 -> 32 kernels fetching four positions at a time too was measured: @12x37x50 49.9 -> 60.0 us, worse)
  constexpr int PG = (WL != 0) ? ((64 / (NCH * MT * KPL) >= 8) ? 8 : (64 / (NCH * MT * KPL) >= 4) ? 4 : 1) : 1;
  Frag<KPL> bfa[PG][NCH][MT];
#pragma unroll
  for (int pos = 0; pos < 8; ++pos) {
    const int od = 1 - (pos >> 2), oh = 1 - ((pos >> 1) & 1), ow = pos & 1;
    const unsigned need = 8u | (od ? 1u : 0u) | (oh ? 2u : 0u) | (ow ? 4u : 0u);
    if constexpr (PG > 1) {
      if (pos % PG == 0) {
#pragma unroll
        for (int p2 = pos; p2 < pos + PG; ++p2) {
          const int od2 = 1 - (p2 >> 2), oh2 = 1 - ((p2 >> 1) & 1), ow2 = p2 & 1;
          const unsigned need2 = 8u | (od2 ? 1u : 0u) | (oh2 ? 2u : 0u) | (ow2 ? 4u : 0u);
          const int tapoff2 = ((od2 * p.Hi + oh2) * p.Wi + ow2) * CIN;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int t = 0; t < MT; ++t) bfa[p2 - pos][ch][t].load(xq + in_off[t] + (((vmask[t] & need2) == need2) ? tapoff2 : 0) + ch * CK);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int tapoff = ((od * p.Hi + oh) * p.Wi + ow) * CIN;
    if (NS == NTA && NTA > 1 && ow == 1 && (nt0 + 1) * 16 <= COUT) continue;   // one n-tile per wave, of parity pw = 0: nothing to do at offset +1
    if (od == 1 && no_next_plane) continue;             // shallow volumes: no voxel of the wave has plane d + 1 (see conv3d_kernel: kd_skip)
    Frag<KPL> bf[NCH][MT];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int t = 0; t < MT; ++t) {   // (branch-free, as in conv3d_kernel: an absent neighbour reads the voxel itself and is zeroed)
        const bool ok = (vmask[t] & need) == need;
        if constexpr (PG > 1) bf[ch][t] = bfa[pos % PG][ch][t];
        else bf[ch][t].load(xq + in_off[t] + (ok ? tapoff : 0) + ch * CK);
        bf[ch][t].scale(ok ? 1.0f : 0.0f);       // (PG > 1: zeroed at use -- the group's loads are still in flight; else at load, as conv3d_kernel)
      }
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
      const int pd = cls >> 1, ph = cls & 1;
      if (od > pd || oh > ph) continue;                   // parity 0 has its one tap at offset 0
      const int kd = pd ? (od ? 0 : 2) : 1, kh = ph ? (oh ? 0 : 2) : 1;
      const float* wt = wl + (size_t)((kd * 3 + kh) * 2 + ow) * (NCH * NTA * 64 * KPL);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        Frag<KPL> af[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) af[nt].load(wt + (size_t)(ch * NTA + nt0 + nt * NS) * (64 * KPL));
#pragma unroll
        for (int s = 0; s < KPL; ++s)
#pragma unroll
          for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              // offset +1 feeds parity pw = 1 only: the n-tiles of pw = 0 are structurally zero (NS = 2 of 4 tiles: the wave's first; else wave-uniform)
              const bool pw0_tile = (NS == 2 && NTA == 4) ? (nt == 0) : ((nt0 + nt * NS + 1) * 16 <= COUT);
              if (ow == 1 && pw0_tile) continue;
              acc[cls][t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[nt].v[s], bf[ch][t].v[s], acc[cls][t][nt], 0, 0, 0);
            }
      }
    }
  }
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int pd = cls >> 1, ph = cls & 1;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int r0 = (nt0 + nt * NS) * 16 + 4 * q;
      if (r0 >= ROWS) continue;
      const int pw_out = r0 / COUT, c0 = r0 % COUT;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (!(vmask[t] & 8u)) continue;
        float4 o = scale_shift_relu(acc[cls][t][nt], ep_al[nt], ep_be[nt], p.relu);
        const size_t oi = (size_t)(out_vox[t] + ((long long)pd * p.Ho + ph) * p.Wo + pw_out) * COUT + c0;
        // (the skip values: prefetched by the persistent form only, see kPreRes)
        add_res_store<kPreRes>(p, oi, o, ep_res[kPreRes ? cls : 0][kPreRes ? t : 0][kPreRes ? nt : 0]);
      }
    }
  }
  }  // tile loop (one tile unless WL)
}

// ---- 64 -> 32 transposed layers: one parity class per persistent block, the class's tap slots in LDS ---------------------------------
// The 64 -> 32 weight set (18 slots x 16 KB) does not fit LDS, and the all-classes kernel streams it through the vector L1 once per
// 16 input voxels (0.6 GB from the L2s per launch at 12x37x50: that stream, not the MFMAs, is its time).  The slots of ONE (pd, ph) class
// do fit (2 / 4 / 4 / 8 slots = 32-128 KB): the 256 blocks are shared out 32 : 56 : 56 : 112 over the four classes (their MFMA counts
// are 1 : 2 : 2 : 4; multiples of 8, so every class has blocks on all XCDs), a block copies its class's slots to LDS once and its waves
// walk ALL m-tiles for that class (XCD-chunked, as conv3d_wlds_kernel): A fragments by ds_read_b128, the B fragments of up to four
// input positions and the skip values requested together.  Per accumulator the taps run in conv3d_kernel<kTr>'s order: bit-identical.
template <int CIN, int COUT, int NWV, int PGMAX, int PD, int PH>
__device__ __forceinline__ void convtr_cls_body(const ConvParams& p, float* wsm, unsigned cls_first, unsigned cls_blocks) {
  constexpr int KPL = 4, CK = 16, NCH = CIN / CK, ROWS = 2 * COUT, NT = (ROWS + 15) / 16;
  constexpr int SLOTF = NCH * NT * 64 * KPL;             // floats per tap slot
  constexpr int NKH = 1 + PH, NCOMB = (1 + PD) * NKH, NPOS = 2 * NCOMB;
  constexpr int PG = (NPOS < PGMAX) ? NPOS : PGMAX;      // positions fetched together (16 registers each at 64 input channels)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, n16 = lane & 15;
  {   // the class's slots, in tap order: LDS slot (c, ow) = packed slot (kd*3 + kh)*2 + ow
#pragma unroll
    for (int c = 0; c < NCOMB; ++c) {
      const int jd = c / NKH, jh = c % NKH;
      const int kd = PD ? 2 * jd : 1, kh = PH ? 2 * jh : 1;
      const float4* src = reinterpret_cast<const float4*>(p.wpack + (size_t)((kd * 3 + kh) * 2) * SLOTF);
      float4* dst = reinterpret_cast<float4*>(wsm + (size_t)(c * 2) * SLOTF);
      for (int i = threadIdx.x; i < 2 * SLOTF / 4; i += NWV * 64) dst[i] = src[i];
    }
  }
  __syncthreads();
  const float* xq = p.x + KPL * q;
  const float* wl = wsm + lane * KPL;
  const unsigned bx = (blockIdx.x - cls_first) >> 3, nbx = cls_blocks >> 3;
  const mdf::XcdChunk chunk = mdf::xcd_chunk(blockIdx.x, p.nblk);        // (p.nblk = m-tiles)
  for (unsigned l = (unsigned)wave * nbx + bx; l < chunk.len; l += (unsigned)NWV * nbx) {
    long long m = (long long)(chunk.start + l) * 16 + n16;
    const bool live = m < p.m_total;
    if (!live) m = p.m_total - 1;
    const Voxel v = split_voxel(m, p.Di, p.Hi, p.Wi);
    const unsigned vmask = next_mask(live, v, p.Di, p.Hi, p.Wi);
    const int in_off = (int)((((long long)v.b * p.Di + v.d) * p.Hi + v.h) * p.Wi + v.w) * CIN;
    const long long out_vox = (((long long)v.b * p.Do + 2 * v.d + PD) * p.Ho + 2 * v.h + PH) * p.Wo + 2 * v.w;
    const bool no_next_plane = p.kd_skip && !__any((int)(vmask & 1u));
    float4 ep_res[NT];
    if (p.res) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int r0 = nt * 16 + 4 * q;
        ep_res[nt] = (r0 < ROWS && live) ? *reinterpret_cast<const float4*>(p.res + (size_t)(out_vox + r0 / COUT) * COUT + r0 % COUT)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    Frag<KPL> bfa[PG][NCH];
#pragma unroll
    for (int pos = 0; pos < NPOS; ++pos) {     // pos = c*2 + ow: conv3d_kernel<kTr>'s tap order
      if (pos % PG == 0) {
#pragma unroll
        for (int p2 = pos; p2 < pos + PG && p2 < NPOS; ++p2) {
          const int c2 = p2 >> 1, ow2 = p2 & 1, jd2 = c2 / NKH, jh2 = c2 % NKH;
          const int od2 = (PD && jd2 == 0) ? 1 : 0, oh2 = (PH && jh2 == 0) ? 1 : 0;
          const unsigned need2 = 8u | (od2 ? 1u : 0u) | (oh2 ? 2u : 0u) | (ow2 ? 4u : 0u);
          const int tapoff2 = ((od2 * p.Hi + oh2) * p.Wi + ow2) * CIN;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) bfa[p2 - pos][ch].load(xq + in_off + (((vmask & need2) == need2) ? tapoff2 : 0) + ch * CK);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      const int c = pos >> 1, ow = pos & 1, jd = c / NKH, jh = c % NKH;
      const int od = (PD && jd == 0) ? 1 : 0, oh = (PH && jh == 0) ? 1 : 0;
      const unsigned need = 8u | (od ? 1u : 0u) | (oh ? 2u : 0u) | (ow ? 4u : 0u);
      if (od == 1 && no_next_plane) continue;       // shallow volumes: no voxel of the wave has plane d + 1 (conv3d_kernel: kd_skip)
      const float okf = ((vmask & need) == need) ? 1.0f : 0.0f;
      const float* wt = wl + pos * SLOTF;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        Frag<KPL> bf = bfa[pos % PG][ch];
        bf.scale(okf);                             // (zeroed at use: the group's loads are still in flight where they are issued)
        Frag<KPL> af[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) af[nt].load(wt + (ch * NT + nt) * (64 * KPL));
#pragma unroll
        for (int s = 0; s < KPL; ++s)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            if (ow == 1 && (nt + 1) * 16 <= COUT) continue;   // offset +1 feeds parity pw = 1 only
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[nt].v[s], bf.v[s], acc[nt], 0, 0, 0);
          }
      }
    }
    if (!live) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int r0 = nt * 16 + 4 * q;
      if (r0 >= ROWS) continue;
      const int pw_out = r0 / COUT, c0 = r0 % COUT;
      float4 al, be;
      fetch_scale_shift(p, true, c0, al, be);
      float4 o = scale_shift_relu(acc[nt], al, be, p.relu);
      add_res_store<true>(p, (size_t)(out_vox + pw_out) * COUT + c0, o, ep_res[nt]);      // (the skip values were requested ahead of the MFMAs)
    }
  }
}

template <int CIN, int COUT, int NWV, int PGMAX>
__global__ __launch_bounds__(NWV * 64) void convtr_cls_kernel(const ConvParams p) {
  extern __shared__ float wsm[];
  const unsigned bid = blockIdx.x;       // grid = 256 blocks
  if (bid < 32u) convtr_cls_body<CIN, COUT, NWV, PGMAX, 0, 0>(p, wsm, 0u, 32u);
  else if (bid < 88u) convtr_cls_body<CIN, COUT, NWV, PGMAX, 0, 1>(p, wsm, 32u, 56u);
  else if (bid < 144u) convtr_cls_body<CIN, COUT, NWV, PGMAX, 1, 0>(p, wsm, 88u, 56u);
  else convtr_cls_body<CIN, COUT, NWV, PGMAX, 1, 1>(p, wsm, 144u, 112u);
}

template <int CIN, int COUT, int NWV, int PGMAX>
int launch_convtr_cls(ConvParams& p, hipStream_t st) {
  constexpr int NCH = CIN / 16, NT = (2 * COUT + 15) / 16;
  constexpr size_t kLds = (size_t)8 * NCH * NT * 64 * 4 * sizeof(float);      // the (1, 1) class: 8 slots
  static_assert(kLds <= 160 * 1024, "a class's tap slots must fit LDS");
  return launch_lds_weights<&convtr_cls_kernel<CIN, COUT, NWV, PGMAX>>(p, (unsigned)((p.m_total + 15) / 16) /* m-tiles */, NWV * 64, kLds, st,
                                                                       "convtr_cls_kernel");
}

template <int CIN, int COUT, int MT, int NWV>
int launch_convtr_all_wl(ConvParams& p, hipStream_t st) {
  constexpr int KPL = (CIN >= 16) ? 4 : 2, NCH = CIN / (4 * KPL), NTA = (2 * COUT + 15) / 16;
  constexpr size_t kLds = (size_t)18 * NCH * NTA * 64 * KPL * sizeof(float);
  static_assert(kLds <= 160 * 1024, "the packed weight set must fit LDS");
  return launch_lds_weights<&convtr_all_kernel<CIN, COUT, MT, 1, NWV>>(p, (unsigned)((p.m_total + MT * 16 - 1) / (MT * 16)) /* wave tiles */,
                                                                       NWV * 64, kLds, st, "convtr_all_kernel");
}

template <int CIN, int COUT, int MT, int NS = 1>
int launch_convtr_all(ConvParams& p, hipStream_t st) {
  p.nblk = (unsigned)((p.m_total + 4LL * MT * 16 - 1) / (4LL * MT * 16));
  hipLaunchKernelGGL((convtr_all_kernel<CIN, COUT, MT, NS, 0>), dim3(p.nblk, NS), dim3(256), 0, st, p);
  return mdf::check_launch("convtr_all_kernel");
}

}  // namespace

// Internal entry (conv_dispatch.h) used by conv3d_entry for the transposed layers of the eval path; where no rule below takes the layer the caller goes on to conv3d_kernel<kTr>.
int mdf_convtr3d_dispatch(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res, float* y, int B,
                          int Di, int Hi, int Wi, int Cin, int Cout, int relu, int kd_skip, void* stream) {
  ConvParams p = conv_params(x, wpack, alpha, beta, res, y, B, Di, Hi, Wi, kTr, relu, kd_skip, nullptr);
  // large transposed layers: all four parity classes per tile (convtr_all_kernel)
  const long long tr_min = mdf::env_int("MDF_CONVTR_ALL_MIN_VOXELS", 40000);   // dev A/B (read per call); -1 = never  (r05: 100000 -> 40000, 32->16 @2x148x200 36.7 -> 30.2 us, @6x74x100 29.2 -> 24.7)
  const int ns = mdf::env_int("MDF_CONVTR_NS", 0);   // dev A/B and the equality test (read per call): 0 = the rule, 1 = off
  // one class per persistent block with the class's slots in LDS (convtr_cls_kernel; r05: @12x37x50 42.6 -> 32.9 us, @3x37x50 19.0 -> 14.4;
  // a single-plane volume halves the work of the pd = 1 classes and with it the block shares: @1x74x100 15.3 -> 16.6, so that one stays)
  const int tcl = mdf::env_int("MDF_CONVTR_CLS", -1);   // dev A/B and the equality test (read per call): 0 = off
  if (tr_min >= 0 && Cin == 64 && Cout == 32 && ns == 0) {
    if (tcl == 1) return launch_convtr_cls<64, 32, 12, 4>(p, (hipStream_t)stream);
    if (tcl == 2 || (tcl < 0 && Di >= 2)) return launch_convtr_cls<64, 32, 16, 2>(p, (hipStream_t)stream);
  }
  if (tr_min >= 0 && p.m_total >= tr_min && !(Cin == 64 && Cout == 32 && ns > 1)) {
    // One 16-voxel m-tile per wave (r05; two until then): these layers' time is MFMA time PLUS streaming time (skip + output), and the
    // smaller accumulator set lets 4-5 waves per SIMD instead of 3-4 overlap one block's streaming with another's MFMAs:
    // 32->16 @24x74x100 89.2 -> 69.3 us, 16->8 @12x148x200 51.2 -> 47.4, @4x296x400 79.4 -> 74.7 (four tiles: 88 / 67 / 97)
    // LDS-weights persistent form (r05): 32->16 @24x74x100 69.5 -> 60.8 us, @2x148x200 29.9 -> 26.1, @6x74x100 24.2 -> 21.3; 16->8 @12x148x200 47.6 -> 44.9, @4x296x400 71.0 -> 59.3
    const int twl = mdf::env_int("MDF_CONVTR_WLDS", 1);   // dev A/B and the equality test (read per call): 0 = off, 2 = fewer waves / two m-tiles
    if (Cin == 16 && Cout == 8 && twl == 1) return launch_convtr_all_wl<16, 8, 1, 16>(p, (hipStream_t)stream);
    if (Cin == 16 && Cout == 8 && twl == 2) return launch_convtr_all_wl<16, 8, 2, 12>(p, (hipStream_t)stream);
    if (Cin == 32 && Cout == 16 && twl == 1) return launch_convtr_all_wl<32, 16, 1, 12>(p, (hipStream_t)stream);
    if (Cin == 32 && Cout == 16 && twl == 2) return launch_convtr_all_wl<32, 16, 1, 8>(p, (hipStream_t)stream);
    if (Cin == 16 && Cout == 8) return launch_convtr_all<16, 8, 1>(p, (hipStream_t)stream);
    if (Cin == 32 && Cout == 16) return launch_convtr_all<32, 16, 1>(p, (hipStream_t)stream);
    if (Cin == 64 && Cout == 32) return launch_convtr_all<64, 32, 1>(p, (hipStream_t)stream);
  }
  // The innermost 64 -> 32 layers (1388 / 347 / 463 m-tiles at cfg2: fewer waves than the chip has SIMDs, each with 864 MFMAs behind 27
  // weight taps): the four n-tiles of an m-tile over two or four waves
  // (r05, against conv3d_kernel<kTr>: @12x37x50 53.9 -> 40.5 us over two waves, 38.7 over four; @3x37x50 21.4 -> 16.8 over four)
  if (tr_min >= 0 && Cin == 64 && Cout == 32 && ns != 1 && (p.m_total < tr_min || ns > 1)) {
    if (ns == 2) return launch_convtr_all<64, 32, 1, 2>(p, (hipStream_t)stream);
    return launch_convtr_all<64, 32, 1, 4>(p, (hipStream_t)stream);
  }
  return MDF_EUNSUPPORTED;
}
