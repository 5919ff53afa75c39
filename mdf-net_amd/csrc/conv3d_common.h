// Device-side pieces shared by the 3-D conv kernels (conv3d.hip, convtr3d.hip) and, for the epilogue sums, by the LDS-staged
// kernels (conv_lds_common.h): the launch parameters, the operand fragments, the voxel bookkeeping of an m-tile and the fused
// epilogue.  The tap loops stay with their kernels -- each is scheduled for its own layer sizes.  Everything here has internal
// linkage: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum ConvMode { kS1 = 0, kS2 = 1, kTr = 2 };

struct ConvParams {
  const float* x;
  const float* wpack;
  const float* alpha;
  const float* beta;
  const float* res;
  float* y;
  int B, Di, Hi, Wi, Do, Ho, Wo;
  int relu;
  long long m_total;  // voxels in the M index space (per parity class for kTr)
  unsigned nblk;
  // training (ST kernels): per-channel sums of the OUTPUT ride in the epilogue -- one pass over the activations less per BatchNorm
  //   stat_mode 1: out[c] += sum y, out[C+c] += sum y^2 of the raw conv output (the layer's own batch statistics)
  //   stat_mode 2: the output is dz of the PRODUCING layer (input gradient + skip gradient): out[c] += sum dr,
  //                out[C+c] += sum dr*xhat with dr = dz*[y*a+b > 0], xhat = (y-mean)*invstd; stat_y = that layer's raw conv
  //                output (same shape as the output), stat_aux = its (a, b, mean, invstd)[C]
  int stat_mode;
  const float* stat_y;
  const float* stat_aux;
  double* stat_out;
  int stat_slices;        // slices of stat_out this launch spreads its blocks over (common.h: conv_stat_send)
  int kd_skip;            // shallow volumes (<= 3 input planes): skip the depth taps no voxel of a wave has (kd_any_of)
};

// The parameters of one launch; the launcher sets nblk (and, for the ST kernels, stat_slices).
inline ConvParams conv_params(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res, float* y, int B,
                              int Di, int Hi, int Wi, int mode, int relu, int kd_skip, const mdf::ConvStat* stat) {
  ConvParams p{};
  p.x = x; p.wpack = wpack; p.alpha = alpha; p.beta = beta; p.res = res; p.y = y;
  p.B = B; p.Di = Di; p.Hi = Hi; p.Wi = Wi; p.relu = relu;
  if (stat) { p.stat_mode = stat->mode; p.stat_y = stat->y; p.stat_aux = stat->aux; p.stat_out = stat->out; p.stat_slices = stat->nslices; }
  p.kd_skip = kd_skip;
  if (mode == kS1) { p.Do = Di; p.Ho = Hi; p.Wo = Wi; }
  else if (mode == kS2) { p.Do = (Di - 1) / 2 + 1; p.Ho = (Hi - 1) / 2 + 1; p.Wo = (Wi - 1) / 2 + 1; }
  else { p.Do = 2 * Di; p.Ho = 2 * Hi; p.Wo = 2 * Wi; }
  p.m_total = (mode == kTr) ? (long long)B * Di * Hi * Wi : (long long)B * p.Do * p.Ho * p.Wo;
  return p;
}

// The persistent weights-in-LDS launch (conv3d_wlds_kernel, convtr_all_kernel<WL>, convtr_cls_kernel): 256 blocks, one per CU,
// that walk nblk tiles with the weight set in `lds` bytes of dynamic LDS.
template <auto KERN>
int launch_lds_weights(ConvParams& p, unsigned nblk, int threads, size_t lds, hipStream_t st, const char* name) {
  if (int rc = mdf::ensure_dynamic_lds<KERN>(lds)) return rc;
  p.nblk = nblk;
  hipLaunchKernelGGL(KERN, dim3(256), dim3(threads), lds, st, p);
  return mdf::check_launch(name);
}

// fp64 LDS add (ds_add_f64) / the DPP sum over the 16 lanes of an MFMA column group (lanes q*16 .. q*16+15 hold the 16
// voxels of one m-tile for the same 4 output channels)
__device__ __forceinline__ void lds_add_f64(double* p, double v) { atomicAdd(p, v); }
template <int CTRL>
__device__ __forceinline__ float dpp_mov_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov_f<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov_f<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov_f<0x141>(v);   // row_half_mirror
  v += dpp_mov_f<0x140>(v);   // row_mirror
  return v;
}

template <int KPL>
struct Frag;
template <>
struct Frag<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void zero() { v[0] = v[1] = v[2] = v[3] = 0.f; }
  __device__ __forceinline__ void scale(float m) { v[0] *= m; v[1] *= m; v[2] *= m; v[3] *= m; }
};
template <>
struct Frag<2> {
  float v[2];
  __device__ __forceinline__ void load(const float* p) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  }
  __device__ __forceinline__ void zero() { v[0] = v[1] = 0.f; }
  __device__ __forceinline__ void scale(float m) { v[0] *= m; v[1] *= m; }
};

// Voxel m of an index space [B][Md][Mh][Mw] -> (b, d, h, w).
// (m < 2^31: the entry bounds the volume to 32-bit offsets.  32-bit divisions: the 64-bit ones were ~240 vector instructions per
//  m-tile in front of the 100-400 MFMAs of a block -- a quarter of the run time of the small-volume launches, r05)
struct Voxel { int b, d, h, w; };
__device__ __forceinline__ Voxel split_voxel(long long m, int Md, int Mh, int Mw) {
  const unsigned mu = (unsigned)m, r1 = mu / (unsigned)Mw, r2 = r1 / (unsigned)Mh;
  const int mw = (int)(mu - r1 * (unsigned)Mw), mh = (int)(r1 - r2 * (unsigned)Mh);
  const int b = (int)(r2 / (unsigned)Md), md = (int)(r2 - (unsigned)b * (unsigned)Md);
  return Voxel{b, md, mh, mw};
}

// Tap validity of the 3x3x3 stride-1 / stride-2 kernels around base input voxel (bd, bh, bw): bits 0-2 kd valid, 3-5 kh valid,
// 6-8 kw valid; tap k reads offset k - 1.  TR (conv3d_kernel<kTr>): the same nine slots, slot 0 <-> offset +1, slots 1, 2 <-> offset 0.
template <bool TR = false>
__device__ __forceinline__ unsigned tap_mask(int bd, int bh, int bw, int Di, int Hi, int Wi) {
  unsigned vm = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int o = TR ? ((k == 0) ? 1 : 0) : k - 1;
    if (bd + o >= 0 && bd + o < Di) vm |= 1u << k;
    if (bh + o >= 0 && bh + o < Hi) vm |= 8u << k;
    if (bw + o >= 0 && bw + o < Wi) vm |= 64u << k;
  }
  return vm;
}

// The "+1 neighbour" mask of the transposed kernels that walk input positions: bit 0: d+1 inside, bit 1: h+1 inside, bit 2: w+1
// inside, bit 3: live (0 altogether for a lane past the last voxel).
__device__ __forceinline__ unsigned next_mask(bool live, const Voxel& v, int Di, int Hi, int Wi) {
  return live ? (8u | (v.d + 1 < Di ? 1u : 0u) | (v.h + 1 < Hi ? 2u : 0u) | (v.w + 1 < Wi ? 4u : 0u)) : 0u;
}

// Depth taps that ANY voxel of the wave's tiles has (bit kd), wave-uniform: see conv3d_kernel.
template <int MT>
__device__ __forceinline__ unsigned kd_any_of(const unsigned (&vmask)[MT]) {
  unsigned m_or = 0u;
#pragma unroll
  for (int t = 0; t < MT; ++t) m_or |= vmask[t];
  const unsigned kd_any = (__any((int)(m_or & 1u)) ? 1u : 0u) | (__any((int)(m_or & 2u)) ? 2u : 0u) | (__any((int)(m_or & 4u)) ? 4u : 0u);
  return (unsigned)__builtin_amdgcn_readfirstlane((int)kd_any);
}

// ---- epilogue:  y = [res +] [relu]( acc * alpha + beta )  for the lane's 4 channels c0.. of one voxel -------------------------------
// alpha / beta of channels c0..c0+3 (1 / 0 without folded BatchNorm, or for a lane whose GEMM rows do not exist)
__device__ __forceinline__ void fetch_scale_shift(const ConvParams& p, bool row_ok, int c0, float4& al, float4& be) {
  al = make_float4(1.f, 1.f, 1.f, 1.f);
  be = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row_ok && p.alpha) {
    al = *reinterpret_cast<const float4*>(p.alpha + c0);
    be = *reinterpret_cast<const float4*>(p.beta + c0);
  }
}
__device__ __forceinline__ float4 scale_shift_relu(const f32x4& acc, const float4& al, const float4& be, int relu) {
  float4 o;
  o.x = acc[0] * al.x + be.x;
  o.y = acc[1] * al.y + be.y;
  o.z = acc[2] * al.z + be.z;
  o.w = acc[3] * al.w + be.w;
  if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
  return o;
}
// PRE: the residual was requested ahead of the tap loop and arrives in `pre`; otherwise it is read here and the call names no `pre`.
// o keeps the stored value.
// (references, not values: handing the operands over by value was tried and moved registers and occupancy in a dozen
//  conv3d_kernel instantiations; this form moves none for the worse)
template <bool PRE>
__device__ __forceinline__ void add_res_store(const ConvParams& p, size_t oi, float4& o, const float4& pre = float4()) {
  if (p.res) {
    float4 rr;
    if constexpr (PRE) rr = pre;
    else rr = *reinterpret_cast<const float4*>(p.res + oi);
    o.x += rr.x; o.y += rr.y; o.z += rr.z; o.w += rr.w;
  }
  *reinterpret_cast<float4*>(p.y + oi) = o;
}

// ST epilogue (ConvParams::stat_mode): the lane's 4 output values o[] of channels c0.. at output index oi -> its running sums
// (ps, pq).  aux: the block's LDS copy of the producing layer's (a, b, mean, invstd) [4][64].  MODE 1 / 2: the caller instantiates
// the two modes separately (conv_lds_kernel) and only that mode's code exists; MODE 0: it branches on `mode` at run time (p.stat_mode).
// AUX_OFF: where the table starts behind `aux_base`, for a caller that keeps it in its dynamic LDS image (a constant the compiler
// folds into the reads here: handed over as a finished pointer, conv_lds_kernel's instruction sequence moves).
template <int MODE, int AUX_OFF = 0>
__device__ __forceinline__ void stat_accum(int mode, const float* stat_y, const float* aux_base, size_t oi, int c0, const float (&o)[4],
                                           float (&ps)[4], float (&pq)[4]) {
  if (MODE == 1 || (MODE == 0 && mode == 1)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { ps[k] += o[k]; pq[k] = fmaf(o[k], o[k], pq[k]); }
  } else {
    const float* aux = aux_base + AUX_OFF;
    const float4 yv4 = *reinterpret_cast<const float4*>(stat_y + oi);
    const float yv[4] = {yv4.x, yv4.y, yv4.z, yv4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dr = (fmaf(yv[k], aux[c0 + k], aux[64 + c0 + k]) > 0.0f) ? o[k] : 0.0f;
      ps[k] += dr;
      pq[k] = fmaf(dr, (yv[k] - aux[128 + c0 + k]) * aux[192 + c0 + k], pq[k]);
    }
  }
}
// ... and the sums of the 16 voxels of the lane's column group into the block's fp64 LDS table [2][64], TAB_OFF floats behind `base`
// (one body for a `double*` table and for a `float*` LDS image + offset: a plain-pointer overload with a forwarding
//  stat_commit<TAB_OFF>(float*) beside it was tried and moved 36 conv_lds_kernel instantiations)
template <int TAB_OFF = 0, typename T>
__device__ __forceinline__ void stat_commit(T* base, int c0, int n16, const float (&ps)[4], const float (&pq)[4]) {
  double* tab = reinterpret_cast<double*>(reinterpret_cast<float*>(base) + TAB_OFF);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float a1 = row16_sum(ps[k]), a2 = row16_sum(pq[k]);
    if (n16 == 0) { lds_add_f64(&tab[c0 + k], (double)a1); lds_add_f64(&tab[64 + c0 + k], (double)a2); }
  }
}

}  // namespace
