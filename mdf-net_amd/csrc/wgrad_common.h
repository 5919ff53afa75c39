// Shared by the weight-gradient kernels (wgrad.hip: direct and A = 1 forms, slab sums; wgrad_lds.hip: LDS-staged forms): the host
// plan of a launch and the device pieces every form ends with.  The device helpers have internal linkage.
#pragma once
#include "common.h"
#include "conv3d_common.h"      // f32x4

namespace mdf {

// What the workspace size and every launch of one layer agree on, computed in ONE place (wgrad.hip: wgrad_plan).
struct WgradPlan {
  int NA, NB, pairs;     // 16-channel tiles of `small` and `big`; pairs = NA * NB
  int split;             // waves of a block that share one pair and split its chunks (1, 2 or 4)
  int gy, gz;            // pair groups (4 waves each); z taps: 3 kd planes (3-D) or ksize kernel rows (2-D)
  int n;                 // elements of dw = of one slab: A * Bc * 27 (3-D) or A * Bc * ksize^2 (2-D)
  int gx;                // slabs the workspace holds = the most blocks along x a launch may use
};

// slices of a slab sum (blockIdx.y of slab_sum_kernel, gys of a slab_sum_batch_kernel job): >= 8 slabs per partial sum
inline int wgrad_sum_slices(int nslab) {
  const int gys = nslab / 8;
  return gys < 1 ? 1 : (gys > 32 ? 32 : gys);
}

}  // namespace mdf

// wgrad_lds.hip.  gx_io: in = slabs the workspace holds, out = blocks launched (= slabs written).  Returns MDF_EUNSUPPORTED when the
// shape has no LDS instantiation (the caller falls back to the direct kernels).
int mdf_wgrad_lds_dispatch(const mdf::WgradPlan& pl, const float* small_, const float* big, float* workspace, int* gx_io, int B, int Ds, int Hs,
                           int Ws, int A, int Bc, int stride, int ksize, int is3d, float* zero_out, void* stream);

namespace {

// partial tiles of the `split` waves that share a pair: summed through LDS (`mine`: NACC * 256 floats per pair, the sharing waves
// take turns); wave part 0 ends up with the pair's tiles.  Every wave of the block runs the same barrier sequence.
template <int NACC>
__device__ __forceinline__ void split_wave_sum(f32x4 (&acc)[NACC], float* mine, int split, int part, int lane) {
  for (int turn = 1; turn < split; ++turn) {
    if (part == turn) {
#pragma unroll
      for (int t = 0; t < NACC; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) mine[(t * 4 + i) * 64 + lane] = acc[t][i];
    }
    __syncthreads();
    if (part == 0) {
#pragma unroll
      for (int t = 0; t < NACC; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i] += mine[(t * 4 + i) * 64 + lane];
    }
    __syncthreads();
  }
}

// the NACC tap tiles of a pair -> the block's slab [A][Bc][ntaps], taps z0 .. z0 + NACC - 1 (C/D layout: lane holds rows 4q .. 4q+3 of column bcol)
template <int NACC>
__device__ __forceinline__ void store_tap_tiles(const f32x4 (&acc)[NACC], float* out, int na, int q, int bcol, int A, int Bc, int ntaps, int z0) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = na * 16 + 4 * q + i;
    if (row < A) {
      float* o = out + ((long long)row * Bc + bcol) * ntaps + z0;
#pragma unroll
      for (int t = 0; t < NACC; ++t) o[t] = acc[t][i];
    }
  }
}

}  // namespace
