// Shared host-side helpers for the C ABI (include/mdfnet_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "mdfnet_hip.h"

template <int I, int N, typename F>   // f(integral_constant<int, i>) for i in [I, N): a loop whose index is a compile-time constant in the body
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

namespace mdf {

void set_error(const char* fmt, ...);
void note_launch(const char* kernel);     // abi.cpp: the kernel the calling thread enqueued last (mdf_last_launch)
void note_wgrad_plan(int form, int R, int TH, int tv, long long n_tiles, int gx, int gy, int gz, int split);   // abi.cpp: mdf_wgrad_last_plan

inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  set_error("%s", buf);
  return code;
}

inline int check_launch(const char* what) {
  note_launch(what);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MDF_EHIP, "%s: %s", what, hipGetErrorString(e));
  return MDF_OK;
}

// Development switches (MDF_* environment variables).  A `static const` caller reads its switch once per process; every other
// caller reads it per call, because tests flip those inside one process.
inline long long env_int(const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; }   // any integer
inline long long env_pos(const char* name, long long dflt) { const long long v = env_int(name, 0); return v > 0 ? v : dflt; }   // the value counts only if > 0
inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt) != 0; }

// Bijective XCD-aware remap (cdna_hip_programming.md T1): blocks b and b+8 share an XCD, so give
// every XCD a contiguous chunk of the tile range (neighbouring tiles share source footprints / halos).
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk) {
  const unsigned q = nblk >> 3, r = nblk & 7u, x = bid & 7u;
  const unsigned base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + (bid >> 3);
}
// The same share, for persistent kernels whose waves walk it themselves: the first item and the length of the contiguous chunk of
// n items that block bid's XCD (bid & 7) owns (the first n % 8 XCDs hold one more).  xcd_remap(bid, n) = xcd_chunk(bid, n).start +
// (bid >> 3); it keeps its own lines because the kernels that call it compile to the same instructions only that way.
struct XcdChunk { unsigned start, len; };
__device__ __forceinline__ XcdChunk xcd_chunk(unsigned bid, unsigned n) {
  const unsigned x = bid & 7u, q = n >> 3, r = n & 7u;
  return XcdChunk{(x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q, q + (x < r ? 1u : 0u)};
}

// Kernels that need more than the default 64 KB of dynamic LDS: hipFuncAttributeMaxDynamicSharedMemorySize, set before the first
// launch.  The attribute is a per-DEVICE property of the function (several GPUs in one process, DataParallel-style), so there is one
// flag per device and -- KERN being a template argument -- per kernel instantiation; a device id outside the table sets it on every
// call.  Benign race: the call is idempotent.
template <auto KERN>
inline int ensure_dynamic_lds(size_t bytes) {
  static bool done_dev[64] = {};
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  bool& done = done_dev[(dev_id >= 0 && dev_id < 64) ? dev_id : 0];
  if (!done || dev_id >= 64) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(MDF_EHIP, "hipFuncSetAttribute(dynamic LDS %zu): %s", bytes, hipGetErrorString(e));
    done = true;
  }
  return MDF_OK;
}

// ATen's CPU float sum (SumKernel.cpp multi_row_sum / cascade_sum): elements are added sequentially into
// level 0; after every 16 elements level 0 is folded into level 1 (after every 256 into level 2, ...); the
// result is ((l0 + l1) + l2) + l3.  Mirroring it makes `torch.sum(a*b, dim)`-style reductions bit-identical
// to the reference's CPU result for the same inputs (verified against the goldens for D = 8, 24, 48).
// Scope of that claim: this is the order of ATen's VECTORISED outer-sum path, which covers every pixel only when the
// flattened h*w axis is a multiple of four SIMD vectors of the reference's host (32 floats with AVX2, 64 with AVX-512).
// The tail pixels of any other map go through a 4-way interleaved row sum there and differ in the last bits, so
// live torch has no single order.  Everywhere else this order IS the definition: tests/heads_mirror.py:cascade_sum
// states it, tests/test_heads_mirror_cpu.py ties it to the goldens, and other shapes are held to float64 bounds.
struct CascadeSum {
  float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
  unsigned n = 0;
  __device__ __forceinline__ void add(float v) {
    l0 += v;
    ++n;
    if ((n & 15u) == 0) {
      l1 += l0; l0 = 0.f;
      if ((n & 255u) == 0) {
        l2 += l1; l1 = 0.f;
        if ((n & 4095u) == 0) { l3 += l2; l2 = 0.f; }
      }
    }
  }
  __device__ __forceinline__ float result() const { return ((l0 + l1) + l2) + l3; }
};

// Epilogue sums of the training path (conv3d.hip / conv_lds.hip; all null / 0 for inference): see ConvParams::stat_mode (conv3d_common.h).
struct ConvStat {
  int mode;
  const float* y;
  const float* aux;
  double* out;
  int group_imgs;      // 2-D: images per BatchNorm group (the tensor is [groups][imgs][H][W][C]); 0 = one group
  int nslices;         // the sums are spread over this many copies ("slices") of [groups][2C]; the consumers add them up
};

// Sending a block's sums to memory costs 2C fp64 atomics on the SAME 2C addresses for every block, and same-address atomics
// retire one per ~11 ns (rocprof, r03: a 2592-block launch paid 28 us for them -- more than its MFMA work).  A two-level
// scheme with per-slice counters (last arriver collapses the slice) was built and is far worse: its release fence writes the
// L2 back per block (24 -> 120 us).  So: block b adds into slice b % R of out[R][groups][2C] (contention / R, no ordering
// needed) and the BatchNorm kernels that consume the sums add the R slices up (16 x 32 B per thread, L2 hits).
inline int conv_stat_slices(long long blocks_per_group, int nslices) {
  long long r = (blocks_per_group + 47) / 48;          // <= ~48 blocks per address
  if (r > nslices) r = nslices;
  return (int)(r < 1 ? 1 : r);
}
// tab: the block's LDS table [2][64] (sum, sum2).  out: slice 0 of this block's group; consecutive slices are slice_stride apart.
template <int COUT>
__device__ __forceinline__ void conv_stat_send(const double* tab, double* out, long long slice_stride, int R, unsigned local_blk) {
  const int tid = threadIdx.x;
  if (tid < 2 * COUT) {
    const int c = tid % COUT, which = tid / COUT;
    const double v = tab[which * 64 + c];
    if (v != 0.0) atomicAdd(&out[(size_t)(local_blk % (unsigned)R) * slice_stride + which * COUT + c], v);
  }
}

}  // namespace mdf

#define MDF_REQUIRE(cond, ...) \
  do {                         \
    if (!(cond)) return mdf::fail(MDF_EARG, __VA_ARGS__); \
  } while (0)

namespace mdf {
// the epilogue-sum arguments of the training entries (mdf_conv2d_train_fwd, mdf_conv3d_train_fwd)
inline int check_stat(int stat_mode, const float* stat_y, const float* stat_aux, const double* stat_out, int nslices, int Cout) {
  MDF_REQUIRE(stat_mode == 1 || stat_mode == 2, "stat_mode=%d not in {1 (sum y, sum y^2), 2 (BatchNorm-backward sums)}", stat_mode);
  MDF_REQUIRE(stat_out, "stat_out is null");
  MDF_REQUIRE(nslices >= 1 && nslices <= 64, "nslices=%d out of range [1,64]", nslices);
  MDF_REQUIRE(stat_mode == 1 || (stat_y && stat_aux), "stat_mode 2 needs stat_y and stat_aux");
  MDF_REQUIRE(Cout % 4 == 0 && Cout >= 8 && Cout <= 64, "epilogue sums are built for Cout in {8,..,64}, Cout %% 4 == 0 (got %d)", Cout);
  return MDF_OK;
}
}  // namespace mdf
