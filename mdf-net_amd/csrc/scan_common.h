// Block-level scans and folds as device bodies.  Every `__global__` that uses them stays in its own .hip under its own name
// (mdfnet_hip/kernel_families.py attributes time by kernel name), so this header declares none.
#pragma once
#include <hip/hip_runtime.h>

namespace mdf {

constexpr int kScanThreads = 1024;   // block of the one-block scan
constexpr int kScanBlock = 256;      // block of the per-chunk sums, scans and folds

// Hillis-Steele inclusive scan of one value per thread of an N-thread block.  part[] holds the scanned values afterwards
// (part[N - 1] = the sum); -> the calling thread's own.
template <typename T, int N>
__device__ __forceinline__ T block_inclusive_scan(T (&part)[N], T v) {
  const int t = threadIdx.x;
  part[t] = v;
  __syncthreads();
  for (int off = 1; off < N; off <<= 1) {
    const T add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  return part[t];
}

// Exclusive scan of nitems int counts into int64 offsets by one block of kScanThreads (contiguous chunks, one per thread);
// *total = the sum (nullable).  kViews: view v's total, the sum of items [v*nblk, (v+1)*nblk), goes to view_counts[v] for
// v < n (nullable).
template <typename Index, bool kViews>
__device__ __forceinline__ void block_exclusive_scan(const int* __restrict__ counts, Index nitems, long long* __restrict__ offsets,
                                                     long long* __restrict__ total, int nblk = 0, int n = 0,
                                                     int* __restrict__ view_counts = nullptr) {
  __shared__ long long part[kScanThreads];
  const int t = threadIdx.x;
  const Index chunk = (nitems + kScanThreads - 1) / kScanThreads;
  const Index lo = min(nitems, t * chunk), hi = min(nitems, lo + chunk);
  long long s = 0;
  for (Index i = lo; i < hi; ++i) s += counts[i];
  long long run = block_inclusive_scan(part, s) - s;
  for (Index i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (!kViews) {
    if (t == kScanThreads - 1 && total != nullptr) *total = part[t];
    return;
  }
  __threadfence_block();
  __syncthreads();
  const long long all = part[kScanThreads - 1];
  if (view_counts != nullptr) {
    for (int v = t; v < n; v += kScanThreads) {
      const long long a = offsets[(size_t)v * nblk], b = v + 1 < n ? offsets[(size_t)(v + 1) * nblk] : all;
      view_counts[v] = (int)(b - a);
    }
  }
  if (t == 0 && total != nullptr) *total = all;
}

// Sum of one int per thread of a kScanBlock-thread block (valid in every thread after the last barrier; thread 0 stores it).
__device__ __forceinline__ int block_sum(int v) {
  __shared__ int part[kScanBlock];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int off = kScanBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  return part[0];
}

// Inclusive scan of one int per thread of a kScanBlock-thread block.
__device__ __forceinline__ int block_inclusive_scan(int v) {
  __shared__ int part[kScanBlock];
  return block_inclusive_scan(part, v);
}

// Fold of K doubles per thread over a kScanBlock-thread block with one fixed tree (thread t takes t + s for s = 128, 64, ... 1),
// so the result depends on the values only: red[k][0] = the fold of v[k].  combine(k, a, b) -> double.
template <int K, typename Combine>
__device__ __forceinline__ void block_fold(const double (&v)[K], double (*red)[kScanBlock], Combine combine) {
  for (int k = 0; k < K; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int s = kScanBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int k = 0; k < K; ++k) red[k][threadIdx.x] = combine(k, red[k][threadIdx.x], red[k][threadIdx.x + s]);
    __syncthreads();
  }
}

}  // namespace mdf
