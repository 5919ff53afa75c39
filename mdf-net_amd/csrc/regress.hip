// Per-pixel heads between the stages: soft-argmin depth regression (net/unit/regress.py:5-7),
// photometric confidence (regress.py:9-25) and the curve-fit hypothesis generator
// (net/unit/depthhypos.py:27-215).  All are HBM-bound streaming kernels: one thread per
// pixel, the D axis walked with stride h*w so every load of a wavefront is one coalesced 256-B row.
// The reference builds [B,h,w,D,3] temporaries and a batched 3x3 inverse for the gauss fit; here the
// fit is a dot product with a host-prepared row (hypotheses are shared by all pixels at that stage); gauss0 and gauss1 with
// per-pixel hypotheses are centred fits in registers (hypos_curve_fit_kernel).
#include "common.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float hyp_at(const float* __restrict__ hypos, int per_pixel, size_t b, int D, int d, size_t hw,
                                        size_t pix) {
  return per_pixel ? hypos[(b * D + d) * hw + pix] : hypos[b * D + d];
}

__global__ void depth_regress_kernel(const float* __restrict__ prob, const float* __restrict__ hypos, int per_pixel,
                                     float* __restrict__ depth, int B, int D, int hw) {
  const size_t n = (size_t)B * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw, pix = i % hw;
    mdf::CascadeSum acc;  // torch.sum(prob * hypos, 1): product tensor, then ATen's cascade sum
    for (int d = 0; d < D; ++d) acc.add(prob[(b * D + d) * hw + pix] * hyp_at(hypos, per_pixel, b, D, d, hw, pix));
    depth[i] = acc.result();
  }
}

// conf = sum prob[idx-1 .. idx+2], idx = trunc(sum_d prob_d * d)   (n=4, pad=(1,2))
__global__ void confidence_kernel(const float* __restrict__ prob, float* __restrict__ conf, int64_t* __restrict__ idx_out,
                                  int B, int D, int hw) {
  const size_t n = (size_t)B * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw, pix = i % hw;
    const float* p = prob + b * D * hw + pix;
    mdf::CascadeSum ex;
    for (int d = 0; d < D; ++d) ex.add(p[(size_t)d * hw] * (float)d);
    long long idx = (long long)ex.result();  // .long() truncates toward zero
    if (idx_out) idx_out[i] = idx;
    idx = idx < 0 ? 0 : (idx > D - 1 ? D - 1 : idx);  // torch.gather would raise outside [0,D-1]; prob sums to 1 so never hit
    float s = 0.0f;
    for (int k = (int)idx - 1; k <= (int)idx + 2; ++k) s += (k >= 0 && k < D) ? p[(size_t)k * hw] : 0.0f;
    conf[i] = s;
  }
}

// the same with the nearest-neighbour x2 upsampling of core.py:76 (F.interpolate(conf, scale_factor=2, mode="nearest")) folded in:
// every value goes to its 2x2 output pixels
template <int DT>   // D at compile time (8: the model's last stage) or 0: the plane loads leave together and the window sum reads registers
__global__ void confidence_up2_kernel(const float* __restrict__ prob, float* __restrict__ conf2, int B, int D_rt, int h, int w) {
  const int D = DT ? DT : D_rt;
  const int hw = h * w;
  const size_t n = (size_t)B * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw, pix = i % hw;
    const float* p = prob + b * D * hw + pix;
    mdf::CascadeSum ex;
    float s = 0.0f;
    if constexpr (DT != 0) {
      float pv[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) pv[d] = p[(size_t)d * hw];
#pragma unroll
      for (int d = 0; d < DT; ++d) ex.add(pv[d] * (float)d);
      long long idx = (long long)ex.result();
      idx = idx < 0 ? 0 : (idx > D - 1 ? D - 1 : idx);
      // the same four terms in the same order (k = idx-1 .. idx+2), selected from the registers
      for (int k = (int)idx - 1; k <= (int)idx + 2; ++k) {
        float v = 0.0f;
#pragma unroll
        for (int d = 0; d < DT; ++d) v = (d == k) ? pv[d] : v;
        s += v;
      }
    } else {
      for (int d = 0; d < D; ++d) ex.add(p[(size_t)d * hw] * (float)d);
      long long idx = (long long)ex.result();
      idx = idx < 0 ? 0 : (idx > D - 1 ? D - 1 : idx);
      for (int k = (int)idx - 1; k <= (int)idx + 2; ++k) s += (k >= 0 && k < D) ? p[(size_t)k * hw] : 0.0f;
    }
    const int y = (int)(pix / w), x = (int)(pix % w);
    float* o = conf2 + (b * 2 * h + 2 * y) * (size_t)(2 * w) + 2 * x;
    *reinterpret_cast<float2*>(o) = make_float2(s, s);
    *reinterpret_cast<float2*>(o + 2 * w) = make_float2(s, s);
  }
}

// ATen upsample_bicubic2d, align_corners=False, scale 2, A = -0.75: src = 0.5*(o+0.5)-0.5 = o/2 - 0.25, NOT clamped at 0, so the
// fraction is 0.75 at every even o (taps k-2 .. k+1, o = 2k) and 0.25 at every odd o (taps k-1 .. k+2, o = 2k+1): one weight
// quadruple, read forwards or backwards.  All four are exact in fp32.  Tap indices are clamped to [0, n_in-1].
__device__ __forceinline__ void bicubic2_taps(int o, int n_in, int (&idx)[4], float (&c)[4]) {
  constexpr float kW[4] = {-0.03515625f, 0.26171875f, 0.87890625f, -0.10546875f};
  const int odd = o & 1, first = (o >> 1) - 2 + odd;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = first + j;
    idx[j] = t < 0 ? 0 : (t > n_in - 1 ? n_in - 1 : t);
    c[j] = odd ? kW[3 - j] : kW[j];
  }
}

// confidence_regress(prob, last_confidence) of regress.py:9-25 with any window the reference's signature carries:
//   cur  = sum prob[idx-pf .. idx-pf+nwin-1] (0 outside [0,D), ascending, from 0.0f), idx as in confidence_kernel;
//   conf = w_last * bicubic_x2(last) + w_cur * cur       (last [B,h/2,w/2]; null: conf = cur, the bits of the kernels above
//          at nwin = 4, pf = 1).
// Fixed order, every product and sum rounded on its own (-ffp-contract=off, no fma): per tap row ((p0*c0 + p1*c1) + p2*c2) + p3*c3
// along x, the same form along y over the four row results, then the blend.  up2: every value goes to its 2x2 pixels of
// [B,2h,2w] (the nearest x2 of core.py:76), as in confidence_up2_kernel.  The 16 taps of `last` come through the caches: that
// map is a quarter of this stage's size and neighbouring lanes share their taps.
template <int DT>   // D at compile time (48 / 24 / 8: the model's stages; the plane loads leave together, see hypos_fit_kernel) or 0
__global__ __launch_bounds__(kThreads) void confidence_cascade_kernel(const float* __restrict__ prob, const float* __restrict__ last,
                                                                      float w_last, float w_cur, int nwin, int pf, int up2,
                                                                      float* __restrict__ conf, int B, int D_rt, int h, int w) {
  const int D = DT ? DT : D_rt;
  const int hw = h * w;
  const size_t n = (size_t)B * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw, pix = i % hw;
    const int y = (int)(pix / w), x = (int)(pix % w);
    const float* p = prob + b * D * hw + pix;
    mdf::CascadeSum ex;
    float s = 0.0f;
    if constexpr (DT != 0) {
      float pv[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) pv[d] = p[(size_t)d * hw];
#pragma unroll
      for (int d = 0; d < DT; ++d) ex.add(pv[d] * (float)d);
      long long idx = (long long)ex.result();
      idx = idx < 0 ? 0 : (idx > D - 1 ? D - 1 : idx);
      for (int k = (int)idx - pf; k < (int)idx - pf + nwin; ++k) {
        float v = 0.0f;
#pragma unroll
        for (int d = 0; d < DT; ++d) v = (d == k) ? pv[d] : v;
        s += v;
      }
    } else {
      for (int d = 0; d < D; ++d) ex.add(p[(size_t)d * hw] * (float)d);
      long long idx = (long long)ex.result();
      idx = idx < 0 ? 0 : (idx > D - 1 ? D - 1 : idx);
      for (int k = (int)idx - pf; k < (int)idx - pf + nwin; ++k) s += (k >= 0 && k < D) ? p[(size_t)k * hw] : 0.0f;
    }
    if (last) {
      const int hl = h >> 1, wl = w >> 1;
      const float* m = last + b * hl * wl;
      int yi[4], xi[4];
      float cy[4], cx[4], row[4];
      bicubic2_taps(y, hl, yi, cy);
      bicubic2_taps(x, wl, xi, cx);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* mr = m + (size_t)yi[r] * wl;
        row[r] = ((mr[xi[0]] * cx[0] + mr[xi[1]] * cx[1]) + mr[xi[2]] * cx[2]) + mr[xi[3]] * cx[3];
      }
      const float up = ((row[0] * cy[0] + row[1] * cy[1]) + row[2] * cy[2]) + row[3] * cy[3];
      s = w_last * up + w_cur * s;
    }
    if (up2) {
      float* o = conf + (b * 2 * h + 2 * y) * (size_t)(2 * w) + 2 * x;
      *reinterpret_cast<float2*>(o) = make_float2(s, s);
      *reinterpret_cast<float2*>(o + 2 * w) = make_float2(s, s);
    } else {
      conf[i] = s;
    }
  }
}

// Range mapping around the refinement net (refine.py:29,44), one launch each instead of two or three ATen ones; the separate
// roundings of torch's op sequence are kept: mode 0: y = (x - lo[b]) / span[b];  mode 1: y = lo[b] + x * span[b]
__global__ void range_affine_kernel(const float* __restrict__ x, const float* __restrict__ lo, const float* __restrict__ span, int mode,
                                    float* __restrict__ y, int B, size_t n) {
  const size_t total = (size_t)B * n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / n;
    const float l = lo[b], sp = span[b], v = x[i];
    y[i] = (mode == 0) ? __fdiv_rn(__fsub_rn(v, l), sp) : __fadd_rn(l, __fmul_rn(v, sp));
  }
}

// mode 1: s = |-1 / sum_d row[b,d] * ln(max(p,1e-40))|          depthhypos.py:194-212
// mode 2: s = 1 / |sum(x*y)/sum(x*x)|, x = |hyp - depth|          depthhypos.py:116-123
// DT = D at compile time (48 / 24 / 8: the model's stages) or 0: with a runtime trip count the compiler issues the plane loads a few at
// a time and a thread waits out D / 4 memory round trips in a launch that has one wave per SIMD; unrolled, they leave together.  The
// arithmetic and its order are the same.
template <int DT>
__global__ void hypos_fit_kernel(int mode, const float* __restrict__ prob, const float* __restrict__ depth,
                                 const float* __restrict__ hypos, int per_pixel, const float* __restrict__ row,
                                 float* __restrict__ s_out, int B, int D_rt, int hw) {
  const int D = DT ? DT : D_rt;
  const size_t n = (size_t)B * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw, pix = i % hw;
    const float* p = prob + b * D * hw + pix;
    if (mode == 1) {
      // b0 = row . ln(p): torch.matmul([.,3,D] @ [.,D,1]) runs ATen's naive bmm kernel (contraction*rows*cols
      // < 400): sequential k loop, separate multiply and add in fp32.  The sum cancels heavily, so mirroring
      // the order (verified bit-exact on the goldens given torch's log) matters more than accuracy here.
      float acc = 0.0f;
      if constexpr (DT != 0) {
        float pv[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) pv[d] = p[(size_t)d * hw];
#pragma unroll
        for (int d = 0; d < DT; ++d) acc = acc + row[b * D + d] * logf(fmaxf(pv[d], 1e-40f));
      } else {
        for (int d = 0; d < D; ++d) acc = acc + row[b * D + d] * logf(fmaxf(p[(size_t)d * hw], 1e-40f));
      }
      s_out[i] = fabsf(-1.0f / acc);
    } else {
      const float dep = depth[i];
      mdf::CascadeSum sxy, sxx;  // torch.sum(x*y, -1), torch.sum(x*x, -1)
      if constexpr (DT != 0) {
        float pv[DT], hv[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) { pv[d] = p[(size_t)d * hw]; hv[d] = hyp_at(hypos, per_pixel, b, D, d, hw, pix); }
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const float x = fabsf(hv[d] - dep);
          const float y = logf(fmaxf(pv[d], 1e-40f));
          sxy.add(x * y);
          sxx.add(x * x);
        }
      } else {
        for (int d = 0; d < D; ++d) {
          const float x = fabsf(hyp_at(hypos, per_pixel, b, D, d, hw, pix) - dep);
          const float y = logf(fmaxf(p[(size_t)d * hw], 1e-40f));
          sxy.add(x * y);
          sxx.add(x * x);
        }
      }
      s_out[i] = 1.0f / fabsf(sxy.result() / sxx.result());
    }
  }
}

// ---- modes 3 and 4: the gauss0 fit and the gauss1 fit with hypotheses of either form (depthhypos.py:127-166, 169-215) ----
// The reference inverts the normal matrix of the uncentred regressors per pixel; with hypotheses near 600 and a spread of
// millimetres its fp32 result is noise (gauss1: median relative error 0.48 against its own code in float64).  These two modes
// therefore do not mirror its bits: they compute the same least-squares slope from centred regressors, and are held to the
// reference's code in float64 (tests/hypos_oracle.py has the operation order restated and the rounding count).
//
// Every sum runs in four interleaved accumulators: a dependent chain of D / 4 instead of D (one wave per SIMD: nothing else hides
// the latency) and as many fewer roundings.  d & 3 is a constant in the unrolled forms.
struct Sum4 {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  __device__ __forceinline__ void fma(int d, float x, float y) {   // += x * y; add: y = 1 is exact
    switch (d & 3) {
      case 0: a0 = __fmaf_rn(x, y, a0); break;
      case 1: a1 = __fmaf_rn(x, y, a1); break;
      case 2: a2 = __fmaf_rn(x, y, a2); break;
      default: a3 = __fmaf_rn(x, y, a3); break;
    }
  }
  __device__ __forceinline__ void add(int d, float v) { fma(d, v, 1.0f); }
  __device__ __forceinline__ float result() const { return (a0 + a1) + (a2 + a3); }
};

template <int DT> constexpr int kUnrollD = DT ? DT : 1;   // the register forms unroll fully, the generic form not at all

// Mean, then corrected by the mean of the residuals: what is left is the rounding of the last addition, and D equal values give
// exactly that value (the residuals are a rounding error of it, far below half an ulp), so a degenerate pixel centres to exact zeros.
template <int DT, class V>
__device__ __forceinline__ float mean_corrected(int D_rt, V v) {
  const int D = DT ? DT : D_rt;
  Sum4 s, r;
#pragma unroll kUnrollD<DT>
  for (int d = 0; d < D; ++d) s.add(d, v(d));
  const float m1 = s.result() / (float)D;
#pragma unroll kUnrollD<DT>
  for (int d = 0; d < D; ++d) r.add(d, v(d) - m1);
  return m1 + r.result() / (float)D;
}

// mode 3: z = b0 u + b1 with u = (x - depth)^2;  b0 = sum (u - mean u) z / sum (u - mean u)^2;  s = |-1 / b0| = |den / num|.
// Fewer than two distinct u: every centred u is an exact zero and s = 0/0 = NaN (the reference's torch.inverse raises there).
template <int DT, class U, class Z>
__device__ __forceinline__ float gauss0_fit(int D_rt, U u, Z z) {
  const int D = DT ? DT : D_rt;
  const float um = mean_corrected<DT>(D_rt, u);
  Sum4 num, den;
#pragma unroll kUnrollD<DT>
  for (int d = 0; d < D; ++d) {
    const float c = u(d) - um;
    num.fma(d, c, z(d));
    den.fma(d, c, c);
  }
  return fabsf(den.result() / num.result());
}

// mode 4: z = b0 x^2 + b1 x + b2.  b0 does not change under a shift of x and scales by sigma^2 under x -> x / sigma, so the fit runs
// in t = (x - mean x) * 2^-k, 2^k the power of two above max |x - mean x| (an exact scaling, |t| < 1), with the quadratic
// orthogonalised against 1 and t: q = t^2 - alpha t - beta, (alpha, beta) from the 2x2 system in n, sum t, sum t^2, sum t^3;
// b0 = sum q z / sum q^2 * 2^-2k;  s = |-1 / b0|.
// Fewer than three distinct hypotheses (every x is the pixel's smallest or largest): q is identically zero there, rounding would
// leave noise in its place, so both sums are set to that zero and s = 0/0 = NaN (the reference's torch.inverse raises there).
template <int DT, class X, class Z>
__device__ __forceinline__ float gauss1_fit(int D_rt, X x, Z z) {
  const int D = DT ? DT : D_rt;
  const float xm = mean_corrected<DT>(D_rt, x);
  float lo = x(0), hi = lo, sig = 0.0f;
#pragma unroll kUnrollD<DT>
  for (int d = 0; d < D; ++d) {
    const float v = x(d);
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
    sig = fmaxf(sig, fabsf(v - xm));
  }
  bool three = false;
#pragma unroll kUnrollD<DT>
  for (int d = 0; d < D; ++d) three = three || (x(d) != lo && x(d) != hi);
  int k;
  frexpf(sig, &k);
  Sum4 m1, m2, m3;
#pragma unroll kUnrollD<DT>
  for (int d = 0; d < D; ++d) {
    const float t = ldexpf(x(d) - xm, -k), w = t * t;
    m1.add(d, t);
    m2.add(d, w);
    m3.fma(d, w, t);
  }
  const float n = (float)D, s1 = m1.result(), s2 = m2.result(), s3 = m3.result();
  const float det = __fmaf_rn(n, s2, -(s1 * s1));
  const float alpha = __fmaf_rn(n, s3, -(s1 * s2)) / det;
  const float beta = __fmaf_rn(s2, s2, -(s1 * s3)) / det;
  Sum4 num, den;
#pragma unroll kUnrollD<DT>
  for (int d = 0; d < D; ++d) {
    const float t = ldexpf(x(d) - xm, -k);
    const float q = __fmaf_rn(t, t - alpha, -beta);
    num.fma(d, q, z(d));
    den.fma(d, q, q);
  }
  const float nu = three ? num.result() : 0.0f, de = three ? den.result() : 0.0f;
  return fabsf(ldexpf(de / nu, 2 * k));
}

// mode 3: gauss0, mode 4: gauss1.  One thread per pixel; with D at compile time the D planes of prob and hypos are loaded into
// registers first (plane stride h*w: coalesced rows) and every pass runs over registers; DT = 0 walks memory again in every pass.
template <int DT>
__global__ __launch_bounds__(kThreads) void hypos_curve_fit_kernel(int mode, const float* __restrict__ prob, const float* __restrict__ depth,
                                       const float* __restrict__ hypos, int per_pixel, float* __restrict__ s_out, int B, int D_rt,
                                       int hw) {
  const int D = DT ? DT : D_rt;
  const size_t n = (size_t)B * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw, pix = i % hw;
    const float* p = prob + b * D * hw + pix;
    const float dep = mode == 3 ? depth[i] : 0.0f;
    if constexpr (DT != 0) {
      float zv[DT], xv[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) { zv[d] = p[(size_t)d * hw]; xv[d] = hyp_at(hypos, per_pixel, b, D, d, hw, pix); }
#pragma unroll
      for (int d = 0; d < DT; ++d) zv[d] = logf(fmaxf(zv[d], 1e-40f));
      auto z = [&](int d) { return zv[d]; };
      if (mode == 3) {
#pragma unroll
        for (int d = 0; d < DT; ++d) { const float e = xv[d] - dep; xv[d] = e * e; }
        s_out[i] = gauss0_fit<DT>(D, [&](int d) { return xv[d]; }, z);
      } else {
        s_out[i] = gauss1_fit<DT>(D, [&](int d) { return xv[d]; }, z);
      }
    } else {
      auto z = [&](int d) { return logf(fmaxf(p[(size_t)d * hw], 1e-40f)); };
      auto x = [&](int d) { return hyp_at(hypos, per_pixel, b, D, d, hw, pix); };
      if (mode == 3) {
        s_out[i] = gauss0_fit<0>(D, [&](int d) { const float e = x(d) - dep; return e * e; }, z);
      } else {
        s_out[i] = gauss1_fit<0>(D, x, z);
      }
    }
  }
}

// ATen upsample_bilinear2d, align_corners=False, scale 2: src = (o+0.5)*0.5-0.5 clamped at 0.
__device__ __forceinline__ void up2_coord(int o, int n_in, int& i0, int& i1, float& l0, float& l1) {
  float src = ((float)o + 0.5f) * 0.5f - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.0f - l1;
}

__device__ __forceinline__ float up2_sample(const float* __restrict__ m, int w, int y0, int y1, int x0, int x1, float ly0,
                                            float ly1, float lx0, float lx1) {
  // rounding order of ATen's CPU upsample_bilinear2d (found by exhaustive search, bit-exact on the goldens):
  //   w_ij = ly_i*lx_j ;  out = fma(w11,v11, fma(w10,v10, fma(w00,v00, w01*v01)))
  const float v00 = m[(size_t)y0 * w + x0], v01 = m[(size_t)y0 * w + x1];
  const float v10 = m[(size_t)y1 * w + x0], v11 = m[(size_t)y1 * w + x1];
  const float w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1;
  return __fmaf_rn(w11, v11, __fmaf_rn(w10, v10, __fmaf_rn(w00, v00, w01 * v01)));
}

// depthhypos.py:49-76.  One thread per OUTPUT pixel; writes D_out hypotheses (stride Ho*Wo -> coalesced).
__global__ void hypos_from_fit_kernel(int mode, const float* __restrict__ s, const float* __restrict__ depth,
                                      const float* __restrict__ range, float log_thresh, float* __restrict__ out, int B,
                                      int D_out, int h, int w, int upsample) {
  const int Ho = upsample ? 2 * h : h, Wo = upsample ? 2 * w : w;
  const size_t ohw = (size_t)Ho * Wo, n = (size_t)B * ohw;
  float gmin = range[0], gmax = range[1];
  for (int b = 1; b < B; ++b) {
    gmin = fminf(gmin, range[2 * b]);
    gmax = fmaxf(gmax, range[2 * b + 1]);
  }
  const float cap_all = (gmax - gmin) / 2.0f;  // depthhypos.py:58
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / ohw;
    const int oy = (int)((i % ohw) / Wo), ox = (int)(i % Wo);
    const float lo = range[2 * b], hi = range[2 * b + 1];
    float sv, dv;
    if (upsample) {
      int y0, y1, x0, x1;
      float ly0, ly1, lx0, lx1;
      up2_coord(oy, h, y0, y1, ly0, ly1);
      up2_coord(ox, w, x0, x1, lx0, lx1);
      sv = up2_sample(s + b * h * w, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
      dv = up2_sample(depth + b * h * w, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
    } else {
      sv = s[i];
      dv = depth[i];
    }
    float res = (mode == 1) ? sqrtf((-1.0f * sv) * log_thresh) : fabsf(sv * log_thresh);  // :54-57
    res = res < 1e-6f ? 1e-6f : res;                                                      // :58 clamp keeps NaN
    res = res > cap_all ? cap_all : res;
    const float cap_b = (hi - lo) * 0.2f;                                                 // :60-61
    res = res > cap_b ? cap_b : res;
    const float step = res / (float)(D_out - 1);                                          // :64
    const float base = dv - 0.5f * res;                                                   // :65
    for (int k = 0; k < D_out; ++k) {
      float hk = base + step * (float)k;                                                  // :66-67
      float t = hk - lo;                                                                  // :71-72
      hk = lo + (t < 0.0f ? 0.0f : t);
      t = hk - hi;                                                                        // :73-74
      hk = hi + (t > 0.0f ? 0.0f : t);
      out[(b * D_out + k) * ohw + (i % ohw)] = hk;
    }
  }
}

// ---- the adaptive-thin-volume range (depthhypos.py:218-253, UCS-Net's baseline the curve fits are compared with) ----
// Spread of the previous stage's distribution around its regressed depth: e = scale * sqrt(sum_d p_d (x_d - depth)^2), the
// exp_variance that atv_hypos takes.  Nothing in the reference computes it, so there are no bits to mirror: the sum runs in four
// interleaved fma accumulators (Sum4) and is held to the formula in float64, (D/2 + 4) * 2^-24 relative.  The probabilities are
// summed as p * 2^64 and the root scaled back by 2^-32, both exact: a softmax's denormal tails times a squared distance of a few
// millimetres would otherwise round in the denormal range, where the error is absolute.  A sum of exact zeros (p = 0 everywhere,
// or a one-hot p on a hypothesis equal to the depth) gives exactly 0.  Same traffic as hypos_curve_fit_kernel's mode 3.
template <int DT>
__global__ __launch_bounds__(kThreads) void atv_spread_kernel(const float* __restrict__ prob, const float* __restrict__ depth,
                                                              const float* __restrict__ hypos, int per_pixel, float scale,
                                                              float* __restrict__ e_out, int B, int D_rt, int hw) {
  const int D = DT ? DT : D_rt;
  const size_t n = (size_t)B * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw, pix = i % hw;
    const float* p = prob + b * D * hw + pix;
    const float dep = depth[i];
    Sum4 acc;
    if constexpr (DT != 0) {
      float pv[DT], xv[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) { pv[d] = p[(size_t)d * hw]; xv[d] = hyp_at(hypos, per_pixel, b, D, d, hw, pix); }
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const float t = xv[d] - dep;
        acc.fma(d, ldexpf(pv[d], 64), t * t);
      }
    } else {
      for (int d = 0; d < D; ++d) {
        const float t = hyp_at(hypos, per_pixel, b, D, d, hw, pix) - dep;
        acc.fma(d, ldexpf(p[(size_t)d * hw], 64), t * t);
      }
    }
    e_out[i] = scale * ldexpf(sqrtf(acc.result()), -32);
  }
}

// depthhypos.py:239-253 with the depth upsampled as HyposByFit does it (:51).  One thread per OUTPUT pixel, D_out coalesced planes:
//   low = -min(d2, e2);  step = (e2 - low) / (D_out - 1);  hyp_i = ((d2 + low) + step * i) + 1e-12
// torch's operations one by one, each rounded on its own (no fma: the reference has none); torch.min hands on a NaN of either side.
// No clamp to the depth range: the reference has none, the lower bound keeps every hypothesis >= 1e-12.
__global__ void atv_hypos_kernel(const float* __restrict__ e, const float* __restrict__ depth, float* __restrict__ out, int B,
                                 int D_out, int h, int w, int upsample) {
  const int Ho = upsample ? 2 * h : h, Wo = upsample ? 2 * w : w;
  const size_t ohw = (size_t)Ho * Wo, n = (size_t)B * ohw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / ohw;
    float ev, dv;
    if (upsample) {
      const int oy = (int)((i % ohw) / Wo), ox = (int)(i % Wo);
      int y0, y1, x0, x1;
      float ly0, ly1, lx0, lx1;
      up2_coord(oy, h, y0, y1, ly0, ly1);
      up2_coord(ox, w, x0, x1, lx0, lx1);
      ev = up2_sample(e + b * h * w, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
      dv = up2_sample(depth + b * h * w, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
    } else {
      ev = e[i];
      dv = depth[i];
    }
    float m = dv < ev ? dv : ev;                                                          // :243
    m = ev != ev ? ev : (dv != dv ? dv : m);
    const float low = -m;
    const float step = __fdiv_rn(__fsub_rn(ev, low), (float)(D_out - 1));                 // :245
    const float base = __fadd_rn(dv, low);                                                // :249
    for (int k = 0; k < D_out; ++k)
      out[(b * D_out + k) * ohw + (i % ohw)] = __fadd_rn(__fadd_rn(base, __fmul_rn(step, (float)k)), 1e-12f);
  }
}

// One thread per pixel: at 1/8 resolution (148 x 200) that is 29,600 threads -- 116 blocks of 256 on 256 CUs, i.e. 140 CUs idle and
// four waves on each of the others.  Small problems therefore go out as one-wave blocks, which the dispatcher spreads over all CUs
// (the kernels index with blockDim.x; nothing in them is block-cooperative).
inline int block_for(size_t n) { return n < (size_t)256 * 1024 ? 64 : kThreads; }
inline int grid_for(size_t n) {
  const size_t t = (size_t)block_for(n);
  size_t g = (n + t - 1) / t;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

extern "C" int mdf_depth_regress_fwd(const float* prob, const float* hypos, int hypos_per_pixel, float* depth, int B,
                                     int D, int h, int w, void* stream) {
  MDF_REQUIRE(prob && hypos && depth, "null pointer argument");
  MDF_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0, "bad shape");
  hipLaunchKernelGGL(depth_regress_kernel, dim3(grid_for((size_t)B * h * w)), dim3(block_for((size_t)B * h * w)), 0, (hipStream_t)stream,
                     prob, hypos, hypos_per_pixel, depth, B, D, h * w);
  return mdf::check_launch("depth_regress_kernel");
}

extern "C" int mdf_confidence_fwd(const float* prob, float* conf, int64_t* idx_out, int B, int D, int h, int w,
                                  void* stream) {
  MDF_REQUIRE(prob && conf, "null pointer argument");
  MDF_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0, "bad shape");
  hipLaunchKernelGGL(confidence_kernel, dim3(grid_for((size_t)B * h * w)), dim3(block_for((size_t)B * h * w)), 0, (hipStream_t)stream, prob,
                     conf, idx_out, B, D, h * w);
  return mdf::check_launch("confidence_kernel");
}

extern "C" int mdf_confidence_up2_fwd(const float* prob, float* conf2, int B, int D, int h, int w, void* stream) {
  MDF_REQUIRE(prob && conf2, "null pointer argument");
  MDF_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0, "bad shape");
  if (D == 8) hipLaunchKernelGGL(confidence_up2_kernel<8>, dim3(grid_for((size_t)B * h * w)), dim3(block_for((size_t)B * h * w)), 0, (hipStream_t)stream, prob, conf2, B, D, h, w);
  else hipLaunchKernelGGL(confidence_up2_kernel<0>, dim3(grid_for((size_t)B * h * w)), dim3(block_for((size_t)B * h * w)), 0, (hipStream_t)stream, prob, conf2, B, D, h, w);
  return mdf::check_launch("confidence_up2_kernel");
}

extern "C" int mdf_confidence_cascade_fwd(const float* prob, const float* last, float w_last, float w_cur, int n, int pad_front,
                                          int up2, float* conf, int B, int D, int H, int W, void* stream) {
  MDF_REQUIRE(prob && conf, "null pointer argument");
  MDF_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "bad shape");
  MDF_REQUIRE(n == 1 || n == 2 || n == 4 || n == 8, "window length n must be 1, 2, 4 or 8 (n * avg_pool is a sum only then), got %d", n);
  MDF_REQUIRE(pad_front >= 0, "pad_front must not be negative, got %d", pad_front);
  MDF_REQUIRE(!last || (H % 2 == 0 && W % 2 == 0), "last confidence [B,H/2,W/2] needs even H and W, got %d x %d", H, W);
  const size_t px = (size_t)B * H * W;
#define MDF_CC(DT) hipLaunchKernelGGL(confidence_cascade_kernel<DT>, dim3(grid_for(px)), dim3(block_for(px)), 0, (hipStream_t)stream, prob, \
                                      last, w_last, w_cur, n, pad_front, up2 ? 1 : 0, conf, B, D, H, W)
  if (D == 48) MDF_CC(48); else if (D == 24) MDF_CC(24); else if (D == 8) MDF_CC(8); else MDF_CC(0);
#undef MDF_CC
  return mdf::check_launch("confidence_cascade_kernel");
}

extern "C" int mdf_range_affine_fwd(const float* x, const float* lo, const float* span, int mode, float* y, int B, long long n, void* stream) {
  MDF_REQUIRE(x && lo && span && y, "null pointer argument");
  MDF_REQUIRE(B > 0 && n > 0 && (mode == 0 || mode == 1), "bad shape / mode");
  hipLaunchKernelGGL(range_affine_kernel, dim3(grid_for((size_t)B * n)), dim3(block_for((size_t)B * n)), 0, (hipStream_t)stream, x, lo, span, mode, y, B, (size_t)n);
  return mdf::check_launch("range_affine_kernel");
}

extern "C" int mdf_hypos_fit_fwd(int mode, const float* prob, const float* depth, const float* hypos,
                                 int hypos_per_pixel, const float* fit_row, float* s_out, int B, int D, int h, int w,
                                 void* stream) {
  MDF_REQUIRE(prob && s_out, "null pointer argument");
  MDF_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0, "bad shape");
  if (mode == 1) {
    MDF_REQUIRE(fit_row, "gauss1 fit needs fit_row (row 0 of (X^T X)^-1 X^T, [B,D])");
    if (hypos_per_pixel)
      return mdf::fail(MDF_EUNSUPPORTED, "gauss1 fit with per-pixel hypotheses is not built (config.py:199-201 uses it "
                                         "only after the uniform stage)");
  } else if (mode == 2) {
    MDF_REQUIRE(depth && hypos, "laplace fit needs depth and hypos");
  } else if (mode == 3 || mode == 4) {
    if (mode == 3) MDF_REQUIRE(depth && hypos, "gauss0 fit needs depth and hypos");
    else MDF_REQUIRE(hypos, "gauss1 fit (mode 4) needs hypos");
#define MDF_HC(DT) hipLaunchKernelGGL(hypos_curve_fit_kernel<DT>, dim3(grid_for((size_t)B * h * w)), dim3(block_for((size_t)B * h * w)), 0, (hipStream_t)stream, \
                                      mode, prob, depth, hypos, hypos_per_pixel, s_out, B, D, h * w)
    if (D == 48) MDF_HC(48); else if (D == 24) MDF_HC(24); else if (D == 8) MDF_HC(8); else MDF_HC(0);
#undef MDF_HC
    return mdf::check_launch("hypos_curve_fit_kernel");
  } else {
    return mdf::fail(MDF_EARG, "mode must be 1 (gauss1, shared hypotheses), 2 (laplace), 3 (gauss0) or 4 (gauss1), got %d", mode);
  }
#define MDF_HF(DT) hipLaunchKernelGGL(hypos_fit_kernel<DT>, dim3(grid_for((size_t)B * h * w)), dim3(block_for((size_t)B * h * w)), 0, (hipStream_t)stream, mode, \
                                      prob, depth, hypos, hypos_per_pixel, fit_row, s_out, B, D, h * w)
  if (D == 48) MDF_HF(48); else if (D == 24) MDF_HF(24); else if (D == 8) MDF_HF(8); else MDF_HF(0);
#undef MDF_HF
  return mdf::check_launch("hypos_fit_kernel");
}

extern "C" int mdf_hypos_from_fit_fwd(int mode, const float* s, const float* depth, const float* range, float log_thresh,
                                      float* hypos_out, int B, int D_out, int h, int w, int upsample, void* stream) {
  MDF_REQUIRE(s && depth && range && hypos_out, "null pointer argument");
  MDF_REQUIRE(B > 0 && D_out > 1 && h > 0 && w > 0, "bad shape");
  MDF_REQUIRE(mode == 1 || mode == 2, "mode must be 1 (gauss1) or 2 (laplace), got %d", mode);
  const size_t n = (size_t)B * h * w * (upsample ? 4 : 1);
  hipLaunchKernelGGL(hypos_from_fit_kernel, dim3(grid_for(n)), dim3(block_for(n)), 0, (hipStream_t)stream, mode, s, depth,
                     range, log_thresh, hypos_out, B, D_out, h, w, upsample);
  return mdf::check_launch("hypos_from_fit_kernel");
}

extern "C" int mdf_atv_spread_fwd(const float* prob, const float* depth, const float* hypos, int hypos_per_pixel, float scale,
                                  float* spread_out, int B, int D, int h, int w, void* stream) {
  MDF_REQUIRE(prob && depth && hypos && spread_out, "null pointer argument");
  MDF_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0, "bad shape");
  MDF_REQUIRE(scale > 0.0f && scale <= 3.402823466e38f, "scale must be finite and positive, got %g", (double)scale);
  const size_t px = (size_t)B * h * w;
#define MDF_AS(DT) hipLaunchKernelGGL(atv_spread_kernel<DT>, dim3(grid_for(px)), dim3(block_for(px)), 0, (hipStream_t)stream, prob, depth, \
                                      hypos, hypos_per_pixel, scale, spread_out, B, D, h * w)
  if (D == 48) MDF_AS(48); else if (D == 24) MDF_AS(24); else if (D == 8) MDF_AS(8); else MDF_AS(0);
#undef MDF_AS
  return mdf::check_launch("atv_spread_kernel");
}

extern "C" int mdf_atv_hypos_fwd(const float* spread, const float* depth, float* hypos_out, int B, int D_out, int h, int w,
                                 int upsample, void* stream) {
  MDF_REQUIRE(spread && depth && hypos_out, "null pointer argument");
  MDF_REQUIRE(B > 0 && h > 0 && w > 0, "bad shape");
  MDF_REQUIRE(D_out >= 2, "D_out must be at least 2 (the step divides by D_out - 1), got %d", D_out);
  const size_t n = (size_t)B * h * w * (upsample ? 4 : 1);
  hipLaunchKernelGGL(atv_hypos_kernel, dim3(grid_for(n)), dim3(block_for(n)), 0, (hipStream_t)stream, spread, depth, hypos_out, B,
                     D_out, h, w, upsample ? 1 : 0);
  return mdf::check_launch("atv_hypos_kernel");
}
