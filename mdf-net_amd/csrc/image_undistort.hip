// Scene import: resampling a distorted photograph to a pinhole camera (include/mdfnet_hip.h states the semantics and the operation
// order; tests/undistort_oracle.py restates it in float64).  Coordinates, weights and the sample mean are fp64, every product, sum
// and quotient rounded once (the __d*_rn intrinsics; sqrt is correctly rounded), so the rational kind is a function of its inputs bit
// for bit; the fisheye kind goes through the device's atan.
//   launch   one thread per output pixel over the flattened [B*Hd*Wd] index: neighbouring lanes take neighbouring columns, so the
//            3-byte taps of a wave fall into few cache lines.  A block's 256 pixels are 768 contiguous bytes of dst: they are put
//            together in LDS and leave as 192 aligned dwords (valid: 64 dwords), bytes only at a ragged end or an unaligned base.
// No atomics, no allocation, no synchronisation with the host; the coefficients travel in the kernel arguments.
#include <cmath>
#include <cstdint>
#include "common.h"

namespace {

constexpr int kBlock = 256;

struct UndistortParams {
  const uint8_t* src;
  uint8_t* dst;
  uint8_t* valid;
  int B, Hs, Ws, Hd, Wd, kind, nsub;
  long long npix;            // B * Hd * Wd
  double k[12];
  double fx, fy, cx, cy, zfx, zfy, scale;
};

__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double quo(double a, double b) { return __ddiv_rn(a, b); }

// (x, y) -> (xd, yd), in the header's order
__device__ __forceinline__ void distort(const UndistortParams& P, double x, double y, double& xd, double& yd) {
  const double xx = mul(x, x), yy = mul(y, y);
  const double r2 = add(xx, yy);
  const double* k = P.k;
  if (P.kind == MDF_UNDISTORT_RATIONAL) {
    const double r4 = mul(r2, r2), r6 = mul(r4, r2);
    const double num = add(add(add(1.0, mul(k[0], r2)), mul(k[1], r4)), mul(k[4], r6));
    const double den = add(add(add(1.0, mul(k[5], r2)), mul(k[6], r4)), mul(k[7], r6));
    const double rad = quo(num, den);
    const double xy2 = mul(2.0, mul(x, y));
    const double tx = add(mul(k[2], xy2), mul(k[3], add(r2, mul(2.0, xx))));
    const double ty = add(mul(k[3], xy2), mul(k[2], add(r2, mul(2.0, yy))));
    xd = add(mul(x, rad), tx);
    yd = add(mul(y, rad), ty);
  } else {
    const double r = sqrt(r2);
    if (r == 0.0) {
      xd = x;
      yd = y;
      return;
    }
    const double th = atan(r);
    const double t2 = mul(th, th), t4 = mul(t2, t2), t6 = mul(t4, t2), t8 = mul(t4, t4);
    const double poly = add(add(add(add(1.0, mul(k[0], t2)), mul(k[1], t4)), mul(k[2], t6)), mul(k[3], t8));
    const double sc = quo(mul(th, poly), r);
    xd = mul(x, sc);
    yd = mul(y, sc);
  }
}

__global__ __launch_bounds__(kBlock) void image_undistort_kernel(const UndistortParams P) {
  __shared__ uint32_t tile[kBlock * 3 / 4];
  __shared__ uint32_t vtile[kBlock / 4];
  uint8_t* tile8 = reinterpret_cast<uint8_t*>(tile);
  uint8_t* vtile8 = reinterpret_cast<uint8_t*>(vtile);
  const int tid = threadIdx.x;
  const long long first = (long long)blockIdx.x * kBlock, pix = first + tid;
  if (pix < P.npix) {
    const int j = (int)(pix % P.Wd), i = (int)((pix / P.Wd) % P.Hd), b = (int)(pix / ((long long)P.Wd * P.Hd));
    const uint8_t* img = P.src + (long long)b * P.Hs * P.Ws * 3;       // < 2^31 bytes in all: the entry checked
    const double n = (double)P.nsub, umax = sub((double)P.Ws, 0.5), vmax = sub((double)P.Hs, 0.5);
    double acc[3] = {0.0, 0.0, 0.0};
    int ok = 1;
    for (int sb = 0; sb < P.nsub; ++sb) {
      const double Y = quo(add((double)i, quo(add((double)sb, 0.5), n)), P.scale);
      const double y = quo(sub(Y, P.cy), P.zfy);
      for (int sa = 0; sa < P.nsub; ++sa) {
        const double X = quo(add((double)j, quo(add((double)sa, 0.5), n)), P.scale);
        const double x = quo(sub(X, P.cx), P.zfx);
        double xd, yd;
        distort(P, x, y, xd, yd);
        const double U = sub(add(mul(P.fx, xd), P.cx), 0.5), V = sub(add(mul(P.fy, yd), P.cy), 0.5);
        if (!(U >= -0.5 && U <= umax && V >= -0.5 && V <= vmax)) {      // a NaN fails every comparison: blank
          ok = 0;
          continue;
        }
        const double fu = floor(U), fv = floor(V);                    // in [-1, Ws - 1] x [-1, Hs - 1]
        const double wu = sub(U, fu), wv = sub(V, fv), mu = sub(1.0, wu), mv = sub(1.0, wv);
        const int u0 = max((int)fu, 0), u1 = min((int)fu + 1, P.Ws - 1), v0 = max((int)fv, 0), v1 = min((int)fv + 1, P.Hs - 1);
        const uint8_t* p00 = img + ((long long)v0 * P.Ws + u0) * 3;
        const uint8_t* p01 = img + ((long long)v0 * P.Ws + u1) * 3;
        const uint8_t* p10 = img + ((long long)v1 * P.Ws + u0) * 3;
        const uint8_t* p11 = img + ((long long)v1 * P.Ws + u1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double top = add(mul((double)p00[c], mu), mul((double)p01[c], wu));
          const double bot = add(mul((double)p10[c], mu), mul((double)p11[c], wu));
          acc[c] = add(acc[c], add(mul(top, mv), mul(bot, wv)));
        }
      }
    }
    const double nn = mul(n, n);
#pragma unroll
    for (int c = 0; c < 3; ++c) tile8[tid * 3 + c] = (uint8_t)min(floor(add(quo(acc[c], nn), 0.5)), 255.0);
    vtile8[tid] = (uint8_t)ok;
  }
  __syncthreads();
  const long long left = P.npix - first;                              // > 0: the grid is ceil(npix / kBlock)
  const int count = left < kBlock ? (int)left : kBlock;
  uint8_t* out = P.dst + first * 3;
  if (count == kBlock && reinterpret_cast<uintptr_t>(out) % 4 == 0) {
    if (tid < kBlock * 3 / 4) reinterpret_cast<uint32_t*>(out)[tid] = tile[tid];
  } else {
    for (int q = tid; q < count * 3; q += kBlock) out[q] = tile8[q];
  }
  if (P.valid) {
    uint8_t* vout = P.valid + first;
    if (count == kBlock && reinterpret_cast<uintptr_t>(vout) % 4 == 0) {
      if (tid < kBlock / 4) reinterpret_cast<uint32_t*>(vout)[tid] = vtile[tid];
    } else if (tid < count) {
      vout[tid] = vtile8[tid];
    }
  }
}

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

// B * H * W * 3 <= 2^31 - 1, the three factors positive (no product here leaves long long)
bool fits_int32(int B, int H, int W) {
  const long long lim = ((1ll << 31) - 1) / 3, hw = (long long)H * W;
  return hw <= lim && B <= lim / hw;
}

}  // namespace

extern "C" int mdf_image_undistort(const uint8_t* src, uint8_t* dst, uint8_t* valid, int B, int Hs, int Ws, int Hd, int Wd, int kind,
                                   const double* coeffs, double fx, double fy, double cx, double cy, double zoom, double scale, int nsub,
                                   void* stream) {
  MDF_REQUIRE(src && dst, "null pointer argument: src / dst");
  MDF_REQUIRE(coeffs, "null pointer argument: coeffs");
  MDF_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "sizes must be positive: B=%d, source %d x %d, output %d x %d", B, Ws, Hs, Wd, Hd);
  MDF_REQUIRE(kind == MDF_UNDISTORT_RATIONAL || kind == MDF_UNDISTORT_FISHEYE, "kind=%d not in {0 (rational), 1 (fisheye)}", kind);
  MDF_REQUIRE(nsub >= 1 && nsub <= MDF_UNDISTORT_MAX_NSUB, "nsub=%d out of range [1,%d]", nsub, MDF_UNDISTORT_MAX_NSUB);
  MDF_REQUIRE(positive(fx) && positive(fy), "focal lengths fx=%g, fy=%g must be finite and > 0", fx, fy);
  MDF_REQUIRE(std::isfinite(cx) && std::isfinite(cy), "principal point cx=%g, cy=%g must be finite", cx, cy);
  MDF_REQUIRE(positive(zoom), "zoom=%g must be finite and > 0", zoom);
  MDF_REQUIRE(positive(scale), "scale=%g must be finite and > 0", scale);
  MDF_REQUIRE(fits_int32(B, Hs, Ws), "source %d x %d x %d x 3 bytes exceed int32 indexing", B, Hs, Ws);
  MDF_REQUIRE(fits_int32(B, Hd, Wd), "output %d x %d x %d x 3 bytes exceed int32 indexing", B, Hd, Wd);
  UndistortParams P{};
  P.src = src, P.dst = dst, P.valid = valid;
  P.B = B, P.Hs = Hs, P.Ws = Ws, P.Hd = Hd, P.Wd = Wd, P.kind = kind, P.nsub = nsub;
  P.npix = (long long)B * Hd * Wd;
  for (int a = 0; a < 12; ++a) {
    MDF_REQUIRE(std::isfinite(coeffs[a]), "coeffs[%d]=%g must be finite", a, coeffs[a]);
    P.k[a] = coeffs[a];
  }
  P.fx = fx, P.fy = fy, P.cx = cx, P.cy = cy, P.scale = scale;
  P.zfx = zoom * fx, P.zfy = zoom * fy;                                // one rounding each (host code is built without contraction too)
  MDF_REQUIRE(positive(P.zfx) && positive(P.zfy), "zoom * focal length (%g, %g) must be finite and > 0", P.zfx, P.zfy);
  const unsigned grid = (unsigned)((P.npix + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(image_undistort_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, P);
  return mdf::check_launch("image_undistort_kernel");
}
