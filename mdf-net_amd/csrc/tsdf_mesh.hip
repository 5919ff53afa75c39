// Meshing ("TSDF meshing"): depth maps -> truncated signed distance volume -> triangle mesh -> vertex colours.
//   integrate  tsdf_integrate_kernel, voxel-stationary: a thread owns one lattice point and walks the views of a chunk in the
//              order given; a block owns a 16x4x4 brick and may skip a view for the whole brick (culling, never changes a bit).
//   extract    marching tetrahedra over the Kuhn split of each cell: mesh_count_kernel (triangles per cell, edge marks),
//              mesh_scan_kernel (chunk sums, their scan, per-point offsets), mesh_emit_kernel (vertices and triangles in order).
//   colour     mesh_colour_kernel, vertex-stationary, views in the order given.
// Arithmetic order == tests/tsdf_mesh_oracle.py (numpy fp32, one correctly rounded operation at a time); the library builds
// with -ffp-contract=off and every operation that decides an output bit is an explicit __f*_rn.
#include "common.h"
#include "scan_common.h"
#include "tsdf_mesh.h"

namespace {

using namespace mdf::tsdf;

constexpr int kBlock = mdf::kScanBlock;   // 256
constexpr int kBx = 16, kBy = 4, kBz = 4;  // the brick of a block (x fastest: a wave reads 4 rows of 64 B)
static_assert(kBx * kBy * kBz == kBlock, "a thread per brick point");

__device__ __forceinline__ float row(const float* r, float t, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r[0], x), __fmul_rn(r[1], y)), __fmul_rn(r[2], z)), t);
}

// World point -> (texel index, camera depth) of one view; false = the view does not see it (behind, not finite, off the map).
__device__ __forceinline__ bool project(const float* c, int h, int w, float x, float y, float z, int* texel, float* zc) {
  const float px = row(c + kR, c[kT], x, y, z), py = row(c + kR + 3, c[kT + 1], x, y, z), pz = row(c + kR + 6, c[kT + 2], x, y, z);
  if (!(pz > 0.f) || !isfinite(pz)) return false;
  const float u = floorf(__fadd_rn(__fadd_rn(__fdiv_rn(__fmul_rn(c[kFx], px), pz), c[kCx]), 0.5f));
  const float v = floorf(__fadd_rn(__fadd_rn(__fdiv_rn(__fmul_rn(c[kFy], py), pz), c[kCy]), 0.5f));
  if (!(u >= 0.f && u < (float)w && v >= 0.f && v < (float)h)) return false;   // NaN fails
  *texel = (int)v * w + (int)u;
  *zc = pz;
  return true;
}

__device__ __forceinline__ float lattice(float o, float s, int i) { return __fadd_rn(o, __fmul_rn(s, (float)i)); }

struct IntegrateArgs {
  float* D;
  float* W;
  const float* depth[kChunk];
  float cam[kChunk][kCamFloats];
  int nviews, h, w, nx, ny, nz, cull;
  float ox, oy, oz, s, tau;
};

// May every point of the box [x0,x1]x[y0,y1]x[z0,z1] skip this view?  Only "certainly yes" answers true: the bounds carry the
// rounding error of the points' own fp32 projections (e* below, 16 eps of the magnitude sums, twice what the chains can lose),
// and a NaN or infinity anywhere fails every comparison that leads to true.
__device__ bool brick_skips_view(const float* c, int h, int w, float tau, float x0, float x1, float y0, float y1, float z0, float z1) {
  const float inf = __builtin_inff();
  float zmin = inf, umin = inf, umax = -inf, vmin = inf, vmax = -inf, mx = 0.f, my = 0.f, mz = 0.f, ax = 0.f, ay = 0.f;
  float pxs[8], pys[8], pzs[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = (k & 1) ? x1 : x0, y = (k & 2) ? y1 : y0, z = (k & 4) ? z1 : z0;
    pxs[k] = row(c + kR, c[kT], x, y, z);
    pys[k] = row(c + kR + 3, c[kT + 1], x, y, z);
    pzs[k] = row(c + kR + 6, c[kT + 2], x, y, z);
    mx = fmaxf(mx, fabsf(c[kR + 0] * x) + fabsf(c[kR + 1] * y) + fabsf(c[kR + 2] * z));
    my = fmaxf(my, fabsf(c[kR + 3] * x) + fabsf(c[kR + 4] * y) + fabsf(c[kR + 5] * z));
    mz = fmaxf(mz, fabsf(c[kR + 6] * x) + fabsf(c[kR + 7] * y) + fabsf(c[kR + 8] * z));
    ax = fmaxf(ax, fabsf(pxs[k]));
    ay = fmaxf(ay, fabsf(pys[k]));
    zmin = fminf(zmin, pzs[k]);
    if (!isfinite(pxs[k]) || !isfinite(pys[k]) || !isfinite(pzs[k])) return false;
  }
  const float ex = 1e-6f * (mx + fabsf(c[kT])), ey = 1e-6f * (my + fabsf(c[kT + 1])), ez = 1e-6f * (mz + fabsf(c[kT + 2]));
  const float zlo = zmin - ez;
  if (!(zlo > 0.f)) return false;                                  // a corner at (or too near) z <= 0: never culled
  if (zlo > (c[kDmax] + tau) * 1.00001f) return true;              // behind every valid depth by more than tau: sdf < -tau
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float u = c[kFx] * pxs[k] / pzs[k] + c[kCx], v = c[kFy] * pys[k] / pzs[k] + c[kCy];
    umin = fminf(umin, u); umax = fmaxf(umax, u);
    vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
  }
  const float eu = 2.f * fabsf(c[kFx]) * (ex + (ax + ex) * ez / zlo) / zlo + 1e-5f * (fmaxf(fabsf(umin), fabsf(umax)) + fabsf(c[kCx]) + 1.f);
  const float ev = 2.f * fabsf(c[kFy]) * (ey + (ay + ey) * ez / zlo) / zlo + 1e-5f * (fmaxf(fabsf(vmin), fabsf(vmax)) + fabsf(c[kCy]) + 1.f);
  // the rounded pixel is floor(u + 0.5): off the map by more than a pixel on one side for the whole (convex) brick
  return umax + eu < -1.5f || umin - eu > (float)w + 0.5f || vmax + ev < -1.5f || vmin - ev > (float)h + 0.5f;
}

__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(const IntegrateArgs p) {
  __shared__ unsigned skip_views;
  const int i0 = blockIdx.x * kBx, j0 = blockIdx.y * kBy, k0 = blockIdx.z * kBz;
  if (threadIdx.x < 64) {
    bool skip = false;
    if (p.cull && (int)threadIdx.x < p.nviews) {
      const int i1 = min(i0 + kBx, p.nx) - 1, j1 = min(j0 + kBy, p.ny) - 1, k1 = min(k0 + kBz, p.nz) - 1;
      skip = brick_skips_view(p.cam[threadIdx.x], p.h, p.w, p.tau, lattice(p.ox, p.s, i0), lattice(p.ox, p.s, i1),
                              lattice(p.oy, p.s, j0), lattice(p.oy, p.s, j1), lattice(p.oz, p.s, k0), lattice(p.oz, p.s, k1));
    }
    const unsigned long long m = __ballot(skip);
    if (threadIdx.x == 0) skip_views = (unsigned)m;
  }
  __syncthreads();
  const unsigned skip = skip_views;
  const int i = i0 + (threadIdx.x & (kBx - 1)), j = j0 + ((threadIdx.x / kBx) & (kBy - 1)), k = k0 + threadIdx.x / (kBx * kBy);
  if (i >= p.nx || j >= p.ny || k >= p.nz) return;
  const size_t at = ((size_t)k * p.ny + j) * p.nx + i;
  const float x = lattice(p.ox, p.s, i), y = lattice(p.oy, p.s, j), z = lattice(p.oz, p.s, k);
  float D = p.D[at], W = p.W[at];
  for (int v = 0; v < p.nviews; ++v) {
    if (skip >> v & 1u) continue;
    int texel;
    float zc;
    if (!project(p.cam[v], p.h, p.w, x, y, z, &texel, &zc)) continue;
    const float d = p.depth[v][texel];
    if (!isfinite(d) || !(d > 0.f)) continue;
    const float sdf = __fsub_rn(d, zc);
    if (sdf < -p.tau) continue;
    const float f = fminf(1.f, __fdiv_rn(sdf, p.tau));
    const float w1 = __fadd_rn(W, 1.f);
    D = __fdiv_rn(__fadd_rn(__fmul_rn(D, W), f), w1);
    W = w1;
  }
  p.D[at] = D;
  p.W[at] = W;
}

// ---------------------------------------------------------------------------------------------------- extraction
struct MeshArgs {
  const float* D;
  const float* W;
  unsigned char* marks;      // [N][8]: marks[8 p + d] != 0 <=> edge (p, p + d) carries a vertex (d = 1..7 as a bit mask)
  unsigned char* tcount;     // [N] triangles of the cell whose minimum corner is p
  unsigned char* emask;      // [N] bit d <=> marks[8 p + d]
  int* voff;                 // [N] index of p's first vertex
  int* toff;                 // [N] index of the first triangle of p's cell
  int* chunk_sums;           // [2][nchunk] vertices, triangles per chunk of kMeshChunk points
  long long* chunk_off;      // [2][nchunk]
  long long* totals;         // [2] n_vertices, n_triangles
  float* vertices;
  int* triangles;
  int nx, ny, nz, nchunk;
  long long n;
  long long nv, nt;          // capacity of vertices / triangles (emit): nothing is stored past them
  float ox, oy, oz, s, min_weight;
};

__device__ __forceinline__ int corner_at(const MeshArgs& p, int at, int c) {
  return at + (c & 1) + ((c >> 1 & 1) + (c >> 2 & 1) * p.ny) * p.nx;
}

// Inside mask of the cell whose minimum corner is lattice point `at` (bit c = corner c); -1 if a corner is not observed.
__device__ __forceinline__ int cell_mask(const MeshArgs& p, int at) {
  int mask = 0;
  bool valid = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int q = corner_at(p, at, c);
    const bool seen = p.W[q] >= p.min_weight;
    valid = valid && seen;
    mask |= (seen && p.D[q] < 0.f) ? 1 << c : 0;
  }
  return valid ? mask : -1;
}

// Tetrahedron t = 0..5 of the Kuhn split: corners (0, a, a|b, 7), 4 bits each from the low end, for the permutations (a, b, c) of
// (1, 2, 4) in lexicographic order; *odd = the permutation is odd (the tetrahedron is negatively oriented).
__device__ __forceinline__ unsigned tet_corners(int t, bool* odd) {
  const int a = 1 << (t >> 1);
  const int lo = a == 1 ? 2 : 1, hi = a == 4 ? 2 : 4;           // the two other axes, ascending
  const int b = (t & 1) ? hi : lo;
  // (a,b,c): (1,2,4)+ (1,4,2)- (2,1,4)- (2,4,1)+ (4,1,2)+ (4,2,1)-
  *odd = t == 1 || t == 2 || t == 5;
  return 0u | (unsigned)a << 4 | (unsigned)(a | b) << 8 | 7u << 12;
}

// The tetrahedron's positions 0..3, 2 bits each from the low end: the inside ones first, then the outside ones, both ascending.
__device__ __forceinline__ unsigned order_by_side(unsigned in4, int* n_in) {
  unsigned perm = 0;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (in4 >> k & 1u) perm |= (unsigned)k << (2 * n++);
  *n_in = n;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (!(in4 >> k & 1u)) perm |= (unsigned)k << (2 * n++);
  return perm;
}

__device__ __forceinline__ unsigned tet_inside(unsigned corners, int mask) {
  unsigned in4 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) in4 |= (unsigned)(mask >> (corners >> (4 * k) & 7u) & 1) << k;
  return in4;
}

__global__ __launch_bounds__(kBlock) void mesh_count_kernel(const MeshArgs p) {
  const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (gid >= p.n) return;
  const int at = (int)gid;
  const int i = at % p.nx, j = at / p.nx % p.ny, k = at / p.nx / p.ny;
  int ntri = 0;
  if (i + 1 < p.nx && j + 1 < p.ny && k + 1 < p.nz) {
    const int mask = cell_mask(p, at);
    if (mask > 0 && mask < 255) {
      for (int t = 0; t < 6; ++t) {
        bool odd;
        const unsigned corners = tet_corners(t, &odd);
        const unsigned in4 = tet_inside(corners, mask);
        if (in4 == 0u || in4 == 15u) continue;
        ntri += __popc(in4) == 2 ? 2 : 1;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = a + 1; b < 4; ++b)
            if ((in4 >> a & 1u) != (in4 >> b & 1u)) {
              const int ca = corners >> (4 * a) & 7u, cb = corners >> (4 * b) & 7u;     // ca is a subset of cb
              p.marks[(size_t)corner_at(p, at, ca) * 8 + (cb ^ ca)] = 1;               // idempotent: every writer stores 1
            }
      }
    }
  }
  p.tcount[at] = (unsigned char)ntri;
}

// MODE 0: per-chunk sums of the vertex and triangle counts (and the edge masks).  MODE 1: exclusive scan of the chunk sums by
// one block, totals.  MODE 2: per-point offsets inside each chunk from its offset.
template <int MODE>
__global__ __launch_bounds__(MODE == 1 ? mdf::kScanThreads : kBlock) void mesh_scan_kernel(const MeshArgs p) {
  if (MODE == 1) {
    const int which = blockIdx.x;
    mdf::block_exclusive_scan<int, false>(p.chunk_sums + (size_t)which * p.nchunk, p.nchunk, p.chunk_off + (size_t)which * p.nchunk,
                                          p.totals + which);
    return;
  }
  const long long base = (long long)blockIdx.x * kMeshChunk + threadIdx.x * kMeshPer;
  int nv[kMeshPer], nt[kMeshPer], sv = 0, st = 0;
#pragma unroll
  for (int k = 0; k < kMeshPer; ++k) {
    nv[k] = nt[k] = 0;
    if (base + k < p.n) {
      if (MODE == 0) {
        const unsigned long long m = *reinterpret_cast<const unsigned long long*>(p.marks + (size_t)(base + k) * 8);
        unsigned bits = 0;
#pragma unroll
        for (int d = 1; d < 8; ++d) bits |= (m >> (8 * d) & 0xffull) ? 1u << d : 0u;
        p.emask[base + k] = (unsigned char)bits;
        nv[k] = __popc(bits);
      } else {
        nv[k] = __popc((unsigned)p.emask[base + k]);
      }
      nt[k] = p.tcount[base + k];
    }
    sv += nv[k];
    st += nt[k];
  }
  if (MODE == 0) {
    const int tv = mdf::block_sum(sv);
    __syncthreads();
    const int tt = mdf::block_sum(st);
    if (threadIdx.x == 0) {
      p.chunk_sums[blockIdx.x] = tv;
      p.chunk_sums[p.nchunk + blockIdx.x] = tt;
    }
    return;
  }
  long long rv = p.chunk_off[blockIdx.x] + (mdf::block_inclusive_scan(sv) - sv);
  __syncthreads();
  long long rt = p.chunk_off[p.nchunk + blockIdx.x] + (mdf::block_inclusive_scan(st) - st);
#pragma unroll
  for (int k = 0; k < kMeshPer; ++k) {
    if (base + k < p.n) {
      p.voff[base + k] = (int)rv;
      p.toff[base + k] = (int)rt;
    }
    rv += nv[k];
    rt += nt[k];
  }
}

// Index of the vertex on the edge between cube corners ca and cb of the cell at `at` (one a subset of the other).
__device__ __forceinline__ int edge_vertex(const MeshArgs& p, int at, int ca, int cb) {
  const int lo = ca < cb ? ca : cb, d = ca ^ cb;
  const int q = corner_at(p, at, lo);
  return p.voff[q] + __popc((unsigned)p.emask[q] & ((1u << d) - 1u));
}

__global__ __launch_bounds__(kBlock) void mesh_emit_kernel(const MeshArgs p) {
  const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (gid >= p.n) return;
  const int at = (int)gid;
  const unsigned em = p.emask[at];
  const int ntri = p.tcount[at];
  if (em == 0u && ntri == 0) return;
  const int i = at % p.nx, j = at / p.nx % p.ny, k = at / p.nx / p.ny;
  if (em != 0u) {
    const float da = p.D[at];
    int o = p.voff[at];
    for (int d = 1; d < 8; ++d) {
      if (!(em >> d & 1u) || o >= p.nv) continue;
      const float db = p.D[corner_at(p, at, d)];
      const float t = __fdiv_rn(da, __fsub_rn(da, db));
      const float fi = (d & 1) ? __fadd_rn((float)i, t) : (float)i;
      const float fj = (d & 2) ? __fadd_rn((float)j, t) : (float)j;
      const float fk = (d & 4) ? __fadd_rn((float)k, t) : (float)k;
      p.vertices[3 * (size_t)o + 0] = __fadd_rn(p.ox, __fmul_rn(p.s, fi));
      p.vertices[3 * (size_t)o + 1] = __fadd_rn(p.oy, __fmul_rn(p.s, fj));
      p.vertices[3 * (size_t)o + 2] = __fadd_rn(p.oz, __fmul_rn(p.s, fk));
      ++o;
    }
  }
  if (ntri == 0) return;
  const int mask = cell_mask(p, at);
  int o = p.toff[at];
  for (int t = 0; t < 6; ++t) {
    bool odd;
    const unsigned corners = tet_corners(t, &odd);
    const unsigned in4 = tet_inside(corners, mask);
    if (in4 == 0u || in4 == 15u) continue;
    int n_in;
    const unsigned perm = order_by_side(in4, &n_in);
    if (o + (n_in == 2 ? 2 : 1) > p.nt) return;
    const int c0 = corners >> (4 * (perm & 3u)) & 7u, c1 = corners >> (4 * (perm >> 2 & 3u)) & 7u;
    const int c2 = corners >> (4 * (perm >> 4 & 3u)) & 7u, c3 = corners >> (4 * (perm >> 6 & 3u)) & 7u;
    int* tri = p.triangles + 3 * (size_t)o;
    if (n_in == 2) {
      // insides (c0, c1), outsides (c2, c3): the quad v02 v03 v13 v12, split along v02 - v13
      const bool flip = ((((perm & 3u) + (perm >> 2 & 3u) + 1u) & 1u) != 0u) != odd;
      const int v02 = edge_vertex(p, at, c0, c2), v03 = edge_vertex(p, at, c0, c3);
      const int v13 = edge_vertex(p, at, c1, c3), v12 = edge_vertex(p, at, c1, c2);
      tri[0] = v02; tri[1] = flip ? v13 : v03; tri[2] = flip ? v03 : v13;
      tri[3] = v02; tri[4] = flip ? v12 : v13; tri[5] = flip ? v13 : v12;
      o += 2;
    } else {
      // the lone corner (inside if n_in == 1, else outside) is the apex; the triangle (v1, v2, v3) of the other corners in
      // order has its normal away from the apex iff the apex's position and the tetrahedron's orientation are both even or odd
      const int apex = n_in == 1 ? c0 : c3, apex_pos = n_in == 1 ? (int)(perm & 3u) : (int)(perm >> 6 & 3u);
      const int b1 = n_in == 1 ? c1 : c0, b2 = n_in == 1 ? c2 : c1, b3 = n_in == 1 ? c3 : c2;
      const bool away = ((apex_pos & 1) != 0) == odd;
      const bool flip = n_in == 1 ? !away : away;
      const int v1 = edge_vertex(p, at, apex, b1), v2 = edge_vertex(p, at, apex, b2), v3 = edge_vertex(p, at, apex, b3);
      tri[0] = v1; tri[1] = flip ? v3 : v2; tri[2] = flip ? v2 : v3;
      o += 1;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- colour
struct ColourArgs {
  const float* vertices;
  const float* depth[kChunk];
  const unsigned char* image[kChunk];
  float cam[kChunk][kCamFloats];
  float* acc;                 // [n][4] running sums r, g, b, count
  unsigned char* rgb;         // written when `last`
  long long n;
  int nviews, h, w, last;
  float tau;
};

__global__ __launch_bounds__(kBlock) void mesh_colour_kernel(const ColourArgs p) {
  const long long at = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (at >= p.n) return;
  const float x = p.vertices[3 * at], y = p.vertices[3 * at + 1], z = p.vertices[3 * at + 2];
  float4 a = reinterpret_cast<const float4*>(p.acc)[at];
  for (int v = 0; v < p.nviews; ++v) {
    int texel;
    float zc;
    if (!project(p.cam[v], p.h, p.w, x, y, z, &texel, &zc)) continue;
    const float d = p.depth[v][texel];
    if (!isfinite(d) || !(d > 0.f)) continue;
    if (!(fabsf(__fsub_rn(d, zc)) <= p.tau)) continue;
    const unsigned char* c = p.image[v] + 3 * (size_t)texel;
    a.x = __fadd_rn(a.x, (float)c[0]);
    a.y = __fadd_rn(a.y, (float)c[1]);
    a.z = __fadd_rn(a.z, (float)c[2]);
    a.w = __fadd_rn(a.w, 1.f);
  }
  if (!p.last) {
    reinterpret_cast<float4*>(p.acc)[at] = a;
    return;
  }
  unsigned char r = 128, g = 128, b = 128;
  if (a.w > 0.f) {
    r = (unsigned char)floorf(__fadd_rn(__fdiv_rn(a.x, a.w), 0.5f));
    g = (unsigned char)floorf(__fadd_rn(__fdiv_rn(a.y, a.w), 0.5f));
    b = (unsigned char)floorf(__fadd_rn(__fdiv_rn(a.z, a.w), 0.5f));
  }
  p.rgb[3 * at] = r;
  p.rgb[3 * at + 1] = g;
  p.rgb[3 * at + 2] = b;
}

inline bool finite_host(float v) { return v - v == 0.f; }   // host code: false for NaN and the infinities
inline long long align16(long long b) { return (b + 15) & ~15ll; }

int check_volume(const int* dims, const float* origin, float voxel) {
  MDF_REQUIRE(dims && origin, "null pointer argument");
  MDF_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "dims=(%d,%d,%d): every side needs at least one lattice point", dims[0],
              dims[1], dims[2]);
  MDF_REQUIRE((long long)dims[0] * dims[1] * dims[2] < (1ll << 31), "dims=(%d,%d,%d): 2^31 lattice points or more", dims[0], dims[1],
              dims[2]);
  MDF_REQUIRE(voxel > 0.f && finite_host(voxel), "voxel=%g must be finite and > 0", (double)voxel);
  MDF_REQUIRE(finite_host(origin[0]) && finite_host(origin[1]) && finite_host(origin[2]), "origin is not finite");
  return MDF_OK;
}

int check_views(const float* const* depths, const float* cams, int nviews, int h, int w, float tau) {
  MDF_REQUIRE(depths && cams, "null pointer argument");
  MDF_REQUIRE(nviews >= 1, "nviews=%d: at least one view is needed", nviews);
  MDF_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < (1ll << 31) / 3, "bad depth map shape %dx%d", h, w);
  MDF_REQUIRE(tau > 0.f && finite_host(tau), "trunc=%g must be finite and > 0", (double)tau);
  for (int v = 0; v < nviews; ++v) MDF_REQUIRE(depths[v], "depths[%d] is null", v);
  return MDF_OK;
}

// Workspace of the extraction: marks [8N] | voff [N] i32 | toff [N] i32 | tcount [N] | emask [N] | chunk sums [2][nchunk] i32 |
// chunk offsets [2][nchunk] i64   (each 16-byte aligned; MDF_MESH_WORKSPACE_BYTES bounds it)
void mesh_layout(MeshArgs* m, char* ws) {
  long long o = 0;
  auto take = [&](long long bytes) { const long long at = o; o += align16(bytes); return ws + at; };
  m->nchunk = (int)((m->n + kMeshChunk - 1) / kMeshChunk);
  m->marks = reinterpret_cast<unsigned char*>(take(m->n * 8));
  m->voff = reinterpret_cast<int*>(take(m->n * 4));
  m->toff = reinterpret_cast<int*>(take(m->n * 4));
  m->tcount = reinterpret_cast<unsigned char*>(take(m->n));
  m->emask = reinterpret_cast<unsigned char*>(take(m->n));
  m->chunk_sums = reinterpret_cast<int*>(take(2ll * m->nchunk * 4));
  m->chunk_off = reinterpret_cast<long long*>(take(2ll * m->nchunk * 8));
}

int mesh_args(MeshArgs* m, const float* D, const float* W, const int* dims, const float* origin, float voxel, float min_weight,
              void* workspace, long long workspace_bytes) {
  MDF_REQUIRE(D && W && workspace, "null pointer argument");
  if (int rc = check_volume(dims, origin, voxel)) return rc;
  MDF_REQUIRE(min_weight > 0.f && finite_host(min_weight), "min_weight=%g must be finite and > 0", (double)min_weight);
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
  m->D = D; m->W = W;
  m->nx = dims[0]; m->ny = dims[1]; m->nz = dims[2];
  m->n = (long long)dims[0] * dims[1] * dims[2];
  m->ox = origin[0]; m->oy = origin[1]; m->oz = origin[2]; m->s = voxel; m->min_weight = min_weight;
  MDF_REQUIRE(workspace_bytes >= MDF_MESH_WORKSPACE_BYTES(m->n), "workspace of %lld bytes, %lld needed", workspace_bytes,
              (long long)MDF_MESH_WORKSPACE_BYTES(m->n));
  mesh_layout(m, static_cast<char*>(workspace));
  return MDF_OK;
}

}  // namespace

extern "C" int mdf_tsdf_integrate(float* D, float* W, const int* dims, const float* origin, float voxel, float trunc,
                                  const float* const* depths, const float* cams, int nviews, int h, int w, int chunk, void* stream) {
  MDF_REQUIRE(D && W, "null pointer argument");
  if (int rc = check_volume(dims, origin, voxel)) return rc;
  if (int rc = check_views(depths, cams, nviews, h, w, trunc)) return rc;
  MDF_REQUIRE(chunk >= 0 && chunk <= kChunk, "chunk=%d out of range [0,%d] (0 = the default, %d)", chunk, kChunk, kChunk);
  if (chunk == 0) chunk = kChunk;
  IntegrateArgs p{};
  p.D = D; p.W = W; p.h = h; p.w = w;
  p.nx = dims[0]; p.ny = dims[1]; p.nz = dims[2];
  p.ox = origin[0]; p.oy = origin[1]; p.oz = origin[2]; p.s = voxel; p.tau = trunc;
  p.cull = mdf::env_flag("MDF_TSDF_CULL", true) ? 1 : 0;    // 0: no brick skips a view (the bit-identity checker; read per call)
  const dim3 grid((p.nx + kBx - 1) / kBx, (p.ny + kBy - 1) / kBy, (p.nz + kBz - 1) / kBz);
  MDF_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "dims=(%d,%d,%d): too many bricks along y or z", p.nx, p.ny, p.nz);
  for (int v0 = 0; v0 < nviews; v0 += chunk) {
    p.nviews = nviews - v0 < chunk ? nviews - v0 : chunk;
    for (int v = 0; v < p.nviews; ++v) {
      p.depth[v] = depths[v0 + v];
      for (int k = 0; k < kCamFloats; ++k) p.cam[v][k] = cams[(size_t)(v0 + v) * kCamFloats + k];
    }
    hipLaunchKernelGGL(tsdf_integrate_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, p);
    if (int rc = mdf::check_launch("tsdf_integrate_kernel")) return rc;
  }
  return MDF_OK;
}

extern "C" int mdf_mesh_count(const float* D, const float* W, const int* dims, const float* origin, float voxel, float min_weight,
                              void* workspace, long long workspace_bytes, long long* totals, void* stream) {
  MDF_REQUIRE(totals, "null pointer argument");
  MeshArgs m{};
  if (int rc = mesh_args(&m, D, W, dims, origin, voxel, min_weight, workspace, workspace_bytes)) return rc;
  m.totals = totals;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(m.marks, 0, (size_t)m.n * 8, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemsetAsync failed");
  const dim3 per_point((unsigned)((m.n + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(mesh_count_kernel, per_point, dim3(kBlock), 0, s, m);
  if (int rc = mdf::check_launch("mesh_count_kernel")) return rc;
  hipLaunchKernelGGL(mesh_scan_kernel<0>, dim3(m.nchunk), dim3(kBlock), 0, s, m);
  if (int rc = mdf::check_launch("mesh_scan_kernel")) return rc;
  hipLaunchKernelGGL(mesh_scan_kernel<1>, dim3(2), dim3(mdf::kScanThreads), 0, s, m);
  if (int rc = mdf::check_launch("mesh_scan_kernel")) return rc;
  hipLaunchKernelGGL(mesh_scan_kernel<2>, dim3(m.nchunk), dim3(kBlock), 0, s, m);
  return mdf::check_launch("mesh_scan_kernel");
}

extern "C" int mdf_mesh_emit(const float* D, const float* W, const int* dims, const float* origin, float voxel, float min_weight,
                             void* workspace, long long workspace_bytes, long long n_vertices, long long n_triangles,
                             float* vertices, int* triangles, void* stream) {
  MDF_REQUIRE(vertices && triangles, "null pointer argument");
  MeshArgs m{};
  if (int rc = mesh_args(&m, D, W, dims, origin, voxel, min_weight, workspace, workspace_bytes)) return rc;
  MDF_REQUIRE(n_vertices >= 1 && n_triangles >= 1, "n_vertices=%lld, n_triangles=%lld: an empty mesh needs no emit call", n_vertices,
              n_triangles);
  if (n_vertices >= (1ll << 31) || n_triangles >= (1ll << 31))
    return mdf::fail(MDF_EUNSUPPORTED, "%lld vertices, %lld triangles: indices are int32; use a coarser volume", n_vertices, n_triangles);
  m.vertices = vertices;
  m.triangles = triangles;
  m.nv = n_vertices;
  m.nt = n_triangles;
  hipLaunchKernelGGL(mesh_emit_kernel, dim3((unsigned)((m.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, m);
  return mdf::check_launch("mesh_emit_kernel");
}

extern "C" int mdf_mesh_colour(const float* vertices, long long n, const float* const* depths, const unsigned char* const* images,
                               const float* cams, int nviews, int h, int w, float trunc, float* acc, unsigned char* rgb,
                               void* stream) {
  MDF_REQUIRE(vertices && images && acc && rgb, "null pointer argument");
  MDF_REQUIRE(n >= 1 && n < (1ll << 31), "n=%lld vertices out of range [1,2^31)", n);
  if (int rc = check_views(depths, cams, nviews, h, w, trunc)) return rc;
  for (int v = 0; v < nviews; ++v) MDF_REQUIRE(images[v], "images[%d] is null", v);
  MDF_REQUIRE(reinterpret_cast<uintptr_t>(acc) % 16 == 0, "acc must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(acc, 0, (size_t)n * 16, s) != hipSuccess) return mdf::fail(MDF_EHIP, "hipMemsetAsync failed");
  ColourArgs p{};
  p.vertices = vertices; p.acc = acc; p.rgb = rgb; p.n = n; p.h = h; p.w = w; p.tau = trunc;
  for (int v0 = 0; v0 < nviews; v0 += kChunk) {
    p.nviews = nviews - v0 < kChunk ? nviews - v0 : kChunk;
    p.last = v0 + kChunk >= nviews;
    for (int v = 0; v < p.nviews; ++v) {
      p.depth[v] = depths[v0 + v];
      p.image[v] = images[v0 + v];
      for (int k = 0; k < kCamFloats; ++k) p.cam[v][k] = cams[(size_t)(v0 + v) * kCamFloats + k];
    }
    hipLaunchKernelGGL(mesh_colour_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, p);
    if (int rc = mdf::check_launch("mesh_colour_kernel")) return rc;
  }
  return MDF_OK;
}
