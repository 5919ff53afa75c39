// The layout of a packed conv weight set, once: what the pack kernels (conv_pack.hip) write and where every reader finds its
// segment.  Plain constexpr C++17 with no HIP include, so the pack kernels and a host-only translation unit can both use it.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MDF_HD __host__ __device__
#else
#define MDF_HD
#endif

namespace mdf {

MDF_HD constexpr int padded_cin(int c) { return c <= 4 ? 4 : c; }
MDF_HD constexpr int rw_of(int Cout) { return Cout == 8 ? 2 : (Cout == 4 ? 4 : 0); }   // w-phase factor of a stride-1 k3 layer (0 = none)
MDF_HD constexpr bool wino_built(int Cin, int Cout) {   // 3-D ((16, 32): the input-gradient conv of the stage-0 regulariser's first layer, training)
  return ((Cout == 16 || Cout == 32) && (Cin == 16 || Cin == 32)) || (Cin == 16 && Cout == 8);
}
MDF_HD constexpr bool wino2d_built(int Cin, int Cout) {   // ((16, 32), (32, 64): input gradients of the k5-s2 layers as 3x3 convs over the parity classes, training)
  return (Cin == 16 && Cout == 16) || (Cin == 32 && Cout == 32) || (Cin == 64 && Cout == 64) || (Cin == 16 && Cout == 32) || (Cin == 32 && Cout == 64);
}
MDF_HD constexpr bool wd_built(int Cin, int Cout) { return Cout == 8 && (Cin == 8 || Cin == 16); }   // 3-D, depth-pair Winograd
// 2-D k5 s2 layers that also run as a Winograd 3x3 conv over the four parity images of their input (conv_lds.hip, LdsConvParams::s2d)
MDF_HD constexpr bool k5w_built(int Cin, int Cout) { return (Cin == 32 && Cout == 64) || (Cin == 16 && Cout == 32) || (Cin == 8 && Cout == 16); }

// One complete packed weight set, as mdf_conv3d_pack_weights / mdf_conv_pack_weights lay it out: the plain fragments, then
// (Cout 8 / 4, 3x3 taps) the w-phase fragments, then (where a Winograd kernel exists) the transform-domain fragments, then (3-D,
// Cout 8) the depth-pair Winograd fragments; or the transposed-conv fragments alone (as `plain`).  Lengths in floats, 0 = absent.
// The ABI passes a packed set without its length: a reader takes its pointer from here and does not launch on a length of 0.
struct PackLayout {
  long long plain, rw, wino, wd;
  MDF_HD constexpr long long total() const { return plain + rw + wino + wd; }
  MDF_HD constexpr long long rw_off() const { return plain; }
  MDF_HD constexpr long long wino_off() const { return plain + rw; }
  MDF_HD constexpr long long wd_off() const { return plain + rw + wino; }
};

MDF_HD constexpr PackLayout pack_layout(int is3d, int transposed, int Cin_mem, int Cout, int ntaps) {
  const int Cin = padded_cin(Cin_mem);
  const int KPL = (Cin >= 16) ? 4 : (Cin == 8 ? 2 : 1), NCH = Cin / (4 * KPL);
  PackLayout L{0, 0, 0, 0};
  if (transposed) {
    const int K2 = (Cin >= 16) ? 4 : 2;
    L.plain = 18ll * (Cin / (4 * K2)) * ((2 * Cout + 15) / 16) * 64 * K2;
    return L;
  }
  L.plain = (long long)ntaps * NCH * ((Cout + 15) / 16) * 64 * KPL;
  const bool k3 = is3d ? (ntaps == 27) : (ntaps == 9);
  if (k3 && rw_of(Cout)) L.rw = (long long)(is3d ? 9 : 3) * (3 + rw_of(Cout) - 1) * NCH * 64 * KPL;
  if (k3 && (is3d ? wino_built(Cin_mem, Cout) : wino2d_built(Cin_mem, Cout))) L.wino = (long long)(is3d ? 3 : 1) * (Cin / 16) * 16 * ((Cout + 15) / 16) * 64 * 4;
  if (k3 && is3d && wd_built(Cin_mem, Cout)) L.wd = 4ll * NCH * 16 * 64 * KPL;
  if (!is3d && ntaps == 25 && k5w_built(Cin_mem, Cout)) L.wino = (long long)(4 * Cin / 16) * 16 * ((Cout + 15) / 16) * 64 * 4;   // (its only extra segment)
  return L;
}

// The offsets the readers carried as literals before this header existed, for the shapes that reach each reader.
namespace pack_layout_check {
constexpr long long up16(int c) { return ((c + 15) / 16) * 16; }
// w-phase readers (conv_lds.hip: the Rw / RwT rows): kd*k*k*ci*16
static_assert(pack_layout(1, 0, 16, 8, 27).rw_off() == 27 * 16 * 16 && pack_layout(1, 0, 16, 8, 27).rw > 0, "rw 3-D 16->8");
static_assert(pack_layout(1, 0, 8, 8, 27).rw_off() == 27 * 8 * 16 && pack_layout(1, 0, 8, 8, 27).rw > 0, "rw 3-D 8->8");
static_assert(pack_layout(0, 0, 16, 4, 9).rw_off() == 9 * 16 * 16 && pack_layout(0, 0, 16, 4, 9).rw > 0, "rw 2-D 16->4");
static_assert(pack_layout(0, 0, 8, 4, 9).rw_off() == 9 * 8 * 16 && pack_layout(0, 0, 8, 4, 9).rw > 0, "rw 2-D 8->4");
static_assert(pack_layout(0, 0, 8, 8, 9).rw_off() == 9 * 8 * 16 && pack_layout(0, 0, 8, 8, 9).rw > 0, "rw 2-D 8->8");
static_assert(pack_layout(0, 0, 3, 8, 9).rw_off() == 9 * 4 * 16 && pack_layout(0, 0, 3, 8, 9).rw > 0, "rw 2-D image layer, 3 channels");
static_assert(pack_layout(0, 0, 1, 8, 9).rw_off() == 9 * 4 * 16 && pack_layout(0, 0, 1, 8, 9).rw > 0, "rw 2-D image layer, 1 channel");
// 3-D Winograd (the Wg3 rows): 27*ci*up16(co) + (co == 8 ? 36*ci*16 : 0)
constexpr bool wg_ok(int ci, int co) {
  return pack_layout(1, 0, ci, co, 27).wino_off() == 27 * ci * up16(co) + (co == 8 ? 36 * ci * 16 : 0) && pack_layout(1, 0, ci, co, 27).wino > 0;
}
static_assert(wg_ok(16, 16) && wg_ok(32, 16) && wg_ok(32, 32) && wg_ok(16, 8) && wg_ok(16, 32), "3-D Winograd segment");
// 2-D Winograd (the Wg2 rows, and mdf_wino2d_dispatch over the same sets): 9*ci*up16(co)
constexpr bool wg2_ok(int ci, int co) { return pack_layout(0, 0, ci, co, 9).wino_off() == 9 * ci * up16(co) && pack_layout(0, 0, ci, co, 9).wino > 0; }
static_assert(wg2_ok(16, 16) && wg2_ok(32, 32) && wg2_ok(64, 64) && wg2_ok(16, 32) && wg2_ok(32, 64), "2-D Winograd segment");
// depth-pair Winograd (the Wd / WdStream rows): 27*ci*16 + 36*ci*16 + (ci == 16 ? 3*16*64*4 : 0)
static_assert(pack_layout(1, 0, 8, 8, 27).wd_off() == 27 * 8 * 16 + 36 * 8 * 16 && pack_layout(1, 0, 8, 8, 27).wd > 0, "depth-pair 8->8");
static_assert(pack_layout(1, 0, 16, 8, 27).wd_off() == 27 * 16 * 16 + 36 * 16 * 16 + 3 * 16 * 64 * 4 && pack_layout(1, 0, 16, 8, 27).wd > 0, "depth-pair 16->8");
// k5 s2 over the parity images, wino2d.hip form: 25 taps x NCH x NT x 64 lanes x KPL
static_assert(pack_layout(0, 0, 32, 64, 25).wino_off() == 25 * 64 * (2 * 4 * 4) && pack_layout(0, 0, 32, 64, 25).wino > 0, "k5 s2 32->64");
static_assert(pack_layout(0, 0, 16, 32, 25).wino_off() == 25 * 64 * (2 * 4) && pack_layout(0, 0, 16, 32, 25).wino > 0, "k5 s2 16->32");
static_assert(pack_layout(0, 0, 8, 16, 25).wino_off() == 25 * 64 * (1 * 2) && pack_layout(0, 0, 8, 16, 25).wino > 0, "k5 s2 8->16");
// k5 s2 16 -> 32, conv_lds.hip form: 25*1*2*64*4
static_assert(pack_layout(0, 0, 16, 32, 25).wino_off() == 25 * 1 * 2 * 64 * 4, "k5 s2 16->32 (LDS kernel)");
// mdf_wino3d_dispatch (Cout % 16 == 0): 27*Cin*Cout
constexpr bool w3_ok(int ci, int co) { return pack_layout(1, 0, ci, co, 27).wino_off() == 27 * ci * co && pack_layout(1, 0, ci, co, 27).wino > 0; }
static_assert(w3_ok(16, 16) && w3_ok(32, 16) && w3_ok(32, 32) && w3_ok(16, 32), "3-D Winograd segment of the Cout %% 16 == 0 sets");
// prob_fused.hip (cin 16 or 8, cout 4): 9*Cin*16;  conv_pair.hip (image layer 3 -> 8, then 8 -> 8) and res_pair.hip (8 -> 8): 9*4*16, 9*8*16
static_assert(pack_layout(0, 0, 16, 4, 9).rw_off() == 9 * 16 * 16 && pack_layout(0, 0, 8, 4, 9).rw_off() == 9 * 8 * 16, "prob head sets");
static_assert(pack_layout(0, 0, 3, 8, 9).rw_off() == 9 * 4 * 16 && pack_layout(0, 0, 8, 8, 9).rw_off() == 9 * 8 * 16, "pair-kernel sets");
// the transposed set stands alone
static_assert(pack_layout(1, 1, 16, 8, 27).total() == pack_layout(1, 1, 16, 8, 27).plain, "transposed: one segment");
}  // namespace pack_layout_check

}  // namespace mdf
