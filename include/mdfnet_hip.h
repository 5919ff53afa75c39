/*
 * mdfnet_hip.h -- C ABI of the MI355X (gfx950) kernels behind MDF-Net's multi-stage MVS hot path.
 *
 * The reference (zongh5a/MDF-Net) has no FFI on this path: every operator is a chain of stock
 * PyTorch ops.  Each entry point below replaces one such chain; the reference interface it
 * replaces is cited as file:line (paths relative to the reference root).
 *
 * Conventions (all entry points)
 *   - Plain pointers and sizes only.  Every `const float*` / `float*` is DEVICE memory unless the
 *     parameter comment says HOST.  The caller (PyTorch) owns every buffer; the library never
 *     allocates, frees or retains device memory.
 *   - Asynchronous: work is enqueued on `stream` (a hipStream_t passed as void*); no implicit
 *     synchronisation.  Re-entrant; callable from several host threads / one process per GPU.
 *   - Return 0 on success; <0 on failure: MDF_EARG (-1) bad argument/shape, MDF_EUNSUPPORTED (-2)
 *     configuration not built, MDF_EHIP (-3) HIP runtime error.  mdf_last_error() returns a
 *     thread-local message valid until the next call on that thread.  Never aborts.
 *   - fp32 everywhere.  "Bit-exact" below means bit-identical to torch-2.10 CPU on the same inputs.
 */
#ifndef MDFNET_HIP_H
#define MDFNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDF_ABI_VERSION 1

#define MDF_OK 0
#define MDF_EARG (-1)
#define MDF_EUNSUPPORTED (-2)
#define MDF_EHIP (-3)

/* feature-map layouts ([B,C,h,w] logical) */
#define MDF_FEA_NCHW 0
#define MDF_FEA_NHWC 1
/* volume layouts ([B,C,D,h,w] logical) */
#define MDF_VOL_NCDHW 0
#define MDF_VOL_NDHWC 1

#define MDF_MAX_SRC_VIEWS 16
#define MDF_MAX_FUSE_VIEWS 1024   /* views of one scan in mdf_consensus_fuse_fwd's camera table */

int mdf_abi_version(void);
const char* mdf_last_error(void);
/* Name of the __global__ function the calling thread's most recent entry enqueued last ("" before the first launch): lets a
 * profiler attribute an entry's algorithmic bytes / flops to the kernel that served it (bench.py: roofline.per_kernel).      */
const char* mdf_last_launch(void);
/* The conv kernels keep one device-side work-item counter pair per HIP stream that has launched them (128 slots per
 * process; launches on one stream are ordered, launches on different streams may overlap).  A long-lived process that
 * destroys streams hands their slots back with this call (before hipStreamDestroy, with no conv launch of this library
 * still running on the stream).  Always returns MDF_OK; unknown streams are ignored.                               */
int mdf_release_stream(void* stream);

/* ---- a4  homo_warping (net/unit/base.py:85-126) ---------------------------------------------
 * Plane-sweep homography warp of ONE source feature map; bilinear, zero padding, the reference's
 * mixed align_corners convention (ix = px*w/(w-1) - 0.5).  Output values are bit-exact.
 *   src_fea  [B,h,w,C] (MDF_FEA_NHWC) ; C in {16,32,64}
 *   proj     [B,12]  rows of (src_proj @ inverse(ref_proj))[:3,:4], computed by the host with the
 *            same torch call as base.py:98 so kernel and oracle consume identical floats
 *   hypos    [B,D] (hypos_per_pixel=0; reference shape [B,D,1,1]) or [B,D,h,w] (=1)
 *   out      [B,C,D,h,w] (MDF_VOL_NCDHW) or [B,D,h,w,C] (MDF_VOL_NDHWC)                         */
int mdf_homo_warp_fwd(const float* src_fea, int fea_layout, const float* proj, const float* hypos,
                      int hypos_per_pixel, float* out, int out_layout, int B, int C, int D, int h, int w,
                      void* stream);

/* Test hook for "indexing bit-exact": integer corner (floor) of every sample position.
 *   x0y0 [B,D,h,w,2] int32 = (floor(ix), floor(iy)); INT32_MIN for non-finite positions,
 *   clamped to +-2^30.  Same device function as the kernels above/below.                        */
int mdf_warp_corner_indices(const float* proj, const float* hypos, int hypos_per_pixel, int32_t* x0y0,
                            int B, int D, int h, int w, void* stream);

/* ---- a5  VectorAggregate.forward, eval mode (net/unit/homoaggregate.py:25-46) ----------------
 * Fused warp + group softmax + similarity + learned view weight + weighted mean over views.
 * Fills CoreNet's Homoaggre[s] slot (net/core.py:58).  C/G must be 2 (config.py:196,205).
 *   ref_fea   [B,h,w,C] NHWC
 *   src_feas  HOST array of n_src DEVICE pointers, each [B,h,w,C] NHWC
 *   proj      [n_src,B,12]
 *   w_params  [G+4] = depth_weight.0.conv.weight[G], alpha, beta, w2, b2 where BatchNorm3d(1) is
 *             folded as ATen does in eval: alpha = gamma/sqrt(var+eps), beta = bias - mean*alpha
 *   cost      [B,G,D,h,w] (NCDHW) or [B,D,h,w,G] (NDHWC)                                         */
int mdf_warp_aggregate_vec_fwd(const float* ref_fea, const float* const* src_feas, int fea_layout,
                               const float* proj, const float* hypos, int hypos_per_pixel,
                               const float* w_params, float* cost, int cost_layout, int B, int C, int G,
                               int D, int h, int w, int n_src, void* stream);

/* ---- a5d The same operator over PAIR-DIFFERENCE maps (eval).  With C/G = 2 the operator uses a feature
 * pair only through softmax(a, b)[0] = 1 / (1 + exp(b - a)), and bilinear sampling is linear, so it can
 * be fed d[g] = f[2g+1] - f[2g] (G channels) instead of f (C = 2G channels): half the tap bytes, half
 * the blends.  Same sample positions and weights, same arithmetic from the similarity on; the result
 * differs from mdf_warp_aggregate_vec_fwd by the rounding of the blend only.
 *   ref_diff  [B,h,w,G] NHWC;  src_diffs  HOST array of n_src DEVICE pointers, each [B,h,w,G] NHWC
 *   G in {8,16,32}; every other argument as mdf_warp_aggregate_vec_fwd                            */
int mdf_warp_aggregate_pairdiff_fwd(const float* ref_diff, const float* const* src_diffs, int fea_layout,
                                    const float* proj, const float* hypos, int hypos_per_pixel,
                                    const float* w_params, float* cost, int cost_layout, int B, int G, int D,
                                    int h, int w, int n_src, void* stream);

/* ---- a5' homo_aggregate_by_variance (net/unit/homoaggregate.py:49-69) ------------------------
 * var = E[x^2] - E[x]^2 over {ref, softmax_C(warped src_v)}.  cost has C channels.               */
int mdf_warp_aggregate_var_fwd(const float* ref_fea, const float* const* src_feas, int fea_layout,
                               const float* proj, const float* hypos, int hypos_per_pixel, float* cost,
                               int cost_layout, int B, int C, int D, int h, int w, int n_src, void* stream);

/* ---- a6/a7/a8  3-D convolution layers of the regularisers (net/unit/regular.py:9-133,
 *      net/unit/base.py:50-68): Conv3d / ConvTranspose3d, k=3, pad=1, (output_padding=1), no bias,
 *      optional folded BatchNorm3d (alpha,beta per output channel), ReLU and residual add, in that
 *      order:  y = [res +] [relu] (conv(x) * alpha + beta).  fp32 MFMA (exact f32 fma chain).
 *   x        [B,Di,Hi,Wi,Cin]  NDHWC
 *   wpack    weights pre-packed by mdf_conv3d_pack_weights (device)
 *   alpha,beta [Cout] or NULL (no BN);  res [B,Do,Ho,Wo,Cout] or NULL
 *   y        [B,Do,Ho,Wo,Cout] NDHWC.   stride in {1,2}; transposed in {0,1} (transposed => stride 2)
 *   Cin,Cout in {8,16,32,64}                                                                      */
int mdf_conv3d_fwd(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res,
                   float* y, int B, int Di, int Hi, int Wi, int Cin, int Cout, int stride, int transposed,
                   int relu, void* stream);

/* The depth-preserving sampling layers of RegularNet_4Scales(sample_stride=(1,2,2), sample_padding=(0,1,1))
 * (net/unit/regular.py:76-77), same operands, layouts, epilogue and return codes as mdf_conv3d_fwd:
 *   transposed = 0: Conv3d(k3, stride (1,2,2), pad 1)            Do = Di, Ho = (Hi-1)/2+1, Wo = (Wi-1)/2+1
 *   transposed = 1: ConvTranspose3d(k3, stride (1,2,2), pad 1, output_padding (0,1,1))   Do = Di, Ho = 2Hi, Wo = 2Wi
 *   wpack    from mdf_conv3d_pack_weights with the same `transposed` (no packing of its own)
 *   (Cin,Cout) in {(8,16),(16,32),(32,64)} (transposed = 0), {(64,32),(32,16),(16,8)} (transposed = 1).  Eval only. */
int mdf_conv3d_hw2_fwd(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res,
                       float* y, int B, int Di, int Hi, int Wi, int Cin, int Cout, int transposed, int relu,
                       void* stream);

/* Packed-weight size in floats for a (Cin,Cout) k=3 layer. */
int64_t mdf_conv3d_packed_size(int Cin, int Cout);
/* Re-order torch weights into the MFMA B-fragment order (device -> device, on `stream`).
 *   w: Conv3d [Cout,Cin,3,3,3] (transposed=0) or ConvTranspose3d [Cin,Cout,3,3,3] (transposed=1). */
int mdf_conv3d_pack_weights(const float* w, float* wpack, int Cin, int Cout, int transposed, void* stream);

/* ---- a11/a12  2-D convolution layers of the feature pyramid and refinement net (net/unit/backbone.py:17-45,
 *      net/unit/refine.py:13-21, net/unit/base.py:7-25,71-82): Conv2d k in {1,3,5}, pad (k-1)/2, stride {1,2},
 *      y = [res + res_scale *] ( [up2(res_up) +] [relu]( conv(x) * alpha + beta ) )
 *      (alpha NULL: beta is the conv bias or NULL; res_up [B,Ho/2,Wo/2,Cout]: its bilinear x2 upsample,
 *      align_corners=False, is added -- the FPN top-down step backbone.py:60,62 fused into the lateral conv).
 *   x [B,H,W,Cin] NHWC, or planar [B,Cin,H,W] when planar_in != 0 (Cin < 4 only: the RGB images as eval.py hands
 *   them over, so no layout copy is needed); y [B,Ho,Wo,Cout] NHWC; wpack from mdf_conv_pack_weights (Cin 3 or 1 is
 *   zero-padded to 4).  pixel_shuffle2 != 0 (Cout = 32, or 32 -> 64 with k = 3; stride 1, no residual): y is nn.PixelShuffle(2)
 *   of the result, [B,2Ho,2Wo,Cout/4] NHWC (refine.py:19), and the weight rows must have been packed sub-pixel-major: row
 *   (dy*2+dx)*Cout/4 + oc = torch output channel oc*4 + dy*2 + dx.  (Training uses the same store for the input gradient of the
 *   k5-s2 pyramid layers, a 3x3 conv over dy whose output rows are the four parity classes of dx.)                       */
int mdf_conv2d_fwd(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res,
                   float res_scale, const float* res_up, float* y, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int relu,
                   int planar_in, int pixel_shuffle2, void* stream);
int64_t mdf_conv_packed_size(int Cin, int Cout, int ntaps);
/* w: [Cout,Cin,k,k] (ntaps = k*k) or [Cout,Cin,3,3,3] (ntaps = 27), device -> device. */
int mdf_conv_pack_weights(const float* w, float* wpack, int Cin, int Cout, int ntaps, void* stream);

/* `prob` head: Conv3d(Cin->1,k3,p1,no bias) + softmax over D [+ soft-argmin]  (regular.py:43,69 /
 * :110,133 and net/unit/regress.py:5-7).  x NDHWC [B,D,h,w,Cin]; w [Cin*27] torch order [1,Cin,3,3,3];
 *   prob [B,D,h,w]; depth [B,h,w] or NULL; hypos as above (may be NULL when depth is NULL).       */
int mdf_prob_softmax_regress_fwd(const float* x, const float* w, const float* hypos, int hypos_per_pixel,
                                 float* prob, float* depth, int B, int D, int h, int wd, int Cin, void* stream);
/* Same head in partial-sum form (the fast path): first run mdf_conv2d_fwd over the B*D planes of x ([B*D,h,w,Cin]) with the
 * 2-D weight w2[kd][cin][kh][kw] = w[0][cin][kd][kh][kw], kd = 0..2, plus a 4th all-zero output channel (Cout = 4),
 * giving partials [B,D,h,w,4]; this call then forms logit[d] = P0[d-1] + P1[d] + P2[d+1], the softmax over D and the
 * soft-argmin.  D <= 96.  partials 16-byte aligned.                                                               */
int mdf_prob_from_partials_fwd(const float* partials, const float* hypos, int hypos_per_pixel, float* prob, float* depth,
                               int B, int D, int h, int wd, void* stream);
/* The partial-sum form in ONE launch: a block owns a 4 x 64 pixel tile, walks the depth axis with the MFMA step of that 2-D conv
 * and keeps the partials in registers (they never reach memory).  wpack = mdf_conv_pack_weights of the 4-channel 2-D weight above
 * (Cin_mem = Cin, Cout = 4, 9 taps).  Cin in {8,16}.  Bit-identical to mdf_conv2d_fwd + mdf_prob_from_partials_fwd; parallel over
 * pixels only, so for maps that fill the chip (B*ceil(h/4)*ceil(wd/64) blocks).                                            */
int mdf_prob_fused_fwd(const float* x, const float* wpack, const float* hypos, int hypos_per_pixel, float* prob, float* depth,
                       int B, int D, int h, int wd, int Cin, void* stream);

/* ---- tail of the refinement net as one launch (net/unit/refine.py:18-20,42-44):
 *      y = [lo +] conv2(PixelShuffle(2)(conv1(x))) [* span]     Conv2d(8,32,k3,p1,no bias) -> PixelShuffle(2) -> Conv2d(8,1,k3,p1,no bias)
 *      x NHWC [B,H,W,8]; w1pack = mdf_conv_pack_weights of conv1's weight with its output rows in PixelShuffle order
 *      (row sub*8 + oc <- channel oc*4 + sub); w2 = conv2's weight [1,8,3,3]; lo / span [B] or both NULL (the range mapping
 *      lo + y * span with torch's roundings); y [B,2H,2W].  The 8-channel map at twice the resolution never reaches memory.   */
int mdf_refine_tail_fwd(const float* x, const float* w1pack, const float* w2, const float* lo, const float* span, float* y,
                        int B, int H, int W, void* stream);

/* ---- the two full-resolution layers of the feature pyramid as one launch (net/unit/backbone.py:28, eval):
 *      y = relu(bn2(conv2(relu(bn1(conv1(x))))))   Conv2d(3,8,k3,p1) -> Conv2d(8,8,k3,p1), BatchNorm folded to (alpha, beta);
 *      x planar [N,3,H,W] as the loader hands it over, y NHWC [N,H,W,8]; w1pack / w2pack = mdf_conv_pack_weights of the two
 *      layers.  Bit-identical to the two mdf_conv2d_fwd launches; the 8-channel map between them never reaches memory.    */
int mdf_conv2d_pair_fwd(const float* x, const float* w1pack, const float* alpha1, const float* beta1, const float* w2pack,
                        const float* alpha2, const float* beta2, float* y, int N, int H, int W, void* stream);

/* ---- several 1x1 heads over one input as one launch (the feature pyramid's composed heads, net/unit/backbone.py:58-66, eval):
 *      y[h] = [up2(res_ups[h]) +] W_h x + bias_h  for h < n_heads (2 or 3); x NHWC [B,H,W,Cin], y[h] NHWC [B,H,W,couts[h]],
 *      res_ups[h] [B,H/2,W/2,couts[h]] or NULL (bilinear x2, align_corners=False, added BEFORE nothing else: torch's order
 *      up + conv), biases[h] [couts[h]] or NULL, wpacks[h] = mdf_conv_pack_weights of head h (one tap).  The arrays are HOST arrays
 *      of device pointers.  Built: Cin 64 -> (64, 32, 16) and Cin 32 -> (32, 16), and their pair-difference forms Cin 64 -> (32, 16, 8), Cin 32 -> (16, 8); every output bit-identical to mdf_conv2d_fwd.  */
int mdf_conv1x1_heads_fwd(const float* x, int n_heads, const float* const* wpacks, const float* const* biases,
                          const float* const* res_ups, float* const* ys, const int* couts, int B, int H, int W, int Cin,
                          void* stream);

/* ---- head of the refinement net as one launch (net/unit/refine.py:29,36, eval): y = conv0((depth - lo[b]) / span[b]),
 *      conv0 = Conv2d(1,8,k3,p1,no bias) with `weight` [8,1,3,3] as the module holds it; depth [B,H,W], y NHWC [B,H,W,8];
 *      lo / span [B] or both NULL (no mapping).  torch's roundings (sub, true divide); bit-identical to
 *      mdf_range_affine_fwd(mode 0) + mdf_conv2d_fwd.                                                                     */
int mdf_refine_head_fwd(const float* depth, const float* lo, const float* span, const float* weight, float* y, int B, int H, int W,
                        void* stream);

/* ---- a residual block of the refinement net as one launch (net/unit/base.py:39-47 `Res`, net/unit/refine.py:29,40, eval):
 *      y = x + scale * conv_b(relu(conv_a(x)))   both Conv2d(8,8,k3,p1,no bias); x, y NHWC [N,H,W,8], y != x;
 *      wa_pack / wb_pack = mdf_conv_pack_weights of the two layers.  Bit-identical to the two mdf_conv2d_fwd launches
 *      (relu; then res + scale * conv); the intermediate map never reaches memory.                                      */
int mdf_conv2d_res_pair_fwd(const float* x, const float* wa_pack, const float* wb_pack, float scale, float* y, int N, int H,
                            int W, void* stream);

/* ---- a9  depth_regression (net/unit/regress.py:5-7): depth = sum_d prob*hypos ----------------- */
int mdf_depth_regress_fwd(const float* prob, const float* hypos, int hypos_per_pixel, float* depth, int B, int D,
                          int h, int w, void* stream);

/* ---- a10 confidence_regress (net/unit/regress.py:9-25), n=4, pad=(1,2) ------------------------
 *   conf [B,h,w] = sum prob[idx-1..idx+2], idx = (int64) trunc(sum_d prob_d*d); idx_out int64 or NULL */
int mdf_confidence_fwd(const float* prob, float* conf, int64_t* idx_out, int B, int D, int h, int w, void* stream);
/* the same with the nearest x2 upsampling of net/core.py:76 folded in: conf2 [B,2h,2w]                            */
int mdf_confidence_up2_fwd(const float* prob, float* conf2, int B, int D, int h, int w, void* stream);
/* confidence_regress with the previous stage's confidence (net/unit/regress.py:9-25, all of it), any window of its signature:
 *   cur  = sum prob[idx-pad_front .. idx-pad_front+n-1] (0 outside [0,D), ascending from 0.0f), idx as above; n in {1,2,4,8}
 *   conf = w_last * bicubic_x2(last) + w_cur * cur;  last [B,H/2,W/2] (H, W even) or NULL: conf = cur, which at n=4,
 *          pad_front=1 has the bits of mdf_confidence_fwd (up2: of mdf_confidence_up2_fwd).
 *   bicubic_x2 = ATen upsample_bicubic2d, align_corners=False, scale 2, A=-0.75: taps k-2..k+1 with weights (-0.03515625,
 *          0.26171875, 0.87890625, -0.10546875) at output 2k, taps k-1..k+2 with the reversed weights at 2k+1, tap indices
 *          clamped; per tap row ((p0*c0 + p1*c1) + p2*c2) + p3*c3 along x, the same form along y, then the blend; every
 *          product and sum rounded on its own.  Held to the reference's code in float64, not to ATen's fp32 bits.
 *   up2 != 0: conf [B,2H,2W], every value at its 2x2 pixels (the nearest x2 of net/core.py:76); else conf [B,H,W].       */
int mdf_confidence_cascade_fwd(const float* prob, const float* last, float w_last, float w_cur, int n, int pad_front, int up2,
                               float* conf, int B, int D, int H, int W, void* stream);
/* range mapping around the refinement net (net/unit/refine.py:29,44), per batch item b over n elements:
 *   mode 0: y = (x - lo[b]) / span[b]      mode 1: y = lo[b] + x * span[b]     (torch's separate roundings kept)   */
int mdf_range_affine_fwd(const float* x, const float* lo, const float* span, int mode, float* y, int B, long long n, void* stream);

/* ---- a3  HyposByFit.forward (net/unit/depthhypos.py:27-76) -------------------------------------
 * mode 1 = gauss1 (depthhypos.py:169-215) with hypotheses shared by all pixels: `fit_row` is
 *          row 0 of (X^T X)^-1 X^T, [B,D], computed by the host with the reference's own torch
 *          calls (the 3x3 normal matrix has cond ~1e14 in fp32);
 * mode 2 = laplace (depthhypos.py:78-125), per-pixel or shared hypotheses;
 * mode 3 = gauss0 (depthhypos.py:127-166), per-pixel or shared hypotheses; needs depth and hypos;
 * mode 4 = gauss1 with per-pixel or shared hypotheses; needs hypos, `fit_row` is not used (may be
 *          null).  Modes 3 and 4 fit centred regressors on the device and are held to the
 *          reference's code in float64, not to its fp32 bits (its fp32 3x3 inverse is noise for
 *          per-pixel hypotheses); a pixel with fewer than 2 distinct (x - depth)^2 (mode 3) or
 *          fewer than 3 distinct hypotheses (mode 4) gets s = NaN.
 * Step 1: s [B,h,w].  Step 2 (mode 1 for every Gaussian curve, 2 for laplace): bilinear x2
 * upsample of s and depth (align_corners=False), range
 * from the curve, clamps, D_out hypotheses per pixel -> hypos_out [B,D_out,2h,2w].
 *   range [B,2] = (depth_min, depth_max) as float32;  log_thresh = f32 ln(prob_thresh), computed by
 *   the host with torch.log (depthhypos.py:55,57) so it carries the reference's rounding.          */
int mdf_hypos_fit_fwd(int mode, const float* prob, const float* depth, const float* hypos, int hypos_per_pixel,
                      const float* fit_row, float* s_out, int B, int D, int h, int w, void* stream);
int mdf_hypos_from_fit_fwd(int mode, const float* s, const float* depth, const float* range, float log_thresh,
                           float* hypos_out, int B, int D_out, int h, int w, int upsample, void* stream);

/* ---- a3''' atv_hypos (net/unit/depthhypos.py:218-253): the adaptive-thin-volume range of UCS-Net, the baseline the curve fits
 *      are compared with; HyposByFit's fourth curve, "atv".
 * mdf_atv_spread_fwd: spread [B,h,w] = scale * sqrt(sum_d prob_d (hypos_d - depth)^2), the exp_variance atv_hypos takes (nothing
 *      in the reference computes it).  prob [B,D,h,w]; depth [B,h,w]; hypos as above; scale finite and > 0 (UCS-Net: 1.5).
 *      Held to the formula in float64 on the same inputs: (D/2 + 4) * 2^-24 relative; a sum of exact zeros gives exactly 0.
 * mdf_atv_hypos_fwd: e2, d2 = bilinear x2 of spread, depth (align_corners=False; upsample == 0: the maps as they are);
 *      low = -min(d2, e2); step = (e2 - low) / (D_out - 1); hypos_out[i] = ((d2 + low) + step * i) + 1e-12 -> [B,D_out,2h,2w]
 *      (or [B,D_out,h,w]), the reference's fp32 bits.  D_out >= 2.  NOT clamped to the depth range (the reference has no
 *      clamp): the hypotheses can leave [depth_min, depth_max]; every one is >= 1e-12.                                     */
int mdf_atv_spread_fwd(const float* prob, const float* depth, const float* hypos, int hypos_per_pixel, float scale,
                       float* spread_out, int B, int D, int h, int w, void* stream);
int mdf_atv_hypos_fwd(const float* spread, const float* depth, float* hypos_out, int B, int D_out, int h, int w, int upsample,
                      void* stream);

/* ---- N1  depth-map consistency filter + fusion (tools/filter/dynamic_filter_gpu.py:63-103,166-238) ----------
 * One fused pass over a reference view and its n_src source views: reprojection, bilinear depth gather, the nine
 * dynamic thresholds (dist < i/thre1, rel < i/thre2, i = 2..10), geo = #(count_i >= i) >= nconditions,
 * photo = conf > photo_threshold, masked average depth.  Bit-exact vs the reference's CPU arithmetic.
 *   depth_ref, conf [h,w]; src_depths HOST array of n_src DEVICE pointers [h,w];
 *   mats [n_src][68] = per view: inverse(K_ref)[9], E_src@inverse(E_ref)[16], K_src[9], inverse(K_src)[9],
 *                       E_ref@inverse(E_src)[16], K_ref[9]  (row-major, computed by the host with the reference's calls)
 *   depth_avg [h,w]; masks [3,h,w] uint8 = (photo, geo, final)
 *   view_masks [n_src,h,w] uint16 (bit i <-> threshold i+2) or NULL; rep_out [n_src,h,w] (depth_reprojected) or NULL
 *   thre1, thre2 are DOUBLES: the reference compares fp32 tensors with the Python double i / thre, rounded to fp32 once, so the
 *   eighteen thresholds are (float)(i / thre) of the caller's double (a float thre moves some of them by one ulp).             */
int mdf_consistency_fuse_fwd(const float* depth_ref, const float* conf, const float* const* src_depths, const float* mats,
                             int n_src, int h, int w, float photo_threshold, int nconditions, double thre1, double thre2,
                             float* depth_avg, unsigned char* masks, unsigned short* view_masks, float* rep_out, void* stream);

/* ---- DTU depth-map fusion by multi-view consensus (tools/gipuma/main.py -d -> fusibile, fusibile.cu:138-276 with
 *      normal_thresh 360 and view selection off) ----------------------------------------------------------------------
 * One call per scan: every view is the reference view once, every other view of the scan is checked.  For pixel (x, y) of
 * view r with depth d: X = M_inv_r (d*x - p4.x, d*y - p4.y, d - p4.z); for each v != r project X with P_v to (u, w, z),
 * pt = (u/z, w/z), skip v unless 0 <= pt < (w, h); sample v's depth bilinearly at pt (wrap addressing, exact fp32 weights)
 * -> d^; v agrees when |f*b/z - f*b/d^| < disp_thresh with b = |C_r - C_v|; an agreeing view adds
 * M_inv_v (d^*floor(pt.x) - p4.x, d^*floor(pt.y) - p4.y, d^ - p4.z) and its bilinear colour to the sums.  A point is kept when
 * n >= num_consistent and none of its averaged coordinates is exactly 0; a non-finite point is written as (0,0,0).
 * Output order: reference view, then row-major pixel (order-preserving compaction, no atomics).
 *   depths [n,h,w] fp32 (0 = invalid); colors [n,h,w,4] uint8 (R,G,B,unused; 4-byte aligned)
 *   cams [n][32] fp32 per view: P [3x4 row-major], M_inv = inv(P[:, :3]) [9], centre C = -M_inv P[:, 3] [3], 8 unused
 *   f: the focal length of the scan's first camera, used for every view
 *   workspace: mdf_consensus_fuse_workspace(n, h, w) bytes, 16-byte aligned
 *   xyz [capacity,3] fp32, rgb [capacity,3] uint8 (points past capacity are not written), or both NULL: then only the fusion
 *   and the count scan run, and mdf_consensus_compact writes the points from the same workspace once the caller has read
 *   *total and sized the output (what ops.consensus_fuse does: the output holds exactly the kept points);
 *   view_counts [n] int32 points kept per reference view; total [1] int64 points kept (may exceed capacity)
 * Device memory: the workspace is 16 B per (view, pixel) (+ 12 B per 256-pixel block): 1.5 GB for 49 x 1600 x 1184.       */
long long mdf_consensus_fuse_workspace(int n, int h, int w);
int mdf_consensus_fuse_fwd(const float* depths, const unsigned char* colors, const float* cams, int n, int h, int w, float f,
                           float disp_thresh, int num_consistent, void* workspace, float* xyz, unsigned char* rgb,
                           long long capacity, int* view_counts, long long* total, void* stream);
int mdf_consensus_compact(void* workspace, int n, int h, int w, float* xyz, unsigned char* rgb, long long capacity, void* stream);

/* ---- Point-cloud fusion with visibility and small-segment filters (tools/pcd/fusion.py:get_cloud, stages 2-6; the two C++
 *      cores of tools/pcd/utils/fusion.cpp) ---------------------------------------------------------------------------
 * One call per scan runs steps first_step..last_step of the pipeline over every view (each step computes every view's update
 * from the state before the step, then applies all updates), in place on depths / masks:
 *   MDF_PCD_STEP_VIS1/2/3  visibility filter (get_reproj + vis_filter, img_dist 1, depth_thresh 0.01): a pixel stays when at
 *                          least `need` of its sources reproject within 1 px and 1 % depth; depth *= mask
 *   MDF_PCD_STEP_FUSION    visibility fusion (vis_fusion + vis_fusion_core): per pixel bin, the first (depth, violations)-sorted
 *                          candidate k with k >= violations[k], else the last; depth = fused * mask
 *   MDF_PCD_STEP_AVE       average fusion: (sum_v reproj_d * mask_v + d) / (sum_v mask_v + 1); depth = ave * mask
 *   MDF_PCD_STEP_SEG       small-segment filter (small_seg_core(depth, 4, 1e-3, 10)): 9x9-window components of < 10 pixels
 *                          are dropped; mask &= seg; depth *= mask
 * then counts the mask-true pixels: view_counts [n] int32, total [1] int64.  mdf_pcd_compact then writes the points of the
 * mask-true pixels (lifted at pixel centres), their colours and the direction to the camera centre, in view then row-major
 * order (ordered compaction, no atomics), from the same workspace and the unchanged depths / masks.
 *   depths [n,h,w] fp32, masks [n,h,w] uint8 (0/1); rgb [n,h,w,3] uint8
 *   cams [n][64] fp32 per view: K [9], K^-1 [9], E [16], E^-1 [16], centre -R^T t [3] (K^-1, E^-1, centre in float64 from the
 *   fp32 K, E, rounded to fp32), 11 unused
 *   srcs [n][v] int32 source views of each view (-1 = none; an entry outside [0, n) is treated as none); v <= MDF_PCD_MAX_SOURCES;
 *   need = ceil(fp32(vthresh - 1.1))
 *   workspace: mdf_pcd_fuse_workspace(n, h, w, v) bytes, 16-byte aligned: 13 B per (view, pixel) + 8 (v + 3) B per pixel
 *   of one view (1.77 GiB for 64 x 1056 x 1920 with 10 sources)
 *   xyz, dirs [capacity,3] fp32, rgb_out [capacity,3] uint8 (points past capacity are not written)                        */
#define MDF_PCD_MAX_SOURCES 64
#define MDF_PCD_STEP_VIS1 1
#define MDF_PCD_STEP_FUSION 2
#define MDF_PCD_STEP_VIS2 3
#define MDF_PCD_STEP_AVE 4
#define MDF_PCD_STEP_VIS3 5
#define MDF_PCD_STEP_SEG 6
long long mdf_pcd_fuse_workspace(int n, int h, int w, int v);
int mdf_pcd_fuse_fwd(float* depths, unsigned char* masks, const float* cams, const int* srcs, int n, int h, int w, int v, int need,
                     int first_step, int last_step, void* workspace, int* view_counts, long long* total, void* stream);
int mdf_pcd_compact(const float* depths, const unsigned char* masks, const unsigned char* rgb, const float* cams, int n, int h,
                    int w, int v, void* workspace, float* xyz, unsigned char* rgb_out, float* dirs, long long capacity,
                    void* stream);

/* ---- DTU point-cloud evaluation (the MATLAB scorer: reducePts_haa.m, MaxDistCP.m, PointCompareMain.m), fp64 throughout --------
 * Spatial index over n points pts [n][3] fp64: mdf_pts_index_workspace(n) bytes, 16-byte aligned, filled by mdf_pts_index_build (63-bit
 * Morton keys over the points' bounding box, a stable radix sort, leaves of 32 sorted points under an implicit binary tree of
 * AABBs).  The index holds a copy of the points; pts may be freed after the build.  Every call below that reads an index takes its
 * n and its buffer size (index_bytes) and refuses a buffer smaller than mdf_pts_index_workspace(n).
 * Distances: d^2 = ((dx*dx) + dy*dy) + dz*dz without contraction, d = sqrt(d^2), all correctly rounded.
 *   mdf_pts_nn_dist    dist[i] = the nearest-neighbour distance of query i among the index's points if the query lies in the region
 *                      and that distance is < cap, else cap (MaxDistCP(Qto = index, Qfrom = queries, BB, cap) below cap).  Queries:
 *                      either `queries` [m][3] fp64 (results in query order) or `qindex`, another index over m points (its points
 *                      are walked in key order and the results land at their input positions), not both.  bb: HOST [6] = BB(1,:),
 *                      BB(2,:), or NULL for no region; the region is the union of MaxDistCP's cubes: on every axis a,
 *                      fl(bb[a] + k*cap) <= q_a < fl(fl(bb[a] + k*cap) + cap) for some k in 0..floor((bb[3+a] - bb[a]) / cap).
 *                      visits [m] int32 (or NULL): leaves visited per query.  n = 0 gives cap everywhere.
 *   mdf_pts_reduce_*   reducePts_haa(pts, dst) for a given visiting order: rank [n] int32 (input indexing) is each point's position
 *                      in the order (ties by input index).  A point is kept iff no kept point that precedes it lies within
 *                      d <= dst: the sequential greedy result.  mdf_pts_reduce_count writes the number of (point, earlier
 *                      neighbour) pairs to edges [1] int64 (device); then mdf_pts_reduce with resume = 0 places that CSR in
 *                      csr [capacity] int32 (capacity >= edges) and runs up to max_rounds parallel rounds; resume = 1 runs
 *                      max_rounds more from the same workspace.  keep [n] uint8 (0/1, input indexing) is written after every
 *                      call; state [3] int32 (device, or NULL): rounds run, points still undecided (0 = done), 1 if the CSR did
 *                      not fit (then no round runs).  workspace: mdf_pts_reduce_workspace(n) bytes, 16-byte aligned (22 B a point).
 *   mdf_dtu_masks      DataInMask and StlAbovePlane of PointCompareMain.m: qdata [n][3], qstl [m][3] fp64; obs_mask uint8 0/1 of
 *                      size s1 x s2 x s3 in MATLAB (column-major) order; bb HOST [6] (only bb[0..2] = BB(1,:) is read); plane
 *                      HOST [4].  in_mask[i] = ObsMask(round((q - BB(1,:)) / res + 1)) inside [1, size], round() halving away
 *                      from zero; above[j] = ((P1 x + P2 y) + P3 z) + P4 > 0.  in_mask / above [n] / [m] uint8.            */
long long mdf_pts_index_workspace(long long n);
int mdf_pts_index_build(const double* pts, long long n, void* index, long long index_bytes, void* stream);
int mdf_pts_nn_dist(const void* index, long long n, long long index_bytes, const void* qindex, const double* queries, long long m,
                    long long qindex_bytes, const double* bb, double cap, double* dist, int* visits, void* stream);
long long mdf_pts_reduce_workspace(long long n);
int mdf_pts_reduce_count(const void* index, long long n, long long index_bytes, const int* rank, double dst, void* workspace,
                         long long ws_bytes, long long* edges, void* stream);
int mdf_pts_reduce(const void* index, long long n, long long index_bytes, const int* rank, double dst, void* workspace,
                   long long ws_bytes, int* csr, long long capacity, int resume, int max_rounds, unsigned char* keep, int* state,
                   void* stream);
int mdf_dtu_masks(const double* qdata, long long n, const unsigned char* obs_mask, int s1, int s2, int s3, const double* bb,
                  double res, unsigned char* in_mask, const double* qstl, long long m, const double* plane, unsigned char* above,
                  void* stream);

/* ---- Tanks and Temples F-score evaluation (crop volume, voxel-grid downsampling, point-to-point ICP), fp64 throughout ----------
 * The spatial index, the distance formula and the rounding rules are those of the DTU section above.
 *   mdf_pts_nn         mdf_pts_nn_dist's walk without a region, reporting which point was nearest: nearest[i] int32 = the INPUT
 *                      index (the position in the pts the index was built from) of query i's nearest point if its distance is
 *                      < cap, else -1; ties on d^2 go to the lowest input index.  dist [m] (or NULL): that distance, or cap;
 *                      dist2 [m] (or NULL): d^2, or +inf; visits [m] (or NULL).  Queries as an array or as an index, as above.
 *   mdf_pts_transform  out[i] = M p_i for a HOST 4x4 row-major matrix (rows 0..2 are read): x' = ((m00 x + m01 y) + m02 z) + m03,
 *                      every operation rounded once.  out may be pts.
 *   mdf_pts_crop       keep[i] uint8 = 1 iff axis_min <= p[axis] <= axis_max and (u, v) lies inside the polygon, HOST [k][2],
 *                      3 <= k <= 64, where (u, v) = (y, z), (x, z), (x, y) for axis 0, 1, 2.  Even-odd rule: edge (i, j = i+1 mod k)
 *                      counts iff (v_i < v && v_j >= v) || (v_j < v && v_i >= v) and u_i + ((v - v_i) / (v_j - v_i)) * (u_j - u_i) < u,
 *                      each operation rounded once; inside = an odd count.  Points on an edge follow that formula.
 *   mdf_pts_voxel_*    voxel-grid downsampling at cell size voxel: origin = (per-axis minimum of pts) - voxel/2, cell =
 *                      floor((p - origin) / voxel) per axis, one output point per occupied cell = (0 + the cell's points summed in
 *                      input order) / count, cells in ascending (x, y, z) cell order.  attrs [n][nattr] (nattr <= 6, or NULL with
 *                      nattr = 0) are averaged the same way.  out_pts [n][3], out_attrs [n][nattr], out_count [n] int32 are sized
 *                      for the worst case; m [1] int64 (device) receives the number of cells, or -1 when an axis needs more than
 *                      2^21 cells (nothing is written then).  workspace: mdf_pts_voxel_workspace(n) bytes, 16-byte aligned.
 *   mdf_pts_icp_sums   the sums of one point-to-point ICP step over the inliers (nearest[i] >= 0 and sqrt(dist2[i]) < threshold):
 *                      src [n][3] the transformed source, tgt [nt][3] the target in input order.  out [17] (device): inlier count,
 *                      sum of d^2, the source and target centroids, and H[a][b] = sum (s_a - cs_a)(t_b - ct_b) row-major.  Sums
 *                      run over a fixed tree whose shape depends on n only.  workspace: mdf_pts_icp_workspace() bytes.      */
int mdf_pts_nn(const void* index, long long n, long long index_bytes, const void* qindex, const double* queries, long long m,
               long long qindex_bytes, double cap, double* dist, double* dist2, int* nearest, int* visits, void* stream);
int mdf_pts_transform(double* out, const double* pts, long long n, const double* matrix, void* stream);
int mdf_pts_crop(const double* pts, long long n, int axis, double axis_min, double axis_max, const double* polygon, int k,
                 unsigned char* keep, void* stream);
long long mdf_pts_voxel_workspace(long long n);
int mdf_pts_voxel_downsample(const double* pts, const double* attrs, int nattr, long long n, double voxel, void* workspace,
                             long long ws_bytes, double* out_pts, double* out_attrs, int* out_count, long long* m, void* stream);
long long mdf_pts_icp_workspace(void);
int mdf_pts_icp_sums(const double* src, long long n, const double* tgt, long long nt, const int* nearest, const double* dist2,
                     double threshold, void* workspace, long long ws_bytes, double* out, void* stream);

/* ---- Point-cloud post-processing (k nearest neighbours, normal estimation), fp64 throughout ------------------------------------
 * The counterparts of the Open3D calls of the reference's tools/pcd/fusion.py (estimate_normals with its default 30-neighbour search,
 * compute_nearest_neighbor_distance), stated here and not measured against an Open3D build.  The spatial index, the distance
 * formula and the rounding rules are those of the DTU section above.
 *   mdf_pts_knn        the k nearest index points of every query, 1 <= k <= MDF_PTS_KNN_MAX.  Row i of nbr [m][k] int32 holds the
 *                      INPUT indices of query i's min(k, n) nearest points in ascending (d^2, input index) order, a total order:
 *                      ties on d^2 go to the lowest input index, as in mdf_pts_nn.  A point identical to the query is a neighbour
 *                      like any other, so a self-query has the point itself (or a lower-indexed duplicate) in slot 0.  Slots past
 *                      min(k, n) hold -1 and +inf.  dist2 [m][k] (or NULL): the d^2 of each slot; visits [m] (or NULL): leaves
 *                      visited.  Queries as an array or as an index, as for mdf_pts_nn.  A subtree is walked while its box
 *                      distance^2 is <= the k-th best so far (an equal distance may win on the index), so a cloud made of many
 *                      identical points degrades to a linear walk.
 *   mdf_pts_normals    a self-query over the index's own points that keeps no neighbour list in memory.  With N the
 *                      k_eff = min(k, n) neighbours of point i in the order above: nine sums over N in that order, each from 0 and
 *                      every product rounded once (x, y, z, xx, xy, xz, yy, yz, zz), each divided by k_eff, then
 *                      C_ab = E[ab] - E[a] * E[b], written to cov [n][6] (xx, xy, xz, yy, yz, zz; or NULL).  normals [n][3]: the
 *                      unit eigenvector of C for its smallest eigenvalue (cyclic Jacobi, a fixed number of sweeps), or (0, 0, 1)
 *                      when k_eff < 3.  dirs [n][3] fp32 (or NULL) orients it: s = ((nx*dx) + ny*dy) + nz*dz with dirs widened to
 *                      double; the normal is kept when s > 0 and negated otherwise (an exact 0 negates).  normals, cov and dirs
 *                      are in input order.                                                                                    */
#define MDF_PTS_KNN_MAX 32
int mdf_pts_knn(const void* index, long long n, long long index_bytes, const void* qindex, const double* queries, long long m,
                long long qindex_bytes, int k, int* nbr, double* dist2, int* visits, void* stream);
int mdf_pts_normals(const void* index, long long n, long long index_bytes, int k, const float* dirs, double* normals, double* cov,
                    void* stream);

/* ---- Scene import from a sparse model: per-image depth ranges and the view-selection score, fp64 throughout -----------------------
 * What turns "images + a COLMAP sparse model" into the cam files' depth range and pair.txt (tools/colmap); the reference has no
 * counterpart.  No contraction, every operation rounded once, sums in the stated order, no floating-point atomics: the integer
 * outputs, the ranges and the camera centres are a function of the inputs bit for bit, and the scores are reproducible run to run.
 * Inputs (device unless marked HOST): rot [n_img][9], trans [n_img][3] fp64, world -> camera, row-major; pts [n_pts][3] fp64; the
 * tracks as a CSR by point, track_off [n_pts + 1] int64 and track_img [n_obs] int32, image indices strictly ascending inside a
 * track, so each (image, point) pair appears once.
 *   camera centre      c_i[a] = -(((R_i[0][a] t_i[0]) + R_i[1][a] t_i[1]) + R_i[2][a] t_i[2]).
 *   depth              z = (((r20 x) + r21 y) + r22 z) + t2 of an observation of image i.
 *   mdf_view_depth_ranges   the n_i depths of image i in ascending order under the total order of their orderable bits (sign bit
 *                      flipped for positive values, all bits for negative ones: -0.0 < +0.0; equal depths keep CSR order):
 *                      range[i][0] = element min((long long)(q_lo * n_i), n_i - 1), range[i][1] the same with q_hi, the product in
 *                      double; 0 <= q_lo <= q_hi <= 1.  count [n_img] int32 = n_i; an image with n_i = 0 gets NaN, NaN.
 *   mdf_view_scores    for i < j and every point p both see, in ascending p: u = c_i - p, v = c_j - p, s = sqrt(((cx cx) + cy cy)
 *                      + cz cz) of u x v (each component a b - c d), d = ((u0 v0) + u1 v1) + u2 v2, theta = atan2(s, d) *
 *                      57.29577951308232 (degrees), e = theta - theta0, sigma = sigma1 if theta <= theta0 else sigma2,
 *                      term = exp(-(e e) / ((2 sigma) sigma)).  score[i][j] = score[j][i] = 0 + the terms one after the other;
 *                      shared[i][j] = shared[j][i] int32 = their number; both [n_img][n_img], zero elsewhere and on the diagonal.
 *                      n_rec = the sum over tracks of t (t - 1) / 2, which the caller computes from track_off; more than
 *                      2^31 - 4096 - 1 records (or observations) return MDF_EUNSUPPORTED.
 *   status [4] int32 (device): status[0] = the OR of the MDF_VIEW_* bits below, 0 when every track was used.  A track with an
 *                      offset outside [0, n_obs] or descending offsets, an image index outside [0, n_img) or indices that do not
 *                      ascend strictly is skipped as a whole; a wrong n_rec sets MDF_VIEW_BAD_COUNT and nothing is written past
 *                      n_rec.  The call still returns MDF_OK.
 *   workspace          mdf_view_workspace(n_img, n_pts, n_obs, n_rec) bytes (0: sizes out of range), 16-byte aligned; n_rec = 0
 *                      suffices for mdf_view_depth_ranges.  After mdf_view_scores it begins with the camera centres [n_img][3].
 * n_img <= 32768.  Empty sizes (n_img <= 1, n_pts = 0, n_obs = 0, n_rec = 0) are valid and give zeros / NaN ranges.             */
#define MDF_VIEW_BAD_IMAGE 1
#define MDF_VIEW_NOT_ASCENDING 2
#define MDF_VIEW_BAD_OFFSETS 4
#define MDF_VIEW_BAD_COUNT 8
long long mdf_view_workspace(int n_img, long long n_pts, long long n_obs, long long n_rec);
int mdf_view_depth_ranges(const double* rot, const double* trans, int n_img, const double* pts, long long n_pts,
                          const long long* track_off, const int* track_img, long long n_obs, double q_lo, double q_hi,
                          void* workspace, long long ws_bytes, double* range, int* count, int* status, void* stream);
int mdf_view_scores(const double* rot, const double* trans, int n_img, const double* pts, long long n_pts,
                    const long long* track_off, const int* track_img, long long n_obs, long long n_rec, double theta0,
                    double sigma1, double sigma2, void* workspace, long long ws_bytes, double* score, int* shared, int* status,
                    void* stream);

/* ---- Scene import: undistorting a photograph to a pinhole camera, fp64 coordinates -------------------------------------------------
 * What lets tools/colmap/main.py --undistort take a sparse model whose cameras are SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV or
 * OPENCV_FISHEYE (COLMAP's documented models); the reference has no counterpart.  src [B][Hs][Ws][3], dst [B][Hd][Wd][3], valid
 * [B][Hd][Wd] (or NULL): device, uint8, interleaved RGB.  coeffs: HOST, 12 doubles, copied into the kernel arguments.  The source
 * camera is (fx, fy, cx, cy) with the distortion below, the output camera [[zoom fx scale, 0, cx scale], [0, zoom fy scale, cy scale]];
 * pixel j covers [j, j + 1), its centre is j + 0.5.  No contraction, every product, sum and quotient rounded once, in this order:
 *   sample (b, a) of output pixel (i, j), b outer, a, b = 0..nsub-1, n = nsub:
 *                      X = (j + (a + 0.5) / n) / scale,  Y = (i + (b + 0.5) / n) / scale,
 *                      x = (X - cx) / (zoom fx),  y = (Y - cy) / (zoom fy),  (xd, yd) = distort(x, y),
 *                      U = ((fx xd) + cx) - 0.5,  V = ((fy yd) + cy) - 0.5.
 *   distort, kind MDF_UNDISTORT_RATIONAL, coeffs = k1, k2, p1, p2, k3, k4, k5, k6, then four unused:
 *                      xx = x x, yy = y y, r2 = xx + yy, r4 = r2 r2, r6 = r4 r2,
 *                      rad = (((1 + k1 r2) + k2 r4) + k3 r6) / (((1 + k4 r2) + k5 r4) + k6 r6),  q = 2 (x y),
 *                      xd = (x rad) + ((p1 q) + p2 (r2 + 2 xx)),  yd = (y rad) + ((p2 q) + p1 (r2 + 2 yy)).
 *   distort, kind MDF_UNDISTORT_FISHEYE, coeffs = k1, k2, k3, k4, then eight unused:
 *                      r = sqrt(r2); r = 0 gives (x, y); else t = atan(r), t2 = t t, t4 = t2 t2, t6 = t4 t2, t8 = t4 t4,
 *                      sc = (t ((((1 + k1 t2) + k2 t4) + k3 t6) + k4 t8)) / r,  xd = x sc,  yd = y sc.
 *   blank sample       U or V not finite, U < -0.5, U > Ws - 0.5, V < -0.5 or V > Hs - 0.5: it adds 0 to every channel.
 *   any other sample   u = floor(U), wu = U - u, mu = 1 - wu (v, wv, mv alike), taps at columns max(u, 0), min(u + 1, Ws - 1) and
 *                      rows max(v, 0), min(v + 1, Hs - 1); per channel top = (p00 mu) + p01 wu, bot = (p10 mu) + p11 wu,
 *                      value = (top mv) + bot wv.
 *   output             byte = floor(sum / (n n) + 0.5), the sum from 0 in (b, a) order; valid = 1 iff no sample of the pixel is blank.
 * MDF_EARG: a null src, dst or coeffs, a size <= 0, nsub outside [1, 16], an unknown kind, a focal length, zoom or scale that is not
 * finite and > 0, a coefficient or principal point that is not finite, B H W 3 > 2^31 - 1 for the source or the output.  Never
 * allocates, never synchronises.                                                                                                  */
#define MDF_UNDISTORT_RATIONAL 0
#define MDF_UNDISTORT_FISHEYE 1
#define MDF_UNDISTORT_MAX_NSUB 16
int mdf_image_undistort(const uint8_t* src, uint8_t* dst, uint8_t* valid, int B, int Hs, int Ws, int Hd, int Wd, int kind,
                        const double* coeffs, double fx, double fy, double cx, double cy, double zoom, double scale, int nsub,
                        void* stream);

/* =====================================================================================================
 * Training path (BASELINE config 3; train.py:36-45 -> loss.backward()).  The reference has no explicit backward:
 * autograd differentiates the op chains cited above.  Each entry below is the hand-written forward-in-train-mode or
 * backward of one such chain; gradients match torch autograd to fp32 summation-order tolerance.
 * ===================================================================================================== */

/* ---- BatchNorm3d in batch-statistics mode + ReLU (+ residual) around a conv layer (net/unit/base.py:61-68 with
 *      nn.BatchNorm3d.training, the blocks of net/unit/regular.py:17-41,82-108).  Activations channels-last [N,C],
 *      N = B*D*H*W voxels, C in {8,16,32,64}.
 *   stats:    sums[0..C) += sum_n y[n][c], sums[C..2C) += sum_n y^2      (sums: fp64, zeroed by the caller)
 *   finalize: aux[4C] = (a = gamma*invstd, b = beta - mean*a, mean, invstd) with the biased variance; when given,
 *             running_mean/var are updated as nn.BatchNorm does (momentum, unbiased variance) and *nbt += 1
 *   apply:    z = [res +] relu(y*a + b)
 *   bwd_reduce: red[0..C) += sum dr, red[C..2C) += sum dr*xhat,  dr = dz*[y*a+b > 0], xhat = (y-mean)*invstd
 *   bwd:      dy = gamma*invstd*(dr - red0/N - xhat*red1/N);  dgamma[c] = red1, dbeta[c] = red0
 *   ngroups: the tensor is [ngroups][N][C] and every group is one call of the module with its own batch statistics
 *   (the feature pyramid runs once per view, net/core.py:42): sums/red [ngroups][2C], aux [ngroups][4C]; dgamma/dbeta [C]
 *   are summed over the groups (one module, its calls' gradients add); finalize walks the groups in order for the running
 *   statistics and adds ngroups to *nbt.                                                                             */
int mdf_bn_stats_fwd(const float* y, long long N, int C, int ngroups, double* sums, void* stream);
int mdf_bn_finalize_fwd(const double* sums, const float* gamma, const float* beta, float eps, float momentum, long long N,
                        int C, int ngroups, float* aux, float* running_mean, float* running_var,
                        long long* num_batches_tracked, int nslices, void* stream);
int mdf_bn_relu_apply_fwd(const float* y, const float* aux, const float* res, float* z, long long N, int C, int ngroups,
                          void* stream);
/* finalize + apply as one launch (what the training path uses): z = [res +] relu(y*a + b) with (a, b) derived from `sums` in
 * the kernel; aux [ngroups][4C] is written for the backward pass, the running statistics are updated as by finalize.   */
int mdf_bn_finalize_apply_fwd(const float* y, const double* sums, const float* gamma, const float* beta, float eps, float momentum,
                              const float* res, float* z, float* aux, float* running_mean, float* running_var,
                              long long* num_batches_tracked, long long N, int C, int ngroups, int nslices, void* stream);
int mdf_bn_relu_bwd_reduce(const float* dz, const float* y, const float* aux, long long N, int C, int ngroups, double* red,
                           void* stream);
int mdf_bn_relu_bwd(const float* dz, const float* y, const float* aux, const double* red, const float* gamma, long long N,
                    int C, int ngroups, float* dy, float* dgamma, float* dbeta, int nslices, void* stream);
/* (`nslices`: the sums / reductions these three read may be spread over nslices copies [slice][group][2C] whose totals count --
 *  that is how the conv epilogues of mdf_conv*_train_fwd deliver them; 1 for mdf_bn_stats_fwd / mdf_bn_relu_bwd_reduce.) */

/* ---- weight gradient of nn.Conv3d(k3,p1,stride s) / nn.ConvTranspose3d(k3,s2,p1,op1) (net/unit/regular.py:17-43,
 *      80-110) as ONE correlation on the fp32 matrix cores:
 *          dw[a][b][tap] (+)= sum_o small[o][a] * big[stride*o + tap - 1][b]        (zero outside big)
 *      Conv3d: small = dy [B,Ds,Hs,Ws,A=Cout], big = x [B,s*Ds,s*Hs,s*Ws,Bc=Cin]      -> dw = torch [Cout,Cin,3,3,3]
 *      ConvTranspose3d: small = x [.., A=Cin], big = dy [.., Bc=Cout], stride 2         -> dw = torch [Cin,Cout,3,3,3]
 *      (the `prob` conv: A = 1).  NDHWC operands; workspace: mdf_conv3d_wgrad_workspace(...) floats.            */
int64_t mdf_conv3d_wgrad_workspace(int B, int Ds, int Hs, int Ws, int A, int Bc);
int mdf_conv3d_wgrad(const float* small_, const float* big, float* dw, float* workspace, int B, int Ds, int Hs, int Ws,
                     int A, int Bc, int stride, int accumulate, void* stream);
/* The same for the 2-D layers of the feature pyramid (net/unit/backbone.py:17-45; Conv2d k in {1,3,5}, pad (k-1)/2, stride s):
 *      dw[a][b][kh][kw] (+)= sum_o small[o][a] * big[s*o + (kh,kw) - pad][b];  small = dy [B,Hs,Ws,A], big = x [B,s*Hs,s*Ws,Bc]
 *      NHWC -> dw = torch [Cout,Cin,k,k].                                                                          */
int64_t mdf_conv2d_wgrad_workspace(int B, int Hs, int Ws, int A, int Bc, int ksize);
int mdf_conv2d_wgrad(const float* small_, const float* big, float* dw, float* workspace, int B, int Hs, int Ws, int A, int Bc,
                     int ksize, int stride, int accumulate, void* stream);
/* The same in two steps, for a whole backward pass: *_partial clears dw and leaves the partial tiles in `workspace` as
 * *nslab_out slabs of dw.numel() floats; mdf_wgrad_sum_batch adds the slabs of MANY layers into their gradient tensors in one
 * launch (host arrays of njobs slab / dw pointers, slab counts and element counts; jobs travel by value in the kernel
 * arguments).  The weight gradients are not needed before the optimizer, so a training step sums them once, at the end. */
int mdf_conv3d_wgrad_partial(const float* small_, const float* big, float* dw, float* workspace, int B, int Ds, int Hs, int Ws,
                             int A, int Bc, int stride, int* nslab_out, void* stream);
int mdf_conv2d_wgrad_partial(const float* small_, const float* big, float* dw, float* workspace, int B, int Hs, int Ws, int A, int Bc,
                             int ksize, int stride, int* nslab_out, void* stream);
int mdf_wgrad_sum_batch(const float* const* slabs, float* const* outs, const int* nslabs, const int* ns, int njobs, void* stream);
/* Deferred weight-gradient launches.  Between mdf_wgrad_batch_begin() and mdf_wgrad_batch_flush(stream) the calling thread's
 * mdf_conv3d_wgrad_partial / mdf_conv2d_wgrad_partial calls that take the LDS-staged kernel are RECORDED (operands, workspace and dw
 * must stay valid until the flush; *nslab_out is final at once); the flush launches them grouped by kernel instantiation, the layers
 * of a group as ONE launch (job table in the kernel arguments).  Results are those of the separate launches bit for bit.       */
int mdf_wgrad_batch_begin(void);
int mdf_wgrad_batch_flush(void* stream);
/* Read-only: what the calling thread's last weight-gradient dispatch decided (a dispatch that mdf_wgrad_batch_begin only recorded
 * counts), so that a test can tell which kernel form and tiling a shape took.  Copies min(n, MDF_WGRAD_PLAN_FIELDS) ints to `out`:
 *     form, R, TH, tv, n_tiles, gx, gy, gz, split
 * form: 0 wgrad_lds_kernel, 1 wgrad_kernel, 2 wgrad_a1_kernel, 3 wgrad_a1_valu_kernel, 4 wgrad2d_kernel (-1 before the first dispatch).
 * LDS form: tap packing R, rows TH and voxels tv of a tile, the launch's tiles.  The direct forms report R = 0, TH = 1, the voxels one
 * work item covers as tv (a 16-voxel chunk; the voxels a block of the vector-ALU form takes per iteration) and their item count as
 * n_tiles.  gx = partial-tile slabs written, (gx, gy, gz) the grid, split the waves that share a channel-tile pair.  Returns
 * MDF_WGRAD_PLAN_FIELDS.  Launches nothing.                                                                                      */
#define MDF_WGRAD_PLAN_FIELDS 9
int mdf_wgrad_last_plan(int* out, int n);
/* (input gradients of these layers are mdf_conv3d_fwd with re-packed weights: a stride-1 conv with flipped taps and
 *  swapped channels, the transposed conv for a stride-2 conv and vice versa.) */

/* ---- training-mode conv launches whose EPILOGUE carries the BatchNorm reductions (base.py:50-68: conv -> BatchNorm(batch
 *      statistics) -> ReLU; the statistics of a layer and the two sums of its BatchNorm backward each cost a full pass over
 *      the activations as kernels of their own -- here they ride in the conv that produces the tensor):
 *        y = [res +] conv(x)   raw (no scale / shift / ReLU), same operands and layouts as mdf_conv3d_fwd / mdf_conv2d_fwd
 *        stat_mode 1  stat_out[c] += sum y[.,c],  stat_out[C+c] += sum y[.,c]^2          (the layer's own batch statistics)
 *        stat_mode 2  the launch is the INPUT-GRADIENT conv of the next layer, so y (with res = the skip gradient) is dz of the
 *                     layer whose raw conv output is stat_y and whose (a, b, mean, invstd)[C] is stat_aux:
 *                     stat_out[c] += sum dr, stat_out[C+c] += sum dr*xhat, dr = dz*[stat_y*a+b > 0], xhat = (stat_y-mean)*invstd
 *      stat_out: fp64, zero-initialised by the caller, C = Cout in {8,16,32,64}.  2-D: `ngroups` consecutive sets of B/ngroups
 *      images are separate BatchNorm groups (one per view, net/core.py:42): stat_out [ngroups][2C], stat_aux [ngroups][4C].
 *      `nslices` (1..64): stat_out is [nslices][ngroups][2C] and the sums are the TOTALS over the slices -- a launch spreads its
 *      blocks over them so that no address takes more than a few dozen same-address atomics (~11 ns each, serialised).      */
int mdf_conv3d_train_fwd(const float* x, const float* wpack, const float* res, float* y, int B, int Di, int Hi, int Wi, int Cin,
                         int Cout, int stride, int transposed, int stat_mode, const float* stat_y, const float* stat_aux,
                         double* stat_out, int nslices, void* stream);
int mdf_conv2d_train_fwd(const float* x, const float* wpack, float* y, int B, int H, int W, int Cin_mem, int Cout, int ksize,
                         int stride, int planar_in, int stat_mode, const float* stat_y, const float* stat_aux, double* stat_out,
                         int nslices, int ngroups, void* stream);

/* ---- batched weight packing: every packed weight set a training step reads (forward convs and their input-gradient
 *      convs, train.py:36-45 after optimizer.step()), written by ONE launch.  A job is one weight set in the layout of
 *      mdf_conv3d_pack_weights (is3d = 1) / mdf_conv_pack_weights (is3d = 0), read from the parameter `src` through `mode`:
 *        0 the parameter itself [Cout][Cin][taps]          1 input gradient of a stride-1 conv: [Cin][Cout], taps mirrored
 *        2 input gradient of Conv2d(k5,s2,p2) as a 3x3 conv over dy with the 4 output-parity classes as channels
 *          (aux0 = the layer's in_channels, aux1 = first row of this part; Cin = the layer's out_channels, taps = 9)
 *        3 the `prob` conv [1][Cin][3][3][3] as 2-D conv rows per depth tap (Cout = 4, taps = 9)
 *        4 rows reordered for the PixelShuffle(2) epilogue    5 the parameter read as [Cin][Cout][taps]
 *      mdf_pack_job_fill writes job `index` into a HOST table of mdf_pack_job_bytes() bytes per job and returns the number
 *      of blocks the job takes (< 0: error code); first_block = sum of the earlier jobs' blocks.  The caller uploads the
 *      table and an int32 per-block job index once; mdf_pack_batch then re-packs everything per call.               */
int64_t mdf_pack_job_bytes(void);
int64_t mdf_pack_job_fill(void* jobs_host, int index, const float* src, float* dst, int is3d, int transposed, int mode,
                          int Cin, int Cout, int ntaps, int aux0, int aux1, int first_block);
int mdf_pack_batch(const void* jobs_dev, const int* block_job_dev, int nblocks, void* stream);

/* ---- adjoint of the FPN's bilinear x2 upsampling (backbone.py:60,62; F.interpolate(scale_factor=2, "bilinear",
 *      align_corners=False)), NHWC: dcoarse [B,h,w,C] (+)= up^T(dfine [B,2h,2w,C]); C % 4 == 0.                  */
int mdf_upsample2_bilinear_bwd(const float* dfine, float* dcoarse, int B, int h, int w, int C, int accumulate, void* stream);

/* ---- backward of the `prob` head: softmax over D + soft-argmin (regular.py:69/133, regress.py:5-7), and the input
 *      gradient of its Conv3d(C->1,k3,p1).   dlogit [B,D,h,w]; ddepth [B,h,w] and/or dprob [B,D,h,w] (either may be
 *      NULL); w torch [1,C,3,3,3]; dx NDHWC [B,D,h,w,C], C in {8,16}.  hypos is read only when ddepth is given and
 *      may be NULL without it.                                                                                   */
int mdf_prob_softmax_regress_bwd(const float* prob, const float* hypos, int hypos_per_pixel, const float* ddepth,
                                 const float* dprob, float* dlogit, int B, int D, int h, int w, void* stream);
/*      Read-only: the threads that share a pixel (1, 2, 4 or 8) in the launch above for this shape (< 0: error code).
 *      Launches nothing.                                                                                          */
int mdf_prob_softmax_regress_bwd_split(int B, int D, int h, int w);
int mdf_prob_conv_dgrad(const float* dlogit, const float* w, float* dx, int B, int D, int h, int wd, int C, void* stream);
/*      The same with the BatchNorm-backward sums of the regulariser's last layer taken on the way (dx is that layer's complete dz):
 *      stat_y = the layer's raw conv output [B*D*h*wd][C], stat_aux = its (a, b, mean, invstd) [4C] as mdf_bn_finalize_fwd wrote them,
 *      red = [nslices][2C] doubles zeroed by the caller (block b adds into copy b % nslices): sum dr | sum dr * xhat, the input of
 *      mdf_bn_relu_bwd (instead of a pass of mdf_bn_relu_bwd_reduce over dx and stat_y).                                          */
int mdf_prob_conv_dgrad_stat(const float* dlogit, const float* w, float* dx, int B, int D, int h, int wd, int C, const float* stat_y,
                             const float* stat_aux, double* red, int nslices, void* stream);

/* ---- training-mode VectorAggregate fused with the warp (homoaggregate.py:16-20,25-46 with the 1-channel
 *      BatchNorm3d in batch-statistics mode -- a global reduction per source view between similarity and view weight;
 *      base.py:97: no gradient through the sampling grid).  pass:
 *        0 stats       red_out[2v], [2v+1] += sum t_v, sum t_v^2  (t_v = Conv3d(G->1)(sim_v); fp64, zeroed by caller)
 *        1 forward     cost [B,D,h,w,G] and wsum [B,D,h,w] = sum_v w_v, with per-view (alpha_v, beta_v) from `par`
 *        2 bwd-reduce  red_out[2v], [2v+1] += sum dz_v, sum dz_v*xhat_v; red_out[2n], [2n+1] += d w2, d b2; aux [n_src][B*D*h*w][4]
 *                      = (w_v, dz_v, t_v, -) per sample, which pass 3 reads instead of re-deriving them from all channels
 *        3 backward    dref [B,h,w,C] (+=; zeroed by caller), dsrc[v] [B,h,w,G] (+= by fp32 atomics; zeroed by caller; the gradient of
 *                      channel 2g of every softmax pair -- channel 2g+1 gets its negative), dcw[G] (+=)
 *      par (float): [0,G) conv weight | G: w2 | G+1: b2 | G+2: gamma | G+3: 1/N | G+4+4v: alpha_v, beta_v, mean_v,
 *      invstd_v.  Features NHWC, C in {16,32,64}, G = C/2.                                                        */
int mdf_warp_aggregate_vec_train(int pass, const float* ref_fea, const float* const* src_feas, const float* proj,
                                 const float* hypos, int hypos_per_pixel, const float* par, const double* red_in,
                                 const float* dcost, float* cost, float* wsum, double* red_out, float* dref,
                                 float* const* dsrc, float* dcw, float* aux, int B, int C, int G, int D, int h, int w,
                                 int n_src, void* stream);
/* Control plane of the passes above, on the device (homoaggregate.py:16-20: the BatchNorm3d(1) of depth_weight, called
 * once per source view, :35-40):
 *   prepare       par[0,G+4) = (conv weight, w2, b2, gamma, 1/n), par[G+4, G+4+4 n_src) = 0, red[0,nred) = 0
 *   finalize      after pass 0: par[G+4+4v..] = (alpha_v, beta_v, mean_v, invstd_v) from red; running_mean / running_var /
 *                 num_batches_tracked (any may be NULL) advanced as by n_src successive calls with `momentum`
 *   bwd_finalize  after pass 3: dsrc [n_src][B,h,w,C] from the even-channel gradients dhalf [n_src][B,h,w,G] (n_half = their
 *                 total element count), and dpar = (d gamma, d beta, d w2, d b2) from pass 2's red; when dref_acc is given,
 *                 its n_ref floats (the zero-initialised buffer pass 3 accumulated d ref into) are copied to dref           */
int mdf_aggregate_train_prepare(const float* cw, const float* w2, const float* b2, const float* gamma, long long n, int G,
                                int n_src, float* par, double* red, int nred, void* stream);
int mdf_aggregate_train_finalize(const double* red, const float* gamma, const float* beta, float eps, float momentum, long long n,
                                 int G, int n_src, float* par, float* running_mean, float* running_var,
                                 long long* num_batches_tracked, void* stream);
int mdf_aggregate_train_bwd_finalize(const float* dhalf, const double* red, int n_src, long long n_half, float* dsrc,
                                     float* dpar, const float* dref_acc, float* dref, long long n_ref, void* stream);

/* ---- backward of homo_aggregate_by_variance fused with the warp (homoaggregate.py:49-69; base.py:97: no gradient through the
 *      sampling grid).  The operator has no parameters: its training forward is mdf_warp_aggregate_var_fwd with an
 *      MDF_VOL_NDHWC cost volume, bit-identical to eval.  With N = n_src + 1, x_0 = ref, x_v = softmax_C(warp(src_v)),
 *      m = sum_v x_v / N (recomputed from the features, never stored) and g = dcost:
 *        dref          [B,h,w,C]  = sum_d (2/N) g (ref - m)                      (+= by the depth slices; zeroed by caller)
 *        dsrc[v]       [B,h,w,C] += wt_k * x_v (gp - sum_c x_v gp), gp = (2/N) g (x_v - m), over the four bilinear taps of
 *                      every sample (fp32 atomics; zeroed by caller; out-of-bounds taps receive nothing)
 *      Features NHWC, C in {16,32,64}; dcost [B,D,h,w,C]; src_feas / dsrc HOST arrays of n_src DEVICE pointers.            */
int mdf_warp_aggregate_var_bwd(const float* ref_fea, const float* const* src_feas, const float* proj, const float* hypos,
                               int hypos_per_pixel, const float* dcost, float* dref, float* const* dsrc, int B, int C, int D,
                               int h, int w, int n_src, void* stream);
/*      Backward of mdf_homo_warp_fwd w.r.t. the source feature map (the transpose of the gather; the same kernel with the
 *      soft-max stage compiled out):  dsrc [B,h,w,C] += wt_k * dvol over the four taps (zeroed by caller).
 *      dvol [B,C,D,h,w] (MDF_VOL_NCDHW) or [B,D,h,w,C] (MDF_VOL_NDHWC); proj [B,12].                                       */
int mdf_homo_warp_bwd(const float* dvol, int vol_layout, const float* proj, const float* hypos, int hypos_per_pixel,
                      float* dsrc, int B, int C, int D, int h, int w, void* stream);

/* ---- training loss (net/loss.py:10-27): sum over the output scales of smooth-L1 (beta 1, mean) over the pixels with
 *      gt > depth_min[b].  est, gt [B][per_batch] float; depth_min element b at floor_[b*floor_stride], float64 when
 *      floor_f64 (as the loader hands depth_range over) else float32.
 *   reduce    acc[0] += sum of the per-pixel losses, acc[1] += number of valid pixels      (fp64, zeroed by the caller)
 *   finalize  loss[0] = sum_s acc[2s]/acc[2s+1] over nscales scales; inv_count[s] = 1/acc[2s+1]
 *   bwd       dest = dloss[0] * inv_count[0] * clamp(est - gt, -1, 1) on valid pixels, 0 elsewhere                    */
int mdf_masked_smooth_l1_reduce(const float* est, const float* gt, const void* floor_, int floor_f64, int floor_stride, int B,
                                long long per_batch, double* acc, void* stream);
int mdf_masked_smooth_l1_finalize(const double* acc, int nscales, float* loss, float* inv_count, void* stream);
int mdf_masked_smooth_l1_bwd(const float* est, const float* gt, const void* floor_, int floor_f64, int floor_stride, int B,
                             long long per_batch, const float* dloss, const float* inv_count, float* dest, void* stream);

/*      The same over all output scales in ONE launch each (Loss.forward sums four scales, net/loss.py:19-25): est / gt / dest are HOST
 *      arrays of nscales (<= 8) device pointers, per_batch a host array of element counts; acc is [2*nscales] as above; a NULL dest[i]
 *      skips scale i; inv_count is the [nscales] array mdf_masked_smooth_l1_finalize wrote.                                              */
int mdf_masked_smooth_l1_reduce_multi(const float* const* est, const float* const* gt, const long long* per_batch, int nscales,
                                      const void* floor_, int floor_f64, int floor_stride, int B, double* acc, void* stream);
int mdf_masked_smooth_l1_bwd_multi(const float* const* est, const float* const* gt, const long long* per_batch, int nscales,
                                   const void* floor_, int floor_f64, int floor_stride, int B, const float* dloss,
                                   const float* inv_count, float* const* dest, void* stream);

/* ---- validation metrics of depth maps (no counterpart in the reference: it has no validation code).  Up to 8 maps
 *      of different sizes in ONE reduction launch plus one small finalize launch.  Per map m (HOST arrays of nmaps entries):
 *        est[m], gt[m]  [B][per_batch[m]] float;
 *        hypos[m]       NULL, or the hypotheses a stage was given: [B][hypos_D[m]][per_batch[m]] when hypos_per_pixel[m], else
 *                       [B][hypos_D[m]]; plane 0 is the interval's lower end `lo`, plane D-1 its upper end `hi`;
 *        conf[m]        NULL, or [B][per_batch[m]] float.
 *      Per batch item: depth_min at floor_[b*floor_stride] (float64 when floor_f64, else float32, as mdf_masked_smooth_l1_reduce
 *      takes it) and thr[b][0..T-1] float absolute thresholds, 1 <= T <= 4.
 *      A pixel is valid iff (double)gt > depth_min[b].  A valid pixel whose est (or conf, lo, hi where given) is not finite counts
 *      in n_nonfinite and in nothing else.  e = fabsf(est - gt).  A table is [33][9] float64: row 0 over all pixels, rows 1..32 the
 *      confidence bins min(max((int)floorf(conf * 32), 0), 31); columns n, n_nonfinite, sum_e, under[0..3] (e < thr, strict),
 *      covered (lo <= gt && gt <= hi), sum_width (of the float hi - lo).  Bin rows fill n, sum_e, under[]; whatever has no input is 0.
 *      No floating-point atomics: every block writes a partial table to `workspace` (mdf_depth_metrics_workspace bytes for the
 *      same per_batch / nmaps / B; returns < 0 on a bad shape), mdf_depth_metrics_finalize adds them in block order into
 *      tables [nmaps][33][9].  conf_mask: bit m set iff conf[m] was given to the reduction.  Run-to-run bit-identical.           */
int64_t mdf_depth_metrics_workspace(const long long* per_batch, int nmaps, int B);
int mdf_depth_metrics_reduce_multi(const float* const* est, const float* const* gt, const float* const* hypos, const int* hypos_D,
                                   const int* hypos_per_pixel, const float* const* conf, const long long* per_batch, int nmaps,
                                   const void* floor_, int floor_f64, int floor_stride, const float* thr, int T, int B,
                                   void* workspace, long long workspace_bytes, void* stream);
int mdf_depth_metrics_finalize(const void* workspace, long long workspace_bytes, const long long* per_batch, int nmaps, int B,
                               int conf_mask, double* tables, void* stream);

/* ---- feature-pyramid heads in training mode, the small algebra (net/unit/backbone.py:59-63: lat2, lat3, out2, out3, out4 -- 1x1 convs
 *      around two bilinear up-samplings, evaluated through the products O2 L2, O2 L3, O3 L3; train_ops.py:FPNHeadsComposedFn).
 *      Matrices are the Conv2d weights, row-major [out][in]: O2 [c2][cm], O3 [c3][cm], L2 [cm][c2], L3 [cm][c3], biases b2, b3 [cm].
 *      _fwd writes comp = A2 = O2 L2 [c2][c2] | B3 = O2 L3 [c2][c3] | A3 = O3 L3 [c3][c3] | O2 b2 [c2] | O2 b3 [c2] | O3 b3 [c3].
 *      _bwd maps the gradients of the composed matrices (dA2, dB3, dA3), the pixel sums W2 = sum g (x) t4 [c2][cm], W3 [c3][cm] and
 *      the per-channel gradient sums s2, sc3 [c2], s3 [c3] (double, as mdf_bn_stats_fwd leaves them) onto the parameters' gradients.  */
int mdf_fpn_compose_fwd(const float* O2, const float* O3, const float* L2, const float* b2, const float* L3, const float* b3,
                        int c2, int c3, int cm, float* comp, void* stream);
int mdf_fpn_compose_bwd(const float* O2, const float* O3, const float* L2, const float* b2, const float* L3, const float* b3,
                        const float* dA2, const float* dB3, const float* dA3, const float* W2, const float* W3,
                        const double* s2, const double* sc3, const double* s3, int c2, int c3, int cm, float* dO2, float* dO3,
                        float* dL2, float* dL3, float* db2, float* db3, void* stream);

/* ---- optimizer step (train.py:14,43: torch.optim.Adam(lr) -> optimizer.step()) over all parameters in one launch.  The
 *      parameters stay the module's tensors; grads, exp_avg, exp_avg_sq are flat float buffers in parameter order.  A job
 *      is one parameter tensor (param, its offset in the flat buffers, n elements); mdf_adam_job_fill writes job `index`
 *      into a HOST table of mdf_adam_job_bytes() bytes per job and returns its block count (< 0: error code); the caller
 *      uploads the table and an int32 per-block job index once.  `step` = 1-based step count (bias corrections
 *      1 - beta^step); torch's defaults otherwise (no amsgrad; weight_decay is added to the gradient as torch does).  */
int64_t mdf_adam_job_bytes(void);
int64_t mdf_adam_job_fill(void* jobs_host, int index, float* param, long long offset, long long n, int first_block);
int mdf_adam_step(const void* jobs_dev, const int* block_job_dev, int nblocks, const float* grads, float* exp_avg,
                  float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay, long long step,
                  void* stream);
/*      The same step with its per-step scalars in DEVICE memory: hyper_dev[3] = (lr, 1 - beta1^step, sqrt(1 - beta2^step)), computed
 *      by the caller as mdf_adam_step computes them.  For a training step recorded once and replayed as a hipGraph
 *      (mdfnet_hip/graphstep.py): kernel arguments are frozen in the recording, memory is not.  */
int mdf_adam_step_hyper(const void* jobs_dev, const int* block_job_dev, int nblocks, const float* grads, float* exp_avg,
                        float* exp_avg_sq, const float* hyper_dev, float beta1, float beta2, float eps, float weight_decay,
                        void* stream);

/* ---- meshing (no counterpart in the reference: it stops at a point cloud; DESIGN section 7 "TSDF meshing").
 *      Volume: dims = (nx, ny, nz) lattice points, x fastest; point (i,j,k) sits at origin + voxel * (i,j,k).  dims and origin are
 *      HOST arrays of 3.  D, W [nz][ny][nx] float: the truncated signed distance (in units of trunc, <= 1) and the observation count.
 *      Views: depths (and images) are HOST arrays of nviews DEVICE pointers to [h][w] float maps ([h][w][3] uint8 images); cams is a
 *      HOST table [nviews][MDF_TSDF_CAM_FLOATS] float: R row-major [0..8], t [9..11] (p_cam = R x + t, the rows of the extrinsic),
 *      fx, fy, cx, cy [12..15] (no skew), [16] the largest finite positive texel of the view's depth map (-inf if it has none; read
 *      by mdf_tsdf_integrate only), rest 0.  A point projects to the texel (floor(fx x/z + cx + 0.5), floor(fy y/z + cy + 0.5)).
 *
 *   mdf_tsdf_integrate  every lattice point walks the views in the order given: skip if z <= 0 or not finite, if the texel is off
 *                       the map, if its depth d is not finite or <= 0, if d - z < -trunc; else f = min(1, (d - z) / trunc),
 *                       D <- (D W + f) / (W + 1), W <- W + 1.  `chunk` views per launch (0 = MDF_TSDF_CHUNK, the largest); the
 *                       result does not depend on it, nor on MDF_TSDF_CULL=0 (no brick of points skips a view as a whole).
 *   mdf_mesh_count      marching tetrahedra over the Kuhn split of every cell whose 8 corners have W >= min_weight; a corner is
 *                       inside if D < 0.  Leaves totals[0] = vertices, totals[1] = triangles (DEVICE, int64) and, in the
 *                       workspace (>= MDF_MESH_WORKSPACE_BYTES(nx ny nz) bytes, 16-byte aligned), what mdf_mesh_emit needs.
 *   mdf_mesh_emit       with the same volume, min_weight and workspace: vertices [n_vertices][3] float in increasing (lattice
 *                       index, edge direction), triangles [n_triangles][3] int32 in increasing (cell, tetrahedron, triangle),
 *                       normals towards D > 0.  Not to be called for an empty mesh; a total >= 2^31 is MDF_EUNSUPPORTED.
 *   mdf_mesh_colour     per vertex, over the views that see it with |d - z| <= trunc: the mean of the nearest texels of the images,
 *                       rounded half up; (128,128,128) where no view does.  acc: [n][4] float scratch, 16-byte aligned.            */
#define MDF_TSDF_CHUNK 16
#define MDF_TSDF_CAM_FLOATS 20
#define MDF_MESH_CHUNK 1024
#define MDF_MESH_WORKSPACE_BYTES(n) (18ll * (n) + 24ll * (((n) + MDF_MESH_CHUNK - 1) / MDF_MESH_CHUNK) + 256)
int mdf_tsdf_integrate(float* D, float* W, const int* dims, const float* origin, float voxel, float trunc,
                       const float* const* depths, const float* cams, int nviews, int h, int w, int chunk, void* stream);
int mdf_mesh_count(const float* D, const float* W, const int* dims, const float* origin, float voxel, float min_weight,
                   void* workspace, long long workspace_bytes, long long* totals, void* stream);
int mdf_mesh_emit(const float* D, const float* W, const int* dims, const float* origin, float voxel, float min_weight,
                  void* workspace, long long workspace_bytes, long long n_vertices, long long n_triangles, float* vertices,
                  int* triangles, void* stream);
int mdf_mesh_colour(const float* vertices, long long n, const float* const* depths, const unsigned char* const* images,
                    const float* cams, int nviews, int h, int w, float trunc, float* acc, unsigned char* rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDFNET_HIP_H */
