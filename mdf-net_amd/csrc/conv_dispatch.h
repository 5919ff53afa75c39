// The conv family's internal cross-file entries (not part of the C ABI), declared once for the files that define and that call them: a call that no
// longer matches its definition fails to link.  All answer MDF_EUNSUPPORTED when they have no kernel for the layer: the caller goes on to its next route.
#pragma once
#include "common.h"
int mdf_conv_lds_dispatch(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res, float res_scale, const float* res_up, float* y,
                          int B, int D, int H, int W, int Cin, int Cin_mem, int Cout, int KD, int KHW, int stride, int relu, void* stream, int planar_in, int shuffle2,
                          const mdf::ConvStat* stat);      // conv_lds.hip; from conv3d.hip and the 2-D entries
int mdf_wino3d_dispatch(const float* x, const float* wpack_wino, const float* alpha, const float* beta, const float* res, float res_scale, float* y, int B, int D, int H,
                        int W, int Cin, int Cout, int relu, void* stream);      // wino3d.hip; from conv_lds.hip, as the next two (wino2d.hip)
int mdf_wino2d_dispatch(const float* x, const float* wpack_wino, const float* alpha, const float* beta, const float* res, float res_scale, float* y, int B, int H, int W,
                        int Cin, int Cout, int relu, void* stream);
int mdf_wino2d_s2d_dispatch(const float* x, const float* wpack_k5w, const float* alpha, const float* beta, float* y, int B, int Ho, int Wo, int Cin_mem, int Cout, int relu, void* stream);
int mdf_conv1x1_dispatch(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res, float res_scale, const float* res_up, float* y, int B,
                         int H, int W, int Cin, int Cout, int relu, void* stream);      // conv1x1.hip; from the 2-D entries
int mdf_convtr3d_dispatch(const float* x, const float* wpack, const float* alpha, const float* beta, const float* res, float* y, int B, int Di, int Hi, int Wi, int Cin,
                          int Cout, int relu, int kd_skip, void* stream);      // convtr3d.hip; from conv3d.hip
