// vt_act.h -- the activation codes of the BatchNorm passes (vt_elementwise.hip, vt_mbconv.hip) and of the SE MLP (vt_gconv.hip).
#pragma once
#include "vt_common.h"

#ifdef __HIPCC__
namespace {

// ---------------------------------------------------------------------------------
// Activation codes of the `relu` argument of vt_bn_act_apply / _bwd_reduce / _bwd_apply (components.py:37-44): 0 none, 1 ReLU,
// 2 LeakyReLU(0.2), 3 SiLU ("swish"), 4 GELU (exact, erf), 5 ReLU6, 6 Hardswish (the MobileNets).  Codes 0 / 1 run the kernels' original instantiations (the hot
// path); codes >= 2 a GEN instantiation of the same kernels, so that the Darknet / VoVNet launches keep their code.
__device__ __forceinline__ float act_fwd(int code, float u) {
    switch (code) {
        case 1: return fmaxf(u, 0.f);
        case 2: return u > 0.f ? u : 0.2f * u;
        case 3: return u / (1.f + expf(-u));
        case 4: return 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
        case 5: return fminf(fmaxf(u, 0.f), 6.f);
        case 6: return u * fminf(fmaxf(u + 3.f, 0.f), 6.f) * (1.f / 6.f);
        default: return u;
    }
}
// d act / d u at pre-activation u
__device__ __forceinline__ float act_grad(int code, float u) {
    switch (code) {
        case 1: return u > 0.f ? 1.f : 0.f;
        case 2: return u > 0.f ? 1.f : 0.2f;
        case 3: {
            const float s = 1.f / (1.f + expf(-u));
            return s * (1.f + u * (1.f - s));
        }
        case 4: return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * 0.3989422804014327f * expf(-0.5f * u * u);
        case 5: return (u > 0.f && u < 6.f) ? 1.f : 0.f;
        case 6: return u < -3.f ? 0.f : (u <= 3.f ? (2.f * u + 3.f) * (1.f / 6.f) : 1.f);  // (torch's hardswish_backward)
        default: return 1.f;
    }
}

}  // namespace
#endif
