// vt_augment_erase.h -- the counter-based erase generator of the input pipeline (vt_amd.h, vt_augment_batch), shared by the
// kernels that end with the erase: vt_augment.hip and vt_trivial_augment.hip.
#pragma once
#include "vt_common.h"

namespace {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ float erase_normal(uint32_t seed, uint32_t b, uint32_t c, uint32_t y, uint32_t x) {
    uint32_t k = mix32(seed + 0x9e3779b9u);
    k = mix32(k + b);
    k = mix32(k + c);
    k = mix32(k + y);
    k = mix32(k + x);
    const uint32_t h1 = mix32(k ^ 0x68bc21ebu), h2 = mix32(k ^ 0x02e5be93u);
    const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-8f;  // 2^-24, exact
    const float u2 = (float)(h2 >> 8) * 5.9604644775390625e-8f;
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

}  // namespace
