// vt_attn_frag.h -- the register fragments of the bf16 attention kernels (vt_attention.hip, vt_window_attention.hip): how a
// lane reads the operands of mfma_f32_16x16x32_bf16 from a [64][D + 8] tile in LDS or from memory, and how an accumulator
// tile becomes the B operand of the product that follows.  The orientation is described at the top of vt_attention.hip.
#pragma once
#include "vt_common.h"

namespace {

constexpr int kT = 64;  // rows of a tile, both sides

// the fragment of row `row` (the lane's), reduction elements 32 kk + 8 g + j
template <int D>
__device__ __forceinline__ bf16x8 frag_lds(const bf16_t* tile, int row, int kk, int g) {
    return *(const bf16x8*)(tile + row * (D + 8) + 32 * kk + 8 * g);
}

__device__ __forceinline__ bf16x8 frag_global(const bf16_t* __restrict__ src, int ld, int row, bool valid, int kk, int g) {
    if (!valid) return __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
    return *(const bf16x8*)(src + (long)row * ld + 32 * kk + 8 * g);
}

// column d0 + u of the tile's rows 32 s + 16 (j >> 2) + 4 g + (j & 3), j = 0..7: the A operand that pairs with pack8()
template <int D>
__device__ __forceinline__ bf16x8 frag_tr(const bf16_t* tile, int s, int d0, int g, int u) {
    const bf16_t* a0 = tile + (32 * s + 4 * g + (u >> 2)) * (D + 8) + d0 + 4 * (u & 3);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 16 * (D + 8)));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// two 16-row accumulator sub-tiles -> the bf16 B operand of one 32-deep k-step
__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
    return __builtin_bit_cast(bf16x8, make_uint4(VecIO<bf16_t>::pack2(a[0], a[1]), VecIO<bf16_t>::pack2(a[2], a[3]),
                                                 VecIO<bf16_t>::pack2(b[0], b[1]), VecIO<bf16_t>::pack2(b[2], b[3])));
}

__device__ __forceinline__ void store4_bf16(bf16_t* dst, const f32x4 v, float s) {
    *(uint2*)dst = make_uint2(VecIO<bf16_t>::pack2(v[0] * s, v[1] * s), VecIO<bf16_t>::pack2(v[2] * s, v[3] * s));
}

#define VT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

}  // namespace
