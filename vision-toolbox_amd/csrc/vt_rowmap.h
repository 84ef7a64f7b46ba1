// vt_rowmap.h -- the thread mapping of the streaming activation kernels (vt_elementwise.hip, vt_resnet.hip).
//
// One mapping ("RowMap"): a thread owns ONE 16-byte channel chunk column and walks rows (pixels), so per-channel
// coefficients live in registers and consecutive lanes touch consecutive 16-byte chunks of a pixel row (full-line
// coalesced NHWC accesses, G13).
#pragma once
#include "vt_common.h"

namespace {

#ifndef VT_EW_THREADS
#define VT_EW_THREADS 256
#endif
constexpr int kThreads = VT_EW_THREADS;
constexpr int kUnroll = 4;  // rows in flight per thread in the streaming kernels

// thread -> (channel chunk column, row lane) for an [M][C] matrix of 16-byte chunks
struct RowMap {
    int CPR;  // chunks per row
    int CT;   // threads along the row
    int RT;   // rows per block pass
    int iters;
    int rev;  // walk the row blocks from the last to the first (see vt_bn_order)
    __host__ static RowMap make(int C, int epc, long M, int target_blocks = 4096) {
        RowMap r;
        r.CPR = C / epc;
        r.CT = r.CPR < kThreads ? r.CPR : kThreads;
        r.RT = kThreads / r.CT;
        long it = (M + (long)r.RT * target_blocks - 1) / ((long)r.RT * target_blocks);
        if (it < 1) it = 1;
        if (it > 64) it = 64;
        r.iters = (int)it;
        r.rev = 0;
        return r;
    }
    __host__ unsigned blocks(long M) const {
        const long rows_per_block = (long)RT * iters;
        return (unsigned)((M + rows_per_block - 1) / rows_per_block);
    }
};

template <typename T>
__device__ __forceinline__ uint4 ld16(const T* p) { return *(const uint4*)p; }
template <typename T>
__device__ __forceinline__ void st16(T* p, const uint4& v) { *(uint4*)p = v; }

// Finalize INSIDE the consuming launch (vt_bn_fin.h): every workgroup finalizes the channels of its own channel group
constexpr int kFinCg = kThreads / 2;  // channels per channel group: a thread pair per channel

// the channel group of C channels: the largest divisor <= 128 that is a multiple of the 16-byte chunk (0: none)
__host__ inline int fin_group(int C, int epc) {
    for (int g = kFinCg / epc * epc; g >= epc; g -= epc)
        if (C % g == 0) return (g >= 32 || g == C) ? g : 0;
    return 0;
}

#define VT_DISPATCH_T(dtype, NAME, ...)                               \
    do {                                                              \
        if ((dtype) == VT_BF16) {                                     \
            typedef bf16_t T;                                         \
            __VA_ARGS__;                                              \
        } else if ((dtype) == VT_F32) {                               \
            typedef float T;                                          \
            __VA_ARGS__;                                              \
        } else {                                                      \
            vt_set_error("%s: unsupported dtype %d", NAME, (dtype)); \
            return VT_ERR_UNSUPPORTED;                                \
        }                                                             \
    } while (0)

inline int check_mat(const char* name, const void* p, int ld, int C, int dtype) {
    const int epc = vt_epc(dtype);
    if (!p || !vt_aligned16(p)) {
        vt_set_error("%s: null or misaligned pointer", name);
        return VT_ERR_INVALID;
    }
    if (C <= 0 || C % epc || ld % epc || ld < C) {
        vt_set_error("%s: C=%d ld=%d must be positive multiples of %d with ld>=C", name, C, ld, epc);
        return VT_ERR_UNSUPPORTED;
    }
    return VT_OK;
}
#define VT_TRY(expr)              \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != VT_OK) return rc__; \
    } while (0)

}  // namespace
