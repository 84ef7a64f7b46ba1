// vt_rowmap.h -- the thread mapping of the streaming activation kernels (vt_elementwise.hip, vt_resnet.hip, vt_mbconv.hip).
//
// One mapping ("RowMap"): a thread owns ONE 16-byte channel chunk column and walks rows (pixels), so per-channel
// coefficients live in registers and consecutive lanes touch consecutive 16-byte chunks of a pixel row (full-line
// coalesced NHWC accesses, G13).  The reduction passes on this mapping end in rowlane_fold, which adds the row lanes of a
// block; rowlane_fold_bytes is the dynamic LDS their launches ask for.
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

// ---- the fold of the row lanes: the tail of every reduction pass on this mapping ------------------------------------------
// Each thread of a block holds NS partial sums per channel of its chunk (s[NS][EPC]; a thread without rows holds zeros); the
// block's RT row lanes of a channel are added and the sum is handed to emit(which, local_channel, sum), once per (sum, channel
// of the pass: CT * EPC of them) in the first NS * CT * EPC threads.  No LDS atomics: with RT rows per column they serialised
// RT-way and cost as much as the streaming itself on the 28x28 .. 7x7 maps.
// With CT a power of two below 64 a wave holds 64 / CT row lanes of every column it touches; those are folded in registers
// first (xor shuffles), so the LDS staging shrinks from RT to kThreads / 64 rows -- 4 KiB instead of 16 KiB at C = 128.  (The
// reductions run beside the filter gradients of the side stream, whose workgroups hold most of a CU's LDS: at 16 KiB per
// block their occupancy, not HBM, set their in-step time.)
// The LDS contract is rowlane_fold_bytes: the host sizes the launch's dynamic LDS with it, from the predicate the device uses.
__host__ __device__ inline bool rowlane_inwave(int CT) { return CT < 64 && (CT & (CT - 1)) == 0; }
// bytes of LDS at `sred` (16-byte aligned) that rowlane_fold<NS, EPC> touches: [rows][NS][CT * EPC] floats
__host__ inline int rowlane_fold_bytes(int NS, int CT, int RT, int EPC) {
    return (rowlane_inwave(CT) ? kThreads / 64 : RT) * NS * CT * EPC * (int)sizeof(float);
}
// All kThreads threads of the block call it (two barriers; the trailing one frees `sred` for the next pass of a column loop).
template <int NS, int EPC, typename Emit>
__device__ __forceinline__ void rowlane_fold(float* sred, float (&s)[NS][EPC], int CT, int RT, Emit&& emit) {
    const int t = threadIdx.x;
    const int r = t / CT, tc = t % CT;
    const int W = CT * EPC;  // channels covered per pass
    int rows_l = RT, r_l = r;
    if (rowlane_inwave(CT)) {
        for (int off = CT; off < 64; off <<= 1) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
#pragma unroll
                for (int k = 0; k < NS; ++k) s[k][e] += __shfl_xor(s[k][e], off, 64);
            }
        }
        rows_l = kThreads / 64;
        r_l = (t & 63) < CT ? (t >> 6) : -1;  // one writer per (wave, column)
    } else if (r >= RT) {
        r_l = -1;
    }
    if (r_l >= 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            float4* d = (float4*)(sred + ((long)(r_l * NS + k) * W + tc * EPC));
#pragma unroll
            for (int q = 0; q < EPC / 4; ++q) d[q] = make_float4(s[k][4 * q], s[k][4 * q + 1], s[k][4 * q + 2], s[k][4 * q + 3]);
        }
    }
    __syncthreads();
    for (int i = t; i < NS * W; i += kThreads) {
        const int which = NS > 1 ? i / W : 0, lc = NS > 1 ? i % W : i;
        float acc = 0.f;
        for (int rr = 0; rr < rows_l; ++rr) acc += sred[(long)(rr * NS + which) * W + lc];
        emit(which, lc, acc);
    }
    __syncthreads();
}

// Finalize INSIDE the consuming launch (vt_bn_fin.h): every workgroup finalizes the channels of its own channel group
constexpr int kFinCg = kThreads / 2;  // channels per channel group: a thread pair per channel

// the channel group of C channels: the largest divisor <= 128 that is a multiple of the 16-byte chunk (0: none)
__host__ inline int fin_group(int C, int epc) {
    for (int g = kFinCg / epc * epc; g >= epc; g -= epc)
        if (C % g == 0) return (g >= 32 || g == C) ? g : 0;
    return 0;
}

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
}  // namespace
