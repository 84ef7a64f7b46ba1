// vt_rowmap.h -- the thread mapping of the streaming activation kernels (vt_elementwise.hip, vt_resnet.hip, vt_mbconv.hip).
//
// One mapping ("RowMap"): a thread owns ONE 16-byte channel chunk column and walks rows (pixels), so per-channel
// coefficients live in registers and consecutive lanes touch consecutive 16-byte chunks of a pixel row (full-line
// coalesced NHWC accesses, G13).  The reduction passes on this mapping end in rowlane_fold, which adds the row lanes of a
// block; rowlane_fold_bytes is the dynamic LDS their launches ask for.  The BatchNorm passes of the three files share the walk
// of a column (rowmap_trips) and the host rules that cut their grids (fin_rowmap, fin_in_launch, bn_reduce_plan, check_keep).
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
    __host__ static RowMap make(int C, int epc, long M, int target_blocks = 4096) {
        RowMap r;
        r.CPR = C / epc;
        r.CT = r.CPR < kThreads ? r.CPR : kThreads;
        r.RT = kThreads / r.CT;
        long it = (M + (long)r.RT * target_blocks - 1) / ((long)r.RT * target_blocks);
        if (it < 1) it = 1;
        if (it > 64) it = 64;
        r.iters = (int)it;
        return r;
    }
    __host__ unsigned blocks(long M) const {
        const long rows_per_block = (long)RT * iters;
        return (unsigned)((M + rows_per_block - 1) / rows_per_block);
    }
    // the first row of row lane `lane` (threadIdx.x / CT; lanes >= RT idle) in row block blockIdx.x; its next ones follow RT apart
    __device__ __forceinline__ long row0(int lane) const { return (long)blockIdx.x * RT * iters + lane; }
};

template <typename T>
__device__ __forceinline__ uint4 ld16(const T* p) { return *(const uint4*)p; }
template <typename T>
__device__ __forceinline__ void st16(T* p, const uint4& v) { *(uint4*)p = v; }

// ---- the walk: what every streaming BatchNorm pass does with its rows ------------------------------------------------------
// The trips of one column: kUnroll rows per trip, and every load of a trip is issued before its first use (bytes in flight).
//   load(u, i, ok): zero slot u of the caller's arrays, then issue its loads if ok   (i: the trip slot, row = row0 + i * rm.RT)
//   use(u, i, ok):  unpack slot u, compute, store
// ok: slot i is one of the thread's rows (i < iters, row < M).  The caller keeps its uint4 v*[kUnroll] (and keep factors) in
// its own scope and the callables take them by reference; slots are used in row order, so a reduction adds in row order.
// The callables are lambdas marked VT_TRIP_LAMBDA: left to the inliner's cost model, the bf16 bodies are inlined after the
// passes that turn the per-element selects into v_cndmask and pair the sums (bn_bwd_reduce_kernel<bf16>: 829 instructions
// became 1146, a branch per element).
#define VT_TRIP_LAMBDA __attribute__((always_inline))
template <typename Load, typename Use>
__device__ __forceinline__ void rowmap_trips(const RowMap& rm, long row0, long M, Load&& load, Use&& use) {
    for (int it = 0; it < rm.iters; it += kUnroll) {
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            ok[u] = (it + u < rm.iters) && (row0 + (long)(it + u) * rm.RT < M);
            load(u, it + u, ok[u]);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) use(u, it + u, ok[u]);
    }
}

// the EPC coefficients of chunk column `col` of a row: a workgroup's LDS row (vt_fin_*_to_lds) or a global one
template <int EPC>
__device__ __forceinline__ void chunk_coef(float (&v)[EPC], const float* row, int col) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = row[col * EPC + e];
}
// (the Darknet forms: a NULL row is the constant `dflt` -- scale 1, shift 0)
template <int EPC>
__device__ __forceinline__ void chunk_coef(float (&v)[EPC], const float* row, int col, float dflt) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = dflt;
    if (row) chunk_coef(v, row, col);
}

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

// What the BatchNorm-backward reductions hand to rowlane_fold as `emit`: channel c (< C) of a channel group that starts at
// channel c0 of Ctot; the second sum takes invstd once, here; both go to replica `rep` of the statistics buffer.
__device__ __forceinline__ void bn_sums_emit(float* sums, int rep, int Ctot, int c0, const float* invstd, int C, int which, int c,
                                             float acc) {
    if (c >= C) return;
    if (which) acc *= invstd[c];
    vt_stat_add(sums, ((long)rep * 2 + which) * Ctot + c0 + c, acc);
}

// Finalize INSIDE the consuming launch (vt_bn_fin.h): every workgroup finalizes the channels of its own channel group
constexpr int kFinCg = kThreads / 2;  // channels per channel group: a thread pair per channel

// the channel group of C channels: the largest divisor <= 128 that is a multiple of the 16-byte chunk (0: none)
__host__ inline int fin_group(int C, int epc) {
    for (int g = kFinCg / epc * epc; g >= epc; g -= epc)
        if (C % g == 0) return (g >= 32 || g == C) ? g : 0;
    return 0;
}

// whether a pass finalizes for itself: C has a channel group (Cg = fin_group) and the switch is on; else the two launches
inline bool fin_in_launch(int Cg) { return Cg && VT_KNOB("VT_BN_FIN_APPLY", 1); }

// the grid of such a pass: VT_BN_FIN_APPLY_WGS workgroups over the channel groups (~1536 instead of the 4096 of the plain
// passes, so that the redundant finalize reads stay small beside the tensor traffic: vt_elementwise.hip)
inline RowMap fin_rowmap(int Cg, int groups, int epc, long M) {
    const int wgs = VT_KNOB("VT_BN_FIN_APPLY_WGS", 1536);
    return RowMap::make(Cg, epc, M, wgs / groups > 0 ? wgs / groups : 1);
}

// the grid of a BatchNorm-backward reduction: (rm.blocks(M), cgroups) workgroups, smem bytes of dynamic LDS
struct BnReducePlan {
    int cgroups, Cg;  // channel groups (blockIdx.y) of Cg channels each
    RowMap rm;
    int smem;
};
inline BnReducePlan bn_reduce_plan(long M, int C, int epc) {
    BnReducePlan p;
    // every block ends with 2*C 64-bit atomics into one of the statistics replicas: ~100 ns each when they queue on the same address,
    // so fewer, longer blocks win over grid-filling ones (measured per step: 1024 -> 23.53, 512 -> 23.36, 256 -> 23.27 ms)
    // channel groups of 64 on the small maps with many channels (see bn_bwd_reduce_kernel): the row splits shrink by the same factor
    p.cgroups = (M <= 65536 && C >= 256 && C % 64 == 0) ? C / 64 : 1;
    p.Cg = C / p.cgroups;
    // (round 6, beside the CU-owning filter-gradient kernels of the side stream: 128 -> 19.74, 256 -> 19.49, 512 / 1024 -> 19.45,
    //  2048 -> 19.55 ms per step)
    const int blocks_knob = VT_KNOB("VT_BN_RED_BLOCKS", 1024);
    p.rm = RowMap::make(p.Cg, epc, M, blocks_knob / p.cgroups > 0 ? blocks_knob / p.cgroups : 1);
    p.smem = rowlane_fold_bytes(2, p.rm.CT, p.rm.RT, epc);
    return p;
}

// a per-image operand of a pass (the keep row, the addend of vt_mbconv.hip): image b owns rows [b * HW, (b + 1) * HW) of the
// [M][C] matrix, and the kernels form b as (unsigned)row / HW
inline int check_image_rows(const char* who, int HW, long M) {
    VT_REQUIRE(HW > 0 && M > 0 && M % HW == 0 && M <= 0x7fffffffL, VT_ERR_INVALID,
               "%s: M=%ld must be a multiple of HW=%d (rows per image) below 2^31", who, M, HW);
    return VT_OK;
}
inline int check_keep(const char* who, const float* keep, int HW, long M) {
    VT_REQUIRE(keep, VT_ERR_INVALID, "%s: keep is a float[M / HW] row", who);
    return check_image_rows(who, HW, M);
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
