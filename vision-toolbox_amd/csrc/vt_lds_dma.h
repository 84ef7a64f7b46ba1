// vt_lds_dma.h -- the LDS-DMA, wait and barrier primitives of the convolution kernels (vt_igemm*.hip, vt_wgrad*.hip,
// vt_stem.hip, vt_stem6.hip), each once, with the hazard argument its instruction string relies on.
//
// hipcc treats an asm statement as ONE opaque instruction: it allocates the operands, but it neither counts the memory
// operations inside (these kernels count their own vmcnt) nor pads the hazards inside, and it does not preserve M0
// around a statement.  The cases that matter here:
//   (a) s_mov_b32 m0 -> an LDS-DMA reading M0 as its LDS base: 1 wait state (the s_nop 0 behind every write of M0);
//   (b) an SGPR written by a VALU instruction (v_readfirstlane; a v_readlane that reloads a spilled SGPR) -> a VMEM
//       instruction reading it as its base: 5 wait states, counted from the top of the statement, because hipcc may put
//       that VALU write directly in front of it.  An s_mov_b32 reading such an SGPR is an SALU read and needs none;
//   (c) M0 is compiler-reserved: a value written in one statement is only safe for a LATER statement while the
//       compiler writes no M0 in between (see the "M0 set by the caller" forms).
// A VGPR address written right before the statement needs nothing: the VALU -> VMEM address path is interlocked.
//
// Names: glds16 = one global_load_lds_dwordx4 wave-instruction, lane l copies 16 B to LDS byte M0 + 16 l.
//   _m0_saved    the statement saves M0, sets it, issues and restores it: usable anywhere in a kernel
//   _m0_written  the statement sets M0 and leaves it: the wave restores M0 (get_m0 / set_m0) before it ends
//   _m0_preset   the statement only issues: M0 was set by a set_m0() statement before it
//   (none)       source = a per-lane 64-bit address in a VGPR pair
//   _sbase       source = an SGPR base plus a per-lane 32-bit byte offset (no 64-bit VALU arithmetic per instruction)
//   _rfl         one-line wrapper that first makes the scalar operands wave-uniform with v_readfirstlane.  The plain
//                forms take operands the compiler already PROVES uniform (kernel arguments, blockIdx, a readfirstlane'd
//                wave index); a kernel that has no v_readfirstlane there keeps having none.
#pragma once
#include <type_traits>

#include "vt_common.h"

namespace {

// The source of every padded / out-of-range chunk: the LDS destination of an LDS-DMA is lane-linear and cannot be
// predicated, so a lane that has nothing to fetch reads these 16 zero bytes instead.  One per translation unit (the
// library is built without relocatable device code: there is no cross-file device symbol).
__device__ __attribute__((aligned(16))) unsigned int vt_zero16[4];

// ---- LDS-DMA -----------------------------------------------------------------------------------------------------------
// M0 saved and restored, per-lane 64-bit address.  M0 is written in the statement that reads it (c), one wait state
// before the DMA (a); the DMA has taken its LDS base when it issues, so M0 is restored right behind it.  lds_base is
// read by an s_mov_b32 only: no (b).  keep is early-clobber: it is written before lds_base is read.
__device__ __forceinline__ void glds16_m0_saved(unsigned long gsrc, unsigned lds_base) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_base)
        : "memory");
}
__device__ __forceinline__ void glds16_m0_saved_rfl(unsigned long gsrc, unsigned lds_base) {
    glds16_m0_saved(gsrc, __builtin_amdgcn_readfirstlane(lds_base));  // (wave-uniform by construction, not provably)
}

// M0 saved and restored, SGPR base + 32-bit lane offset.  sbase is read by the VMEM instruction (b): the two s_mov_b32
// in front of it are two of the five wait states, s_nop 2 the other three -- which also covers (a).
__device__ __forceinline__ void glds16_m0_saved_sbase(unsigned voff, const void* sbase, unsigned lds_base) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 2\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_base)
        : "memory");
}

// M0 written and left, SGPR base + 32-bit lane offset, operands already wave-uniform.  Nothing of the statement but the
// s_mov_b32 stands in front of the VMEM read of sbase, so s_nop 4 supplies the five wait states of (b) alone (and (a)).
__device__ __forceinline__ void glds16_m0_written_sbase(unsigned voff, const void* sbase_uniform, unsigned lds_addr_uniform) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %0, %1"
                 ::"v"(voff), "s"(sbase_uniform), "s"(lds_addr_uniform)
                 : "memory");
}

// ---- M0 set by the caller: the loader waves of vt_igemm_span6.hip, vt_igemm_pspan.hip and vt_wgrad6.hip ---------------
// These DEPART from "write M0 in the statement that reads it" (c): set_m0() is one statement, the bare DMA the next, and
// the wave's original M0 comes back only at the end of the loader (get_m0() on entry, set_m0(keep) on exit): one scalar
// move per piece instead of three in waves that do nothing but issue pieces.  (No measurement here shows that the two
// moves matter -- on vt_wgrad_span.hip "not restoring M0" measured without effect -- so the saved form would be the
// sounder one; changing it changes the kernels and is not done here.)  What they rely on instead: both statements are volatile with a "memory" clobber, so they keep their
// order; between them stands only the VALU select of the lane's source address; and on gfx950 hipcc writes M0 itself
// only for indirect register indexing, s_sendmsg / GWS and its own LDS-DMA builtins, none of which a loader wave
// contains.  That is a property of the build, not a guarantee of the compiler: after a change to a loader, read its
// assembly and require that no instruction writes m0 between a set_m0 and the DMA behind it.
__device__ __forceinline__ unsigned get_m0() {
    unsigned v;
    asm volatile("s_mov_b32 %0, m0" : "=s"(v)::"memory");
    return v;
}
// (the wait state of (a) sits here, so the DMA statements below open without one; the operand is read by an SALU)
__device__ __forceinline__ void set_m0(unsigned v) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(__builtin_amdgcn_readfirstlane(v)) : "memory");
}
// M0 set by the caller, per-lane 64-bit address: no scalar operand, nothing to pad.
__device__ __forceinline__ void glds16_m0_preset(unsigned long gsrc) {
    asm volatile("global_load_lds_dwordx4 %0, off" ::"v"(gsrc) : "memory");
}
// M0 set by the caller, SGPR base + 32-bit lane offset: the statement is the VMEM instruction alone, and its base may
// come straight from the v_readfirstlane of the wrapper (or from a v_readlane reloading a spilled SGPR): s_nop 4 = the
// five wait states of (b).  Without it the load can use a stale base: a memory fault.
__device__ __forceinline__ void glds16_m0_preset_sbase(unsigned voff, const void* sbase_uniform) {
    asm volatile("s_nop 4\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase_uniform) : "memory");
}

__device__ __forceinline__ const void* uniform_ptr(const void* p) {
    const unsigned long v = (unsigned long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const void*)(((unsigned long)hi << 32) | lo);
}
__device__ __forceinline__ void glds16_m0_preset_sbase_rfl(unsigned voff, const void* sbase) {
    glds16_m0_preset_sbase(voff, uniform_ptr(sbase));
}
__device__ __forceinline__ void glds16_m0_written_sbase_rfl(unsigned voff, const void* sbase, unsigned lds_addr) {
    glds16_m0_written_sbase(voff, uniform_ptr(sbase), __builtin_amdgcn_readfirstlane(lds_addr));
}

// ---- waits and barriers ------------------------------------------------------------------------------------------------
// Counted wait for this wave's LDS-DMAs (hipcc counts none of them): at most N still in flight.  The data of the
// retired ones may be read after the NEXT workgroup barrier.  A run-time count needs a decision tree over immediates:
// the three vm_wait_dyn stay in their files, with their own caps.
template <int N>
__device__ __forceinline__ void vm_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// this wave's LDS reads and writes have completed (ahead of re-using what they touched without a barrier)
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// workgroup barrier of the tick-scheduled 12-wave kernels: nothing migrates across a tick boundary
__device__ __forceinline__ void wg_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- LDS images --------------------------------------------------------------------------------------------------------
// Chunk swizzle of a 64-byte row (4 chunks of 16 B), g = row >> 2: conflict free for a ds_read_b128 issued as
// (row = l & 15, chunk = l >> 4) over 16 rows that start at a multiple of 4 (filter slices; vt_igemm.hip's stages).
__device__ __forceinline__ int swz4(int g) { return (0x1320 >> ((g & 3) * 4)) & 3; }
// Span image: chunk ^= 2 * ((row >> 2) & 1).  A tap shifts the fragment's 16 rows by an arbitrary offset; this is the
// swizzle (found by enumeration over all 4-entry tables) under which the four 16-lane groups of a ds_read_b128 hit 16
// distinct 16-byte slots for EVERY row offset -- the 0x1320 table is conflict free only for offsets that are
// multiples of 4 (2-way on half of the taps).
__device__ __forceinline__ int swzA(int g) { return (g & 1) << 1; }

// ---- MFMA and lane arithmetic ------------------------------------------------------------------------------------------
// one 16 x 16 accumulator tile += A chunk x B chunk (16 B each): v_mfma_f32_16x16x32_bf16, or 4 x v_mfma_f32_16x16x4_f32
// over elements 0..3 of the chunks (exact f32 parity mode; only the order of the K summation differs)
template <typename T>
__device__ __forceinline__ void mma(const uint4& a, const uint4& b, f32x4& acc);
template <>
__device__ __forceinline__ void mma<bf16_t>(const uint4& a, const uint4& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                  __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma<float>(const uint4& a, const uint4& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

// sum of a value over the 16 lanes of its DPP row (lanes 16k .. 16k+15), returned in every lane of the row
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_sum16(float x) {
    x = dpp_add<0x128>(x);  // row_ror:8
    x = dpp_add<0x124>(x);  // row_ror:4
    x = dpp_add<0x122>(x);  // row_ror:2
    return dpp_add<0x121>(x);  // row_ror:1
}

// a compile-time integer as a function argument (the macro-free way to unroll a lambda over steps or tile heights)
template <int T>
using I_ = std::integral_constant<int, T>;

// ---- position streams of the span filter-gradient kernels --------------------------------------------------------------
struct Pos {  // a padded position, decomposed, and the element offset of its pixel
    int b, i, j, off;
    __device__ __forceinline__ void init(long P, int S, int PW, int H, long row, int ld) {
        long bb = P / S;
        long rem = P - bb * S;
        if (rem < 0) rem += S, --bb;
        b = (int)bb;
        i = (int)(rem / PW);
        j = (int)(rem - (long)i * PW);
        off = (int)(((long)b * H + i) * row + (long)j * ld);  // (mod 2^32 while b < 0; exact for every real pixel)
    }
};
// Advance a Pos by STEP positions with additions only: recomputing (b, i, j) by multiply-high quotients and the offset by
// 64-bit multiplies every step was 18 quarter-rate integer multiplies among ~100 vector instructions per wave and step,
// against 20 MFMAs -- the loop was bound by vector issue (rocprofv3 PMC, 128 -> 128 @28x28: SQ_INSTS_VALU 22.4 M,
// SQ_INSTS_MFMA 3.9 M, LDS array 16 % busy, no bank conflicts), not by the transposing reads.
template <int STEP>
struct PosStep {
    int q, r;        // STEP = q * PW + r
    int c0, c1, c2;  // offset deltas: STEP positions ahead | a column wrap | a row wrap (next image)
    __device__ __forceinline__ void init(int PH, int PW, int H, long row, int ld) {
        q = STEP / PW, r = STEP - q * PW;
        c0 = (int)(r * (long)ld + q * row);
        c1 = (int)(row - (long)PW * ld);
        c2 = (int)((long)(H - PH) * row);
    }
    __device__ __forceinline__ void advance(Pos& p, int PH, int PW) const {
        p.j += r, p.i += q, p.off += c0;
        if (p.j >= PW) p.j -= PW, ++p.i, p.off += c1;
        if (p.i >= PH) p.i -= PH, ++p.b, p.off += c2;
        if (p.i >= PH) p.i -= PH, ++p.b, p.off += c2;  // (q + 1 < 2 PH: checked by the launchers)
    }
};

}  // namespace
