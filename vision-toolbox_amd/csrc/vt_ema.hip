// vt_ema.hip -- the exponential moving average of the weights (include/vt_amd.h states the recurrence).
//
// Three launches close an optimiser step that keeps an average:
//   vt_ema_tick    one thread: which kind of step is this (skip / copy / blend)?  The answer is left in the control buffer,
//                  so the launches behind it -- and a captured graph of them -- are the same on every step.
//   vt_ema_update  one streaming pass over a flat f32 buffer: e <- p (copy) or e <- e + alpha * (p - e) (blend), and the
//                  bf16 mirror of the NEW e in the same pass.  14 bytes per element with a mirror (read e, p: 8; write e: 4,
//                  mirror: 2), 12 without; a copy step does not read e.  In skip mode every workgroup returns behind its
//                  read of the control words: neither buffer is touched.
//   vt_ema_copy    the integer buffers (BatchNorm's num_batches_tracked), which are copied, never averaged -- on the steps
//                  the average moves, so that a skipped step leaves every shadow buffer alone.
//
// Roundings of a blend, per element: d = p - e (one), e' = fma(alpha, d, e) (one).  Nothing else rounds: alpha arrives as an
// f32 the host made from the double 1 - decay, and the mirror is a cast of the stored e'.
#include "vt_common.h"

namespace {

constexpr int kEmaThreads = 256;
// grid cap of the streaming kernels: 256 CUs x 8 workgroups.  A workgroup covers kEmaThreads 16-byte chunks per round, so
// every workgroup loops once n exceeds kEmaMaxBlocks * kEmaThreads * 4 = 2 097 152 elements (the tests take their large n
// from vt_ema_grid_cap).
constexpr int kEmaMaxBlocks = 2048;

__global__ void __launch_bounds__(64)
ema_tick_kernel(float* __restrict__ ctl) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int* c = (int*)ctl;
    const int step = c[VT_EMA_STEP], period = c[VT_EMA_PERIOD] < 1 ? 1 : c[VT_EMA_PERIOD];
    int mode = VT_EMA_SKIP;
    if (step % period == 0) {  // optimiser steps are numbered from 0: steps 0, k, 2k, .. move the average
        mode = c[VT_EMA_COUNT] == 0 ? VT_EMA_COPY : VT_EMA_BLEND;
        c[VT_EMA_COUNT] += 1;
    }
    c[VT_EMA_STEP] = step + 1;
    c[VT_EMA_MODE] = mode;
}

__device__ __forceinline__ float ema_blend(float e, float p, float alpha) { return fmaf(alpha, p - e, e); }

template <bool kMirror>
__global__ void __launch_bounds__(kEmaThreads)
ema_update_kernel(float* __restrict__ e, const float* __restrict__ p, bf16_t* __restrict__ mirror, long n,
                  const float* __restrict__ ctl) {
    const int mode = ((const int*)ctl)[VT_EMA_MODE];  // (uniform: a scalar load)
    if (mode != VT_EMA_COPY && mode != VT_EMA_BLEND) return;
    const bool blend = mode == VT_EMA_BLEND;
    const float alpha = ctl[VT_EMA_ALPHA];
    const long n4 = n >> 2, stride = (long)gridDim.x * kEmaThreads;
    for (long c = (long)blockIdx.x * kEmaThreads + threadIdx.x; c < n4; c += stride) {
        float4 v = ((const float4*)p)[c];
        if (blend) {
            const float4 ev = ((const float4*)e)[c];
            v.x = ema_blend(ev.x, v.x, alpha), v.y = ema_blend(ev.y, v.y, alpha);
            v.z = ema_blend(ev.z, v.z, alpha), v.w = ema_blend(ev.w, v.w, alpha);
        }
        ((float4*)e)[c] = v;
        if constexpr (kMirror)
            ((uint2*)mirror)[c] = make_uint2(VecIO<bf16_t>::pack2(v.x, v.y), VecIO<bf16_t>::pack2(v.z, v.w));
    }
    // n % 4 != 0: the last 1..3 elements, one lane each
    const long i = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && i < n) {
        float v = p[i];
        if (blend) v = ema_blend(e[i], v, alpha);
        e[i] = v;
        if constexpr (kMirror) mirror[i] = (bf16_t)v;
    }
}

__global__ void __launch_bounds__(kEmaThreads)
ema_copy_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, long n16, const float* __restrict__ ctl) {
    const int mode = ((const int*)ctl)[VT_EMA_MODE];
    if (mode != VT_EMA_COPY && mode != VT_EMA_BLEND) return;
    const long stride = (long)gridDim.x * kEmaThreads;
    for (long c = (long)blockIdx.x * kEmaThreads + threadIdx.x; c < n16; c += stride) dst[c] = src[c];
}

unsigned stream_blocks(long chunks) {
    const long b = (chunks + kEmaThreads - 1) / kEmaThreads;
    return (unsigned)(b < 1 ? 1 : (b < kEmaMaxBlocks ? b : kEmaMaxBlocks));
}

}  // namespace

extern "C" {

int64_t vt_ema_grid_cap(void) { return (int64_t)kEmaMaxBlocks * kEmaThreads * 4; }

int vt_ema_tick(float* ctl, void* stream) {
    VT_REQUIRE(ctl && vt_aligned16(ctl), VT_ERR_INVALID, "vt_ema_tick: ctl must be a 16-byte aligned device float[8]");
    hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl);
    VT_CHECK_LAUNCH("vt_ema_tick");
    return VT_OK;
}

int vt_ema_update(float* ema, const float* p, void* ema_mirror, int64_t n, const float* ctl, void* stream) {
    VT_REQUIRE(ema && p && ctl && n > 0, VT_ERR_INVALID, "vt_ema_update: bad argument (null ema / p / ctl, or n <= 0)");
    VT_REQUIRE(vt_aligned16(ema) && vt_aligned16(p) && vt_aligned16(ctl) && ((uintptr_t)ema_mirror & 7) == 0, VT_ERR_INVALID,
               "vt_ema_update: ema, p and ctl must be 16-byte aligned, the bf16 mirror 8-byte aligned");
    VT_REQUIRE(ema != p, VT_ERR_INVALID, "vt_ema_update: ema and p are the same buffer");
    const unsigned blocks = stream_blocks(n >> 2);
    if (ema_mirror)
        hipLaunchKernelGGL(ema_update_kernel<true>, dim3(blocks), dim3(kEmaThreads), 0, (hipStream_t)stream, ema, p,
                           (bf16_t*)ema_mirror, (long)n, ctl);
    else
        hipLaunchKernelGGL(ema_update_kernel<false>, dim3(blocks), dim3(kEmaThreads), 0, (hipStream_t)stream, ema, p,
                           (bf16_t*)nullptr, (long)n, ctl);
    VT_CHECK_LAUNCH("vt_ema_update");
    return VT_OK;
}

int vt_ema_copy(void* dst, const void* src, int64_t bytes, const float* ctl, void* stream) {
    VT_REQUIRE(dst && src && ctl && bytes > 0 && bytes % 16 == 0, VT_ERR_INVALID,
               "vt_ema_copy: bad argument (null dst / src / ctl, or bytes no positive multiple of 16)");
    VT_REQUIRE(vt_aligned16(dst) && vt_aligned16(src) && vt_aligned16(ctl) && dst != src, VT_ERR_INVALID,
               "vt_ema_copy: dst, src and ctl must be 16-byte aligned, dst and src distinct");
    hipLaunchKernelGGL(ema_copy_kernel, dim3(stream_blocks(bytes / 16)), dim3(kEmaThreads), 0, (hipStream_t)stream, (uint4*)dst,
                       (const uint4*)src, (long)(bytes / 16), ctl);
    VT_CHECK_LAUNCH("vt_ema_copy");
    return VT_OK;
}

}  // extern "C"
