// vt_lamb.hip -- what sits between the backward pass and the weights besides SGD / AdamW (vt_elementwise.hip):
// the global gradient norm, the clip factor made from it, and LAMB (timm.optim.Lamb's form, include/vt_amd.h).
//
// One primitive serves all of it: a deterministic sum of squares over a flat f32 buffer.  The buffer is cut into ITEMS of
// VT_OPT_ITEM elements; a workgroup reduces an item to one double and writes it with a plain store, so the set of partials
// -- and every sum formed from it -- depends on the buffer alone, never on the grid, the CU count or the order workgroups
// finish in.  No kernel here uses a float atomic, and no value is handed from one workgroup to another inside a launch:
// whoever needs a total adds the partials of an EARLIER launch in its own prologue (the launch-boundary reduce).
//
// The order of every sum (kOptThreads = 256 lanes, item = 4096 elements = 4 rounds of one float4 per lane):
//   lane:   f32, fmaf(x, x, acc) over its <= 16 elements in address order         (<= 16 roundings of 2^-24)
//   wave:   the lanes' values as doubles, xor-butterfly 32, 16, .. 1              (double: 2^-53 per level)
//   block:  ((w0 + w1) + w2) + w3 through LDS                                      (double)
//   total:  lane t adds partials t, t + 256, .. ascending, then the same wave / block tree (double)
#include "vt_common.h"

namespace {

constexpr int kOptThreads = 256;
constexpr int kItem = VT_OPT_ITEM;
constexpr int kRounds = kItem / (kOptThreads * 4);
static_assert(kItem == kRounds * kOptThreads * 4, "an item is whole rounds of one float4 per lane");
static_assert(kItem % 64 == 0, "store slots are multiples of 64: an item boundary never cuts a 16-byte chunk");

// both sums of every lane -> both totals in every lane; lds holds 2 * (kOptThreads / 64) doubles.  Called by all threads.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[2 * w] = a, lds[2 * w + 1] = b;
    __syncthreads();
    a = lds[0], b = lds[1];
#pragma unroll
    for (int k = 1; k < kOptThreads / 64; ++k) a += lds[2 * k], b += lds[2 * k + 1];
    __syncthreads();  // (the next item of this workgroup writes lds again)
}

// ---------------------------------------------------------------------------------
// sum of squares of g[0..n): one double per item
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kOptThreads)
grad_sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ partials, long n_items) {
    __shared__ double lds[2 * (kOptThreads / 64)];
    for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const long base = it * kItem;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            const long i = base + (long)(k * kOptThreads + threadIdx.x) * 4;
            if (i + 4 <= n) {
                const float4 x = *(const float4*)(g + i);
                acc = fmaf(x.x, x.x, acc), acc = fmaf(x.y, x.y, acc), acc = fmaf(x.z, x.z, acc), acc = fmaf(x.w, x.w, acc);
            } else {
                for (long j = i; j < n; ++j) acc = fmaf(g[j], g[j], acc);  // (n % 4 != 0: the last chunk, one lane)
            }
        }
        double a = (double)acc, b = 0.0;
        block_sum2(a, b, lds);
        if (threadIdx.x == 0) partials[it] = a;
    }
}

// ---------------------------------------------------------------------------------
// partials -> N = grad_scale * sqrt(sum), and the factor grad_scale * c1 / c2 every consumer multiplies g by
// ---------------------------------------------------------------------------------
__device__ __forceinline__ bool threshold_on(float t) { return t > 0.f && t < __builtin_inff(); }

__global__ void __launch_bounds__(kOptThreads)
clip_coef_kernel(const double* __restrict__ partials, long n_items, double gs, float* __restrict__ ctl) {
    __shared__ double lds[2 * (kOptThreads / 64)];
    double a = 0.0, b = 0.0;
    for (long j = threadIdx.x; j < n_items; j += kOptThreads) a += partials[j];
    block_sum2(a, b, lds);
    if (threadIdx.x != 0) return;
    const float C = ctl[VT_CTL_CLIP], M = ctl[VT_CTL_LAMB_MAX];
    const double N = gs * sqrt(a);
    double c1 = 1.0, c2 = 1.0;
    if (threshold_on(C)) {
        const double q = (double)C / (N + 1e-6);  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
        c1 = q > 1.0 ? 1.0 : q;                    // (a NaN norm stays a NaN factor, as torch.clamp keeps it)
    }
    if (threshold_on(M)) {
        const double N1 = c1 * N;  // LAMB's own clip sees the clipped gradient
        if (N1 > (double)M) c2 = N1 / (double)M;  // (false for NaN: 1)
    }
    ctl[VT_CTL_FACTOR] = (float)(gs * c1 / c2);
    ctl[VT_CTL_NORM] = (float)N;
}

// ---------------------------------------------------------------------------------
// LAMB over (tensor, item) work items
// ---------------------------------------------------------------------------------
struct LambScalars {
    float beta1, omb1, beta2, omb2, eps;  // omb = 1 - beta, rounded from double on the host (as vt_adamw)
    int trust_clip, always_adapt;
};

// the update direction of one element, from the NEW moments and the OLD weight.  Both passes call this and nothing else,
// with explicit fused operations only, so the second pass re-forms the bits the first pass summed.
__device__ __forceinline__ float lamb_u(float p, float m, float v, float bc1, float bc2s, float eps, float wd) {
    return fmaf(wd, p, (m / bc1) / (sqrtf(v) / bc2s + eps));  // correctly rounded sqrt and divisions (no -ffast-math here)
}

struct LambItem {
    long base;  // element offset of the item in the flat buffers; < 0: the table entry is not usable
    int cnt;    // elements (a multiple of 64)
    int item0, n_it;
    float wd;
};

// table: int32[n_segs][4] = (element offset, elements, first item, weight decay as float bits), then int32[n_items] =
// the segment of each item.  Every field is checked against the buffer length before anything is addressed with it.
__device__ __forceinline__ LambItem lamb_item(const int* __restrict__ table, int n_segs, long it, long n_items, long n_total) {
    LambItem r;
    r.base = -1, r.cnt = 0, r.item0 = 0, r.n_it = 0, r.wd = 0.f;
    const int s = table[4L * n_segs + it];
    if (s < 0 || s >= n_segs) return r;
    const int4 e = *(const int4*)(table + 4L * s);
    const long off = e.x, n = e.y, j = it - e.z;
    const long n_it = (n + kItem - 1) / kItem;
    if (off < 0 || n <= 0 || ((off | n) & 63) || off + n > n_total || j < 0 || j >= n_it || e.z < 0 || e.z + n_it > n_items)
        return r;
    r.base = off + j * kItem;
    r.cnt = (int)(n - j * kItem < kItem ? n - j * kItem : kItem);
    r.item0 = e.z, r.n_it = (int)n_it;
    r.wd = __int_as_float(e.w);
    return r;
}

__global__ void __launch_bounds__(kOptThreads)
lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                    const int* __restrict__ table, int n_segs, long n_items, long n_total, double* __restrict__ partials,
                    const float* __restrict__ coef, LambScalars a, const float* __restrict__ hyper) {
    __shared__ double lds[2 * (kOptThreads / 64)];
    const float gs = coef[0], bc1 = hyper[5], bc2s = hyper[6];
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const LambItem w = lamb_item(table, n_segs, it, n_items, n_total);
        if (w.base < 0) {  // (uniform over the workgroup)
            if (threadIdx.x == 0) partials[2 * it] = qnan, partials[2 * it + 1] = qnan;
            continue;
        }
        float sp = 0.f, su = 0.f;
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            const int i = (k * kOptThreads + threadIdx.x) * 4;
            if (i < w.cnt) {
                const float4 pv = *(const float4*)(p + w.base + i);
                const float4 gv = *(const float4*)(g + w.base + i);
                float4 mv = *(float4*)(m + w.base + i);
                float4 vv = *(float4*)(v + w.base + i);
                const float* pp = (const float*)&pv;
                const float* gp = (const float*)&gv;
                float* mp = (float*)&mv;
                float* vp = (float*)&vv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float gg = gp[e] * gs;
                    mp[e] = fmaf(a.beta1, mp[e], a.omb1 * gg);
                    vp[e] = fmaf(a.beta2, vp[e], a.omb2 * gg * gg);
                    const float u = lamb_u(pp[e], mp[e], vp[e], bc1, bc2s, a.eps, w.wd);
                    sp = fmaf(pp[e], pp[e], sp);
                    su = fmaf(u, u, su);
                }
                *(float4*)(m + w.base + i) = mv;
                *(float4*)(v + w.base + i) = vv;
            }
        }
        double dp = (double)sp, du = (double)su;
        block_sum2(dp, du, lds);
        if (threadIdx.x == 0) partials[2 * it] = dp, partials[2 * it + 1] = du;
    }
}

template <typename MT>
__global__ void __launch_bounds__(kOptThreads)
lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, MT* __restrict__ mirror,
                  const int* __restrict__ table, int n_segs, long n_items, long n_total,
                  const double* __restrict__ partials, LambScalars a, const float* __restrict__ hyper) {
    __shared__ double lds[2 * (kOptThreads / 64)];
    const float lr = hyper[0], bc1 = hyper[5], bc2s = hyper[6];
    for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const LambItem w = lamb_item(table, n_segs, it, n_items, n_total);
        if (w.base < 0) continue;
        float r = 1.f;
        if (w.wd != 0.f || a.always_adapt) {  // (uniform over the workgroup)
            // the tensor's two sums: every workgroup of the tensor adds the same partials in the same order
            double sp = 0.0, su = 0.0;
            for (int j = threadIdx.x; j < w.n_it; j += kOptThreads)
                sp += partials[2L * (w.item0 + j)], su += partials[2L * (w.item0 + j) + 1];
            block_sum2(sp, su, lds);
            if (sp > 0.0 && su > 0.0) r = (float)(sqrt(sp) / sqrt(su));  // (false for NaN: 1, and u carries the NaN)
            if (a.trust_clip) r = fminf(r, 1.f);
        }
        const float step = lr * r;
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            const int i = (k * kOptThreads + threadIdx.x) * 4;
            if (i < w.cnt) {
                float4 pv = *(float4*)(p + w.base + i);
                const float4 mv = *(const float4*)(m + w.base + i);
                const float4 vv = *(const float4*)(v + w.base + i);
                float* pp = (float*)&pv;
                const float* mp = (const float*)&mv;
                const float* vp = (const float*)&vv;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    pp[e] = fmaf(-step, lamb_u(pp[e], mp[e], vp[e], bc1, bc2s, a.eps, w.wd), pp[e]);
                *(float4*)(p + w.base + i) = pv;
                if (mirror) {
                    if constexpr (sizeof(MT) == 2)
                        *(uint2*)(mirror + w.base + i) =
                            make_uint2(VecIO<bf16_t>::pack2(pp[0], pp[1]), VecIO<bf16_t>::pack2(pp[2], pp[3]));
                    else
                        *(float4*)(mirror + w.base + i) = pv;
                }
            }
        }
    }
}

unsigned item_blocks(long n_items) {
    return (unsigned)(n_items < 8192 ? n_items : 8192);  // (no result depends on it: a workgroup loops over items)
}

int lamb_scalars(const char* who, double beta1, double beta2, float eps, int32_t flags, LambScalars* a) {
    VT_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f, VT_ERR_INVALID,
               "%s: betas in [0, 1), eps >= 0", who);
    a->beta1 = (float)beta1, a->omb1 = (float)(1.0 - beta1), a->beta2 = (float)beta2, a->omb2 = (float)(1.0 - beta2);
    a->eps = eps, a->trust_clip = (flags & VT_LAMB_TRUST_CLIP) ? 1 : 0, a->always_adapt = (flags & VT_LAMB_ALWAYS_ADAPT) ? 1 : 0;
    return VT_OK;
}

}  // namespace

extern "C" {

int32_t vt_opt_item(void) { return kItem; }

int vt_grad_sumsq(const float* g, int64_t n, double* partials, void* stream) {
    VT_REQUIRE(g && partials && n > 0, VT_ERR_INVALID, "vt_grad_sumsq: bad argument");
    VT_REQUIRE(vt_aligned16(g) && ((uintptr_t)partials & 7) == 0, VT_ERR_INVALID,
               "vt_grad_sumsq: g must be 16-byte aligned, partials 8-byte aligned");
    const long n_items = VT_OPT_ITEMS(n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(item_blocks(n_items)), dim3(kOptThreads), 0, (hipStream_t)stream, g, (long)n,
                       partials, n_items);
    VT_CHECK_LAUNCH("vt_grad_sumsq");
    return VT_OK;
}

int vt_clip_coef(const double* partials, int64_t n_items, float grad_scale, float* ctl, void* stream) {
    VT_REQUIRE(partials && ctl && n_items > 0, VT_ERR_INVALID, "vt_clip_coef: bad argument");
    VT_REQUIRE(((uintptr_t)partials & 7) == 0 && vt_aligned16(ctl), VT_ERR_INVALID,
               "vt_clip_coef: partials must be 8-byte aligned, ctl 16-byte aligned");
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(kOptThreads), 0, (hipStream_t)stream, partials, (long)n_items,
                       (double)grad_scale, ctl);
    VT_CHECK_LAUNCH("vt_clip_coef");
    return VT_OK;
}

int vt_lamb_moments(const float* p, const float* g, float* m, float* v, const int32_t* table, int32_t n_segs,
                    int64_t n_items, int64_t n_total, double* partials, const float* coef, double beta1, double beta2,
                    float eps, int32_t flags, const float* hyper, void* stream) {
    VT_REQUIRE(p && g && m && v && table && partials && coef && hyper && n_segs > 0 && n_items > 0 && n_total > 0 &&
                   n_total < (1LL << 31),
               VT_ERR_INVALID, "vt_lamb_moments: bad argument");
    VT_REQUIRE(vt_aligned16(p) && vt_aligned16(g) && vt_aligned16(m) && vt_aligned16(v) && vt_aligned16(table) &&
                   ((uintptr_t)partials & 7) == 0,
               VT_ERR_INVALID, "vt_lamb_moments: p/g/m/v/table must be 16-byte aligned, partials 8-byte aligned");
    LambScalars a;
    VT_TRY(lamb_scalars("vt_lamb_moments", beta1, beta2, eps, flags, &a));
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(item_blocks(n_items)), dim3(kOptThreads), 0, (hipStream_t)stream, p, g, m, v,
                       (const int*)table, n_segs, (long)n_items, (long)n_total, partials, coef, a, hyper);
    VT_CHECK_LAUNCH("vt_lamb_moments");
    return VT_OK;
}

int vt_lamb_apply(float* p, const float* m, const float* v, void* mirror, int32_t mirror_dtype, const int32_t* table,
                  int32_t n_segs, int64_t n_items, int64_t n_total, const double* partials, float eps, int32_t flags,
                  const float* hyper, void* stream) {
    VT_REQUIRE(p && m && v && table && partials && hyper && n_segs > 0 && n_items > 0 && n_total > 0 && n_total < (1LL << 31),
               VT_ERR_INVALID, "vt_lamb_apply: bad argument");
    VT_REQUIRE(vt_aligned16(p) && vt_aligned16(m) && vt_aligned16(v) && vt_aligned16(table) && ((uintptr_t)partials & 7) == 0,
               VT_ERR_INVALID, "vt_lamb_apply: p/m/v/table must be 16-byte aligned, partials 8-byte aligned");
    const bool bf = mirror && mirror_dtype == VT_BF16;
    if (mirror && !bf && mirror_dtype != VT_F32) {
        vt_set_error("vt_lamb_apply: mirror dtype %d", mirror_dtype);
        return VT_ERR_UNSUPPORTED;
    }
    VT_REQUIRE(!mirror || ((uintptr_t)mirror & (bf ? 7 : 15)) == 0, VT_ERR_INVALID,
               "vt_lamb_apply: the mirror must be aligned to four of its elements");
    LambScalars a;
    VT_TRY(lamb_scalars("vt_lamb_apply", 0.0, 0.0, eps, flags, &a));
    const unsigned blocks = item_blocks(n_items);
    if (bf)
        hipLaunchKernelGGL(lamb_apply_kernel<bf16_t>, dim3(blocks), dim3(kOptThreads), 0, (hipStream_t)stream, p, m, v,
                           (bf16_t*)mirror, (const int*)table, n_segs, (long)n_items, (long)n_total, partials, a, hyper);
    else
        hipLaunchKernelGGL(lamb_apply_kernel<float>, dim3(blocks), dim3(kOptThreads), 0, (hipStream_t)stream, p, m, v,
                           (float*)mirror, (const int*)table, n_segs, (long)n_items, (long)n_total, partials, a, hyper);
    VT_CHECK_LAUNCH("vt_lamb_apply");
    return VT_OK;
}

}  // extern "C"
