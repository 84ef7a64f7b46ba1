// vt_bce.hip -- binary cross-entropy on logits against the smoothed, optionally mixed and thresholded one-hot target
// (the definition is in include/vt_amd.h), with its gradient, for the fused train step (loss="bce").
//
// Two launches behind one entry point, no float atomic, nothing handed from one workgroup to another inside a launch:
//   bce_rows_kernel   one workgroup per row: writes the row's gradient and ONE double, the row's sum of element losses,
//                     with a plain store into rows[b]
//   bce_total_kernel  one workgroup: adds rows[0], rows[1], .. rows[B-1] in that order in double, loss[0] += total / D
// so the loss is a fixed-order sum -- two runs give the same bits, whatever order the rows finish in.
//
// The order of a row's sum (kBceThreads = 256 lanes):
//   lane:   double, its elements t, t + 256, .. in address order (each element loss is formed in f32 first)
//   wave:   xor butterfly 32, 16, .. 1 in double
//   block:  ((w0 + w1) + w2) + w3 through LDS
#include "vt_common.h"

namespace {

constexpr int kBceThreads = 256;

template <typename T>
__device__ __forceinline__ float ldf(const T* p) { return (float)(*p); }

struct BceArgs {
    float eps, gscale, thr;  // label smoothing; grad_scale * (sum_classes ? 1 : 1 / N); the target threshold
    int use_thr;
};

template <typename T>
__global__ void __launch_bounds__(kBceThreads)
bce_rows_kernel(const T* __restrict__ logits, int ldl, const int64_t* __restrict__ labels, BceArgs a,
                double* __restrict__ rows, T* __restrict__ dlogits, int lddl, int B, int N, const float* __restrict__ mix) {
    __shared__ double lds[kBceThreads / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const T* lp = logits + (long)b * ldl;
    const int64_t yb = labels[b];
    // MixUp / CutMix: the partner of sample b is sample b-1 (mod B), as in xent_kernel
    const bool mixed = mix && mix[0] != 0.f;
    const float lam = mixed ? mix[1] : 1.f;
    const int64_t yp = mixed ? labels[(b + B - 1) % B] : yb;
    // a label outside [0, N): it is only ever compared with a column index, never added to a pointer; the row's loss
    // term becomes NaN so that the bad batch is noticed
    const bool bad = yb < 0 || yb >= (int64_t)N || yp < 0 || yp >= (int64_t)N;
    const float keep = 1.f - a.eps, off = a.eps / (float)N;
    const float wb = keep * lam, wp = keep * (1.f - lam);
    T* dp = dlogits ? dlogits + (long)b * lddl : nullptr;
    double acc = 0.0;
    for (int i = t; i < N; i += kBceThreads) {
        const float x = ldf(lp + i);
        float m = 0.f;  // (1 - s) * mixed one-hot: the two terms add when both labels name this column
        if ((int64_t)i == yb) m += wb;
        if ((int64_t)i == yp) m += wp;
        float tg = m + off;
        if (a.use_thr) tg = tg > a.thr ? 1.f : 0.f;
        // e = exp(-|x|) in (0, 1] serves both the softplus term and the sigmoid: nothing overflows for any finite x,
        // and x * tg with tg in [0, 1] stays finite
        const float e = expf(-fabsf(x));
        const float l = (fmaxf(x, 0.f) - x * tg) + log1pf(e);
        acc += (double)l;
        if (dp) {
            const float r = 1.f / (1.f + e);
            const float sg = x >= 0.f ? r : e * r;
            dp[i] = from_float<T>((sg - tg) * a.gscale);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((t & 63) == 0) lds[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        double s = lds[0];
#pragma unroll
        for (int k = 1; k < kBceThreads / 64; ++k) s += lds[k];
        rows[b] = bad ? __longlong_as_double(0x7ff8000000000000LL) : s;
    }
}

// rows[0..B) were written by the launch before this one.  Staged through LDS a chunk at a time so that the loads run in
// parallel; the additions are one chain in ascending row order.
__global__ void __launch_bounds__(kBceThreads)
bce_total_kernel(const double* __restrict__ rows, int B, double inv_d, float* __restrict__ loss) {
    __shared__ double lds[kBceThreads];
    double total = 0.0;
    for (int base = 0; base < B; base += kBceThreads) {
        const int n = B - base < kBceThreads ? B - base : kBceThreads;
        if ((int)threadIdx.x < n) lds[threadIdx.x] = rows[base + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < n; ++k) total += lds[k];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] += (float)(total * inv_d);
}

}  // namespace

extern "C" {

int vt_sigmoid_bce(const void* logits, int32_t ldl, const int64_t* labels, float label_smoothing, float grad_scale,
                   float* loss, void* dlogits, int32_t lddl, int32_t B, int32_t N, int32_t dtype, const float* mix,
                   int32_t flags, float target_threshold, double* rows, void* stream) {
    VT_REQUIRE(logits && labels && loss && rows && B > 0 && N > 0 && ldl >= N, VT_ERR_INVALID, "vt_sigmoid_bce: bad argument");
    VT_REQUIRE(!dlogits || lddl >= N, VT_ERR_INVALID, "vt_sigmoid_bce: lddl < N");
    VT_REQUIRE(((uintptr_t)rows & 7) == 0, VT_ERR_INVALID, "vt_sigmoid_bce: rows must be 8-byte aligned");
    VT_REQUIRE((flags & ~(VT_BCE_SUM_CLASSES | VT_BCE_THRESHOLD)) == 0, VT_ERR_INVALID, "vt_sigmoid_bce: unknown flag in %d",
               flags);
    VT_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, VT_ERR_INVALID, "vt_sigmoid_bce: label_smoothing in [0, 1]");
    VT_REQUIRE(!(flags & VT_BCE_THRESHOLD) || target_threshold == target_threshold, VT_ERR_INVALID,
               "vt_sigmoid_bce: the target threshold is NaN");
    const bool sum_classes = (flags & VT_BCE_SUM_CLASSES) != 0;
    BceArgs a;
    a.eps = label_smoothing;
    a.gscale = sum_classes ? grad_scale : grad_scale * (1.f / (float)N);
    a.use_thr = (flags & VT_BCE_THRESHOLD) ? 1 : 0;
    a.thr = a.use_thr ? target_threshold : 0.f;
    const double inv_d = 1.0 / ((double)B * (sum_classes ? 1.0 : (double)N));
    VT_DISPATCH_T(dtype, "vt_sigmoid_bce",
                  hipLaunchKernelGGL(bce_rows_kernel<T>, dim3(B), dim3(kBceThreads), 0, (hipStream_t)stream, (const T*)logits,
                                     ldl, labels, a, rows, (T*)dlogits, lddl, B, N, mix));
    VT_CHECK_LAUNCH("vt_sigmoid_bce");
    hipLaunchKernelGGL(bce_total_kernel, dim3(1), dim3(kBceThreads), 0, (hipStream_t)stream, (const double*)rows, B, inv_d,
                       loss);
    VT_CHECK_LAUNCH("vt_sigmoid_bce");
    return VT_OK;
}

}  // extern "C"
