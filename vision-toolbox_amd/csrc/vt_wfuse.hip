// vt_wfuse.hip -- the weighted fusion node of BiFPN (reference necks.py:197-215, WeightedFeatureFusion.forward):
//
//   out = (sum_i relu(w)_i * R_i(x_i)) / (sum_i relu(w)_i + eps),   i < n, n in {2, 3}
//
// R_i is the identity (code 0), nearest x2 (code 1: the source is [B][H/2][W/2][C], read at (i/2, j/2)) or nearest x0.5
// (code 2: the source is [B][2H][2W][C], read at (2i, 2j)) -- the index maps of vt_resample2x_add_fwd modes 0 and 1.  The
// raw parameter `w` is a device float[n]: every thread applies the ReLU and forms 1 / (sum + eps) itself, so nothing is
// read back on the host, the launches sit in a captured graph and follow the optimiser's updates.
//
// Memory-bound streaming kernels over NHWC rows (pixel stride ld >= C, channel slices work), one 16-byte chunk per thread
// and pixel, f32 arithmetic, one rounding at the store.  No resampled or scaled map is ever written.
//
// Backward is ONE launch per node.  Its work item is a 2x2 block of OUTPUT pixels times one channel chunk: the block is
// what a code-1 input's gradient sums over and what a code-2 input's even/even pixels map onto, so every input gradient is
// written by exactly one thread and needs no atomics.  The sums behind the weight gradients,
//   T_i = sum_{pixels, channels} g * (R_i(x_i) - out),     out recomputed in f32 from the inputs (never read back rounded),
// are formed as a per-thread f32 partial over the item (4 pixels x 8 bf16 or 4 f32 channels: at most 32 terms), added to a
// per-thread double, folded in double over the wave (shuffles) and the workgroup (LDS) and handed over as ONE fixed-point
// integer atomic per input and workgroup into a replicated channel-sums buffer (int64[VT_STAT_REPLICAS][1][n][2], the format
// vt_stat_sum reads).  Integer atomics are associative: every run is bit-identical, deterministic mode needs nothing extra.
//
// WHERE THE TWO SCALAR FACTORS LIVE: vt_wfuse_bwd hands over the raw T_i.  vt_wfuse_finalize applies both [w_i > 0] (torch's
// relu'(0) = 0) and 1 / (sum + eps), in double, and adds the n results to the parameter-gradient slots; a weight that is not
// positive gets no add at all, so its gradient stays exactly what it was.
#include "vt_common.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kMaxIn = 3;

struct FuseIn {
    const void* x[kMaxIn];
    int ld[kMaxIn];
    int code[kMaxIn];
};

struct FuseGrad {
    void* dx[kMaxIn];
    int ld[kMaxIn];
    int acc[kMaxIn];
};

// relu(w) as torch computes it: a NaN weight stays NaN
__device__ __forceinline__ float relu_w(float w) { return w <= 0.f ? 0.f : w; }

// pixel index of input `code` that output pixel (b, i, j) of an [B][H][W] grid reads
__device__ __forceinline__ long src_pixel(int code, long b, int i, int j, int H, int W) {
    if (code == 1) return (b * (H >> 1) + (i >> 1)) * (long)(W >> 1) + (j >> 1);
    if (code == 2) return (b * (2L * H) + 2L * i) * (2L * W) + 2L * j;
    return (b * H + i) * (long)W + j;
}

template <typename T, int N>
__global__ void __launch_bounds__(kT) wfuse_fwd_kernel(FuseIn in, const float* __restrict__ weights, float eps,
                                                       T* __restrict__ out, int ldo, int B, int H, int W, int cpr) {
    constexpr int EPC = VecIO<T>::EPC;
    float r[N], sum = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        r[k] = relu_w(weights[k]);
        sum += r[k];
    }
    const float inv = 1.0f / (sum + eps);
    const long total = (long)B * H * W * cpr;
    for (long idx = (long)blockIdx.x * kT + threadIdx.x; idx < total; idx += (long)gridDim.x * kT) {
        const int ch = (int)(idx % cpr);
        const long p = idx / cpr;
        const int j = (int)(p % W);
        const long q = p / W;
        const int i = (int)(q % H);
        const long b = q / H;
        float acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const T* x = (const T*)in.x[k];
            float v[EPC];
            VecIO<T>::unpack(*(const uint4*)(x + src_pixel(in.code[k], b, i, j, H, W) * in.ld[k] + ch * EPC), v);
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaf(r[k], v[e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] *= inv;
        *(uint4*)(out + p * ldo + ch * EPC) = VecIO<T>::pack(acc);
    }
}

// the fixed-point add of vt_common.h (vt_stat_add) for a double: the split is exact, so the hand-over loses nothing
__device__ __forceinline__ void stat_add_f64(float* stats, long idx, double v) {
    unsigned long long* q = (unsigned long long*)stats + 2 * idx;
    if (!(fabs(v) < (double)kStatLimit)) {  // non-finite or beyond the legitimate range: the marker vt_stat_sum turns into NaN
        atomicAdd(q, (unsigned long long)kStatPoison);
        return;
    }
    const double hf = trunc(v * (1.0 / 4096.0));
    const double rem = v - hf * 4096.0;  // exact: |rem| < 4096
    atomicAdd(q + 1, (unsigned long long)__double2ll_rn(rem * 8589934592.0));  // 2^33
    if (hf != 0.0) atomicAdd(q, (unsigned long long)(long long)hf);
}

template <typename T>
__device__ __forceinline__ void store_grad(T* dst, const float* v, bool acc) {
    constexpr int EPC = VecIO<T>::EPC;
    float o[EPC];
    if (acc) {
        VecIO<T>::unpack(*(const uint4*)dst, o);
#pragma unroll
        for (int e = 0; e < EPC; ++e) o[e] += v[e];
    } else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) o[e] = v[e];
    }
    *(uint4*)dst = VecIO<T>::pack(o);
}

template <typename T, int N>
__global__ void __launch_bounds__(kT) wfuse_bwd_kernel(FuseIn in, FuseGrad gr, const T* __restrict__ g, int ldg,
                                                       const float* __restrict__ weights, float eps, float* sums, int B, int H,
                                                       int W, int cpr) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ double red[kWaves][kMaxIn];
    float r[N], s[N], sum = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        r[k] = relu_w(weights[k]);
        sum += r[k];
    }
    const float inv = 1.0f / (sum + eps);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = r[k] * inv;
    const int Hb = (H + 1) >> 1, Wb = (W + 1) >> 1;
    double wide[N];
#pragma unroll
    for (int k = 0; k < N; ++k) wide[k] = 0.0;
    const long total = (long)B * Hb * Wb * cpr;
    for (long idx = (long)blockIdx.x * kT + threadIdx.x; idx < total; idx += (long)gridDim.x * kT) {
        const int ch = (int)(idx % cpr);
        const long p = idx / cpr;
        const int bj = (int)(p % Wb);
        const long q = p / Wb;
        const int bi = (int)(q % Hb);
        const long b = q / Hb;
        float part[N], xv[N][EPC], gsum[EPC];  // part: at most 4 pixels x EPC <= 32 terms
#pragma unroll
        for (int k = 0; k < N; ++k) {
            part[k] = 0.f;
            if (in.code[k] == 1)  // one source pixel serves the whole block (H and W are even then)
                VecIO<T>::unpack(*(const uint4*)((const T*)in.x[k] + src_pixel(1, b, 2 * bi, 2 * bj, H, W) * in.ld[k] + ch * EPC),
                                 xv[k]);
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) gsum[e] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 2 * bi + (t >> 1), j = 2 * bj + (t & 1);
            if (i >= H || j >= W) continue;
            const long po = (b * H + i) * (long)W + j;
            float gv[EPC], o[EPC];
            VecIO<T>::unpack(*(const uint4*)(g + po * ldg + ch * EPC), gv);
#pragma unroll
            for (int e = 0; e < EPC; ++e) o[e] = 0.f, gsum[e] += gv[e];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                if (in.code[k] != 1)
                    VecIO<T>::unpack(*(const uint4*)((const T*)in.x[k] + src_pixel(in.code[k], b, i, j, H, W) * in.ld[k] + ch * EPC),
                                     xv[k]);
#pragma unroll
                for (int e = 0; e < EPC; ++e) o[e] = fmaf(r[k], xv[k][e], o[e]);
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) o[e] *= inv;  // the forward's arithmetic, unrounded
#pragma unroll
            for (int k = 0; k < N; ++k) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) part[k] = fmaf(gv[e], xv[k][e] - o[e], part[k]);
                T* dx = (T*)gr.dx[k];
                if (!dx || in.code[k] == 1) continue;
                float v[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) v[e] = s[k] * gv[e];
                const long ps = src_pixel(in.code[k], b, i, j, H, W);
                const long ld = gr.ld[k];
                store_grad<T>(dx + ps * ld + ch * EPC, v, gr.acc[k] != 0);
                if (in.code[k] == 2 && !gr.acc[k]) {  // the three pixels of the source that no output pixel reads
                    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
                    *(uint4*)(dx + (ps + 1) * ld + ch * EPC) = z;
                    *(uint4*)(dx + (ps + 2L * W) * ld + ch * EPC) = z;
                    *(uint4*)(dx + (ps + 2L * W + 1) * ld + ch * EPC) = z;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            wide[k] += (double)part[k];
            T* dx = (T*)gr.dx[k];
            if (!dx || in.code[k] != 1) continue;
            float v[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) v[e] = s[k] * gsum[e];
            store_grad<T>(dx + src_pixel(1, b, 2 * bi, 2 * bj, H, W) * gr.ld[k] + ch * EPC, v, gr.acc[k] != 0);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double v = wide[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += red[w][threadIdx.x];
        stat_add_f64(sums, (long)(blockIdx.x % kStatReplicas) * N + threadIdx.x, v);
    }
}

__global__ void wfuse_finalize_kernel(const float* __restrict__ sums, const float* __restrict__ weights, float eps, int n,
                                      float* dw) {
    const int k = threadIdx.x;
    if (k >= n) return;
    float sum = 0.f;
    for (int m = 0; m < n; ++m) sum += relu_w(weights[m]);
    if (weights[k] <= 0.f) return;  // relu'(w <= 0) = 0: nothing is added
    dw[k] += (float)(vt_stat_sum(sums, k, n) / (double)(sum + eps));
}

int check_map(const char* who, const char* what, int k, const void* p, int ld, int C, int dtype) {
    const int epc = vt_epc(dtype);
    VT_REQUIRE(p && vt_aligned16(p), VT_ERR_INVALID, "%s: %s%d is null or misaligned", who, what, k);
    VT_REQUIRE(ld >= C && ld % epc == 0, VT_ERR_INVALID, "%s: %s%d has pixel stride %d (C=%d, multiples of %d)", who, what, k, ld, C,
               epc);
    return VT_OK;
}

int check_geometry(const char* who, int n, const int* codes, int B, int H, int W, int C, int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(n == 2 || n == 3, VT_ERR_UNSUPPORTED, "%s: n=%d inputs (2 or 3)", who, n);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C > 0 && C % epc == 0, VT_ERR_UNSUPPORTED, "%s: C=%d must be a positive multiple of %d", who, C, epc);
    VT_REQUIRE(B > 0 && H > 0 && W > 0, VT_ERR_INVALID, "%s: B=%d H=%d W=%d", who, B, H, W);
    for (int k = 0; k < n; ++k) {
        VT_REQUIRE(codes[k] >= 0 && codes[k] <= 2, VT_ERR_UNSUPPORTED, "%s: resample code %d of input %d (0, 1 or 2)", who, codes[k],
                   k);
        VT_REQUIRE(codes[k] != 1 || (H % 2 == 0 && W % 2 == 0), VT_ERR_INVALID,
                   "%s: input %d is upsampled x2 onto an odd %d x %d grid", who, k, H, W);
    }
    return VT_OK;
}

unsigned grid_for(long items) {
    long b = (items + kT - 1) / kT;
    const long cap = (long)vt_device_cus() * 8;
    if (b > cap) b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}

#define VT_WFUSE_DISPATCH(dtype, n, ...)                    \
    do {                                                    \
        if ((dtype) == VT_BF16) {                           \
            typedef bf16_t T;                               \
            if ((n) == 2) { constexpr int NI = 2; __VA_ARGS__; } \
            else { constexpr int NI = 3; __VA_ARGS__; }     \
        } else {                                            \
            typedef float T;                                \
            if ((n) == 2) { constexpr int NI = 2; __VA_ARGS__; } \
            else { constexpr int NI = 3; __VA_ARGS__; }     \
        }                                                   \
    } while (0)

}  // namespace

extern "C" {

int vt_wfuse_fwd(int32_t n, const void* x0, int32_t ld0, int32_t code0, const void* x1, int32_t ld1, int32_t code1,
                 const void* x2, int32_t ld2, int32_t code2, const float* weights, float eps, void* out, int32_t ldo, int32_t B,
                 int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_wfuse_fwd";
    FuseIn in = {{x0, x1, x2}, {ld0, ld1, ld2}, {code0, code1, code2}};
    VT_TRY(check_geometry(who, n, in.code, B, H, W, C, dtype));
    VT_REQUIRE(eps >= 0.f, VT_ERR_INVALID, "%s: eps=%g", who, (double)eps);
    VT_REQUIRE(weights, VT_ERR_INVALID, "%s: weights is null", who);
    VT_TRY(check_map(who, "out", 0, out, ldo, C, dtype));
    for (int k = 0; k < n; ++k) {
        VT_TRY(check_map(who, "x", k, in.x[k], in.ld[k], C, dtype));
        VT_REQUIRE(in.x[k] != out, VT_ERR_INVALID, "%s: out aliases x%d (the inputs are needed in backward)", who, k);
    }
    const int cpr = C / vt_epc(dtype);
    const long items = (long)B * H * W * cpr;
    VT_WFUSE_DISPATCH(dtype, n,
                      hipLaunchKernelGGL((wfuse_fwd_kernel<T, NI>), dim3(grid_for(items)), dim3(kT), 0, (hipStream_t)stream, in,
                                         weights, eps, (T*)out, ldo, B, H, W, cpr));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_wfuse_bwd(int32_t n, const void* g, int32_t ldg, const void* x0, int32_t ld0, int32_t code0, const void* x1, int32_t ld1,
                 int32_t code1, const void* x2, int32_t ld2, int32_t code2, const float* weights, float eps, void* dx0,
                 int32_t lddx0, int32_t acc0, void* dx1, int32_t lddx1, int32_t acc1, void* dx2, int32_t lddx2, int32_t acc2,
                 float* sums, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_wfuse_bwd";
    FuseIn in = {{x0, x1, x2}, {ld0, ld1, ld2}, {code0, code1, code2}};
    FuseGrad gr = {{dx0, dx1, dx2}, {lddx0, lddx1, lddx2}, {acc0, acc1, acc2}};
    VT_TRY(check_geometry(who, n, in.code, B, H, W, C, dtype));
    VT_REQUIRE(eps >= 0.f, VT_ERR_INVALID, "%s: eps=%g", who, (double)eps);
    VT_REQUIRE(weights && sums && vt_aligned16(sums), VT_ERR_INVALID, "%s: weights / sums null or misaligned", who);
    VT_TRY(check_map(who, "g", 0, g, ldg, C, dtype));
    for (int k = 0; k < n; ++k) {
        VT_TRY(check_map(who, "x", k, in.x[k], in.ld[k], C, dtype));
        if (!gr.dx[k]) continue;  // this input needs no gradient
        VT_TRY(check_map(who, "dx", k, gr.dx[k], gr.ld[k], C, dtype));
        VT_REQUIRE(gr.dx[k] != g, VT_ERR_INVALID, "%s: dx%d aliases g", who, k);
        for (int m = 0; m < k; ++m)
            VT_REQUIRE(gr.dx[m] != gr.dx[k], VT_ERR_INVALID, "%s: dx%d aliases dx%d", who, k, m);
    }
    if (n < kMaxIn) gr.dx[2] = nullptr;
    const int cpr = C / vt_epc(dtype);
    const long items = (long)B * ((H + 1) / 2) * ((W + 1) / 2) * cpr;
    VT_WFUSE_DISPATCH(dtype, n,
                      hipLaunchKernelGGL((wfuse_bwd_kernel<T, NI>), dim3(grid_for(items)), dim3(kT), 0, (hipStream_t)stream, in, gr,
                                         (const T*)g, ldg, weights, eps, sums, B, H, W, cpr));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_wfuse_finalize(const float* sums, const float* weights, float eps, int32_t n, float* dweights, void* stream) {
    const char* who = "vt_wfuse_finalize";
    VT_REQUIRE(n == 2 || n == 3, VT_ERR_UNSUPPORTED, "%s: n=%d inputs (2 or 3)", who, n);
    VT_REQUIRE(sums && weights && dweights && eps >= 0.f, VT_ERR_INVALID, "%s: null operand or eps=%g", who, (double)eps);
    hipLaunchKernelGGL(wfuse_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, weights, eps, n, dweights);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // extern "C"
