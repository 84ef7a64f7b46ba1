// vt_layernorm.hip -- LayerNorm over the channel axis of an NHWC map and LayerScale + residual, forward and backward
// (ConvNeXt: reference backbones/convnext.py:48,53,58 -- nn.LayerNorm(d_model) on (B, H, W, C), `x + gamma * layers(x)`).
//
// Memory-bound streaming kernels.  One mapping for all of them: a pixel row of CPR = C / EPC 16-byte chunks is owned by a
// GROUP of g lanes of one wave, g = the power of two >= CPR capped at 64 (C = 40 bf16: 8 lanes per row, 8 rows per wave;
// C = 2816 bf16: 64 lanes, 6 chunks per lane); lane j of a group holds the chunks j, j + g, ... of its row in registers
// (NCH of them, a template parameter), so
//   * the statistics of a row are a two-pass computation over registers (mean, then sum (u - mean)^2: what torch computes)
//     and the reduction over C is an in-wave xor-shuffle fold of width g -- no LDS, no barrier on the forward path;
//   * a lane keeps the SAME channel chunks for every row it visits (grid-stride loop over rows), so the per-channel sums
//     of the backward kernels (d gamma, d beta, d pre_bias) are per-lane registers across the loop; at the end they fold
//     across the row groups of a wave (shuffles), across the waves of the workgroup (LDS) and leave as ONE fixed-point
//     atomic per channel and workgroup into a replicated channel-sums buffer (vt_common.h: vt_stat_add) -- integer
//     atomics, so these parameter gradients are bit-identical from run to run like the BatchNorm ones.
#include "vt_common.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;

__device__ __forceinline__ float group_sum(float v, int g) {
    for (int o = 1; o < g; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int EPC>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, int c0, float (&v)[EPC]) {
#pragma unroll
    for (int e = 0; e < EPC; e += 4) {
        const float4 q = *(const float4*)(p + c0 + e);
        v[e] = q.x, v[e + 1] = q.y, v[e + 2] = q.z, v[e + 3] = q.w;
    }
}

// per-channel vectors stay in registers for short rows; long rows (NCH > 2) re-read them through the cache
template <int NCH, int EPC>
struct ChanVec {
    static constexpr bool KEEP = NCH <= 2;
    float keep[KEEP ? NCH : 1][EPC];
    const float* p;
    __device__ __forceinline__ void init(const float* ptr, int j, int g, int cpr) {
        p = ptr;
        if (KEEP && ptr) {
#pragma unroll
            for (int i = 0; i < NCH; ++i)
                if (j + i * g < cpr) load_f32<EPC>(ptr, (j + i * g) * EPC, keep[i]);
        }
    }
    __device__ __forceinline__ void get(int i, int c0, float (&v)[EPC]) const {
        if (KEEP) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) v[e] = keep[i][e];
        } else {
            load_f32<EPC>(p, c0, v);
        }
    }
};

// u = x (+ pre_bias) of one row into registers, its mean and 1 / sqrt(var + eps); u leaves as the deviations u - mean
// (forward) or as xhat (XHAT: backward)
template <typename T, int NCH, bool XHAT>
__device__ __forceinline__ void row_stats(const T* __restrict__ xrow, bool valid, int j, int g, int cpr,
                                          const ChanVec<NCH, VecIO<T>::EPC>& pb, float fC, float eps,
                                          float (&u)[NCH][VecIO<T>::EPC], float& mean, float& rstd) {
    constexpr int EPC = VecIO<T>::EPC;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ci = j + i * g;
        if (valid && ci < cpr) {
            VecIO<T>::unpack(*(const uint4*)(xrow + ci * EPC), u[i]);
            if (pb.p) {
                float b[EPC];
                pb.get(i, ci * EPC, b);
#pragma unroll
                for (int e = 0; e < EPC; ++e) u[i][e] += b[e];
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) s += u[i][e];
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] = 0.f;
        }
    }
    mean = group_sum(s, g) / fC;  // (a division: a constant row has exactly zero variance)
    if (XHAT) {
        // Backward: the deviations u - mean feed the per-channel sums sum_m dy * xhat, where a row count of two (the head)
        // leaves no averaging: the f32 rounding of the mean itself (half an ulp of the DATA scale) is then a visible
        // fraction of a small deviation.  The deviations are taken against the mean in double (one f64 add per element and
        // a fold of doubles per row) and are then exact to f32 rounding of the deviation itself.
        double sd = 0.0;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) sd += (double)u[i][e];
        for (int o = 1; o < g; o <<= 1) sd += __shfl_xor(sd, o, 64);
        const double md = sd / (double)fC;
        mean = (float)md;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] = (float)((double)u[i][e] - md);
    } else {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] -= mean;
    }
    float q = 0.f;  // (u holds the deviations from here on)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        if (j + i * g < cpr) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) q = fmaf(u[i][e], u[i][e], q);
        }
    }
    rstd = 1.0f / sqrtf(group_sum(q, g) / fC + eps);
    if (XHAT) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] *= rstd;
    }
}

template <typename T, int NCH>
__global__ void __launch_bounds__(kT) ln_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ pre_bias,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    T* __restrict__ y, int ldy, long M, int C, float eps, int g) {
    constexpr int EPC = VecIO<T>::EPC;
    const int cpr = C / EPC, rpb = kT / g;
    const int j = threadIdx.x & (g - 1), r = threadIdx.x / g;
    const float fC = (float)C;
    ChanVec<NCH, EPC> gm, bt, pb;
    gm.init(gamma, j, g, cpr), bt.init(beta, j, g, cpr), pb.init(pre_bias, j, g, cpr);
    for (long base = (long)blockIdx.x * rpb; base < M; base += (long)gridDim.x * rpb) {
        const long row = base + r;
        const bool valid = row < M;
        float u[NCH][EPC], mean, rstd;
        row_stats<T, NCH, false>(x + row * ldx, valid, j, g, cpr, pb, fC, eps, u, mean, rstd);
        if (valid) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int ci = j + i * g;
                if (ci < cpr) {
                    float gv[EPC], bv[EPC], o[EPC];
                    gm.get(i, ci * EPC, gv), bt.get(i, ci * EPC, bv);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) o[e] = fmaf(u[i][e] * rstd, gv[e], bv[e]);
                    *(uint4*)(y + row * ldy + ci * EPC) = VecIO<T>::pack(o);
                }
            }
        }
    }
}

// per-lane channel sums -> one fixed-point atomic per channel and workgroup: row groups of a wave (shuffles), waves (LDS)
template <int NCH, int EPC>
__device__ __forceinline__ void flush_sums(float (&acc)[NCH][EPC], float* sums, int kind, int kinds, int C, int j, int g,
                                           int cpr, float (*red)[64][8]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rep = blockIdx.x % kStatReplicas;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        for (int off = g; off < 64; off <<= 1) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[i][e] += __shfl_xor(acc[i][e], off, 64);
        }
        if (lane < g) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) red[wave][lane][e] = acc[i][e];
        }
        __syncthreads();
        // chunk column i covers the g * EPC consecutive channels from i * g * EPC: consecutive threads take consecutive
        // channels, so a wave's atomics land on one contiguous segment of the buffer
        const int span = g * EPC;
        for (int t = threadIdx.x; t < span; t += kT) {
            const int c = i * span + t;
            if (c < C) {
                float v = red[0][t / EPC][t % EPC];
#pragma unroll
                for (int w = 1; w < kWaves; ++w) v += red[w][t / EPC][t % EPC];
                vt_stat_add(sums, ((long)rep * kinds + kind) * C + c, v);
            }
        }
        __syncthreads();
    }
}

template <typename T, int NCH>
__global__ void __launch_bounds__(kT) ln_bwd_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ x, int ldx,
                                                    const float* __restrict__ pre_bias, const float* __restrict__ gamma,
                                                    T* dx, int lddx, const T* res, int ldr, float* sums, long M, int C,
                                                    float eps, int g) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float red[kWaves][64][8];
    const int cpr = C / EPC, rpb = kT / g;
    const int j = threadIdx.x & (g - 1), r = threadIdx.x / g;
    const float fC = (float)C;
    ChanVec<NCH, EPC> gm, pb;
    gm.init(gamma, j, g, cpr), pb.init(pre_bias, j, g, cpr);
    float sg[NCH][EPC], sb[NCH][EPC], sx[NCH][EPC];
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) sg[i][e] = sb[i][e] = sx[i][e] = 0.f;
    for (long base = (long)blockIdx.x * rpb; base < M; base += (long)gridDim.x * rpb) {
        const long row = base + r;
        const bool valid = row < M;
        float xh[NCH][EPC], gv[NCH][EPC], mean, rstd;
        row_stats<T, NCH, true>(x + row * ldx, valid, j, g, cpr, pb, fC, eps, xh, mean, rstd);
        float a = 0.f, b = 0.f;  // sum_c g, sum_c g * xhat
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ci = j + i * g;
            if (valid && ci < cpr) {
                float w[EPC];
                VecIO<T>::unpack(*(const uint4*)(dy + row * lddy + ci * EPC), gv[i]);
                gm.get(i, ci * EPC, w);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    sg[i][e] = fmaf(gv[i][e], xh[i][e], sg[i][e]);
                    sb[i][e] += gv[i][e];
                    gv[i][e] *= w[e];
                    a += gv[i][e];
                    b = fmaf(gv[i][e], xh[i][e], b);
                }
            } else {
#pragma unroll
                for (int e = 0; e < EPC; ++e) gv[i][e] = 0.f;
            }
        }
        a = group_sum(a, g) / fC;
        b = group_sum(b, g) / fC;
        if (valid) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int ci = j + i * g;
                if (ci < cpr) {
                    float o[EPC];
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        o[e] = rstd * (gv[i][e] - a - xh[i][e] * b);
                        sx[i][e] += o[e];
                    }
                    if (res) {
                        // (the gradient is rounded to the storage type first, as a separate launch + add would)
                        float rv[EPC], sv[EPC];
                        VecIO<T>::unpack(VecIO<T>::pack(o), sv);
                        VecIO<T>::unpack(*(const uint4*)(res + row * ldr + ci * EPC), rv);
#pragma unroll
                        for (int e = 0; e < EPC; ++e) o[e] = sv[e] + rv[e];
                    }
                    *(uint4*)(dx + row * lddx + ci * EPC) = VecIO<T>::pack(o);
                }
            }
        }
    }
    flush_sums<NCH, EPC>(sg, sums, 0, 3, C, j, g, cpr, red);
    flush_sums<NCH, EPC>(sb, sums, 1, 3, C, j, g, cpr, red);
    if (pre_bias) flush_sums<NCH, EPC>(sx, sums, 2, 3, C, j, g, cpr, red);
}

template <typename T>
__global__ void __launch_bounds__(kT) scale_res_fwd_kernel(const T* __restrict__ t, int ldt, const float* __restrict__ gamma,
                                                           const T* __restrict__ res, int ldr, T* __restrict__ y, int ldy,
                                                           long M, int C, int g) {
    constexpr int EPC = VecIO<T>::EPC;
    const int cpr = C / EPC, rpb = kT / g;
    const int j = threadIdx.x & (g - 1), r = threadIdx.x / g;
    const bool one = cpr <= g;  // one chunk per lane: its gamma stays in registers
    float gm[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) gm[e] = 1.f;
    if (gamma && one && j < cpr) load_f32<EPC>(gamma, j * EPC, gm);
    for (long row = (long)blockIdx.x * rpb + r; row < M; row += (long)gridDim.x * rpb) {
        for (int ci = j; ci < cpr; ci += g) {
            float tv[EPC], rv[EPC];
            VecIO<T>::unpack(*(const uint4*)(t + row * ldt + ci * EPC), tv);
            VecIO<T>::unpack(*(const uint4*)(res + row * ldr + ci * EPC), rv);
            if (gamma && !one) load_f32<EPC>(gamma, ci * EPC, gm);
#pragma unroll
            for (int e = 0; e < EPC; ++e) tv[e] = fmaf(tv[e], gm[e], rv[e]);
            *(uint4*)(y + row * ldy + ci * EPC) = VecIO<T>::pack(tv);
        }
    }
}

template <typename T, int NCH>
__global__ void __launch_bounds__(kT) scale_res_bwd_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ t, int ldt,
                                                           const float* __restrict__ gamma, T* __restrict__ dt, int lddt,
                                                           float* sums, long M, int C, int g) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float red[kWaves][64][8];
    const int cpr = C / EPC, rpb = kT / g;
    const int j = threadIdx.x & (g - 1), r = threadIdx.x / g;
    ChanVec<NCH, EPC> gm;
    gm.init(gamma, j, g, cpr);
    float acc[NCH][EPC];
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[i][e] = 0.f;
    for (long row = (long)blockIdx.x * rpb + r; row < M; row += (long)gridDim.x * rpb) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ci = j + i * g;
            if (ci < cpr) {
                float gv[EPC], tv[EPC], w[EPC];
                VecIO<T>::unpack(*(const uint4*)(dy + row * lddy + ci * EPC), gv);
                VecIO<T>::unpack(*(const uint4*)(t + row * ldt + ci * EPC), tv);
                gm.get(i, ci * EPC, w);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    acc[i][e] = fmaf(gv[e], tv[e], acc[i][e]);
                    gv[e] *= w[e];
                }
                *(uint4*)(dt + row * lddt + ci * EPC) = VecIO<T>::pack(gv);
            }
        }
    }
    flush_sums<NCH, EPC>(acc, sums, 0, 1, C, j, g, cpr, red);
}

__global__ void __launch_bounds__(kT) channel_sums_kernel(const float* __restrict__ sums, int rows, int C, float* d0, float* d1,
                                                          float* d2) {
    const int idx = blockIdx.x * kT + threadIdx.x;
    if (idx >= rows * C) return;
    const int k = idx / C, c = idx - k * C;
    float* dst = k == 0 ? d0 : (k == 1 ? d1 : d2);
    if (!dst) return;
    dst[c] += (float)vt_stat_sum(sums, idx, (long)rows * C);
}

struct Map {
    int g, nch;
};

int make_map(const char* who, int C, int dtype, Map& m) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C > 0 && C % epc == 0, VT_ERR_UNSUPPORTED, "%s: C=%d must be a positive multiple of %d", who, C, epc);
    VT_REQUIRE(C <= 3072, VT_ERR_UNSUPPORTED, "%s: C=%d exceeds 3072 (a row is held in registers)", who, C);
    const int cpr = C / epc;
    int g = 1;
    while (g < cpr && g < 64) g <<= 1;
    const int need = (cpr + g - 1) / g;
    static const int kSteps[] = {1, 2, 4, 6, 8, 12};
    m.g = g, m.nch = 0;
    for (int s : kSteps)
        if (s >= need) {
            m.nch = s;
            break;
        }
    VT_REQUIRE(m.nch > 0, VT_ERR_UNSUPPORTED, "%s: C=%d", who, C);
    return VT_OK;
}

int check_rows(const char* who, const char* what, const void* p, int ld, int C, int dtype) {
    const int epc = vt_epc(dtype);
    VT_REQUIRE(p && vt_aligned16(p), VT_ERR_INVALID, "%s: %s is null or misaligned", who, what);
    VT_REQUIRE(ld >= C && ld % epc == 0, VT_ERR_INVALID, "%s: %s has pixel stride %d (C=%d, multiples of %d)", who, what, ld, C,
               epc);
    return VT_OK;
}

// `sweeps`: at least this many rows per row slot of a workgroup (the backward kernels: every workgroup ends with one atomic
// per channel and sum, so a workgroup that visits four rows pays 3 C atomics for 12 C elements of data -- measured at
// C = 768, M = 3136 with one sweep per workgroup: 108 us for 14 MB)
unsigned grid_for(long M, int g, int per_cu, int sweeps = 1) {
    const long rpb = (long)(kT / g) * sweeps;
    long b = (M + rpb - 1) / rpb;
    const long cap = (long)vt_device_cus() * per_cu;
    if (b > cap) b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}

// (bf16 rows hold 8 elements per chunk: NCH <= 6 covers C <= 3072; f32 rows 4: NCH <= 12)
#define VT_LN_DISPATCH(dtype, nch, ...)                 \
    do {                                                \
        if ((dtype) == VT_BF16) {                       \
            typedef bf16_t T;                           \
            switch (nch) {                              \
                case 1: { constexpr int NCH = 1; __VA_ARGS__; } break; \
                case 2: { constexpr int NCH = 2; __VA_ARGS__; } break; \
                case 4: { constexpr int NCH = 4; __VA_ARGS__; } break; \
                default: { constexpr int NCH = 6; __VA_ARGS__; } break; \
            }                                           \
        } else {                                        \
            typedef float T;                            \
            switch (nch) {                              \
                case 1: { constexpr int NCH = 1; __VA_ARGS__; } break; \
                case 2: { constexpr int NCH = 2; __VA_ARGS__; } break; \
                case 4: { constexpr int NCH = 4; __VA_ARGS__; } break; \
                case 6: { constexpr int NCH = 6; __VA_ARGS__; } break; \
                case 8: { constexpr int NCH = 8; __VA_ARGS__; } break; \
                default: { constexpr int NCH = 12; __VA_ARGS__; } break; \
            }                                           \
        }                                               \
    } while (0)

}  // namespace

extern "C" {

int vt_layernorm_fwd(const void* x, int32_t ldx, const float* pre_bias, const float* gamma, const float* beta, void* y,
                     int32_t ldy, int64_t M, int32_t C, float eps, int32_t dtype, void* stream) {
    const char* who = "vt_layernorm_fwd";
    Map m;
    VT_TRY(make_map(who, C, dtype, m));
    VT_REQUIRE(M > 0 && eps >= 0.f, VT_ERR_INVALID, "%s: M=%ld eps=%g", who, (long)M, (double)eps);
    VT_TRY(check_rows(who, "x", x, ldx, C, dtype));
    VT_TRY(check_rows(who, "y", y, ldy, C, dtype));
    VT_REQUIRE(gamma && beta && vt_aligned16(gamma) && vt_aligned16(beta) && vt_aligned16(pre_bias), VT_ERR_INVALID,
               "%s: gamma / beta null, or a per-channel vector misaligned", who);
    VT_LN_DISPATCH(dtype, m.nch,
                   hipLaunchKernelGGL((ln_fwd_kernel<T, NCH>), dim3(grid_for(M, m.g, 8)), dim3(kT), 0, (hipStream_t)stream,
                                      (const T*)x, ldx, pre_bias, gamma, beta, (T*)y, ldy, (long)M, C, eps, m.g));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_layernorm_bwd(const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* pre_bias, const float* gamma,
                     void* dx, int32_t lddx, const void* residual, int32_t ldr, float* sums, int64_t M, int32_t C, float eps,
                     int32_t dtype, void* stream) {
    const char* who = "vt_layernorm_bwd";
    Map m;
    VT_TRY(make_map(who, C, dtype, m));
    VT_REQUIRE(M > 0 && eps >= 0.f, VT_ERR_INVALID, "%s: M=%ld eps=%g", who, (long)M, (double)eps);
    VT_TRY(check_rows(who, "dy", dy, lddy, C, dtype));
    VT_TRY(check_rows(who, "x", x, ldx, C, dtype));
    VT_TRY(check_rows(who, "dx", dx, lddx, C, dtype));
    if (residual) VT_TRY(check_rows(who, "residual", residual, ldr, C, dtype));
    VT_REQUIRE(gamma && sums && vt_aligned16(gamma) && vt_aligned16(pre_bias) && vt_aligned16(sums), VT_ERR_INVALID,
               "%s: gamma / sums null, or a per-channel vector misaligned", who);
    VT_LN_DISPATCH(dtype, m.nch,
                   hipLaunchKernelGGL((ln_bwd_kernel<T, NCH>), dim3(grid_for(M, m.g, 4, 4)), dim3(kT), 0, (hipStream_t)stream,
                                      (const T*)dy, lddy, (const T*)x, ldx, pre_bias, gamma, (T*)dx, lddx, (const T*)residual,
                                      ldr, sums, (long)M, C, eps, m.g));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_scale_residual_fwd(const void* t, int32_t ldt, const float* gamma, const void* residual, int32_t ldr, void* y,
                          int32_t ldy, int64_t M, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_scale_residual_fwd";
    Map m;
    VT_TRY(make_map(who, C, dtype, m));
    VT_REQUIRE(M > 0, VT_ERR_INVALID, "%s: M=%ld", who, (long)M);
    VT_TRY(check_rows(who, "t", t, ldt, C, dtype));
    VT_TRY(check_rows(who, "residual", residual, ldr, C, dtype));
    VT_TRY(check_rows(who, "y", y, ldy, C, dtype));
    VT_REQUIRE(vt_aligned16(gamma), VT_ERR_INVALID, "%s: gamma misaligned", who);
    if (dtype == VT_BF16) {
        hipLaunchKernelGGL(scale_res_fwd_kernel<bf16_t>, dim3(grid_for(M, m.g, 8)), dim3(kT), 0, (hipStream_t)stream,
                           (const bf16_t*)t, ldt, gamma, (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, (long)M, C, m.g);
    } else {
        hipLaunchKernelGGL(scale_res_fwd_kernel<float>, dim3(grid_for(M, m.g, 8)), dim3(kT), 0, (hipStream_t)stream,
                           (const float*)t, ldt, gamma, (const float*)residual, ldr, (float*)y, ldy, (long)M, C, m.g);
    }
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_scale_residual_bwd(const void* dy, int32_t lddy, const void* t, int32_t ldt, const float* gamma, void* dt,
                          int32_t lddt, float* sums, int64_t M, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_scale_residual_bwd";
    Map m;
    VT_TRY(make_map(who, C, dtype, m));
    VT_REQUIRE(M > 0, VT_ERR_INVALID, "%s: M=%ld", who, (long)M);
    VT_TRY(check_rows(who, "dy", dy, lddy, C, dtype));
    VT_TRY(check_rows(who, "t", t, ldt, C, dtype));
    VT_TRY(check_rows(who, "dt", dt, lddt, C, dtype));
    VT_REQUIRE(gamma && sums && vt_aligned16(gamma) && vt_aligned16(sums), VT_ERR_INVALID,
               "%s: gamma / sums null or misaligned", who);
    VT_LN_DISPATCH(dtype, m.nch,
                   hipLaunchKernelGGL((scale_res_bwd_kernel<T, NCH>), dim3(grid_for(M, m.g, 4, 4)), dim3(kT), 0,
                                      (hipStream_t)stream, (const T*)dy, lddy, (const T*)t, ldt, gamma, (T*)dt, lddt, sums,
                                      (long)M, C, m.g));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_channel_sums_to_f32(const float* sums, int32_t rows, int32_t C, float* dst0, float* dst1, float* dst2, void* stream) {
    VT_REQUIRE(sums && rows >= 1 && rows <= 3 && C > 0, VT_ERR_INVALID, "vt_channel_sums_to_f32: bad argument");
    hipLaunchKernelGGL(channel_sums_kernel, dim3((rows * C + kT - 1) / kT), dim3(kT), 0, (hipStream_t)stream, sums, rows, C,
                       dst0, dst1, dst2);
    VT_CHECK_LAUNCH("vt_channel_sums_to_f32");
    return VT_OK;
}

}  // extern "C"
