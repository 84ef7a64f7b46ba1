// vt_prefix_tokens.hip -- the token bookkeeping of DeiT (reference backbones/deit.py:37-41): P learned prefix rows in front of
// the position-embedded patch rows, and the pooled head norm(out[:, :P]).mean(1), forward and backward, general in P (1..4).
//
// Memory-bound streaming kernels; every global access is one 16-byte chunk per lane.
//   tokens:  a thread owns ONE (token row, chunk) pair -- one division per thread, none per element -- and walks the images:
//            forward keeps its pe / prefix chunk in registers across the images (the images are dealt to blockIdx.y);
//            backward walks ALL images in order with four loads in flight, copies the patch rows to d(embed) on the way
//            and adds its f32 sum to d(pe) / d(prefix) with a plain read-modify-write: one owner, a fixed order.
//   pool:    a wave owns the P prefix rows of one image, lane l the chunks l, l + 64, ... of a row in registers (NCH of
//            them, a template parameter), so the statistics of a row are a two-pass computation over registers with a wave
//            fold, as in vt_layernorm.hip; four images share a workgroup.  The backward grid is (image group, row slab):
//            slab 0 does the LayerNorm backward of the prefix rows, every slab writes its share of the zero rows, and the
//            per-channel sums of the four waves fold through LDS into ONE fixed-point atomic per channel and workgroup
//            (vt_common.h: vt_stat_add) -- integer atomics, so d gamma / d beta are bit-identical from run to run.
#include "vt_common.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kMaxPrefix = 4;
constexpr int kSlabRows = 16;  // token rows of one backward workgroup (the zero fill)

struct PrefixPtrs {
    float* p[kMaxPrefix];
};

template <int EPC>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, float (&v)[EPC]) {
#pragma unroll
    for (int e = 0; e < EPC; e += 4) {
        const float4 q = *(const float4*)(p + e);
        v[e] = q.x, v[e + 1] = q.y, v[e + 2] = q.z, v[e + 3] = q.w;
    }
}

template <int EPC>
__device__ __forceinline__ void add_f32(float* __restrict__ p, const float (&v)[EPC]) {
#pragma unroll
    for (int e = 0; e < EPC; e += 4) {
        float4 q = *(float4*)(p + e);
        q.x += v[e], q.y += v[e + 1], q.z += v[e + 2], q.w += v[e + 3];
        *(float4*)(p + e) = q;
    }
}

// out[b][p] = prefix[p], out[b][P + t] = embed[b][t] + pe[t]
template <typename T>
__global__ void __launch_bounds__(kT) prefix_tokens_fwd_kernel(const T* __restrict__ embed, int lde, const float* __restrict__ pe,
                                                               PrefixPtrs prefix, int P, T* __restrict__ out, int ldo, int B,
                                                               int Tn, int C) {
    constexpr int EPC = VecIO<T>::EPC;
    const int cpr = C / EPC, L = P + Tn;
    const long idx = (long)blockIdx.x * kT + threadIdx.x;
    if (idx >= (long)L * cpr) return;
    const int t = (int)(idx / cpr), c0 = ((int)(idx - (long)t * cpr)) * EPC;
    float own[EPC];  // the prefix row's chunk, or pe's
    if (t < P) {
        load_f32<EPC>(prefix.p[t] + c0, own);
        const uint4 v = VecIO<T>::pack(own);
        for (int b = blockIdx.y; b < B; b += gridDim.y) *(uint4*)(out + ((long)b * L + t) * ldo + c0) = v;
        return;
    }
    load_f32<EPC>(pe + (long)(t - P) * C + c0, own);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        float u[EPC];
        VecIO<T>::unpack(*(const uint4*)(embed + ((long)b * Tn + (t - P)) * lde + c0), u);
#pragma unroll
        for (int e = 0; e < EPC; ++e) u[e] += own[e];
        *(uint4*)(out + ((long)b * L + t) * ldo + c0) = VecIO<T>::pack(u);
    }
}

// dembed[b][t] = dout[b][P + t]; dpe[t] += sum_b dout[b][P + t]; dprefix[p] += sum_b dout[b][p]
template <typename T>
__global__ void __launch_bounds__(kT) prefix_tokens_bwd_kernel(const T* __restrict__ dout, int lddo, T* __restrict__ dembed, int lde,
                                                               float* __restrict__ dpe, PrefixPtrs dprefix, int P, int B, int Tn,
                                                               int C) {
    constexpr int EPC = VecIO<T>::EPC;
    constexpr int NB = 4;  // images in flight
    const int cpr = C / EPC, L = P + Tn;
    const long idx = (long)blockIdx.x * kT + threadIdx.x;
    if (idx >= (long)L * cpr) return;
    const int t = (int)(idx / cpr), c0 = ((int)(idx - (long)t * cpr)) * EPC;
    float* sum_dst = t < P ? dprefix.p[t] : dpe;
    T* copy_dst = t < P ? nullptr : dembed;
    if (!sum_dst && !copy_dst) return;
    if (sum_dst) sum_dst += (t < P ? 0L : (long)(t - P) * C) + c0;
    if (copy_dst) copy_dst += (long)(t - P) * lde + c0;
    const T* src = dout + (long)t * lddo + c0;
    const long sstep = (long)L * lddo, dstep = (long)Tn * lde;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    int b = 0;
    for (; b + NB <= B; b += NB) {
        uint4 v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = *(const uint4*)(src + (b + k) * sstep);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            if (copy_dst) *(uint4*)(copy_dst + (b + k) * dstep) = v[k];
            float u[EPC];
            VecIO<T>::unpack(v[k], u);
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] += u[e];
        }
    }
    for (; b < B; ++b) {
        const uint4 v = *(const uint4*)(src + b * sstep);
        if (copy_dst) *(uint4*)(copy_dst + b * dstep) = v;
        float u[EPC];
        VecIO<T>::unpack(v, u);
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] += u[e];
    }
    if (sum_dst) add_f32<EPC>(sum_dst, acc);
}

// one row of x into registers (zeros beyond the row), its mean and 1 / sqrt(var + eps); u leaves as the deviations u - mean
// (forward) or as xhat with the deviations taken against the mean in double (XHAT: backward; the reason is the one of
// vt_layernorm.hip's row_stats -- with a handful of rows nothing averages the rounding of the mean out of the channel sums)
template <typename T, int NCH, bool XHAT>
__device__ __forceinline__ void wave_row_stats(const T* __restrict__ xrow, bool valid, int lane, int cpr, float fC, float eps,
                                               float (&u)[NCH][VecIO<T>::EPC], float& rstd) {
    constexpr int EPC = VecIO<T>::EPC;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ci = lane + i * 64;
        if (valid && ci < cpr) {
            VecIO<T>::unpack(*(const uint4*)(xrow + ci * EPC), u[i]);
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] = 0.f;
        }
    }
    if (XHAT) {
        double sd = 0.0;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) sd += (double)u[i][e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
        const double md = sd / (double)fC;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] = (float)((double)u[i][e] - md);
    } else {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) s += u[i][e];
        const float mean = wave_sum(s) / fC;  // (a division: a constant row has exactly zero variance)
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] -= mean;
    }
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        if (lane + i * 64 < cpr) {  // (the padding chunks hold -mean, not a deviation)
#pragma unroll
            for (int e = 0; e < EPC; ++e) q = fmaf(u[i][e], u[i][e], q);
        }
    }
    rstd = 1.0f / sqrtf(wave_sum(q) / fC + eps);
    if (XHAT) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int e = 0; e < EPC; ++e) u[i][e] *= rstd;
    }
}

// y[b] = (1 / P) sum_p LayerNorm(x[b][p])
template <typename T, int NCH>
__global__ void __launch_bounds__(kT) prefix_pool_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, T* __restrict__ y, int ldy, int B,
                                                             int L, int P, int C, float eps) {
    constexpr int EPC = VecIO<T>::EPC;
    const int cpr = C / EPC, lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (b >= B) return;  // (wave-uniform; the kernel has no barrier)
    const float fC = (float)C, invP = 1.0f / (float)P;
    float acc[NCH][EPC];
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[i][e] = 0.f;
    for (int p = 0; p < P; ++p) {
        float u[NCH][EPC], rstd;
        wave_row_stats<T, NCH, false>(x + ((long)b * L + p) * ldx, true, lane, cpr, fC, eps, u, rstd);
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ci = lane + i * 64;
            if (ci < cpr) {
                float gv[EPC], bv[EPC];
                load_f32<EPC>(gamma + ci * EPC, gv), load_f32<EPC>(beta + ci * EPC, bv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[i][e] += fmaf(u[i][e] * rstd, gv[e], bv[e]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ci = lane + i * 64;
        if (ci < cpr) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[i][e] *= invP;
            *(uint4*)(y + (long)b * ldy + ci * EPC) = VecIO<T>::pack(acc[i]);
        }
    }
}

// the four waves' per-lane channel sums -> one fixed-point atomic per channel and workgroup
template <int NCH, int EPC>
__device__ __forceinline__ void flush_wave_sums(float (&acc)[NCH][EPC], float* sums, int kind, int C, unsigned rep,
                                                float (*red)[64][8]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[wave][lane][e] = acc[i][e];
        __syncthreads();
        // chunk column i covers the 64 * EPC consecutive channels from i * 64 * EPC: consecutive threads take consecutive
        // channels, so a wave's atomics land on one contiguous segment of the buffer
        for (int t = threadIdx.x; t < 64 * EPC; t += kT) {
            const int c = i * 64 * EPC + t;
            if (c < C) {
                float v = red[0][t / EPC][t % EPC];
#pragma unroll
                for (int w = 1; w < kWaves; ++w) v += red[w][t / EPC][t % EPC];
                vt_stat_add(sums, ((long)rep * 2 + kind) * C + c, v);
            }
        }
        __syncthreads();
    }
}

// grid (row slabs, image groups of kWaves): slab 0 owns the LayerNorm backward of the prefix rows of its images (wave w:
// image group * kWaves + w) and the channel sums; every slab zero-fills its rows >= P unless `accumulate`
template <typename T, int NCH>
__global__ void __launch_bounds__(kT) prefix_pool_bwd_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ x, int ldx,
                                                             const float* __restrict__ gamma, T* dx, int lddx, int accumulate,
                                                             float* sums, int B, int L, int P, int C, float eps) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float red[kWaves][64][8];
    const int cpr = C / EPC, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.y * kWaves;
    if (blockIdx.x == 0) {
        const int b = b0 + wave;
        const bool valid = b < B;
        const float fC = (float)C, invP = 1.0f / (float)P;
        float g[NCH][EPC], sg[NCH][EPC];  // dy[b] (d beta's terms), sum_p (dy / P) xhat (d gamma's)
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ci = lane + i * 64;
            if (valid && ci < cpr) {
                VecIO<T>::unpack(*(const uint4*)(dy + (long)b * lddy + ci * EPC), g[i]);
            } else {
#pragma unroll
                for (int e = 0; e < EPC; ++e) g[i][e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) sg[i][e] = 0.f;
        }
        for (int p = 0; p < P; ++p) {
            float xh[NCH][EPC], gw[NCH][EPC], rstd;
            const long row = (long)b * L + p;
            wave_row_stats<T, NCH, true>(x + row * ldx, valid, lane, cpr, fC, eps, xh, rstd);
            float a = 0.f, bb = 0.f;  // sum_c gw, sum_c gw * xhat
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int ci = lane + i * 64;
                if (valid && ci < cpr) {
                    float w[EPC];
                    load_f32<EPC>(gamma + ci * EPC, w);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const float gp = g[i][e] * invP;
                        sg[i][e] = fmaf(gp, xh[i][e], sg[i][e]);
                        gw[i][e] = gp * w[e];
                        a += gw[i][e];
                        bb = fmaf(gw[i][e], xh[i][e], bb);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < EPC; ++e) gw[i][e] = 0.f;
                }
            }
            a = wave_sum(a) / fC;
            bb = wave_sum(bb) / fC;
            if (valid) {
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const int ci = lane + i * 64;
                    if (ci < cpr) {
                        float o[EPC];
#pragma unroll
                        for (int e = 0; e < EPC; ++e) o[e] = rstd * (gw[i][e] - a - xh[i][e] * bb);
                        T* dst = dx + row * lddx + ci * EPC;
                        if (accumulate) {
                            // (the gradient is rounded to the storage type first, as a separate launch + add would)
                            float rv[EPC], sv[EPC];
                            VecIO<T>::unpack(VecIO<T>::pack(o), sv);
                            VecIO<T>::unpack(*(const uint4*)dst, rv);
#pragma unroll
                            for (int e = 0; e < EPC; ++e) o[e] = sv[e] + rv[e];
                        }
                        *(uint4*)dst = VecIO<T>::pack(o);
                    }
                }
            }
        }
        const unsigned rep = blockIdx.y % kStatReplicas;
        flush_wave_sums<NCH, EPC>(sg, sums, 0, C, rep, red);
        flush_wave_sums<NCH, EPC>(g, sums, 1, C, rep, red);
    }
    if (accumulate) return;
    const int r0 = blockIdx.x * kSlabRows < P ? P : blockIdx.x * kSlabRows;
    const int r1 = (blockIdx.x + 1) * kSlabRows < L ? (blockIdx.x + 1) * kSlabRows : L;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int k = 0; k < kWaves; ++k) {
        const int b = b0 + k;
        if (b >= B) break;
        for (int r = r0 + wave; r < r1; r += kWaves) {
            T* row = dx + ((long)b * L + r) * lddx;
            for (int ci = lane; ci < cpr; ci += 64) *(uint4*)(row + ci * EPC) = zero;
        }
    }
}

int check_shape(const char* who, int C, int dtype, int P, bool in_registers) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C > 0 && C % epc == 0, VT_ERR_UNSUPPORTED, "%s: C=%d must be a positive multiple of %d", who, C, epc);
    VT_REQUIRE(!in_registers || C <= 3072, VT_ERR_UNSUPPORTED, "%s: C=%d exceeds 3072 (a row is held in registers)", who, C);
    VT_REQUIRE(P >= 1 && P <= kMaxPrefix, VT_ERR_INVALID, "%s: P=%d prefix rows (1..%d)", who, P, kMaxPrefix);
    return VT_OK;
}

int check_rows(const char* who, const char* what, const void* p, int ld, int C, int dtype) {
    const int epc = vt_epc(dtype);
    VT_REQUIRE(p && vt_aligned16(p), VT_ERR_INVALID, "%s: %s is null or misaligned", who, what);
    VT_REQUIRE(ld >= C && ld % epc == 0, VT_ERR_INVALID, "%s: %s has row stride %d (C=%d, multiples of %d)", who, what, ld, C, epc);
    return VT_OK;
}

// chunks per lane of a wave that holds a row: the steps the kernels are instantiated for
int chunks_per_lane(int C, int dtype) {
    const int need = (C / vt_epc(dtype) + 63) / 64;
    static const int kSteps[] = {1, 2, 4, 6, 8, 12};
    for (int s : kSteps)
        if (s >= need) return s;
    return 12;
}

// (bf16 rows hold 8 elements per chunk: NCH <= 6 covers C <= 3072; f32 rows 4: NCH <= 12)
#define VT_POOL_DISPATCH(dtype, nch, ...)                       \
    do {                                                        \
        if ((dtype) == VT_BF16) {                               \
            typedef bf16_t T;                                   \
            switch (nch) {                                      \
                case 1: { constexpr int NCH = 1; __VA_ARGS__; } break; \
                case 2: { constexpr int NCH = 2; __VA_ARGS__; } break; \
                case 4: { constexpr int NCH = 4; __VA_ARGS__; } break; \
                default: { constexpr int NCH = 6; __VA_ARGS__; } break; \
            }                                                   \
        } else {                                                \
            typedef float T;                                    \
            switch (nch) {                                      \
                case 1: { constexpr int NCH = 1; __VA_ARGS__; } break; \
                case 2: { constexpr int NCH = 2; __VA_ARGS__; } break; \
                case 4: { constexpr int NCH = 4; __VA_ARGS__; } break; \
                case 6: { constexpr int NCH = 6; __VA_ARGS__; } break; \
                case 8: { constexpr int NCH = 8; __VA_ARGS__; } break; \
                default: { constexpr int NCH = 12; __VA_ARGS__; } break; \
            }                                                   \
        }                                                       \
    } while (0)

}  // namespace

extern "C" {

int vt_prefix_tokens_fwd(const void* embed, int32_t lde, const float* pe, const float* const* prefix, int32_t P, void* out,
                         int32_t ldo, int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_prefix_tokens_fwd";
    VT_TRY(check_shape(who, C, dtype, P, false));
    VT_REQUIRE(B > 0 && T > 0, VT_ERR_INVALID, "%s: B=%d T=%d", who, B, T);
    VT_TRY(check_rows(who, "embed", embed, lde, C, dtype));
    VT_TRY(check_rows(who, "out", out, ldo, C, dtype));
    VT_REQUIRE(pe && vt_aligned16(pe) && prefix, VT_ERR_INVALID, "%s: pe / prefix null or misaligned", who);
    PrefixPtrs pp = {};
    for (int p = 0; p < P; ++p) {
        VT_REQUIRE(prefix[p] && vt_aligned16(prefix[p]), VT_ERR_INVALID, "%s: prefix[%d] is null or misaligned", who, p);
        pp.p[p] = const_cast<float*>(prefix[p]);
    }
    const long items = (long)(P + T) * (C / vt_epc(dtype));
    const dim3 grid((unsigned)((items + kT - 1) / kT), (unsigned)(B < 8 ? B : 8));
    if (dtype == VT_BF16) {
        hipLaunchKernelGGL(prefix_tokens_fwd_kernel<bf16_t>, grid, dim3(kT), 0, (hipStream_t)stream, (const bf16_t*)embed, lde, pe,
                           pp, P, (bf16_t*)out, ldo, B, T, C);
    } else {
        hipLaunchKernelGGL(prefix_tokens_fwd_kernel<float>, grid, dim3(kT), 0, (hipStream_t)stream, (const float*)embed, lde, pe, pp,
                           P, (float*)out, ldo, B, T, C);
    }
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_prefix_tokens_bwd(const void* dout, int32_t lddo, void* dembed, int32_t lde, float* dpe, float* const* dprefix, int32_t P,
                         int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_prefix_tokens_bwd";
    VT_TRY(check_shape(who, C, dtype, P, false));
    VT_REQUIRE(B > 0 && T > 0, VT_ERR_INVALID, "%s: B=%d T=%d", who, B, T);
    VT_TRY(check_rows(who, "dout", dout, lddo, C, dtype));
    if (dembed) VT_TRY(check_rows(who, "dembed", dembed, lde, C, dtype));
    VT_REQUIRE(vt_aligned16(dpe), VT_ERR_INVALID, "%s: dpe misaligned", who);
    PrefixPtrs pp = {};
    bool any = dembed || dpe;
    for (int p = 0; p < P && dprefix; ++p) {
        VT_REQUIRE(vt_aligned16(dprefix[p]), VT_ERR_INVALID, "%s: dprefix[%d] misaligned", who, p);
        pp.p[p] = dprefix[p];
        any = any || dprefix[p];
    }
    VT_REQUIRE(any, VT_ERR_INVALID, "%s: dembed, dpe and every dprefix are null", who);
    const long items = (long)(P + T) * (C / vt_epc(dtype));
    const dim3 grid((unsigned)((items + kT - 1) / kT));
    if (dtype == VT_BF16) {
        hipLaunchKernelGGL(prefix_tokens_bwd_kernel<bf16_t>, grid, dim3(kT), 0, (hipStream_t)stream, (const bf16_t*)dout, lddo,
                           (bf16_t*)dembed, lde, dpe, pp, P, B, T, C);
    } else {
        hipLaunchKernelGGL(prefix_tokens_bwd_kernel<float>, grid, dim3(kT), 0, (hipStream_t)stream, (const float*)dout, lddo,
                           (float*)dembed, lde, dpe, pp, P, B, T, C);
    }
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_prefix_pool_fwd(const void* x, int32_t ldx, const float* gamma, const float* beta, void* y, int32_t ldy, int32_t B,
                       int32_t L, int32_t P, int32_t C, float eps, int32_t dtype, void* stream) {
    const char* who = "vt_prefix_pool_fwd";
    VT_TRY(check_shape(who, C, dtype, P, true));
    VT_REQUIRE(B > 0 && L >= P && eps >= 0.f, VT_ERR_INVALID, "%s: B=%d L=%d P=%d eps=%g", who, B, L, P, (double)eps);
    VT_TRY(check_rows(who, "x", x, ldx, C, dtype));
    VT_TRY(check_rows(who, "y", y, ldy, C, dtype));
    VT_REQUIRE(gamma && beta && vt_aligned16(gamma) && vt_aligned16(beta), VT_ERR_INVALID, "%s: gamma / beta null or misaligned",
               who);
    const dim3 grid((unsigned)((B + kWaves - 1) / kWaves));
    VT_POOL_DISPATCH(dtype, chunks_per_lane(C, dtype),
                     hipLaunchKernelGGL((prefix_pool_fwd_kernel<T, NCH>), grid, dim3(kT), 0, (hipStream_t)stream, (const T*)x, ldx,
                                        gamma, beta, (T*)y, ldy, B, L, P, C, eps));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_prefix_pool_bwd(const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* gamma, void* dx, int32_t lddx,
                       int32_t accumulate, float* sums, int32_t B, int32_t L, int32_t P, int32_t C, float eps, int32_t dtype,
                       void* stream) {
    const char* who = "vt_prefix_pool_bwd";
    VT_TRY(check_shape(who, C, dtype, P, true));
    VT_REQUIRE(B > 0 && L >= P && eps >= 0.f, VT_ERR_INVALID, "%s: B=%d L=%d P=%d eps=%g", who, B, L, P, (double)eps);
    VT_TRY(check_rows(who, "dy", dy, lddy, C, dtype));
    VT_TRY(check_rows(who, "x", x, ldx, C, dtype));
    VT_TRY(check_rows(who, "dx", dx, lddx, C, dtype));
    VT_REQUIRE(gamma && sums && vt_aligned16(gamma) && vt_aligned16(sums), VT_ERR_INVALID, "%s: gamma / sums null or misaligned",
               who);
    const int slabs = accumulate ? 1 : (L + kSlabRows - 1) / kSlabRows;
    const dim3 grid((unsigned)slabs, (unsigned)((B + kWaves - 1) / kWaves));
    VT_REQUIRE(grid.y <= 65535u, VT_ERR_UNSUPPORTED, "%s: B=%d exceeds %d images", who, B, 65535 * kWaves);
    VT_POOL_DISPATCH(dtype, chunks_per_lane(C, dtype),
                     hipLaunchKernelGGL((prefix_pool_bwd_kernel<T, NCH>), grid, dim3(kT), 0, (hipStream_t)stream, (const T*)dy, lddy,
                                        (const T*)x, ldx, gamma, (T*)dx, lddx, accumulate, sums, B, L, P, C, eps));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // extern "C"
