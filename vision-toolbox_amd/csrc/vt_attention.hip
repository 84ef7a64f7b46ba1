// vt_attention.hip -- multi-head self-attention, forward and backward, and the token bookkeeping of a ViT (class token,
// position embedding, class-token pooling) for gfx950 (MI355X).  Reference vision_toolbox/backbones/vit.py:34-46 (MHA:
// F.scaled_dot_product_attention over (B, heads, L, head_dim) views) and :145-151 (`+ pe`, the class token, `out[:, 0]`).
//
//   forward    O = softmax(scale Q K^T) V per (image, head), lse[b][h][q] = log sum_k exp(scale q.k)
//   backward   P = exp(scale Q K^T - lse), delta = rowsum(dO o O), dS = P o (dO V^T - delta)
//              dV = P^T dO, dK = scale dS^T Q, dQ = scale dS K
//
// Layout.  Q, K, V, O and their gradients are [B][L][heads * D] token-major rows with a row stride each; head h is the
// channel slice [h D, (h + 1) D).  Nothing is transposed in memory and the three operands may be channel slices of one
// [B][L][3 d] buffer, which is how the launch lists hold them.  The L x L scores never reach memory.
//
// bf16 (mfma_f32_16x16x32_bf16, f32 accumulators).  A workgroup is 4 waves and owns one 64-row tile of (image, head); a
// wave owns 16 of the rows and keeps their operand fragments in registers for its whole life, loaded straight from HBM.
// The workgroup walks the 64-row tiles of the OTHER side, staged row-major in LDS with rows at or beyond L zeroed.
// Every product is oriented so that the wave's own row index is the COLUMN (the lane) of the accumulator tile:
//
//   forward / dQ pass  (own rows: queries)   S^T = K Q^T     [key on the registers][query on the lane]
//   dK, dV pass        (own rows: keys)      S   = Q K^T     [query on the registers][key on the lane]
//
// so the softmax statistics (running maximum, sum, lse, delta) are one scalar per lane -- a row reduction is 15 in-lane
// operations and two cross-lane steps -- and the accumulator tile, rounded to bf16, IS the B operand of the product that
// follows (O^T = V^T P^T, dV^T = dO^T P, dK^T = Q^T dS, dQ^T = K^T dS^T), with no lane movement and no trip through LDS:
// k-step s takes registers of the 16-row sub-tiles 2s and 2s + 1, i.e. fragment element j of lane group g is row
// 32 s + 16 (j >> 2) + 4 g + (j & 3) of the tile.  The A operand of that product is the staged tile read TRANSPOSED in
// the same row order with ds_read_b64_tr_b16 (as vt_token_mix.hip reads x): V for the forward, K for dQ, dO and Q for
// dV / dK.  The results come out [d on the registers][own row on the lane]: a lane stores 4 consecutive channels of its
// row, 8 bytes.
//
// Rounding points of the bf16 path: P (operand of P V and of dV), dS (operand of dK and dQ), and the stores.  Scores,
// the exponent, lse, delta and every sum are f32; the maximum is subtracted before the exponent (online rescaling
// across key tiles), so scores of +-130 are as good as scores of +-1.
//
// Backward without atomics: the dK / dV kernel owns a key tile and loops over query tiles, the dQ kernel owns a query
// tile and loops over key tiles; delta comes from a small kernel of its own into the caller's scratch.  Every sum has one
// owner and a fixed order: results are bit-identical from run to run.
//
// Tails.  Keys at or beyond L are -inf before the maximum (forward) or P = 0 (backward); rows at or beyond L of a staged
// tile are ZEROS, never memory (0 * NaN from a padded V row would poison O); own rows at or beyond L load zeros and are
// not stored.
//
// The f32 dtype runs f32 FMA kernels with the same decomposition (exact f32 products, like every f32 kernel here).
#include "vt_common.h"
#include "vt_attn_frag.h"  // the bf16 register fragments, shared with vt_window_attention.hip

#include <math.h>

namespace {

struct AttnArgs {
    const void *q, *k, *v, *o, *dout;
    void *out, *dq, *dk, *dv;
    float* lse;
    float* delta;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, L;
    float scale;
};

// ---- bf16 pieces ---------------------------------------------------------------------------------------------------
// rows [row0, row0 + 64) of one (image, head) slice -> LDS [64][D + 8], rows >= L zero
template <int D>
__device__ __forceinline__ void stage_bf16(bf16_t* dst, const bf16_t* __restrict__ src, int ld, int row0, int L, int tid) {
    constexpr int PR = D / 8;
    for (int e = tid; e < kT * PR; e += 256) {
        const int r = e / PR, c = (e - r * PR) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row0 + r < L) v = *(const uint4*)(src + (long)(row0 + r) * ld + c);
        *(uint4*)(dst + r * (D + 8) + c) = v;
    }
}

template <int D>
__global__ void __launch_bounds__(256) attn_fwd_bf16_kernel(const AttnArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[kT * (D + 8)];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[kT * (D + 8)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, u = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z, L = p.L;
    const int myq = blockIdx.x * kT + wave * 16 + u;
    const bool qv = myq < L;
    const bf16_t* __restrict__ Q = (const bf16_t*)p.q + (long)b * L * p.ldq + h * D;
    const bf16_t* __restrict__ K = (const bf16_t*)p.k + (long)b * L * p.ldk + h * D;
    const bf16_t* __restrict__ V = (const bf16_t*)p.v + (long)b * L * p.ldv + h * D;
    bf16x8 qf[D / 32];
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) qf[kk] = frag_global(Q, p.ldq, myq, qv, kk, g);
    f32x4 o[D / 16];
#pragma unroll
    for (int i = 0; i < D / 16; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    for (int k0 = 0; k0 < L; k0 += kT) {
        __syncthreads();  // the previous tiles are dead
        stage_bf16<D>(Ks, K, p.ldk, k0, L, tid);
        stage_bf16<D>(Vs, V, p.ldv, k0, L, tid);
        __syncthreads();
        // s[t][r] = score of key k0 + 16 t + 4 g + r against query u
        f32x4 s[4];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < D / 32; ++kk) s[t] = VT_MFMA(frag_lds<D>(Ks, 16 * t + u, kk, g), qf[kk], s[t]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (k0 + 16 * t + 4 * g + r < L) ? s[t][r] * p.scale : -INFINITY;
                s[t][r] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);  // finite: key k0 exists
        const float alpha = __expf(m - mn);
        float rs = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(s[t][r] - mn);
                s[t][r] = e;
                rs += e;
            }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        m = mn;
#pragma unroll
        for (int i = 0; i < D / 16; ++i) o[i] *= alpha;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pf = pack8(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
            for (int i = 0; i < D / 16; ++i) o[i] = VT_MFMA(frag_tr<D>(Vs, ks, 16 * i, g, u), pf, o[i]);
        }
    }
    if (qv) {
        // o[i][r] = O^T[d = 16 i + 4 g + r][query u]
        const float inv = 1.f / l;
        bf16_t* dst = (bf16_t*)p.out + ((long)b * L + myq) * p.ldo + h * D + 4 * g;
#pragma unroll
        for (int i = 0; i < D / 16; ++i) store4_bf16(dst + 16 * i, o[i], inv);
        if (g == 0) p.lse[((long)b * p.H + h) * L + myq] = m + __logf(l);
    }
}

// dK, dV: the workgroup owns 64 keys (a wave 16 of them) and walks the query tiles
template <int D>
__global__ void __launch_bounds__(256) attn_bwd_kv_bf16_kernel(const AttnArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t Qs[kT * (D + 8)];
    __shared__ __attribute__((aligned(16))) bf16_t Gs[kT * (D + 8)];  // dO
    __shared__ __attribute__((aligned(16))) float lses[kT];
    __shared__ __attribute__((aligned(16))) float dls[kT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, u = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z, L = p.L;
    const int mykey = blockIdx.x * kT + wave * 16 + u;
    const bool kv = mykey < L;
    const bf16_t* __restrict__ Q = (const bf16_t*)p.q + (long)b * L * p.ldq + h * D;
    const bf16_t* __restrict__ K = (const bf16_t*)p.k + (long)b * L * p.ldk + h * D;
    const bf16_t* __restrict__ V = (const bf16_t*)p.v + (long)b * L * p.ldv + h * D;
    const bf16_t* __restrict__ G = (const bf16_t*)p.dout + (long)b * L * p.lddo + h * D;
    const float* __restrict__ lse = p.lse + ((long)b * p.H + h) * L;
    const float* __restrict__ delta = p.delta + ((long)b * p.H + h) * L;
    bf16x8 kf[D / 32], vf[D / 32];
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
        kf[kk] = frag_global(K, p.ldk, mykey, kv, kk, g);
        vf[kk] = frag_global(V, p.ldv, mykey, kv, kk, g);
    }
    f32x4 dk[D / 16], dv[D / 16];
#pragma unroll
    for (int i = 0; i < D / 16; ++i) dk[i] = dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int q0 = 0; q0 < L; q0 += kT) {
        __syncthreads();
        stage_bf16<D>(Qs, Q, p.ldq, q0, L, tid);
        stage_bf16<D>(Gs, G, p.lddo, q0, L, tid);
        if (tid < kT) {
            const bool ok = q0 + tid < L;
            lses[tid] = ok ? lse[q0 + tid] : 0.f;
            dls[tid] = ok ? delta[q0 + tid] : 0.f;
        }
        __syncthreads();
        // s[t][r]: query q0 + 16 t + 4 g + r against key u
        f32x4 s[4], dp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < D / 32; ++kk) {
                s[t] = VT_MFMA(frag_lds<D>(Qs, 16 * t + u, kk, g), kf[kk], s[t]);
                dp[t] = VT_MFMA(frag_lds<D>(Gs, 16 * t + u, kk, g), vf[kk], dp[t]);
            }
            const float4 ls = *(const float4*)&lses[16 * t + 4 * g], dl = *(const float4*)&dls[16 * t + 4 * g];
            const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dlv[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = kv && (q0 + 16 * t + 4 * g + r < L);
                const float pr = ok ? __expf(s[t][r] * p.scale - lsv[r]) : 0.f;
                s[t][r] = pr;
                dp[t][r] = pr * (dp[t][r] - dlv[r]);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pf = pack8(s[2 * ks], s[2 * ks + 1]);
            const bf16x8 df = pack8(dp[2 * ks], dp[2 * ks + 1]);
#pragma unroll
            for (int i = 0; i < D / 16; ++i) {
                dv[i] = VT_MFMA(frag_tr<D>(Gs, ks, 16 * i, g, u), pf, dv[i]);
                dk[i] = VT_MFMA(frag_tr<D>(Qs, ks, 16 * i, g, u), df, dk[i]);
            }
        }
    }
    if (kv) {
        if (p.dk) {
            bf16_t* dst = (bf16_t*)p.dk + ((long)b * L + mykey) * p.lddk + h * D + 4 * g;
#pragma unroll
            for (int i = 0; i < D / 16; ++i) store4_bf16(dst + 16 * i, dk[i], p.scale);
        }
        if (p.dv) {
            bf16_t* dst = (bf16_t*)p.dv + ((long)b * L + mykey) * p.lddv + h * D + 4 * g;
#pragma unroll
            for (int i = 0; i < D / 16; ++i) store4_bf16(dst + 16 * i, dv[i], 1.f);
        }
    }
}

// dQ: the workgroup owns 64 queries and walks the key tiles
template <int D>
__global__ void __launch_bounds__(256) attn_bwd_q_bf16_kernel(const AttnArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[kT * (D + 8)];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[kT * (D + 8)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, u = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z, L = p.L;
    const int myq = blockIdx.x * kT + wave * 16 + u;
    const bool qv = myq < L;
    const bf16_t* __restrict__ Q = (const bf16_t*)p.q + (long)b * L * p.ldq + h * D;
    const bf16_t* __restrict__ K = (const bf16_t*)p.k + (long)b * L * p.ldk + h * D;
    const bf16_t* __restrict__ V = (const bf16_t*)p.v + (long)b * L * p.ldv + h * D;
    const bf16_t* __restrict__ G = (const bf16_t*)p.dout + (long)b * L * p.lddo + h * D;
    bf16x8 qf[D / 32], gf[D / 32];
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
        qf[kk] = frag_global(Q, p.ldq, myq, qv, kk, g);
        gf[kk] = frag_global(G, p.lddo, myq, qv, kk, g);
    }
    const float lq = qv ? p.lse[((long)b * p.H + h) * L + myq] : 0.f;
    const float dq_ = qv ? p.delta[((long)b * p.H + h) * L + myq] : 0.f;
    f32x4 dq[D / 16];
#pragma unroll
    for (int i = 0; i < D / 16; ++i) dq[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < L; k0 += kT) {
        __syncthreads();
        stage_bf16<D>(Ks, K, p.ldk, k0, L, tid);
        stage_bf16<D>(Vs, V, p.ldv, k0, L, tid);
        __syncthreads();
        f32x4 ds[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
            ds[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < D / 32; ++kk) {
                s = VT_MFMA(frag_lds<D>(Ks, 16 * t + u, kk, g), qf[kk], s);
                ds[t] = VT_MFMA(frag_lds<D>(Vs, 16 * t + u, kk, g), gf[kk], ds[t]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = qv && (k0 + 16 * t + 4 * g + r < L);
                const float pr = ok ? __expf(s[r] * p.scale - lq) : 0.f;
                ds[t][r] = pr * (ds[t][r] - dq_);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 df = pack8(ds[2 * ks], ds[2 * ks + 1]);
#pragma unroll
            for (int i = 0; i < D / 16; ++i) dq[i] = VT_MFMA(frag_tr<D>(Ks, ks, 16 * i, g, u), df, dq[i]);
        }
    }
    if (qv) {
        bf16_t* dst = (bf16_t*)p.dq + ((long)b * L + myq) * p.lddq + h * D + 4 * g;
#pragma unroll
        for (int i = 0; i < D / 16; ++i) store4_bf16(dst + 16 * i, dq[i], p.scale);
    }
}

// ---- f32 pieces: 64 x 64 tiles in LDS, 4 threads per owned row, each a quarter of the head's channels ---------------------
template <int D>
__device__ __forceinline__ void stage_f32(float* dst, const float* __restrict__ src, int ld, int row0, int L, int tid) {
    constexpr int PR = D / 4;
    for (int e = tid; e < kT * PR; e += 256) {
        const int r = e / PR, c = (e - r * PR) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < L) v = *(const float4*)(src + (long)(row0 + r) * ld + c);
        float* d = dst + r * (D + 1) + c;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
}

template <int D>
__device__ __forceinline__ float dot_f32(const float* a, const float* b) {
    float s = 0.f;
#pragma unroll 8
    for (int d = 0; d < D; ++d) s = fmaf(a[d], b[d], s);
    return s;
}

template <int D>
constexpr int attn_f32_lds(int tiles, int mats) {
    return (tiles * kT * (D + 1) + mats * kT * (kT + 1) + 2 * kT) * 4;
}

template <int D>
__global__ void __launch_bounds__(256) attn_fwd_f32_kernel(const AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    constexpr int P = D + 1, DQ = D / 4;
    float* Qs = smf;
    float* Ks = Qs + kT * P;
    float* Vs = Ks + kT * P;
    float* Ps = Vs + kT * P;  // [64][65]
    const int tid = threadIdx.x, qi = tid >> 2, part = tid & 3;
    const int h = blockIdx.y, b = blockIdx.z, L = p.L, q0 = blockIdx.x * kT;
    const float* __restrict__ Q = (const float*)p.q + (long)b * L * p.ldq + h * D;
    const float* __restrict__ K = (const float*)p.k + (long)b * L * p.ldk + h * D;
    const float* __restrict__ V = (const float*)p.v + (long)b * L * p.ldv + h * D;
    stage_f32<D>(Qs, Q, p.ldq, q0, L, tid);
    float acc[DQ];
#pragma unroll
    for (int d = 0; d < DQ; ++d) acc[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < L; k0 += kT) {
        __syncthreads();
        stage_f32<D>(Ks, K, p.ldk, k0, L, tid);
        stage_f32<D>(Vs, V, p.ldv, k0, L, tid);
        __syncthreads();
        float s[16], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int key = part + 4 * j;
            const float v = (k0 + key < L) ? dot_f32<D>(Qs + qi * P, Ks + key * P) * p.scale : -INFINITY;
            s[j] = v;
            mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        float rs = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float e = expf(s[j] - mn);
            Ps[qi * (kT + 1) + part + 4 * j] = e;
            rs += e;
        }
        rs += __shfl_xor(rs, 1, 64);
        rs += __shfl_xor(rs, 2, 64);
        l = l * alpha + rs;
        m = mn;
        __syncthreads();
#pragma unroll
        for (int d = 0; d < DQ; ++d) acc[d] *= alpha;
        for (int key = 0; key < kT; ++key) {
            const float pv = Ps[qi * (kT + 1) + key];
#pragma unroll
            for (int d = 0; d < DQ; ++d) acc[d] = fmaf(pv, Vs[key * P + part * DQ + d], acc[d]);
        }
    }
    if (q0 + qi < L) {
        float* dst = (float*)p.out + ((long)b * L + q0 + qi) * p.ldo + h * D + part * DQ;
        const float inv = 1.f / l;
#pragma unroll
        for (int d = 0; d < DQ; ++d) dst[d] = acc[d] * inv;
        if (part == 0) p.lse[((long)b * p.H + h) * L + q0 + qi] = m + logf(l);
    }
}

// P and dS of one (query row, key row) pair of the staged tiles
template <int D>
__device__ __forceinline__ void pds_f32(const float* qrow, const float* grow, const float* krow, const float* vrow, bool ok,
                                        float lse, float delta, float scale, float& pr, float& ds) {
    const float s = dot_f32<D>(qrow, krow), dp = dot_f32<D>(grow, vrow);
    pr = ok ? expf(s * scale - lse) : 0.f;
    ds = pr * (dp - delta);
}

// role 0: dK, dV of a key tile (loop over query tiles); role 1: dQ of a query tile (loop over key tiles)
template <int D, int ROLE>
__global__ void __launch_bounds__(256) attn_bwd_f32_kernel(const AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    constexpr int P = D + 1, DQ = D / 4, PP = kT + 1;
    float* Qs = smf;
    float* Gs = Qs + kT * P;
    float* Ks = Gs + kT * P;
    float* Vs = Ks + kT * P;
    float* Ps = Vs + kT * P;   // [query][key]
    float* Ss = Ps + kT * PP;  // dS, [query][key]
    float* lses = Ss + kT * PP;
    float* dls = lses + kT;
    const int tid = threadIdx.x, own = tid >> 2, part = tid & 3;
    const int h = blockIdx.y, b = blockIdx.z, L = p.L, own0 = blockIdx.x * kT;
    const float* __restrict__ Q = (const float*)p.q + (long)b * L * p.ldq + h * D;
    const float* __restrict__ K = (const float*)p.k + (long)b * L * p.ldk + h * D;
    const float* __restrict__ V = (const float*)p.v + (long)b * L * p.ldv + h * D;
    const float* __restrict__ G = (const float*)p.dout + (long)b * L * p.lddo + h * D;
    const float* __restrict__ lse = p.lse + ((long)b * p.H + h) * L;
    const float* __restrict__ delta = p.delta + ((long)b * p.H + h) * L;
    float a0[DQ], a1[DQ];  // role 0: dK, dV; role 1: dQ, unused
#pragma unroll
    for (int d = 0; d < DQ; ++d) a0[d] = a1[d] = 0.f;
    for (int o0 = 0; o0 < L; o0 += kT) {
        const int q0 = ROLE == 0 ? o0 : own0, k0 = ROLE == 0 ? own0 : o0;
        __syncthreads();
        if (ROLE == 0 || o0 == 0) {
            stage_f32<D>(Qs, Q, p.ldq, q0, L, tid);
            stage_f32<D>(Gs, G, p.lddo, q0, L, tid);
            if (tid < kT) {
                const bool ok = q0 + tid < L;
                lses[tid] = ok ? lse[q0 + tid] : 0.f;
                dls[tid] = ok ? delta[q0 + tid] : 0.f;
            }
        }
        if (ROLE == 1 || o0 == 0) {
            stage_f32<D>(Ks, K, p.ldk, k0, L, tid);
            stage_f32<D>(Vs, V, p.ldv, k0, L, tid);
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < 16; ++j) {
            const int other = part + 4 * j;
            const int qr = ROLE == 0 ? other : own, kr = ROLE == 0 ? own : other;
            float pr, ds;
            pds_f32<D>(Qs + qr * P, Gs + qr * P, Ks + kr * P, Vs + kr * P, q0 + qr < L && k0 + kr < L, lses[qr], dls[qr], p.scale,
                       pr, ds);
            Ps[qr * PP + kr] = pr;
            Ss[qr * PP + kr] = ds;
        }
        __syncthreads();
        for (int o = 0; o < kT; ++o) {
            if (ROLE == 0) {
                const float pv = Ps[o * PP + own], dsv = Ss[o * PP + own];
#pragma unroll
                for (int d = 0; d < DQ; ++d) {
                    a0[d] = fmaf(dsv, Qs[o * P + part * DQ + d], a0[d]);
                    a1[d] = fmaf(pv, Gs[o * P + part * DQ + d], a1[d]);
                }
            } else {
                const float dsv = Ss[own * PP + o];
#pragma unroll
                for (int d = 0; d < DQ; ++d) a0[d] = fmaf(dsv, Ks[o * P + part * DQ + d], a0[d]);
            }
        }
    }
    if (own0 + own < L) {
        const long row = (long)b * L + own0 + own;
        if (ROLE == 0) {
            if (p.dk) {
                float* dst = (float*)p.dk + row * p.lddk + h * D + part * DQ;
#pragma unroll
                for (int d = 0; d < DQ; ++d) dst[d] = a0[d] * p.scale;
            }
            if (p.dv) {
                float* dst = (float*)p.dv + row * p.lddv + h * D + part * DQ;
#pragma unroll
                for (int d = 0; d < DQ; ++d) dst[d] = a1[d];
            }
        } else {
            float* dst = (float*)p.dq + row * p.lddq + h * D + part * DQ;
#pragma unroll
            for (int d = 0; d < DQ; ++d) dst[d] = a0[d] * p.scale;
        }
    }
}

// delta[b][h][q] = sum_d dO[b][q][h D + d] O[b][q][h D + d]
template <typename T>
__global__ void __launch_bounds__(256) attn_delta_kernel(const T* __restrict__ o, int ldo, const T* __restrict__ g, int ldg,
                                                         float* __restrict__ delta, long n, int H, int L, int D) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int q = (int)(idx % L);
    const long t = idx / L;
    const int h = (int)(t % H);
    const long b = t / H;
    const T* po = o + (b * L + q) * ldo + h * D;
    const T* pg = g + (b * L + q) * ldg + h * D;
    float s = 0.f;
    for (int d = 0; d < D; d += VecIO<T>::EPC) {
        float x[VecIO<T>::EPC], y[VecIO<T>::EPC];
        VecIO<T>::unpack(*(const uint4*)(po + d), x);
        VecIO<T>::unpack(*(const uint4*)(pg + d), y);
#pragma unroll
        for (int j = 0; j < VecIO<T>::EPC; ++j) s = fmaf(x[j], y[j], s);
    }
    delta[idx] = s;
}

// ---- token bookkeeping ------------------------------------------------------------------------------------------------
// out[b][0] = cls (c0 = 1), out[b][c0 + t] = embed[b][t] + pe[t]
template <typename T>
__global__ void __launch_bounds__(256) vit_tokens_fwd_kernel(const T* __restrict__ embed, int lde, const float* __restrict__ pe,
                                                             const float* __restrict__ cls, T* __restrict__ out, int ldo, long n,
                                                             int Tn, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c0 = cls ? 1 : 0;
    const int c = (int)(idx % C);
    const long r = idx / C;
    const int row = (int)(r % (Tn + c0));
    const long b = r / (Tn + c0);
    float v;
    if (row < c0)
        v = cls[c];
    else
        v = (float)embed[(b * Tn + row - c0) * lde + c] + pe[(long)(row - c0) * C + c];
    out[r * ldo + c] = from_float<T>(v);
}

// a thread owns (token row, channel) and walks the images in order: the copy, and the batch sums without atomics
template <typename T>
__global__ void __launch_bounds__(256) vit_tokens_bwd_kernel(const T* __restrict__ dout, int lddo, T* __restrict__ dembed, int lde,
                                                             float* __restrict__ dpe, float* __restrict__ dcls, int c0, int B,
                                                             int Tn, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)(Tn + c0) * C) return;
    const int c = (int)(idx % C), row = (int)(idx / C);
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const T v = dout[((long)b * (Tn + c0) + row) * lddo + c];
        s += (float)v;
        if (row >= c0 && dembed) dembed[((long)b * Tn + row - c0) * lde + c] = v;
    }
    if (row < c0) {
        if (dcls) dcls[c] += s;
    } else if (dpe) {
        dpe[(long)(row - c0) * C + c] += s;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) token_select_fwd_kernel(const T* __restrict__ x, int ldx, T* __restrict__ out, int ldo,
                                                               long n, int Tn, int t0, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C);
    const long b = idx / C;
    out[b * ldo + c] = x[(b * Tn + t0) * ldx + c];
}

template <typename T>
__global__ void __launch_bounds__(256) token_select_bwd_kernel(const T* __restrict__ dout, int lddo, T* __restrict__ dx, int ldx,
                                                               long n, int Tn, int t0, int C, int accumulate) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C);
    const long r = idx / C;
    const int row = (int)(r % Tn);
    const long b = r / Tn;
    T* dst = dx + r * ldx + c;
    if (row == t0) {
        const float v = (float)dout[b * lddo + c];
        *dst = accumulate ? from_float<T>((float)*dst + v) : from_float<T>(v);
    } else if (!accumulate) {
        *dst = from_float<T>(0.f);
    }
}

int check_attn(const char* who, int B, int heads, int L, int head_dim, int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && heads > 0 && L > 0 && head_dim > 0, VT_ERR_INVALID, "%s: B=%d heads=%d L=%d head_dim=%d", who, B, heads, L,
               head_dim);
    VT_REQUIRE(head_dim == 32 || head_dim == 64, VT_ERR_UNSUPPORTED, "%s: head_dim %d (32 and 64 have kernels)", who, head_dim);
    VT_REQUIRE(B <= 65535 && heads <= 65535 && (long)B * heads * L < 0x7fffffffL, VT_ERR_UNSUPPORTED,
               "%s: B=%d heads=%d L=%d exceed the grid", who, B, heads, L);
    return VT_OK;
}

template <typename K>
int launch_attn(K kern, int lds, const AttnArgs& p, int tiles, hipStream_t st, const char* who) {
    if (lds > 64 * 1024) {
        const int rc = vt_raise_dynamic_lds((const void*)kern, lds, who);
        if (rc != VT_OK) return rc;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)p.H, (unsigned)p.B), dim3(256), lds, st, p);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                float* lse, float scale, int32_t B, int32_t heads, int32_t L, int32_t head_dim, int32_t dtype, void* stream) {
    const char* who = "vt_attn_fwd";
    VT_TRY(check_attn(who, B, heads, L, head_dim, dtype));
    const int C = heads * head_dim;
    VT_TRY(vt_check_rows(who, "q", q, ldq, C, dtype));
    VT_TRY(vt_check_rows(who, "k", k, ldk, C, dtype));
    VT_TRY(vt_check_rows(who, "v", v, ldv, C, dtype));
    VT_TRY(vt_check_rows(who, "o", o, ldo, C, dtype));
    VT_REQUIRE(lse, VT_ERR_INVALID, "%s: lse null", who);
    AttnArgs p = {};
    p.q = q, p.k = k, p.v = v, p.out = o, p.lse = lse;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    p.B = B, p.H = heads, p.L = L, p.scale = scale;
    const int tiles = (L + kT - 1) / kT;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VT_BF16)
        return head_dim == 64 ? launch_attn(attn_fwd_bf16_kernel<64>, 0, p, tiles, st, who)
                              : launch_attn(attn_fwd_bf16_kernel<32>, 0, p, tiles, st, who);
    return head_dim == 64 ? launch_attn(attn_fwd_f32_kernel<64>, attn_f32_lds<64>(3, 1), p, tiles, st, who)
                          : launch_attn(attn_fwd_f32_kernel<32>, attn_f32_lds<32>(3, 1), p, tiles, st, who);
}

int64_t vt_attn_bwd_scratch_bytes(int32_t B, int32_t heads, int32_t L) {
    if (B <= 0 || heads <= 0 || L <= 0) return 0;
    return (int64_t)B * heads * L * 4;
}

int vt_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o, int32_t ldo,
                const void* dout, int32_t lddo, const float* lse, void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv,
                int32_t lddv, void* scratch, int64_t scratch_bytes, float scale, int32_t B, int32_t heads, int32_t L,
                int32_t head_dim, int32_t dtype, void* stream) {
    const char* who = "vt_attn_bwd";
    VT_TRY(check_attn(who, B, heads, L, head_dim, dtype));
    const int C = heads * head_dim;
    VT_TRY(vt_check_rows(who, "q", q, ldq, C, dtype));
    VT_TRY(vt_check_rows(who, "k", k, ldk, C, dtype));
    VT_TRY(vt_check_rows(who, "v", v, ldv, C, dtype));
    VT_TRY(vt_check_rows(who, "o", o, ldo, C, dtype));
    VT_TRY(vt_check_rows(who, "dout", dout, lddo, C, dtype));
    if (dq) VT_TRY(vt_check_rows(who, "dq", dq, lddq, C, dtype));
    if (dk) VT_TRY(vt_check_rows(who, "dk", dk, lddk, C, dtype));
    if (dv) VT_TRY(vt_check_rows(who, "dv", dv, lddv, C, dtype));
    VT_REQUIRE(dq || dk || dv, VT_ERR_INVALID, "%s: no output", who);
    VT_REQUIRE(lse, VT_ERR_INVALID, "%s: lse null", who);
    VT_REQUIRE(scratch && vt_aligned16(scratch) && scratch_bytes >= vt_attn_bwd_scratch_bytes(B, heads, L), VT_ERR_INVALID,
               "%s: scratch null, misaligned or below vt_attn_bwd_scratch_bytes = %ld bytes", who,
               (long)vt_attn_bwd_scratch_bytes(B, heads, L));
    AttnArgs p = {};
    p.q = q, p.k = k, p.v = v, p.o = o, p.dout = dout, p.dq = dq, p.dk = dk, p.dv = dv;
    p.lse = (float*)lse, p.delta = (float*)scratch;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddo = lddo, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
    p.B = B, p.H = heads, p.L = L, p.scale = scale;
    const int tiles = (L + kT - 1) / kT;
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)B * heads * L;
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(attn_delta_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const bf16_t*)o, ldo,
                           (const bf16_t*)dout, lddo, p.delta, n, heads, L, head_dim);
    else
        hipLaunchKernelGGL(attn_delta_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)o, ldo,
                           (const float*)dout, lddo, p.delta, n, heads, L, head_dim);
    VT_CHECK_LAUNCH(who);
    if (dk || dv) {
        if (dtype == VT_BF16)
            VT_TRY(head_dim == 64 ? launch_attn(attn_bwd_kv_bf16_kernel<64>, 0, p, tiles, st, who)
                                  : launch_attn(attn_bwd_kv_bf16_kernel<32>, 0, p, tiles, st, who));
        else
            VT_TRY(head_dim == 64 ? launch_attn(attn_bwd_f32_kernel<64, 0>, attn_f32_lds<64>(4, 2), p, tiles, st, who)
                                  : launch_attn(attn_bwd_f32_kernel<32, 0>, attn_f32_lds<32>(4, 2), p, tiles, st, who));
    }
    if (dq) {
        if (dtype == VT_BF16)
            VT_TRY(head_dim == 64 ? launch_attn(attn_bwd_q_bf16_kernel<64>, 0, p, tiles, st, who)
                                  : launch_attn(attn_bwd_q_bf16_kernel<32>, 0, p, tiles, st, who));
        else
            VT_TRY(head_dim == 64 ? launch_attn(attn_bwd_f32_kernel<64, 1>, attn_f32_lds<64>(4, 2), p, tiles, st, who)
                                  : launch_attn(attn_bwd_f32_kernel<32, 1>, attn_f32_lds<32>(4, 2), p, tiles, st, who));
    }
    return VT_OK;
}

int vt_vit_tokens_fwd(const void* embed, int32_t lde, const float* pe, const float* cls, void* out, int32_t ldo, int32_t B,
                      int32_t T, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_vit_tokens_fwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(embed && pe && out && B > 0 && T > 0 && C > 0 && lde >= C && ldo >= C, VT_ERR_INVALID,
               "%s: B=%d T=%d C=%d lde=%d ldo=%d or a null operand", who, B, T, C, lde, ldo);
    const long n = (long)B * (T + (cls ? 1 : 0)) * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(vit_tokens_fwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)embed, lde, pe, cls,
                           (bf16_t*)out, ldo, n, T, C);
    else
        hipLaunchKernelGGL(vit_tokens_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)embed, lde, pe, cls,
                           (float*)out, ldo, n, T, C);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_vit_tokens_bwd(const void* dout, int32_t lddo, void* dembed, int32_t lde, float* dpe, float* dcls, int32_t has_cls,
                      int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_vit_tokens_bwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(dout && B > 0 && T > 0 && C > 0 && lddo >= C && (!dembed || lde >= C) && (has_cls == 0 || has_cls == 1),
               VT_ERR_INVALID, "%s: B=%d T=%d C=%d lddo=%d lde=%d has_cls=%d or dout null", who, B, T, C, lddo, lde, has_cls);
    VT_REQUIRE(dembed || dpe || (has_cls && dcls), VT_ERR_INVALID, "%s: no output", who);
    const long n = (long)(T + has_cls) * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(vit_tokens_bwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout, lddo,
                           (bf16_t*)dembed, lde, dpe, dcls, has_cls, B, T, C);
    else
        hipLaunchKernelGGL(vit_tokens_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dout, lddo,
                           (float*)dembed, lde, dpe, dcls, has_cls, B, T, C);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_token_select_fwd(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t B, int32_t T, int32_t t0, int32_t C,
                        int32_t dtype, void* stream) {
    const char* who = "vt_token_select_fwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(x && out && B > 0 && T > 0 && C > 0 && t0 >= 0 && t0 < T && ldx >= C && ldo >= C, VT_ERR_INVALID,
               "%s: B=%d T=%d t0=%d C=%d ldx=%d ldo=%d or a null operand", who, B, T, t0, C, ldx, ldo);
    const long n = (long)B * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(token_select_fwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx,
                           (bf16_t*)out, ldo, n, T, t0, C);
    else
        hipLaunchKernelGGL(token_select_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, (float*)out,
                           ldo, n, T, t0, C);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_token_select_bwd(const void* dout, int32_t lddo, void* dx, int32_t ldx, int32_t accumulate, int32_t B, int32_t T,
                        int32_t t0, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_token_select_bwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(dout && dx && B > 0 && T > 0 && C > 0 && t0 >= 0 && t0 < T && ldx >= C && lddo >= C, VT_ERR_INVALID,
               "%s: B=%d T=%d t0=%d C=%d lddo=%d ldx=%d or a null operand", who, B, T, t0, C, lddo, ldx);
    const long n = (long)B * T * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(token_select_bwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout, lddo,
                           (bf16_t*)dx, ldx, n, T, t0, C, accumulate);
    else
        hipLaunchKernelGGL(token_select_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dout, lddo,
                           (float*)dx, ldx, n, T, t0, C, accumulate);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // extern "C"

#undef VT_MFMA  // vt_attn_frag.h
