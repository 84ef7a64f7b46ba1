// vt_talking_attention.hip -- the two attention forms of CaiT (reference vision_toolbox/backbones/cait.py:16-51) and the
// token bookkeeping of its class-attention stage, for gfx950 (MI355X).
//
//   talking heads   A_h = s q_h k_h^T,  M_g = sum_h Wl[g,h] A_h + bl[g],  P_g = softmax_j M_g,  lse_g = logsumexp_j M_g,
//                   R_g = sum_h Ww[g,h] P_h + bw[g],  O_g = R_g v_g            (all heads of an image are coupled twice)
//   class attention plain softmax attention of ONE query row per image over Lk keys
//   token prepend   out[b] = [first | x[b]]: the class row in front of the patch rows
//
// Layout as vt_attention.hip: [B][L][heads * head_dim] token-major rows with a row stride each, head h is the channel slice
// [h D, (h + 1) D), so q | k | v may be slices of one buffer.  The L x L planes (A, M, P, R and their gradients) never reach
// memory.
//
// Talking heads (head_dim 48, heads <= 16).  A workgroup of 256 threads owns a 16-row tile of one image and ALL heads, and
// walks the 16-row tiles of the other side; thread (i, j) owns the pair (own-side row, other-side row) and holds the
// values of every head for that pair in registers, so both mixes are per-thread register arithmetic in f32.  The tiles
// are staged as f32 in LDS (rows at or beyond L and the channels of the padded heads are ZEROS, never memory); the head
// count is padded to HP in {2, 4, 8, 16} with zero rows / columns of Wl and Ww, which leaves every stored value exact.
// The f32 dtype, and the backward of both dtypes, run this f32-FMA decomposition (bf16 operands are widened when they are
// staged: loads and stores are the only bf16 rounding points).
//
// The bf16 FORWARD runs on the matrix unit (talk_fwd_mfma_kernel).  A workgroup owns 64 queries of an image and all heads, a
// wave 16 of them; Q (64 rows) and 16-key tiles of K and V are staged as bf16 rows of all heads in LDS.  Per head,
// S^T = K Q^T is two mfma_f32_16x16x32_bf16 whose second 32-deep step holds channels 32..47 and zeros (the operand
// fragments of lane groups 2 and 3 are zero registers): on gfx950 the 16-deep mfma_f32_16x16x16_bf16 issues at the same
// rate as the 32-deep one, so two padded steps beat three exact ones.  The accumulator tiles of all heads share one lane
// layout -- element r of lane (g, u) is key 4 g + r against query u -- so both mixes are per-lane f32 register arithmetic
// and the softmax statistics are one scalar per lane and head.  R, rounded to bf16, IS the B operand of
// O^T = V^T R^T in mfma_f32_16x16x16_bf16 (16 keys deep, exact for a 16-key tile), V read transposed with
// ds_read_b64_tr_b16.  Rounding points of this path: R as the operand of R V, and the store of O.
//
//   forward     pass 1 over the key tiles: running (max, sum) of M_g per pair owner, combined over the 16 key lanes -> lse;
//               pass 2: P = exp(M - lse), R = Ww P + bw through an LDS plane, O += R V.  Two passes because R mixes the
//               NORMALISED P of all heads: a running rescale per head does not commute with the mix.
//   backward    role Q owns a query tile: loop 1 over the key tiles builds delta_h = sum_j dP_h P_h (NOT rowsum(dO o O):
//               the post-softmax mix and its bias break that identity) into scratch; loop 2 forms dM, dA, accumulates dQ
//               and the workgroup's share of dWl, dbl, dWw, dbw (a 256-pair product per tile from two LDS planes).
//               role K owns a key tile and walks the query tiles with lse and delta: dK and dV.
//               A second kernel adds the parameter shares of all workgroups in a fixed order.  No atomics: every sum has
//               one owner and a fixed order, results are bit-identical from run to run.
//
// Class attention (head_dim 32 / 48 / 64): one wave per (image, head); a lane walks keys lane, lane + 64, ... with a running
// (max, sum, accumulator), the 64 partial states are combined by a butterfly and lane 0 stores.  K and V are read once.
// The backward takes delta = dO . O, recomputes P from lse and writes every row of dK and dV with plain stores.
#include "vt_common.h"
#include "vt_attn_frag.h"  // the bf16 register fragments of vt_attention.hip

#include <math.h>

namespace {

constexpr int kD = 48;    // head_dim of the talking-heads kernels
constexpr int kR = 16;    // rows of a tile, both sides
constexpr int kPL = 257;  // pitch of a [head][pair] plane (256 pairs + 1)

struct TalkArgs {
    const void *q, *k, *v, *dout;
    void *out, *dq, *dk, *dv;
    float* lse;
    const float *wl, *bl, *ww, *bw;
    float* delta;
    float* shares;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, L;
    float scale;
};

template <int HP>
constexpr int talk_lds_bytes() {
    return (2 * kR * (HP * kD + 1) + 2 * HP * kPL + 2 * HP * HP + 2 * HP + 2 * HP * kR) * 4;
}

template <int HP>
struct TalkLds {
    float *X, *Y, *P0, *P1, *Wl, *Ww, *bl, *bw, *lses, *dls;
    __device__ explicit TalkLds(float* sm) {
        constexpr int P = HP * kD + 1;
        X = sm;
        Y = X + kR * P;
        P0 = Y + kR * P;
        P1 = P0 + HP * kPL;
        Wl = P1 + HP * kPL;
        Ww = Wl + HP * HP;
        bl = Ww + HP * HP;
        bw = bl + HP;
        lses = bw + HP;
        dls = lses + HP * kR;
    }
};

// the mixing parameters, zero-padded to HP x HP / HP (visible after the next barrier)
template <int HP>
__device__ __forceinline__ void load_mix(const TalkLds<HP>& s, const TalkArgs& p, int tid) {
    const int H = p.H;
    for (int e = tid; e < HP * HP; e += 256) {
        const int g = e / HP, h = e - g * HP;
        const bool ok = g < H && h < H;
        s.Wl[e] = ok ? p.wl[g * H + h] : 0.f;
        s.Ww[e] = ok ? p.ww[g * H + h] : 0.f;
    }
    if (tid < HP) {
        s.bl[tid] = (tid < H && p.bl) ? p.bl[tid] : 0.f;
        s.bw[tid] = (tid < H && p.bw) ? p.bw[tid] : 0.f;
    }
}

// rows [row0, row0 + 16) of one image, channels [0, HP * 48) -> f32 LDS [16][HP * 48 + 1]; rows >= L and channels >= C zero
template <typename T, int HP>
__device__ __forceinline__ void stage_rows(float* dst, const T* __restrict__ src, int ld, int row0, int L, int C, int tid) {
    constexpr int E = VecIO<T>::EPC, P = HP * kD + 1, CH = HP * kD / E;
    for (int e = tid; e < kR * CH; e += 256) {
        const int r = e / CH, c = (e - r * CH) * E;
        float f[E];
#pragma unroll
        for (int x = 0; x < E; ++x) f[x] = 0.f;
        if (row0 + r < L && c < C) VecIO<T>::unpack(*(const uint4*)(src + (long)(row0 + r) * ld + c), f);
#pragma unroll
        for (int x = 0; x < E; ++x) dst[r * P + c + x] = f[x];
    }
}

__device__ __forceinline__ float dot48(const float* a, const float* b) {
    float s = 0.f;
#pragma unroll 4  // (a full unroll of every head's 48 steps lets the scheduler hoist the loads of all heads: spills)
    for (int d = 0; d < kD; ++d) s = fmaf(a[d], b[d], s);
    return s;
}

// scores of all heads for the pair (row i of X = Q, row j of Y = K), mixed: mv[g] = M_g
template <int HP>
__device__ __forceinline__ void mixed_scores(const TalkLds<HP>& s, int i, int j, float scale, float* a, float* mv) {
    constexpr int P = HP * kD + 1;
#pragma unroll
    for (int h = 0; h < HP; ++h) a[h] = scale * dot48(s.X + i * P + h * kD, s.Y + j * P + h * kD);
#pragma unroll
    for (int g = 0; g < HP; ++g) {
        float v = s.bl[g];
#pragma unroll
        for (int h = 0; h < HP; ++h) v = fmaf(s.Wl[g * HP + h], a[h], v);
        mv[g] = v;
    }
}

template <typename T, int HP>
__global__ void __launch_bounds__(256) talk_fwd_kernel(const TalkArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int P = HP * kD + 1;
    const TalkLds<HP> s(sm);
    const int tid = threadIdx.x, j = tid & 15, i = tid >> 4;
    const int b = blockIdx.y, q0 = blockIdx.x * kR, L = p.L, H = p.H, C = H * kD;
    const T* __restrict__ Q = (const T*)p.q + (long)b * L * p.ldq;
    const T* __restrict__ K = (const T*)p.k + (long)b * L * p.ldk;
    const T* __restrict__ V = (const T*)p.v + (long)b * L * p.ldv;
    load_mix<HP>(s, p, tid);
    stage_rows<T, HP>(s.X, Q, p.ldq, q0, L, C, tid);

    // pass 1: lse of the mixed scores
    float m[HP], l[HP];
#pragma unroll
    for (int g = 0; g < HP; ++g) m[g] = -INFINITY, l[g] = 0.f;
    for (int k0 = 0; k0 < L; k0 += kR) {
        __syncthreads();
        stage_rows<T, HP>(s.Y, K, p.ldk, k0, L, C, tid);
        __syncthreads();
        if (k0 + j < L) {
            float a[HP], mv[HP];
            mixed_scores<HP>(s, i, j, p.scale, a, mv);
#pragma unroll
            for (int g = 0; g < HP; ++g) {
                const float mn = fmaxf(m[g], mv[g]);  // finite
                l[g] = l[g] * expf(m[g] - mn) + expf(mv[g] - mn);
                m[g] = mn;
            }
        }
    }
    float lse[HP];
#pragma unroll
    for (int g = 0; g < HP; ++g) {
        float mg = m[g], lg = l[g];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const float m2 = __shfl_xor(mg, off, 64), l2 = __shfl_xor(lg, off, 64);
            const float mn = fmaxf(mg, m2);
            lg = (mn == -INFINITY) ? 0.f : lg * expf(mg - mn) + l2 * expf(m2 - mn);
            mg = mn;
        }
        // one value per query row, whatever order a lane added in: the row's lane 0 (key 0 exists, so its sum is > 0)
        lse[g] = __shfl(mg + logf(lg), (tid & 63) & ~15, 64);
        if (j == 0 && g < H && q0 + i < L) p.lse[((long)b * H + g) * L + q0 + i] = lse[g];
    }

    // pass 2: O = R V; thread (i, part) owns 3 channels of every head of query i
    const int part = j;
    float acc[HP][3];
#pragma unroll
    for (int g = 0; g < HP; ++g) acc[g][0] = acc[g][1] = acc[g][2] = 0.f;
    for (int k0 = 0; k0 < L; k0 += kR) {
        __syncthreads();
        stage_rows<T, HP>(s.Y, K, p.ldk, k0, L, C, tid);
        __syncthreads();
        {
            const bool valid = k0 + j < L;
            float a[HP], mv[HP];
            mixed_scores<HP>(s, i, j, p.scale, a, mv);
#pragma unroll
            for (int g = 0; g < HP; ++g) a[g] = valid ? expf(mv[g] - lse[g]) : 0.f;  // P
#pragma unroll
            for (int g = 0; g < HP; ++g) {
                float r = valid ? s.bw[g] : 0.f;
#pragma unroll
                for (int h = 0; h < HP; ++h) r = fmaf(s.Ww[g * HP + h], a[h], r);
                s.P0[g * kPL + tid] = r;
            }
        }
        __syncthreads();  // K is dead, R is complete
        stage_rows<T, HP>(s.Y, V, p.ldv, k0, L, C, tid);
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < kR; ++jj) {
#pragma unroll
            for (int g = 0; g < HP; ++g) {
                const float r = s.P0[g * kPL + i * kR + jj];
                const float* vr = s.Y + jj * P + g * kD + part * 3;
#pragma unroll
                for (int d = 0; d < 3; ++d) acc[g][d] = fmaf(r, vr[d], acc[g][d]);
            }
        }
    }
    if (q0 + i < L) {
        T* dst = (T*)p.out + ((long)b * L + q0 + i) * p.ldo + part * 3;
#pragma unroll
        for (int g = 0; g < HP; ++g)
            if (g < H) {
#pragma unroll
                for (int d = 0; d < 3; ++d) dst[g * kD + d] = from_float<T>(acc[g][d]);
            }
    }
}

// ---- bf16 forward on the matrix unit -------------------------------------------------------------------------------------
constexpr int kQT = 64;  // queries of a workgroup (16 per wave)

template <int HP>
constexpr int talk_mfma_lds_bytes() {
    return (kQT + 2 * kR) * (HP * kD + 8) * 2 + (2 * HP * HP + 2 * HP) * 4;
}

// rows [row0, row0 + rows) of one image, channels [0, HP * 48) -> bf16 LDS [rows][HP * 48 + 8]; rows >= L and channels >= C zero
template <int HP>
__device__ __forceinline__ void stage_bf16_rows(bf16_t* dst, const bf16_t* __restrict__ src, int ld, int row0, int rows, int L,
                                                int C, int tid) {
    constexpr int PR = HP * kD / 8, P8 = HP * kD + 8;
    for (int e = tid; e < rows * PR; e += 256) {
        const int r = e / PR, c = (e - r * PR) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row0 + r < L && c < C) v = *(const uint4*)(src + (long)(row0 + r) * ld + c);
        *(uint4*)(dst + r * P8 + c) = v;
    }
}

// head h of row `row`: reduction elements 32 kk + 8 g + j of its 48 channels, zeros beyond them
template <int HP>
__device__ __forceinline__ bf16x8 head_frag(const bf16_t* tile, int row, int h, int kk, int g) {
    if (kk == 1 && g >= 2) return __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
    return *(const bf16x8*)(tile + row * (HP * kD + 8) + h * kD + 32 * kk + 8 * g);
}

// scaled scores of all heads for the wave's 16 queries against the staged 16 keys: a[h][r] = A_h[query u][key 4 g + r]
template <int HP>
__device__ __forceinline__ void mfma_scores(const bf16_t* Qs, const bf16_t* Ks, int qrow, int u, int g, float scale, f32x4* a) {
#pragma unroll
    for (int h = 0; h < HP; ++h) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) acc = VT_MFMA(head_frag<HP>(Ks, u, h, kk, g), head_frag<HP>(Qs, qrow, h, kk, g), acc);
        a[h] = acc * scale;
    }
}

template <int HP>
__global__ void __launch_bounds__(256) talk_fwd_mfma_kernel(const TalkArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int P8 = HP * kD + 8;
    bf16_t* Qs = (bf16_t*)sm;
    bf16_t* Ks = Qs + kQT * P8;
    bf16_t* Vs = Ks + kR * P8;
    float* Wl = (float*)(Vs + kR * P8);
    float* Ww = Wl + HP * HP;
    float* bl = Ww + HP * HP;
    float* bw = bl + HP;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, u = lane & 15;
    const int b = blockIdx.y, q0 = blockIdx.x * kQT, L = p.L, H = p.H, C = H * kD;
    const int qrow = wave * 16 + u, myq = q0 + qrow;
    const bf16_t* __restrict__ Q = (const bf16_t*)p.q + (long)b * L * p.ldq;
    const bf16_t* __restrict__ K = (const bf16_t*)p.k + (long)b * L * p.ldk;
    const bf16_t* __restrict__ V = (const bf16_t*)p.v + (long)b * L * p.ldv;
    for (int e = tid; e < HP * HP; e += 256) {
        const int gg = e / HP, hh = e - gg * HP;
        const bool ok = gg < H && hh < H;
        Wl[e] = ok ? p.wl[gg * H + hh] : 0.f;
        Ww[e] = ok ? p.ww[gg * H + hh] : 0.f;
    }
    if (tid < HP) {
        bl[tid] = (tid < H && p.bl) ? p.bl[tid] : 0.f;
        bw[tid] = (tid < H && p.bw) ? p.bw[tid] : 0.f;
    }
    stage_bf16_rows<HP>(Qs, Q, p.ldq, q0, kQT, L, C, tid);

    // pass 1: lse of the mixed scores; a lane keeps the running (max, sum) of its own 4 keys per tile
    float m[HP], l[HP];
#pragma unroll
    for (int gg = 0; gg < HP; ++gg) m[gg] = -INFINITY, l[gg] = 0.f;
    for (int k0 = 0; k0 < L; k0 += kR) {
        __syncthreads();
        stage_bf16_rows<HP>(Ks, K, p.ldk, k0, kR, L, C, tid);
        __syncthreads();
        f32x4 a[HP];
        mfma_scores<HP>(Qs, Ks, qrow, u, g, p.scale, a);
#pragma unroll
        for (int gg = 0; gg < HP; ++gg) {
            f32x4 mv = f32x4{bl[gg], bl[gg], bl[gg], bl[gg]};
#pragma unroll
            for (int h = 0; h < HP; ++h) mv += a[h] * Wl[gg * HP + h];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (k0 + 4 * g + r < L) {
                    const float mn = fmaxf(m[gg], mv[r]);  // finite
                    l[gg] = l[gg] * __expf(m[gg] - mn) + __expf(mv[r] - mn);
                    m[gg] = mn;
                }
        }
    }
    float lse[HP];
#pragma unroll
    for (int gg = 0; gg < HP; ++gg) {
        float mg = m[gg], lg = l[gg];
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const float m2 = __shfl_xor(mg, off, 64), l2 = __shfl_xor(lg, off, 64);
            const float mn = fmaxf(mg, m2);
            lg = (mn == -INFINITY) ? 0.f : lg * __expf(mg - mn) + l2 * __expf(m2 - mn);
            mg = mn;
        }
        lse[gg] = __shfl(mg + __logf(lg), u, 64);  // one value per query: lane group 0's (it owns key 0, its sum is > 0)
        if (g == 0 && gg < H && myq < L) p.lse[((long)b * H + gg) * L + myq] = lse[gg];
    }

    // pass 2: P = exp(M - lse), R = Ww P + bw, O^T += V^T R^T
    f32x4 o[HP][3];
#pragma unroll
    for (int gg = 0; gg < HP; ++gg) o[gg][0] = o[gg][1] = o[gg][2] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < L; k0 += kR) {
        __syncthreads();
        stage_bf16_rows<HP>(Ks, K, p.ldk, k0, kR, L, C, tid);
        stage_bf16_rows<HP>(Vs, V, p.ldv, k0, kR, L, C, tid);
        __syncthreads();
        f32x4 a[HP], pr[HP];
        mfma_scores<HP>(Qs, Ks, qrow, u, g, p.scale, a);
#pragma unroll
        for (int gg = 0; gg < HP; ++gg) {
            f32x4 mv = f32x4{bl[gg], bl[gg], bl[gg], bl[gg]};
#pragma unroll
            for (int h = 0; h < HP; ++h) mv += a[h] * Wl[gg * HP + h];
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[gg][r] = (k0 + 4 * g + r < L) ? __expf(mv[r] - lse[gg]) : 0.f;
        }
#pragma unroll
        for (int gg = 0; gg < HP; ++gg) {
            if (gg < H) {
                f32x4 rv;
#pragma unroll
                for (int r = 0; r < 4; ++r) rv[r] = (k0 + 4 * g + r < L) ? bw[gg] : 0.f;
#pragma unroll
                for (int h = 0; h < HP; ++h) rv += pr[h] * Ww[gg * HP + h];
                const s16x4 rf = __builtin_bit_cast(
                    s16x4, make_uint2(VecIO<bf16_t>::pack2(rv[0], rv[1]), VecIO<bf16_t>::pack2(rv[2], rv[3])));
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    // column gg 48 + 16 i + u of the tile's rows 4 g + (0..3): the A operand of a 16-key step
                    const bf16_t* a0 = Vs + (4 * g + (u >> 2)) * P8 + gg * kD + 16 * i + 4 * (u & 3);
                    const s16x4 vf = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
                    o[gg][i] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vf, rf, o[gg][i], 0, 0, 0);
                }
            }
        }
    }
    if (myq < L) {
        // o[gg][i][r] = O^T[d = 16 i + 4 g + r][query u]
        bf16_t* dst = (bf16_t*)p.out + ((long)b * L + myq) * p.ldo + 4 * g;
#pragma unroll
        for (int gg = 0; gg < HP; ++gg)
            if (gg < H) {
#pragma unroll
                for (int i = 0; i < 3; ++i) store4_bf16(dst + gg * kD + 16 * i, o[gg][i], 1.f);
            }
    }
}

template <int HP>
int launch_talk_mfma(const TalkArgs& p, hipStream_t st, const char* who) {
    constexpr int lds = talk_mfma_lds_bytes<HP>();
    if (lds > 64 * 1024) {
        const int rc = vt_raise_dynamic_lds((const void*)talk_fwd_mfma_kernel<HP>, lds, who);
        if (rc != VT_OK) return rc;
    }
    hipLaunchKernelGGL(talk_fwd_mfma_kernel<HP>, dim3((unsigned)((p.L + kQT - 1) / kQT), (unsigned)p.B), dim3(256), lds, st, p);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

// Everything both backward roles need of the pair (query q0 + i, key k0 + j): a = A, pr = P, dR, dP.  lse_src[g * lstride]
// is the pair's lse_g (registers of role Q, the LDS tile of role K).  On return X holds the Q tile and Y the K tile.
template <typename T, int HP>
__device__ __forceinline__ void pair_terms(const TalkLds<HP>& s, const TalkArgs& p, const T* __restrict__ Q,
                                           const T* __restrict__ K, const T* __restrict__ V, const T* __restrict__ G, int q0,
                                           int k0, int i, int j, int tid, const float* lse_src, int lstride, float* a, float* pr,
                                           float* dR, float* dP) {
    constexpr int P = HP * kD + 1;
    const int L = p.L, C = p.H * kD;
    __syncthreads();
    stage_rows<T, HP>(s.X, G, p.lddo, q0, L, C, tid);
    stage_rows<T, HP>(s.Y, V, p.ldv, k0, L, C, tid);
    __syncthreads();
#pragma unroll
    for (int g = 0; g < HP; ++g) dR[g] = dot48(s.X + i * P + g * kD, s.Y + j * P + g * kD);  // zero outside L
    __syncthreads();
    stage_rows<T, HP>(s.X, Q, p.ldq, q0, L, C, tid);
    stage_rows<T, HP>(s.Y, K, p.ldk, k0, L, C, tid);
    __syncthreads();
    const bool valid = q0 + i < L && k0 + j < L;
    float mv[HP];
    mixed_scores<HP>(s, i, j, p.scale, a, mv);
#pragma unroll
    for (int g = 0; g < HP; ++g) pr[g] = valid ? expf(mv[g] - lse_src[g * lstride]) : 0.f;
#pragma unroll
    for (int h = 0; h < HP; ++h) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < HP; ++g) v = fmaf(s.Ww[g * HP + h], dR[g], v);
        dP[h] = v;
    }
}

// sum over the 256 pairs of plane0[tg] * plane1[th] (and of plane0[tg] alone): one (g, h) entry per thread
template <int HP>
__device__ __forceinline__ void pair_products(const TalkLds<HP>& s, int tid, float& mat, float& vec) {
    if (tid < HP * HP) {
        const int tg = tid / HP, th = tid - tg * HP;
        const float* x = s.P0 + tg * kPL;
        const float* y = s.P1 + th * kPL;
        float sm_ = 0.f, sv = 0.f;
        for (int e = 0; e < 256; ++e) {
            sm_ = fmaf(x[e], y[e], sm_);
            sv += x[e];
        }
        mat += sm_;
        vec += sv;
    }
}

// role Q: delta, dQ and the workgroup's share of the parameter gradients
template <typename T, int HP>
__global__ void __launch_bounds__(256) talk_bwd_q_kernel(const TalkArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int P = HP * kD + 1;
    const TalkLds<HP> s(sm);
    const int tid = threadIdx.x, j = tid & 15, i = tid >> 4;
    const int b = blockIdx.y, q0 = blockIdx.x * kR, L = p.L, H = p.H;
    const T* __restrict__ Q = (const T*)p.q + (long)b * L * p.ldq;
    const T* __restrict__ K = (const T*)p.k + (long)b * L * p.ldk;
    const T* __restrict__ V = (const T*)p.v + (long)b * L * p.ldv;
    const T* __restrict__ G = (const T*)p.dout + (long)b * L * p.lddo;
    load_mix<HP>(s, p, tid);
    float lse[HP], dl[HP];
#pragma unroll
    for (int g = 0; g < HP; ++g) {
        lse[g] = (g < H && q0 + i < L) ? p.lse[((long)b * H + g) * L + q0 + i] : 0.f;
        dl[g] = 0.f;
    }
    for (int k0 = 0; k0 < L; k0 += kR) {
        float a[HP], pr[HP], dR[HP], dP[HP];
        pair_terms<T, HP>(s, p, Q, K, V, G, q0, k0, i, j, tid, lse, 1, a, pr, dR, dP);
#pragma unroll
        for (int h = 0; h < HP; ++h) dl[h] = fmaf(dP[h], pr[h], dl[h]);
    }
#pragma unroll
    for (int h = 0; h < HP; ++h) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) dl[h] += __shfl_xor(dl[h], off, 64);  // a + b on both lanes: identical
        if (j == 0 && h < H && q0 + i < L) p.delta[((long)b * H + h) * L + q0 + i] = dl[h];
    }
    if (!p.dq && !p.shares) return;

    const int part = j;
    float acc[HP][3];
#pragma unroll
    for (int h = 0; h < HP; ++h) acc[h][0] = acc[h][1] = acc[h][2] = 0.f;
    float gWl = 0.f, gbl = 0.f, gWw = 0.f, gbw = 0.f;
    for (int k0 = 0; k0 < L; k0 += kR) {
        float a[HP], pr[HP], dR[HP], dP[HP], dM[HP];
        pair_terms<T, HP>(s, p, Q, K, V, G, q0, k0, i, j, tid, lse, 1, a, pr, dR, dP);
#pragma unroll
        for (int h = 0; h < HP; ++h) dM[h] = pr[h] * (dP[h] - dl[h]);
        if (p.shares) {
#pragma unroll
            for (int h = 0; h < HP; ++h) s.P0[h * kPL + tid] = dR[h], s.P1[h * kPL + tid] = pr[h];
            __syncthreads();
            pair_products<HP>(s, tid, gWw, gbw);
            __syncthreads();
#pragma unroll
            for (int h = 0; h < HP; ++h) s.P0[h * kPL + tid] = dM[h], s.P1[h * kPL + tid] = a[h];
            __syncthreads();
            pair_products<HP>(s, tid, gWl, gbl);
            __syncthreads();
        }
        if (p.dq) {
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                float v = 0.f;
#pragma unroll
                for (int g = 0; g < HP; ++g) v = fmaf(s.Wl[g * HP + h], dM[g], v);
                s.P0[h * kPL + tid] = v;  // dA
            }
            __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < kR; ++jj) {
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    const float da = s.P0[h * kPL + i * kR + jj];
                    const float* kr = s.Y + jj * P + h * kD + part * 3;
#pragma unroll
                    for (int d = 0; d < 3; ++d) acc[h][d] = fmaf(da, kr[d], acc[h][d]);
                }
            }
        }
    }
    if (p.dq && q0 + i < L) {
        T* dst = (T*)p.dq + ((long)b * L + q0 + i) * p.lddq + part * 3;
#pragma unroll
        for (int h = 0; h < HP; ++h)
            if (h < H) {
#pragma unroll
                for (int d = 0; d < 3; ++d) dst[h * kD + d] = from_float<T>(acc[h][d] * p.scale);
            }
    }
    if (p.shares && tid < HP * HP) {
        const int tg = tid / HP, th = tid - tg * HP;
        if (tg < H && th < H) {
            // [dWl H^2 | dbl H | dWw H^2 | dbw H] per workgroup
            float* sh = p.shares + ((long)b * gridDim.x + blockIdx.x) * (2 * H * H + 2 * H);
            sh[tg * H + th] = gWl;
            sh[H * H + H + tg * H + th] = gWw;
            if (th == 0) {
                sh[H * H + tg] = gbl;
                sh[2 * H * H + H + tg] = gbw;
            }
        }
    }
}

// role K: dK and dV of a key tile over all query tiles
template <typename T, int HP>
__global__ void __launch_bounds__(256) talk_bwd_kv_kernel(const TalkArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int P = HP * kD + 1;
    const TalkLds<HP> s(sm);
    const int tid = threadIdx.x, j = tid & 15, i = tid >> 4;
    const int jo = tid >> 4, part = tid & 15;  // the owner of (key jo, 3 channels of every head)
    const int b = blockIdx.y, k0 = blockIdx.x * kR, L = p.L, H = p.H, C = H * kD;
    const T* __restrict__ Q = (const T*)p.q + (long)b * L * p.ldq;
    const T* __restrict__ K = (const T*)p.k + (long)b * L * p.ldk;
    const T* __restrict__ V = (const T*)p.v + (long)b * L * p.ldv;
    const T* __restrict__ G = (const T*)p.dout + (long)b * L * p.lddo;
    load_mix<HP>(s, p, tid);
    float ak[HP][3], av[HP][3];
#pragma unroll
    for (int h = 0; h < HP; ++h) ak[h][0] = ak[h][1] = ak[h][2] = av[h][0] = av[h][1] = av[h][2] = 0.f;
    for (int q0 = 0; q0 < L; q0 += kR) {
        __syncthreads();  // the previous tile's readers of lses / dls are done
        for (int e = tid; e < HP * kR; e += 256) {
            const int g = e / kR, r = e - g * kR;
            const bool ok = g < H && q0 + r < L;
            s.lses[e] = ok ? p.lse[((long)b * H + g) * L + q0 + r] : 0.f;
            s.dls[e] = ok ? p.delta[((long)b * H + g) * L + q0 + r] : 0.f;
        }
        float a[HP], pr[HP], dR[HP], dP[HP];
        pair_terms<T, HP>(s, p, Q, K, V, G, q0, k0, i, j, tid, s.lses + i, kR, a, pr, dR, dP);
        const bool valid = q0 + i < L && k0 + j < L;
#pragma unroll
        for (int g = 0; g < HP; ++g) {
            float r = valid ? s.bw[g] : 0.f;
#pragma unroll
            for (int h = 0; h < HP; ++h) r = fmaf(s.Ww[g * HP + h], pr[h], r);
            s.P1[g * kPL + tid] = r;  // R
        }
#pragma unroll
        for (int h = 0; h < HP; ++h) dR[h] = pr[h] * (dP[h] - s.dls[h * kR + i]);  // dM
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            float v = 0.f;
#pragma unroll
            for (int g = 0; g < HP; ++g) v = fmaf(s.Wl[g * HP + h], dR[g], v);
            s.P0[h * kPL + tid] = v;  // dA
        }
        __syncthreads();
        if (p.dk) {
#pragma unroll 1
        for (int ii = 0; ii < kR; ++ii) {
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    const float da = s.P0[h * kPL + ii * kR + jo];
                    const float* qr = s.X + ii * P + h * kD + part * 3;
#pragma unroll
                    for (int d = 0; d < 3; ++d) ak[h][d] = fmaf(da, qr[d], ak[h][d]);
                }
            }
        }
        if (p.dv) {
            __syncthreads();
            stage_rows<T, HP>(s.X, G, p.lddo, q0, L, C, tid);
            __syncthreads();
#pragma unroll 1
        for (int ii = 0; ii < kR; ++ii) {
#pragma unroll
                for (int g = 0; g < HP; ++g) {
                    const float r = s.P1[g * kPL + ii * kR + jo];
                    const float* gr = s.X + ii * P + g * kD + part * 3;
#pragma unroll
                    for (int d = 0; d < 3; ++d) av[g][d] = fmaf(r, gr[d], av[g][d]);
                }
            }
        }
    }
    if (k0 + jo < L) {
        const long row = (long)b * L + k0 + jo;
#pragma unroll
        for (int h = 0; h < HP; ++h)
            if (h < H) {
                if (p.dk) {
                    T* dst = (T*)p.dk + row * p.lddk + h * kD + part * 3;
#pragma unroll
                    for (int d = 0; d < 3; ++d) dst[d] = from_float<T>(ak[h][d] * p.scale);
                }
                if (p.dv) {
                    T* dst = (T*)p.dv + row * p.lddv + h * kD + part * 3;
#pragma unroll
                    for (int d = 0; d < 3; ++d) dst[d] = from_float<T>(av[h][d]);
                }
            }
    }
}

// entry e of the parameter gradients += the shares of all workgroups: thread t adds shares t, t + 256, ... in order, then a
// fixed tree over the 256 partial sums
__global__ void __launch_bounds__(256) talk_param_reduce_kernel(const float* __restrict__ shares, long nwg, int H, float* dwl,
                                                                float* dbl, float* dww, float* dbw) {
    __shared__ float red[256];
    const int e = blockIdx.x, tid = threadIdx.x, ns = 2 * H * H + 2 * H;
    float sacc = 0.f;
    for (long w = tid; w < nwg; w += 256) sacc += shares[w * ns + e];
    red[tid] = sacc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const int hh = H * H;
        float* dst;
        if (e < hh)
            dst = dwl ? dwl + e : nullptr;
        else if (e < hh + H)
            dst = dbl ? dbl + (e - hh) : nullptr;
        else if (e < 2 * hh + H)
            dst = dww ? dww + (e - hh - H) : nullptr;
        else
            dst = dbw ? dbw + (e - 2 * hh - H) : nullptr;
        if (dst) *dst += red[0];
    }
}

// ---- class attention ---------------------------------------------------------------------------------------------------
template <typename T, int D>
__device__ __forceinline__ void load_row(const T* __restrict__ src, float* f) {
    constexpr int E = VecIO<T>::EPC;
#pragma unroll
    for (int c = 0; c < D; c += E) VecIO<T>::unpack(*(const uint4*)(src + c), f + c);
}

template <typename T, int D>
__device__ __forceinline__ void store_row(T* dst, const float* f) {
    constexpr int E = VecIO<T>::EPC;
#pragma unroll
    for (int c = 0; c < D; c += E) *(uint4*)(dst + c) = VecIO<T>::pack(f + c);
}

struct ClsArgs {
    const void *q, *k, *v, *o, *dout;
    void *out, *dq, *dk, *dv;
    float* lse;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int H, Lk;
    float scale;
};

template <typename T, int D>
__global__ void __launch_bounds__(64) cls_fwd_kernel(const ClsArgs p) {
    const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y, Lk = p.Lk;
    float qr[D], acc[D];
    load_row<T, D>((const T*)p.q + (long)b * p.ldq + h * D, qr);
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int j = lane; j < Lk; j += 64) {
        float r[D];
        load_row<T, D>((const T*)p.k + ((long)b * Lk + j) * p.ldk + h * D, r);
        float sc = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) sc = fmaf(qr[d], r[d], sc);
        sc *= p.scale;
        const float mn = fmaxf(m, sc);
        const float al = expf(m - mn), e = expf(sc - mn);
        l = l * al + e;
        m = mn;
        load_row<T, D>((const T*)p.v + ((long)b * Lk + j) * p.ldv + h * D, r);
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] = fmaf(e, r[d], acc[d] * al);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
        const float mn = fmaxf(m, m2);
        const bool any = mn != -INFINITY;  // a lane without keys carries (-inf, 0, 0)
        const float a1 = any ? expf(m - mn) : 0.f, a2 = any ? expf(m2 - mn) : 0.f;
        l = l * a1 + l2 * a2;
        m = mn;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] = acc[d] * a1 + __shfl_xor(acc[d], off, 64) * a2;
    }
    if (lane == 0) {
        const float inv = 1.f / l;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] *= inv;
        store_row<T, D>((T*)p.out + (long)b * p.ldo + h * D, acc);
        p.lse[(long)b * p.H + h] = m + logf(l);
    }
}

template <typename T, int D>
__global__ void __launch_bounds__(64) cls_bwd_kernel(const ClsArgs p) {
    const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y, Lk = p.Lk;
    float qr[D], gr[D], dqa[D];
    load_row<T, D>((const T*)p.q + (long)b * p.ldq + h * D, qr);
    load_row<T, D>((const T*)p.dout + (long)b * p.lddo + h * D, gr);
    float delta = 0.f;
    {
        float orow[D];
        load_row<T, D>((const T*)p.o + (long)b * p.ldo + h * D, orow);
#pragma unroll
        for (int d = 0; d < D; ++d) delta = fmaf(gr[d], orow[d], delta);
    }
    const float lse = p.lse[(long)b * p.H + h];
#pragma unroll
    for (int d = 0; d < D; ++d) dqa[d] = 0.f;
    for (int j = lane; j < Lk; j += 64) {
        const long row = (long)b * Lk + j;
        float r[D], w[D];
        load_row<T, D>((const T*)p.k + row * p.ldk + h * D, r);
        float sc = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) sc = fmaf(qr[d], r[d], sc);
        const float pr = expf(sc * p.scale - lse);
        load_row<T, D>((const T*)p.v + row * p.ldv + h * D, w);
        float dp = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) dp = fmaf(gr[d], w[d], dp);
        const float ds = pr * (dp - delta);
        if (p.dq) {
#pragma unroll
            for (int d = 0; d < D; ++d) dqa[d] = fmaf(ds, r[d], dqa[d]);
        }
        if (p.dv) {
#pragma unroll
            for (int d = 0; d < D; ++d) w[d] = pr * gr[d];
            store_row<T, D>((T*)p.dv + row * p.lddv + h * D, w);
        }
        if (p.dk) {
            const float c = ds * p.scale;
#pragma unroll
            for (int d = 0; d < D; ++d) w[d] = c * qr[d];
            store_row<T, D>((T*)p.dk + row * p.lddk + h * D, w);
        }
    }
    if (p.dq) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            float v = dqa[d];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
            dqa[d] = v * p.scale;
        }
        if (lane == 0) store_row<T, D>((T*)p.dq + (long)b * p.lddq + h * D, dqa);
    }
}

// ---- token prepend -----------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) token_prepend_fwd_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ first,
                                                                int ldf, const float* __restrict__ first_param,
                                                                T* __restrict__ out, int ldo, long n, int Tn, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C);
    const long r = idx / C;
    const int row = (int)(r % (Tn + 1));
    const long b = r / (Tn + 1);
    T v;
    if (row == 0)
        v = first ? first[b * ldf + c] : from_float<T>(first_param[c]);
    else
        v = x[(b * Tn + row - 1) * ldx + c];
    out[r * ldo + c] = v;
}

template <typename T>
__global__ void __launch_bounds__(256) token_prepend_bwd_kernel(const T* __restrict__ dout, int lddo, T* __restrict__ dx, int ldx,
                                                                int accumulate, T* __restrict__ dfirst, int ldf, long n, int Tn,
                                                                int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C);
    const long r = idx / C;
    const int row = (int)(r % (Tn + 1));
    const long b = r / (Tn + 1);
    const T v = dout[r * lddo + c];
    if (row == 0) {
        if (dfirst) dfirst[b * ldf + c] = v;
    } else if (dx) {
        T* dst = dx + (b * Tn + row - 1) * ldx + c;
        *dst = accumulate ? from_float<T>((float)*dst + (float)v) : v;
    }
}

// dfirst_param[c] += sum_b dout[b][0][c], the images in order
template <typename T>
__global__ void __launch_bounds__(256) token_prepend_param_kernel(const T* __restrict__ dout, int lddo, float* __restrict__ dparam,
                                                                  int B, int Tn, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float sacc = 0.f;
    for (int b = 0; b < B; ++b) sacc += (float)dout[(long)b * (Tn + 1) * lddo + c];
    dparam[c] += sacc;
}

int check_talk(const char* who, int B, int heads, int L, int head_dim, int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && heads > 0 && L > 0 && head_dim > 0, VT_ERR_INVALID, "%s: B=%d heads=%d L=%d head_dim=%d", who, B, heads, L,
               head_dim);
    VT_REQUIRE(head_dim == kD, VT_ERR_UNSUPPORTED, "%s: head_dim %d (48 has kernels)", who, head_dim);
    VT_REQUIRE(heads <= 16, VT_ERR_UNSUPPORTED, "%s: heads %d (at most 16: a workgroup holds every head of a pair)", who, heads);
    VT_REQUIRE(B <= 65535 && (long)B * heads * L < 0x7fffffffL, VT_ERR_UNSUPPORTED, "%s: B=%d heads=%d L=%d exceed the grid", who, B,
               heads, L);
    return VT_OK;
}

int check_cls(const char* who, int B, int heads, int Lk, int head_dim, int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && heads > 0 && Lk > 0 && head_dim > 0, VT_ERR_INVALID, "%s: B=%d heads=%d Lk=%d head_dim=%d", who, B, heads,
               Lk, head_dim);
    VT_REQUIRE(head_dim == 32 || head_dim == 48 || head_dim == 64, VT_ERR_UNSUPPORTED,
               "%s: head_dim %d (32, 48 and 64 have kernels)", who, head_dim);
    VT_REQUIRE(B <= 65535 && (long)B * Lk < 0x7fffffffL, VT_ERR_UNSUPPORTED, "%s: B=%d Lk=%d exceed the grid", who, B, Lk);
    return VT_OK;
}

template <typename K>
int launch_talk(K kern, int lds, const TalkArgs& p, hipStream_t st, const char* who) {
    if (lds > 64 * 1024) {
        const int rc = vt_raise_dynamic_lds((const void*)kern, lds, who);
        if (rc != VT_OK) return rc;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((p.L + kR - 1) / kR), (unsigned)p.B), dim3(256), lds, st, p);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

// KERN<T, HP> for the dtype and the padded head count
#define VT_TALK_DISPATCH(KERN, T)                                                                    \
    (p.H <= 2   ? launch_talk(KERN<T, 2>, talk_lds_bytes<2>(), p, st, who)                           \
     : p.H <= 4 ? launch_talk(KERN<T, 4>, talk_lds_bytes<4>(), p, st, who)                           \
     : p.H <= 8 ? launch_talk(KERN<T, 8>, talk_lds_bytes<8>(), p, st, who)                           \
                : launch_talk(KERN<T, 16>, talk_lds_bytes<16>(), p, st, who))
#define VT_TALK_LAUNCH(KERN) (dtype == VT_BF16 ? VT_TALK_DISPATCH(KERN, bf16_t) : VT_TALK_DISPATCH(KERN, float))

#define VT_CLS_LAUNCH(KERN, T, D) hipLaunchKernelGGL((KERN<T, D>), dim3((unsigned)heads, (unsigned)B), dim3(64), 0, st, p)
#define VT_CLS_DISPATCH(KERN)                          \
    do {                                               \
        if (dtype == VT_BF16) {                        \
            if (head_dim == 32)                        \
                VT_CLS_LAUNCH(KERN, bf16_t, 32);       \
            else if (head_dim == 48)                   \
                VT_CLS_LAUNCH(KERN, bf16_t, 48);       \
            else                                       \
                VT_CLS_LAUNCH(KERN, bf16_t, 64);       \
        } else {                                       \
            if (head_dim == 32)                        \
                VT_CLS_LAUNCH(KERN, float, 32);        \
            else if (head_dim == 48)                   \
                VT_CLS_LAUNCH(KERN, float, 48);        \
            else                                       \
                VT_CLS_LAUNCH(KERN, float, 64);        \
        }                                              \
    } while (0)

}  // namespace

extern "C" {

int vt_talk_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                     float* lse, const float* wl, const float* bl, const float* ww, const float* bw, float scale, int32_t B,
                     int32_t heads, int32_t L, int32_t head_dim, int32_t dtype, void* stream) {
    const char* who = "vt_talk_attn_fwd";
    VT_TRY(check_talk(who, B, heads, L, head_dim, dtype));
    const int C = heads * head_dim;
    VT_TRY(vt_check_rows(who, "q", q, ldq, C, dtype));
    VT_TRY(vt_check_rows(who, "k", k, ldk, C, dtype));
    VT_TRY(vt_check_rows(who, "v", v, ldv, C, dtype));
    VT_TRY(vt_check_rows(who, "o", o, ldo, C, dtype));
    VT_REQUIRE(lse && wl && ww, VT_ERR_INVALID, "%s: lse, wl or ww null", who);
    TalkArgs p = {};
    p.q = q, p.k = k, p.v = v, p.out = o, p.lse = lse, p.wl = wl, p.bl = bl, p.ww = ww, p.bw = bw;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    p.B = B, p.H = heads, p.L = L, p.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VT_BF16)
        return p.H <= 2 ? launch_talk_mfma<2>(p, st, who) : p.H <= 4 ? launch_talk_mfma<4>(p, st, who)
               : p.H <= 8 ? launch_talk_mfma<8>(p, st, who) : launch_talk_mfma<16>(p, st, who);
    return VT_TALK_DISPATCH(talk_fwd_kernel, float);
}

int64_t vt_talk_attn_bwd_scratch_bytes(int32_t B, int32_t heads, int32_t L) {
    if (B <= 0 || heads <= 0 || L <= 0) return 0;
    const int64_t tiles = (L + kR - 1) / kR;
    return 4 * ((int64_t)B * heads * L + (int64_t)B * tiles * (2 * heads * heads + 2 * heads));
}

int vt_talk_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* dout,
                     int32_t lddo, const float* lse, const float* wl, const float* bl, const float* ww, const float* bw, void* dq,
                     int32_t lddq, void* dk, int32_t lddk, void* dv, int32_t lddv, float* dwl, float* dbl, float* dww, float* dbw,
                     void* scratch, int64_t scratch_bytes, float scale, int32_t B, int32_t heads, int32_t L, int32_t head_dim,
                     int32_t dtype, void* stream) {
    const char* who = "vt_talk_attn_bwd";
    VT_TRY(check_talk(who, B, heads, L, head_dim, dtype));
    const int C = heads * head_dim;
    VT_TRY(vt_check_rows(who, "q", q, ldq, C, dtype));
    VT_TRY(vt_check_rows(who, "k", k, ldk, C, dtype));
    VT_TRY(vt_check_rows(who, "v", v, ldv, C, dtype));
    VT_TRY(vt_check_rows(who, "dout", dout, lddo, C, dtype));
    if (dq) VT_TRY(vt_check_rows(who, "dq", dq, lddq, C, dtype));
    if (dk) VT_TRY(vt_check_rows(who, "dk", dk, lddk, C, dtype));
    if (dv) VT_TRY(vt_check_rows(who, "dv", dv, lddv, C, dtype));
    const bool params = dwl || dbl || dww || dbw;
    VT_REQUIRE(dq || dk || dv || params, VT_ERR_INVALID, "%s: no output", who);
    VT_REQUIRE(lse && wl && ww, VT_ERR_INVALID, "%s: lse, wl or ww null", who);
    VT_REQUIRE(scratch && vt_aligned16(scratch) && scratch_bytes >= vt_talk_attn_bwd_scratch_bytes(B, heads, L), VT_ERR_INVALID,
               "%s: scratch null, misaligned or below vt_talk_attn_bwd_scratch_bytes = %ld bytes", who,
               (long)vt_talk_attn_bwd_scratch_bytes(B, heads, L));
    TalkArgs p = {};
    p.q = q, p.k = k, p.v = v, p.dout = dout, p.dq = dq, p.dk = dk, p.dv = dv;
    p.lse = (float*)lse, p.wl = wl, p.bl = bl, p.ww = ww, p.bw = bw;
    p.delta = (float*)scratch;
    p.shares = params ? (float*)scratch + (long)B * heads * L : nullptr;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.lddo = lddo, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
    p.B = B, p.H = heads, p.L = L, p.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    VT_TRY(VT_TALK_LAUNCH(talk_bwd_q_kernel));  // delta always: role K reads it
    if (params) {
        const long nwg = (long)B * ((L + kR - 1) / kR);
        hipLaunchKernelGGL(talk_param_reduce_kernel, dim3((unsigned)(2 * heads * heads + 2 * heads)), dim3(256), 0, st, p.shares, nwg,
                           heads, dwl, dbl, dww, dbw);
        VT_CHECK_LAUNCH(who);
    }
    if (dk || dv) VT_TRY(VT_TALK_LAUNCH(talk_bwd_kv_kernel));
    return VT_OK;
}

int vt_cls_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                    float* lse, float scale, int32_t B, int32_t heads, int32_t Lk, int32_t head_dim, int32_t dtype, void* stream) {
    const char* who = "vt_cls_attn_fwd";
    VT_TRY(check_cls(who, B, heads, Lk, head_dim, dtype));
    const int C = heads * head_dim;
    VT_TRY(vt_check_rows(who, "q", q, ldq, C, dtype));
    VT_TRY(vt_check_rows(who, "k", k, ldk, C, dtype));
    VT_TRY(vt_check_rows(who, "v", v, ldv, C, dtype));
    VT_TRY(vt_check_rows(who, "o", o, ldo, C, dtype));
    VT_REQUIRE(lse, VT_ERR_INVALID, "%s: lse null", who);
    ClsArgs p = {};
    p.q = q, p.k = k, p.v = v, p.out = o, p.lse = lse;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    p.H = heads, p.Lk = Lk, p.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    VT_CLS_DISPATCH(cls_fwd_kernel);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_cls_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o, int32_t ldo,
                    const void* dout, int32_t lddo, const float* lse, void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv,
                    int32_t lddv, float scale, int32_t B, int32_t heads, int32_t Lk, int32_t head_dim, int32_t dtype,
                    void* stream) {
    const char* who = "vt_cls_attn_bwd";
    VT_TRY(check_cls(who, B, heads, Lk, head_dim, dtype));
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
    ClsArgs p = {};
    p.q = q, p.k = k, p.v = v, p.o = o, p.dout = dout, p.dq = dq, p.dk = dk, p.dv = dv, p.lse = (float*)lse;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddo = lddo, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
    p.H = heads, p.Lk = Lk, p.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    VT_CLS_DISPATCH(cls_bwd_kernel);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_token_prepend_fwd(const void* x, int32_t ldx, const void* first, int32_t ldf, const float* first_param, void* out,
                         int32_t ldo, int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_token_prepend_fwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(x && out && B > 0 && T > 0 && C > 0 && ldx >= C && ldo >= C, VT_ERR_INVALID,
               "%s: B=%d T=%d C=%d ldx=%d ldo=%d or a null operand", who, B, T, C, ldx, ldo);
    VT_REQUIRE((first != nullptr) != (first_param != nullptr) && (!first || ldf >= C), VT_ERR_INVALID,
               "%s: exactly one of first (ldf=%d) and first_param must be given", who, ldf);
    const long n = (long)B * (T + 1) * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(token_prepend_fwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx,
                           (const bf16_t*)first, ldf, first_param, (bf16_t*)out, ldo, n, T, C);
    else
        hipLaunchKernelGGL(token_prepend_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx,
                           (const float*)first, ldf, first_param, (float*)out, ldo, n, T, C);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_token_prepend_bwd(const void* dout, int32_t lddo, void* dx, int32_t ldx, int32_t accumulate, void* dfirst, int32_t ldf,
                         float* dfirst_param, int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_token_prepend_bwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(dout && B > 0 && T > 0 && C > 0 && lddo >= C && (!dx || ldx >= C) && (!dfirst || ldf >= C), VT_ERR_INVALID,
               "%s: B=%d T=%d C=%d lddo=%d ldx=%d ldf=%d or dout null", who, B, T, C, lddo, ldx, ldf);
    VT_REQUIRE(dx || dfirst || dfirst_param, VT_ERR_INVALID, "%s: no output", who);
    VT_REQUIRE(!(dfirst && dfirst_param), VT_ERR_INVALID, "%s: dfirst and dfirst_param are the two forms of one gradient", who);
    hipStream_t st = (hipStream_t)stream;
    if (dx || dfirst) {
        const long n = (long)B * (T + 1) * C;
        const dim3 grid((unsigned)((n + 255) / 256));
        if (dtype == VT_BF16)
            hipLaunchKernelGGL(token_prepend_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)dout, lddo, (bf16_t*)dx, ldx,
                               accumulate, (bf16_t*)dfirst, ldf, n, T, C);
        else
            hipLaunchKernelGGL(token_prepend_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)dout, lddo, (float*)dx, ldx,
                               accumulate, (float*)dfirst, ldf, n, T, C);
        VT_CHECK_LAUNCH(who);
    }
    if (dfirst_param) {
        const dim3 grid((unsigned)((C + 255) / 256));
        if (dtype == VT_BF16)
            hipLaunchKernelGGL(token_prepend_param_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)dout, lddo, dfirst_param, B,
                               T, C);
        else
            hipLaunchKernelGGL(token_prepend_param_kernel<float>, grid, dim3(256), 0, st, (const float*)dout, lddo, dfirst_param, B, T,
                               C);
        VT_CHECK_LAUNCH(who);
    }
    return VT_OK;
}

}  // extern "C"

#undef VT_MFMA  // vt_attn_frag.h
