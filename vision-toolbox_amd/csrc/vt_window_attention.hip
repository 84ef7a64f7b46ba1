// vt_window_attention.hip -- shifted-window multi-head attention with a learned relative-position bias, forward and
// backward, for gfx950 (MI355X).  Reference vision_toolbox/backbones/swin.py:32-86 (WindowAttention: roll(-shift) ->
// window_partition -> MHA.forward(attn_bias = table[index] (+ the -100 region mask)) -> window_unpartition -> roll(+shift)).
//
//   forward    S = scale Q K^T + bias + mask per (window, head), O = softmax(S) V, lse = log sum_k exp(S)
//   backward   P = exp(S - lse), delta = rowsum(dO o O), dS = P o (dO V^T - delta)
//              dV = P^T dO, dK = scale dS^T Q, dQ = scale dS K, dtable[h][rel(q, k)] += dS[q][k]
//
// Layout.  Q, K, V, O and their gradients are [B][H][W][heads * 32] pixel-major rows of an NHWC map with a pixel stride
// each; head h is the channel slice [32 h, 32 (h + 1)), and q | k | v may be three channel slices of one [B][H][W][3 C]
// buffer.  The partition, both rolls and the un-partition are index arithmetic (vt_window_index.h): token t of a window IS
// a pixel of the un-rolled map, for the loads and for the store; no map is gathered, rolled or copied.
//
// A window has ws^2 <= 64 tokens: one 64-row tile of the decomposition of vt_attention.hip, so a workgroup (4 waves) owns a
// (window, head) and there is no loop over tiles and no online rescaling.  Token rows at or beyond ws^2 are ZEROS in LDS and
// are never read from memory; keys there are -inf (forward) / P = 0 (backward).  The head's table row, the pixel of every
// token and its (i, j, region) live in LDS.
//
// bf16 (mfma_f32_16x16x32_bf16, f32 accumulators), orientations as in vt_attention.hip: the forward takes S^T = K Q^T
// [key on the registers][query on the lane], so the row maximum, the row sum and lse are one scalar per lane and P, rounded
// to bf16, is the B operand of O^T = V^T P^T as it stands.  The backward is ONE kernel: it takes S = Q K^T and dP = dO V^T
// [query on the registers][key on the lane], forms P and dS once, feeds them (rounded to bf16) to dV^T = dO^T P and
// dK^T = Q^T dS, and leaves dS in f32 in LDS, from where dQ^T = K^T dS^T reads its B operand and the table gradient its
// addends.  delta is computed in the kernel from O and dO.  Rounding points: P, dS as MFMA operands, and the stores.
//
// The table gradient without atomics: thread idx of the workgroup sums the dS[q][k] with rel(q, k) = idx in a fixed order
// and stores the window's share into the caller's scratch [B][windows][heads][(2 ws - 1)^2]; a second kernel adds the
// shares of a table element in a fixed order (64 lanes stride the windows, then a butterfly).  Results are bit-identical from
// run to run.
//
// f32: exact f32 FMA with the same decomposition (4 threads per token row).
#include "vt_common.h"
#include "vt_attn_frag.h"
#include "vt_window_index.h"

#include <math.h>

namespace {

constexpr int kD = 32;               // head_dim
constexpr int kP = kD + 8;           // bf16 tile pitch
constexpr int kPF = kD + 1;          // f32 tile pitch
constexpr int kPS = kT + 1;          // pitch of a [64][64] f32 matrix
constexpr int kMaxWs = 8;            // ws^2 <= 64
constexpr int kMaxIdx = (2 * kMaxWs - 1) * (2 * kMaxWs - 1);

struct WinArgs {
    const void *q, *k, *v, *o, *dout;
    void *out, *dq, *dk, *dv;
    float* lse;
    const float* table;
    float* partial;  // [B][windows][heads][(2 ws - 1)^2] or NULL
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, H, W, heads, ws, shift;
    float scale;
};

// pix[t]: y W + x of token t of window w (-1: t >= ws^2); info[t] = i | j << 8 | region << 16; tab: the head's table row
__device__ __forceinline__ void win_setup(const WinArgs& p, int w, int h, int tid, int* pix, int* info, float* tab) {
    const int ws = p.ws, L = ws * ws, n = (2 * ws - 1) * (2 * ws - 1);
    const int nwx = p.W / ws, wy = w / nwx, wx = w - wy * nwx;
    if (tid < kT) {
        int px = -1, inf = 0;
        if (tid < L) {
            int y, x;
            vt_win_pixel(wy, wx, tid, ws, p.shift, p.H, p.W, &y, &x);
            px = y * p.W + x;
            const int i = tid / ws, j = tid - i * ws;
            inf = i | (j << 8) | (vt_win_token_region(wy, wx, tid, ws, p.shift, p.H, p.W) << 16);
        }
        pix[tid] = px;
        info[tid] = inf;
    }
    for (int e = tid; e < n; e += 256) tab[e] = p.table[(long)h * n + e];
}

__device__ __forceinline__ int win_rel(int qi, int ki, int ws) {
    return vt_win_rel_index(qi & 255, (qi >> 8) & 255, ki & 255, (ki >> 8) & 255, ws);
}

// bias + mask of (query info, key info): -100 where the regions differ, as the reference (not -inf)
__device__ __forceinline__ float win_bias(const float* tab, int qi, int ki, int ws) {
    return tab[win_rel(qi, ki, ws)] + ((qi >> 16) != (ki >> 16) ? -100.f : 0.f);
}

// the window's share of the table gradient: thread idx sums dS[q][k] over the pairs with rel(q, k) = idx, q ascending
__device__ __forceinline__ void win_dtable_share(const float* Ss, float* dst, int ws, int tid) {
    const int m = 2 * ws - 1;
    if (tid >= m * m) return;
    const int di = tid / m - (ws - 1), dj = tid % m - (ws - 1);
    float acc = 0.f;
    for (int iq = max(0, di); iq < min(ws, ws + di); ++iq)
        for (int jq = max(0, dj); jq < min(ws, ws + dj); ++jq)
            acc += Ss[(iq * ws + jq) * kPS + (iq - di) * ws + (jq - dj)];
    dst[tid] = acc;
}

// ---- bf16 ------------------------------------------------------------------------------------------------------------
// the 64 token rows of one (window, head) -> LDS [64][40]; one 16-byte chunk per thread
__device__ __forceinline__ void win_stage_bf16(bf16_t* dst, const bf16_t* __restrict__ src, int ld, const int* pix, int tid) {
    const int r = tid >> 2, c = (tid & 3) * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (pix[r] >= 0) v = *(const uint4*)(src + (long)pix[r] * ld + c);
    *(uint4*)(dst + r * kP + c) = v;
}

__global__ void __launch_bounds__(256) win_fwd_bf16_kernel(const WinArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[kT * kP];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[kT * kP];
    __shared__ int pix[kT], info[kT];
    __shared__ float tab[kMaxIdx];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, u = lane & 15;
    const int w = blockIdx.x, h = blockIdx.y, b = blockIdx.z, ws = p.ws, L = ws * ws;
    win_setup(p, w, h, tid, pix, info, tab);
    __syncthreads();
    const long img = (long)b * p.H * p.W;
    const bf16_t* __restrict__ Q = (const bf16_t*)p.q + img * p.ldq + h * kD;
    win_stage_bf16(Ks, (const bf16_t*)p.k + img * p.ldk + h * kD, p.ldk, pix, tid);
    win_stage_bf16(Vs, (const bf16_t*)p.v + img * p.ldv + h * kD, p.ldv, pix, tid);
    const int myt = wave * 16 + u;
    const bool qv = myt < L;
    const int mypix = pix[myt], qi = info[myt];
    const bf16x8 qf = frag_global(Q, p.ldq, mypix, qv, 0, g);
    __syncthreads();
    // s[t][r] = score of key 16 t + 4 g + r against query u
    f32x4 s[4];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        s[t] = VT_MFMA(frag_lds<kD>(Ks, 16 * t + u, 0, g), qf, (f32x4{0.f, 0.f, 0.f, 0.f}));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = 16 * t + 4 * g + r;
            const float v = key < L ? s[t][r] * p.scale + win_bias(tab, qi, info[key], ws) : -INFINITY;
            s[t][r] = v;
            mx = fmaxf(mx, v);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // finite: key 0 exists and the mask is -100
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(s[t][r] - mx);
            s[t][r] = e;
            l += e;
        }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 o[kD / 16];
#pragma unroll
    for (int i = 0; i < kD / 16; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 pf = pack8(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
        for (int i = 0; i < kD / 16; ++i) o[i] = VT_MFMA(frag_tr<kD>(Vs, ks, 16 * i, g, u), pf, o[i]);
    }
    if (qv) {
        // o[i][r] = O^T[d = 16 i + 4 g + r][query u]
        const float inv = 1.f / l;
        bf16_t* dst = (bf16_t*)p.out + (img + mypix) * p.ldo + h * kD + 4 * g;
#pragma unroll
        for (int i = 0; i < kD / 16; ++i) store4_bf16(dst + 16 * i, o[i], inv);
        if (g == 0) p.lse[((long)b * p.heads + h) * p.H * p.W + mypix] = mx + __logf(l);
    }
}

__global__ void __launch_bounds__(256) win_bwd_bf16_kernel(const WinArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t Qs[kT * kP];
    __shared__ __attribute__((aligned(16))) bf16_t Ks[kT * kP];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[kT * kP];
    __shared__ __attribute__((aligned(16))) bf16_t Gs[kT * kP];  // dO
    __shared__ float Ss[kT * kPS];                               // dS, [query][key]
    __shared__ __attribute__((aligned(16))) float lses[kT];
    __shared__ __attribute__((aligned(16))) float dls[kT];
    __shared__ int pix[kT], info[kT];
    __shared__ float tab[kMaxIdx];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, u = lane & 15;
    const int w = blockIdx.x, h = blockIdx.y, b = blockIdx.z, ws = p.ws, L = ws * ws;
    win_setup(p, w, h, tid, pix, info, tab);
    __syncthreads();
    const long img = (long)b * p.H * p.W;
    const bf16_t* __restrict__ G = (const bf16_t*)p.dout + img * p.lddo + h * kD;
    win_stage_bf16(Qs, (const bf16_t*)p.q + img * p.ldq + h * kD, p.ldq, pix, tid);
    win_stage_bf16(Ks, (const bf16_t*)p.k + img * p.ldk + h * kD, p.ldk, pix, tid);
    win_stage_bf16(Vs, (const bf16_t*)p.v + img * p.ldv + h * kD, p.ldv, pix, tid);
    win_stage_bf16(Gs, G, p.lddo, pix, tid);
    {
        // delta of row tid >> 2: four threads, 8 channels each
        const int r = tid >> 2, c = (tid & 3) * 8, px = pix[r];
        float d = 0.f;
        if (px >= 0) {
            float x[8], y[8];
            VecIO<bf16_t>::unpack(*(const uint4*)((const bf16_t*)p.o + (img + px) * p.ldo + h * kD + c), x);
            VecIO<bf16_t>::unpack(*(const uint4*)(G + (long)px * p.lddo + c), y);
#pragma unroll
            for (int j = 0; j < 8; ++j) d = fmaf(x[j], y[j], d);
        }
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        if ((tid & 3) == 0) {
            dls[r] = d;
            lses[r] = px >= 0 ? p.lse[((long)b * p.heads + h) * p.H * p.W + px] : 0.f;
        }
    }
    __syncthreads();

    // the wave's 16 rows as KEYS: s[t][r], dp[t][r] of query 16 t + 4 g + r against key u
    const int myt = wave * 16 + u;
    const bool tv = myt < L;
    const int mypix = pix[myt], ki = info[myt];
    {
        const bf16x8 kf = frag_lds<kD>(Ks, myt, 0, g), vf = frag_lds<kD>(Vs, myt, 0, g);
        f32x4 s[4], dp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = VT_MFMA(frag_lds<kD>(Qs, 16 * t + u, 0, g), kf, (f32x4{0.f, 0.f, 0.f, 0.f}));
            dp[t] = VT_MFMA(frag_lds<kD>(Gs, 16 * t + u, 0, g), vf, (f32x4{0.f, 0.f, 0.f, 0.f}));
            const float4 ls = *(const float4*)&lses[16 * t + 4 * g], dl = *(const float4*)&dls[16 * t + 4 * g];
            const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dlv[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = 16 * t + 4 * g + r;
                const bool ok = tv && qr < L;
                const float pr = ok ? __expf(s[t][r] * p.scale + win_bias(tab, info[qr], ki, ws) - lsv[r]) : 0.f;
                const float ds = pr * (dp[t][r] - dlv[r]);
                s[t][r] = pr;
                dp[t][r] = ds;
                Ss[qr * kPS + myt] = ds;
            }
        }
        f32x4 dk[kD / 16], dv[kD / 16];
#pragma unroll
        for (int i = 0; i < kD / 16; ++i) dk[i] = dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pf = pack8(s[2 * ks], s[2 * ks + 1]);
            const bf16x8 df = pack8(dp[2 * ks], dp[2 * ks + 1]);
#pragma unroll
            for (int i = 0; i < kD / 16; ++i) {
                dv[i] = VT_MFMA(frag_tr<kD>(Gs, ks, 16 * i, g, u), pf, dv[i]);
                dk[i] = VT_MFMA(frag_tr<kD>(Qs, ks, 16 * i, g, u), df, dk[i]);
            }
        }
        if (tv) {
            if (p.dk) {
                bf16_t* dst = (bf16_t*)p.dk + (img + mypix) * p.lddk + h * kD + 4 * g;
#pragma unroll
                for (int i = 0; i < kD / 16; ++i) store4_bf16(dst + 16 * i, dk[i], p.scale);
            }
            if (p.dv) {
                bf16_t* dst = (bf16_t*)p.dv + (img + mypix) * p.lddv + h * kD + 4 * g;
#pragma unroll
                for (int i = 0; i < kD / 16; ++i) store4_bf16(dst + 16 * i, dv[i], 1.f);
            }
        }
    }
    __syncthreads();  // dS is complete

    // the wave's 16 rows as QUERIES: dS^T[key 16 t + 4 g + r][query u] from LDS is the B operand of dQ^T = K^T dS^T
    if (p.dq) {
        f32x4 ds[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[t][r] = Ss[myt * kPS + 16 * t + 4 * g + r];
        f32x4 dq[kD / 16];
#pragma unroll
        for (int i = 0; i < kD / 16; ++i) dq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 df = pack8(ds[2 * ks], ds[2 * ks + 1]);
#pragma unroll
            for (int i = 0; i < kD / 16; ++i) dq[i] = VT_MFMA(frag_tr<kD>(Ks, ks, 16 * i, g, u), df, dq[i]);
        }
        if (tv) {
            bf16_t* dst = (bf16_t*)p.dq + (img + mypix) * p.lddq + h * kD + 4 * g;
#pragma unroll
            for (int i = 0; i < kD / 16; ++i) store4_bf16(dst + 16 * i, dq[i], p.scale);
        }
    }
    if (p.partial) {
        const int m = 2 * ws - 1;
        win_dtable_share(Ss, p.partial + (((long)b * gridDim.x + w) * p.heads + h) * (m * m), ws, tid);
    }
}

// ---- f32: 4 threads per token row, each a quarter of the keys (scores) / of the head's channels (products) ------------------
__device__ __forceinline__ void win_stage_f32(float* dst, const float* __restrict__ src, int ld, const int* pix, int tid) {
    for (int e = tid; e < kT * (kD / 4); e += 256) {
        const int r = e / (kD / 4), c = (e - r * (kD / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pix[r] >= 0) v = *(const float4*)(src + (long)pix[r] * ld + c);
        float* d = dst + r * kPF + c;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
}

__device__ __forceinline__ float win_dot(const float* a, const float* b) {
    float s = 0.f;
#pragma unroll 8
    for (int d = 0; d < kD; ++d) s = fmaf(a[d], b[d], s);
    return s;
}

__global__ void __launch_bounds__(256) win_fwd_f32_kernel(const WinArgs p) {
    __shared__ float Qs[kT * kPF], Ks[kT * kPF], Vs[kT * kPF], Ps[kT * kPS];
    __shared__ int pix[kT], info[kT];
    __shared__ float tab[kMaxIdx];
    constexpr int DQ = kD / 4;
    const int tid = threadIdx.x, own = tid >> 2, part = tid & 3;
    const int w = blockIdx.x, h = blockIdx.y, b = blockIdx.z, ws = p.ws, L = ws * ws;
    win_setup(p, w, h, tid, pix, info, tab);
    __syncthreads();
    const long img = (long)b * p.H * p.W;
    win_stage_f32(Qs, (const float*)p.q + img * p.ldq + h * kD, p.ldq, pix, tid);
    win_stage_f32(Ks, (const float*)p.k + img * p.ldk + h * kD, p.ldk, pix, tid);
    win_stage_f32(Vs, (const float*)p.v + img * p.ldv + h * kD, p.ldv, pix, tid);
    __syncthreads();
    const int qi = info[own];
    float s[16], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int key = part + 4 * j;
        const float v = key < L ? win_dot(Qs + own * kPF, Ks + key * kPF) * p.scale + win_bias(tab, qi, info[key], ws) : -INFINITY;
        s[j] = v;
        mx = fmaxf(mx, v);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float e = expf(s[j] - mx);
        Ps[own * kPS + part + 4 * j] = e;
        l += e;
    }
    l += __shfl_xor(l, 1, 64);
    l += __shfl_xor(l, 2, 64);
    __syncthreads();
    float acc[DQ];
#pragma unroll
    for (int d = 0; d < DQ; ++d) acc[d] = 0.f;
    for (int key = 0; key < kT; ++key) {
        const float pv = Ps[own * kPS + key];
#pragma unroll
        for (int d = 0; d < DQ; ++d) acc[d] = fmaf(pv, Vs[key * kPF + part * DQ + d], acc[d]);
    }
    if (own < L) {
        float* dst = (float*)p.out + (img + pix[own]) * p.ldo + h * kD + part * DQ;
        const float inv = 1.f / l;
#pragma unroll
        for (int d = 0; d < DQ; ++d) dst[d] = acc[d] * inv;
        if (part == 0) p.lse[((long)b * p.heads + h) * p.H * p.W + pix[own]] = mx + logf(l);
    }
}

constexpr int kBwdF32Lds = (4 * kT * kPF + 2 * kT * kPS + 2 * kT + kMaxIdx) * 4 + 2 * kT * 4;

__global__ void __launch_bounds__(256) win_bwd_f32_kernel(const WinArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    constexpr int DQ = kD / 4;
    float* Qs = smf;
    float* Gs = Qs + kT * kPF;
    float* Ks = Gs + kT * kPF;
    float* Vs = Ks + kT * kPF;
    float* Ps = Vs + kT * kPF;   // [query][key]
    float* Ss = Ps + kT * kPS;   // dS, [query][key]
    float* lses = Ss + kT * kPS;
    float* dls = lses + kT;
    float* tab = dls + kT;
    int* pix = (int*)(tab + kMaxIdx);
    int* info = pix + kT;
    const int tid = threadIdx.x, own = tid >> 2, part = tid & 3;
    const int w = blockIdx.x, h = blockIdx.y, b = blockIdx.z, ws = p.ws, L = ws * ws;
    win_setup(p, w, h, tid, pix, info, tab);
    __syncthreads();
    const long img = (long)b * p.H * p.W;
    const float* __restrict__ G = (const float*)p.dout + img * p.lddo + h * kD;
    win_stage_f32(Qs, (const float*)p.q + img * p.ldq + h * kD, p.ldq, pix, tid);
    win_stage_f32(Ks, (const float*)p.k + img * p.ldk + h * kD, p.ldk, pix, tid);
    win_stage_f32(Vs, (const float*)p.v + img * p.ldv + h * kD, p.ldv, pix, tid);
    win_stage_f32(Gs, G, p.lddo, pix, tid);
    const int px = pix[own];
    {
        float d = 0.f;
        if (px >= 0) {
            const float* po = (const float*)p.o + (img + px) * p.ldo + h * kD + part * DQ;
            const float* pg = G + (long)px * p.lddo + part * DQ;
#pragma unroll
            for (int j = 0; j < DQ; ++j) d = fmaf(po[j], pg[j], d);
        }
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        if (part == 0) {
            dls[own] = d;
            lses[own] = px >= 0 ? p.lse[((long)b * p.heads + h) * p.H * p.W + px] : 0.f;
        }
    }
    __syncthreads();
    {
        const int qi = info[own];
        const float lq = lses[own], dq_ = dls[own];
#pragma unroll 1
        for (int j = 0; j < 16; ++j) {
            const int key = part + 4 * j;
            const float sc = win_dot(Qs + own * kPF, Ks + key * kPF), dp = win_dot(Gs + own * kPF, Vs + key * kPF);
            const float pr = (own < L && key < L) ? expf(sc * p.scale + win_bias(tab, qi, info[key], ws) - lq) : 0.f;
            Ps[own * kPS + key] = pr;
            Ss[own * kPS + key] = pr * (dp - dq_);
        }
    }
    __syncthreads();
    float a0[DQ], a1[DQ], a2[DQ];  // dK, dV, dQ of token row `own`
#pragma unroll
    for (int d = 0; d < DQ; ++d) a0[d] = a1[d] = a2[d] = 0.f;
    for (int o = 0; o < kT; ++o) {
        const float pv = Ps[o * kPS + own], dsk = Ss[o * kPS + own], dsq = Ss[own * kPS + o];
#pragma unroll
        for (int d = 0; d < DQ; ++d) {
            a0[d] = fmaf(dsk, Qs[o * kPF + part * DQ + d], a0[d]);
            a1[d] = fmaf(pv, Gs[o * kPF + part * DQ + d], a1[d]);
            a2[d] = fmaf(dsq, Ks[o * kPF + part * DQ + d], a2[d]);
        }
    }
    if (own < L) {
        const long row = img + px;
        if (p.dk) {
            float* dst = (float*)p.dk + row * p.lddk + h * kD + part * DQ;
#pragma unroll
            for (int d = 0; d < DQ; ++d) dst[d] = a0[d] * p.scale;
        }
        if (p.dv) {
            float* dst = (float*)p.dv + row * p.lddv + h * kD + part * DQ;
#pragma unroll
            for (int d = 0; d < DQ; ++d) dst[d] = a1[d];
        }
        if (p.dq) {
            float* dst = (float*)p.dq + row * p.lddq + h * kD + part * DQ;
#pragma unroll
            for (int d = 0; d < DQ; ++d) dst[d] = a2[d] * p.scale;
        }
    }
    if (p.partial) {
        const int m = 2 * ws - 1;
        win_dtable_share(Ss, p.partial + (((long)b * gridDim.x + w) * p.heads + h) * (m * m), ws, tid);
    }
}

// dtable[h][idx] += sum over the nwg (image, window) shares, in a fixed order: lane l adds shares l, l + 64, ... in order,
// then a butterfly over the 64 lanes.  One wave per table element.
__global__ void __launch_bounds__(64) win_dtable_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dtable,
                                                               long nwg, int heads, int n) {
    const int idx = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    float s = 0.f;
    for (long w = lane; w < nwg; w += 64) s += partial[(w * heads + h) * n + idx];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) dtable[(long)h * n + idx] += s;
}

int win_check_rows(const char* who, const char* what, const void* ptr, int ld, int C, int dtype) {
    VT_REQUIRE(ptr && vt_aligned16(ptr) && ld >= C && ld % vt_epc(dtype) == 0, VT_ERR_INVALID,
               "%s: %s null, not 16-byte aligned, or its pixel stride %d is below %d channels / no multiple of a 16-byte chunk (%d "
               "elements)",
               who, what, ld, C, vt_epc(dtype));
    return VT_OK;
}

int win_check(const char* who, int B, int H, int W, int heads, int head_dim, int ws, int shift, int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0 && head_dim > 0 && ws > 0, VT_ERR_INVALID,
               "%s: B=%d H=%d W=%d heads=%d head_dim=%d ws=%d", who, B, H, W, heads, head_dim, ws);
    VT_REQUIRE(head_dim == kD, VT_ERR_UNSUPPORTED, "%s: head_dim %d (32 has kernels)", who, head_dim);
    VT_REQUIRE(ws <= kMaxWs, VT_ERR_UNSUPPORTED, "%s: ws=%d: a window of %d tokens does not fit the 64-row tile (ws <= %d)", who, ws,
               ws * ws, kMaxWs);
    VT_REQUIRE(shift >= 0 && shift < ws, VT_ERR_INVALID, "%s: shift=%d is not in [0, ws=%d)", who, shift, ws);
    VT_REQUIRE(H % ws == 0 && W % ws == 0, VT_ERR_INVALID, "%s: H=%d W=%d are no multiples of ws=%d", who, H, W, ws);
    VT_REQUIRE(B <= 65535 && heads <= 65535 && (long)H * W < 0x7fffffffL && (long)B * heads * H * W < (1L << 40), VT_ERR_UNSUPPORTED,
               "%s: B=%d heads=%d H=%d W=%d exceed the grid", who, B, heads, H, W);
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_win_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                    float* lse, const float* table, float scale, int32_t B, int32_t H, int32_t W, int32_t heads, int32_t head_dim,
                    int32_t ws, int32_t shift, int32_t dtype, void* stream) {
    const char* who = "vt_win_attn_fwd";
    VT_TRY(win_check(who, B, H, W, heads, head_dim, ws, shift, dtype));
    const int C = heads * head_dim;
    VT_TRY(win_check_rows(who, "q", q, ldq, C, dtype));
    VT_TRY(win_check_rows(who, "k", k, ldk, C, dtype));
    VT_TRY(win_check_rows(who, "v", v, ldv, C, dtype));
    VT_TRY(win_check_rows(who, "o", o, ldo, C, dtype));
    VT_REQUIRE(lse && table, VT_ERR_INVALID, "%s: lse or table null", who);
    WinArgs p = {};
    p.q = q, p.k = k, p.v = v, p.out = o, p.lse = lse, p.table = table;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    p.B = B, p.H = H, p.W = W, p.heads = heads, p.ws = ws, p.shift = shift, p.scale = scale;
    const dim3 grid((unsigned)((H / ws) * (W / ws)), (unsigned)heads, (unsigned)B);
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(win_fwd_bf16_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(win_fwd_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int64_t vt_win_attn_bwd_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t heads, int32_t ws) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || ws <= 0) return 0;
    return (int64_t)B * (H / ws) * (W / ws) * heads * (2 * ws - 1) * (2 * ws - 1) * 4;
}

int vt_win_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o,
                    int32_t ldo, const void* dout, int32_t lddo, const float* lse, const float* table, void* dq, int32_t lddq,
                    void* dk, int32_t lddk, void* dv, int32_t lddv, float* dtable, void* scratch, int64_t scratch_bytes,
                    float scale, int32_t B, int32_t H, int32_t W, int32_t heads, int32_t head_dim, int32_t ws, int32_t shift,
                    int32_t dtype, void* stream) {
    const char* who = "vt_win_attn_bwd";
    VT_TRY(win_check(who, B, H, W, heads, head_dim, ws, shift, dtype));
    const int C = heads * head_dim;
    VT_TRY(win_check_rows(who, "q", q, ldq, C, dtype));
    VT_TRY(win_check_rows(who, "k", k, ldk, C, dtype));
    VT_TRY(win_check_rows(who, "v", v, ldv, C, dtype));
    VT_TRY(win_check_rows(who, "o", o, ldo, C, dtype));
    VT_TRY(win_check_rows(who, "dout", dout, lddo, C, dtype));
    if (dq) VT_TRY(win_check_rows(who, "dq", dq, lddq, C, dtype));
    if (dk) VT_TRY(win_check_rows(who, "dk", dk, lddk, C, dtype));
    if (dv) VT_TRY(win_check_rows(who, "dv", dv, lddv, C, dtype));
    VT_REQUIRE(dq || dk || dv || dtable, VT_ERR_INVALID, "%s: no output", who);
    VT_REQUIRE(lse && table, VT_ERR_INVALID, "%s: lse or table null", who);
    const int64_t need = vt_win_attn_bwd_scratch_bytes(B, H, W, heads, ws);
    VT_REQUIRE(!dtable || (scratch && vt_aligned16(scratch) && scratch_bytes >= need), VT_ERR_INVALID,
               "%s: scratch null, misaligned or its %ld bytes are below vt_win_attn_bwd_scratch_bytes = %ld bytes", who,
               (long)scratch_bytes, (long)need);
    WinArgs p = {};
    p.q = q, p.k = k, p.v = v, p.o = o, p.dout = dout, p.dq = dq, p.dk = dk, p.dv = dv;
    p.lse = (float*)lse, p.table = table, p.partial = dtable ? (float*)scratch : nullptr;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddo = lddo, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
    p.B = B, p.H = H, p.W = W, p.heads = heads, p.ws = ws, p.shift = shift, p.scale = scale;
    const int nw = (H / ws) * (W / ws);
    const dim3 grid((unsigned)nw, (unsigned)heads, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VT_BF16) {
        hipLaunchKernelGGL(win_bwd_bf16_kernel, grid, dim3(256), 0, st, p);
    } else {
        VT_TRY(vt_raise_dynamic_lds((const void*)win_bwd_f32_kernel, kBwdF32Lds, who));
        hipLaunchKernelGGL(win_bwd_f32_kernel, grid, dim3(256), kBwdF32Lds, st, p);
    }
    VT_CHECK_LAUNCH(who);
    if (dtable) {
        const int n = (2 * ws - 1) * (2 * ws - 1);
        hipLaunchKernelGGL(win_dtable_reduce_kernel, dim3((unsigned)n, (unsigned)heads), dim3(64), 0, st, (const float*)scratch, dtable,
                           (long)B * nw, heads, n);
        VT_CHECK_LAUNCH(who);
    }
    return VT_OK;
}

}  // extern "C"

#undef VT_MFMA  // vt_attn_frag.h
