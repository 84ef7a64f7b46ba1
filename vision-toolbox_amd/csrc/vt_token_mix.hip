// vt_token_mix.hip -- token mixing (a Linear over the TOKEN axis of an NHWC map) and the patch embedding's
// patch gather for gfx950 (MI355X).  MLP-Mixer: reference vision_toolbox/backbones/mlp_mixer.py:28,34
// (`token_mixing(norm1(x).transpose(-1, -2)).transpose(-1, -2)`) and :52,60 (the p x p stride-p convolution).
//
//   forward / data gradient   out[b][m][c] = sum_k A[m][k] in[b][k][c] (+ bias[m]) (+ residual[b][m][c])
//                             A[m][k] = W[m * ldw + k], or W[k * ldw + m] (transw: the data gradient reads the same W)
//   filter gradient           dW[m][k] += sum_{b,c} dz[b][m][c] x[b][k][c],  dbias[m] += sum_{b,c} dz[b][m][c]
//
// Every other GEMM of this library reduces over channels.  Here the reduction index of the forward is the PIXEL index:
// x has c contiguous while an MFMA operand wants k contiguous per lane.  The map is never transposed in memory (the
// reference materialises two transposes per block): a [128 k][64 c] tile of x is staged row-major in LDS exactly as
// it lies in HBM (16-byte loads, whole 128-byte rows), and the fragments are formed by the transposing read
// ds_read_b64_tr_b16 -- lane 4q+pp of a 16-lane group addresses row q, columns 4pp..4pp+3 of a 4 x 16 block and
// receives column (lane & 15) of the block's 4 rows.  EXEC is all ones at these reads: tiles are zero padded (K tails,
// M tails, C tails), lanes are never masked in the loop.
//
// bf16 forward: a workgroup (4 waves, 2 x 2) owns 64 output rows m for its whole life.  Its slice of W (64 x K, zero
// padded to a multiple of 32) is loaded into LDS once and stays; the workgroup then walks (image, 64-channel tile)
// items, prefetching the next x tile into registers while the MFMAs of the current one run.  X^T is the A operand and W
// the B operand, so a lane ends with 4 CONSECUTIVE channels of one output row: bias, residual, the pre-activation and
// act(pre-activation) leave in 8-byte accesses from the accumulators -- the token MLP needs no bias / activation pass
// and the block's shortcut no add pass.
//
// Filter gradient: both operands have the reduction index (c) contiguous, so the fragments are plain 16-byte global
// loads.  The reduction (B * C long for an M x K output) is split over blockIdx.y; every split STORES its partial tile
// into its own slab of a scratch and a second kernel adds the slabs in split order: no float atomics, bit-identical
// from run to run in every mode.  dbias comes from one more MFMA against a tile of ones.
//
// The f32 dtype runs f32 FMA kernels with the same decomposition (exact f32 products, like every f32 kernel here).
#include "vt_common.h"

namespace {

constexpr int kMT = 64;        // output rows per workgroup
constexpr int kCT = 64;        // channels per item
constexpr int kKC = 128;       // reduction rows of x staged per step
constexpr int kXP = kCT + 8;   // pitch of the x tile (elements): 144-byte rows
constexpr int kWPad = 8;       // pad of a W row in LDS (elements)

__device__ __forceinline__ float tok_act(int code, float u) {
    return code == 4 ? 0.5f * u * (1.f + erff(u * 0.70710678118654752f)) : u;
}

struct TokArgs {
    const void* x;
    const void* w;
    const float* bias;
    const void* r;
    void* z;
    void* a;
    int ldx, ldw, ldr, ldz, lda, transw, act;
    int B, K, M, C;
    int ctiles, items, kpad, wp, nch;
};

__global__ void __launch_bounds__(256) tok_fwd_bf16_kernel(const TokArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* Ws = (bf16_t*)smem;       // [kMT][wp]
    bf16_t* Xs = Ws + kMT * p.wp;     // [kKC][kXP]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wc = wave & 1;
    const int g = lane >> 4, u = lane & 15, q = u >> 2, pp = u & 3;
    const int m0 = blockIdx.y * kMT;
    const int K = p.K, M = p.M, C = p.C, kp = p.kpad, wp = p.wp;
    const bf16_t* __restrict__ W = (const bf16_t*)p.w;
    const bf16_t* __restrict__ X = (const bf16_t*)p.x;
    const bf16_t zero = (bf16_t)0.f;

    // ---- the workgroup's slice of W, zero padded: Ws[r][k] = A[m0 + r][k] ----------------------------------
    if (!p.transw) {
        if ((p.ldw & 3) == 0 && (((uintptr_t)W) & 7) == 0) {  // 8-byte pieces of a row
            const int k4 = kp >> 2;
            for (int e = tid; e < kMT * k4; e += 256) {
                const int r = e / k4, k = (e - r * k4) << 2, m = m0 + r;
                uint2 v = make_uint2(0u, 0u);
                if (m < M && k < K) {  // (K tail inside a piece: masked below)
                    const bf16_t* src = W + (long)m * p.ldw + k;
                    if (k + 4 <= K) {
                        v = *(const uint2*)src;
                    } else {
                        unsigned short t[4] = {0, 0, 0, 0};
                        for (int j = 0; j < 4; ++j)
                            if (k + j < K) t[j] = __builtin_bit_cast(unsigned short, src[j]);
                        v = make_uint2((unsigned)t[0] | ((unsigned)t[1] << 16), (unsigned)t[2] | ((unsigned)t[3] << 16));
                    }
                }
                *(uint2*)(Ws + r * wp + k) = v;
            }
        } else {
            for (int e = tid; e < kMT * kp; e += 256) {
                const int r = e / kp, k = e - r * kp, m = m0 + r;
                Ws[r * wp + k] = (m < M && k < K) ? W[(long)m * p.ldw + k] : zero;
            }
        }
    } else {
        for (int e = tid; e < kMT * kp; e += 256) {  // r fastest: coalesced reads of W's rows
            const int k = e / kMT, r = e - k * kMT, m = m0 + r;
            Ws[r * wp + k] = (m < M && k < K) ? W[(long)k * p.ldw + m] : zero;
        }
    }

    const int nch = p.nch;
    const int my_items = (p.items - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int nsteps = my_items * nch;
    const int frow = tid >> 3, fch = (tid & 7) * 8;  // this thread's 16-byte pieces: rows frow + 32 i, channels fch..fch+7
    uint4 pre[4];

    auto fetch = [&](int s) {
        const int it = (int)blockIdx.x + (s / nch) * (int)gridDim.x, kc = s % nch;
        const int b = it / p.ctiles, ct = it - b * p.ctiles;
        const int c = ct * kCT + fch;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kc * kKC + frow + 32 * i;
            pre[i] = (k < K && c < C) ? *(const uint4*)(X + ((long)b * K + k) * p.ldx + c) : make_uint4(0u, 0u, 0u, 0u);
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nsteps > 0) fetch(0);
    for (int s = 0; s < nsteps; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *(uint4*)(Xs + (frow + 32 * i) * kXP + fch) = pre[i];
        __syncthreads();  // (the first one also publishes Ws)
        if (s + 1 < nsteps) fetch(s + 1);
        const int kc = s % nch, kbase = kc * kKC;
        const int klen = min(kKC, kp - kbase);  // a multiple of 32, uniform over the workgroup
        for (int kk = 0; kk < klen; kk += 32) {
            bf16x8 wf[2], xf[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) wf[j] = *(const bf16x8*)(Ws + (wm * 32 + j * 16 + u) * wp + kbase + kk + 8 * g);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                // rows kk + 8g + q (lo) and + 4 (hi): fragment element e <-> k = kk + 8g + e, as in the W fragment
                const bf16_t* a0 = Xs + (kk + 8 * g + q) * kXP + wc * 32 + i * 16 + 4 * pp;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * kXP));
                xf[i] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[i], wf[j], acc[i][j], 0, 0, 0);
        }
        if (kc == nch - 1) {
            // D[row = channel 4g + r][col = output row u]
            const int it = (int)blockIdx.x + (s / nch) * (int)gridDim.x;
            const int b = it / p.ctiles, ct = it - b * p.ctiles;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int m = m0 + wm * 32 + j * 16 + u;
                const float bv = (p.bias && m < M) ? p.bias[m] : 0.f;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int c = ct * kCT + wc * 32 + i * 16 + 4 * g;
                    if (m < M && c < C) {
                        const long row = (long)b * M + m;
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + bv;
                        if (p.r) {
                            const uint2 rr = *(const uint2*)((const bf16_t*)p.r + row * p.ldr + c);
                            v[0] += __uint_as_float(rr.x << 16);
                            v[1] += __uint_as_float(rr.x & 0xffff0000u);
                            v[2] += __uint_as_float(rr.y << 16);
                            v[3] += __uint_as_float(rr.y & 0xffff0000u);
                        }
                        const uint2 zz = make_uint2(VecIO<bf16_t>::pack2(v[0], v[1]), VecIO<bf16_t>::pack2(v[2], v[3]));
                        if (p.z) *(uint2*)((bf16_t*)p.z + row * p.ldz + c) = zz;
                        if (p.a) {  // the activation of the STORED pre-activation (what backward differentiates)
                            const float a0 = tok_act(p.act, __uint_as_float(zz.x << 16));
                            const float a1 = tok_act(p.act, __uint_as_float(zz.x & 0xffff0000u));
                            const float a2 = tok_act(p.act, __uint_as_float(zz.y << 16));
                            const float a3 = tok_act(p.act, __uint_as_float(zz.y & 0xffff0000u));
                            *(uint2*)((bf16_t*)p.a + row * p.lda + c) =
                                make_uint2(VecIO<bf16_t>::pack2(a0, a1), VecIO<bf16_t>::pack2(a2, a3));
                        }
                    }
                    acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
        __syncthreads();  // the tile is dead: the next step overwrites it
    }
}

// f32: 64 x 64 output tile per workgroup, 4 x 4 per thread, f32 FMA in k order
__global__ void __launch_bounds__(256) tok_fwd_f32_kernel(const TokArgs p) {
    __shared__ __attribute__((aligned(16))) float Ws[16][kMT + 4];
    __shared__ __attribute__((aligned(16))) float Xs[16][kCT];
    const int tid = threadIdx.x, tm = tid >> 4, tc = tid & 15;
    const int it = blockIdx.x, b = it / p.ctiles, ct = it - b * p.ctiles;
    const int m0 = blockIdx.y * kMT;
    const int K = p.K, M = p.M, C = p.C;
    const float* __restrict__ W = (const float*)p.w;
    const float* __restrict__ X = (const float*)p.x;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            int r, k;
            if (!p.transw) {
                r = e >> 4, k = e & 15;
            } else {
                k = e >> 6, r = e & 63;
            }
            const int m = m0 + r, kk = k0 + k;
            float v = 0.f;
            if (m < M && kk < K) v = p.transw ? W[(long)kk * p.ldw + m] : W[(long)m * p.ldw + kk];
            Ws[k][r] = v;
        }
        {
            const int row = tid >> 4, c = ct * kCT + tc * 4, k = k0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < K && c < C) v = *(const float4*)(X + ((long)b * K + k) * p.ldx + c);
            *(float4*)&Xs[row][tc * 4] = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4 a = *(const float4*)&Ws[k][tm * 4];
            const float4 x = *(const float4*)&Xs[k][tc * 4];
            const float av[4] = {a.x, a.y, a.z, a.w}, xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], xv[j], acc[i][j]);
        }
        __syncthreads();
    }
    const int c = ct * kCT + tc * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + tm * 4 + i;
        if (m < M && c < C) {
            const long row = (long)b * M + m;
            const float bv = p.bias ? p.bias[m] : 0.f;
            float4 v = make_float4(acc[i][0] + bv, acc[i][1] + bv, acc[i][2] + bv, acc[i][3] + bv);
            if (p.r) {
                const float4 rr = *(const float4*)((const float*)p.r + row * p.ldr + c);
                v.x += rr.x, v.y += rr.y, v.z += rr.z, v.w += rr.w;
            }
            if (p.z) *(float4*)((float*)p.z + row * p.ldz + c) = v;
            if (p.a)
                *(float4*)((float*)p.a + row * p.lda + c) =
                    make_float4(tok_act(p.act, v.x), tok_act(p.act, v.y), tok_act(p.act, v.z), tok_act(p.act, v.w));
        }
    }
}

// ---- filter gradient ------------------------------------------------------------------------------------------
struct TokWgArgs {
    const void* dz;
    const void* x;
    float* slab;
    long slab_stride;  // floats per split: M * K + M
    int lddz, ldx, B, K, M, C;
    int kt, csteps, total, per;
};

__global__ void __launch_bounds__(256) tok_wgrad_bf16_kernel(const TokWgArgs p) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wk = wave & 1;
    const int g = lane >> 4, u = lane & 15;
    const int tmi = blockIdx.x / p.kt, tki = blockIdx.x - tmi * p.kt;
    const int m0 = tmi * 64 + wm * 32, k0 = tki * 64 + wk * 32;
    const int K = p.K, M = p.M, C = p.C;
    const bf16_t* __restrict__ DZ = (const bf16_t*)p.dz;
    const bf16_t* __restrict__ X = (const bf16_t*)p.x;
    const int s0 = blockIdx.y * p.per, s1 = min(p.total, s0 + p.per);
    const bool do_bias = tki == 0 && wk == 0;
    const unsigned one2 = 0x3F803F80u;
    const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(one2, one2, one2, one2));
    const bf16x8 zero8 = __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
    f32x4 acc[2][2], accb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int st = s0; st < s1; ++st) {
        const int b = st / p.csteps, cc = (st - b * p.csteps) * 32 + 8 * g;
        const bool cv = cc < C;
        bf16x8 af[2], bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + i * 16 + u;
            af[i] = (cv && m < M) ? *(const bf16x8*)(DZ + ((long)b * M + m) * p.lddz + cc) : zero8;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + j * 16 + u;
            bf[j] = (cv && k < K) ? *(const bf16x8*)(X + ((long)b * K + k) * p.ldx + cc) : zero8;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        if (do_bias) {
#pragma unroll
            for (int i = 0; i < 2; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], ones, accb[i], 0, 0, 0);
        }
    }
    float* slab = p.slab + (long)blockIdx.y * p.slab_stride;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + i * 16 + 4 * g + r;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = k0 + j * 16 + u;
                if (k < K) slab[(long)m * K + k] = acc[i][j][r];
            }
            if (do_bias && u == 0) slab[(long)M * K + m] = accb[i][r];
        }
}

__global__ void __launch_bounds__(256) tok_wgrad_f32_kernel(const TokWgArgs p) {
    __shared__ __attribute__((aligned(16))) float As[16][68];
    __shared__ __attribute__((aligned(16))) float Bs[16][68];
    const int tid = threadIdx.x, tm = tid >> 4, tk = tid & 15;
    const int tmi = blockIdx.x / p.kt, tki = blockIdx.x - tmi * p.kt;
    const int m0 = tmi * 64, k0 = tki * 64;
    const int K = p.K, M = p.M, C = p.C;
    const float* __restrict__ DZ = (const float*)p.dz;
    const float* __restrict__ X = (const float*)p.x;
    const int s0 = blockIdx.y * p.per, s1 = min(p.total, s0 + p.per);
    const bool do_bias = tki == 0 && tk == 0;
    float acc[4][4], accb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    const int row = tid >> 2, c4 = (tid & 3) * 4;
    for (int st = s0; st < s1; ++st) {
        const int b = st / p.csteps, c = (st - b * p.csteps) * 16 + c4;
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
        if (c < C && m0 + row < M) va = *(const float4*)(DZ + ((long)b * M + m0 + row) * p.lddz + c);
        if (c < C && k0 + row < K) vb = *(const float4*)(X + ((long)b * K + k0 + row) * p.ldx + c);
        As[c4 + 0][row] = va.x, As[c4 + 1][row] = va.y, As[c4 + 2][row] = va.z, As[c4 + 3][row] = va.w;
        Bs[c4 + 0][row] = vb.x, Bs[c4 + 1][row] = vb.y, Bs[c4 + 2][row] = vb.z, Bs[c4 + 3][row] = vb.w;
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
            const float4 a = *(const float4*)&As[cc][tm * 4];
            const float4 x = *(const float4*)&Bs[cc][tk * 4];
            const float av[4] = {a.x, a.y, a.z, a.w}, xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                accb[i] += av[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], xv[j], acc[i][j]);
            }
        }
        __syncthreads();
    }
    float* slab = p.slab + (long)blockIdx.y * p.slab_stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + tm * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + tk * 4 + j;
            if (k < K) slab[(long)m * K + k] = acc[i][j];
        }
        if (do_bias) slab[(long)M * K + m] = accb[i];
    }
}

// dW / dbias += the slabs, in split order
__global__ void __launch_bounds__(256) tok_wgrad_reduce_kernel(const float* __restrict__ slab, int S, long stride, long nw, int M,
                                                               float* __restrict__ dw, float* __restrict__ dbias) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nw + M) return;
    if (idx < nw ? dw == nullptr : dbias == nullptr) return;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += slab[(long)i * stride + idx];
    if (idx < nw)
        dw[idx] += s;
    else
        dbias[idx - nw] += s;
}

// ---- patch gather / scatter --------------------------------------------------------------------------------------
// out[b][gy][gx][(py * p + px) * Cin + c] = img[b][gy * p + py][gx * p + px][c]: the row order of the channels_last
// filter image [d_model][p][p][Cin], so the patch embedding is a Linear over these rows with the filter as it lies.
template <typename T>
__global__ void __launch_bounds__(256) patchify_fwd_kernel(const T* __restrict__ img, int ldi, T* __restrict__ out, int ldo,
                                                           long npix, int H, int W, int Cin, int p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= npix) return;
    const int x = (int)(idx % W);
    const long t = idx / W;
    const int y = (int)(t % H);
    const long b = t / H;
    const int gy = y / p, py = y - gy * p, gx = x / p, px = x - gx * p;
    const int gh = H / p, gw = W / p;
    const T* src = img + idx * ldi;
    T* dst = out + ((b * gh + gy) * gw + gx) * ldo + (py * p + px) * Cin;
    for (int c = 0; c < Cin; ++c) dst[c] = src[c];
}

// dimg[b][y][x][c] = dout[patch row] for c < Cin, 0 for the pad channels (+ residual)
template <typename T>
__global__ void __launch_bounds__(256) patchify_bwd_kernel(const T* __restrict__ dout, int lddo, T* dimg, int ldg, const T* res,
                                                           int ldr, long npix, int H, int W, int Cin, int Cpad, int p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= npix) return;
    const int x = (int)(idx % W);
    const long t = idx / W;
    const int y = (int)(t % H);
    const long b = t / H;
    const int gy = y / p, py = y - gy * p, gx = x / p, px = x - gx * p;
    const int gh = H / p, gw = W / p;
    const T* src = dout + ((b * gh + gy) * gw + gx) * lddo + (py * p + px) * Cin;
    T* dst = dimg + idx * ldg;
    for (int c = 0; c < Cpad; ++c) {
        float v = c < Cin ? (float)src[c] : 0.f;
        if (res) v += (float)res[idx * ldr + c];
        dst[c] = from_float<T>(v);
    }
}

int check_map(const char* who, const char* what, const void* ptr, int ld, int C, int dtype) {
    VT_REQUIRE(ptr && vt_aligned16(ptr) && ld >= C && ld % vt_epc(dtype) == 0, VT_ERR_INVALID,
               "%s: %s null, not 16-byte aligned, or its row stride %d is below C = %d / no multiple of a 16-byte chunk", who, what,
               ld, C);
    return VT_OK;
}

// splits of the filter gradient's reduction: ~512 workgroups per launch, at most 64 slabs, at least one step each
int wgrad_splits(int tiles, int total) {
    int s = (512 + tiles - 1) / tiles;
    if (s > 64) s = 64;
    if (s > total) s = total;
    return s < 1 ? 1 : s;
}

}  // namespace

extern "C" {

int vt_token_mix_fwd(const void* x, int32_t ldx, const void* w, int32_t ldw, int32_t transw, const float* bias,
                     const void* residual, int32_t ldr, void* z, int32_t ldz, void* a, int32_t lda, int32_t act, int32_t B,
                     int32_t K, int32_t M, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_token_mix_fwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && K > 0 && M > 0 && C > 0 && C % vt_epc(dtype) == 0, VT_ERR_INVALID,
               "%s: B=%d K=%d M=%d C=%d (C must be a multiple of %d)", who, B, K, M, C, vt_epc(dtype));
    VT_REQUIRE(act == 0 || act == 4, VT_ERR_UNSUPPORTED, "%s: activation code %d (0 none, 4 exact GELU)", who, act);
    VT_REQUIRE(w && ldw >= (transw ? M : K), VT_ERR_INVALID, "%s: w null or ldw=%d below its row length", who, ldw);
    VT_REQUIRE(z || a, VT_ERR_INVALID, "%s: no output", who);
    VT_REQUIRE((long)B * (K > M ? K : M) < 0x7fffffffL / 2, VT_ERR_UNSUPPORTED, "%s: B * tokens too large", who);
    VT_TRY(check_map(who, "x", x, ldx, C, dtype));
    if (residual) VT_TRY(check_map(who, "residual", residual, ldr, C, dtype));
    if (z) VT_TRY(check_map(who, "z", z, ldz, C, dtype));
    if (a) VT_TRY(check_map(who, "a", a, lda, C, dtype));
    TokArgs p;
    p.x = x, p.w = w, p.bias = bias, p.r = residual, p.z = z, p.a = a;
    p.ldx = ldx, p.ldw = ldw, p.ldr = ldr, p.ldz = ldz, p.lda = lda, p.transw = transw, p.act = act;
    p.B = B, p.K = K, p.M = M, p.C = C;
    p.ctiles = (C + kCT - 1) / kCT;
    VT_REQUIRE((long)B * p.ctiles < 0x7fffffffL, VT_ERR_UNSUPPORTED, "%s: too many items", who);
    p.items = B * p.ctiles;
    p.kpad = (K + 31) / 32 * 32;
    p.wp = p.kpad + kWPad;
    p.nch = (K + kKC - 1) / kKC;
    const int mtiles = (M + kMT - 1) / kMT;
    if (dtype == VT_F32) {
        hipLaunchKernelGGL(tok_fwd_f32_kernel, dim3((unsigned)p.items, (unsigned)mtiles), dim3(256), 0, (hipStream_t)stream, p);
        VT_CHECK_LAUNCH(who);
        return VT_OK;
    }
    const int smem = (kMT * p.wp + kKC * kXP) * 2;
    VT_REQUIRE(smem <= 160 * 1024, VT_ERR_UNSUPPORTED,
               "%s: a 64-row slice of W over K = %d tokens (%d bytes with the x tile) exceeds the 160 KiB of LDS", who, K, smem);
    if (smem > 64 * 1024) VT_TRY(vt_raise_dynamic_lds((const void*)tok_fwd_bf16_kernel, smem, who));
    int per_cu = (160 * 1024) / smem;
    if (per_cu > 4) per_cu = 4;
    long gx = (long)per_cu * vt_device_cus() / mtiles;
    if (gx < 1) gx = 1;
    if (gx > p.items) gx = p.items;
    hipLaunchKernelGGL(tok_fwd_bf16_kernel, dim3((unsigned)gx, (unsigned)mtiles), dim3(256), smem, (hipStream_t)stream, p);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int64_t vt_token_mix_wgrad_scratch_bytes(int32_t B, int32_t K, int32_t M, int32_t C, int32_t dtype) {
    if (B <= 0 || K <= 0 || M <= 0 || C <= 0) return 0;
    const int tiles = ((M + 63) / 64) * ((K + 63) / 64);
    const int csteps = (C + (dtype == VT_BF16 ? 32 : 16) - 1) / (dtype == VT_BF16 ? 32 : 16);
    const long total = (long)B * csteps;
    const int S = wgrad_splits(tiles, total > 0x7fffffffL ? 0x7fffffff : (int)total);
    return (int64_t)S * ((int64_t)M * K + M) * 4;
}

int vt_token_mix_wgrad(const void* dz, int32_t lddz, const void* x, int32_t ldx, float* dw, float* dbias, void* scratch,
                       int64_t scratch_bytes, int32_t B, int32_t K, int32_t M, int32_t C, int32_t dtype, void* stream) {
    const char* who = "vt_token_mix_wgrad";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && K > 0 && M > 0 && C > 0 && C % vt_epc(dtype) == 0, VT_ERR_INVALID,
               "%s: B=%d K=%d M=%d C=%d (C must be a multiple of %d)", who, B, K, M, C, vt_epc(dtype));
    VT_REQUIRE(dw || dbias, VT_ERR_INVALID, "%s: no output", who);
    VT_TRY(check_map(who, "dz", dz, lddz, C, dtype));
    VT_TRY(check_map(who, "x", x, ldx, C, dtype));
    TokWgArgs p;
    p.dz = dz, p.x = x, p.slab = (float*)scratch;
    p.slab_stride = (long)M * K + M;
    p.lddz = lddz, p.ldx = ldx, p.B = B, p.K = K, p.M = M, p.C = C;
    p.kt = (K + 63) / 64;
    const int tiles = ((M + 63) / 64) * p.kt;
    const int cstep = dtype == VT_BF16 ? 32 : 16;
    p.csteps = (C + cstep - 1) / cstep;
    VT_REQUIRE((long)B * p.csteps < 0x7fffffffL, VT_ERR_UNSUPPORTED, "%s: reduction too long", who);
    p.total = B * p.csteps;
    int S = wgrad_splits(tiles, p.total);
    const int64_t fit = scratch_bytes / (p.slab_stride * 4);  // a smaller scratch: fewer, longer splits
    if (S > fit) S = (int)fit;
    VT_REQUIRE(scratch && vt_aligned16(scratch) && S >= 1, VT_ERR_INVALID,
               "%s: scratch null, misaligned or below one slab (%ld bytes)", who, (long)p.slab_stride * 4);
    p.per = (p.total + S - 1) / S;
    S = (p.total + p.per - 1) / p.per;
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(tok_wgrad_bf16_kernel, dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(tok_wgrad_f32_kernel, dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, (hipStream_t)stream, p);
    VT_CHECK_LAUNCH(who);
    const long n = p.slab_stride;
    hipLaunchKernelGGL(tok_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)scratch, S, p.slab_stride, (long)M * K, M, dw, dbias);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_patchify_fwd(const void* img, int32_t ldi, void* out, int32_t ldo, int32_t B, int32_t H, int32_t W, int32_t Cin,
                    int32_t p, int32_t dtype, void* stream) {
    const char* who = "vt_patchify_fwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(img && out && B > 0 && Cin > 0 && p > 0 && H > 0 && W > 0 && H % p == 0 && W % p == 0 && ldi >= Cin &&
                   ldo >= Cin * p * p,
               VT_ERR_INVALID, "%s: B=%d H=%d W=%d Cin=%d p=%d ldi=%d ldo=%d", who, B, H, W, Cin, p, ldi, ldo);
    const long npix = (long)B * H * W;
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(patchify_fwd_kernel<bf16_t>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)img, ldi, (bf16_t*)out, ldo, npix, H, W, Cin, p);
    else
        hipLaunchKernelGGL(patchify_fwd_kernel<float>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)img, ldi, (float*)out, ldo, npix, H, W, Cin, p);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_patchify_bwd(const void* dout, int32_t lddo, void* dimg, int32_t ldg, const void* residual, int32_t ldr, int32_t B,
                    int32_t H, int32_t W, int32_t Cin, int32_t Cpad, int32_t p, int32_t dtype, void* stream) {
    const char* who = "vt_patchify_bwd";
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_INVALID, "%s: dtype %d", who, dtype);
    VT_REQUIRE(dout && dimg && B > 0 && Cin > 0 && Cpad >= Cin && p > 0 && H > 0 && W > 0 && H % p == 0 && W % p == 0 &&
                   ldg >= Cpad && lddo >= Cin * p * p && (!residual || ldr >= Cpad),
               VT_ERR_INVALID, "%s: B=%d H=%d W=%d Cin=%d Cpad=%d p=%d lddo=%d ldg=%d ldr=%d", who, B, H, W, Cin, Cpad, p, lddo,
               ldg, ldr);
    const long npix = (long)B * H * W;
    if (dtype == VT_BF16)
        hipLaunchKernelGGL(patchify_bwd_kernel<bf16_t>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)dout, lddo, (bf16_t*)dimg, ldg, (const bf16_t*)residual, ldr, npix, H, W, Cin, Cpad, p);
    else
        hipLaunchKernelGGL(patchify_bwd_kernel<float>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)dout, lddo, (float*)dimg, ldg, (const float*)residual, ldr, npix, H, W, Cin, Cpad, p);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // extern "C"
