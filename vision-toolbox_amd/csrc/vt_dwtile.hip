// vt_dwtile.hip -- tiled depthwise convolution for the Conv-BN-act units of the MobileNets (backbones/mobilenet.py):
// k in {3, 5}, stride in {1, 2}, padding (k - 1) / 2, dilation 1.  Forward with batch statistics, and a backward that forms
// the data gradient and the filter gradient from ONE staging of dz and x, without a float atomic.
//
// vt_dwconv.hip re-reads every tap through the caches and adds its filter gradient with f32 atomics into one [C][k*k] image
// that every workgroup hits (README: 252 of 296.8 ms of a ConvNeXt-T backward).  Here a workgroup owns
//     (image b, band of R output rows [i0, i0 + R), slab of SC 16-byte channel chunks)
// and stages what it needs in LDS once, zero-filled outside the image:
//     x tile   rows [i0*s - pad, (i0 + R - 1)*s - pad + k), columns [-pad, Wi + pad)
//     dz tile  (backward) the rows the band's INPUT rows [i0*s, (i0 + R)*s) reach, ceil((i0*s + pad - k + 1) / s) ..
//              ((i0 + R)*s - 1 + pad) / s, columns [-pad, Wo + pad)
// A thread owns one chunk (8 bf16 / 4 f32 channels) of a pixel: lanes run along the slab's chunks, then along pixels, so a
// wave reads consecutive 16-byte pieces of LDS and of a pixel row in memory.
//   forward   f32 accumulation from 0 in ascending tap order (kr, kc) with fmaf over ALL k*k taps: a zero halo adds exact
//             zeros, so z is bit-identical to vt_dwconv_fwd's, which skips those taps.  Statistics of the STORED z: the
//             threads of a slab chunk fold through LDS in a fixed order, then one vt_stat_add per channel and workgroup.
//   backward  dx for the band's input rows (every input pixel once; per-tap parity test under stride 2; + residual, which
//             may alias dx, the sum rounded to the storage type first).  Then the filter-gradient share of the band: a thread
//             owns (tap, chunk) -- and, where 256 threads allow, one of G pixel ranges -- and walks the band's output pixels
//             with its accumulators in registers; the G ranges fold through LDS in range order; the share [k*k][slab
//             channels] goes to shares[b][band][tap][c].  Nothing is handed from one workgroup to another.
//   reduce    a second launch, one owner per dw[c][t]: adds the shares in (image, band) order -- eight contiguous runs of
//             that order, then the runs in order -- and does dw += sum.
// The tile: SC starts at min(C / epc, 8) and R is the tallest band (<= 8 rows) whose two tiles fit 48 KiB; where fewer than
// 4 (stride 1) / 2 (stride 2) rows fit even in 64 KiB, SC is halved.  At most 64 KiB of LDS per workgroup, so two or more
// share a CU.  Forward and backward use the same tile (vt_dwt_tile).
#include "vt_common.h"

namespace {

constexpr int kT = 256;
constexpr int kLdsMax = 64 * 1024, kLdsAim = 48 * 1024;

struct DwtArgs {
    const void* x;
    const float* w;
    void* z;        // forward: z (written); backward: dz (read)
    float* stats;
    void* dx;
    const void* res;
    float* shares;
    int B, Hi, Wi, Ho, Wo, C, CPR, pad;
    int ldx, ldz, lddx, ldr;
    int R, SC, NB, NS, NX, NZ, WTX, WTZ;
    int lds;
};

__device__ __forceinline__ int floordiv(int n, int d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }

// rows [r0, r0 + nrows) x columns [c0, c0 + WT) of one image's [H][W] map (pixel stride ld) -> tile[row][col][SC], zeros
// outside the map; thread (tp, tc) of PT x SC
template <typename T>
__device__ __forceinline__ void stage(uint4* tile, const T* img, int ld, int H, int W, int r0, int c0, int nrows, int WT, int SC,
                                      int ch, int tc, int tp, int PT) {
    int r = tp / WT, c = tp - r * WT;
    const int dr = PT / WT, dc = PT - dr * WT;
    while (r < nrows) {
        const int h = r0 + r, w_ = c0 + c;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (h >= 0 && h < H && w_ >= 0 && w_ < W) v = *(const uint4*)(img + ((long)h * W + w_) * ld + ch);
        tile[(r * WT + c) * SC + tc] = v;
        r += dr, c += dc;
        if (c >= WT) c -= WT, ++r;
    }
}

// The filter of a thread's chunk, rounded as vt_dwconv_fwd's load_w rounds it.  k = 3: nine taps in registers.  k = 5: 25 taps
// of 8 channels are 200 registers, so the slab's taps live in LDS as f32 [k*k][SC][EPC] behind the tiles and a tap is read
// where it is used (the lanes of a chunk read one address).
template <typename T, int K>
struct Filter {
    static constexpr int EPC = VecIO<T>::EPC, KK = K * K, NREG = K == 3 ? KK : 1;
    float reg[NREG][EPC];
    const float* lds;
    __device__ __forceinline__ void load(const float* w, int ch, float* wl, int SC, int tc, int tp, bool live) {
        if constexpr (K == 3) {
            if (live) {
#pragma unroll
                for (int t = 0; t < KK; ++t)
#pragma unroll
                    for (int e = 0; e < EPC; ++e) reg[t][e] = VecIO<T>::round(w[(long)(ch + e) * KK + t]);
            }
        } else {
            if (live && tp < KK) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) wl[(tp * SC + tc) * EPC + e] = VecIO<T>::round(w[(long)(ch + e) * KK + tp]);
            }
            lds = wl + tc * EPC;
            stride = SC * EPC;
        }
    }
    int stride;
    __device__ __forceinline__ void tap(int t, float (&wv)[EPC]) const {
        if constexpr (K == 3) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) wv[e] = reg[t][e];
        } else {
#pragma unroll
            for (int e = 0; e < EPC; e += 4) {
                const float4 v = *(const float4*)(lds + t * stride + e);
                wv[e] = v.x, wv[e + 1] = v.y, wv[e + 2] = v.z, wv[e + 3] = v.w;
            }
        }
    }
};

struct Own {
    int b, band, slab, chunk0, nsc, i0, Rb;
};
__device__ __forceinline__ Own owner(const DwtArgs& a) {
    Own o;
    unsigned id = blockIdx.x;
    o.slab = (int)(id % (unsigned)a.NS);
    id /= (unsigned)a.NS;
    o.band = (int)(id % (unsigned)a.NB);
    o.b = (int)(id / (unsigned)a.NB);
    o.chunk0 = o.slab * a.SC;
    o.nsc = min(a.SC, a.CPR - o.chunk0);
    o.i0 = o.band * a.R;
    o.Rb = min(a.R, a.Ho - o.i0);
    return o;
}

template <typename T, int K, int S, bool STATS>
__global__ void __launch_bounds__(kT, K == 3 ? 2 : 3) dwt_fwd_kernel(const DwtArgs a) {
    constexpr int EPC = VecIO<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4* xt = (uint4*)smem;
    const int t = threadIdx.x, SC = a.SC, PT = kT / SC;
    const int tc = t % SC, tp = t / SC;
    const Own o = owner(a);
    const bool live = tp < PT && tc < o.nsc;
    const int ch = (o.chunk0 + tc) * EPC;
    Filter<T, K> f;
    if (live)
        stage<T>(xt, (const T*)a.x + (long)o.b * a.Hi * a.Wi * a.ldx, a.ldx, a.Hi, a.Wi, o.i0 * S - a.pad, -a.pad,
                 (o.Rb - 1) * S + K, a.WTX, SC, ch, tc, tp, PT);
    f.load(a.w, ch, (float*)(xt + a.NX * a.WTX * SC), SC, tc, tp, live);
    __syncthreads();
    float s1[EPC], s2[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = 0.f;
    if (live) {
        T* z = (T*)a.z + ((long)o.b * a.Ho + o.i0) * a.Wo * a.ldz + ch;
        const int n = o.Rb * a.Wo;
        int i = tp / a.Wo, j = tp - i * a.Wo;
        const int di = PT / a.Wo, dj = PT - di * a.Wo;
        for (int p = tp; p < n; p += PT) {
            if constexpr (K == 5) asm volatile("" ::: "memory");  // (the taps are re-read per pixel, not hoisted into 200 registers)
            float acc[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
            const uint4* src = xt + ((i * S) * a.WTX + j * S) * SC + tc;
#pragma unroll
            for (int kr = 0; kr < K; ++kr)
#pragma unroll
                for (int kc = 0; kc < K; ++kc) {
                    float xv[EPC], wv[EPC];
                    VecIO<T>::unpack(src[(kr * a.WTX + kc) * SC], xv);
                    f.tap(kr * K + kc, wv);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[e] = fmaf(xv[e], wv[e], acc[e]);
                }
            const uint4 out = VecIO<T>::pack(acc);
            *(uint4*)(z + (long)p * a.ldz) = out;
            if (STATS) {
                float rv[EPC];
                VecIO<T>::unpack(out, rv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) s1[e] += rv[e], s2[e] = fmaf(rv[e], rv[e], s2[e]);
            }
            i += di, j += dj;
            if (j >= a.Wo) j -= a.Wo, ++i;
        }
    }
    if (STATS) {
        // red[t][2 EPC] -> columns (chunk, value) folded over the pixel lanes by `parts` threads each, then by one
        __syncthreads();  // (the tile is dead)
        float* red = (float*)smem;
        float* red2 = red + kT * 2 * EPC;
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[t * 2 * EPC + e] = s1[e], red[t * 2 * EPC + EPC + e] = s2[e];
        __syncthreads();
        const int ncol = SC * 2 * EPC, parts = kT / ncol;
        const int col = t % ncol, part = t / ncol;
        if (part < parts) {
            float s = 0.f;
            for (int q = part; q < PT; q += parts) s += red[q * ncol + col];
            red2[part * ncol + col] = s;
        }
        __syncthreads();
        if (t < ncol && t / (2 * EPC) < o.nsc) {
            float s = 0.f;
            for (int q = 0; q < parts; ++q) s += red2[q * ncol + t];
            const int which = (t % (2 * EPC)) / EPC, c = (o.chunk0 + t / (2 * EPC)) * EPC + t % EPC;
            vt_stat_add(a.stats, ((long)(blockIdx.x % kStatReplicas) * 2 + which) * a.C + c, s);
        }
    }
}

template <typename T, int K, int S>
__global__ void __launch_bounds__(kT, K == 3 ? 2 : 4) dwt_bwd_kernel(const DwtArgs a) {
    constexpr int EPC = VecIO<T>::EPC, KK = K * K;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4* xt = (uint4*)smem;
    uint4* zt = xt + a.NX * a.WTX * a.SC;
    const int t = threadIdx.x, SC = a.SC, PT = kT / SC;
    const int tc = t % SC, tp = t / SC;
    const Own o = owner(a);
    const bool live = tp < PT && tc < o.nsc;
    const int ch = (o.chunk0 + tc) * EPC;
    const int h0 = o.i0 * S, h1 = o.band == a.NB - 1 ? a.Hi : (o.i0 + a.R) * S;  // the band's input rows
    const int zlo = floordiv(h0 + a.pad - (K - 1) + (S - 1), S), zhi = (h1 - 1 + a.pad) / S;
    Filter<T, K> f;
    f.load(a.w, ch, (float*)(zt + a.NZ * a.WTZ * SC), SC, tc, tp, live);
    if (live) {
        stage<T>(xt, (const T*)a.x + (long)o.b * a.Hi * a.Wi * a.ldx, a.ldx, a.Hi, a.Wi, h0 - a.pad, -a.pad, (o.Rb - 1) * S + K,
                 a.WTX, SC, ch, tc, tp, PT);
        stage<T>(zt, (const T*)a.z + (long)o.b * a.Ho * a.Wo * a.ldz, a.ldz, a.Ho, a.Wo, zlo, -a.pad, zhi - zlo + 1, a.WTZ, SC, ch,
                 tc, tp, PT);
    }
    __syncthreads();
    if (live) {  // ---- dx over the band's input rows
        const long base = ((long)o.b * a.Hi + h0) * a.Wi;
        T* dx = (T*)a.dx + base * a.lddx + ch;
        const T* res = a.res ? (const T*)a.res + base * a.ldr + ch : nullptr;
        const int n = (h1 - h0) * a.Wi;
        int hl = tp / a.Wi, w_ = tp - hl * a.Wi;
        const int dh = PT / a.Wi, dw_ = PT - dh * a.Wi;
        for (int p = tp; p < n; p += PT) {
            if constexpr (K == 5) asm volatile("" ::: "memory");  // (the taps are re-read per pixel, not hoisted into 200 registers)
            float acc[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
#pragma unroll
            for (int kr = 0; kr < K; ++kr) {
                const int hn = h0 + hl + a.pad - kr;
                if (S == 2 && (hn & 1)) continue;
                const int zr = (S == 2 ? hn >> 1 : hn) - zlo;
#pragma unroll
                for (int kc = 0; kc < K; ++kc) {
                    const int wn = w_ + a.pad - kc;
                    if (S == 2 && (wn & 1)) continue;
                    const int zc = (S == 2 ? wn >> 1 : wn) + a.pad;
                    float gv[EPC], wv[EPC];
                    VecIO<T>::unpack(zt[(zr * a.WTZ + zc) * SC + tc], gv);
                    f.tap(kr * K + kc, wv);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[e] = fmaf(gv[e], wv[e], acc[e]);
                }
            }
            if (res) {
                // (the sum is rounded to the storage type first, as vt_dwconv_dgrad does)
                float rv[EPC], sv[EPC];
                VecIO<T>::unpack(VecIO<T>::pack(acc), sv);
                VecIO<T>::unpack(*(const uint4*)(res + (long)p * a.ldr), rv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] = sv[e] + rv[e];
            }
            *(uint4*)(dx + (long)p * a.lddx) = VecIO<T>::pack(acc);
            hl += dh, w_ += dw_;
            if (w_ >= a.Wi) w_ -= a.Wi, ++hl;
        }
    }
    // ---- the band's filter-gradient share: thread = (pixel range g, tap, chunk)
    const int G = PT / KK, tap = tp % KK, g = tp / KK;
    const bool wlive = tc < o.nsc && g < G;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    if (wlive) {
        const int kr = tap / K, kc = tap - kr * K;
        const int n = o.Rb * a.Wo, per = (n + G - 1) / G;
        const int p0 = g * per, p1 = min(n, p0 + per);
        int i = p0 / a.Wo, j = p0 - i * a.Wo;
        for (int p = p0; p < p1; ++p) {
            float gv[EPC], xv[EPC];
            VecIO<T>::unpack(zt[((o.i0 + i - zlo) * a.WTZ + j + a.pad) * SC + tc], gv);
            VecIO<T>::unpack(xt[((i * S + kr) * a.WTX + j * S + kc) * SC + tc], xv);
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaf(gv[e], xv[e], acc[e]);
            if (++j == a.Wo) j = 0, ++i;
        }
    }
    __syncthreads();  // (the tiles are dead)
    float* red = (float*)smem;  // [G][KK][SC][EPC]
    if (wlive) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[((g * KK + tap) * SC + tc) * EPC + e] = acc[e];
    }
    __syncthreads();
    if (wlive && g == 0) {
        float s[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s[e] = 0.f;
        for (int q = 0; q < G; ++q)
#pragma unroll
            for (int e = 0; e < EPC; ++e) s[e] += red[((q * KK + tap) * SC + tc) * EPC + e];
        float* dst = a.shares + (((long)o.b * a.NB + o.band) * KK + tap) * a.C + ch;
#pragma unroll
        for (int e = 0; e < EPC; e += 4) *(float4*)(dst + e) = make_float4(s[e], s[e + 1], s[e + 2], s[e + 3]);
    }
}

// one owner per dw[c][tap]: 32 elements x 8 runs of the (image, band) order per workgroup
__global__ void __launch_bounds__(kT) dwt_wgrad_reduce_kernel(const float* __restrict__ shares, float* __restrict__ dw, int n,
                                                              int C, int KK) {
    __shared__ float red[8][32];
    const int col = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int total = KK * C, idx = blockIdx.x * 32 + col;  // idx = tap * C + c
    const int per = (n + 7) / 8, m0 = part * per, m1 = min(n, m0 + per);
    float s = 0.f;
    if (idx < total) {
        const float* p = shares + idx;
#pragma unroll 4
        for (int m = m0; m < m1; ++m) s += p[(long)m * total];
    }
    red[part][col] = s;
    __syncthreads();
    if (part == 0 && idx < total) {
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) v += red[q][col];
        const int tap = idx / C, c = idx - tap * C;
        dw[(long)c * KK + tap] += v;
    }
}

// the x tile, the dz tile and (k = 5) the slab's filter: the backward kernel's LDS; the forward kernel asks for the same
long tile_bytes(int R, int SC, int k, int s, int Wi, int Wo) {
    const int pad = (k - 1) / 2;
    return 16L * SC * ((long)((R - 1) * s + k) * (Wi + 2 * pad) + (long)(R + (k - 1) / s) * (Wo + 2 * pad)) +
           (k == 5 ? 25L * SC * 8 * (long)sizeof(float) : 0);
}

int fill(DwtArgs& a, const char* who, int dtype, int B, int Hi, int Wi, int C, int k, int s) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(k == 3 || k == 5, VT_ERR_UNSUPPORTED, "%s: k=%d (3 or 5)", who, k);
    VT_REQUIRE(s == 1 || s == 2, VT_ERR_UNSUPPORTED, "%s: s=%d (1 or 2)", who, s);
    VT_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && C > 0, VT_ERR_INVALID, "%s: bad geometry B=%d Hi=%d Wi=%d C=%d", who, B, Hi, Wi, C);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C % epc == 0, VT_ERR_UNSUPPORTED, "%s: C=%d must be a multiple of %d", who, C, epc);
    memset(&a, 0, sizeof(a));
    a.B = B, a.Hi = Hi, a.Wi = Wi, a.C = C, a.CPR = C / epc, a.pad = (k - 1) / 2;
    a.Ho = (Hi - 1) / s + 1, a.Wo = (Wi - 1) / s + 1;
    const int want = (s == 1 ? 4 : 2) < a.Ho ? (s == 1 ? 4 : 2) : a.Ho;
    int SC = a.CPR < 8 ? a.CPR : 8, R = 0;
    for (;; SC = (SC + 1) / 2) {
        const int cap = a.Ho < 8 ? a.Ho : 8;
        R = 0;
        while (R < cap && tile_bytes(R + 1, SC, k, s, Wi, a.Wo) <= (R < want ? kLdsMax : kLdsAim)) ++R;
        if (R >= want || SC == 1) break;
    }
    VT_REQUIRE(R >= 1, VT_ERR_UNSUPPORTED, "%s: Wi=%d: one output row with its halo (%ld bytes) exceeds 64 KiB of LDS", who, Wi,
               tile_bytes(1, 1, k, s, Wi, a.Wo));
    a.R = R, a.SC = SC, a.NB = (a.Ho + R - 1) / R, a.NS = (a.CPR + SC - 1) / SC;
    a.NX = (R - 1) * s + k, a.NZ = R + (k - 1) / s, a.WTX = Wi + 2 * a.pad, a.WTZ = a.Wo + 2 * a.pad;
    a.lds = (int)tile_bytes(R, SC, k, s, Wi, a.Wo);
    VT_REQUIRE((long)B * a.NB * a.NS < (1L << 31), VT_ERR_UNSUPPORTED, "%s: B=%d: too many workgroups", who, B);
    return VT_OK;
}

bool mat_ok(const void* p, int ld, int C, int epc) { return p && ld >= C && ld % epc == 0 && vt_aligned16(p); }

#define DWT_DISPATCH(dtype, k, s, ...)                                        \
    do {                                                                      \
        if ((dtype) == VT_BF16) {                                             \
            typedef bf16_t T;                                                 \
            DWT_DISPATCH_KS(k, s, __VA_ARGS__);                               \
        } else {                                                              \
            typedef float T;                                                  \
            DWT_DISPATCH_KS(k, s, __VA_ARGS__);                               \
        }                                                                     \
    } while (0)
#define DWT_DISPATCH_KS(k, s, ...)                                            \
    do {                                                                      \
        if ((k) == 3 && (s) == 1) {                                           \
            constexpr int K = 3, S = 1;                                       \
            __VA_ARGS__;                                                      \
        } else if ((k) == 3) {                                                \
            constexpr int K = 3, S = 2;                                       \
            __VA_ARGS__;                                                      \
        } else if ((s) == 1) {                                                \
            constexpr int K = 5, S = 1;                                       \
            __VA_ARGS__;                                                      \
        } else {                                                              \
            constexpr int K = 5, S = 2;                                       \
            __VA_ARGS__;                                                      \
        }                                                                     \
    } while (0)

}  // namespace

extern "C" {

int vt_dwt_tile(int32_t Hi, int32_t Wi, int32_t C, int32_t k, int32_t s, int32_t dtype, int32_t* rows_per_band,
                int32_t* channels_per_slab) {
    DwtArgs a;
    VT_TRY(fill(a, "vt_dwt_tile", dtype, 1, Hi, Wi, C, k, s));
    if (rows_per_band) *rows_per_band = a.R;
    if (channels_per_slab) *channels_per_slab = a.SC * vt_epc(dtype);
    return VT_OK;
}

int64_t vt_dwt_shares_bytes(int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t k, int32_t s, int32_t dtype) {
    DwtArgs a;
    if (fill(a, "vt_dwt_shares_bytes", dtype, B, Hi, Wi, C, k, s) != VT_OK) return -1;
    return (int64_t)B * a.NB * k * k * C * (int64_t)sizeof(float);
}

int vt_dwt_fwd(const void* x, int32_t ldx, const float* w, void* z, int32_t ldz, float* stats, int32_t B, int32_t Hi, int32_t Wi,
               int32_t C, int32_t k, int32_t s, int32_t dtype, void* stream) {
    VT_REQUIRE(x && w && z, VT_ERR_INVALID, "vt_dwt_fwd: null argument");
    DwtArgs a;
    VT_TRY(fill(a, "vt_dwt_fwd", dtype, B, Hi, Wi, C, k, s));
    const int epc = vt_epc(dtype);
    VT_REQUIRE(mat_ok(x, ldx, C, epc) && mat_ok(z, ldz, C, epc), VT_ERR_INVALID, "vt_dwt_fwd: bad strides / alignment (ldx=%d ldz=%d)",
               ldx, ldz);
    a.x = x, a.w = w, a.z = z, a.stats = stats, a.ldx = ldx, a.ldz = ldz;
    const int red = (kT * 2 * epc + kT) * (int)sizeof(float);  // the statistics fold reuses the tile
    const int lds = stats && red > a.lds ? red : a.lds;
    const dim3 grid((unsigned)((long)B * a.NB * a.NS));
    if (stats) {
        DWT_DISPATCH(dtype, k, s, hipLaunchKernelGGL((dwt_fwd_kernel<T, K, S, true>), grid, dim3(kT), lds, (hipStream_t)stream, a));
    } else {
        DWT_DISPATCH(dtype, k, s, hipLaunchKernelGGL((dwt_fwd_kernel<T, K, S, false>), grid, dim3(kT), lds, (hipStream_t)stream, a));
    }
    VT_CHECK_LAUNCH("vt_dwt_fwd");
    return VT_OK;
}

int vt_dwt_bwd(const void* dz, int32_t lddz, const void* x, int32_t ldx, const float* w, void* dx, int32_t lddx, const void* residual,
               int32_t ldr, float* shares, int64_t shares_bytes, int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t k, int32_t s,
               int32_t dtype, void* stream) {
    VT_REQUIRE(dz && x && w && dx && shares, VT_ERR_INVALID, "vt_dwt_bwd: null argument");
    DwtArgs a;
    VT_TRY(fill(a, "vt_dwt_bwd", dtype, B, Hi, Wi, C, k, s));
    const int epc = vt_epc(dtype);
    VT_REQUIRE(mat_ok(dz, lddz, C, epc) && mat_ok(x, ldx, C, epc) && mat_ok(dx, lddx, C, epc) &&
                   (!residual || mat_ok(residual, ldr, C, epc)) && vt_aligned16(shares),
               VT_ERR_INVALID, "vt_dwt_bwd: bad strides / alignment (lddz=%d ldx=%d lddx=%d ldr=%d)", lddz, ldx, lddx, ldr);
    const int64_t need = (int64_t)B * a.NB * k * k * C * (int64_t)sizeof(float);
    VT_REQUIRE(shares_bytes >= need, VT_ERR_INVALID, "vt_dwt_bwd: shares_bytes=%ld, %ld needed", (long)shares_bytes, (long)need);
    a.x = x, a.w = w, a.z = const_cast<void*>(dz), a.dx = dx, a.res = residual, a.shares = shares;
    a.ldx = ldx, a.ldz = lddz, a.lddx = lddx, a.ldr = ldr;
    const int red = kT * epc * (int)sizeof(float);  // the fold of the pixel ranges reuses the tiles
    const int lds = red > a.lds ? red : a.lds;
    const dim3 grid((unsigned)((long)B * a.NB * a.NS));
    DWT_DISPATCH(dtype, k, s, hipLaunchKernelGGL((dwt_bwd_kernel<T, K, S>), grid, dim3(kT), lds, (hipStream_t)stream, a));
    VT_CHECK_LAUNCH("vt_dwt_bwd");
    return VT_OK;
}

int vt_dwt_wgrad_reduce(const float* shares, int64_t shares_bytes, float* dw, int32_t B, int32_t Hi, int32_t Wi, int32_t C,
                        int32_t k, int32_t s, int32_t dtype, void* stream) {
    VT_REQUIRE(shares && dw, VT_ERR_INVALID, "vt_dwt_wgrad_reduce: null argument");
    DwtArgs a;
    VT_TRY(fill(a, "vt_dwt_wgrad_reduce", dtype, B, Hi, Wi, C, k, s));
    const int64_t need = (int64_t)B * a.NB * k * k * C * (int64_t)sizeof(float);
    VT_REQUIRE(shares_bytes >= need, VT_ERR_INVALID, "vt_dwt_wgrad_reduce: shares_bytes=%ld, %ld needed", (long)shares_bytes,
               (long)need);
    hipLaunchKernelGGL(dwt_wgrad_reduce_kernel, dim3((unsigned)((k * k * C + 31) / 32)), dim3(kT), 0, (hipStream_t)stream, shares, dw,
                       B * a.NB, C, k * k);
    VT_CHECK_LAUNCH("vt_dwt_wgrad_reduce");
    return VT_OK;
}

}  // extern "C"
