// vt_gconv.hip -- grouped 3x3 convolution (padding 1, stride 1 or 2, Cin = Cout = C in C / gw groups of gw channels: the
// `f.b` unit of every RegNet block), forward, data gradient and filter gradient, each ONE launch over the whole map with
// block-diagonal filters; and the Squeeze-Excitation MLP of the RegNetY blocks (vt_se_mlp_fwd / vt_se_mlp_bwd).
//
// At 8 .. 64 channels per group the convolution is HBM-bound (gw = 16: 288 flop per output element against 4 bytes), so
// nothing is staged: a wave owns ONE group and a run of 16-pixel tiles, and every operand fragment is a load from global
// memory that the L1 / L2 serve after its first touch (the nine taps of a pixel, the group's filter).  No LDS, no barriers.
//
// One index map for the three kernels and both dtypes.  The product of a tile is D[row][col] with 16 rows, 16 columns and
// the reduction index k cut into chunks; a lane is (pl = lane & 15, q4 = lane >> 4):
//   forward   rows = output channels of the group, cols = 16 output pixels,  k = (tap, input channel)   [9 * gw]
//   dgrad     rows = input channels of the group,  cols = 16 input pixels,   k = (tap, output channel)  [9 * gw]
//   wgrad     rows = output channels,              cols = input channels,    k = the pixels of a slab
// and a lane owns D[rows 4 q4 .. 4 q4 + 3][col pl]: four consecutive channels of one pixel (one 8 / 16 byte store) in
// forward and dgrad, four filter rows at one input channel in wgrad.
//   bf16: v_mfma_f32_16x16x32_bf16.  A lane's operand fragment is 8 consecutive k at row / column pl, chunk q = 4 kstep + q4.
//         In forward k = tap * gw + ci is exactly the filter row [3][3][gw] and, inside one tap, a 16-byte channel chunk of
//         the pixel: both fragments are ONE 16-byte load.  9 gw / 8 chunks are padded with zero fragments to a multiple of
//         four (gw = 16: 18 -> 20).  The 16-deep form would need no padding but halves the fragment to 8 bytes and doubles
//         the MFMA issues; at these widths the loads, not the zero chunks, are what a wave waits for.
//         dgrad and wgrad gather the fragments whose 8 k are not contiguous in memory (the transposed filter; 8 pixels of
//         one channel) with 8 two-byte loads.
//   f32:  the same lanes, tiles, tap maps, masks and stores; the lane forms its four outputs with an FMA chain over k in
//         ascending order instead of the MFMA.  Exact f32: what pins the index maps in the tests.
// Group widths that are no multiple of 16 (8, 24, 40, 56) run whole 16-row tiles with the rows / columns beyond gw masked.
//
// Statistics (forward): per-channel sum and sum of squares of the STORED z, fixed point (vt_stat_add), the contract of
// VT_CONV_STATS.  Filter gradient: the pixels are cut into S slabs, a wave owns (slab, group, 16 filter rows, filter row
// kh) and stores its partial tile into scratch [S][C][9][gw]; a second kernel adds the slabs in slab order, one owner per
// filter element (dw += sum).  No float atomics anywhere: two runs are bit-identical.
#include "vt_act.h"
#include "vt_common.h"

namespace {

constexpr int kT = 256;  // 4 waves; a wave never waits for another one

struct GArgs {
    const void* x;    // fwd: x; dgrad: dz; wgrad: x
    const void* w;    // filter [C][3][3][gw] in the compute dtype
    void* y;          // fwd: z; dgrad: dx; wgrad: dz (read)
    const void* res;  // dgrad: added to dx (may alias dx)
    float* stats;
    float* part;      // wgrad: [S][C][9][gw]
    long M;           // pixels the launch tiles over (fwd / wgrad: output pixels, dgrad: input pixels)
    int B, Hi, Wi, Ho, Wo, C, gw, s, G;
    int ldx, ldy, ldr;
    int tiles, tpw;   // 16-pixel tiles, tiles per wave
    int S, pps, MT;   // wgrad: slabs, pixels per slab (a multiple of 32), 16-row tiles per group
};

template <typename T>
struct Frag;  // a 16-byte chunk of operands
template <>
struct Frag<bf16_t> {
    static __device__ __forceinline__ void mma(const uint4& a, const uint4& b, f32x4& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
};

__device__ __forceinline__ uint4 zero4() { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint32_t ld16(const bf16_t* p) { return (uint32_t)*(const unsigned short*)p; }

// four consecutive channels of one pixel in the storage type; `r` receives the stored (rounded) values
template <typename T>
__device__ __forceinline__ void store4(T* p, const float (&v)[4], float (&r)[4]);
template <>
__device__ __forceinline__ void store4<float>(float* p, const float (&v)[4], float (&r)[4]) {
    *(uint4*)p = VecIO<float>::pack(v);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = v[i];
}
template <>
__device__ __forceinline__ void store4<bf16_t>(bf16_t* p, const float (&v)[4], float (&r)[4]) {
    const uint2 o = make_uint2(VecIO<bf16_t>::pack2(v[0], v[1]), VecIO<bf16_t>::pack2(v[2], v[3]));
    *(uint2*)p = o;
    r[0] = __uint_as_float(o.x << 16), r[1] = __uint_as_float(o.x & 0xffff0000u);
    r[2] = __uint_as_float(o.y << 16), r[3] = __uint_as_float(o.y & 0xffff0000u);
}
template <typename T>
__device__ __forceinline__ void load4(const T* p, float (&v)[4]);
template <>
__device__ __forceinline__ void load4<float>(const float* p, float (&v)[4]) {
    VecIO<float>::unpack(*(const uint4*)p, v);
}
template <>
__device__ __forceinline__ void load4<bf16_t>(const bf16_t* p, float (&v)[4]) {
    const uint2 o = *(const uint2*)p;
    v[0] = __uint_as_float(o.x << 16), v[1] = __uint_as_float(o.x & 0xffff0000u);
    v[2] = __uint_as_float(o.y << 16), v[3] = __uint_as_float(o.y & 0xffff0000u);
}

// pixel index -> (image, row, column) of an [B][H][W] map
__device__ __forceinline__ void decode(long p, int H, int W, long& b, int& h, int& w) {
    const unsigned q = (unsigned)p, hw = (unsigned)(H * W);  // (fill() keeps the pixel count far below 2^31)
    const unsigned bi = q / hw, rem = q - bi * hw;
    b = bi;
    h = (int)(rem / (unsigned)W), w = (int)(rem - (unsigned)h * (unsigned)W);
}

// the source pixel of tap (kh, kw) as the FORWARD reads it from output pixel (oh, ow): offset into x, or -1 (padding)
__device__ __forceinline__ long fwd_src(const GArgs& a, long b, int oh, int ow, int kh, int kw) {
    const int ih = oh * a.s - 1 + kh, iw = ow * a.s - 1 + kw;
    if (ih < 0 || ih >= a.Hi || iw < 0 || iw >= a.Wi) return -1;
    return ((b * a.Hi + ih) * a.Wi + iw) * (long)a.ldx;
}
// the dz pixel that tap (kh, kw) of input pixel (ih, iw) receives a gradient from: offset into dz, or -1 (no such output)
__device__ __forceinline__ long dgrad_src(const GArgs& a, long b, int ih, int iw, int kh, int kw) {
    const int hn = ih + 1 - kh, wn = iw + 1 - kw;
    if (hn < 0 || wn < 0 || (hn % a.s) || (wn % a.s)) return -1;
    const int oh = hn / a.s, ow = wn / a.s;
    if (oh >= a.Ho || ow >= a.Wo) return -1;
    return ((b * a.Ho + oh) * a.Wo + ow) * (long)a.ldx;
}

// ---- forward / data gradient: one kernel body, DGRAD picks the tap map and the filter transposition -------------------
template <typename T, int NT, bool DGRAD, bool STATS>
__global__ void __launch_bounds__(kT) gconv_tile_kernel(const GArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.y * 4 + wave;
    if (g >= a.G) return;
    const int pl = lane & 15, q4 = lane >> 4;
    const int gw = a.gw, c0 = g * gw;
    const int H = DGRAD ? a.Hi : a.Ho, W = DGRAD ? a.Wi : a.Wo;  // the map the tiles walk
    const T* x = (const T*)a.x;
    const T* w = (const T*)a.w + (long)c0 * 9 * gw;  // the group's filter rows [gw][9][gw]
    T* y = (T*)a.y;
    const T* res = (const T*)a.res;
    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) s1[nt][i] = s2[nt][i] = 0.f;

    for (int tt = 0; tt < a.tpw; ++tt) {
        const int tile = blockIdx.x * a.tpw + tt;
        if (tile >= a.tiles) break;
        const long p = (long)tile * 16 + pl;
        const bool pv = p < a.M;
        long b;
        int ph, pw;
        decode(pv ? p : 0, H, W, b, ph, pw);
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

        if constexpr (sizeof(T) == 2) {
            const int cpg = gw >> 3, nq = 9 * cpg;  // 8-element chunks per tap, chunks of k
            for (int q0 = 0; q0 < nq; q0 += 4) {
                const int q = q0 + q4;
                const bool qv = q < nq;
                const int tap = qv ? q / cpg : 0, cc = qv ? q - tap * cpg : 0;
                uint4 bf = zero4();
                if (qv && pv) {
                    const long off = DGRAD ? dgrad_src(a, b, ph, pw, tap / 3, tap % 3) : fwd_src(a, b, ph, pw, tap / 3, tap % 3);
                    if (off >= 0) bf = *(const uint4*)(x + off + c0 + cc * 8);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int row = nt * 16 + pl;  // fwd: output channel, dgrad: input channel (inside the group)
                    uint4 af = zero4();
                    if (qv && row < gw) {
                        if (!DGRAD) {
                            af = *(const uint4*)(w + (long)row * 9 * gw + q * 8);
                        } else {  // w[co = 8 cc + j][tap][ci = row], j = 0 .. 7
                            const T* wp = w + ((long)(cc * 8) * 9 + tap) * gw + row;
                            const long st = 9L * gw;
                            af.x = ld16((const bf16_t*)wp) | (ld16((const bf16_t*)(wp + st)) << 16);
                            af.y = ld16((const bf16_t*)(wp + 2 * st)) | (ld16((const bf16_t*)(wp + 3 * st)) << 16);
                            af.z = ld16((const bf16_t*)(wp + 4 * st)) | (ld16((const bf16_t*)(wp + 5 * st)) << 16);
                            af.w = ld16((const bf16_t*)(wp + 6 * st)) | (ld16((const bf16_t*)(wp + 7 * st)) << 16);
                        }
                    }
                    Frag<bf16_t>::mma(af, bf, acc[nt]);
                }
            }
        } else {
            // exact f32: the lane's own four rows 4 q4 .. 4 q4 + 3 at column pl, k ascending (tap, then channel)
            for (int tap = 0; tap < 9; ++tap) {
                if (!pv) break;
                const long off = DGRAD ? dgrad_src(a, b, ph, pw, tap / 3, tap % 3) : fwd_src(a, b, ph, pw, tap / 3, tap % 3);
                if (off < 0) continue;
                const float* xp = (const float*)x + off + c0;
                for (int k4 = 0; k4 < gw; k4 += 4) {
                    float xv[4];
                    load4<float>(xp + k4, xv);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const int r0 = nt * 16 + q4 * 4;
                        if (r0 >= gw) continue;
                        if (!DGRAD) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                float wv[4];
                                load4<float>((const float*)w + ((long)(r0 + i) * 9 + tap) * gw + k4, wv);
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc[nt][i] = fmaf(wv[j], xv[j], acc[nt][i]);
                            }
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                float wv[4];  // w[co = k4 + j][tap][ci = r0 .. r0 + 3]
                                load4<float>((const float*)w + ((long)(k4 + j) * 9 + tap) * gw + r0, wv);
#pragma unroll
                                for (int i = 0; i < 4; ++i) acc[nt][i] = fmaf(wv[i], xv[j], acc[nt][i]);
                            }
                        }
                    }
                }
            }
        }

        if (pv) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int r0 = nt * 16 + q4 * 4;
                if (r0 >= gw) continue;
                float v[4] = {acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]}, r[4];
                if (DGRAD && res) {
                    // (the sum is rounded to the storage type first, as a separate data-gradient launch + add would)
                    float rv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = VecIO<T>::round(v[i]);
                    load4<T>(res + p * a.ldr + c0 + r0, rv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += rv[i];
                }
                store4<T>(y + p * a.ldy + c0 + r0, v, r);
                if (STATS) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) s1[nt][i] += r[i], s2[nt][i] = fmaf(r[i], r[i], s2[nt][i]);
                }
            }
        }
    }
    if (STATS) {
        const int rep = blockIdx.x % kStatReplicas;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float u = s1[nt][i], v = s2[nt][i];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) u += __shfl_xor(u, o, 64), v += __shfl_xor(v, o, 64);
                const int r0 = nt * 16 + q4 * 4;
                if (pl == 0 && r0 < gw) {
                    vt_stat_add(a.stats, ((long)rep * 2 + 0) * a.C + c0 + r0 + i, u);
                    vt_stat_add(a.stats, ((long)rep * 2 + 1) * a.C + c0 + r0 + i, v);
                }
            }
        }
    }
}

// ---- filter gradient, stage 1: a wave owns (slab, group, 16 filter rows mt, filter row kh) ------------------------------
template <typename T, int NT>
__global__ void __launch_bounds__(kT) gconv_wgrad_kernel(const GArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.y * 4 + wave;
    if (item >= a.G * a.MT * 3) return;
    const int kh = item % 3, mt = (item / 3) % a.MT, g = item / (3 * a.MT);
    const int pl = lane & 15, q4 = lane >> 4;
    const int gw = a.gw, c0 = g * gw, sl = blockIdx.x;
    const T* x = (const T*)a.x;
    const T* dz = (const T*)a.y;
    const long p0 = (long)sl * a.pps;
    const long p1 = (p0 + a.pps < a.M) ? p0 + a.pps : a.M;
    f32x4 acc[3][NT];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[kw][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (sizeof(T) == 2) {
        const int row = mt * 16 + pl;  // the output channel of the A fragment
        for (long pk = p0; pk < p1; pk += 32) {
            uint32_t ah[8];
            long off[3][8];
            // the lane's 8 consecutive pixels: one decode, then steps along the row (no division per pixel)
            long b;
            int oh, ow;
            decode(pk + q4 * 8 < p1 ? pk + q4 * 8 : p0, a.Ho, a.Wo, b, oh, ow);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long p = pk + q4 * 8 + j;
                ah[j] = 0;
                off[0][j] = off[1][j] = off[2][j] = -1;
                if (p < p1) {
                    if (row < gw) ah[j] = ld16(dz + p * a.ldy + c0 + row);
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) off[kw][j] = fwd_src(a, b, oh, ow, kh, kw);
                }
                if (++ow == a.Wo) {
                    ow = 0;
                    if (++oh == a.Ho) oh = 0, ++b;
                }
            }
            const uint4 af = make_uint4(ah[0] | (ah[1] << 16), ah[2] | (ah[3] << 16), ah[4] | (ah[5] << 16), ah[6] | (ah[7] << 16));
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int col = nt * 16 + pl;  // the input channel of the B fragment
                    uint32_t bh[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) bh[j] = (off[kw][j] >= 0 && col < gw) ? ld16(x + off[kw][j] + c0 + col) : 0u;
                    const uint4 bf = make_uint4(bh[0] | (bh[1] << 16), bh[2] | (bh[3] << 16), bh[4] | (bh[5] << 16), bh[6] | (bh[7] << 16));
                    Frag<bf16_t>::mma(af, bf, acc[kw][nt]);
                }
            }
        }
    } else {
        const int r0 = mt * 16 + q4 * 4;
        for (long p = p0; p < p1; ++p) {  // (uniform over the wave: every lane walks the slab's pixels in order)
            long b;
            int oh, ow;
            decode(p, a.Ho, a.Wo, b, oh, ow);
            float gv[4] = {0.f, 0.f, 0.f, 0.f};
            if (r0 < gw) load4<float>((const float*)dz + p * a.ldy + c0 + r0, gv);
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const long off = fwd_src(a, b, oh, ow, kh, kw);
                if (off < 0) continue;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int col = nt * 16 + pl;
                    if (col >= gw) continue;
                    const float xv = ((const float*)x)[off + c0 + col];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[kw][nt][i] = fmaf(gv[i], xv, acc[kw][nt][i]);
                }
            }
        }
    }
    // partial tile -> scratch [sl][C][9][gw]: rows 4 q4 .. 4 q4 + 3 of tile mt, column pl of tile nt
    const int r0 = mt * 16 + q4 * 4;
    if (r0 < gw) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nt * 16 + pl;
                if (col >= gw) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a.part[(((long)sl * a.C + c0 + r0 + i) * 9 + kh * 3 + kw) * gw + col] = acc[kw][nt][i];
            }
    }
}

// stage 2: one owner per filter element adds the slabs in slab order
__global__ void __launch_bounds__(kT) gconv_wgrad_reduce_kernel(const float* part, float* dw, long n, int S) {
    const long e = (long)blockIdx.x * kT + threadIdx.x;
    if (e >= n) return;
    float sum = 0.f;
    for (int sl = 0; sl < S; ++sl) sum += part[(long)sl * n + e];
    dw[e] += sum;
}

int fill(GArgs& a, const char* who, int dtype, int B, int Hi, int Wi, int C, int gw, int s) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && C > 0 && gw > 0, VT_ERR_INVALID, "%s: bad geometry", who);
    VT_REQUIRE(s == 1 || s == 2, VT_ERR_UNSUPPORTED, "%s: stride %d (1 or 2)", who, s);
    VT_REQUIRE(gw % 8 == 0 && gw >= 8 && gw <= 64, VT_ERR_UNSUPPORTED,
               "%s: group width %d (a multiple of 8 from 8 to 64: narrower groups are below one 16-byte bf16 chunk, wider ones run "
               "as per-group convolutions)", who, gw);
    VT_REQUIRE(C % gw == 0, VT_ERR_INVALID, "%s: C=%d is no multiple of the group width %d", who, C, gw);
    VT_REQUIRE((long)B * Hi * Wi < 0x7fffffffL / 64, VT_ERR_UNSUPPORTED, "%s: map too large", who);
    a.B = B, a.Hi = Hi, a.Wi = Wi, a.C = C, a.gw = gw, a.s = s, a.G = C / gw;
    a.Ho = (Hi - 1) / s + 1, a.Wo = (Wi - 1) / s + 1;
    a.MT = (gw + 15) / 16;
    return VT_OK;
}
void tile_plan(GArgs& a, long M) {
    a.M = M;
    a.tiles = (int)((M + 15) / 16);
    long tpw = (long)a.tiles * a.G / 8192;
    a.tpw = (int)(tpw < 1 ? 1 : (tpw > 8 ? 8 : tpw));
}
void slab_plan(GArgs& a) {
    a.M = (long)a.B * a.Ho * a.Wo;
    const long items = (long)a.G * a.MT * 3, n = (long)a.C * 9 * a.gw;
    long S = (3072 + items - 1) / items;
    const long by_pixels = (a.M + 63) / 64, by_bytes = (64L << 20) / (n * 4);
    if (S > by_pixels) S = by_pixels;
    if (S > by_bytes) S = by_bytes;
    if (S > 256) S = 256;
    if (S < 1) S = 1;
    long pps = ((a.M + S - 1) / S + 31) / 32 * 32;
    a.pps = (int)pps;
    a.S = (int)((a.M + pps - 1) / pps);
}
bool ok_ptr(const void* p, int ld, int C, int epc) { return p && vt_aligned16(p) && ld >= C && ld % epc == 0; }

#define VT_GCONV_NT(NTV, ...)        \
    do {                             \
        switch (NTV) {               \
            case 1: { constexpr int NT = 1; __VA_ARGS__; } break; \
            case 2: { constexpr int NT = 2; __VA_ARGS__; } break; \
            case 3: { constexpr int NT = 3; __VA_ARGS__; } break; \
            default: { constexpr int NT = 4; __VA_ARGS__; } break; \
        }                            \
    } while (0)

template <typename T, bool DGRAD, bool STATS>
void launch_tile(const GArgs& a, hipStream_t st) {
    const dim3 grid((a.tiles + a.tpw - 1) / a.tpw, (a.G + 3) / 4);
    VT_GCONV_NT(a.MT, hipLaunchKernelGGL((gconv_tile_kernel<T, NT, DGRAD, STATS>), grid, dim3(kT), 0, st, a));
}

// ---- Squeeze-Excitation MLP on the pooled row of an image ---------------------------------------------------------------
constexpr int kSeMaxC = 8192, kSeMaxS = 2048;

struct SeArgs {
    const void* pooled;   // fwd: [B][C]; bwd: the same rows again
    const void* dlogits;  // bwd
    const float *w1, *b1, *w2, *b2;
    float* hidden;        // [B][S] f32, holds storage-rounded values; act = 3: followed by the [B][S] f32 pre-activations
    void* out;            // fwd: logits; bwd: dpooled
    float* dhid;          // bwd: [B][S] d(pre-activation)
    float *dw1, *db1, *dw2, *db2;
    int B, C, S, ldp, ldo, ldg;
    int act;              // the squeeze activation: 1 ReLU, 3 SiLU (vt_act.h)
};

template <typename T>
__device__ __forceinline__ float ldT(const T* p) { return (float)*p; }

template <typename T>
__global__ void __launch_bounds__(kT) se_mlp_fwd_kernel(const SeArgs a) {
    __shared__ float sp[kSeMaxC];
    __shared__ float sh[kSeMaxS];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const T* p = (const T*)a.pooled + (long)b * a.ldp;
    for (int c = t; c < a.C; c += kT) sp[c] = ldT<T>(p + c);
    __syncthreads();
    for (int s = wave; s < a.S; s += kT / 64) {  // one wave per hidden value: lane-strided products, a fixed butterfly
        const float* wr = a.w1 + (long)s * a.C;
        float acc = 0.f;
        for (int c = lane; c < a.C; c += 64) acc = fmaf(VecIO<T>::round(wr[c]), sp[c], acc);
        acc = wave_sum(acc) + a.b1[s];
        const float h = VecIO<T>::round(a.act == 3 ? act_fwd(3, acc) : (acc > 0.f ? acc : 0.f));
        if (lane == 0) {
            sh[s] = h, a.hidden[(long)b * a.S + s] = h;
            if (a.act == 3) a.hidden[((long)a.B + b) * a.S + s] = acc;  // silu' needs the pre-activation
        }
    }
    __syncthreads();
    T* o = (T*)a.out + (long)b * a.ldo;
    for (int c = t; c < a.C; c += kT) {
        const float* wr = a.w2 + (long)c * a.S;
        float acc = 0.f;
        for (int s = 0; s < a.S; ++s) acc = fmaf(VecIO<T>::round(wr[s]), sh[s], acc);
        o[c] = from_float<T>(acc + a.b2[c]);
    }
}

// backward, per image: d(pre) = (W2^T dl) * [h > 0] (SiLU: * silu'(pre)) -> dhid, then d(pooled) = W1^T d(pre)
template <typename T>
__global__ void __launch_bounds__(kT) se_mlp_bwd_kernel(const SeArgs a) {
    __shared__ float sg[kSeMaxC];
    __shared__ float sd[kSeMaxS];
    const int b = blockIdx.x, t = threadIdx.x;
    const T* g = (const T*)a.dlogits + (long)b * a.ldg;
    for (int c = t; c < a.C; c += kT) sg[c] = ldT<T>(g + c);
    __syncthreads();
    for (int s = t; s < a.S; s += kT) {  // one owner per hidden value, channels in order
        float acc = 0.f;
        for (int c = 0; c < a.C; ++c) acc = fmaf(VecIO<T>::round(a.w2[(long)c * a.S + s]), sg[c], acc);
        const float d = a.act == 3 ? acc * act_grad(3, a.hidden[((long)a.B + b) * a.S + s])
                                   : (a.hidden[(long)b * a.S + s] > 0.f ? acc : 0.f);
        sd[s] = d, a.dhid[(long)b * a.S + s] = d;
    }
    __syncthreads();
    if (a.out) {
        T* o = (T*)a.out + (long)b * a.ldo;
        for (int c = t; c < a.C; c += kT) {
            float acc = 0.f;
            for (int s = 0; s < a.S; ++s) acc = fmaf(VecIO<T>::round(a.w1[(long)s * a.C + c]), sd[s], acc);
            o[c] = from_float<T>(acc);
        }
    }
}

// parameter gradients: one owner per element of (W1 | b1 | W2 | b2) adds the images in image order
template <typename T>
__global__ void __launch_bounds__(kT) se_mlp_param_kernel(const SeArgs a) {
    const long nW = (long)a.S * a.C;
    const long e = (long)blockIdx.x * kT + threadIdx.x;
    if (e >= 2 * nW + a.S + a.C) return;
    const T* p = (const T*)a.pooled;
    const T* g = (const T*)a.dlogits;
    float acc = 0.f;
    if (e < nW) {  // dW1[s][c] = sum_b d(pre)[b][s] * pooled[b][c]
        const int s = (int)(e / a.C), c = (int)(e % a.C);
        for (int b = 0; b < a.B; ++b) acc = fmaf(a.dhid[(long)b * a.S + s], ldT<T>(p + (long)b * a.ldp + c), acc);
        if (a.dw1) a.dw1[e] += acc;
    } else if (e < nW + a.S) {
        const int s = (int)(e - nW);
        for (int b = 0; b < a.B; ++b) acc += a.dhid[(long)b * a.S + s];
        if (a.db1) a.db1[s] += acc;
    } else if (e < 2 * nW + a.S) {  // dW2[c][s] = sum_b dl[b][c] * h[b][s]
        const long k = e - nW - a.S;
        const int c = (int)(k / a.S), s = (int)(k % a.S);
        for (int b = 0; b < a.B; ++b) acc = fmaf(ldT<T>(g + (long)b * a.ldg + c), a.hidden[(long)b * a.S + s], acc);
        if (a.dw2) a.dw2[k] += acc;
    } else {
        const int c = (int)(e - 2 * nW - a.S);
        for (int b = 0; b < a.B; ++b) acc += ldT<T>(g + (long)b * a.ldg + c);
        if (a.db2) a.db2[c] += acc;
    }
}

int se_check(const char* who, int B, int C, int S, int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && C > 0 && S > 0, VT_ERR_INVALID, "%s: bad geometry", who);
    VT_REQUIRE(C <= kSeMaxC && S <= kSeMaxS, VT_ERR_UNSUPPORTED, "%s: C=%d, S=%d exceed %d / %d", who, C, S, kSeMaxC, kSeMaxS);
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_gconv3_fwd(const void* x, int32_t ldx, const void* w, void* z, int32_t ldz, float* stats, int32_t B, int32_t Hi, int32_t Wi,
                  int32_t C, int32_t gw, int32_t stride, int32_t dtype, void* stream) {
    GArgs a;
    memset(&a, 0, sizeof(a));
    VT_TRY(fill(a, "vt_gconv3_fwd", dtype, B, Hi, Wi, C, gw, stride));
    const int epc = vt_epc(dtype);
    VT_REQUIRE(ok_ptr(x, ldx, C, epc) && ok_ptr(z, ldz, C, epc) && w && vt_aligned16(w), VT_ERR_INVALID,
               "vt_gconv3_fwd: null argument, bad strides or alignment");
    a.x = x, a.w = w, a.y = z, a.stats = stats, a.ldx = ldx, a.ldy = ldz;
    tile_plan(a, (long)B * a.Ho * a.Wo);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VT_BF16) {
        if (stats) launch_tile<bf16_t, false, true>(a, st);
        else launch_tile<bf16_t, false, false>(a, st);
    } else {
        if (stats) launch_tile<float, false, true>(a, st);
        else launch_tile<float, false, false>(a, st);
    }
    VT_CHECK_LAUNCH("vt_gconv3_fwd");
    return VT_OK;
}

int vt_gconv3_dgrad(const void* dz, int32_t lddz, const void* w, void* dx, int32_t lddx, const void* residual, int32_t ldr,
                    int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t gw, int32_t stride, int32_t dtype, void* stream) {
    GArgs a;
    memset(&a, 0, sizeof(a));
    VT_TRY(fill(a, "vt_gconv3_dgrad", dtype, B, Hi, Wi, C, gw, stride));
    const int epc = vt_epc(dtype);
    VT_REQUIRE(ok_ptr(dz, lddz, C, epc) && ok_ptr(dx, lddx, C, epc) && w && vt_aligned16(w) &&
                   (!residual || ok_ptr(residual, ldr, C, epc)),
               VT_ERR_INVALID, "vt_gconv3_dgrad: null argument, bad strides or alignment");
    a.x = dz, a.w = w, a.y = dx, a.res = residual, a.ldx = lddz, a.ldy = lddx, a.ldr = ldr;
    tile_plan(a, (long)B * Hi * Wi);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VT_BF16) launch_tile<bf16_t, true, false>(a, st);
    else launch_tile<float, true, false>(a, st);
    VT_CHECK_LAUNCH("vt_gconv3_dgrad");
    return VT_OK;
}

int64_t vt_gconv3_wgrad_scratch_bytes(int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t gw, int32_t stride) {
    GArgs a;
    memset(&a, 0, sizeof(a));
    if (fill(a, "vt_gconv3_wgrad_scratch_bytes", VT_F32, B, Hi, Wi, C, gw, stride) != VT_OK) return -1;
    slab_plan(a);
    return (int64_t)a.S * C * 9 * gw * 4;
}

int vt_gconv3_wgrad(const void* x, int32_t ldx, const void* dz, int32_t lddz, float* dw, void* scratch, int64_t scratch_bytes,
                    int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t gw, int32_t stride, int32_t dtype, void* stream) {
    GArgs a;
    memset(&a, 0, sizeof(a));
    VT_TRY(fill(a, "vt_gconv3_wgrad", dtype, B, Hi, Wi, C, gw, stride));
    const int epc = vt_epc(dtype);
    VT_REQUIRE(ok_ptr(x, ldx, C, epc) && ok_ptr(dz, lddz, C, epc) && dw && scratch, VT_ERR_INVALID,
               "vt_gconv3_wgrad: null argument, bad strides or alignment");
    slab_plan(a);
    const long n = (long)C * 9 * gw;
    VT_REQUIRE(scratch_bytes >= (int64_t)a.S * n * 4, VT_ERR_INVALID, "vt_gconv3_wgrad: scratch of %lld bytes, needs %lld",
               (long long)scratch_bytes, (long long)a.S * n * 4);
    a.x = x, a.y = const_cast<void*>(dz), a.part = (float*)scratch, a.ldx = ldx, a.ldy = lddz;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(a.S, (a.G * a.MT * 3 + 3) / 4);
    if (dtype == VT_BF16) VT_GCONV_NT(a.MT, hipLaunchKernelGGL((gconv_wgrad_kernel<bf16_t, NT>), grid, dim3(kT), 0, st, a));
    else VT_GCONV_NT(a.MT, hipLaunchKernelGGL((gconv_wgrad_kernel<float, NT>), grid, dim3(kT), 0, st, a));
    VT_CHECK_LAUNCH("vt_gconv3_wgrad");
    hipLaunchKernelGGL(gconv_wgrad_reduce_kernel, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, st, (const float*)scratch, dw, n,
                       a.S);
    VT_CHECK_LAUNCH("vt_gconv3_wgrad (reduce)");
    return VT_OK;
}

int vt_se_mlp_fwd(const void* pooled, int32_t ldp, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden,
                  void* logits, int32_t ldl, int32_t B, int32_t C, int32_t S, int32_t dtype, void* stream) {
    return vt_se_mlp_act_fwd(pooled, ldp, w1, b1, w2, b2, hidden, logits, ldl, B, C, S, 1, dtype, stream);
}

int vt_se_mlp_act_fwd(const void* pooled, int32_t ldp, const float* w1, const float* b1, const float* w2, const float* b2,
                      float* hidden, void* logits, int32_t ldl, int32_t B, int32_t C, int32_t S, int32_t act, int32_t dtype,
                      void* stream) {
    VT_TRY(se_check("vt_se_mlp_fwd", B, C, S, dtype));
    VT_REQUIRE(act == 1 || act == 3, VT_ERR_UNSUPPORTED, "vt_se_mlp_fwd: activation code %d (1 ReLU, 3 SiLU)", act);
    VT_REQUIRE(pooled && w1 && b1 && w2 && b2 && hidden && logits && ldp >= C && ldl >= C, VT_ERR_INVALID,
               "vt_se_mlp_fwd: null argument or bad strides");
    SeArgs a;
    memset(&a, 0, sizeof(a));
    a.pooled = pooled, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2, a.hidden = hidden, a.out = logits;
    a.B = B, a.C = C, a.S = S, a.ldp = ldp, a.ldo = ldl, a.act = act;
    if (dtype == VT_BF16) hipLaunchKernelGGL(se_mlp_fwd_kernel<bf16_t>, dim3(B), dim3(kT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(se_mlp_fwd_kernel<float>, dim3(B), dim3(kT), 0, (hipStream_t)stream, a);
    VT_CHECK_LAUNCH("vt_se_mlp_fwd");
    return VT_OK;
}

int vt_se_mlp_bwd(const void* dlogits, int32_t ldg, const void* pooled, int32_t ldp, const float* w1, const float* w2,
                  const float* hidden, float* dhidden, void* dpooled, int32_t lddp, float* dw1, float* db1, float* dw2, float* db2,
                  int32_t B, int32_t C, int32_t S, int32_t dtype, void* stream) {
    return vt_se_mlp_act_bwd(dlogits, ldg, pooled, ldp, w1, w2, hidden, dhidden, dpooled, lddp, dw1, db1, dw2, db2, B, C, S, 1, dtype,
                             stream);
}

int vt_se_mlp_act_bwd(const void* dlogits, int32_t ldg, const void* pooled, int32_t ldp, const float* w1, const float* w2,
                      const float* hidden, float* dhidden, void* dpooled, int32_t lddp, float* dw1, float* db1, float* dw2,
                      float* db2, int32_t B, int32_t C, int32_t S, int32_t act, int32_t dtype, void* stream) {
    VT_TRY(se_check("vt_se_mlp_bwd", B, C, S, dtype));
    VT_REQUIRE(act == 1 || act == 3, VT_ERR_UNSUPPORTED, "vt_se_mlp_bwd: activation code %d (1 ReLU, 3 SiLU)", act);
    VT_REQUIRE(dlogits && pooled && w1 && w2 && hidden && dhidden && ldg >= C && ldp >= C && (!dpooled || lddp >= C),
               VT_ERR_INVALID, "vt_se_mlp_bwd: null argument or bad strides");
    SeArgs a;
    memset(&a, 0, sizeof(a));
    a.dlogits = dlogits, a.pooled = pooled, a.w1 = w1, a.w2 = w2, a.hidden = const_cast<float*>(hidden), a.dhid = dhidden;
    a.out = dpooled, a.dw1 = dw1, a.db1 = db1, a.dw2 = dw2, a.db2 = db2;
    a.B = B, a.C = C, a.S = S, a.ldp = ldp, a.ldo = lddp, a.ldg = ldg, a.act = act;
    hipStream_t st = (hipStream_t)stream;
    const long n = 2L * S * C + S + C;
    if (dtype == VT_BF16) {
        hipLaunchKernelGGL(se_mlp_bwd_kernel<bf16_t>, dim3(B), dim3(kT), 0, st, a);
        VT_CHECK_LAUNCH("vt_se_mlp_bwd");
        hipLaunchKernelGGL(se_mlp_param_kernel<bf16_t>, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, st, a);
    } else {
        hipLaunchKernelGGL(se_mlp_bwd_kernel<float>, dim3(B), dim3(kT), 0, st, a);
        VT_CHECK_LAUNCH("vt_se_mlp_bwd");
        hipLaunchKernelGGL(se_mlp_param_kernel<float>, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, st, a);
    }
    VT_CHECK_LAUNCH("vt_se_mlp_bwd (parameters)");
    return VT_OK;
}

}  // extern "C"
