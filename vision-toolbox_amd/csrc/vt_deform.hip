// vt_deform.hip -- the modulated deformable convolution of DeformableConv2d (reference components.py:77-135; the op is
// torchvision's deform_conv2d with one offset group and groups = 1):
//
//   y[b][ho][wo][co] = bias[co] + sum over taps t = i*k + j and channels ci of
//                      w[co][t][ci] * m_t * bilinear(x[b], ho*s - p + i*d + off[2t], wo*s - p + j*d + off[2t+1])[ci]
//
// with m_t = mask_act(mask logit t) (1 without a mask), bilinear over floor and floor + 1, and a corner outside the map
// contributing zero.  At an exactly integer position the floor cell is used: d(offset) is the right-hand derivative.
//
// It is a convolution whose im2col is a data-dependent gather.  The maps are NHWC, so a corner of a sample is a contiguous
// channel vector and a blended 16-byte chunk (8 bf16 channels of one sample) is exactly one lane's operand fragment of
// v_mfma_f32_16x16x32_bf16: the column matrix is never stored, nothing goes through LDS, there are no barriers.  As in
// vt_gconv.hip a wave works alone on 16-pixel tiles, a lane is (pl = lane & 15, q4 = lane >> 4) and owns
// D[rows 4 q4 .. 4 q4 + 3][column pl] of a 16 x 16 product:
//   forward   rows = output channels,  cols = 16 output pixels,  k = (tap, input channel), Cin padded to 32 with zero fragments
//   backward  rows = input channels,   cols = 16 output pixels,  k = output channels       (dcol = W_t^T dy, per tap)
//   wgrad     rows = output channels,  cols = input channels,    k = the pixels of a slab  (dy^T col, per tap)
//   bf16: MFMA; the forward's two fragments are one 16-byte filter load and four blended 16-byte corner loads; backward and
//         wgrad gather the fragments whose 8 k are not contiguous (transposed filter; 8 pixels of one channel) with
//         two-byte loads.
//   f32:  the same lanes, tiles, tap maps, masks and stores; an FMA chain over k ascending instead of the MFMA.  Exact f32.
// Position arithmetic, bilinear weights and the sigmoid are f32 in both dtypes (tap_geom, shared by the three kernels).
//
// BACKWARD, one launch over the pixel tiles.  Per tap and per group of 64 input channels the wave forms dcol in its
// accumulators -- it STAYS f32: d(offset) is a difference of corners -- and uses it at once:
//   d(mask logit) = act' * sum_c dcol_c * sample_c            d(offset) = m * sum_c dcol_c * d(sample_c)/d(y, x)
//   are summed in a fixed order (channel groups, tiles, the lane's four channels, then a butterfly over q4) by the wave that
//   owns the pixel: no atomics, bit-identical runs;
//   d(x) is a scatter to data-dependent places: f32 atomics (16 bytes of one corner per lane) into a zeroed f32 plane
//   [B][H][W][Cin], and a flush pass writes or accumulates the rounded plane into d(x).  d(x) is the one output that is not
//   bit-reproducible.
// WGRAD.  The pixels are cut into S slabs; a wave owns (slab, tap, 16 input channels, a group of output-channel tiles),
// re-samples its column fragment as the forward does (the same blend in the same order, rounded once to bf16) and stores
// its partial tile into scratch [S][Cout][K^2][Cin] (+ [S][Cout] bias partials); a second kernel adds the slabs in slab
// order, one owner per element (dw += sum, db += sum).  No float atomics.
#include "vt_common.h"

namespace {

constexpr int kT = 256;  // 4 waves; a wave never waits for another one

struct DArgs {
    const void* x;
    const void* off;   // [B][Ho][Wo] x (2 K^2) offsets, pixel stride ldo
    const void* msk;   // [B][Ho][Wo] x K^2 raw mask logits, pixel stride ldm, or NULL
    const void* w;     // [Cout][K^2][Cin] in the compute dtype
    const float* bias;
    void* y;           // fwd: y; bwd / wgrad: dy (read)
    void* doff;
    void* dmsk;
    float* plane;      // bwd: [B][H][W][Cin] f32, zero on entry (NULL: no d(x))
    float* part;       // wgrad: [S][Cout][K^2][Cin] | [S][Cout]
    long M;            // output pixels
    int B, H, W, Ho, Wo, Cin, Cout, k, K2, s, p, d, act;
    int ldx, ldo, ldm, ldy, lddo, lddm;
    int tiles;         // 16-pixel tiles
    int S, pps;        // wgrad: slabs, pixels per slab (a multiple of 32)
    int CT, CZ;        // wgrad: 16-column tiles of Cin, groups of MT 16-row tiles of Cout
};

__device__ __forceinline__ void mma_bf16(const uint4& a, const uint4& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
__device__ __forceinline__ uint4 zero4() { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint32_t ld16(const bf16_t* p) { return (uint32_t)*(const unsigned short*)p; }
__device__ __forceinline__ uint32_t bits16(float v) {
    const bf16_t h = (bf16_t)v;
    return (uint32_t)__builtin_bit_cast(unsigned short, h);
}

// four consecutive channels of one pixel in the storage type
template <typename T>
__device__ __forceinline__ void store4(T* p, const float (&v)[4]);
template <>
__device__ __forceinline__ void store4<float>(float* p, const float (&v)[4]) {
    *(uint4*)p = VecIO<float>::pack(v);
}
template <>
__device__ __forceinline__ void store4<bf16_t>(bf16_t* p, const float (&v)[4]) {
    *(uint2*)p = make_uint2(VecIO<bf16_t>::pack2(v[0], v[1]), VecIO<bf16_t>::pack2(v[2], v[3]));
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

// pixel index -> (image, row, column) of a [B][H][W] map (check_geometry keeps the pixel count below 2^31)
__device__ __forceinline__ void decode(long p, int H, int W, long& b, int& h, int& w) {
    const unsigned q = (unsigned)p, hw = (unsigned)(H * W);
    const unsigned bi = q / hw, rem = q - bi * hw;
    b = bi;
    h = (int)(rem / (unsigned)W), w = (int)(rem - (unsigned)h * (unsigned)W);
}

// One (output pixel, tap): the four corners (y0, x0), (y0, x1), (y1, x0), (y1, x1) as pixel indices of x (-1: outside the
// map, or the whole sample is), their bilinear weights and the weights' derivatives by the sampling position (zero for a
// corner outside), the mask value m and act'(logit).
struct Tap {
    long px[4];
    float w[4], gy[4], gx[4];
    float m, dm;
};

__device__ __forceinline__ void tap_none(Tap& g) {
#pragma unroll
    for (int c = 0; c < 4; ++c) g.px[c] = -1, g.w[c] = 0.f, g.gy[c] = 0.f, g.gx[c] = 0.f;
    g.m = 1.f, g.dm = 0.f;
}

template <typename T>
__device__ __forceinline__ void tap_geom(const DArgs& a, long pix, long b, int ho, int wo, int t, Tap& g) {
    tap_none(g);
    const int i = t / a.k, j = t - i * a.k;
    const T* op = (const T*)a.off + pix * a.ldo + 2 * t;
    const float py = (float)(ho * a.s - a.p + i * a.d) + (float)op[0];
    const float px = (float)(wo * a.s - a.p + j * a.d) + (float)op[1];
    if (a.msk) {
        const float z = (float)((const T*)a.msk)[pix * a.ldm + t];
        if (a.act == 1) {
            const float sg = 1.0f / (1.0f + expf(-z));
            g.m = sg, g.dm = sg * (1.0f - sg);
        } else {
            g.m = z, g.dm = 1.0f;
        }
    }
    // no corner inside the map (also a NaN offset).  A position of exactly -1 stays: its floor + 1 corner has weight zero but a
    // right-hand derivative, like every other integer position.
    if (!(py >= -1.0f && py < (float)a.H && px >= -1.0f && px < (float)a.W)) return;
    const float fy = floorf(py), fx = floorf(px);
    const int y0 = (int)fy, x0 = (int)fx;  // -1 .. H - 1, -1 .. W - 1
    const float ly = py - fy, lx = px - fx, hy = 1.0f - ly, hx = 1.0f - lx;
    const bool vy0 = y0 >= 0, vy1 = y0 + 1 < a.H, vx0 = x0 >= 0, vx1 = x0 + 1 < a.W;
    const long base = (b * a.H + y0) * (long)a.W + x0;
    if (vy0 && vx0) g.px[0] = base, g.w[0] = hy * hx, g.gy[0] = -hx, g.gx[0] = -hy;
    if (vy0 && vx1) g.px[1] = base + 1, g.w[1] = hy * lx, g.gy[1] = -lx, g.gx[1] = hy;
    if (vy1 && vx0) g.px[2] = base + a.W, g.w[2] = ly * hx, g.gy[2] = hx, g.gx[2] = -ly;
    if (vy1 && vx1) g.px[3] = base + a.W + 1, g.w[3] = ly * lx, g.gy[3] = lx, g.gx[3] = ly;
}

// ---- forward -------------------------------------------------------------------------------------------------------------
// grid (tiles / 4, Cout / (16 NT)): a wave owns 16 output pixels and NT 16-row tiles of output channels.  NT reaches 16, so
// up to 256 output channels share one sampling of the tile; wider layers re-sample once per 256.
template <typename T, int NT>
__global__ void __launch_bounds__(kT) deform_fwd_kernel(const DArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= a.tiles) return;
    const int pl = lane & 15, q4 = lane >> 4;
    const int co0 = blockIdx.y * NT * 16;
    const long p = (long)tile * 16 + pl;
    const bool pv = p < a.M;
    long b;
    int ho, wo;
    decode(pv ? p : 0, a.Ho, a.Wo, b, ho, wo);
    const T* x = (const T*)a.x;
    const T* w = (const T*)a.w;
    const int K2 = a.K2, Cin = a.Cin;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < K2; ++t) {
        Tap g;
        if (pv) tap_geom<T>(a, p, b, ho, wo, t, g);
        else tap_none(g);
        float cw[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) cw[c] = g.w[c] * g.m;
        if constexpr (sizeof(T) == 2) {
            const int cpr = Cin >> 3;  // 16-byte chunks per pixel; a k-step of 32 is four of them
            for (int c0 = 0; c0 < cpr; c0 += 4) {
                const int ch = c0 + q4;
                const bool cv = ch < cpr;
                uint4 bf = zero4();
                if (cv && pv) {
                    float sv[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) sv[e] = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (g.px[c] < 0) continue;
                        float f[8];
                        VecIO<bf16_t>::unpack(*(const uint4*)(x + g.px[c] * a.ldx + ch * 8), f);
#pragma unroll
                        for (int e = 0; e < 8; ++e) sv[e] = fmaf(cw[c], f[e], sv[e]);
                    }
                    bf = VecIO<bf16_t>::pack(sv);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int row = co0 + nt * 16 + pl;
                    uint4 af = zero4();
                    if (cv && row < a.Cout) af = *(const uint4*)(w + ((long)row * K2 + t) * Cin + ch * 8);
                    mma_bf16(af, bf, acc[nt]);
                }
            }
        } else {
            if (!pv) continue;
            for (int k4 = 0; k4 < Cin; k4 += 4) {
                float sv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (g.px[c] < 0) continue;
                    float f[4];
                    load4<float>((const float*)x + g.px[c] * a.ldx + k4, f);
#pragma unroll
                    for (int e = 0; e < 4; ++e) sv[e] = fmaf(cw[c], f[e], sv[e]);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int r0 = co0 + nt * 16 + q4 * 4;
                    if (r0 >= a.Cout) continue;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float wv[4];
                        load4<float>((const float*)w + ((long)(r0 + i) * K2 + t) * Cin + k4, wv);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[nt][i] = fmaf(wv[j], sv[j], acc[nt][i]);
                    }
                }
            }
        }
    }
    if (!pv) return;
    T* y = (T*)a.y;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int r0 = co0 + nt * 16 + q4 * 4;
        if (r0 >= a.Cout) continue;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc[nt][i] + (a.bias ? a.bias[r0 + i] : 0.f);
        store4<T>(y + p * a.ldy + r0, v);
    }
}

// ---- backward: d(offset), d(mask logit), and the scatter of d(x) into the f32 plane -------------------------------------------
constexpr int kBN = 4;  // 16-row tiles of input channels a wave holds as dcol at a time

template <typename T>
__global__ void __launch_bounds__(kT) deform_bwd_kernel(const DArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= a.tiles) return;
    const int pl = lane & 15, q4 = lane >> 4;
    const long p = (long)tile * 16 + pl;
    const bool pv = p < a.M;
    long b;
    int ho, wo;
    decode(pv ? p : 0, a.Ho, a.Wo, b, ho, wo);
    const T* x = (const T*)a.x;
    const T* w = (const T*)a.w;
    const T* dy = (const T*)a.y;
    const int K2 = a.K2, Cin = a.Cin, Cout = a.Cout;
    const int groups = (Cin + 16 * kBN - 1) / (16 * kBN);

    for (int t = 0; t < K2; ++t) {
        Tap g;
        if (pv) tap_geom<T>(a, p, b, ho, wo, t, g);
        else tap_none(g);
        float sm = 0.f, sy = 0.f, sx = 0.f;
        for (int cg = 0; cg < groups; ++cg) {
            const int ci0 = cg * 16 * kBN;
            f32x4 acc[kBN];
#pragma unroll
            for (int nt = 0; nt < kBN; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (sizeof(T) == 2) {
                const int nq = Cout >> 3;
                for (int q0 = 0; q0 < nq; q0 += 4) {
                    const int q = q0 + q4;
                    const bool qv = q < nq;
                    uint4 bf = zero4();
                    if (qv && pv) bf = *(const uint4*)(dy + p * a.ldy + q * 8);
#pragma unroll
                    for (int nt = 0; nt < kBN; ++nt) {
                        const int row = ci0 + nt * 16 + pl;  // the input channel of the A fragment
                        uint4 af = zero4();
                        if (qv && row < Cin) {  // w[co = 8 q + j][t][ci = row], j = 0 .. 7
                            const bf16_t* wp = (const bf16_t*)w + ((long)(q * 8) * K2 + t) * Cin + row;
                            const long st = (long)K2 * Cin;
                            af.x = ld16(wp) | (ld16(wp + st) << 16);
                            af.y = ld16(wp + 2 * st) | (ld16(wp + 3 * st) << 16);
                            af.z = ld16(wp + 4 * st) | (ld16(wp + 5 * st) << 16);
                            af.w = ld16(wp + 6 * st) | (ld16(wp + 7 * st) << 16);
                        }
                        mma_bf16(af, bf, acc[nt]);
                    }
                }
            } else {
                if (pv) {
                    for (int co4 = 0; co4 < Cout; co4 += 4) {
                        float gv[4];
                        load4<float>((const float*)dy + p * a.ldy + co4, gv);
#pragma unroll
                        for (int nt = 0; nt < kBN; ++nt) {
                            const int r0 = ci0 + nt * 16 + q4 * 4;
                            if (r0 >= Cin) continue;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                float wv[4];  // w[co = co4 + j][t][ci = r0 .. r0 + 3]
                                load4<float>((const float*)w + ((long)(co4 + j) * K2 + t) * Cin + r0, wv);
#pragma unroll
                                for (int i = 0; i < 4; ++i) acc[nt][i] = fmaf(wv[i], gv[j], acc[nt][i]);
                            }
                        }
                    }
                }
            }
            if (pv) {
#pragma unroll
                for (int nt = 0; nt < kBN; ++nt) {
                    const int r0 = ci0 + nt * 16 + q4 * 4;
                    if (r0 >= Cin) continue;
                    float v[4][4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (g.px[c] >= 0) {
                            load4<T>(x + g.px[c] * a.ldx + r0, v[c]);
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float dc = acc[nt][i];
                        float smp = 0.f, dsy = 0.f, dsx = 0.f;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            smp = fmaf(g.w[c], v[c][i], smp);
                            dsy = fmaf(g.gy[c], v[c][i], dsy);
                            dsx = fmaf(g.gx[c], v[c][i], dsx);
                        }
                        sm = fmaf(dc, smp, sm), sy = fmaf(dc, dsy, sy), sx = fmaf(dc, dsx, sx);
                    }
                    if (a.plane) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (g.px[c] < 0) continue;
                            float* dst = a.plane + g.px[c] * (long)Cin + r0;
                            const float cw = g.m * g.w[c];
#pragma unroll
                            for (int i = 0; i < 4; ++i) atomicAdd(dst + i, cw * acc[nt][i]);
                        }
                    }
                }
            }
        }
        // the four q4 lanes of a pixel hold the shares of its channel quarters: a fixed butterfly (every lane takes part)
        sm += __shfl_xor(sm, 16, 64), sy += __shfl_xor(sy, 16, 64), sx += __shfl_xor(sx, 16, 64);
        sm += __shfl_xor(sm, 32, 64), sy += __shfl_xor(sy, 32, 64), sx += __shfl_xor(sx, 32, 64);
        if (pv && q4 == 0) {
            T* d_o = (T*)a.doff + p * a.lddo + 2 * t;
            d_o[0] = from_float<T>(g.m * sy);
            d_o[1] = from_float<T>(g.m * sx);
            if (a.dmsk) ((T*)a.dmsk)[p * a.lddm + t] = from_float<T>(g.dm * sm);
        }
    }
}

// dx (=|+=) the plane, rounded once to the storage type; one thread per 16-byte chunk of dx
template <typename T>
__global__ void __launch_bounds__(kT) deform_flush_kernel(const float* __restrict__ plane, T* __restrict__ dx, int lddx, int C,
                                                          long chunks, int accumulate) {
    constexpr int EPC = VecIO<T>::EPC;
    const long e = (long)blockIdx.x * kT + threadIdx.x;
    if (e >= chunks) return;
    const int cpr = C / EPC;
    const long pix = e / cpr;
    const int ch = (int)(e - pix * cpr);
    float v[EPC];
    const float4* src = (const float4*)(plane + pix * C + ch * EPC);
#pragma unroll
    for (int q = 0; q < EPC / 4; ++q) {
        const float4 f = src[q];
        v[4 * q] = f.x, v[4 * q + 1] = f.y, v[4 * q + 2] = f.z, v[4 * q + 3] = f.w;
    }
    T* dst = dx + pix * lddx + ch * EPC;
    if (accumulate) {
        float old[EPC];
        VecIO<T>::unpack(*(const uint4*)dst, old);
#pragma unroll
        for (int i = 0; i < EPC; ++i) v[i] += old[i];
    }
    *(uint4*)dst = VecIO<T>::pack(v);
}

// ---- filter gradient, stage 1: a wave owns (slab, tap t, 16 input channels ct, MT 16-row tiles of output channels cz) --------
template <typename T, int MT>
__global__ void __launch_bounds__(kT) deform_wgrad_kernel(const DArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.y * 4 + wave;
    if (item >= a.K2 * a.CT * a.CZ) return;
    const int t = item % a.K2, ct = (item / a.K2) % a.CT, cz = item / (a.K2 * a.CT);
    const int pl = lane & 15, q4 = lane >> 4;
    const int sl = blockIdx.x, Cin = a.Cin, Cout = a.Cout, K2 = a.K2;
    const T* x = (const T*)a.x;
    const T* dy = (const T*)a.y;
    const long p0 = (long)sl * a.pps;
    const long p1 = (p0 + a.pps < a.M) ? p0 + a.pps : a.M;
    const int col = ct * 16 + pl;  // the input channel of the B fragment / of the lane's outputs
    const bool colv = col < Cin;
    const int row0 = cz * MT * 16;
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (sizeof(T) == 2) {
        for (long pk = p0; pk < p1; pk += 32) {
            // the lane's 8 consecutive pixels: one decode, then steps along the row
            long b;
            int ho, wo;
            decode(pk + q4 * 8 < p1 ? pk + q4 * 8 : p0, a.Ho, a.Wo, b, ho, wo);
            uint32_t bh[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long pp = pk + q4 * 8 + j;
                bh[j] = 0;
                if (pp < p1 && colv) {
                    Tap g;
                    tap_geom<T>(a, pp, b, ho, wo, t, g);
                    float sv = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (g.px[c] >= 0) sv = fmaf(g.w[c] * g.m, (float)x[g.px[c] * a.ldx + col], sv);
                    bh[j] = bits16(sv);
                }
                if (++wo == a.Wo) {
                    wo = 0;
                    if (++ho == a.Ho) ho = 0, ++b;
                }
            }
            const uint4 bf = make_uint4(bh[0] | (bh[1] << 16), bh[2] | (bh[3] << 16), bh[4] | (bh[5] << 16), bh[6] | (bh[7] << 16));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = row0 + mt * 16 + pl;  // the output channel of the A fragment
                uint32_t ah[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long pp = pk + q4 * 8 + j;
                    ah[j] = (pp < p1 && row < Cout) ? ld16((const bf16_t*)dy + pp * a.ldy + row) : 0u;
                }
                const uint4 af = make_uint4(ah[0] | (ah[1] << 16), ah[2] | (ah[3] << 16), ah[4] | (ah[5] << 16), ah[6] | (ah[7] << 16));
                mma_bf16(af, bf, acc[mt]);
            }
        }
    } else {
        for (long pp = p0; pp < p1; ++pp) {  // (uniform over the wave: every lane walks the slab's pixels in order)
            long b;
            int ho, wo;
            decode(pp, a.Ho, a.Wo, b, ho, wo);
            Tap g;
            tap_geom<T>(a, pp, b, ho, wo, t, g);
            float sv = 0.f;
            if (colv) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (g.px[c] >= 0) sv = fmaf(g.w[c] * g.m, (float)x[g.px[c] * a.ldx + col], sv);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int r0 = row0 + mt * 16 + q4 * 4;
                if (r0 >= Cout) continue;
                float gv[4];
                load4<float>((const float*)dy + pp * a.ldy + r0, gv);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[mt][i] = fmaf(gv[i], sv, acc[mt][i]);
            }
        }
    }
    if (!colv) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int r0 = row0 + mt * 16 + q4 * 4;
        if (r0 >= Cout) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) a.part[(((long)sl * Cout + r0 + i) * K2 + t) * Cin + col] = acc[mt][i];
    }
}

// bias partials: a thread owns (slab, output channel) and adds the slab's pixels in order
template <typename T>
__global__ void __launch_bounds__(kT) deform_dbias_kernel(const DArgs a, float* partb) {
    const int co = blockIdx.y * kT + threadIdx.x, sl = blockIdx.x;
    if (co >= a.Cout) return;
    const long p0 = (long)sl * a.pps;
    const long p1 = (p0 + a.pps < a.M) ? p0 + a.pps : a.M;
    const T* dy = (const T*)a.y;
    float sum = 0.f;
    for (long pp = p0; pp < p1; ++pp) sum += (float)dy[pp * a.ldy + co];
    partb[(long)sl * a.Cout + co] = sum;
}

// stage 2: one owner per filter / bias element adds the slabs in slab order
__global__ void __launch_bounds__(kT) deform_wgrad_reduce_kernel(const float* part, float* dw, float* db, long n, int Cout, int S) {
    const long e = (long)blockIdx.x * kT + threadIdx.x;
    if (e < n) {
        float sum = 0.f;
        for (int sl = 0; sl < S; ++sl) sum += part[(long)sl * n + e];
        dw[e] += sum;
    } else if (db && e < n + Cout) {
        const float* partb = part + (long)S * n;
        float sum = 0.f;
        for (int sl = 0; sl < S; ++sl) sum += partb[(long)sl * Cout + (e - n)];
        db[e - n] += sum;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int check_geometry(DArgs& a, const char* who, int B, int H, int W, int Cin, int Cout, int k, int s, int p, int d, int act,
                   int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(k == 1 || k == 3, VT_ERR_UNSUPPORTED, "%s: kernel_size %d (1 or 3)", who, k);
    VT_REQUIRE(s == 1 || s == 2, VT_ERR_UNSUPPORTED, "%s: stride %d (1 or 2)", who, s);
    VT_REQUIRE(act == 0 || act == 1, VT_ERR_UNSUPPORTED, "%s: mask_act %d (0 identity, 1 sigmoid)", who, act);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(Cin > 0 && Cout > 0 && Cin % epc == 0 && Cout % epc == 0, VT_ERR_UNSUPPORTED,
               "%s: Cin=%d and Cout=%d must be positive multiples of %d (whole 16-byte chunks)", who, Cin, Cout, epc);
    VT_REQUIRE(B > 0 && H > 0 && W > 0 && p >= 0 && d >= 1, VT_ERR_INVALID, "%s: B=%d H=%d W=%d padding=%d dilation=%d", who, B, H, W,
               p, d);
    const long reach = (long)H + 2L * p - (long)d * (k - 1) - 1, reachw = (long)W + 2L * p - (long)d * (k - 1) - 1;
    VT_REQUIRE(reach >= 0 && reachw >= 0, VT_ERR_INVALID, "%s: a %dx%d map is smaller than the dilated kernel", who, H, W);
    a.B = B, a.H = H, a.W = W, a.Cin = Cin, a.Cout = Cout, a.k = k, a.K2 = k * k, a.s = s, a.p = p, a.d = d, a.act = act;
    a.Ho = (int)(reach / s) + 1, a.Wo = (int)(reachw / s) + 1;
    a.M = (long)B * a.Ho * a.Wo;
    const long cmax = Cin > Cout ? Cin : Cout;
    VT_REQUIRE((long)B * H * W < (1L << 30) && a.M < (1L << 30) && (long)B * H * W * cmax < (1L << 40) && a.M * cmax < (1L << 40),
               VT_ERR_UNSUPPORTED, "%s: map too large", who);
    VT_REQUIRE((long)p + (long)d * k + (long)s * (a.Ho > a.Wo ? a.Ho : a.Wo) < (1L << 24), VT_ERR_UNSUPPORTED,
               "%s: sampling positions beyond the exact range of f32", who);
    a.tiles = (int)((a.M + 15) / 16);
    return VT_OK;
}

int check_map(const char* who, const char* what, const void* p, int ld, int C, int dtype) {
    const int epc = vt_epc(dtype);
    VT_REQUIRE(p && vt_aligned16(p), VT_ERR_INVALID, "%s: %s is null or misaligned", who, what);
    VT_REQUIRE(ld >= C && ld % epc == 0, VT_ERR_INVALID, "%s: %s has pixel stride %d (needs >= %d, a multiple of %d)", who, what, ld,
               C, epc);
    return VT_OK;
}

// the offset / mask maps and their gradients are read and written element by element: any element-aligned slice will do
int check_side(const char* who, const char* what, const void* p, int ld, int C, int dtype) {
    VT_REQUIRE(p && ((uintptr_t)p % vt_elem_size(dtype)) == 0, VT_ERR_INVALID, "%s: %s is null or misaligned", who, what);
    VT_REQUIRE(ld >= C, VT_ERR_INVALID, "%s: %s has pixel stride %d (needs >= %d)", who, what, ld, C);
    return VT_OK;
}

void slab_plan(DArgs& a, int mt) {
    a.CT = (a.Cin + 15) / 16;
    a.CZ = (a.Cout + 16 * mt - 1) / (16 * mt);
    const long items = (long)a.K2 * a.CT * a.CZ, n = (long)a.Cout * a.K2 * a.Cin + a.Cout;
    long S = (2048 + items - 1) / items;
    const long by_pixels = (a.M + 63) / 64, by_bytes = (64L << 20) / (n * 4);
    if (S > by_pixels) S = by_pixels;
    if (S > by_bytes) S = by_bytes;
    if (S > 256) S = 256;
    if (S < 1) S = 1;
    const long pps = ((a.M + S - 1) / S + 31) / 32 * 32;
    a.pps = (int)pps;
    a.S = (int)((a.M + pps - 1) / pps);
}

// 16-row tiles a wave holds: the smallest of 1, 2, 4, 8, 16 that covers the rows
int tiles_held(int rows) {
    const int need = (rows + 15) / 16;
    int nt = 1;
    while (nt < need && nt < 16) nt *= 2;
    return nt;
}

#define VT_DEFORM_NT(NTV, ...)                                      \
    do {                                                            \
        switch (NTV) {                                              \
            case 1: { constexpr int NT = 1; __VA_ARGS__; } break;   \
            case 2: { constexpr int NT = 2; __VA_ARGS__; } break;   \
            case 4: { constexpr int NT = 4; __VA_ARGS__; } break;   \
            case 8: { constexpr int NT = 8; __VA_ARGS__; } break;   \
            default: { constexpr int NT = 16; __VA_ARGS__; } break; \
        }                                                           \
    } while (0)

}  // namespace

extern "C" {

int vt_deform_supported(int32_t k, int32_t stride, int32_t Cin, int32_t Cout, int32_t dtype) {
    if (dtype != VT_F32 && dtype != VT_BF16) return 0;
    const int epc = vt_epc(dtype);
    return (k == 1 || k == 3) && (stride == 1 || stride == 2) && Cin > 0 && Cout > 0 && Cin % epc == 0 && Cout % epc == 0;
}

int vt_deform_fwd(const void* x, int32_t ldx, const void* offset, int32_t ldo, const void* mask, int32_t ldm, const void* w,
                  const float* bias, void* y, int32_t ldy, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k,
                  int32_t stride, int32_t padding, int32_t dilation, int32_t mask_act, int32_t dtype, void* stream) {
    const char* who = "vt_deform_fwd";
    DArgs a;
    memset(&a, 0, sizeof(a));
    VT_TRY(check_geometry(a, who, B, H, W, Cin, Cout, k, stride, padding, dilation, mask_act, dtype));
    VT_TRY(check_map(who, "x", x, ldx, Cin, dtype));
    VT_TRY(check_map(who, "y", y, ldy, Cout, dtype));
    VT_TRY(check_side(who, "offset", offset, ldo, 2 * a.K2, dtype));
    if (mask) VT_TRY(check_side(who, "mask", mask, ldm, a.K2, dtype));
    VT_REQUIRE(w && vt_aligned16(w), VT_ERR_INVALID, "%s: the filter is null or misaligned", who);
    VT_REQUIRE(x != y, VT_ERR_INVALID, "%s: y aliases x", who);
    a.x = x, a.off = offset, a.msk = mask, a.w = w, a.bias = bias, a.y = y;
    a.ldx = ldx, a.ldo = ldo, a.ldm = ldm, a.ldy = ldy;
    const int nt = tiles_held(Cout);
    const dim3 grid((unsigned)((a.tiles + 3) / 4), (unsigned)((Cout + 16 * nt - 1) / (16 * nt)));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VT_BF16) VT_DEFORM_NT(nt, hipLaunchKernelGGL((deform_fwd_kernel<bf16_t, NT>), grid, dim3(kT), 0, st, a));
    else VT_DEFORM_NT(nt, hipLaunchKernelGGL((deform_fwd_kernel<float, NT>), grid, dim3(kT), 0, st, a));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_deform_bwd(const void* dy, int32_t lddy, const void* x, int32_t ldx, const void* offset, int32_t ldo, const void* mask,
                  int32_t ldm, const void* w, void* doffset, int32_t lddo, void* dmask, int32_t lddm, void* dx, int32_t lddx,
                  int32_t accumulate, float* plane, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k,
                  int32_t stride, int32_t padding, int32_t dilation, int32_t mask_act, int32_t dtype, void* stream) {
    const char* who = "vt_deform_bwd";
    DArgs a;
    memset(&a, 0, sizeof(a));
    VT_TRY(check_geometry(a, who, B, H, W, Cin, Cout, k, stride, padding, dilation, mask_act, dtype));
    VT_TRY(check_map(who, "dy", dy, lddy, Cout, dtype));
    VT_TRY(check_map(who, "x", x, ldx, Cin, dtype));
    VT_TRY(check_side(who, "offset", offset, ldo, 2 * a.K2, dtype));
    VT_TRY(check_side(who, "doffset", doffset, lddo, 2 * a.K2, dtype));
    if (mask) {
        VT_TRY(check_side(who, "mask", mask, ldm, a.K2, dtype));
        VT_TRY(check_side(who, "dmask", dmask, lddm, a.K2, dtype));
    }
    VT_REQUIRE(w && vt_aligned16(w), VT_ERR_INVALID, "%s: the filter is null or misaligned", who);
    if (dx) {
        VT_TRY(check_map(who, "dx", dx, lddx, Cin, dtype));
        VT_REQUIRE(plane && vt_aligned16(plane), VT_ERR_INVALID, "%s: d(x) needs the f32 plane [B][H][W][Cin] (null or misaligned)",
                   who);
        VT_REQUIRE(dx != x && dx != dy, VT_ERR_INVALID, "%s: dx aliases an input", who);
    }
    a.x = x, a.off = offset, a.msk = mask, a.w = w, a.y = const_cast<void*>(dy), a.doff = doffset, a.dmsk = mask ? dmask : nullptr;
    a.plane = dx ? plane : nullptr;
    a.ldx = ldx, a.ldo = ldo, a.ldm = ldm, a.ldy = lddy, a.lddo = lddo, a.lddm = lddm;
    hipStream_t st = (hipStream_t)stream;
    const long nplane = (long)B * H * W * Cin;
    if (dx) {
        const hipError_t e = hipMemsetAsync(plane, 0, (size_t)nplane * 4, st);
        VT_REQUIRE(e == hipSuccess, VT_ERR_HIP, "%s: clearing the plane failed: %s", who, hipGetErrorString(e));
    }
    const dim3 grid((unsigned)((a.tiles + 3) / 4));
    if (dtype == VT_BF16) hipLaunchKernelGGL(deform_bwd_kernel<bf16_t>, grid, dim3(kT), 0, st, a);
    else hipLaunchKernelGGL(deform_bwd_kernel<float>, grid, dim3(kT), 0, st, a);
    VT_CHECK_LAUNCH(who);
    if (dx) {
        const long chunks = nplane / vt_epc(dtype);
        const dim3 fgrid((unsigned)((chunks + kT - 1) / kT));
        if (dtype == VT_BF16)
            hipLaunchKernelGGL(deform_flush_kernel<bf16_t>, fgrid, dim3(kT), 0, st, plane, (bf16_t*)dx, lddx, Cin, chunks,
                               accumulate != 0);
        else
            hipLaunchKernelGGL(deform_flush_kernel<float>, fgrid, dim3(kT), 0, st, plane, (float*)dx, lddx, Cin, chunks,
                               accumulate != 0);
        VT_CHECK_LAUNCH("vt_deform_bwd (flush)");
    }
    return VT_OK;
}

int64_t vt_deform_wgrad_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k, int32_t stride,
                                      int32_t padding, int32_t dilation) {
    DArgs a;
    memset(&a, 0, sizeof(a));
    // (f32 admits every channel count the bf16 path does)
    if (check_geometry(a, "vt_deform_wgrad_scratch_bytes", B, H, W, Cin, Cout, k, stride, padding, dilation, 0, VT_F32) != VT_OK)
        return -1;
    slab_plan(a, tiles_held(Cout));
    return (int64_t)a.S * ((int64_t)Cout * a.K2 * Cin + Cout) * 4;
}

int vt_deform_wgrad(const void* dy, int32_t lddy, const void* x, int32_t ldx, const void* offset, int32_t ldo, const void* mask,
                    int32_t ldm, float* dw, float* dbias, void* scratch, int64_t scratch_bytes, int32_t B, int32_t H, int32_t W,
                    int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t padding, int32_t dilation, int32_t mask_act,
                    int32_t dtype, void* stream) {
    const char* who = "vt_deform_wgrad";
    DArgs a;
    memset(&a, 0, sizeof(a));
    VT_TRY(check_geometry(a, who, B, H, W, Cin, Cout, k, stride, padding, dilation, mask_act, dtype));
    VT_TRY(check_map(who, "dy", dy, lddy, Cout, dtype));
    VT_TRY(check_map(who, "x", x, ldx, Cin, dtype));
    VT_TRY(check_side(who, "offset", offset, ldo, 2 * a.K2, dtype));
    if (mask) VT_TRY(check_side(who, "mask", mask, ldm, a.K2, dtype));
    VT_REQUIRE(dw && scratch && vt_aligned16(scratch), VT_ERR_INVALID, "%s: dw or scratch is null or misaligned", who);
    const int mt = tiles_held(Cout);
    slab_plan(a, mt);
    const long n = (long)Cout * a.K2 * Cin;
    const int64_t need = (int64_t)a.S * (n + Cout) * 4;
    VT_REQUIRE(scratch_bytes >= need, VT_ERR_INVALID, "%s: scratch of %lld bytes, needs %lld", who, (long long)scratch_bytes,
               (long long)need);
    a.x = x, a.off = offset, a.msk = mask, a.y = const_cast<void*>(dy), a.part = (float*)scratch;
    a.ldx = ldx, a.ldo = ldo, a.ldm = ldm, a.ldy = lddy;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)a.S, (unsigned)((a.K2 * a.CT * a.CZ + 3) / 4));
    if (dtype == VT_BF16) VT_DEFORM_NT(mt, hipLaunchKernelGGL((deform_wgrad_kernel<bf16_t, NT>), grid, dim3(kT), 0, st, a));
    else VT_DEFORM_NT(mt, hipLaunchKernelGGL((deform_wgrad_kernel<float, NT>), grid, dim3(kT), 0, st, a));
    VT_CHECK_LAUNCH(who);
    if (dbias) {
        float* partb = a.part + (long)a.S * n;
        const dim3 bgrid((unsigned)a.S, (unsigned)((Cout + kT - 1) / kT));
        if (dtype == VT_BF16) hipLaunchKernelGGL(deform_dbias_kernel<bf16_t>, bgrid, dim3(kT), 0, st, a, partb);
        else hipLaunchKernelGGL(deform_dbias_kernel<float>, bgrid, dim3(kT), 0, st, a, partb);
        VT_CHECK_LAUNCH("vt_deform_wgrad (bias)");
    }
    hipLaunchKernelGGL(deform_wgrad_reduce_kernel, dim3((unsigned)((n + Cout + kT - 1) / kT)), dim3(kT), 0, st,
                       (const float*)scratch, dw, dbias, n, Cout, a.S);
    VT_CHECK_LAUNCH("vt_deform_wgrad (reduce)");
    return VT_OK;
}

}  // extern "C"
