// vt_trivial_augment.hip -- TrivialAugmentWide (the third stage of the reference's training transform) on 8-bit levels:
//
//   uint8 [B][S_h][S_w][3] levels (vt_augment_batch_u8)  +  the table ta f64 [B][8] = (op, m0..m5, arg)
//     ->  one of 14 ops per image, computed level for level as PIL computes it on an 8-bit RGB image
//     ->  float32(level) * (1/255) [-> (v - mean) / std] -> erase  ->  float32 [B][3][S_h][S_w]
//
// The definition of every op is in vt_amd.h (vt_trivial_augment).  Two kernels behind one entry:
//
//   statistics  only for the images whose op needs the whole image: Contrast (the histogram of the gray levels, for their
//               mean), AutoContrast and Equalize (the three channel histograms).  A workgroup owns (image, chunk of 8192
//               pixels), counts into LDS with integer atomics and adds its non-zero bins to workspace[b][4][256] (cleared
//               inside the call) with integer atomics.  Integer sums do not depend on the order: repeated launches are
//               bit-identical.  Workgroups of the other images return at once.
//   apply       a workgroup of 256 threads owns (image, band of <= 32 rows, tile of <= 256 columns) and branches ONCE on
//               the image's op (uniform over the workgroup, so every barrier is reached by all or by none):
//                 Identity                          copy
//                 Brightness, Color, Contrast       blend per level; Contrast's mean is reduced from the gray histogram
//                                                   into LDS once (a 64-bit integer sum, one f64 division)
//                 Sharpness                         the tile and a one-pixel halo are staged in LDS, SMOOTH is integer
//                 Posterize, Solarize, AutoContrast, Equalize   a [3][256] table of levels is built in LDS once (Equalize:
//                                                   a scan of the histograms over the workgroup), then one lookup a level
//                 ShearX/Y, TranslateX/Y, Rotate    a bilinear gather from the levels in global memory (L2: an image is
//                                                   <= a few hundred KB) with f64 coordinates and f64 interpolation
//               then the shared epilogue, which writes every output element once, contiguous along x in each plane.
//
// ROUNDING.  PIL's results are fixed by the order of its float operations, so nothing here may be contracted into an FMA:
// the whole file is compiled with fp contract off, and the operations stand in PIL's order.
//
// SAFETY.  A table on the device is not validated.  op is read as a number: in [0, 14) it is truncated, anything else (NaN
// included) is Identity.  Posterize's bit count is truncated and clamped into 1 .. 8 (NaN: 1).  Table lookups index with
// a uint8.  The affine gather tests 0 <= xin < S_w, 0 <= yin < S_h with comparisons that are false for a NaN before a
// coordinate becomes an index, and clamps the four neighbours into the image.  A factor or threshold that is not a number
// gives unspecified LEVELS, never an address.
#include "vt_augment_erase.h"
#include "vt_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kTileW = 256;       // columns of a tile
constexpr int kTileR = 32;        // rows of a band
constexpr int kStatPixels = 8192; // pixels of a statistics chunk
constexpr int kOps = 14;

enum { OP_IDENTITY = 0, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST,
       OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE };

struct TaGeo {
    int B, Sh, Sw;
    int R, CW, bandsY, tilesX;
    int chunks;  // statistics chunks of an image
};

__device__ __forceinline__ int ta_op(const double* row) {
    const double o = row[0];
    return (o >= 0.0 && o < (double)kOps) ? (int)o : OP_IDENTITY;
}

__device__ __forceinline__ int gray_level(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// PIL's blend of 8-bit levels: deg + f (a - deg) in f32, a product and then a sum; clipped, truncated
__device__ __forceinline__ int blend(int deg, int a, float f) {
    const float d = (float)deg;
    const float p = f * ((float)a - d);
    const float t = d + p;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__global__ __launch_bounds__(kT) void ta_stats_kernel(const uint8_t* __restrict__ u8, const double* __restrict__ ta,
                                                      uint32_t* __restrict__ work, TaGeo g) {
    __shared__ uint32_t hist[4 * 256];
    const int t = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)g.chunks), ch = (int)(blockIdx.x % (unsigned)g.chunks);
    const int op = ta_op(ta + 8 * (long long)b);
    if (op != OP_CONTRAST && op != OP_AUTOCONTRAST && op != OP_EQUALIZE) return;  // (uniform over the workgroup)
    for (int i = t; i < 4 * 256; i += kT) hist[i] = 0u;
    __syncthreads();
    const long long npix = (long long)g.Sh * g.Sw;
    const long long p0 = (long long)ch * kStatPixels, p1 = min(npix, p0 + kStatPixels);
    const uint8_t* img = u8 + (long long)b * npix * 3;
    if (op == OP_CONTRAST) {
        for (long long p = p0 + t; p < p1; p += kT) {
            const uint8_t* q = img + 3 * p;
            atomicAdd(&hist[768 + gray_level(q[0], q[1], q[2])], 1u);
        }
    } else {
        for (long long p = p0 + t; p < p1; p += kT) {
            const uint8_t* q = img + 3 * p;
            atomicAdd(&hist[q[0]], 1u);
            atomicAdd(&hist[256 + q[1]], 1u);
            atomicAdd(&hist[512 + q[2]], 1u);
        }
    }
    __syncthreads();
    uint32_t* w = work + (long long)b * 1024;
    for (int i = t; i < 4 * 256; i += kT)
        if (hist[i]) atomicAdd(&w[i], hist[i]);
}

struct Epilogue {
    float* outb;
    const float* mean_std;
    long long ei, ej, eh, ew;
    int Sh, Sw, mode;
    uint32_t seed, b;
    float cval;
    bool erase;

    // float32(level) / 255 -> mean / std -> erase, the three planes of output pixel (Y, X)
    __device__ __forceinline__ void store(int Y, int X, int l0, int l1, int l2) const {
        const bool inbox = erase && Y >= ei && Y < ei + eh && X >= ej && X < ej + ew;
        const int l[3] = {l0, l1, l2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (float)l[c] * (1.0f / 255.0f);
            if (mean_std) v = (v - mean_std[c]) / mean_std[3 + c];
            if (inbox) v = mode == 1 ? cval : erase_normal(seed, b, (uint32_t)c, (uint32_t)Y, (uint32_t)X);
            outb[((long long)c * Sh + Y) * Sw + X] = v;
        }
    }
};

__global__ __launch_bounds__(kT) void ta_apply_kernel(const uint8_t* __restrict__ u8, const double* __restrict__ ta,
                                                      const int* __restrict__ params, float* __restrict__ out,
                                                      const uint32_t* __restrict__ work, const float* __restrict__ mean_std,
                                                      TaGeo g) {
    __shared__ uint32_t scan[3 * 256];
    __shared__ uint8_t lut[3 * 256];
    __shared__ uint8_t stage[(kTileR + 2) * (kTileW + 2) * 3];
    __shared__ int s_lo[3], s_hi[3], s_nz[3];
    __shared__ uint32_t s_last[3];
    __shared__ unsigned long long s_sum;
    __shared__ int s_mean;

    const int t = threadIdx.x;
    const unsigned L = blockIdx.x;
    const int tx = (int)(L % (unsigned)g.tilesX);
    const int by = (int)((L / (unsigned)g.tilesX) % (unsigned)g.bandsY);
    const int b = (int)(L / ((unsigned)g.tilesX * (unsigned)g.bandsY));
    const int Sh = g.Sh, Sw = g.Sw;
    const int Y0 = by * g.R, X0 = tx * g.CW;
    const int Rb = min(g.R, Sh - Y0), Cb = min(g.CW, Sw - X0);
    const int npx = Rb * Cb;
    const long long npix = (long long)Sh * Sw;
    const uint8_t* img = u8 + (long long)b * npix * 3;
    const double* row = ta + 8 * (long long)b;
    const int op = ta_op(row);
    const double arg = row[7];
    const uint32_t* hb = work + (long long)b * 1024;

    const int* p = params + 16 * (long long)b;
    Epilogue e;
    e.outb = out + (long long)b * 3 * npix;
    e.mean_std = mean_std;
    e.ei = p[9], e.ej = p[10], e.eh = p[11], e.ew = p[12];
    e.Sh = Sh, e.Sw = Sw, e.mode = p[13];
    e.seed = (uint32_t)p[14], e.b = (uint32_t)b;
    e.cval = __int_as_float(p[15]);
    e.erase = (e.mode == 1 || e.mode == 2) && e.eh > 0 && e.ew > 0;

    switch (op) {
    case OP_SHEAR_X:
    case OP_SHEAR_Y:
    case OP_TRANSLATE_X:
    case OP_TRANSLATE_Y:
    case OP_ROTATE: {
        const double m0 = row[1], m1 = row[2], m2 = row[3], m3 = row[4], m4 = row[5], m5 = row[6];
        for (int i = t; i < npx; i += kT) {
            const int r = i / Cb, Y = Y0 + r, X = X0 + i - r * Cb;
            const double xc = (double)X + 0.5, yc = (double)Y + 0.5;
            double xin = m0 * xc + m1 * yc + m2;
            double yin = m3 * xc + m4 * yc + m5;
            int l[3] = {0, 0, 0};
            if (xin >= 0.0 && xin < (double)Sw && yin >= 0.0 && yin < (double)Sh) {
                xin -= 0.5, yin -= 0.5;
                const double xf = floor(xin), yf = floor(yin);
                const double dx = xin - xf, dy = yin - yf;
                const int xi = (int)xf, yi = (int)yf;  // in [-1, S - 1]
                const int xa = max(xi, 0), xb = min(xi + 1, Sw - 1), ya = max(yi, 0), yb = min(yi + 1, Sh - 1);
                const uint8_t* q00 = img + ((long long)ya * Sw + xa) * 3;
                const uint8_t* q01 = img + ((long long)ya * Sw + xb) * 3;
                const uint8_t* q10 = img + ((long long)yb * Sw + xa) * 3;
                const uint8_t* q11 = img + ((long long)yb * Sw + xb) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double p00 = (double)q00[c], p01 = (double)q01[c], p10 = (double)q10[c], p11 = (double)q11[c];
                    const double v1 = p00 + (p01 - p00) * dx;
                    const double v2 = p10 + (p11 - p10) * dx;
                    l[c] = (int)(v1 + (v2 - v1) * dy);
                }
            }
            e.store(Y, X, l[0], l[1], l[2]);
        }
        return;
    }
    case OP_BRIGHTNESS:
    case OP_COLOR:
    case OP_CONTRAST: {
        const float f = (float)arg;
        int mean = 0;
        if (op == OP_CONTRAST) {  // mean of the gray levels from their histogram: an integer sum, one f64 division
            if (t == 0) s_sum = 0ull;
            __syncthreads();
            const unsigned long long part = (unsigned long long)t * hb[768 + t];
            if (part) atomicAdd(&s_sum, part);
            __syncthreads();
            if (t == 0) s_mean = (int)((double)s_sum / (double)npix + 0.5);
            __syncthreads();
            mean = s_mean;
        }
        for (int i = t; i < npx; i += kT) {
            const int r = i / Cb, Y = Y0 + r, X = X0 + i - r * Cb;
            const uint8_t* q = img + ((long long)Y * Sw + X) * 3;
            const int a0 = q[0], a1 = q[1], a2 = q[2];
            const int deg = op == OP_BRIGHTNESS ? 0 : (op == OP_COLOR ? gray_level(a0, a1, a2) : mean);
            e.store(Y, X, blend(deg, a0, f), blend(deg, a1, f), blend(deg, a2, f));
        }
        return;
    }
    case OP_SHARPNESS: {
        const float f = (float)arg;
        const int sw3 = (Cb + 2) * 3;  // bytes of a staged row: columns X0 - 1 .. X0 + Cb, clamped into the image
        for (int i = t; i < (Rb + 2) * sw3; i += kT) {
            const int rr = i / sw3, k = i - rr * sw3, col = k / 3, c = k - 3 * col;
            const int Ys = min(max(Y0 - 1 + rr, 0), Sh - 1), Xs = min(max(X0 - 1 + col, 0), Sw - 1);
            stage[i] = img[((long long)Ys * Sw + Xs) * 3 + c];
        }
        __syncthreads();
        for (int i = t; i < npx; i += kT) {
            const int r = i / Cb, x = i - r * Cb, Y = Y0 + r, X = X0 + x;
            const uint8_t* s = stage + (r + 1) * sw3 + (x + 1) * 3;
            const bool inner = X >= 1 && X <= Sw - 2 && Y >= 1 && Y <= Sh - 2;
            int l[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int a = s[c];
                int deg = a;
                if (inner) {  // SMOOTH: (3 x 3 sum + 4 centre) / 13, rounded half up
                    const int sum = s[c - sw3 - 3] + s[c - sw3] + s[c - sw3 + 3] + s[c - 3] + 5 * a + s[c + 3] + s[c + sw3 - 3] +
                                    s[c + sw3] + s[c + sw3 + 3];
                    deg = (2 * sum + 13) / 26;
                }
                l[c] = blend(deg, a, f);
            }
            e.store(Y, X, l[0], l[1], l[2]);
        }
        return;
    }
    case OP_POSTERIZE:
    case OP_SOLARIZE:
    case OP_AUTOCONTRAST:
    case OP_EQUALIZE: {
        // thread t builds entry t of the three channel tables
        if (op == OP_POSTERIZE) {
            const int k = !(arg >= 1.0) ? 1 : (arg > 8.0 ? 8 : (int)arg);
            const int v = t & (256 - (1 << (8 - k)));
            lut[t] = lut[256 + t] = lut[512 + t] = (uint8_t)v;
        } else if (op == OP_SOLARIZE) {
            const int v = (double)t < arg ? t : 255 - t;
            lut[t] = lut[256 + t] = lut[512 + t] = (uint8_t)v;
        } else {
            if (t < 3) s_lo[t] = 256, s_hi[t] = -1, s_nz[t] = 0;
            __syncthreads();
            uint32_t h[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                h[c] = hb[c * 256 + t];
                if (h[c]) {
                    atomicMin(&s_lo[c], t);
                    atomicMax(&s_hi[c], t);
                    atomicAdd(&s_nz[c], 1);
                }
            }
            __syncthreads();
            if (op == OP_AUTOCONTRAST) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int lo = s_lo[c], hi = s_hi[c];
                    int v = t;
                    if (hi > lo) {
                        const double scale = 255.0 / (double)(hi - lo);
                        const double offset = (double)(-lo) * scale;
                        const double x = (double)t * scale + offset;  // in (-256, 511): the conversion is exact truncation
                        const int ix = (int)x;
                        v = ix < 0 ? 0 : (ix > 255 ? 255 : ix);
                    }
                    lut[c * 256 + t] = (uint8_t)v;
                }
            } else {
                // inclusive scan of the three histograms over the workgroup (Hillis-Steele, 8 steps)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    scan[c * 256 + t] = h[c];
                    if (t == s_hi[c]) s_last[c] = h[c];
                }
                __syncthreads();
                for (int off = 1; off < 256; off <<= 1) {
                    uint32_t v[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = t >= off ? scan[c * 256 + t - off] : 0u;
                    __syncthreads();
#pragma unroll
                    for (int c = 0; c < 3; ++c) scan[c * 256 + t] += v[c];
                    __syncthreads();
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t before = scan[c * 256 + t] - h[c];  // pixels of the levels below t
                    const uint32_t step = s_nz[c] > 1 ? ((uint32_t)npix - s_last[c]) / 255u : 0u;
                    uint32_t v = (uint32_t)t;
                    if (step) {
                        v = (step / 2u + before) / step;
                        v = v > 255u ? 255u : v;
                    }
                    lut[c * 256 + t] = (uint8_t)v;
                }
            }
        }
        __syncthreads();
        for (int i = t; i < npx; i += kT) {
            const int r = i / Cb, Y = Y0 + r, X = X0 + i - r * Cb;
            const uint8_t* q = img + ((long long)Y * Sw + X) * 3;
            e.store(Y, X, lut[q[0]], lut[256 + q[1]], lut[512 + q[2]]);
        }
        return;
    }
    default:
        for (int i = t; i < npx; i += kT) {
            const int r = i / Cb, Y = Y0 + r, X = X0 + i - r * Cb;
            const uint8_t* q = img + ((long long)Y * Sw + X) * 3;
            e.store(Y, X, q[0], q[1], q[2]);
        }
        return;
    }
}

}  // namespace

extern "C" {

int vt_trivial_augment(const uint8_t* u8, const double* ta, const int32_t* params, float* out, uint32_t* workspace, int32_t B,
                       int32_t S_h, int32_t S_w, const float* mean_std, void* stream) {
    const char* who = "vt_trivial_augment";
    VT_REQUIRE(u8 && ta && params && out && workspace, VT_ERR_INVALID,
               "%s: null pointer (u8 %p, ta %p, params %p, out %p, workspace %p)", who, (const void*)u8, (const void*)ta,
               (const void*)params, (const void*)out, (const void*)workspace);
    VT_REQUIRE(B > 0 && S_h > 0 && S_w > 0, VT_ERR_INVALID, "%s: non-positive size (B %d, S_h %d, S_w %d)", who, B, S_h, S_w);
    VT_REQUIRE((long)S_h * S_w < (1L << 31), VT_ERR_INVALID, "%s: %ld pixels an image (the histograms count in 32 bits)", who,
               (long)S_h * S_w);
    VT_REQUIRE((((uintptr_t)ta) & 7) == 0 && (((uintptr_t)params) & 3) == 0 && (((uintptr_t)out) & 3) == 0 &&
                   (((uintptr_t)workspace) & 3) == 0 && (((uintptr_t)mean_std) & 3) == 0,
               VT_ERR_INVALID, "%s: misaligned ta (8), params, out, workspace or mean_std (4)", who);
    TaGeo g;
    g.B = B, g.Sh = S_h, g.Sw = S_w;
    g.CW = S_w < kTileW ? S_w : kTileW;
    g.R = S_h < kTileR ? S_h : kTileR;
    g.bandsY = (S_h + g.R - 1) / g.R, g.tilesX = (S_w + g.CW - 1) / g.CW;
    g.chunks = (int)(((long)S_h * S_w + kStatPixels - 1) / kStatPixels);
    const long blocks = (long)B * g.bandsY * g.tilesX, sblocks = (long)B * g.chunks;
    VT_REQUIRE(blocks < (1L << 31) && sblocks < (1L << 31), VT_ERR_INVALID, "%s: %ld and %ld workgroups", who, sblocks, blocks);
    const hipError_t me = hipMemsetAsync(workspace, 0, (size_t)B * 4 * 256 * sizeof(uint32_t), (hipStream_t)stream);
    VT_REQUIRE(me == hipSuccess, VT_ERR_HIP, "%s: clearing the workspace failed: %s", who, hipGetErrorString(me));
    hipLaunchKernelGGL(ta_stats_kernel, dim3((unsigned)sblocks), dim3(kT), 0, (hipStream_t)stream, u8, ta, workspace, g);
    VT_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ta_apply_kernel, dim3((unsigned)blocks), dim3(kT), 0, (hipStream_t)stream, u8, ta, (const int*)params, out,
                       (const uint32_t*)workspace, mean_std, g);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // extern "C"
