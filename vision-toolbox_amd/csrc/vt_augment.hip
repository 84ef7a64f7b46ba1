// vt_augment.hip -- the training / validation input transform of the reference's data pipeline on the device:
//
//   uint8 HWC images of different sizes (one packed buffer)  ->  float32 [B][3][S_h][S_w]
//   crop box -> separable triangle (bilinear, optionally antialiased) resize to a virtual (OH, OW) image -> the
//   (S_h, S_w) window at (oy, ox) of it -> horizontal flip -> 1/255 [-> (v - mean) / std] -> erase
//
// ONE launch for the whole ragged batch.  All geometry is per image and read from device tables (vt_amd.h), the grid
// depends on (B, S_h, S_w) only: a captured graph follows new tables.
//
// THE FILTER.  Along an axis with n source pixels and `out` virtual pixels, output i has the centre c = n (i + 0.5) / out
// and the support S = max(n / out, 1) (antialias) or 1 (plain two-tap bilinear).  Its taps are the j of
// [max(int(c - S + 0.5), 0), min(int(c + S + 0.5), n)) with the weight max(0, 1 - |j + 0.5 - c| / S) over the sum of the
// weights.  Everything that decides a tap is INTEGER arithmetic on the numerators over the common denominator 2 out:
// with sup = S out (an integer: max(n, out) or out) and c2 = n (2 i + 1),
//   first = max(floor((c2 - 2 sup + out) / (2 out)), 0), last = min(floor((c2 + 2 sup + out) / (2 out)), n),
//   weight_j = max(0, 1 - |a_j| / (2 sup)),  a_j = 2 out j + out - c2  (|a_j| <= 2 sup + 2 out: exact as an int, one
//   rounding as a float) -- no f32 rounding of a coordinate of a few hundred pixels ever reaches a weight.
// A tap whose weight is zero may be in or out of the range depending on how the bounds round; that changes nothing.
//
// THE PLAN.  A workgroup of 256 threads owns (image, band of R output rows, tile of CW <= 256 output columns).
//   tables      each output column / row of the tile gets (first tap, tap count, a_first, 1 / weight sum) in LDS, once.
//   horizontal  for the source rows the band needs, each output column's taps are summed for the three channels straight
//               from the uint8 HWC row into an f32 plane [row][channel][column] in LDS.
//   vertical    a thread owns one column and up to 8 rows x 3 channels of outputs in registers and adds the plane's rows
//               in ascending order; then flip (already in the column table), scale, mean/std, erase, and NCHW stores that
//               are contiguous along x inside each channel plane.
// The plane holds `rows_cap` source rows (from the LDS budget).  A band that needs more (a large downscale factor) runs
// in several chunks of source rows with the same accumulators: the summation order of an output does not depend on the
// chunking, so every LDS budget gives the same bits.  No atomics; repeated launches are bit-identical.
//
// SAFETY.  The image table (byte offset, H, W) is trusted: it is what says where an image is.  Everything in `params`
// is clamped into its image before it forms an address: top / left into the image, h / w into what is left of it, the
// virtual index into [0, OH) x [0, OW), taps into [0, n).  Loads are single bytes, so nothing is read past an image's
// last byte whatever its alignment.
//
// THE ERASE GENERATOR (part of the interface, restated in numpy by the tests).  mix(x): x ^= x >> 16; x *= 0x7feb352d;
// x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (32-bit).  k = mix(seed + 0x9e3779b9); k = mix(k + b); k = mix(k + c);
// k = mix(k + y); k = mix(k + x) with (b, c, y, x) the OUTPUT coordinates; h1 = mix(k ^ 0x68bc21eb), h2 = mix(k ^
// 0x02e5be93); u1 = ((h1 >> 8) + 1) 2^-24 in (0, 1], u2 = (h2 >> 8) 2^-24 in [0, 1);
// z = sqrtf(-2 logf(u1)) * cosf(6.2831855f * u2) with the accurate f32 functions.  (vt_augment_erase.h, shared with
// vt_trivial_augment.hip.)
//
// THE 8-BIT ENTRY.  vt_augment_batch_u8 is the same kernel body with another epilogue (template parameter U8): the levels
// that TrivialAugmentWide works on, uint8 [B][S_h][S_w][3].
#include <type_traits>

#include "vt_augment_erase.h"
#include "vt_common.h"

namespace {

constexpr int kT = 256;
constexpr int kRowsPerThread = 8;
constexpr int kMaxCW = 256;       // output columns of a tile (one thread per column in the vertical pass)
constexpr int kMaxThreadRows = 32;
constexpr int kMaxDim = 1 << 20;  // crop sides and virtual sizes are clamped to this: a_j stays an int
constexpr int kDefaultLds = 64 * 1024;
constexpr int kMaxLds = 160 * 1024;

struct AxisTap {
    int first, count, a0;
    float inv;
};
static_assert(sizeof(AxisTap) == 16, "one 16-byte LDS slot");

struct AugGeo {
    int B, Sh, Sw;
    int R, CW, trows;      // rows of a band, columns of a tile, thread rows (256 / CW, at most kMaxThreadRows)
    int bandsY, tilesX;
    int rows_cap;          // source rows the LDS plane holds
    int antialias;
};

__device__ __forceinline__ int clampi(long long v, long long lo, long long hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

__device__ __forceinline__ float tri(int a, float inv2sup) { return fmaxf(0.0f, 1.0f - fabsf((float)a) * inv2sup); }

// taps of virtual output i in [0, out) over n source pixels; sup = support * out
__device__ AxisTap axis_tap(int i, int n, int out, int sup) {
    const long long c2 = (long long)n * (2 * i + 1);
    const long long d = 2LL * out;
    const long long lo = c2 - 2LL * sup + out;
    long long first = lo > 0 ? lo / d : 0;
    long long last = (c2 + 2LL * sup + out) / d;
    if (last > n) last = n;
    if (first > last - 1) first = last - 1;  // (cannot happen for i in [0, out); keeps count >= 1 whatever comes in)
    if (first < 0) first = 0;
    AxisTap t;
    t.first = (int)first;
    t.count = (int)(last - first);
    t.a0 = (int)(d * first + out - c2);
    const float inv2sup = 1.0f / (2.0f * (float)sup);
    float sum = 0.0f;
    for (int k = 0; k < t.count; ++k) sum += tri(t.a0 + 2 * out * k, inv2sup);
    t.inv = sum > 0.0f ? 1.0f / sum : 0.0f;
    return t;
}

// U8 = false: the float32 NCHW batch (vt_augment_batch).  U8 = true: the EPILOGUE alone changes -- the filtered value on the
// 0 .. 255 scale is rounded half up to a level and stored as uint8 [B][S_h][S_w][3], without 1/255, mean / std or erase
// (vt_augment_batch_u8, the input of vt_trivial_augment).
template <bool U8>
__global__ __launch_bounds__(kT) void augment_kernel(const uint8_t* __restrict__ raw, const long long* __restrict__ table,
                                                     const int* __restrict__ params, std::conditional_t<U8, uint8_t, float>* __restrict__ out,
                                                     const float* __restrict__ mean_std, AugGeo g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    AxisTap* colt = (AxisTap*)smem;                  // [CW]
    AxisTap* rowt = colt + g.CW;                     // [R]
    float* plane = (float*)(rowt + g.R);             // [rows_cap][3][CW]

    const int t = threadIdx.x;
    const unsigned L = blockIdx.x;
    const int tx = (int)(L % (unsigned)g.tilesX);
    const int by = (int)((L / (unsigned)g.tilesX) % (unsigned)g.bandsY);
    const int b = (int)(L / ((unsigned)g.tilesX * (unsigned)g.bandsY));

    const int Y0 = by * g.R, X0 = tx * g.CW;
    const int Rb = min(g.R, g.Sh - Y0), Cb = min(g.CW, g.Sw - X0);
    const int x = t % g.CW, tr = t / g.CW;
    const bool active = tr < g.trows && x < Cb;
    auto* outb = out + (long long)b * 3 * g.Sh * g.Sw;

    const long long off = table[3 * b], Hl = table[3 * b + 1], Wl = table[3 * b + 2];
    if (Hl < 1 || Wl < 1 || off < 0) {  // no image: zeros (uniform over the workgroup, in front of every barrier)
        for (int m = 0; m < kRowsPerThread; ++m) {
            const int r = tr + g.trows * m;
            if (active && r < Rb)
                for (int c = 0; c < 3; ++c) {
                    if constexpr (U8)
                        outb[((long long)(Y0 + r) * g.Sw + X0 + x) * 3 + c] = 0;
                    else
                        outb[((long long)c * g.Sh + (Y0 + r)) * g.Sw + X0 + x] = 0.0f;
                }
        }
        return;
    }
    const int* p = params + 16 * (long long)b;
    const int top = clampi(p[0], 0, Hl - 1), left = clampi(p[1], 0, Wl - 1);
    const int h = clampi(p[2], 1, min(Hl - top, (long long)kMaxDim)), w = clampi(p[3], 1, min(Wl - left, (long long)kMaxDim));
    const int OH = clampi(p[4], 1, kMaxDim), OW = clampi(p[5], 1, kMaxDim);
    const int oy = p[6], ox = p[7];
    const bool flip = p[8] != 0;
    const int suph = g.antialias ? max(h, OH) : OH, supw = g.antialias ? max(w, OW) : OW;

    for (int i = t; i < Cb + Rb; i += kT) {
        if (i < Cb) {
            const int X = X0 + i;
            colt[i] = axis_tap(clampi((long long)ox + (flip ? g.Sw - 1 - X : X), 0, OW - 1), w, OW, supw);
        } else {
            const int r = i - Cb;
            rowt[r] = axis_tap(clampi((long long)oy + Y0 + r, 0, OH - 1), h, OH, suph);
        }
    }
    __syncthreads();

    const int jlo = rowt[0].first, jhi = rowt[Rb - 1].first + rowt[Rb - 1].count;  // (first and last are monotone in the row)
    const float inv2w = 1.0f / (2.0f * (float)supw), inv2h = 1.0f / (2.0f * (float)suph);
    const uint8_t* img = raw + off;
    const int CW = g.CW;

    float acc[3][kRowsPerThread];
#pragma unroll
    for (int m = 0; m < kRowsPerThread; ++m) acc[0][m] = acc[1][m] = acc[2][m] = 0.0f;

    for (int j0 = jlo; j0 < jhi; j0 += g.rows_cap) {
        const int nr = min(g.rows_cap, jhi - j0);
        // horizontal: source rows [j0, j0 + nr) of the crop -> plane
        for (int it = t; it < nr * Cb; it += kT) {
            const int jj = it / Cb, xc = it - jj * Cb;
            const AxisTap ct = colt[xc];
            const uint8_t* q = img + ((long long)(top + j0 + jj) * Wl + left + ct.first) * 3;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int k = 0; k < ct.count; ++k) {
                const float wk = tri(ct.a0 + 2 * OW * k, inv2w);
                s0 += wk * (float)q[3 * k];
                s1 += wk * (float)q[3 * k + 1];
                s2 += wk * (float)q[3 * k + 2];
            }
            float* d = plane + (long long)jj * 3 * CW + xc;
            d[0] = s0 * ct.inv;
            d[CW] = s1 * ct.inv;
            d[2 * CW] = s2 * ct.inv;
        }
        __syncthreads();
        // vertical: every output adds the rows of this chunk that are its taps, in ascending order
        if (active) {
#pragma unroll
            for (int m = 0; m < kRowsPerThread; ++m) {
                const int r = tr + g.trows * m;
                if (r < Rb) {
                    const AxisTap rt = rowt[r];
                    const int lo = max(rt.first, j0), hi = min(rt.first + rt.count, j0 + nr);
                    for (int j = lo; j < hi; ++j) {
                        const float wj = tri(rt.a0 + 2 * OH * (j - rt.first), inv2h);
                        const float* s = plane + (long long)(j - j0) * 3 * CW + x;
                        acc[0][m] += wj * s[0];
                        acc[1][m] += wj * s[CW];
                        acc[2][m] += wj * s[2 * CW];
                    }
                }
            }
        }
        __syncthreads();
    }

    if (!active) return;
    if constexpr (U8) {
        const int X = X0 + x;
#pragma unroll
        for (int m = 0; m < kRowsPerThread; ++m) {
            const int r = tr + g.trows * m;
            if (r < Rb) {
#pragma clang fp contract(off)  // (the product is rounded before the half is added, as on the host)
                const float inv = rowt[r].inv;
                uint8_t* d = outb + ((long long)(Y0 + r) * g.Sw + X) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c)  // half up; fminf / fmaxf also turn a NaN (there is none) into a level
                    d[c] = (uint8_t)fminf(fmaxf(floorf(acc[c][m] * inv + 0.5f), 0.0f), 255.0f);
            }
        }
        return;
    }
    const long long ei = p[9], ej = p[10], eh = p[11], ew = p[12];
    const int mode = p[13];
    const uint32_t seed = (uint32_t)p[14];
    const float cval = __int_as_float(p[15]);
    const bool erase = (mode == 1 || mode == 2) && eh > 0 && ew > 0;
    const int X = X0 + x;
#pragma unroll
    for (int m = 0; m < kRowsPerThread; ++m) {
        const int r = tr + g.trows * m;
        if (r < Rb) {
            const int Y = Y0 + r;
            const float scale = rowt[r].inv * (1.0f / 255.0f);
            const bool inbox = erase && Y >= ei && Y < ei + eh && X >= ej && X < ej + ew;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = acc[c][m] * scale;
                if (mean_std) v = (v - mean_std[c]) / mean_std[3 + c];
                if (inbox) v = mode == 1 ? cval : erase_normal(seed, (uint32_t)b, (uint32_t)c, (uint32_t)Y, (uint32_t)X);
                outb[((long long)c * g.Sh + Y) * g.Sw + X] = v;
            }
        }
    }
}

template <bool U8>
int augment_launch(const char* who, const uint8_t* raw, const int64_t* table, const int32_t* params,
                   std::conditional_t<U8, uint8_t, float>* out, int32_t B, int32_t S_h, int32_t S_w, int32_t antialias,
                   const float* mean_std, int32_t lds_bytes, void* stream) {
    VT_REQUIRE(raw && table && params && out, VT_ERR_INVALID, "%s: null pointer (raw %p, table %p, params %p, out %p)", who,
               (const void*)raw, (const void*)table, (const void*)params, (const void*)out);
    VT_REQUIRE(B > 0 && S_h > 0 && S_w > 0, VT_ERR_INVALID, "%s: non-positive size (B %d, S_h %d, S_w %d)", who, B, S_h, S_w);
    VT_REQUIRE((((uintptr_t)table) & 7) == 0 && (((uintptr_t)params) & 3) == 0 && (U8 || (((uintptr_t)out) & 3) == 0) &&
                   (((uintptr_t)mean_std) & 3) == 0,
               VT_ERR_INVALID, "%s: misaligned table (8), params, out or mean_std (4)", who);
    VT_REQUIRE(lds_bytes >= 0, VT_ERR_INVALID, "%s: lds_bytes %d is negative", who, lds_bytes);
    AugGeo g;
    g.B = B, g.Sh = S_h, g.Sw = S_w, g.antialias = antialias != 0;
    g.CW = S_w < kMaxCW ? S_w : kMaxCW;
    g.trows = kT / g.CW < kMaxThreadRows ? kT / g.CW : kMaxThreadRows;
    g.R = S_h < g.trows * kRowsPerThread ? S_h : g.trows * kRowsPerThread;
    g.bandsY = (S_h + g.R - 1) / g.R, g.tilesX = (S_w + g.CW - 1) / g.CW;
    const long tables = (long)sizeof(AxisTap) * (g.CW + g.R), row = 3L * 4 * g.CW;
    const long cap = lds_bytes == 0 ? kDefaultLds : (lds_bytes < kMaxLds ? lds_bytes : kMaxLds);
    VT_REQUIRE(cap >= tables + row, VT_ERR_INVALID, "%s: lds_bytes %d holds no source row (the tables take %ld bytes, a row %ld)",
               who, lds_bytes, tables, row);
    g.rows_cap = (int)((cap - tables) / row);
    const int smem = (int)(tables + (long)g.rows_cap * row);
    const long blocks = (long)B * g.bandsY * g.tilesX;
    VT_REQUIRE(blocks < (1L << 31), VT_ERR_INVALID, "%s: %ld workgroups", who, blocks);
    if (smem > 64 * 1024) {
        const int rc = vt_raise_dynamic_lds((const void*)augment_kernel<U8>, smem, who);
        if (rc != VT_OK) return rc;
    }
    hipLaunchKernelGGL(augment_kernel<U8>, dim3((unsigned)blocks), dim3(kT), smem, (hipStream_t)stream, raw,
                       (const long long*)table, (const int*)params, out, mean_std, g);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_augment_batch(const uint8_t* raw, const int64_t* table, const int32_t* params, float* out, int32_t B, int32_t S_h,
                     int32_t S_w, int32_t antialias, const float* mean_std, int32_t lds_bytes, void* stream) {
    return augment_launch<false>("vt_augment_batch", raw, table, params, out, B, S_h, S_w, antialias, mean_std, lds_bytes, stream);
}

int vt_augment_batch_u8(const uint8_t* raw, const int64_t* table, const int32_t* params, uint8_t* out, int32_t B, int32_t S_h,
                        int32_t S_w, int32_t antialias, int32_t lds_bytes, void* stream) {
    return augment_launch<true>("vt_augment_batch_u8", raw, table, params, out, B, S_h, S_w, antialias, nullptr, lds_bytes, stream);
}

}  // extern "C"
