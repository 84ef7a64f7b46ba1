// vt_spp.hip -- the cascaded pooling block SPPBlock (reference components.py:139-152):
//
//   p_1 = pool(x), p_s = pool(p_{s-1}), y = cat(p_1 .. p_repeats) over channels,   pool = Max/AvgPool2d(k, 1, (k-1)/2)
//
// ONE forward launch writes every stage into its channel slice of y (the concat is never a copy), ONE backward launch
// turns the gradient of the whole concatenated map into dx, in gather form, without atomics.
//
// Maps are NHWC with a pixel stride ld >= C; a thread works on one 16-byte chunk (8 bf16 / 4 f32) of one pixel.  A
// workgroup owns (image, TH x TW tile of output pixels, slab of SC chunks).  With h = (k-1)/2 and R = repeats*h:
//
// FORWARD.  The x tile grown by R is staged in LDS once (plane A, compute dtype; positions outside the image hold -inf
// for max and 0 for avg).  Stage s runs from LDS as two separable passes over regions that shrink by h per stage: rows
// (A -> plane Trow), then columns (Trow -> A in place, and the tile itself to y).  The value written back to A is the
// STORED value (max: exact; avg: f32 sum * 1/k^2 rounded to the compute dtype), so the maps equal what `repeats` separate
// launches would store, and a position outside the image is re-set to -inf / 0 after every stage: AvgPool2d pads every
// stage with zeros and always divides by k^2, so the cascade is NOT one big window.
// Max also records, per element and stage, the window tap dy*k + dx of the winner (taps[repeats][B][H][W][C], uint8)
// under torch's tie rule -- the first maximum in row-major order of the window: the row pass keeps the LEFTMOST maximum
// of a row (strict >), the column pass the TOPMOST row whose row maximum equals the window maximum (strict >).
// Inputs are finite by contract: what a NaN in x does (value and tap) is not specified.
//
// BACKWARD.  D_s = d(loss)/d(p_s) lives in f32 LDS planes.  D_repeats = dy_repeats on the tile grown by R, then
//   D_{s-1}[i] = dy_{s-1}[i] + sum over the outputs o whose window holds i of [tap_s(o) points at i] * D_s[o]      (max)
//   D_{s-1}[i] = dy_{s-1}[i] + (1/k^2) * sum over the in-image o whose window holds i of D_s[o]                     (avg)
// on regions that shrink by h per stage; dx = D_0 (there is no dy_0: x is not part of the concat) is stored once,
// written or added to what is there.  Every element adds its terms in one fixed order (dy first, then the window in
// row-major order): no atomics of any kind, bit-identical runs.
#include <type_traits>

#include "vt_common.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxHalo = 8;
constexpr int kMaxK = 15;    // a tap dy*k + dx is one byte and 255 means "no tap": k*k - 1 <= 254
constexpr int kMaxTile = 16; // output pixels a side

struct SppGeo {
    int B, H, W, C, cpr;      // cpr: 16-byte chunks per pixel
    int k, h, repeats, R;     // R = repeats * h
    int TH, TW, SC, lsc;      // tile of output pixels, chunks per slab (a power of two) and its log2
    int RH, RW;               // TH + 2R, TW + 2R
    int tilesH, tilesW, slabs;
};

template <typename T>
__device__ __forceinline__ uint4 fill_chunk(float v) {
    float f[VecIO<T>::EPC];
#pragma unroll
    for (int e = 0; e < VecIO<T>::EPC; ++e) f[e] = v;
    return VecIO<T>::pack(f);
}

// the row-pass plane: compute dtype for max (exact), f32 for avg (row sums)
template <typename T, int POOL>
struct RowIO {
    static constexpr int EPC = VecIO<T>::EPC;
    static constexpr int kBytes = 16;
    __device__ static inline void load(const void* plane, int idx, float* f) { VecIO<T>::unpack(((const uint4*)plane)[idx], f); }
    __device__ static inline void store(void* plane, int idx, const float* f) { ((uint4*)plane)[idx] = VecIO<T>::pack(f); }
};
template <typename T>
struct RowIO<T, 1> {
    static constexpr int EPC = VecIO<T>::EPC;
    static constexpr int kBytes = EPC * 4;
    __device__ static inline void load(const void* plane, int idx, float* f) {
        const float4* p = (const float4*)plane + (size_t)idx * (EPC / 4);
#pragma unroll
        for (int q = 0; q < EPC / 4; ++q) {
            const float4 v = p[q];
            f[4 * q] = v.x, f[4 * q + 1] = v.y, f[4 * q + 2] = v.z, f[4 * q + 3] = v.w;
        }
    }
    __device__ static inline void store(void* plane, int idx, const float* f) {
        float4* p = (float4*)plane + (size_t)idx * (EPC / 4);
#pragma unroll
        for (int q = 0; q < EPC / 4; ++q) p[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
    }
};

// q / n for 0 <= q < 2^20 and 1 <= n <= 64 without an integer division (inv = 1.0f / n): (q + 0.5) / n lies at least 0.5 / n
// from an integer, far more than the rounding of the two float operations
__device__ __forceinline__ int fast_div(int q, float inv) { return (int)(((float)q + 0.5f) * inv); }

struct BlockPos {
    int b, i0, j0, cb, nch;  // image, region origin (tile origin - R), first chunk, chunks in this slab
};

__device__ __forceinline__ BlockPos block_pos(const SppGeo& g) {
    unsigned L = blockIdx.x;
    BlockPos p;
    const int slab = (int)(L % (unsigned)g.slabs);
    L /= (unsigned)g.slabs;
    const int tj = (int)(L % (unsigned)g.tilesW);
    L /= (unsigned)g.tilesW;
    const int ti = (int)(L % (unsigned)g.tilesH);
    p.b = (int)(L / (unsigned)g.tilesH);
    p.i0 = ti * g.TH - g.R;
    p.j0 = tj * g.TW - g.R;
    p.cb = slab * g.SC;
    p.nch = min(g.SC, g.cpr - p.cb);
    return p;
}

// LDS: A [RH][RW][SC] chunks | Trow [RH][RW][SC] row results | Arg [RH][RW][SC][EPC] bytes (max with taps)
// KT: the window size as a compile-time constant (3, 5, 7, 9, 13: the tap loops unroll and their LDS reads are issued
// together) or 0 for any other supported k (11, 15)
template <typename T, int POOL, int KT>
__global__ void __launch_bounds__(kT) spp_fwd_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy,
                                                     uint8_t* __restrict__ taps, SppGeo g) {
    constexpr int EPC = VecIO<T>::EPC;
    typedef RowIO<T, POOL> Row;
    extern __shared__ uint4 spp_smem[];
    const int npix = g.RH * g.RW, SC = g.SC, k = KT ? KT : g.k, h = (k - 1) / 2;
    uint4* A = spp_smem;
    unsigned char* Trow = (unsigned char*)(A + (size_t)npix * SC);
    uint8_t* Arg = Trow + (size_t)npix * SC * Row::kBytes;
    const BlockPos bp = block_pos(g);
    const float kFill = POOL == 0 ? -INFINITY : 0.f;
    const uint4 fill = fill_chunk<T>(kFill);
    const float inv = 1.0f / (float)(k * k), inv_rw = 1.0f / (float)g.RW;
    const bool want_taps = POOL == 0 && taps != nullptr;

    for (int idx = threadIdx.x; idx < npix * SC; idx += kT) {
        const int ch = idx & (SC - 1), p = idx >> g.lsc;
        const int pr = fast_div(p, inv_rw);
        const int i = bp.i0 + pr, j = bp.j0 + p - pr * g.RW;
        uint4 v = fill;
        if (ch < bp.nch && i >= 0 && i < g.H && j >= 0 && j < g.W)
            v = *(const uint4*)(x + (((long)bp.b * g.H + i) * g.W + j) * ldx + (bp.cb + ch) * EPC);
        A[idx] = v;
    }
    __syncthreads();

    for (int s = 0; s < g.repeats; ++s) {
        const int m_in = s * h, m_out = m_in + h;
        {  // rows: A[r][c-h .. c+h] -> Trow[r][c] for the rows of the stage's input region, the columns of its output region
            const int nr = g.RH - 2 * m_in, nc = g.RW - 2 * m_out;
            const float inv_nc = 1.0f / (float)nc;
            for (int idx = threadIdx.x; idx < nr * nc * SC; idx += kT) {
                const int ch = idx & (SC - 1), q = idx >> g.lsc;
                const int qr = fast_div(q, inv_nc);
                const int r = m_in + qr, c = m_out + q - qr * nc;
                float acc[EPC];
                uint8_t arg[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] = kFill, arg[e] = 0;
                const uint4* src = A + ((size_t)r * g.RW + (c - h)) * SC + ch;
#pragma unroll KT ? KT : 1
                for (int d = 0; d < k; ++d) {
                    float v[EPC];
                    VecIO<T>::unpack(src[(size_t)d * SC], v);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        if (POOL == 0) {
                            if (v[e] > acc[e]) acc[e] = v[e], arg[e] = (uint8_t)d;  // strict: the leftmost maximum stays
                        } else {
                            acc[e] += v[e];
                        }
                    }
                }
                const int o = (r * g.RW + c) * SC + ch;
                Row::store(Trow, o, acc);
                if (want_taps) {  // EPC bytes, element e in byte e: written as words
                    uint32_t* dst = (uint32_t*)(Arg + (size_t)o * EPC);
#pragma unroll
                    for (int q4 = 0; q4 < EPC / 4; ++q4)
                        dst[q4] = (uint32_t)arg[4 * q4] | ((uint32_t)arg[4 * q4 + 1] << 8) | ((uint32_t)arg[4 * q4 + 2] << 16) |
                                  ((uint32_t)arg[4 * q4 + 3] << 24);
                }
            }
        }
        __syncthreads();
        {  // columns: Trow[r-h .. r+h][c] -> A[r][c] (stored value; -inf / 0 outside the image), the tile itself -> y
            const int nr = g.RH - 2 * m_out, nc = g.RW - 2 * m_out;
            const float inv_nc = 1.0f / (float)nc;
            for (int idx = threadIdx.x; idx < nr * nc * SC; idx += kT) {
                const int ch = idx & (SC - 1), q = idx >> g.lsc;
                const int qr = fast_div(q, inv_nc);
                const int r = m_out + qr, c = m_out + q - qr * nc;
                const int i = bp.i0 + r, j = bp.j0 + c;
                const int o = (r * g.RW + c) * SC + ch;
                if (!(i >= 0 && i < g.H && j >= 0 && j < g.W)) {
                    A[o] = fill;
                    continue;
                }
                float acc[EPC];
                uint8_t arg[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] = kFill, arg[e] = 0;
#pragma unroll KT ? KT : 1
                for (int d = 0; d < k; ++d) {
                    float v[EPC];
                    Row::load(Trow, ((r - h + d) * g.RW + c) * SC + ch, v);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        if (POOL == 0) {
                            if (v[e] > acc[e]) acc[e] = v[e], arg[e] = (uint8_t)d;  // strict: the topmost such row stays
                        } else {
                            acc[e] += v[e];
                        }
                    }
                }
                if (POOL == 1) {
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[e] *= inv;
                }
                const uint4 packed = VecIO<T>::pack(acc);
                A[o] = packed;
                const bool in_tile = r >= g.R && r < g.R + g.TH && c >= g.R && c < g.R + g.TW;
                if (!in_tile || ch >= bp.nch) continue;
                const long pix = ((long)bp.b * g.H + i) * g.W + j;
                *(uint4*)(y + pix * ldy + (long)s * g.C + (bp.cb + ch) * EPC) = packed;
                if (want_taps) {
                    uint32_t w[EPC / 4];
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const int dy = arg[e];
                        const uint32_t t = (uint32_t)(dy * k) + Arg[((size_t)((r - h + dy) * g.RW + c) * SC + ch) * EPC + e];
                        if (e % 4 == 0) w[e / 4] = 0;
                        w[e / 4] |= t << (8 * (e % 4));
                    }
                    uint8_t* dst = taps + (((long)s * g.B + bp.b) * g.H * g.W + ((long)i * g.W + j)) * g.C + (bp.cb + ch) * EPC;
#pragma unroll
                    for (int q4 = 0; q4 < EPC / 4; ++q4) ((uint32_t*)dst)[q4] = w[q4];
                }
            }
        }
        __syncthreads();
    }
}

// LDS: D0, D1 [RH][RW][SC][EPC] f32 | Tap [RH][RW][SC][EPC] bytes (max)
template <typename T, int POOL, int KT>
__global__ void __launch_bounds__(kT) spp_bwd_kernel(const T* __restrict__ dy, int lddy, const uint8_t* __restrict__ taps,
                                                     T* __restrict__ dx, int lddx, int accumulate, SppGeo g) {
    constexpr int EPC = VecIO<T>::EPC;
    typedef RowIO<T, 1> Plane;  // EPC floats per (pixel, chunk)
    extern __shared__ uint4 spp_smem[];
    const int npix = g.RH * g.RW, SC = g.SC, k = KT ? KT : g.k, h = (k - 1) / 2;
    unsigned char* Dcur = (unsigned char*)spp_smem;
    unsigned char* Dnext = Dcur + (size_t)npix * SC * Plane::kBytes;
    uint8_t* Tap = Dnext + (size_t)npix * SC * Plane::kBytes;
    const BlockPos bp = block_pos(g);
    const float inv = 1.0f / (float)(k * k), inv_rw = 1.0f / (float)g.RW;

    // D_repeats = dy_repeats on the whole region, 0 outside the image
    for (int idx = threadIdx.x; idx < npix * SC; idx += kT) {
        const int ch = idx & (SC - 1), p = idx >> g.lsc;
        const int pr = fast_div(p, inv_rw);
        const int i = bp.i0 + pr, j = bp.j0 + p - pr * g.RW;
        float v[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = 0.f;
        if (ch < bp.nch && i >= 0 && i < g.H && j >= 0 && j < g.W)
            VecIO<T>::unpack(*(const uint4*)(dy + (((long)bp.b * g.H + i) * g.W + j) * lddy + (long)(g.repeats - 1) * g.C +
                                             (bp.cb + ch) * EPC),
                             v);
        Plane::store(Dcur, idx, v);
    }

    for (int s = g.repeats - 1; s >= 0; --s) {
        const int m_in = (g.repeats - 1 - s) * h, m_out = m_in + h;  // D_s is valid from margin m_in, D_{s-1} from m_out
        if (POOL == 0) {  // this stage's taps over the region of D_s; 255 (no tap) outside the image
            const int nr = g.RH - 2 * m_in, nc = g.RW - 2 * m_in;
            const float inv_nc = 1.0f / (float)nc;
            for (int idx = threadIdx.x; idx < nr * nc * SC; idx += kT) {
                const int ch = idx & (SC - 1), q = idx >> g.lsc;
                const int qr = fast_div(q, inv_nc);
                const int r = m_in + qr, c = m_in + q - qr * nc;
                const int i = bp.i0 + r, j = bp.j0 + c;
                uint32_t w[EPC / 4];
#pragma unroll
                for (int q4 = 0; q4 < EPC / 4; ++q4) w[q4] = 0xffffffffu;
                if (ch < bp.nch && i >= 0 && i < g.H && j >= 0 && j < g.W) {
                    const uint8_t* src =
                        taps + (((long)s * g.B + bp.b) * g.H * g.W + ((long)i * g.W + j)) * g.C + (bp.cb + ch) * EPC;
#pragma unroll
                    for (int q4 = 0; q4 < EPC / 4; ++q4) w[q4] = ((const uint32_t*)src)[q4];
                }
                uint32_t* dst = (uint32_t*)(Tap + ((size_t)(r * g.RW + c) * SC + ch) * EPC);
#pragma unroll
                for (int q4 = 0; q4 < EPC / 4; ++q4) dst[q4] = w[q4];
            }
        }
        __syncthreads();
        const int nr = g.RH - 2 * m_out, nc = g.RW - 2 * m_out;
        const float inv_nc = 1.0f / (float)nc;
        for (int idx = threadIdx.x; idx < nr * nc * SC; idx += kT) {
            const int ch = idx & (SC - 1), q = idx >> g.lsc;
            const int qr = fast_div(q, inv_nc);
            const int r = m_out + qr, c = m_out + q - qr * nc;
            const int i = bp.i0 + r, j = bp.j0 + c;
            const int o = (r * g.RW + c) * SC + ch;
            const bool live = ch < bp.nch && i >= 0 && i < g.H && j >= 0 && j < g.W;
            float acc[EPC], win[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = 0.f, win[e] = 0.f;
            if (!live) {
                if (s > 0) Plane::store(Dnext, o, acc);
                continue;
            }
            const long pix = ((long)bp.b * g.H + i) * g.W + j;
            if (s > 0) VecIO<T>::unpack(*(const uint4*)(dy + pix * lddy + (long)(s - 1) * g.C + (bp.cb + ch) * EPC), acc);
            // the outputs whose window holds (r, c): (r + a - h, c + b - h); (r, c) is their tap (k-1-a, k-1-b)
            for (int a = 0; a < k; ++a) {
#pragma unroll KT ? KT : 1
                for (int b = 0; b < k; ++b) {
                    const int oo = ((r + a - h) * g.RW + (c + b - h)) * SC + ch;
                    float v[EPC];
                    Plane::load(Dcur, oo, v);
                    if (POOL == 0) {
                        const uint32_t want = (uint32_t)((k - 1 - a) * k + (k - 1 - b));
                        const uint32_t* tw = (const uint32_t*)(Tap + (size_t)oo * EPC);
#pragma unroll
                        for (int e = 0; e < EPC; ++e)
                            if (((tw[e / 4] >> (8 * (e % 4))) & 0xffu) == want) win[e] += v[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < EPC; ++e) win[e] += v[e];
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] += POOL == 0 ? win[e] : win[e] * inv;
            if (s > 0) {
                Plane::store(Dnext, o, acc);
                continue;
            }
            // s == 0: the region is the tile itself; dx = D_0
            T* dst = dx + pix * lddx + (bp.cb + ch) * EPC;
            if (accumulate) {
                float old[EPC];
                VecIO<T>::unpack(*(const uint4*)dst, old);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] += old[e];
            }
            *(uint4*)dst = VecIO<T>::pack(acc);
        }
        __syncthreads();
        unsigned char* t = Dcur;
        Dcur = Dnext;
        Dnext = t;
    }
}

int check_map(const char* who, const char* what, const void* p, int ld, int C, int dtype) {
    const int epc = vt_epc(dtype);
    VT_REQUIRE(p && vt_aligned16(p), VT_ERR_INVALID, "%s: %s is null or misaligned", who, what);
    VT_REQUIRE(ld >= C && ld % epc == 0, VT_ERR_INVALID, "%s: %s has pixel stride %d (needs >= %d, a multiple of %d)", who, what, ld,
               C, epc);
    return VT_OK;
}

int check_geometry(const char* who, int B, int H, int W, int C, int k, int repeats, int pool, int dtype) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(pool == 0 || pool == 1, VT_ERR_UNSUPPORTED, "%s: pool %d (0 max, 1 avg)", who, pool);
    VT_REQUIRE(vt_spp_supported(k, repeats), VT_ERR_UNSUPPORTED,
               "%s: kernel_size k=%d with repeats=%d (k odd, 3 <= k <= %d, repeats in 1..4, repeats*(k-1)/2 <= %d)", who, k,
               repeats, kMaxK, kMaxHalo);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C > 0 && C % epc == 0, VT_ERR_UNSUPPORTED, "%s: C=%d must be a positive multiple of %d", who, C, epc);
    VT_REQUIRE(B > 0 && H > 0 && W > 0, VT_ERR_INVALID, "%s: B=%d H=%d W=%d", who, B, H, W);
    VT_REQUIRE((long)B * H * W * C * repeats < (1L << 40), VT_ERR_UNSUPPORTED, "%s: map too large", who);
    return VT_OK;
}

// Tiles of at most kMaxTile pixels a side, balanced over the map (20 -> 2 x 10, not 16 + 4), and the widest slab of channel
// chunks (8, 4, 2, 1: 128 .. 16 contiguous bytes per pixel) whose planes fit the LDS budget (knob VT_SPP_LDS_KB; wider slabs
// measured slower above 48 KB).  The budget only chooses among slab widths: a slab of ONE chunk always runs, whatever it
// needs -- at most 32 x 32 pixels x 72 bytes = 72 KB (bf16 backward, a full tile, halo 8), which takes the raised
// dynamic-LDS limit.
int plan(const char* who, SppGeo* g, int B, int H, int W, int C, int k, int repeats, int dtype, int bytes_per_chunk, int* smem) {
    const int tmax = kMaxTile;
    const int budget = VT_KNOB("VT_SPP_LDS_KB", 48) * 1024;
    VT_REQUIRE(budget >= 8 * 1024 && budget <= 160 * 1024, VT_ERR_INVALID, "%s: knob VT_SPP_LDS_KB=%d out of range (8..160)", who,
               budget / 1024);
    g->B = B, g->H = H, g->W = W, g->C = C, g->cpr = C / vt_epc(dtype);
    g->k = k, g->h = (k - 1) / 2, g->repeats = repeats, g->R = repeats * g->h;
    g->tilesH = (H + tmax - 1) / tmax, g->tilesW = (W + tmax - 1) / tmax;
    g->TH = (H + g->tilesH - 1) / g->tilesH, g->TW = (W + g->tilesW - 1) / g->tilesW;
    g->tilesH = (H + g->TH - 1) / g->TH, g->tilesW = (W + g->TW - 1) / g->TW;
    g->RH = g->TH + 2 * g->R, g->RW = g->TW + 2 * g->R;
    const long per_chunk = (long)g->RH * g->RW * bytes_per_chunk;
    int sc = 8;
    while (sc > 1 && (sc / 2 >= g->cpr || per_chunk * sc > budget)) sc /= 2;
    VT_REQUIRE(per_chunk * sc <= 160 * 1024, VT_ERR_UNSUPPORTED, "%s: %ld bytes of LDS for one chunk slab", who, per_chunk);
    g->SC = sc;
    g->lsc = sc == 8 ? 3 : (sc == 4 ? 2 : (sc == 2 ? 1 : 0));
    g->slabs = (g->cpr + sc - 1) / sc;
    *smem = (int)(per_chunk * sc);
    const long blocks = (long)B * g->tilesH * g->tilesW * g->slabs;
    VT_REQUIRE(blocks < (1L << 31), VT_ERR_UNSUPPORTED, "%s: %ld workgroups", who, blocks);
    return VT_OK;
}

#define VT_SPP_BY_K(LAUNCH, T, P)           \
    do {                                    \
        switch (k) {                        \
            case 3: LAUNCH(T, P, 3); break;   \
            case 5: LAUNCH(T, P, 5); break;   \
            case 7: LAUNCH(T, P, 7); break;   \
            case 9: LAUNCH(T, P, 9); break;   \
            case 13: LAUNCH(T, P, 13); break; \
            default: LAUNCH(T, P, 0); break;  \
        }                                   \
    } while (0)

template <typename K>
int launch_prep(K kern, int smem, const char* who) {
    if (smem > 64 * 1024) return vt_raise_dynamic_lds((const void*)kern, smem, who);
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_spp_supported(int32_t k, int32_t repeats) {
    return k >= 3 && k <= kMaxK && (k & 1) && repeats >= 1 && repeats <= 4 && repeats * ((k - 1) / 2) <= kMaxHalo;
}

int vt_spp_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, uint8_t* taps, int32_t B, int32_t H, int32_t W, int32_t C,
               int32_t k, int32_t repeats, int32_t pool, int32_t dtype, void* stream) {
    const char* who = "vt_spp_fwd";
    VT_TRY(check_geometry(who, B, H, W, C, k, repeats, pool, dtype));
    VT_TRY(check_map(who, "x", x, ldx, C, dtype));
    VT_TRY(check_map(who, "y", y, ldy, repeats * C, dtype));
    VT_REQUIRE(x != y, VT_ERR_INVALID, "%s: y aliases x", who);
    if (pool != 0) taps = nullptr;
    VT_REQUIRE(!taps || vt_aligned16(taps), VT_ERR_INVALID, "%s: taps is misaligned", who);
    const int epc = vt_epc(dtype);
    // per (pixel, chunk): A 16 B, the row plane 16 B (max) or EPC floats (avg), EPC tap bytes (max with taps)
    const int per_chunk = 16 + (pool == 0 ? 16 : 4 * epc) + (taps ? epc : 0);
    SppGeo g;
    int smem = 0;
    VT_TRY(plan(who, &g, B, H, W, C, k, repeats, dtype, per_chunk, &smem));
    const dim3 grid((unsigned)((long)B * g.tilesH * g.tilesW * g.slabs));
    hipStream_t st = (hipStream_t)stream;
#define VT_SPP_FWD_K(T, P, KT)                                                                                       \
    do {                                                                                                             \
        VT_TRY(launch_prep(spp_fwd_kernel<T, P, KT>, smem, who));                                                    \
        hipLaunchKernelGGL((spp_fwd_kernel<T, P, KT>), grid, dim3(kT), smem, st, (const T*)x, ldx, (T*)y, ldy, taps, g); \
    } while (0)
#define VT_SPP_FWD(T, P) VT_SPP_BY_K(VT_SPP_FWD_K, T, P)
    if (dtype == VT_BF16) {
        if (pool == 0) VT_SPP_FWD(bf16_t, 0);
        else VT_SPP_FWD(bf16_t, 1);
    } else {
        if (pool == 0) VT_SPP_FWD(float, 0);
        else VT_SPP_FWD(float, 1);
    }
#undef VT_SPP_FWD
#undef VT_SPP_FWD_K
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_spp_bwd(const void* dy, int32_t lddy, const uint8_t* taps, void* dx, int32_t lddx, int32_t accumulate, int32_t B, int32_t H,
               int32_t W, int32_t C, int32_t k, int32_t repeats, int32_t pool, int32_t dtype, void* stream) {
    const char* who = "vt_spp_bwd";
    VT_TRY(check_geometry(who, B, H, W, C, k, repeats, pool, dtype));
    VT_TRY(check_map(who, "dy", dy, lddy, repeats * C, dtype));
    VT_TRY(check_map(who, "dx", dx, lddx, C, dtype));
    VT_REQUIRE(dx != dy, VT_ERR_INVALID, "%s: dx aliases dy", who);
    VT_REQUIRE(pool != 0 || (taps && vt_aligned16(taps)), VT_ERR_INVALID, "%s: taps is null or misaligned (max needs the taps)", who);
    const int epc = vt_epc(dtype);
    const int per_chunk = 2 * 4 * epc + (pool == 0 ? epc : 0);  // two f32 planes, EPC tap bytes (max)
    SppGeo g;
    int smem = 0;
    VT_TRY(plan(who, &g, B, H, W, C, k, repeats, dtype, per_chunk, &smem));
    const dim3 grid((unsigned)((long)B * g.tilesH * g.tilesW * g.slabs));
    hipStream_t st = (hipStream_t)stream;
#define VT_SPP_BWD_K(T, P, KT)                                                                                            \
    do {                                                                                                                  \
        VT_TRY(launch_prep(spp_bwd_kernel<T, P, KT>, smem, who));                                                         \
        hipLaunchKernelGGL((spp_bwd_kernel<T, P, KT>), grid, dim3(kT), smem, st, (const T*)dy, lddy, taps, (T*)dx, lddx, \
                           accumulate != 0, g);                                                                           \
    } while (0)
#define VT_SPP_BWD(T, P) VT_SPP_BY_K(VT_SPP_BWD_K, T, P)
    if (dtype == VT_BF16) {
        if (pool == 0) VT_SPP_BWD(bf16_t, 0);
        else VT_SPP_BWD(bf16_t, 1);
    } else {
        if (pool == 0) VT_SPP_BWD(float, 0);
        else VT_SPP_BWD(float, 1);
    }
#undef VT_SPP_BWD
#undef VT_SPP_BWD_K
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // extern "C"
