// vt_jpeg.hip -- baseline JPEG decoding on the device (the reference's image_loader, classifier.py:22-25, is
// torchvision.io.decode_jpeg(..., device=device)): compressed files -> the packed uint8 HWC images that vt_augment_batch reads.
//
// The host (vision_toolbox/data.py) parses the markers, refuses what is out of scope and builds the tables of vt_amd.h.
// Two launches:
//
//   vt_jpeg_entropy   ONE WAVE PER ENTROPY SEGMENT (a file without restart markers is one segment).  The wave's lanes fetch
//                     the segment's bytes into an LDS window together, 1 KiB at a time; the symbol decode (vt_jpeg_bits.h,
//                     the same code the host sanitizer run exercises) is wave-uniform; lane n keeps coefficient n (natural
//                     order) of the current block in a register, so a block leaves as one 128-byte store.  The decoding
//                     tables (T.81 F.2.2.3) of the image's up to six Huffman tables are built in LDS from BITS.
//   vt_jpeg_idct_rgb  a workgroup owns (image, band of R MCU rows, tile of 8 MCU columns).  A thread takes one block: 64
//                     coefficients, dequantised, through both passes of the accurate integer IDCT (jidctint: 13-bit
//                     constants, 2 pass-1 bits, +128, clamp) in registers, 8 x 8 samples into an LDS plane.  The chroma
//                     planes carry ONE BLOCK OF HALO on every side of the tile where the component is sub-sampled, recomputed
//                     from the scratch, so the triangle filters (h2v1: 3 near + far; h2v2: 9-3-3-1) see the neighbours they
//                     need and the result does not depend on the split.  Then a thread per pixel: upsample, the 16-bit
//                     fixed-point colour conversion, three byte stores, cropped to the true W and H.
//
// Edge replication of the filters is the clamp of the neighbour index into the component's TRUE size ceil(W / 2) x ceil(H / 2),
// which reproduces libjpeg's first / last column cases ((4 t + 8) >> 4, (4 t + 7) >> 4, and t itself for h2v1).  As in libjpeg,
// the triangle filters are used only where the chroma plane is more than two samples wide; a narrower one is replicated.
//
// SAFETY (vt_amd.h has the full statement).  Every row of `segments` and `images` is range-checked on entry against B,
// data_bytes, coef_blocks, NH, NQ and raw_bytes before it forms an address; a row that fails writes nothing but its status.
// The loops of the entropy kernel are bounded by the MCU count of the host table and by 64 symbols per block.  No atomics.
#include "vt_common.h"
#include "vt_jpeg_bits.h"

namespace {

constexpr int kI = VT_JPEG_IMG_FIELDS, kS = VT_JPEG_SEG_FIELDS, kHuff = VT_JPEG_HUFF_BYTES;
constexpr int kWin = 1024;         // bytes of the LDS window of the bit reader
constexpr int kTX = 8;             // MCU columns of an IDCT tile
constexpr int kMaxR = 4;           // MCU rows of a band, at most (and the default)
constexpr long long kMaxMcus = 1 << 17;  // per axis: 2^20 pixels

__constant__ uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// lane n keeps the coefficient whose zigzag position is its own
struct LaneSink {
    int myzz, val;
    __device__ void put(int k, int v) {
        if (k == myzz) val = v;
    }
};

// The segment's bytes through a 1 KiB LDS window that only moves forward.  get() is called with a wave-uniform position in
// [begin, end) (vt_jpeg_fill checks it); the refill is done by all 64 lanes of the one wave of the workgroup.
struct WindowSrc {
    const uint8_t* data;
    int64_t end;       // one past the last byte of the segment (<= data_bytes, checked by the kernel)
    int64_t w0;        // first byte of the window (a multiple of 4), -1: empty
    uint8_t* win;      // LDS [kWin]
    int lane;
    __device__ uint32_t get(int64_t pos) {
        if (w0 < 0 || pos >= w0 + kWin) {
            __syncthreads();  // (one wave: the earlier reads of the window are done)
            w0 = pos & ~(int64_t)3;
#pragma unroll
            for (int j = 0; j < kWin / 256; ++j) {
                const int o = (j * 64 + lane) * 4;
                const int64_t g = w0 + o;
                uint32_t w = 0;
                if (g + 4 <= end) {
                    w = *(const uint32_t*)(data + g);  // data is 4-byte aligned (checked by the host entry), g a multiple of 4
                } else {
                    for (int k = 0; k < 4; ++k)
                        if (g + k < end) w |= (uint32_t)data[g + k] << (8 * k);
                }
                *(uint32_t*)(win + o) = w;
            }
            __syncthreads();
        }
        return win[pos - w0];
    }
};

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ data, long long data_bytes,
                                                          const long long* __restrict__ images, int B,
                                                          const long long* __restrict__ segments, int S,
                                                          const uint8_t* __restrict__ huff, int NH, short* __restrict__ coef,
                                                          long long coef_blocks, int* __restrict__ status) {
    __shared__ VtJpegHuff tab[6];
    __shared__ uint8_t vals[6][256];
    __shared__ __attribute__((aligned(16))) uint8_t win[kWin];

    const int lane = threadIdx.x, seg = blockIdx.x;
    if (seg >= S) return;
    const long long* sg = segments + (long long)seg * kS;
    const long long b = sg[0], begin = sg[1], end = sg[2], m0 = sg[3], mc = sg[4];
    bool ok = b >= 0 && b < B && begin >= 0 && begin <= end && end <= data_bytes && m0 >= 0 && mc >= 0;
    long long nc = 0, hm = 0, vm = 0, mx = 0, my = 0, base = 0;
    if (ok) {
        const long long* im = images + b * kI;
        nc = im[2], hm = im[3], vm = im[4], mx = im[5], my = im[6], base = im[16];
        ok = (nc == 1 || nc == 3) && (hm == 1 || hm == 2) && (vm == 1 || vm == 2) && !(nc == 1 && (hm != 1 || vm != 1)) &&
             mx >= 1 && mx <= kMaxMcus && my >= 1 && my <= kMaxMcus && base >= 0 && base <= coef_blocks;
        if (ok) {
            const long long blocks = mx * my * (hm * vm + (nc == 3 ? 2 : 0));
            ok = blocks <= coef_blocks - base && m0 <= mx * my && mc <= mx * my - m0;
            for (int t = 0; t < 2 * (int)nc; ++t) ok = ok && im[10 + t] >= 0 && im[10 + t] < NH;
        }
    }
    if (!ok) {  // (uniform over the wave, in front of every barrier)
        if (lane == 0) status[seg] = VT_JPEG_ERR_TABLE;
        return;
    }
    const long long* im = images + b * kI;
    const int ntab = 2 * (int)nc;  // table 2 c: DC of component c, 2 c + 1: AC
    for (int i = lane; i < ntab * 256; i += 64) vals[i >> 8][i & 255] = huff[im[10 + (i >> 8)] * kHuff + 16 + (i & 255)];
    if (lane < ntab) vt_jpeg_huff_build(huff + im[10 + lane] * kHuff, &tab[lane]);
    __syncthreads();
    int st = VT_JPEG_OK;
    for (int t = 0; t < ntab; ++t)
        if (!tab[t].valid) st = VT_JPEG_ERR_TABLE;  // its blocks are written as zeros

    LaneSink sink;
    sink.myzz = 0, sink.val = 0;
    for (int k = 0; k < 64; ++k)
        if (kNatural[k] == lane) sink.myzz = k;

    WindowSrc src;
    src.data = data, src.end = end, src.w0 = -1, src.win = win, src.lane = lane;
    VtJpegBits r;
    vt_jpeg_bits_init(&r, begin, end);
    int pred[3] = {0, 0, 0};
    const long long ybw = mx * hm, cbase = base + mx * hm * my * vm, cplane = mx * my;
    for (long long m = 0; m < mc; ++m) {  // mc <= MCUs of the image <= coef_blocks, from the host table
        const long long mcu = m0 + m, mcx = mcu % mx, mcy = mcu / mx;
        for (int c = 0; c < (int)nc; ++c) {
            const int hc = c == 0 ? (int)hm : 1, vc = c == 0 ? (int)vm : 1;
            for (int v = 0; v < vc; ++v)
                for (int h = 0; h < hc; ++h) {
                    const long long blk = c == 0 ? base + (mcy * vm + v) * ybw + mcx * hm + h : cbase + (c - 1) * cplane + mcy * mx + mcx;
                    sink.val = 0;
                    if (st == VT_JPEG_OK) {
                        int rc = vt_jpeg_block(&r, src, &tab[2 * c], vals[2 * c], &tab[2 * c + 1], vals[2 * c + 1], &pred[c], sink);
                        if (rc == VT_JPEG_OK && vt_jpeg_overrun(&r) > 0) rc = VT_JPEG_ERR_TRUNCATED;
                        if (rc != VT_JPEG_OK) st = rc, sink.val = 0;
                    }
                    coef[blk * 64 + lane] = (short)sink.val;
                }
        }
    }
    if (st == VT_JPEG_OK && vt_jpeg_unread(&r) >= 8) st = VT_JPEG_ERR_TRAILING;
    if (lane == 0) status[seg] = st;
}

// ---- IDCT, upsampling, colour ------------------------------------------------------------------------------------------
constexpr int kC0298 = 2446, kC0390 = 3196, kC0541 = 4433, kC0765 = 6270, kC0899 = 7373, kC1175 = 9633, kC1501 = 12299,
              kC1847 = 15137, kC1961 = 16069, kC2053 = 16819, kC2562 = 20995, kC3072 = 25172;

// one 1-D pass of jidctint on eight values with stride `s`; SHIFT = 11 (pass 1) or 18 (pass 2).  Sums and products are
// formed modulo 2^32 (unsigned) and read as a signed 32-bit value only for the final arithmetic shift.  For the coefficients
// of a real image nothing ever wraps and this is jidctint to the bit; for the garbage a damaged stream can leave in the
// scratch (any int16 times a table entry up to 255) it is still a defined function of the input, the same one as the host
// stage's (data.jpeg_idct_blocks: exact int64, wrapped to 32 bits before each shift), with no signed overflow anywhere.
template <int SHIFT>
__device__ __forceinline__ void idct8(int* d, int s) {
    typedef uint32_t U;
    auto C = [](int c) { return (U)c; };
    U z2 = (U)d[2 * s], z3 = (U)d[6 * s];
    U z1 = (z2 + z3) * C(kC0541);
    U tmp2 = z1 + z3 * C(-kC1847), tmp3 = z1 + z2 * C(kC0765);
    z2 = (U)d[0], z3 = (U)d[4 * s];
    U tmp0 = (z2 + z3) * 8192u, tmp1 = (z2 - z3) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)d[7 * s], tmp1 = (U)d[5 * s], tmp2 = (U)d[3 * s], tmp3 = (U)d[1 * s];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * C(kC1175);
    tmp0 *= C(kC0298), tmp1 *= C(kC2053), tmp2 *= C(kC3072), tmp3 *= C(kC1501);
    z1 *= C(-kC0899), z2 *= C(-kC2562), z3 *= C(-kC1961), z4 *= C(-kC0390);
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    constexpr U R = 1u << (SHIFT - 1);
    d[0] = (int)(tmp10 + tmp3 + R) >> SHIFT, d[7 * s] = (int)(tmp10 - tmp3 + R) >> SHIFT;
    d[1 * s] = (int)(tmp11 + tmp2 + R) >> SHIFT, d[6 * s] = (int)(tmp11 - tmp2 + R) >> SHIFT;
    d[2 * s] = (int)(tmp12 + tmp1 + R) >> SHIFT, d[5 * s] = (int)(tmp12 - tmp1 + R) >> SHIFT;
    d[3 * s] = (int)(tmp13 + tmp0 + R) >> SHIFT, d[4 * s] = (int)(tmp13 - tmp0 + R) >> SHIFT;
}

__device__ __forceinline__ uint32_t level(int v) { return (uint32_t)min(max(v + 128, 0), 255); }

// block -> 8 rows of 8 samples at dst (row stride `ld` bytes, 8-byte aligned)
__device__ __forceinline__ void idct_block(const short* __restrict__ cf, const uint8_t* __restrict__ q, uint8_t* dst, int ld) {
    int ws[64];
    const uint4* c4 = (const uint4*)cf;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = c4[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[8 * i + 2 * j] = (int)(short)(w[j] & 0xffffu) * (int)q[8 * i + 2 * j];
            ws[8 * i + 2 * j + 1] = (int)(short)(w[j] >> 16) * (int)q[8 * i + 2 * j + 1];
        }
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) idct8<11>(ws + x, 8);
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        idct8<18>(ws + 8 * y, 1);
        uint2 o;
        o.x = level(ws[8 * y]) | level(ws[8 * y + 1]) << 8 | level(ws[8 * y + 2]) << 16 | level(ws[8 * y + 3]) << 24;
        o.y = level(ws[8 * y + 4]) | level(ws[8 * y + 5]) << 8 | level(ws[8 * y + 6]) << 16 | level(ws[8 * y + 7]) << 24;
        *(uint2*)(dst + y * ld) = o;
    }
}

constexpr int kLumaLd = kTX * 2 * 8;          // 128
constexpr int kChromaLd = (kTX + 2) * 8;      // 80
constexpr int kChromaRows = (kMaxR + 2) * 8;  // 48

__global__ __launch_bounds__(256) void jpeg_idct_rgb_kernel(const short* __restrict__ coef, long long coef_blocks,
                                                            const long long* __restrict__ images, int B,
                                                            const uint8_t* __restrict__ qtabs, int NQ, uint8_t* __restrict__ raw,
                                                            long long raw_bytes, int R) {
    __shared__ __attribute__((aligned(16))) uint8_t luma[kMaxR * 2 * 8 * kLumaLd];       // 8 KiB
    __shared__ __attribute__((aligned(16))) uint8_t chroma[2][kChromaRows * kChromaLd];  // 2 x 3840 B
    __shared__ uint8_t qs[3][64];

    const int t = threadIdx.x;
    const int tile = blockIdx.x, band = blockIdx.y, b = blockIdx.z;
    if (b >= B) return;
    const long long* im = images + (long long)b * kI;
    const long long H = im[0], W = im[1], nc = im[2], hm = im[3], vm = im[4], mx = im[5], my = im[6], base = im[16], off = im[17];
    bool ok = (nc == 1 || nc == 3) && (hm == 1 || hm == 2) && (vm == 1 || vm == 2) && !(hm == 1 && vm == 2) &&
              !(nc == 1 && hm != 1) && mx >= 1 && mx <= kMaxMcus && my >= 1 && my <= kMaxMcus && H >= 1 && W >= 1 &&
              H <= my * vm * 8 && W <= mx * hm * 8 && base >= 0 && base <= coef_blocks && off >= 0 && off <= raw_bytes;
    if (ok) {
        ok = mx * my * (hm * vm + (nc == 3 ? 2 : 0)) <= coef_blocks - base && H * W * 3 <= raw_bytes - off;
        for (int c = 0; c < (int)nc; ++c) ok = ok && im[7 + c] >= 0 && im[7 + c] < NQ;
    }
    if (!ok || (long long)tile * kTX >= mx || (long long)band * R >= my) return;  // (uniform, in front of every barrier)

    if (t < 64 * (int)nc) qs[t >> 6][t & 63] = qtabs[im[7 + (t >> 6)] * 64 + (t & 63)];
    __syncthreads();

    const int ihm = (int)hm, ivm = (int)vm;
    const int hx = ihm == 2, hy = ivm == 2;  // halo blocks of the chroma planes
    const long long mcx0 = (long long)tile * kTX, mcy0 = (long long)band * R;
    const long long ybw = mx * hm, cbase = base + mx * hm * my * vm, cplane = mx * my;
    const int ybx = kTX * ihm, nY = R * ivm * ybx;     // luma blocks of the tile: nY, ybx per row
    const int cgx = kTX + 2, nCg = (R + 2) * cgx;      // chroma grid of the tile with its halo ring
    const int nblk = nY + (nc == 3 ? 2 * nCg : 0);
    for (int i = t; i < nblk; i += 256) {
        if (i < nY) {
            const int ly = i / ybx, lx = i - ly * ybx;
            const long long by = mcy0 * vm + ly, bx = mcx0 * hm + lx;
            if (by < my * vm && bx < ybw) idct_block(coef + (base + by * ybw + bx) * 64, qs[0], luma + ly * 8 * kLumaLd + lx * 8, kLumaLd);
        } else {
            const int c = (i - nY) / nCg, j = (i - nY) - c * nCg;
            const int ly = j / cgx, lx = j - ly * cgx;  // (ly, lx) = 1 + block offset from the tile's first chroma block
            const long long by = mcy0 + ly - 1, bx = mcx0 + lx - 1;
            const bool need = ly >= 1 - hy && ly <= R + hy && lx >= 1 - hx && lx <= kTX + hx;
            if (need && by >= 0 && by < my && bx >= 0 && bx < mx)
                idct_block(coef + (cbase + c * cplane + by * mx + bx) * 64, qs[1 + c], chroma[c] + ly * 8 * kChromaLd + lx * 8, kChromaLd);
        }
    }
    __syncthreads();

    const int cols = ybx * 8, rows = R * ivm * 8;
    const long long X0 = mcx0 * hm * 8, Y0 = mcy0 * vm * 8;
    const long long cw = (W + hm - 1) / hm, ch = (H + vm - 1) / vm;
    const long long cX0 = (mcx0 - 1) * 8, cY0 = (mcy0 - 1) * 8;  // chroma sample at LDS (0, 0)
    // libjpeg takes the triangle ("fancy") upsamplers only for a component MORE than two samples wide; a chroma plane of one
    // or two columns is replicated (box), in both directions
    const bool fancy = cw > 2;
    uint8_t* out = raw + off;
    for (int i = t; i < rows * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        const long long Y = Y0 + ly, X = X0 + lx;
        if (Y >= H || X >= W) continue;
        const int y = luma[ly * kLumaLd + lx];
        int r = y, g = y, bl = y;
        if (nc == 3) {
            long long cx = X, nx = X, cy = Y, ny = Y;
            if (hx) {
                cx = X >> 1, nx = (X & 1) ? cx + 1 : cx - 1;
                nx = nx < 0 ? 0 : (nx > cw - 1 ? cw - 1 : nx);
            }
            if (hy) {
                cy = Y >> 1, ny = (Y & 1) ? cy + 1 : cy - 1;
                ny = ny < 0 ? 0 : (ny > ch - 1 ? ch - 1 : ny);
            }
            const int a = (int)(cy - cY0) * kChromaLd, an = (int)(ny - cY0) * kChromaLd, e = (int)(cx - cX0), en = (int)(nx - cX0);
            int cc[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint8_t* p = chroma[c];
                if (fancy && hx && hy) {
                    const int here = 3 * p[a + e] + p[an + e], there = 3 * p[a + en] + p[an + en];
                    cc[c] = (3 * here + there + ((X & 1) ? 7 : 8)) >> 4;
                } else if (fancy && hx) {
                    cc[c] = (3 * p[a + e] + p[a + en] + ((X & 1) ? 2 : 1)) >> 2;
                } else {
                    cc[c] = p[a + e];
                }
            }
            const int cb = cc[0] - 128, cr = cc[1] - 128;
            r = y + ((91881 * cr + 32768) >> 16);
            g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
            bl = y + ((116130 * cb + 32768) >> 16);
        }
        uint8_t* d = out + (Y * W + X) * 3;
        d[0] = (uint8_t)min(max(r, 0), 255);
        d[1] = (uint8_t)min(max(g, 0), 255);
        d[2] = (uint8_t)min(max(bl, 0), 255);
    }
}

}  // namespace

extern "C" {

int64_t vt_jpeg_scratch_bytes(int64_t blocks) { return blocks > 0 ? blocks * 128 : 0; }

int vt_jpeg_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* images, int32_t B, const int64_t* segments, int32_t S,
                    const uint8_t* hufftabs, int32_t NH, int16_t* coef, int64_t coef_blocks, int32_t* status, void* stream) {
    const char* who = "vt_jpeg_entropy";
    VT_REQUIRE(data && images && segments && hufftabs && coef && status, VT_ERR_INVALID,
               "%s: null pointer (data %p, images %p, segments %p, hufftabs %p, coef %p, status %p)", who, (const void*)data,
               (const void*)images, (const void*)segments, (const void*)hufftabs, (const void*)coef, (const void*)status);
    VT_REQUIRE(data_bytes > 0 && B > 0 && S > 0 && NH > 0 && coef_blocks > 0, VT_ERR_INVALID,
               "%s: non-positive size (data_bytes %lld, B %d, S %d, NH %d, coef_blocks %lld)", who, (long long)data_bytes, B, S, NH,
               (long long)coef_blocks);
    VT_REQUIRE((((uintptr_t)images) & 7) == 0 && (((uintptr_t)segments) & 7) == 0 && (((uintptr_t)status) & 3) == 0 &&
                   (((uintptr_t)data) & 3) == 0 && vt_aligned16(coef),
               VT_ERR_INVALID, "%s: misaligned images / segments (8), status / data (4) or coef (16)", who);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, data, (long long)data_bytes,
                       (const long long*)images, B, (const long long*)segments, S, hufftabs, NH, (short*)coef,
                       (long long)coef_blocks, status);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int vt_jpeg_idct_rgb(const int16_t* coef, int64_t coef_blocks, const int64_t* images, int32_t B, const uint8_t* qtabs, int32_t NQ,
                     uint8_t* raw, int64_t raw_bytes, int32_t max_mcus_x, int32_t max_mcus_y, int32_t band_mcu_rows, void* stream) {
    const char* who = "vt_jpeg_idct_rgb";
    VT_REQUIRE(coef && images && qtabs && raw, VT_ERR_INVALID, "%s: null pointer (coef %p, images %p, qtabs %p, raw %p)", who,
               (const void*)coef, (const void*)images, (const void*)qtabs, (const void*)raw);
    VT_REQUIRE(coef_blocks > 0 && B > 0 && NQ > 0 && raw_bytes > 0 && max_mcus_x > 0 && max_mcus_y > 0, VT_ERR_INVALID,
               "%s: non-positive size (coef_blocks %lld, B %d, NQ %d, raw_bytes %lld, max_mcus_x %d, max_mcus_y %d)", who,
               (long long)coef_blocks, B, NQ, (long long)raw_bytes, max_mcus_x, max_mcus_y);
    VT_REQUIRE((((uintptr_t)images) & 7) == 0 && vt_aligned16(coef), VT_ERR_INVALID, "%s: misaligned images (8) or coef (16)", who);
    VT_REQUIRE(band_mcu_rows >= 0 && band_mcu_rows <= kMaxR, VT_ERR_INVALID, "%s: band_mcu_rows %d is outside 0 .. %d", who,
               band_mcu_rows, kMaxR);
    const int R = band_mcu_rows == 0 ? kMaxR : band_mcu_rows;
    const long tiles = ((long)max_mcus_x + kTX - 1) / kTX, bands = ((long)max_mcus_y + R - 1) / R;
    VT_REQUIRE(B <= 65535 && bands <= 65535 && tiles * bands * B < (1L << 31), VT_ERR_INVALID,
               "%s: a grid of %ld x %ld x %d workgroups", who, tiles, bands, B);
    hipLaunchKernelGGL(jpeg_idct_rgb_kernel, dim3((unsigned)tiles, (unsigned)bands, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const short*)coef, (long long)coef_blocks, (const long long*)images, B, qtabs, NQ, raw, (long long)raw_bytes, R);
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

}  // extern "C"
