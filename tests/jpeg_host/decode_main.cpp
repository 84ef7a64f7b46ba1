// decode_main.cpp -- the entropy stage of the JPEG decoder (csrc/vt_jpeg_bits.h, the code the kernel runs) as a stand-alone
// host program, built by tests/test_jpeg_cpu.py with -fsanitize=address,undefined and run as a child process.
//
//   decode_main <cases.bin> <out.bin>
//
// cases.bin: int64 count, then per case
//   int64 [8]  = bytes, components, h_max, v_max, MCUs per row, MCU rows, segments, 0
//   uint8 [6][272]  BITS + HUFFVAL of DC0, AC0, DC1, AC1, DC2, AC2 (the unused ones zero)
//   int64 [segments][4] = first byte, one past the last byte, first MCU, MCU count
//   uint8 [bytes]  the file (or any byte string)
// out.bin: per case int32 [segments] statuses, then int16 [blocks][64] coefficients in the layout of vt_amd.h.
//
// Every case's bytes are copied into a heap block of EXACTLY their length, so a read outside [0, bytes) is an
// AddressSanitizer report; the segment loop restates the kernel's (same checks on the table rows, same order of blocks).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vt_jpeg_bits.h"

static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct ArraySink {
    int16_t* block;
    void put(int k, int v) { block[kNatural[k]] = (int16_t)v; }
};

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    int64_t count = 0;
    if (!read_exact(in, &count, 8)) return 2;
    for (int64_t ci = 0; ci < count; ++ci) {
        int64_t hd[8];
        if (!read_exact(in, hd, sizeof hd)) return 2;
        const int64_t bytes = hd[0], nc = hd[1], hm = hd[2], vm = hd[3], mx = hd[4], my = hd[5], nseg = hd[6];
        if (bytes < 0 || bytes > (1 << 26) || (nc != 1 && nc != 3) || (hm != 1 && hm != 2) || (vm != 1 && vm != 2) || mx < 1 ||
            mx > 4096 || my < 1 || my > 4096 || nseg < 0 || nseg > (1 << 20)) {
            fprintf(stderr, "case %lld: bad header\n", (long long)ci);
            return 2;
        }
        uint8_t tabs[6][272];
        std::vector<int64_t> segs((size_t)nseg * 4);
        uint8_t* data = (uint8_t*)malloc(bytes ? (size_t)bytes : 1);  // exactly `bytes` long: an over-read is an ASan report
        if (!read_exact(in, tabs, sizeof tabs) || !read_exact(in, segs.data(), segs.size() * 8) || !read_exact(in, data, (size_t)bytes))
            return 2;

        const int64_t nY = mx * hm * my * vm, blocks = nY + (nc == 3 ? 2 * mx * my : 0);
        std::vector<int16_t> coef((size_t)blocks * 64, 0);
        std::vector<int32_t> status((size_t)nseg, 0);
        VtJpegHuff tab[6];
        int table_status = VT_JPEG_OK;
        for (int t = 0; t < 2 * nc; ++t) {
            vt_jpeg_huff_build(tabs[t], &tab[t]);
            if (!tab[t].valid) table_status = VT_JPEG_ERR_TABLE;
        }
        for (int64_t s = 0; s < nseg; ++s) {
            const int64_t begin = segs[4 * s], end = segs[4 * s + 1], m0 = segs[4 * s + 2], mc = segs[4 * s + 3];
            if (!(begin >= 0 && begin <= end && end <= bytes && m0 >= 0 && mc >= 0 && m0 <= mx * my && mc <= mx * my - m0)) {
                status[s] = VT_JPEG_ERR_TABLE;
                continue;
            }
            VtJpegPtrSrc src{data};
            VtJpegBits r;
            vt_jpeg_bits_init(&r, begin, end);
            int pred[3] = {0, 0, 0};
            int st = table_status;
            for (int64_t m = 0; m < mc; ++m) {
                const int64_t mcu = m0 + m, mcx = mcu % mx, mcy = mcu / mx;
                for (int c = 0; c < nc; ++c) {
                    const int hc = c == 0 ? (int)hm : 1, vc = c == 0 ? (int)vm : 1;
                    for (int v = 0; v < vc; ++v)
                        for (int h = 0; h < hc; ++h) {
                            const int64_t blk = c == 0 ? (mcy * vm + v) * mx * hm + mcx * hm + h : nY + (c - 1) * mx * my + mcy * mx + mcx;
                            int16_t* b = coef.data() + blk * 64;
                            memset(b, 0, 128);
                            if (st != VT_JPEG_OK) continue;
                            ArraySink sink{b};
                            int rc = vt_jpeg_block(&r, src, &tab[2 * c], tabs[2 * c] + 16, &tab[2 * c + 1], tabs[2 * c + 1] + 16, &pred[c], sink);
                            if (rc == VT_JPEG_OK && vt_jpeg_overrun(&r) > 0) rc = VT_JPEG_ERR_TRUNCATED;
                            if (rc != VT_JPEG_OK) st = rc, memset(b, 0, 128);
                        }
                }
            }
            if (st == VT_JPEG_OK && vt_jpeg_unread(&r) >= 8) st = VT_JPEG_ERR_TRAILING;
            status[s] = st;
        }
        fwrite(status.data(), 4, status.size(), out);
        fwrite(coef.data(), 2, coef.size(), out);
        free(data);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("decoded %lld cases\n", (long long)count);
    return 0;
}
