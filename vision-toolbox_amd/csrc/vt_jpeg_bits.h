// vt_jpeg_bits.h -- the bit reader and the Huffman symbol decoder of the baseline JPEG entropy stage, shared by the kernel
// (vt_jpeg.hip) and by a plain C++ host build (tests/jpeg_host/decode_main.cpp, which runs it under the host sanitizers).
//
// It is the only code of the library whose control flow follows UNTRUSTED bytes, so everything here is written to be safe
// for ANY byte string and ANY table contents:
//   * a byte is read only at an index in [begin, end) of the segment; past the end, or after a marker (FF followed by
//     anything but 00) inside the segment, the reader supplies zero bits, as libjpeg pads, and counts them;
//   * vt_jpeg_fill runs at most 8 iterations, vt_jpeg_symbol at most 16, vt_jpeg_block's coefficient loop at most 63: every
//     iteration consumes one symbol and moves the coefficient index forward by at least one;
//   * an index into HUFFVAL is checked against the table's value count before it is used;
//   * a derived table whose BITS over-subscribe the code space, or that counts more than 256 values, is marked invalid
//     and never decoded from.
// No code here stores anywhere but through the caller's sink and the reader's own state.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VT_JPEG_HD __host__ __device__ inline
#define VT_JPEG_HD_MEMBER __host__ __device__
#else
#define VT_JPEG_HD inline
#define VT_JPEG_HD_MEMBER
#endif

// status of an entropy segment (vt_amd.h documents them); 0 = clean
#define VT_JPEG_OK 0
#define VT_JPEG_ERR_CODE 1       // a bit pattern that is no code of the table (or longer than 16 bits), or a DC size > 15
#define VT_JPEG_ERR_RUN 2        // a zero run that passes coefficient 63
#define VT_JPEG_ERR_TRUNCATED 3  // the blocks needed bits past the end of the segment (or past a marker inside it)
#define VT_JPEG_ERR_TABLE 4      // a table row that is out of range, or a Huffman table that is not a prefix code
#define VT_JPEG_ERR_TRAILING 5   // every block decoded, but 8 or more bits of the segment were left over

// T.81 F.2.2.3: the decoding tables derived from BITS; values are looked up in HUFFVAL at code + valoff[l]
struct VtJpegHuff {
    int32_t maxcode[17];  // [l] the largest code of length l, -1 if there is none (l = 1 .. 16)
    int32_t valoff[17];   // [l] index of the first value of length l minus the smallest code of length l
    int32_t count;        // values in HUFFVAL
    int32_t valid;
};

VT_JPEG_HD void vt_jpeg_huff_build(const uint8_t* bits, VtJpegHuff* h) {
    int32_t code = 0, k = 0, valid = 1;
    h->maxcode[0] = -1, h->valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int32_t n = bits[l - 1];
        h->valoff[l] = k - code;
        k += n, code += n;
        h->maxcode[l] = n ? code - 1 : -1;
        if (code > (1 << l)) valid = 0;  // more codes of this length than the code space has left
        code <<= 1;
    }
    h->count = k;
    h->valid = valid && k <= 256;
}

// A byte source is any type with `uint32_t get(int64_t pos)`; it is only called with begin <= pos < end.
struct VtJpegPtrSrc {
    const uint8_t* p;
    VT_JPEG_HD_MEMBER uint32_t get(int64_t pos) { return p[pos]; }
};

struct VtJpegBits {
    int64_t pos, end;  // next byte, one past the last byte of the segment
    uint64_t acc;      // the low `nbits` bits are the unread bits, most significant first
    int32_t nbits;
    int64_t padded;    // zero bits supplied so far; they are always the LAST bits pushed
};

VT_JPEG_HD void vt_jpeg_bits_init(VtJpegBits* r, int64_t begin, int64_t end) {
    r->pos = begin, r->end = end > begin ? end : begin;
    r->acc = 0, r->nbits = 0, r->padded = 0;
}

// at least 57 unread bits afterwards; FF 00 is the byte FF, FF followed by anything else ends the data of the segment
template <class Src>
VT_JPEG_HD void vt_jpeg_fill(VtJpegBits* r, Src& src) {
    while (r->nbits <= 56) {
        uint32_t b = 0;
        if (r->pos < r->end) {
            b = src.get(r->pos++);
            if (b == 0xFF) {
                if (r->pos < r->end && src.get(r->pos) == 0) {
                    r->pos++;
                } else {
                    r->pos = r->end, b = 0, r->padded += 8;
                }
            }
        } else {
            r->padded += 8;
        }
        r->acc = (r->acc << 8) | b;
        r->nbits += 8;
    }
}

// zero bits that were not only supplied but CONSUMED
VT_JPEG_HD int64_t vt_jpeg_overrun(const VtJpegBits* r) { return r->padded > r->nbits ? r->padded - r->nbits : 0; }
// bits of the segment itself that are still unread (whole bytes not yet fetched included)
VT_JPEG_HD int64_t vt_jpeg_unread(const VtJpegBits* r) {
    const int64_t in_acc = r->nbits > r->padded ? r->nbits - r->padded : 0;
    return in_acc + 8 * (r->end - r->pos);
}

// n in 1 .. 16 of the (at least 16) unread bits, without consuming them
VT_JPEG_HD uint32_t vt_jpeg_peek(const VtJpegBits* r, int n) { return (uint32_t)(r->acc >> (r->nbits - n)) & ((1u << n) - 1u); }

// one Huffman symbol, or -1 for a bit pattern that is no code.  The caller has filled the reader (>= 16 unread bits).
VT_JPEG_HD int vt_jpeg_symbol(VtJpegBits* r, const VtJpegHuff* h, const uint8_t* huffval) {
    const int32_t look = (int32_t)vt_jpeg_peek(r, 16);
    for (int l = 1; l <= 16; ++l) {
        const int32_t code = look >> (16 - l);
        if (code <= h->maxcode[l]) {
            const int32_t idx = code + h->valoff[l];
            if (idx < 0 || idx >= h->count) return -1;
            r->nbits -= l;
            return huffval[idx];
        }
    }
    return -1;
}

// T.81 F.2.2.1 RECEIVE + EXTEND for s in 1 .. 15
VT_JPEG_HD int vt_jpeg_receive_extend(VtJpegBits* r, int s) {
    const int v = (int)vt_jpeg_peek(r, s);
    r->nbits -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One 8 x 8 block.  sink.put(k, v) receives the coefficient at ZIGZAG position k (0 = DC, already predicted); positions it
// is not called for are zero.  *pred is the DC predictor, kept as an int16 value.  Returns a VT_JPEG_* status.
template <class Src, class Sink>
VT_JPEG_HD int vt_jpeg_block(VtJpegBits* r, Src& src, const VtJpegHuff* dc, const uint8_t* dcval, const VtJpegHuff* ac,
                             const uint8_t* acval, int* pred, Sink& sink) {
    vt_jpeg_fill(r, src);
    int s = vt_jpeg_symbol(r, dc, dcval);
    if (s < 0 || s > 15) return VT_JPEG_ERR_CODE;
    if (s) *pred = (int16_t)(*pred + vt_jpeg_receive_extend(r, s));
    sink.put(0, *pred);
    for (int k = 1; k < 64;) {  // <= 63 iterations: each one consumes a symbol and adds at least 1 to k
        vt_jpeg_fill(r, src);
        const int rs = vt_jpeg_symbol(r, ac, acval);
        if (rs < 0) return VT_JPEG_ERR_CODE;
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (run != 15) break;  // EOB (libjpeg reads every other run with size 0 as the end of the block too)
            if (k + 15 > 63) return VT_JPEG_ERR_RUN;
            k += 16;
            continue;
        }
        k += run;
        if (k > 63) return VT_JPEG_ERR_RUN;
        sink.put(k, vt_jpeg_receive_extend(r, s));
        ++k;
    }
    return VT_JPEG_OK;
}
