// vt_patchconv.hip -- the kernels of the PatchConvNet family (reference backbones/patchconvnet.py:25-103).
//
//   vt_dw3_gelu_pool_fwd / _bwd   the depthwise 3x3 + GELU column of a block together with the global average pool that
//                                 feeds its Squeeze-Excitation: a = GELU(dwconv3x3_pad1(u, w) + bias), pooled = mean(a)
//   vt_se_gate_fwd / _bwd         y = a * sigmoid(s[b][c]) (the sigmoid gate; vt_ese_gate_* is the hard-sigmoid one)
//   vt_channel_stats              per-channel sum / sum of squares of a stored map (a BatchNorm IN FRONT of its convolution
//                                 has no conv epilogue to take them from), the statistics contract of VT_CONV_STATS
//   vt_pool_attn_fwd / _bwd       softmax attention of ONE query row per image with ONE head of any width
//
// Ownership instead of atomics.  The plane kernels and the gate's backward give a workgroup one image and one slab of
// channels and let it walk ALL pixels of that slab: every per-(image, channel) sum -- the pooled mean, the gate's d(s),
// an image's share of the filter and bias gradient -- has one owner and a fixed order (registers -> xor shuffles ->
// the four waves in order), so the results are bit-identical from run to run without a float atomic anywhere.  The
// shares of the filter gradient go to a scratch [B][C][10] and a second small kernel adds them over the images in
// image order.
//
// The plane kernels stage the slab's u plane with a zero halo in LDS (every input element leaves HBM once); the backward
// keeps dz = (d(a) + d(pooled) / HW) * GELU'(z) in a second, f32, plane, recomputing z -- it is never stored.  A slab is
// 4 chunks of 16 bytes wide (a lane group reads 64 contiguous bytes of a pixel row) where the planes fit the 160 KiB of
// LDS, else 2, else 1; a map whose planes do not fit at one chunk is refused.
//
// Arithmetic is f32 from storage-rounded operands; bf16 launches round the filter as vt_dwconv_fwd does.
#include <stdlib.h>

#include "vt_common.h"

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kLdsMax = 160 * 1024;

__device__ __forceinline__ float gelu_f(float u) { return 0.5f * u * (1.f + erff(u * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float u) {
    return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * 0.3989422804014327f * expf(-0.5f * u * u);
}
__device__ __forceinline__ float sigmoid_f(float u) { return 1.f / (1.f + expf(-u)); }

template <typename T>
__device__ __forceinline__ float load1(const T* p) { return (float)*p; }

// sum over the lanes of a wave that share `lane % group` (group: a power of two <= 64), fixed order
__device__ __forceinline__ float group_sum(float v, int group) {
    for (int off = group; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- depthwise 3x3 + GELU + pool ------------------------------------------------------------------------------------
struct PlaneArgs {
    const void* u;
    const void* da;
    const void* dp;
    const float* w;
    const float* bias;
    void* a;
    void* pooled;
    void* du;
    const void* res;
    float* scratch;
    int B, H, W, C;
    int ldu, lda, ldp, ldda, lddp, lddu, ldr;
    int SCH;     // nominal 16-byte chunks per slab: 1, 2 or 4
    int nslabs;  // ceil(chunks per row / SCH)
};

template <typename T>
__device__ __forceinline__ void load_filter(const PlaneArgs& a, int c0, bool on, float (&wv)[9][VecIO<T>::EPC],
                                            float (&bv)[VecIO<T>::EPC]) {
#pragma unroll
    for (int e = 0; e < VecIO<T>::EPC; ++e) {
#pragma unroll
        for (int t = 0; t < 9; ++t) wv[t][e] = on ? VecIO<T>::round(a.w[(long)(c0 + e) * 9 + t]) : 0.f;
        bv[e] = (on && a.bias) ? a.bias[c0 + e] : 0.f;
    }
}

// the slab's u plane with a zero halo: plane[(H + 2) * (W + 2)][SCH] chunks
template <typename T>
__device__ __forceinline__ void stage_plane(const PlaneArgs& a, uint4* plane, int b, int chunk0, int nch) {
    const T* u = (const T*)a.u;
    const int PW = a.W + 2, total = (a.H + 2) * PW * a.SCH;
    for (int idx = threadIdx.x; idx < total; idx += kT) {
        const int pp = idx / a.SCH, cc = idx - pp * a.SCH;
        const int ph = pp / PW, pw = pp - ph * PW;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (ph >= 1 && ph <= a.H && pw >= 1 && pw <= a.W && cc < nch)
            v = *(const uint4*)(u + (((long)b * a.H + (ph - 1)) * a.W + (pw - 1)) * a.ldu + (long)(chunk0 + cc) * VecIO<T>::EPC);
        plane[idx] = v;
    }
}

template <typename T>
__global__ void __launch_bounds__(kT) dw3_gelu_pool_fwd_kernel(const PlaneArgs a) {
    constexpr int EPC = VecIO<T>::EPC;
    extern __shared__ uint4 smem4[];
    const int PW = a.W + 2, HW = a.H * a.W;
    uint4* plane = smem4;
    float* red = (float*)(smem4 + (a.H + 2) * PW * a.SCH);  // [kWaves][SCH][EPC]
    const int b = blockIdx.x / a.nslabs, slab = blockIdx.x - b * a.nslabs;
    const int CPR = a.C / EPC, chunk0 = slab * a.SCH;
    const int nch = min(a.SCH, CPR - chunk0);
    const int t = threadIdx.x, tpix = t / a.SCH, ch = t - tpix * a.SCH, NP = kT / a.SCH;
    const bool on = ch < nch;
    const int c0 = (chunk0 + (on ? ch : 0)) * EPC;
    float wv[9][EPC], bv[EPC], psum[EPC];
    load_filter<T>(a, c0, on, wv, bv);
#pragma unroll
    for (int e = 0; e < EPC; ++e) psum[e] = 0.f;
    stage_plane<T>(a, plane, b, chunk0, nch);
    __syncthreads();
    T* out = (T*)a.a;
    if (on)
        for (int p = tpix; p < HW; p += NP) {
            const int h = p / a.W, w_ = p - h * a.W;
            float acc[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                float xv[EPC];
                VecIO<T>::unpack(plane[((h + tap / 3) * PW + w_ + tap % 3) * a.SCH + ch], xv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] = fmaf(xv[e], wv[tap][e], acc[e]);
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = gelu_f(acc[e] + bv[e]);
            const uint4 o = VecIO<T>::pack(acc);
            *(uint4*)(out + ((long)b * HW + p) * a.lda + c0) = o;
            float rv[EPC];
            VecIO<T>::unpack(o, rv);  // the pooled mean is taken over the STORED values
#pragma unroll
            for (int e = 0; e < EPC; ++e) psum[e] += rv[e];
        }
#pragma unroll
    for (int e = 0; e < EPC; ++e) psum[e] = group_sum(psum[e], a.SCH);
    if ((t & 63) < a.SCH)
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[((t >> 6) * a.SCH + ch) * EPC + e] = psum[e];
    __syncthreads();
    if (t < nch * EPC) {
        float s = 0.f;
        for (int wv_ = 0; wv_ < kWaves; ++wv_) s += red[wv_ * a.SCH * EPC + t];
        ((T*)a.pooled)[(long)b * a.ldp + chunk0 * EPC + t] = from_float<T>(s / (float)HW);
    }
}

template <typename T>
__global__ void __launch_bounds__(kT) dw3_gelu_pool_bwd_kernel(const PlaneArgs a) {
    constexpr int EPC = VecIO<T>::EPC;
    extern __shared__ uint4 smem4[];
    const int PW = a.W + 2, HW = a.H * a.W, cells = (a.H + 2) * PW * a.SCH;
    uint4* plane = smem4;
    float* dzp = (float*)(smem4 + cells);  // [cells][EPC], zero halo
    float* red = dzp + (long)cells * EPC;  // [kWaves][SCH][10][EPC]
    const int b = blockIdx.x / a.nslabs, slab = blockIdx.x - b * a.nslabs;
    const int CPR = a.C / EPC, chunk0 = slab * a.SCH;
    const int nch = min(a.SCH, CPR - chunk0);
    const int t = threadIdx.x, tpix = t / a.SCH, ch = t - tpix * a.SCH, NP = kT / a.SCH;
    const bool on = ch < nch;
    const int c0 = (chunk0 + (on ? ch : 0)) * EPC;
    float wv[9][EPC], bv[EPC], dwa[10][EPC], dpn[EPC];
    load_filter<T>(a, c0, on, wv, bv);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
#pragma unroll
        for (int j = 0; j < 10; ++j) dwa[j][e] = 0.f;
        dpn[e] = (on && a.dp) ? load1((const T*)a.dp + (long)b * a.lddp + c0 + e) / (float)HW : 0.f;
    }
    stage_plane<T>(a, plane, b, chunk0, nch);
    for (int idx = t; idx < cells * EPC; idx += kT) dzp[idx] = 0.f;
    __syncthreads();
    const T* da = (const T*)a.da;
    if (on)
        for (int p = tpix; p < HW; p += NP) {
            const int h = p / a.W, w_ = p - h * a.W;
            float z[EPC], g[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) z[e] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                float xv[EPC];
                VecIO<T>::unpack(plane[((h + tap / 3) * PW + w_ + tap % 3) * a.SCH + ch], xv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) z[e] = fmaf(xv[e], wv[tap][e], z[e]);
            }
            if (da) {
                VecIO<T>::unpack(*(const uint4*)(da + ((long)b * HW + p) * a.ldda + c0), g);
            } else {
#pragma unroll
                for (int e = 0; e < EPC; ++e) g[e] = 0.f;
            }
            float* cell = dzp + ((long)((h + 1) * PW + w_ + 1) * a.SCH + ch) * EPC;
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                g[e] = (g[e] + dpn[e]) * gelu_d(z[e] + bv[e]);
                cell[e] = g[e];
                dwa[9][e] += g[e];
            }
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                float xv[EPC];
                VecIO<T>::unpack(plane[((h + tap / 3) * PW + w_ + tap % 3) * a.SCH + ch], xv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) dwa[tap][e] = fmaf(g[e], xv[e], dwa[tap][e]);
            }
        }
    __syncthreads();
    // du(h, w) = sum over the taps of dz(h + 1 - kr, w + 1 - kc) * w[kr][kc]
    if (on && a.du) {
        T* du = (T*)a.du;
        const T* res = (const T*)a.res;
        for (int p = tpix; p < HW; p += NP) {
            const int h = p / a.W, w_ = p - h * a.W;
            float acc[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float* cell = dzp + ((long)((h + 2 - tap / 3) * PW + w_ + 2 - tap % 3) * a.SCH + ch) * EPC;
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] = fmaf(cell[e], wv[tap][e], acc[e]);
            }
            const long at = ((long)b * HW + p);
            if (res) {  // (the sum is rounded to the storage type first, as a data-gradient launch + add would)
                float rv[EPC], sv[EPC];
                VecIO<T>::unpack(VecIO<T>::pack(acc), sv);
                VecIO<T>::unpack(*(const uint4*)(res + at * a.ldr + c0), rv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] = sv[e] + rv[e];
            }
            *(uint4*)(du + at * a.lddu + c0) = VecIO<T>::pack(acc);
        }
    }
    // this image's share of dw[c][9] and dbias[c]
#pragma unroll
    for (int j = 0; j < 10; ++j)
#pragma unroll
        for (int e = 0; e < EPC; ++e) dwa[j][e] = group_sum(dwa[j][e], a.SCH);
    if ((t & 63) < a.SCH)
#pragma unroll
        for (int j = 0; j < 10; ++j)
#pragma unroll
            for (int e = 0; e < EPC; ++e) red[(((t >> 6) * a.SCH + ch) * 10 + j) * EPC + e] = dwa[j][e];
    __syncthreads();
    for (int r = t; r < nch * 10 * EPC; r += kT) {
        const int cc = r / (10 * EPC), rem = r - cc * 10 * EPC;
        const int e = rem / 10, j = rem - e * 10;
        float s = 0.f;
        for (int wv_ = 0; wv_ < kWaves; ++wv_) s += red[((wv_ * a.SCH + cc) * 10 + j) * EPC + e];
        a.scratch[((long)b * a.C + (chunk0 + cc) * EPC + e) * 10 + j] = s;
    }
}

// dw[c][t] += sum over the images, in image order, of scratch[b][c][t]; dbias[c] += ... [9]
__global__ void __launch_bounds__(kT) dw3_share_sum_kernel(const float* scratch, float* dw, float* dbias, int B, int C) {
    const int idx = blockIdx.x * kT + threadIdx.x;
    if (idx >= C * 10) return;
    const int c = idx / 10, j = idx - c * 10;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += scratch[((long)b * C + c) * 10 + j];
    if (j < 9) {
        if (dw) dw[c * 9 + j] += s;
    } else if (dbias) {
        dbias[c] += s;
    }
}

long plane_lds_bytes(int H, int W, int sch, int dtype, bool bwd) {
    const long cells = (long)(H + 2) * (W + 2) * sch;
    const int epc = vt_epc(dtype);
    return cells * 16 + (bwd ? cells * epc * 4 : 0) + (long)kWaves * sch * (bwd ? 10 : 1) * epc * 4;
}

int plane_fill(PlaneArgs& a, const char* who, int B, int H, int W, int C, int dtype, bool bwd, long* lds) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, VT_ERR_INVALID, "%s: bad geometry", who);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C % epc == 0, VT_ERR_UNSUPPORTED, "%s: C=%d must be a multiple of %d", who, C, epc);
    VT_REQUIRE((long)B * H * W < (1L << 31) / 4, VT_ERR_UNSUPPORTED, "%s: %d x %d x %d pixels", who, B, H, W);
    const int cpr = C / epc;
    int sch = 4;
    while (sch > 1 && (sch > cpr || plane_lds_bytes(H, W, sch, dtype, bwd) > kLdsMax)) sch >>= 1;
    *lds = plane_lds_bytes(H, W, sch, dtype, bwd);
    VT_REQUIRE(*lds <= kLdsMax, VT_ERR_UNSUPPORTED,
               "%s: the planes of a %dx%d map need %ld bytes of LDS at a slab of one 16-byte chunk, the limit is %d", who, H, W, *lds,
               kLdsMax);
    a.B = B, a.H = H, a.W = W, a.C = C, a.SCH = sch, a.nslabs = (cpr + sch - 1) / sch;
    return VT_OK;
}

bool mat_ok(const void* p, int ld, int C, int dtype) { return p && ld >= C && ld % vt_epc(dtype) == 0 && vt_aligned16(p); }

// ---- the sigmoid gate -----------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kT) se_gate_fwd_kernel(const T* a, int lda, const T* s, int lds, T* y, int ldy, long items, int HW,
                                                         int CPR) {
    constexpr int EPC = VecIO<T>::EPC;
    for (long it = (long)blockIdx.x * kT + threadIdx.x; it < items; it += (long)gridDim.x * kT) {
        const long row = it / CPR;
        const int c0 = (int)(it - row * CPR) * EPC;
        const long b = row / HW;
        float av[EPC], sv[EPC];
        VecIO<T>::unpack(*(const uint4*)(a + row * lda + c0), av);
        VecIO<T>::unpack(*(const uint4*)(s + b * lds + c0), sv);
#pragma unroll
        for (int e = 0; e < EPC; ++e) av[e] *= sigmoid_f(sv[e]);
        *(uint4*)(y + row * ldy + c0) = VecIO<T>::pack(av);
    }
}

// one workgroup per (image, slab of SCH chunks): d(a) (+)= dy * sigmoid(s), ds[b][c] = sigmoid'(s) * sum_pixels dy * a
template <typename T>
__global__ void __launch_bounds__(kT) se_gate_bwd_kernel(const T* dy, int lddy, const T* a, int lda, const T* s, int lds, T* da,
                                                         int ldda, float* ds, int HW, int C, int SCH, int nslabs, int accumulate) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float red[kWaves * 4 * 8];
    const int b = blockIdx.x / nslabs, slab = blockIdx.x - b * nslabs;
    const int CPR = C / EPC, chunk0 = slab * SCH;
    const int nch = min(SCH, CPR - chunk0);
    const int t = threadIdx.x, tpix = t / SCH, ch = t - tpix * SCH, NP = kT / SCH;
    const bool on = ch < nch;
    const int c0 = (chunk0 + (on ? ch : 0)) * EPC;
    float sg[EPC], sum[EPC];
    {
        float sv[EPC];
        VecIO<T>::unpack(*(const uint4*)(s + (long)b * lds + c0), sv);
#pragma unroll
        for (int e = 0; e < EPC; ++e) sg[e] = sigmoid_f(sv[e]), sum[e] = 0.f;
    }
    if (on)
        for (int p = tpix; p < HW; p += NP) {
            const long row = (long)b * HW + p;
            float gv[EPC], av[EPC], ov[EPC];
            VecIO<T>::unpack(*(const uint4*)(dy + row * lddy + c0), gv);
            VecIO<T>::unpack(*(const uint4*)(a + row * lda + c0), av);
#pragma unroll
            for (int e = 0; e < EPC; ++e) sum[e] = fmaf(gv[e], av[e], sum[e]), ov[e] = gv[e] * sg[e];
            if (accumulate) {
                float pv[EPC], rv[EPC];
                VecIO<T>::unpack(VecIO<T>::pack(ov), rv);
                VecIO<T>::unpack(*(const uint4*)(da + row * ldda + c0), pv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) ov[e] = rv[e] + pv[e];
            }
            *(uint4*)(da + row * ldda + c0) = VecIO<T>::pack(ov);
        }
#pragma unroll
    for (int e = 0; e < EPC; ++e) sum[e] = group_sum(sum[e], SCH);
    if ((t & 63) < SCH)
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[((t >> 6) * SCH + ch) * EPC + e] = sum[e] * sg[e] * (1.f - sg[e]);
    __syncthreads();
    if (t < nch * EPC) {
        float v = 0.f;
        for (int wv_ = 0; wv_ < kWaves; ++wv_) v += red[wv_ * SCH * EPC + t];
        ds[(long)b * C + chunk0 * EPC + t] = v;
    }
}

// ---- per-channel statistics of a stored map ------------------------------------------------------------------------
// A thread owns one 16-byte chunk of a row and walks `iters` rows; the RT row lanes of the workgroup that share a chunk are
// then added in row-lane order through LDS, so a workgroup issues ONE fixed-point atomic per channel and sum (integer
// atomics: order-free, run-to-run identical).  Without the fold every thread would issue its own 2 EPC atomics on the same
// few hundred addresses.
template <typename T>
__global__ void __launch_bounds__(kT) channel_stats_kernel(const T* x, int ldx, long M, int C, int CPR, int CT, int RT, int iters,
                                                           float* stats) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float red[kT * 2 * 8];
    const int t = threadIdx.x;
    const int r = t / CT, tc = t - r * CT;
    const bool active = r < RT;
    const long row0 = (long)blockIdx.x * RT * iters + r;
    const int rep = blockIdx.x % kStatReplicas;
    for (int col0 = 0; col0 < CPR; col0 += CT) {
        const int col = col0 + tc;
        const int c0 = col * EPC;
        float s1[EPC], s2[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = 0.f;
        if (active && col < CPR)
            for (int it = 0; it < iters; ++it) {
                const long row = row0 + (long)it * RT;
                if (row >= M) break;
                float xv[EPC];
                VecIO<T>::unpack(*(const uint4*)(x + row * ldx + c0), xv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) s1[e] += xv[e], s2[e] = fmaf(xv[e], xv[e], s2[e]);
            }
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[(t * 2 + 0) * EPC + e] = s1[e], red[(t * 2 + 1) * EPC + e] = s2[e];
        __syncthreads();
        if (r == 0 && col < CPR) {
            for (int rr = 1; rr < RT; ++rr)
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    s1[e] += red[((rr * CT + tc) * 2 + 0) * EPC + e];
                    s2[e] += red[((rr * CT + tc) * 2 + 1) * EPC + e];
                }
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                vt_stat_add(stats, ((long)rep * 2 + 0) * C + c0 + e, s1[e]);
                vt_stat_add(stats, ((long)rep * 2 + 1) * C + c0 + e, s2[e]);
            }
        }
        __syncthreads();
    }
}

// ---- attention pooling: one query row, one head -------------------------------------------------------------------------
struct PoolArgs {
    const void *q, *k, *v, *o, *dout;
    const float* lse_in;
    void *out, *dq, *dk, *dv;
    float* lse;
    float scale;
    int B, Lk, C;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <typename T>
__global__ void __launch_bounds__(kT) pool_attn_fwd_kernel(const PoolArgs a) {
    constexpr int EPC = VecIO<T>::EPC;
    extern __shared__ float smem[];
    float* qs = smem;             // [C]
    float* sc = qs + a.C;         // [Lk]: scores, then probabilities (unnormalised)
    float* red = sc + a.Lk;       // [kT][EPC]
    float* wr = red + kT * EPC;   // [8]
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, CPR = a.C / EPC;
    const T* q = (const T*)a.q + (long)b * a.ldq;
    const T* k = (const T*)a.k + (long)b * a.Lk * a.ldk;
    const T* v = (const T*)a.v + (long)b * a.Lk * a.ldv;
    for (int ch = t; ch < CPR; ch += kT) {
        float f[EPC];
        VecIO<T>::unpack(*(const uint4*)(q + ch * EPC), f);
#pragma unroll
        for (int e = 0; e < EPC; ++e) qs[ch * EPC + e] = f[e];
    }
    __syncthreads();
    for (int j = wave; j < a.Lk; j += kWaves) {  // waves split the keys, lanes the channels
        float d = 0.f;
        for (int ch = lane; ch < CPR; ch += 64) {
            float f[EPC];
            VecIO<T>::unpack(*(const uint4*)(k + (long)j * a.ldk + ch * EPC), f);
#pragma unroll
            for (int e = 0; e < EPC; ++e) d = fmaf(f[e], qs[ch * EPC + e], d);
        }
        d = wave_sum(d);
        if (lane == 0) sc[j] = d * a.scale;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = t; j < a.Lk; j += kT) m = fmaxf(m, sc[j]);
    m = wave_max(m);
    if (lane == 0) wr[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wr[0], wr[1]), fmaxf(wr[2], wr[3]));
    float s = 0.f;
    for (int j = t; j < a.Lk; j += kT) {
        const float p = expf(sc[j] - m);
        sc[j] = p;
        s += p;
    }
    s = wave_sum(s);
    if (lane == 0) wr[4 + wave] = s;
    __syncthreads();
    const float total = ((wr[4] + wr[5]) + wr[6]) + wr[7];
    if (t == 0) a.lse[b] = m + logf(total);
    // P V: lanes own channels, the key groups' partial rows are added in group order
    const int ng = kT / CPR, g = t / CPR, ch = t - g * CPR;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    if (g < ng)
        for (int j = g; j < a.Lk; j += ng) {
            float f[EPC];
            VecIO<T>::unpack(*(const uint4*)(v + (long)j * a.ldv + ch * EPC), f);
            const float p = sc[j];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaf(p, f[e], acc[e]);
        }
#pragma unroll
    for (int e = 0; e < EPC; ++e) red[t * EPC + e] = acc[e];
    __syncthreads();
    if (t < CPR) {
        const float inv = 1.f / total;
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        for (int gg = 0; gg < ng; ++gg)
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] += red[(gg * CPR + t) * EPC + e];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] *= inv;
        *(uint4*)((T*)a.out + (long)b * a.ldo + t * EPC) = VecIO<T>::pack(acc);
    }
}

template <typename T>
__global__ void __launch_bounds__(kT) pool_attn_bwd_kernel(const PoolArgs a) {
    constexpr int EPC = VecIO<T>::EPC;
    extern __shared__ float smem[];
    float* qs = smem;             // [C]
    float* gs = qs + a.C;         // [C]: dout
    float* ps = gs + a.C;         // [Lk]: probabilities
    float* dss = ps + a.Lk;       // [Lk]: d(scores)
    float* red = dss + a.Lk;      // [kT][EPC]
    float* wr = red + kT * EPC;   // [8]
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, CPR = a.C / EPC;
    const T* q = (const T*)a.q + (long)b * a.ldq;
    const T* k = (const T*)a.k + (long)b * a.Lk * a.ldk;
    const T* v = (const T*)a.v + (long)b * a.Lk * a.ldv;
    const T* o = (const T*)a.o + (long)b * a.ldo;
    const T* go = (const T*)a.dout + (long)b * a.lddo;
    float d = 0.f;
    for (int ch = t; ch < CPR; ch += kT) {
        float f[EPC], g_[EPC], ov[EPC];
        VecIO<T>::unpack(*(const uint4*)(q + ch * EPC), f);
        VecIO<T>::unpack(*(const uint4*)(go + ch * EPC), g_);
        VecIO<T>::unpack(*(const uint4*)(o + ch * EPC), ov);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            qs[ch * EPC + e] = f[e];
            gs[ch * EPC + e] = g_[e];
            d = fmaf(g_[e], ov[e], d);
        }
    }
    d = wave_sum(d);
    if (lane == 0) wr[wave] = d;
    __syncthreads();
    const float delta = ((wr[0] + wr[1]) + wr[2]) + wr[3];  // dout . o
    const float lse = a.lse_in[b];
    for (int j = wave; j < a.Lk; j += kWaves) {
        float s = 0.f, dp = 0.f;
        for (int ch = lane; ch < CPR; ch += 64) {
            float kf[EPC], vf[EPC];
            VecIO<T>::unpack(*(const uint4*)(k + (long)j * a.ldk + ch * EPC), kf);
            VecIO<T>::unpack(*(const uint4*)(v + (long)j * a.ldv + ch * EPC), vf);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                s = fmaf(kf[e], qs[ch * EPC + e], s);
                dp = fmaf(vf[e], gs[ch * EPC + e], dp);
            }
        }
        s = wave_sum(s);
        dp = wave_sum(dp);
        if (lane == 0) {
            const float p = expf(s * a.scale - lse);
            ps[j] = p;
            dss[j] = p * (dp - delta);
        }
    }
    __syncthreads();
    const int ng = kT / CPR, g = t / CPR, ch = t - g * CPR;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    if (g < ng) {
        float qv[EPC], gv[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) qv[e] = qs[ch * EPC + e] * a.scale, gv[e] = gs[ch * EPC + e];
        for (int j = g; j < a.Lk; j += ng) {
            float kf[EPC], ov[EPC];
            VecIO<T>::unpack(*(const uint4*)(k + (long)j * a.ldk + ch * EPC), kf);
            const float dsj = dss[j], pj = ps[j];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaf(dsj, kf[e], acc[e]);
            if (a.dk) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) ov[e] = dsj * qv[e];
                *(uint4*)((T*)a.dk + ((long)b * a.Lk + j) * a.lddk + ch * EPC) = VecIO<T>::pack(ov);
            }
            if (a.dv) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) ov[e] = pj * gv[e];
                *(uint4*)((T*)a.dv + ((long)b * a.Lk + j) * a.lddv + ch * EPC) = VecIO<T>::pack(ov);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) red[t * EPC + e] = acc[e];
    __syncthreads();
    if (t < CPR && a.dq) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        for (int gg = 0; gg < ng; ++gg)
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] += red[(gg * CPR + t) * EPC + e];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] *= a.scale;
        *(uint4*)((T*)a.dq + (long)b * a.lddq + t * EPC) = VecIO<T>::pack(acc);
    }
}

int pool_fill(PoolArgs& a, const char* who, int B, int Lk, int C, int dtype, bool bwd, long* lds) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
    VT_REQUIRE(B > 0 && Lk > 0 && C > 0, VT_ERR_INVALID, "%s: bad geometry", who);
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C % epc == 0, VT_ERR_UNSUPPORTED, "%s: head_dim C=%d must be a multiple of %d", who, C, epc);
    VT_REQUIRE(C / epc <= kT, VT_ERR_UNSUPPORTED, "%s: head_dim C=%d exceeds %d", who, C, kT * epc);
    *lds = ((long)(bwd ? 2 : 1) * (C + Lk) + kT * epc + 8) * 4;
    VT_REQUIRE(*lds <= kLdsMax, VT_ERR_UNSUPPORTED, "%s: Lk=%d keys of %d channels need %ld bytes of LDS, the limit is %d", who, Lk, C,
               *lds, kLdsMax);
    a.B = B, a.Lk = Lk, a.C = C;
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_dw3_gelu_pool_supported(int32_t H, int32_t W, int32_t dtype) {
    if ((dtype != VT_F32 && dtype != VT_BF16) || H <= 0 || W <= 0) return 0;
    return plane_lds_bytes(H, W, 1, dtype, true) <= kLdsMax ? 1 : 0;
}

int vt_dw3_gelu_pool_fwd(const void* u, int32_t ldu, const float* w, const float* bias, void* a, int32_t lda, void* pooled,
                         int32_t ldp, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
    VT_REQUIRE(u && w && a && pooled, VT_ERR_INVALID, "vt_dw3_gelu_pool_fwd: null argument");
    PlaneArgs p;
    memset(&p, 0, sizeof(p));
    long lds = 0;
    VT_TRY(plane_fill(p, "vt_dw3_gelu_pool_fwd", B, H, W, C, dtype, false, &lds));
    VT_REQUIRE(mat_ok(u, ldu, C, dtype) && mat_ok(a, lda, C, dtype) && ldp >= C, VT_ERR_INVALID,
               "vt_dw3_gelu_pool_fwd: bad strides / alignment");
    p.u = u, p.w = w, p.bias = bias, p.a = a, p.pooled = pooled, p.ldu = ldu, p.lda = lda, p.ldp = ldp;
    if (dtype == VT_BF16) {
        VT_TRY(vt_raise_dynamic_lds((const void*)dw3_gelu_pool_fwd_kernel<bf16_t>, (int)lds, "vt_dw3_gelu_pool_fwd"));
    } else {
        VT_TRY(vt_raise_dynamic_lds((const void*)dw3_gelu_pool_fwd_kernel<float>, (int)lds, "vt_dw3_gelu_pool_fwd"));
    }
    VT_DISPATCH_T(dtype, "vt_dw3_gelu_pool_fwd",
                  hipLaunchKernelGGL(dw3_gelu_pool_fwd_kernel<T>, dim3(B * p.nslabs), dim3(kT), lds, (hipStream_t)stream, p));
    VT_CHECK_LAUNCH("vt_dw3_gelu_pool_fwd");
    return VT_OK;
}

int64_t vt_dw3_gelu_pool_bwd_scratch_bytes(int32_t B, int32_t C) { return (int64_t)B * C * 10 * 4; }

int vt_dw3_gelu_pool_bwd(const void* u, int32_t ldu, const void* da, int32_t ldda, const void* dpooled, int32_t lddp,
                         const float* w, const float* bias, void* du, int32_t lddu, const void* residual, int32_t ldr, float* dw,
                         float* dbias, void* scratch, int64_t scratch_bytes, int32_t B, int32_t H, int32_t W, int32_t C,
                         int32_t dtype, void* stream) {
    VT_REQUIRE(u && w && scratch && (da || dpooled) && (du || dw || dbias), VT_ERR_INVALID, "vt_dw3_gelu_pool_bwd: null argument");
    PlaneArgs p;
    memset(&p, 0, sizeof(p));
    long lds = 0;
    VT_TRY(plane_fill(p, "vt_dw3_gelu_pool_bwd", B, H, W, C, dtype, true, &lds));
    VT_REQUIRE(scratch_bytes >= vt_dw3_gelu_pool_bwd_scratch_bytes(B, C) && vt_aligned16(scratch), VT_ERR_INVALID,
               "vt_dw3_gelu_pool_bwd: scratch of %lld bytes, %lld needed", (long long)scratch_bytes,
               (long long)vt_dw3_gelu_pool_bwd_scratch_bytes(B, C));
    VT_REQUIRE(mat_ok(u, ldu, C, dtype) && (!da || mat_ok(da, ldda, C, dtype)) && (!dpooled || lddp >= C) &&
                   (!du || mat_ok(du, lddu, C, dtype)) && (!residual || (du && mat_ok(residual, ldr, C, dtype))),
               VT_ERR_INVALID, "vt_dw3_gelu_pool_bwd: bad strides / alignment");
    p.u = u, p.da = da, p.dp = dpooled, p.w = w, p.bias = bias, p.du = du, p.res = residual, p.scratch = (float*)scratch;
    p.ldu = ldu, p.ldda = ldda, p.lddp = lddp, p.lddu = lddu, p.ldr = ldr;
    if (dtype == VT_BF16) {
        VT_TRY(vt_raise_dynamic_lds((const void*)dw3_gelu_pool_bwd_kernel<bf16_t>, (int)lds, "vt_dw3_gelu_pool_bwd"));
    } else {
        VT_TRY(vt_raise_dynamic_lds((const void*)dw3_gelu_pool_bwd_kernel<float>, (int)lds, "vt_dw3_gelu_pool_bwd"));
    }
    VT_DISPATCH_T(dtype, "vt_dw3_gelu_pool_bwd",
                  hipLaunchKernelGGL(dw3_gelu_pool_bwd_kernel<T>, dim3(B * p.nslabs), dim3(kT), lds, (hipStream_t)stream, p));
    VT_CHECK_LAUNCH("vt_dw3_gelu_pool_bwd");
    if (dw || dbias) {
        hipLaunchKernelGGL(dw3_share_sum_kernel, dim3((C * 10 + kT - 1) / kT), dim3(kT), 0, (hipStream_t)stream,
                           (const float*)scratch, dw, dbias, B, C);
        VT_CHECK_LAUNCH("vt_dw3_gelu_pool_bwd(shares)");
    }
    return VT_OK;
}

int vt_se_gate_fwd(const void* a, int32_t lda, const void* s, int32_t lds, void* y, int32_t ldy, int32_t B, int32_t HW, int32_t C,
                   int32_t dtype, void* stream) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "vt_se_gate_fwd: dtype %d", dtype);
    VT_REQUIRE(B > 0 && HW > 0 && C > 0, VT_ERR_INVALID, "vt_se_gate_fwd: bad geometry");
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C % epc == 0, VT_ERR_UNSUPPORTED, "vt_se_gate_fwd: C=%d must be a multiple of %d", C, epc);
    VT_REQUIRE(mat_ok(a, lda, C, dtype) && mat_ok(s, lds, C, dtype) && mat_ok(y, ldy, C, dtype), VT_ERR_INVALID,
               "vt_se_gate_fwd: bad strides / alignment");
    const long items = (long)B * HW * (C / epc);
    long blocks = (items + kT - 1) / kT;
    if (blocks > 8192) blocks = 8192;
    VT_DISPATCH_T(dtype, "vt_se_gate_fwd",
                  hipLaunchKernelGGL(se_gate_fwd_kernel<T>, dim3((unsigned)blocks), dim3(kT), 0, (hipStream_t)stream, (const T*)a, lda,
                                     (const T*)s, lds, (T*)y, ldy, items, HW, C / epc));
    VT_CHECK_LAUNCH("vt_se_gate_fwd");
    return VT_OK;
}

int vt_se_gate_bwd(const void* dy, int32_t lddy, const void* a, int32_t lda, const void* s, int32_t lds, void* da, int32_t ldda,
                   float* ds, int32_t B, int32_t HW, int32_t C, int32_t accumulate, int32_t dtype, void* stream) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "vt_se_gate_bwd: dtype %d", dtype);
    VT_REQUIRE(B > 0 && HW > 0 && C > 0 && ds, VT_ERR_INVALID, "vt_se_gate_bwd: bad geometry");
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C % epc == 0, VT_ERR_UNSUPPORTED, "vt_se_gate_bwd: C=%d must be a multiple of %d", C, epc);
    VT_REQUIRE(mat_ok(dy, lddy, C, dtype) && mat_ok(a, lda, C, dtype) && mat_ok(s, lds, C, dtype) && mat_ok(da, ldda, C, dtype),
               VT_ERR_INVALID, "vt_se_gate_bwd: bad strides / alignment");
    const int cpr = C / epc;
    int sch = 4;
    while (sch > cpr) sch >>= 1;
    const int nslabs = (cpr + sch - 1) / sch;
    VT_DISPATCH_T(dtype, "vt_se_gate_bwd",
                  hipLaunchKernelGGL(se_gate_bwd_kernel<T>, dim3(B * nslabs), dim3(kT), 0, (hipStream_t)stream, (const T*)dy, lddy,
                                     (const T*)a, lda, (const T*)s, lds, (T*)da, ldda, ds, HW, C, sch, nslabs, accumulate));
    VT_CHECK_LAUNCH("vt_se_gate_bwd");
    return VT_OK;
}

int vt_channel_stats(const void* x, int32_t ldx, int64_t M, int32_t C, int32_t dtype, float* stats, void* stream) {
    VT_REQUIRE(dtype == VT_F32 || dtype == VT_BF16, VT_ERR_UNSUPPORTED, "vt_channel_stats: dtype %d", dtype);
    VT_REQUIRE(M > 0 && C > 0 && stats, VT_ERR_INVALID, "vt_channel_stats: bad geometry");
    const int epc = vt_epc(dtype);
    VT_REQUIRE(C % epc == 0, VT_ERR_UNSUPPORTED, "vt_channel_stats: C=%d must be a multiple of %d", C, epc);
    VT_REQUIRE(mat_ok(x, ldx, C, dtype), VT_ERR_INVALID, "vt_channel_stats: bad strides / alignment");
    const int cpr = C / epc, ct = cpr < kT ? cpr : kT, rt = kT / ct;
    // about 512 workgroups at most (two per CU): each ends in one atomic per channel and sum
    long it = (M + (long)rt * 512 - 1) / ((long)rt * 512);
    const int iters = (int)(it < 1 ? 1 : (it > 65536 ? 65536 : it));
    const long per = (long)rt * iters;
    VT_REQUIRE((M + per - 1) / per < (1L << 31), VT_ERR_UNSUPPORTED, "vt_channel_stats: M=%lld rows", (long long)M);
    VT_DISPATCH_T(dtype, "vt_channel_stats",
                  hipLaunchKernelGGL(channel_stats_kernel<T>, dim3((unsigned)((M + per - 1) / per)), dim3(kT), 0, (hipStream_t)stream,
                                     (const T*)x, ldx, (long)M, C, cpr, ct, rt, iters, stats));
    VT_CHECK_LAUNCH("vt_channel_stats");
    return VT_OK;
}

int vt_pool_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                     float* lse, float scale, int32_t B, int32_t Lk, int32_t C, int32_t dtype, void* stream) {
    VT_REQUIRE(q && k && v && o && lse, VT_ERR_INVALID, "vt_pool_attn_fwd: null argument");
    PoolArgs p;
    memset(&p, 0, sizeof(p));
    long lds = 0;
    VT_TRY(pool_fill(p, "vt_pool_attn_fwd", B, Lk, C, dtype, false, &lds));
    VT_REQUIRE(mat_ok(q, ldq, C, dtype) && mat_ok(k, ldk, C, dtype) && mat_ok(v, ldv, C, dtype) && mat_ok(o, ldo, C, dtype),
               VT_ERR_INVALID, "vt_pool_attn_fwd: bad strides / alignment");
    p.q = q, p.k = k, p.v = v, p.out = o, p.lse = lse, p.scale = scale, p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    if (dtype == VT_BF16) {
        VT_TRY(vt_raise_dynamic_lds((const void*)pool_attn_fwd_kernel<bf16_t>, (int)lds, "vt_pool_attn_fwd"));
    } else {
        VT_TRY(vt_raise_dynamic_lds((const void*)pool_attn_fwd_kernel<float>, (int)lds, "vt_pool_attn_fwd"));
    }
    VT_DISPATCH_T(dtype, "vt_pool_attn_fwd",
                  hipLaunchKernelGGL(pool_attn_fwd_kernel<T>, dim3(B), dim3(kT), lds, (hipStream_t)stream, p));
    VT_CHECK_LAUNCH("vt_pool_attn_fwd");
    return VT_OK;
}

int vt_pool_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o, int32_t ldo,
                     const void* dout, int32_t lddo, const float* lse, void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv,
                     int32_t lddv, float scale, int32_t B, int32_t Lk, int32_t C, int32_t dtype, void* stream) {
    VT_REQUIRE(q && k && v && o && dout && lse && (dq || dk || dv), VT_ERR_INVALID, "vt_pool_attn_bwd: null argument");
    PoolArgs p;
    memset(&p, 0, sizeof(p));
    long lds = 0;
    VT_TRY(pool_fill(p, "vt_pool_attn_bwd", B, Lk, C, dtype, true, &lds));
    VT_REQUIRE(mat_ok(q, ldq, C, dtype) && mat_ok(k, ldk, C, dtype) && mat_ok(v, ldv, C, dtype) && mat_ok(o, ldo, C, dtype) &&
                   mat_ok(dout, lddo, C, dtype) && (!dq || mat_ok(dq, lddq, C, dtype)) && (!dk || mat_ok(dk, lddk, C, dtype)) &&
                   (!dv || mat_ok(dv, lddv, C, dtype)),
               VT_ERR_INVALID, "vt_pool_attn_bwd: bad strides / alignment");
    p.q = q, p.k = k, p.v = v, p.o = o, p.dout = dout, p.lse_in = lse, p.dq = dq, p.dk = dk, p.dv = dv, p.scale = scale;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddo = lddo, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
    if (dtype == VT_BF16) {
        VT_TRY(vt_raise_dynamic_lds((const void*)pool_attn_bwd_kernel<bf16_t>, (int)lds, "vt_pool_attn_bwd"));
    } else {
        VT_TRY(vt_raise_dynamic_lds((const void*)pool_attn_bwd_kernel<float>, (int)lds, "vt_pool_attn_bwd"));
    }
    VT_DISPATCH_T(dtype, "vt_pool_attn_bwd",
                  hipLaunchKernelGGL(pool_attn_bwd_kernel<T>, dim3(B), dim3(kT), lds, (hipStream_t)stream, p));
    VT_CHECK_LAUNCH("vt_pool_attn_bwd");
    return VT_OK;
}

}  // extern "C"
