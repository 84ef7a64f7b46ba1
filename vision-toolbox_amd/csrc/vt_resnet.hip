// vt_resnet.hip -- what a torchvision ResNet needs beyond the Darknet / VoVNet kernels.
//
// 1. BatchNorm passes whose residual joins BEFORE the activation.  A DarknetBlock is x + relu(bn(conv)) and every pass of
//    vt_elementwise.hip implements that: the ReLU mask is z*scale + shift > 0 and the shortcut's gradient is dy.  A ResNet
//    block ends in relu(bn(conv) + identity): the mask depends on the sum, and the identity's gradient is the MASKED dy.
//      forward          y  = relu(z*scale + shift + r)                         (r may alias y)
//      backward reduce  g  = dy * [y > 0];  sums[0][c] += sum g,  sums[1][c] += sum g * xhat
//      backward apply   dz = coef0*g - coef1*z + coef2;  dr = g  or  dr += g   (one pass, two outputs)
//    The mask is read from the STORED y in its own dtype -- what torch's in-place ReLU does; it is exact against the
//    forward's decision, which a recomputed z*scale + shift + r (r rounded, the sum rounded again) would not be.
//    Forward and backward apply exist with the finalize step inside the launch (vt_bn_fin.h: every workgroup finalizes the
//    channels of its own channel group from the complete sums, row block 0 stores them) and with ready coefficients
//    (eval mode, a frozen bn.eval(), SyncBatchNorm).  Streaming kernels on the RowMap of vt_rowmap.h: 16 bytes per lane,
//    kUnroll rows in flight, plain vector stores; the reduce pass adds its row lanes with rowlane_fold (same header); the
//    only atomics are the integer ones of the statistics buffer.
//    Each pass also exists with a per-image keep factor (kKeep; the vt_bn_add_act_keep_* entry points): stochastic depth as
//    timm's ResNet places it, y = relu(keep[b] * (z*scale + shift) + r); the identity still receives g, the BatchNorm side
//    keep[b] * g.
// 2. The stem Conv2d(3, 64, 7, 2, 3): 49 taps against VT_MAX_TAPS = 36.  Padded to 8x8 with a zero first row and column it
//    is a 4x4 stride-1 filter over the space-to-depth image (12 channels (py, px, c)), taps at offsets -2 .. +1, which the
//    convolution descriptor expresses and the existing forward and filter-gradient kernels run.  Here: the image gather,
//    the filter repack [Cout][7][7][3] -> [Cout][4][4][Cs] and its transpose for the filter gradient.
#include "vt_bn_fin.h"
#include "vt_common.h"
#include "vt_rowmap.h"

namespace {

// ---------------------------------------------------------------------------------
// y = relu(z*scale + shift + r); kFin: grid (row blocks, channel groups of Cg channels), coefficients finalized in the launch
// (r and y are not __restrict__: they may be the same tensor -- every element is read and written by one thread)
// ---------------------------------------------------------------------------------
// kKeep: stochastic depth, y = relu(keep[b] * (z*scale + shift) + r) with one factor per image, b = row / HW (a workgroup's
// band of rows may cross images); where keep[b] == 0 the row of z is not read and y = relu(r).  The plain passes are the
// kKeep = false instances, where the operands and the branch compile out.
template <typename T, bool kFin, bool kKeep = false>
__global__ void __launch_bounds__(kThreads)
bn_add_act_kernel(const VtFinFwd f, const float* __restrict__ scale, const float* __restrict__ shift, const T* __restrict__ z,
                  int ldz, const T* r, int ldr, T* y, int ldy, long M, RowMap rm, int Cg,
                  const float* __restrict__ keep = nullptr, int HW = 1) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float s_sc[kFinCg], s_sf[kFinCg];
    const int t = threadIdx.x;
    const int cg0 = blockIdx.y * Cg;
    if constexpr (kFin) {
        vt_fin_fwd_to_lds(f, cg0, Cg, s_sc, s_sf);
    }
    z += cg0, y += cg0, r += cg0;
    const int rl = t / rm.CT;
    if (rl >= rm.RT) return;
    const long row0 = rm.row0(rl);
    for (int col = t % rm.CT; col < rm.CPR; col += rm.CT) {
        float sc[EPC], sf[EPC];
        chunk_coef(sc, kFin ? s_sc : scale, col);
        chunk_coef(sf, kFin ? s_sf : shift, col);
        const T* pz = z + row0 * ldz + col * EPC;
        const T* pr = r + row0 * ldr + col * EPC;
        T* py = y + row0 * ldy + col * EPC;
        const long sz = (long)rm.RT * ldz, sr = (long)rm.RT * ldr, sy = (long)rm.RT * ldy;
        uint4 vz[kUnroll], vr[kUnroll];
        float kf[kUnroll];
        rowmap_trips(
            rm, row0, M,
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                vz[u] = vr[u] = make_uint4(0, 0, 0, 0);
                kf[u] = 0.f;
                if (ok) {
                    if constexpr (kKeep) {
                        kf[u] = keep[(unsigned)(row0 + (long)i * rm.RT) / (unsigned)HW];  // (M < 2^31 rows: check_keep)
                        if (kf[u] != 0.f) vz[u] = ld16(pz + i * sz);
                    } else {
                        vz[u] = ld16(pz + i * sz);
                    }
                    vr[u] = ld16(pr + i * sr);
                }
            },
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                float v[EPC], rr[EPC];
                VecIO<T>::unpack(vz[u], v);
                VecIO<T>::unpack(vr[u], rr);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    if constexpr (kKeep)  // (keep = 1: fmaf(1, a, r) is a + r, the plain pass's bits)
                        v[e] = kf[u] != 0.f ? fmaxf(fmaf(kf[u], fmaf(v[e], sc[e], sf[e]), rr[e]), 0.f) : fmaxf(rr[e], 0.f);
                    else
                        v[e] = fmaxf(fmaf(v[e], sc[e], sf[e]) + rr[e], 0.f);
                }
                if (ok) st16(py + i * sy, VecIO<T>::pack(v));
            });
    }
}

// ---------------------------------------------------------------------------------
// backward, pass 1: per-channel sum(g) and sum(g*xhat), g = dy * [y > 0]; the row lanes meet in rowlane_fold (vt_rowmap.h)
// ---------------------------------------------------------------------------------
// kKeep: the BatchNorm side sees u = keep[b] * g; a dropped image's rows are not read at all
template <typename T, bool kKeep = false>
__global__ void __launch_bounds__(kThreads)
bn_add_act_bwd_reduce_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ y, int ldy, const T* __restrict__ z, int ldz,
                             const float* __restrict__ mean, const float* __restrict__ invstd, long M, int C, RowMap rm,
                             float* __restrict__ sums, int Ctot, const float* __restrict__ keep = nullptr, int HW = 1) {
    constexpr int EPC = VecIO<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) float sred[];  // rowlane_fold_bytes(2, CT, RT, EPC)
    const int t = threadIdx.x;
    const int r = t / rm.CT;
    const int tc = t % rm.CT;
    const long row0 = rm.row0(r);
    const int rep = blockIdx.x % kStatReplicas;
    const int cg0 = blockIdx.y * rm.CPR;  // first 16-byte chunk of this channel group (C channels each of Ctot)
    dy += (long)cg0 * EPC, y += (long)cg0 * EPC, z += (long)cg0 * EPC;
    mean += cg0 * EPC, invstd += cg0 * EPC;
    for (int cbase = 0; cbase < rm.CPR; cbase += rm.CT) {
        const int col = cbase + tc;
        const bool active = (r < rm.RT) && (col < rm.CPR);
        float s[2][EPC];
        float(&s1)[EPC] = s[0], (&s2)[EPC] = s[1];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = 0.f;
        if (active) {
            float mu[EPC];
            chunk_coef(mu, mean, col);
            const T* pg = dy + row0 * lddy + col * EPC;
            const T* py = y + row0 * ldy + col * EPC;
            const T* pz = z + row0 * ldz + col * EPC;
            const long sg = (long)rm.RT * lddy, sy = (long)rm.RT * ldy, sz = (long)rm.RT * ldz;
            uint4 vg[kUnroll], vy[kUnroll], vz[kUnroll];
            float kf[kUnroll];
            rowmap_trips(
                rm, row0, M,
                [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                    vg[u] = vy[u] = vz[u] = make_uint4(0, 0, 0, 0);  // y = 0 masks the row out
                    kf[u] = 0.f;
                    if (ok) {
                        if constexpr (kKeep) {
                            kf[u] = keep[(unsigned)(row0 + (long)i * rm.RT) / (unsigned)HW];
                            if (kf[u] == 0.f) return;  // (y stays 0: the row contributes nothing)
                        }
                        vg[u] = ld16(pg + i * sg);
                        vy[u] = ld16(py + i * sy);
                        vz[u] = ld16(pz + i * sz);
                    }
                },
                [&](int u, int, bool) VT_TRIP_LAMBDA {
                    float g[EPC], yy[EPC], zz[EPC];
                    VecIO<T>::unpack(vg[u], g);
                    VecIO<T>::unpack(vy[u], yy);
                    VecIO<T>::unpack(vz[u], zz);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        float gg = yy[e] > 0.f ? g[e] : 0.f;
                        if constexpr (kKeep) gg *= kf[u];
                        s1[e] += gg;
                        s2[e] = fmaf(gg, zz[e] - mu[e], s2[e]);  // invstd applied once, below
                    }
                });
        }
        rowlane_fold(sred, s, rm.CT, rm.RT, [&](int which, int lc, float acc) {
            bn_sums_emit(sums, rep, Ctot, cg0 * EPC, invstd, C, which, cbase * EPC + lc, acc);
        });
    }
}

// ---------------------------------------------------------------------------------
// backward, pass 2: dz = a*g - b*z + d and dr (=|+=) g, g = dy * [y > 0]; kFin: grid (row blocks, channel groups), the
// backward finalize step inside the launch.  (dr is not __restrict__: with `acc` it is read and written by one thread.)
// ---------------------------------------------------------------------------------
// kKeep: dz = a*u - b*z + d with u = keep[b] * g, while the identity receives g itself.  A dropped image's z IS read: under
// batch statistics its dz is -b*z + d (its rows moved the mean and the variance of the others).
template <typename T, bool kFin, bool kKeep = false>
__global__ void __launch_bounds__(kThreads)
bn_add_act_bwd_apply_kernel(const VtFinBwd f, const float* __restrict__ coef, const T* __restrict__ dy, int lddy,
                            const T* __restrict__ y, int ldy, const T* __restrict__ z, int ldz, T* __restrict__ dz, int lddz, T* dr,
                            int lddr, int acc, long M, int C, RowMap rm, int Cg, const float* __restrict__ keep = nullptr,
                            int HW = 1) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float s_a[kFinCg], s_b[kFinCg], s_d[kFinCg];
    const int t = threadIdx.x;
    const int cg0 = blockIdx.y * Cg;
    if constexpr (kFin) {
        vt_fin_bwd_to_lds(f, cg0, Cg, s_a, s_b, s_d);
    }
    dy += cg0, y += cg0, z += cg0, dz += cg0, dr += cg0;
    const int r = t / rm.CT;
    if (r >= rm.RT) return;
    const long row0 = rm.row0(r);
    for (int col = t % rm.CT; col < rm.CPR; col += rm.CT) {
        float ca[EPC], cb[EPC], cd[EPC];
        chunk_coef(ca, kFin ? s_a : coef, col);
        chunk_coef(cb, kFin ? s_b : coef + C, col);
        chunk_coef(cd, kFin ? s_d : coef + 2 * C, col);
        uint4 vg[kUnroll], vy[kUnroll], vz[kUnroll], va[kUnroll];
        rowmap_trips(
            rm, row0, M,
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                const long row = row0 + (long)i * rm.RT;
                vg[u] = vy[u] = vz[u] = va[u] = make_uint4(0, 0, 0, 0);
                if (ok) {
                    vg[u] = ld16(dy + row * lddy + col * EPC);
                    vy[u] = ld16(y + row * ldy + col * EPC);
                    vz[u] = ld16(z + row * ldz + col * EPC);
                    if (acc) va[u] = ld16(dr + row * lddr + col * EPC);
                }
            },
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                if (!ok) return;
                const long row = row0 + (long)i * rm.RT;
                float g[EPC], yy[EPC], zz[EPC], aa[EPC], o[EPC];
                VecIO<T>::unpack(vg[u], g);
                VecIO<T>::unpack(vy[u], yy);
                VecIO<T>::unpack(vz[u], zz);
                VecIO<T>::unpack(va[u], aa);
                float kf = 1.f;
                if constexpr (kKeep) kf = keep[(unsigned)row / (unsigned)HW];
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float gg = yy[e] > 0.f ? g[e] : 0.f;
                    if constexpr (kKeep) o[e] = fmaf(ca[e], kf * gg, fmaf(-cb[e], zz[e], cd[e]));
                    else o[e] = fmaf(ca[e], gg, fmaf(-cb[e], zz[e], cd[e]));
                    aa[e] += gg;  // (acc = 0: aa was zero)
                }
                st16(dz + row * lddz + col * EPC, VecIO<T>::pack(o));
                st16(dr + row * lddr + col * EPC, VecIO<T>::pack(aa));
            });
    }
}

// ---------------------------------------------------------------------------------
// The 7x7 stride-2 stem as a 4x4 stride-1 convolution over the space-to-depth image
// ---------------------------------------------------------------------------------
// channel j < 12 of the space-to-depth image is (py, px, c) = (j / 6, j / 3 % 2, j % 3); Cs >= 12 channels, the rest zero
constexpr int kS2dReal = 12;

// out[b][hs][ws][(py, px, c)] = x[b][2 hs + py][2 ws + px][c] (zero outside the image: odd H or W); a thread per output
// pixel: four 16-byte pixel loads (3 real channels in the first chunk), Cs / EPC 16-byte stores
template <typename T>
__global__ void __launch_bounds__(kThreads)
stem7_s2d_kernel(const T* __restrict__ x, int ldx, T* __restrict__ out, int ldo, int B, int H, int W, int Hs, int Ws) {
    constexpr int EPC = VecIO<T>::EPC;
    constexpr int CS = (kS2dReal + EPC - 1) / EPC * EPC;
    const long n = (long)B * Hs * Ws;
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ws = (int)(i % Ws);
    const long t2 = i / Ws;
    const int hs = (int)(t2 % Hs);
    const long b = t2 / Hs;
    float v[CS];
#pragma unroll
    for (int j = 0; j < CS; ++j) v[j] = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int h = 2 * hs + (p >> 1), w = 2 * ws + (p & 1);
        if (h < H && w < W) {
            float px[EPC];
            VecIO<T>::unpack(ld16(x + ((b * H + h) * W + w) * ldx), px);
            v[3 * p] = px[0], v[3 * p + 1] = px[1], v[3 * p + 2] = px[2];
        }
    }
#pragma unroll
    for (int q = 0; q < CS / EPC; ++q) st16(out + i * ldo + q * EPC, VecIO<T>::pack(v + q * EPC));
}

// out[n][a][b][j] = w[n][2a + py - 1][2b + px - 1][c] (zero where an index is -1: the padded first row / column, and for
// j >= 12); w is the channels_last filter image [Cout][7][7][3]
template <typename S, typename D>
__global__ void __launch_bounds__(kThreads)
stem7_pack_filter_kernel(const S* __restrict__ w, D* __restrict__ out, int Cout, int Cs) {
    const int n = Cout * 16 * Cs;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int j = i % Cs, tap = (i / Cs) % 16, o = i / (16 * Cs);
    float v = 0.f;
    if (j < kS2dReal) {
        const int kh = 2 * (tap >> 2) + j / 6 - 1, kw = 2 * (tap & 3) + (j / 3) % 2 - 1;
        if (kh >= 0 && kw >= 0) v = (float)w[((o * 7 + kh) * 7 + kw) * 3 + j % 3];
    }
    out[i] = from_float<D>(v);
}

// the transpose: dw[n][kh][kw][c] += dws[n][a][b][j], every tap of the 7x7 filter has exactly one source
__global__ void __launch_bounds__(kThreads)
stem7_unpack_wgrad_kernel(const float* __restrict__ dws, int Cs, float* __restrict__ dw, int Cout) {
    const int n = Cout * 49 * 3;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int c = i % 3, kw = (i / 3) % 7, kh = (i / 21) % 7, o = i / 147;
    const int a = (kh + 1) >> 1, py = (kh + 1) & 1, b = (kw + 1) >> 1, px = (kw + 1) & 1;
    dw[i] += dws[(o * 16 + a * 4 + b) * Cs + py * 6 + px * 3 + c];
}

// ---------------------------------------------------------------------------------
// the five add-then-ReLU passes, plain (keep == nullptr: the kKeep = false instances) or with per-image keep factors
// ---------------------------------------------------------------------------------
#define ADD_ACT_MAT(what, p, ld)                            \
    do {                                                    \
        char nm__[96];                                      \
        snprintf(nm__, sizeof nm__, "%s(%s)", who, what);   \
        VT_TRY(check_mat(nm__, p, ld, C, dtype));           \
    } while (0)

int add_act_apply(const char* who, const void* z, int ldz, const float* scale, const float* shift, const void* r, int ldr, void* y,
                  int ldy, const float* keep, int HW, long M, int C, int dtype, void* stream) {
    VT_REQUIRE(M > 0 && scale && shift, VT_ERR_INVALID, "%s: bad argument", who);
    ADD_ACT_MAT("z", z, ldz);
    ADD_ACT_MAT("r", r, ldr);
    ADD_ACT_MAT("y", y, ldy);
    const RowMap rm = RowMap::make(C, vt_epc(dtype), M);
    const VtFinFwd f{};
    if (keep)
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_kernel<T, false, true>), dim3(rm.blocks(M)), dim3(kThreads), 0,
                                         (hipStream_t)stream, f, scale, shift, (const T*)z, ldz, (const T*)r, ldr, (T*)y, ldy, M, rm,
                                         C, keep, HW));
    else
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_kernel<T, false>), dim3(rm.blocks(M)), dim3(kThreads), 0, (hipStream_t)stream, f,
                                         scale, shift, (const T*)z, ldz, (const T*)r, ldr, (T*)y, ldy, M, rm, C));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int add_act_finalize_apply(const char* who, const float* stats, int C, double count, const float* gamma, const float* beta,
                           float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           float* scale, float* shift, float* mean, float* invstd, const void* z, int ldz, const void* r, int ldr,
                           void* y, int ldy, const float* keep, int HW, long M, int dtype, void* stream) {
    VT_REQUIRE(stats && scale && shift && mean && invstd && C > 0 && count > 0 && M > 0, VT_ERR_INVALID, "%s: bad argument", who);
    VT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), VT_ERR_INVALID,
               "%s: running_mean/var must both be given or both NULL", who);
    ADD_ACT_MAT("z", z, ldz);
    ADD_ACT_MAT("r", r, ldr);
    ADD_ACT_MAT("y", y, ldy);
    const int Cg = fin_group(C, vt_epc(dtype));
    if (!fin_in_launch(Cg)) {
        VT_TRY(vt_bn_finalize(stats, C, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, scale,
                              shift, mean, invstd, stream));
        return add_act_apply(who, z, ldz, scale, shift, r, ldr, y, ldy, keep, HW, M, C, dtype, stream);
    }
    const int groups = C / Cg;
    const RowMap rm = fin_rowmap(Cg, groups, vt_epc(dtype), M);
    const VtFinFwd f = make_fin_fwd(stats, C, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, scale,
                                    shift, mean, invstd);
    if (keep)
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_kernel<T, true, true>), dim3(rm.blocks(M), groups), dim3(kThreads), 0,
                                         (hipStream_t)stream, f, (const float*)nullptr, (const float*)nullptr, (const T*)z, ldz,
                                         (const T*)r, ldr, (T*)y, ldy, M, rm, Cg, keep, HW));
    else
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_kernel<T, true>), dim3(rm.blocks(M), groups), dim3(kThreads), 0,
                                         (hipStream_t)stream, f, (const float*)nullptr, (const float*)nullptr, (const T*)z, ldz,
                                         (const T*)r, ldr, (T*)y, ldy, M, rm, Cg));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int add_act_bwd_reduce(const char* who, const void* dy, int lddy, const void* y, int ldy, const void* z, int ldz, const float* mean,
                       const float* invstd, const float* keep, int HW, long M, int C, int dtype, float* sums, void* stream) {
    VT_REQUIRE(M > 0 && mean && invstd && sums, VT_ERR_INVALID, "%s: bad argument", who);
    ADD_ACT_MAT("dy", dy, lddy);
    ADD_ACT_MAT("y", y, ldy);
    ADD_ACT_MAT("z", z, ldz);
    const BnReducePlan p = bn_reduce_plan(M, C, vt_epc(dtype));
    if (keep)
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_bwd_reduce_kernel<T, true>), dim3(p.rm.blocks(M), p.cgroups), dim3(kThreads), p.smem,
                                         (hipStream_t)stream, (const T*)dy, lddy, (const T*)y, ldy, (const T*)z, ldz, mean, invstd, M,
                                         p.Cg, p.rm, sums, C, keep, HW));
    else
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL(bn_add_act_bwd_reduce_kernel<T>, dim3(p.rm.blocks(M), p.cgroups), dim3(kThreads), p.smem,
                                         (hipStream_t)stream, (const T*)dy, lddy, (const T*)y, ldy, (const T*)z, ldz, mean, invstd, M,
                                         p.Cg, p.rm, sums, C));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int add_act_bwd_apply(const char* who, const void* dy, int lddy, const void* y, int ldy, const void* z, int ldz, const float* coef,
                      void* dz, int lddz, void* dr, int lddr, int accumulate, const float* keep, int HW, long M, int C, int dtype,
                      void* stream) {
    VT_REQUIRE(M > 0 && coef, VT_ERR_INVALID, "%s: bad argument", who);
    ADD_ACT_MAT("dy", dy, lddy);
    ADD_ACT_MAT("y", y, ldy);
    ADD_ACT_MAT("z", z, ldz);
    ADD_ACT_MAT("dz", dz, lddz);
    ADD_ACT_MAT("dr", dr, lddr);
    VT_REQUIRE(dz != dr, VT_ERR_INVALID, "%s: dz and dr are two outputs", who);
    const RowMap rm = RowMap::make(C, vt_epc(dtype), M);
    const VtFinBwd f{};
    if (keep)
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_bwd_apply_kernel<T, false, true>), dim3(rm.blocks(M)), dim3(kThreads), 0,
                                         (hipStream_t)stream, f, coef, (const T*)dy, lddy, (const T*)y, ldy, (const T*)z, ldz, (T*)dz,
                                         lddz, (T*)dr, lddr, accumulate ? 1 : 0, M, C, rm, C, keep, HW));
    else
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_bwd_apply_kernel<T, false>), dim3(rm.blocks(M)), dim3(kThreads), 0,
                                         (hipStream_t)stream, f, coef, (const T*)dy, lddy, (const T*)y, ldy, (const T*)z, ldz, (T*)dz,
                                         lddz, (T*)dr, lddr, accumulate ? 1 : 0, M, C, rm, C));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}

int add_act_bwd_finalize_apply(const char* who, const float* sums, int C, double count, double pscale, const float* scale,
                               const float* mean, const float* invstd, int train, float* dgamma, float* dbeta, float* coef,
                               const void* dy, int lddy, const void* y, int ldy, const void* z, int ldz, void* dz, int lddz, void* dr,
                               int lddr, int accumulate, const float* keep, int HW, long M, int dtype, void* stream) {
    VT_REQUIRE(sums && scale && mean && invstd && coef && C > 0 && count > 0 && M > 0, VT_ERR_INVALID, "%s: bad argument", who);
    ADD_ACT_MAT("dy", dy, lddy);
    ADD_ACT_MAT("y", y, ldy);
    ADD_ACT_MAT("z", z, ldz);
    ADD_ACT_MAT("dz", dz, lddz);
    ADD_ACT_MAT("dr", dr, lddr);
    VT_REQUIRE(dz != dr, VT_ERR_INVALID, "%s: dz and dr are two outputs", who);
    const int Cg = fin_group(C, vt_epc(dtype));
    if (!fin_in_launch(Cg)) {
        VT_TRY(vt_bn_bwd_finalize(sums, C, count, pscale, scale, mean, invstd, train, dgamma, dbeta, coef, stream));
        return add_act_bwd_apply(who, dy, lddy, y, ldy, z, ldz, coef, dz, lddz, dr, lddr, accumulate, keep, HW, M, C, dtype, stream);
    }
    const int groups = C / Cg;
    const RowMap rm = fin_rowmap(Cg, groups, vt_epc(dtype), M);
    const VtFinBwd f = make_fin_bwd(sums, C, count, pscale, scale, mean, invstd, train, dgamma, dbeta, coef);
    if (keep)
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_bwd_apply_kernel<T, true, true>), dim3(rm.blocks(M), groups), dim3(kThreads), 0,
                                         (hipStream_t)stream, f, (const float*)nullptr, (const T*)dy, lddy, (const T*)y, ldy,
                                         (const T*)z, ldz, (T*)dz, lddz, (T*)dr, lddr, accumulate ? 1 : 0, M, C, rm, Cg, keep, HW));
    else
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL((bn_add_act_bwd_apply_kernel<T, true>), dim3(rm.blocks(M), groups), dim3(kThreads), 0,
                                         (hipStream_t)stream, f, (const float*)nullptr, (const T*)dy, lddy, (const T*)y, ldy,
                                         (const T*)z, ldz, (T*)dz, lddz, (T*)dr, lddr, accumulate ? 1 : 0, M, C, rm, Cg));
    VT_CHECK_LAUNCH(who);
    return VT_OK;
}
#undef ADD_ACT_MAT

}  // namespace

extern "C" {

int vt_bn_add_act_apply(const void* z, int32_t ldz, const float* scale, const float* shift, const void* r, int32_t ldr, void* y,
                        int32_t ldy, int64_t M, int32_t C, int32_t dtype, void* stream) {
    return add_act_apply("vt_bn_add_act_apply", z, ldz, scale, shift, r, ldr, y, ldy, nullptr, 1, (long)M, C, dtype, stream);
}

int vt_bn_add_act_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                                 float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                 float* scale, float* shift, float* mean, float* invstd, const void* z, int32_t ldz, const void* r,
                                 int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t dtype, void* stream) {
    return add_act_finalize_apply("vt_bn_add_act_finalize_apply", stats, C, count, gamma, beta, eps, momentum, running_mean,
                                  running_var, num_batches_tracked, scale, shift, mean, invstd, z, ldz, r, ldr, y, ldy, nullptr, 1,
                                  (long)M, dtype, stream);
}

int vt_bn_add_act_bwd_reduce(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                             const float* mean, const float* invstd, int64_t M, int32_t C, int32_t dtype, float* sums,
                             void* stream) {
    return add_act_bwd_reduce("vt_bn_add_act_bwd_reduce", dy, lddy, y, ldy, z, ldz, mean, invstd, nullptr, 1, (long)M, C, dtype, sums,
                              stream);
}

int vt_bn_add_act_bwd_apply(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                            const float* coef, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate, int64_t M,
                            int32_t C, int32_t dtype, void* stream) {
    return add_act_bwd_apply("vt_bn_add_act_bwd_apply", dy, lddy, y, ldy, z, ldz, coef, dz, lddz, dr, lddr, accumulate, nullptr, 1,
                             (long)M, C, dtype, stream);
}

int vt_bn_add_act_bwd_finalize_apply(const float* sums, int32_t C, double count, double pscale, const float* scale,
                                     const float* mean, const float* invstd, int32_t train, float* dgamma, float* dbeta,
                                     float* coef, const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z,
                                     int32_t ldz, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate, int64_t M,
                                     int32_t dtype, void* stream) {
    return add_act_bwd_finalize_apply("vt_bn_add_act_bwd_finalize_apply", sums, C, count, pscale, scale, mean, invstd, train, dgamma,
                                      dbeta, coef, dy, lddy, y, ldy, z, ldz, dz, lddz, dr, lddr, accumulate, nullptr, 1, (long)M,
                                      dtype, stream);
}

// ---- the same passes with per-image keep factors (stochastic depth of a ResNet block) ----
int vt_bn_add_act_keep_apply(const void* z, int32_t ldz, const float* scale, const float* shift, const void* r, int32_t ldr, void* y,
                             int32_t ldy, const float* keep, int32_t HW, int64_t M, int32_t C, int32_t dtype, void* stream) {
    VT_TRY(check_keep("vt_bn_add_act_keep_apply", keep, HW, (long)M));
    return add_act_apply("vt_bn_add_act_keep_apply", z, ldz, scale, shift, r, ldr, y, ldy, keep, HW, (long)M, C, dtype, stream);
}

int vt_bn_add_act_keep_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                                      float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                      float* scale, float* shift, float* mean, float* invstd, const void* z, int32_t ldz,
                                      const void* r, int32_t ldr, void* y, int32_t ldy, const float* keep, int32_t HW, int64_t M,
                                      int32_t dtype, void* stream) {
    VT_TRY(check_keep("vt_bn_add_act_keep_finalize_apply", keep, HW, (long)M));
    return add_act_finalize_apply("vt_bn_add_act_keep_finalize_apply", stats, C, count, gamma, beta, eps, momentum, running_mean,
                                  running_var, num_batches_tracked, scale, shift, mean, invstd, z, ldz, r, ldr, y, ldy, keep, HW,
                                  (long)M, dtype, stream);
}

int vt_bn_add_act_keep_bwd_reduce(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                                  const float* mean, const float* invstd, const float* keep, int32_t HW, int64_t M, int32_t C,
                                  int32_t dtype, float* sums, void* stream) {
    VT_TRY(check_keep("vt_bn_add_act_keep_bwd_reduce", keep, HW, (long)M));
    return add_act_bwd_reduce("vt_bn_add_act_keep_bwd_reduce", dy, lddy, y, ldy, z, ldz, mean, invstd, keep, HW, (long)M, C, dtype,
                              sums, stream);
}

int vt_bn_add_act_keep_bwd_apply(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                                 const float* coef, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate,
                                 const float* keep, int32_t HW, int64_t M, int32_t C, int32_t dtype, void* stream) {
    VT_TRY(check_keep("vt_bn_add_act_keep_bwd_apply", keep, HW, (long)M));
    return add_act_bwd_apply("vt_bn_add_act_keep_bwd_apply", dy, lddy, y, ldy, z, ldz, coef, dz, lddz, dr, lddr, accumulate, keep, HW,
                             (long)M, C, dtype, stream);
}

int vt_bn_add_act_keep_bwd_finalize_apply(const float* sums, int32_t C, double count, double pscale, const float* scale,
                                          const float* mean, const float* invstd, int32_t train, float* dgamma, float* dbeta,
                                          float* coef, const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z,
                                          int32_t ldz, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate,
                                          const float* keep, int32_t HW, int64_t M, int32_t dtype, void* stream) {
    VT_TRY(check_keep("vt_bn_add_act_keep_bwd_finalize_apply", keep, HW, (long)M));
    return add_act_bwd_finalize_apply("vt_bn_add_act_keep_bwd_finalize_apply", sums, C, count, pscale, scale, mean, invstd, train,
                                      dgamma, dbeta, coef, dy, lddy, y, ldy, z, ldz, dz, lddz, dr, lddr, accumulate, keep, HW,
                                      (long)M, dtype, stream);
}

int32_t vt_stem7_s2d_channels(int32_t dtype) { return dtype == VT_BF16 ? 16 : 12; }

int vt_stem7_s2d(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t B, int32_t H, int32_t W, int32_t dtype,
                 void* stream) {
    VT_REQUIRE(dtype == VT_BF16 || dtype == VT_F32, VT_ERR_UNSUPPORTED, "vt_stem7_s2d: unsupported dtype %d", dtype);
    const int epc = vt_epc(dtype), Cs = vt_stem7_s2d_channels(dtype);
    VT_REQUIRE(x && out && vt_aligned16(x) && vt_aligned16(out), VT_ERR_INVALID, "vt_stem7_s2d: null or misaligned pointer");
    VT_REQUIRE(B > 0 && H > 0 && W > 0, VT_ERR_INVALID, "vt_stem7_s2d: non-positive extent");
    VT_REQUIRE(ldx >= epc && ldx % epc == 0 && ldo >= Cs && ldo % epc == 0, VT_ERR_INVALID,
               "vt_stem7_s2d: ldx=%d ldo=%d: the image has one 16-byte chunk of channels, the output %d", ldx, ldo, Cs);
    const int Hs = (H + 1) / 2, Ws = (W + 1) / 2;
    const long n = (long)B * Hs * Ws;
    VT_REQUIRE((long)B * H * W * ldx < 0x7fffffffL && n * ldo < 0x7fffffffL, VT_ERR_UNSUPPORTED,
               "vt_stem7_s2d: tensor exceeds 2^31 elements");  // (the bound of vt_conv_igemm, which reads the output)
    VT_DISPATCH_T(dtype, "vt_stem7_s2d",
                  hipLaunchKernelGGL(stem7_s2d_kernel<T>, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                                     (hipStream_t)stream, (const T*)x, ldx, (T*)out, ldo, B, H, W, Hs, Ws));
    VT_CHECK_LAUNCH("vt_stem7_s2d");
    return VT_OK;
}

int vt_stem7_pack_filter(const void* w, int32_t src_dtype, void* out, int32_t dst_dtype, int32_t Cout, void* stream) {
    VT_REQUIRE(w && out && Cout > 0 && Cout <= 65536, VT_ERR_INVALID, "vt_stem7_pack_filter: bad argument");
    VT_REQUIRE((src_dtype == VT_F32 || src_dtype == VT_BF16) && (dst_dtype == VT_F32 || dst_dtype == VT_BF16) &&
                   (src_dtype == dst_dtype || src_dtype == VT_F32),
               VT_ERR_UNSUPPORTED, "vt_stem7_pack_filter: dtypes %d -> %d", src_dtype, dst_dtype);
    const int Cs = vt_stem7_s2d_channels(dst_dtype);
    const dim3 grid((unsigned)((Cout * 16 * Cs + kThreads - 1) / kThreads));
    hipStream_t st = (hipStream_t)stream;
    if (src_dtype == VT_BF16)
        hipLaunchKernelGGL((stem7_pack_filter_kernel<bf16_t, bf16_t>), grid, dim3(kThreads), 0, st, (const bf16_t*)w, (bf16_t*)out, Cout, Cs);
    else if (dst_dtype == VT_BF16)
        hipLaunchKernelGGL((stem7_pack_filter_kernel<float, bf16_t>), grid, dim3(kThreads), 0, st, (const float*)w, (bf16_t*)out, Cout, Cs);
    else
        hipLaunchKernelGGL((stem7_pack_filter_kernel<float, float>), grid, dim3(kThreads), 0, st, (const float*)w, (float*)out, Cout, Cs);
    VT_CHECK_LAUNCH("vt_stem7_pack_filter");
    return VT_OK;
}

int vt_stem7_unpack_wgrad(const float* dws, int32_t Cs, float* dw, int32_t Cout, void* stream) {
    VT_REQUIRE(dws && dw && Cout > 0 && Cout <= 65536 && Cs >= kS2dReal, VT_ERR_INVALID, "vt_stem7_unpack_wgrad: bad argument");
    hipLaunchKernelGGL(stem7_unpack_wgrad_kernel, dim3((unsigned)((Cout * 147 + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, dws, Cs, dw, Cout);
    VT_CHECK_LAUNCH("vt_stem7_unpack_wgrad");
    return VT_OK;
}

}  // extern "C"
