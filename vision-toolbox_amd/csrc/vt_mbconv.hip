// vt_mbconv.hip -- what a torchvision EfficientNet block needs beyond the MobileNet kernels.
//
// 1. BatchNorm passes with a per-image keep factor (stochastic depth, "row" mode).  A residual MBConv / FusedMBConv block is
//    x + keep[b] * f(x) in training mode; f ends in a Conv -> BatchNorm [-> act] unit, so the factor rides on that unit's
//    normalise pass and on its BatchNorm backward.  With b = m / HW the image of row m:
//      forward          y  = keep[b] * act(z*scale + shift) + r                 (r may alias y)
//      backward reduce  g  = keep[b] * dy * act'(z*scale + shift);  sums[0][c] += sum g,  sums[1][c] += sum g * xhat
//      backward apply   dz = coef0*g - coef1*z + coef2
//    `keep` is a device float[B] of ANY values (0 and 1 / (1 - p) in training).  Where keep[b] == 0 the forward copies r and
//    never reads z, the backward reduce reads neither dy nor z; the backward apply still reads z (under batch statistics dz of
//    a dropped image is -coef1*z + coef2, not zero) and skips dy.  The residual's gradient is dy itself (the caller's).
//    The two backward passes also take a per-(image, channel) ADDEND: g = (keep[b] * dy + add[b][c] / HW) * act'(.), keep NULL
//    meaning 1 -- the gradient of a per-image average pool of y (the Squeeze-Excitation pool of pass 2 below) joins d(y) in f32
//    inside the BatchNorm backward, instead of being added to an already rounded d(y) by a pass of its own.
//    Forward and backward apply exist with the finalize step inside the launch (vt_bn_fin.h) and with ready coefficients,
//    as in vt_resnet.hip; every activation code of vt_act.h is taken.  Streaming kernels on the RowMap: 16 bytes per lane,
//    kUnroll rows in flight, plain vector stores; the reduce pass and the pool of pass 2 add their row lanes with
//    rowlane_fold (vt_rowmap.h); the only atomics are the integer ones of the statistics buffer.
// 2. Normalise + activation + per-image average pool in one pass: y = act(z*scale + shift) and pooled[b][c] = the mean over
//    the image's pixels of y AS STORED (rounded to the compute dtype) -- the operand of the Squeeze-Excitation MLP, which
//    otherwise costs one more read of the expanded map (vt_global_avgpool_fwd).  A workgroup owns one (image, row slab,
//    channel group): with one slab per image it writes the pooled row itself; with several the slabs' sums meet in a zeroed
//    fixed-point scratch (integer atomics: order-free) that a B x C finishing launch turns into the row.
#include "vt_act.h"
#include "vt_bn_fin.h"
#include "vt_common.h"
#include "vt_rowmap.h"

namespace {

// ---------------------------------------------------------------------------------
// y = keep[b] * act(z*scale + shift) + r; kFin: grid (row blocks, channel groups of Cg channels), coefficients finalized in
// the launch (r and y are not __restrict__: they may be the same tensor -- every element is read and written by one thread)
// ---------------------------------------------------------------------------------
template <typename T, bool kFin>
__global__ void __launch_bounds__(kThreads)
bn_keep_apply_kernel(const VtFinFwd f, const float* __restrict__ scale, const float* __restrict__ shift, const T* __restrict__ z,
                     int ldz, const T* r, int ldr, T* y, int ldy, const float* __restrict__ keep, unsigned HW, long M, RowMap rm,
                     int Cg, int act) {
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
        float kp[kUnroll];
        rowmap_trips(
            rm, row0, M,
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                vz[u] = vr[u] = make_uint4(0, 0, 0, 0);
                kp[u] = 0.f;
                if (ok) {
                    kp[u] = keep[(unsigned)(row0 + (long)i * rm.RT) / HW];
                    vr[u] = ld16(pr + i * sr);
                    if (kp[u] != 0.f) vz[u] = ld16(pz + i * sz);  // (a dropped image's z is never read)
                }
            },
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                if (!ok) return;
                if (kp[u] == 0.f) {  // y = r, bit for bit
                    st16(py + i * sy, vr[u]);
                    return;
                }
                float v[EPC], rr[EPC];
                VecIO<T>::unpack(vz[u], v);
                VecIO<T>::unpack(vr[u], rr);
#pragma unroll
                for (int e = 0; e < EPC; ++e) v[e] = fmaf(kp[u], act_fwd(act, fmaf(v[e], sc[e], sf[e])), rr[e]);
                st16(py + i * sy, VecIO<T>::pack(v));
            });
    }
}

// ---------------------------------------------------------------------------------
// backward, pass 1: per-channel sum(g) and sum(g*xhat), g = keep[b] * dy * act'(z*scale + shift); the row lanes meet in
// rowlane_fold (vt_rowmap.h); grid (row blocks, channel groups of C channels each of Ctot)
// ---------------------------------------------------------------------------------
// (kAdd: the addend form is an instantiation of its own, so that the passes of a residual block keep their registers)
template <typename T, bool kAdd>
__global__ void __launch_bounds__(kThreads)
bn_keep_bwd_reduce_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ z, int ldz, const float* __restrict__ scale,
                          const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ invstd,
                          const float* __restrict__ keep, const T* __restrict__ add, int lda, unsigned HW, long M, int C, RowMap rm,
                          int act, float* __restrict__ sums, int Ctot) {
    constexpr int EPC = VecIO<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) float sred[];  // rowlane_fold_bytes(2, CT, RT, EPC)
    const int t = threadIdx.x;
    const int r = t / rm.CT;
    const int tc = t % rm.CT;
    const long row0 = rm.row0(r);
    const int rep = blockIdx.x % kStatReplicas;
    const int cg0 = blockIdx.y * rm.CPR;  // first 16-byte chunk of this channel group
    dy += (long)cg0 * EPC, z += (long)cg0 * EPC;
    if constexpr (kAdd) add += (long)cg0 * EPC;
    const float ascale = 1.f / (float)HW;
    scale += cg0 * EPC, shift += cg0 * EPC, mean += cg0 * EPC, invstd += cg0 * EPC;
    for (int cbase = 0; cbase < rm.CPR; cbase += rm.CT) {
        const int col = cbase + tc;
        const bool active = (r < rm.RT) && (col < rm.CPR);
        float s[2][EPC];
        float(&s1)[EPC] = s[0], (&s2)[EPC] = s[1];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = 0.f;
        if (active) {
            float sc[EPC], sf[EPC], mu[EPC];
            chunk_coef(sc, scale, col);
            chunk_coef(sf, shift, col);
            chunk_coef(mu, mean, col);
            const T* pg = dy + row0 * lddy + col * EPC;
            const T* pz = z + row0 * ldz + col * EPC;
            const long sg = (long)rm.RT * lddy, sz = (long)rm.RT * ldz;
            uint4 vg[kUnroll], vz[kUnroll], va[kUnroll];
            float kp[kUnroll];
            bool on[kUnroll];
            rowmap_trips(
                rm, row0, M,
                [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                    vg[u] = vz[u] = va[u] = make_uint4(0, 0, 0, 0);
                    kp[u] = 0.f;
                    on[u] = false;
                    if (ok) {
                        const unsigned b = (unsigned)(row0 + (long)i * rm.RT) / HW;
                        kp[u] = keep ? keep[b] : 1.f;
                        if constexpr (kAdd) va[u] = ld16(add + (long)b * lda + col * EPC);
                        on[u] = kAdd || kp[u] != 0.f;
                        if (kp[u] != 0.f) vg[u] = ld16(pg + i * sg);
                        if (on[u]) vz[u] = ld16(pz + i * sz);  // (a dropped image without an addend: neither is read)
                    }
                },
                [&](int u, int, bool) VT_TRIP_LAMBDA {
                    if (!on[u]) return;
                    float g[EPC], zz[EPC], aa[EPC];
                    VecIO<T>::unpack(vg[u], g);
                    VecIO<T>::unpack(vz[u], zz);
                    VecIO<T>::unpack(va[u], aa);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        float d = kp[u] * g[e];
                        if constexpr (kAdd) d = kp[u] != 0.f ? fmaf(kp[u], g[e], aa[e] * ascale) : aa[e] * ascale;
                        const float gg = d * act_grad(act, fmaf(zz[e], sc[e], sf[e]));
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
// backward, pass 2: dz = a*g - b*z + d, g = keep[b] * dy * act'(z*a + shift) (a = scale is the first coefficient); kFin: grid
// (row blocks, channel groups), the backward finalize step inside the launch
// ---------------------------------------------------------------------------------
template <typename T, bool kFin, bool kAdd>
__global__ void __launch_bounds__(kThreads)
bn_keep_bwd_apply_kernel(const VtFinBwd f, const float* __restrict__ coef, const float* __restrict__ shift,
                         const T* __restrict__ dy, int lddy, const T* __restrict__ z, int ldz, const float* __restrict__ keep,
                         const T* __restrict__ add, int lda, unsigned HW, T* __restrict__ dz, int lddz, long M, int C, RowMap rm,
                         int Cg, int act) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float s_a[kFinCg], s_b[kFinCg], s_d[kFinCg];
    const int t = threadIdx.x;
    const int cg0 = blockIdx.y * Cg;
    if constexpr (kFin) {
        vt_fin_bwd_to_lds(f, cg0, Cg, s_a, s_b, s_d);
    }
    dy += cg0, z += cg0, dz += cg0, shift += cg0;
    if constexpr (kAdd) add += cg0;
    const float ascale = 1.f / (float)HW;
    const int r = t / rm.CT;
    if (r >= rm.RT) return;
    const long row0 = rm.row0(r);
    for (int col = t % rm.CT; col < rm.CPR; col += rm.CT) {
        float ca[EPC], cb[EPC], cd[EPC], sf[EPC];
        chunk_coef(ca, kFin ? s_a : coef, col);
        chunk_coef(cb, kFin ? s_b : coef + C, col);
        chunk_coef(cd, kFin ? s_d : coef + 2 * C, col);
        chunk_coef(sf, shift, col);
        uint4 vg[kUnroll], vz[kUnroll], va[kUnroll];
        float kp[kUnroll];
        rowmap_trips(
            rm, row0, M,
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                const long row = row0 + (long)i * rm.RT;
                vg[u] = vz[u] = va[u] = make_uint4(0, 0, 0, 0);
                kp[u] = 0.f;
                if (ok) {
                    const unsigned b = (unsigned)row / HW;
                    kp[u] = keep ? keep[b] : 1.f;
                    if constexpr (kAdd) va[u] = ld16(add + (long)b * lda + col * EPC);
                    vz[u] = ld16(z + row * ldz + col * EPC);
                    if (kp[u] != 0.f) vg[u] = ld16(dy + row * lddy + col * EPC);
                }
            },
            [&](int u, int i, bool ok) VT_TRIP_LAMBDA {
                if (!ok) return;
                const long row = row0 + (long)i * rm.RT;
                float g[EPC], zz[EPC], aa[EPC], o[EPC];
                VecIO<T>::unpack(vg[u], g);
                VecIO<T>::unpack(vz[u], zz);
                VecIO<T>::unpack(va[u], aa);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    float gg;
                    if constexpr (kAdd) {
                        const float d = kp[u] != 0.f ? fmaf(kp[u], g[e], aa[e] * ascale) : aa[e] * ascale;
                        gg = d * act_grad(act, fmaf(zz[e], ca[e], sf[e]));
                    } else {
                        gg = kp[u] != 0.f ? kp[u] * g[e] * act_grad(act, fmaf(zz[e], ca[e], sf[e])) : 0.f;
                    }
                    o[e] = fmaf(ca[e], gg, fmaf(-cb[e], zz[e], cd[e]));
                }
                st16(dz + row * lddz + col * EPC, VecIO<T>::pack(o));
            });
    }
}

// ---------------------------------------------------------------------------------
// y = act(z*scale + shift) and the per-image mean of the stored y.  Grid (B * S, channel groups of Cg channels): workgroup
// (b, slab) walks rows [slab * rps, (slab + 1) * rps) of image b.  S == 1: the owner writes pooled[b][c]; S > 1: the slab's
// sums are added to the fixed-point scratch int64[B][C][2] (vt_stat_add) and pool_finish_kernel forms the row.
// ---------------------------------------------------------------------------------
struct PoolPlan {
    int Cg, groups, CPR, CT, RT, S, rps;
};

template <typename T, bool kFin>
__global__ void __launch_bounds__(kThreads)
bn_act_avgpool_kernel(const VtFinFwd f, const float* __restrict__ scale, const float* __restrict__ shift, const T* __restrict__ z,
                      int ldz, T* __restrict__ y, int ldy, T* __restrict__ pooled, int ldp, float* __restrict__ scratch, int HW,
                      int Ctot, PoolPlan pp, int act) {
    constexpr int EPC = VecIO<T>::EPC;
    __shared__ float s_sc[kFinCg], s_sf[kFinCg];
    // the one-sum rowlane_fold: rowlane_fold_bytes(1, CT, RT, EPC) <= kThreads * EPC floats, since rows * CT <= kThreads
    __shared__ __attribute__((aligned(16))) float sred[kThreads * EPC];
    const int t = threadIdx.x;
    const int cg0 = blockIdx.y * pp.Cg;
    if constexpr (kFin) {
        vt_fin_fwd_to_lds(f, cg0, pp.Cg, s_sc, s_sf);
    } else {
        scale += cg0, shift += cg0;
    }
    const int b = blockIdx.x / pp.S, slab = blockIdx.x % pp.S;
    const int lo = slab * pp.rps, hi = min(HW, lo + pp.rps);
    z += (long)b * HW * ldz + cg0, y += (long)b * HW * ldy + cg0;
    const int r = t / pp.CT, tc = t % pp.CT;
    const float inv = 1.f / (float)HW;
    for (int cbase = 0; cbase < pp.CPR; cbase += pp.CT) {
        const int col = cbase + tc;
        const bool active = (r < pp.RT) && (col < pp.CPR);
        float ps[1][EPC];
        float(&s)[EPC] = ps[0];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s[e] = 0.f;
        if (active) {
            float sc[EPC], sf[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                if constexpr (kFin) sc[e] = s_sc[col * EPC + e], sf[e] = s_sf[col * EPC + e];
                else sc[e] = scale[col * EPC + e], sf[e] = shift[col * EPC + e];
            }
            for (int hw = lo + r; hw < hi; hw += kUnroll * pp.RT) {
                uint4 vz[kUnroll];
                bool ok[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    ok[u] = hw + u * pp.RT < hi;
                    vz[u] = make_uint4(0, 0, 0, 0);
                    if (ok[u]) vz[u] = ld16(z + (long)(hw + u * pp.RT) * ldz + col * EPC);
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    if (!ok[u]) continue;
                    float v[EPC];
                    VecIO<T>::unpack(vz[u], v);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) v[e] = act_fwd(act, fmaf(v[e], sc[e], sf[e]));
                    st16(y + (long)(hw + u * pp.RT) * ldy + col * EPC, VecIO<T>::pack(v));
#pragma unroll
                    for (int e = 0; e < EPC; ++e) s[e] += VecIO<T>::round(v[e]);  // the mean of y as stored
                }
            }
        }
        rowlane_fold(sred, ps, pp.CT, pp.RT, [&](int, int lc, float acc) {
            const int c = cbase * EPC + lc;  // (within the channel group)
            if (c >= pp.Cg) return;
            if (pp.S == 1) pooled[(long)b * ldp + cg0 + c] = from_float<T>(acc * inv);
            else vt_stat_add(scratch, (long)b * Ctot + cg0 + c, acc);
        });
    }
}

// pooled[b][c] = scratch[b][c] / HW (S > 1)
template <typename T>
__global__ void __launch_bounds__(kThreads)
pool_finish_kernel(const float* __restrict__ scratch, T* __restrict__ pooled, int ldp, int B, int C, float inv) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long)B * C) return;
    const long long* q = (const long long*)scratch;
    const double v = vt_stat_decode(q[2 * i], q[2 * i + 1]);
    pooled[(i / C) * ldp + i % C] = from_float<T>((float)v * inv);
}

// backward: keep may be NULL (factor 1) where the addend row [M / HW][C] is given
inline int check_keep_add(const char* who, const float* keep, const void* add, int lda, int HW, long M, int C, int dtype) {
    VT_REQUIRE(keep || add, VT_ERR_INVALID, "%s: a keep row float[M / HW] or an addend [M / HW][C] (or both)", who);
    VT_TRY(check_image_rows(who, HW, M));
    if (add) VT_TRY(check_mat(who, add, lda, C, dtype));
    return VT_OK;
}

// the cut of the pool pass: channel groups of Cg channels (the finalize group where C has one; else the whole row), and as
// many row slabs per image as bring the grid to ~1024 workgroups while every row lane keeps >= 8 rows
inline PoolPlan pool_plan(int B, int HW, int C, int epc) {
    PoolPlan p;
    p.Cg = fin_group(C, epc);
    if (!p.Cg) p.Cg = C;
    p.groups = C / p.Cg;
    p.CPR = p.Cg / epc;
    p.CT = p.CPR < kThreads ? p.CPR : kThreads;
    p.RT = kThreads / p.CT;
    const long owners = (long)B * p.groups;
    long S = owners >= 1024 ? 1 : (1024 + owners - 1) / owners;
    const long smax = HW / (p.RT * 8L);
    if (S > smax) S = smax;
    if (S < 1) S = 1;
    p.rps = (int)((HW + S - 1) / S);
    p.S = (HW + p.rps - 1) / p.rps;
    return p;
}

template <bool kFin>
int launch_pool(const char* who, const VtFinFwd& f, const float* scale, const float* shift, const void* z, int ldz, void* y, int ldy,
                void* pooled, int ldp, void* scratch, int B, int HW, int C, int act, int dtype, hipStream_t st) {
    const PoolPlan pp = pool_plan(B, HW, C, vt_epc(dtype));
    VT_REQUIRE(pp.S == 1 || (scratch && vt_aligned16(scratch)), VT_ERR_INVALID,
               "%s: %d row slabs per image need the zeroed scratch of vt_bn_act_avgpool_scratch_bytes", who, pp.S);
    const dim3 grid((unsigned)B * pp.S, pp.groups);
    VT_DISPATCH_T(dtype, who,
                  hipLaunchKernelGGL((bn_act_avgpool_kernel<T, kFin>), grid, dim3(kThreads), 0, st, f, scale, shift, (const T*)z, ldz,
                                     (T*)y, ldy, (T*)pooled, ldp, (float*)scratch, HW, C, pp, act));
    VT_CHECK_LAUNCH(who);
    if (pp.S > 1) {
        const long n = (long)B * C;
        VT_DISPATCH_T(dtype, who,
                      hipLaunchKernelGGL(pool_finish_kernel<T>, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                                         (const float*)scratch, (T*)pooled, ldp, B, C, 1.f / (float)HW));
        VT_CHECK_LAUNCH(who);
    }
    return VT_OK;
}

inline int check_pool(const char* who, const void* z, int ldz, const void* y, int ldy, const void* pooled, int ldp, int B, int HW,
                      int C, int act, int dtype) {
    VT_REQUIRE(B > 0 && HW > 0 && (long)B * HW <= 0x7fffffffL && act >= 0 && act <= 6, VT_ERR_INVALID, "%s: bad argument", who);
    VT_TRY(check_mat(who, z, ldz, C, dtype));
    VT_TRY(check_mat(who, y, ldy, C, dtype));
    VT_TRY(check_mat(who, pooled, ldp, C, dtype));
    return VT_OK;
}

}  // namespace

extern "C" {

int vt_bn_keep_apply(const void* z, int32_t ldz, const float* scale, const float* shift, const void* r, int32_t ldr, void* y,
                     int32_t ldy, const float* keep, int32_t HW, int64_t M, int32_t C, int32_t act, int32_t dtype, void* stream) {
    VT_REQUIRE(scale && shift && act >= 0 && act <= 6, VT_ERR_INVALID, "vt_bn_keep_apply: bad argument");
    VT_TRY(check_keep("vt_bn_keep_apply", keep, HW, (long)M));
    VT_TRY(check_mat("vt_bn_keep_apply(z)", z, ldz, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_apply(r)", r, ldr, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_apply(y)", y, ldy, C, dtype));
    const RowMap rm = RowMap::make(C, vt_epc(dtype), M);
    const VtFinFwd f{};
    VT_DISPATCH_T(dtype, "vt_bn_keep_apply",
                  hipLaunchKernelGGL((bn_keep_apply_kernel<T, false>), dim3(rm.blocks(M)), dim3(kThreads), 0, (hipStream_t)stream, f,
                                     scale, shift, (const T*)z, ldz, (const T*)r, ldr, (T*)y, ldy, keep, (unsigned)HW, (long)M, rm, C,
                                     act));
    VT_CHECK_LAUNCH("vt_bn_keep_apply");
    return VT_OK;
}

int vt_bn_keep_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* scale,
                              float* shift, float* mean, float* invstd, const void* z, int32_t ldz, const void* r, int32_t ldr,
                              void* y, int32_t ldy, const float* keep, int32_t HW, int64_t M, int32_t act, int32_t dtype,
                              void* stream) {
    VT_REQUIRE(stats && scale && shift && mean && invstd && C > 0 && count > 0 && act >= 0 && act <= 6, VT_ERR_INVALID,
               "vt_bn_keep_finalize_apply: bad argument");
    VT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), VT_ERR_INVALID,
               "vt_bn_keep_finalize_apply: running_mean/var must both be given or both NULL");
    VT_TRY(check_keep("vt_bn_keep_finalize_apply", keep, HW, (long)M));
    VT_TRY(check_mat("vt_bn_keep_finalize_apply(z)", z, ldz, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_finalize_apply(r)", r, ldr, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_finalize_apply(y)", y, ldy, C, dtype));
    const int Cg = fin_group(C, vt_epc(dtype));
    if (!fin_in_launch(Cg)) {
        VT_TRY(vt_bn_finalize(stats, C, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, scale,
                              shift, mean, invstd, stream));
        return vt_bn_keep_apply(z, ldz, scale, shift, r, ldr, y, ldy, keep, HW, M, C, act, dtype, stream);
    }
    const int groups = C / Cg;
    const RowMap rm = fin_rowmap(Cg, groups, vt_epc(dtype), M);
    const VtFinFwd f = make_fin_fwd(stats, C, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, scale,
                                    shift, mean, invstd);
    VT_DISPATCH_T(dtype, "vt_bn_keep_finalize_apply",
                  hipLaunchKernelGGL((bn_keep_apply_kernel<T, true>), dim3(rm.blocks(M), groups), dim3(kThreads), 0,
                                     (hipStream_t)stream, f, (const float*)nullptr, (const float*)nullptr, (const T*)z, ldz,
                                     (const T*)r, ldr, (T*)y, ldy, keep, (unsigned)HW, (long)M, rm, Cg, act));
    VT_CHECK_LAUNCH("vt_bn_keep_finalize_apply");
    return VT_OK;
}

int vt_bn_keep_bwd_reduce(const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* keep, const void* add, int32_t lda, int32_t HW,
                          int64_t M, int32_t C, int32_t act, int32_t dtype, float* sums, void* stream) {
    VT_REQUIRE(scale && shift && mean && invstd && sums && act >= 0 && act <= 6, VT_ERR_INVALID,
               "vt_bn_keep_bwd_reduce: bad argument");
    VT_TRY(check_keep_add("vt_bn_keep_bwd_reduce", keep, add, lda, HW, (long)M, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_reduce(dy)", dy, lddy, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_reduce(z)", z, ldz, C, dtype));
    const BnReducePlan p = bn_reduce_plan(M, C, vt_epc(dtype));
#define VT_KEEP_RED(ADD)                                                                                                          \
    VT_DISPATCH_T(dtype, "vt_bn_keep_bwd_reduce",                                                                                  \
                  hipLaunchKernelGGL((bn_keep_bwd_reduce_kernel<T, ADD>), dim3(p.rm.blocks(M), p.cgroups), dim3(kThreads), p.smem,  \
                                     (hipStream_t)stream, (const T*)dy, lddy, (const T*)z, ldz, scale, shift, mean, invstd, keep,  \
                                     (const T*)add, lda, (unsigned)HW, (long)M, p.Cg, p.rm, act, sums, C))
    if (add) VT_KEEP_RED(true);
    else VT_KEEP_RED(false);
#undef VT_KEEP_RED
    VT_CHECK_LAUNCH("vt_bn_keep_bwd_reduce");
    return VT_OK;
}

int vt_bn_keep_bwd_apply(const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* shift, const float* coef,
                         const float* keep, const void* add, int32_t lda, int32_t HW, void* dz, int32_t lddz, int64_t M, int32_t C,
                         int32_t act, int32_t dtype, void* stream) {
    VT_REQUIRE(shift && coef && act >= 0 && act <= 6, VT_ERR_INVALID, "vt_bn_keep_bwd_apply: bad argument");
    VT_TRY(check_keep_add("vt_bn_keep_bwd_apply", keep, add, lda, HW, (long)M, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_apply(dy)", dy, lddy, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_apply(z)", z, ldz, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_apply(dz)", dz, lddz, C, dtype));
    const RowMap rm = RowMap::make(C, vt_epc(dtype), M);
    const VtFinBwd f{};
#define VT_KEEP_APPLY(ADD)                                                                                                        \
    VT_DISPATCH_T(dtype, "vt_bn_keep_bwd_apply",                                                                                  \
                  hipLaunchKernelGGL((bn_keep_bwd_apply_kernel<T, false, ADD>), dim3(rm.blocks(M)), dim3(kThreads), 0,              \
                                     (hipStream_t)stream, f, coef, shift, (const T*)dy, lddy, (const T*)z, ldz, keep, (const T*)add, \
                                     lda, (unsigned)HW, (T*)dz, lddz, (long)M, C, rm, C, act))
    if (add) VT_KEEP_APPLY(true);
    else VT_KEEP_APPLY(false);
#undef VT_KEEP_APPLY
    VT_CHECK_LAUNCH("vt_bn_keep_bwd_apply");
    return VT_OK;
}

int vt_bn_keep_bwd_finalize_apply(const float* sums, int32_t C, double count, double pscale, const float* scale, const float* shift,
                                  const float* mean, const float* invstd, int32_t train, float* dgamma, float* dbeta, float* coef,
                                  const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* keep, const void* add,
                                  int32_t lda, int32_t HW, void* dz, int32_t lddz, int64_t M, int32_t act, int32_t dtype,
                                  void* stream) {
    VT_REQUIRE(sums && scale && shift && mean && invstd && coef && C > 0 && count > 0 && act >= 0 && act <= 6, VT_ERR_INVALID,
               "vt_bn_keep_bwd_finalize_apply: bad argument");
    VT_TRY(check_keep_add("vt_bn_keep_bwd_finalize_apply", keep, add, lda, HW, (long)M, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_finalize_apply(dy)", dy, lddy, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_finalize_apply(z)", z, ldz, C, dtype));
    VT_TRY(check_mat("vt_bn_keep_bwd_finalize_apply(dz)", dz, lddz, C, dtype));
    const int Cg = fin_group(C, vt_epc(dtype));
    if (!fin_in_launch(Cg)) {
        VT_TRY(vt_bn_bwd_finalize(sums, C, count, pscale, scale, mean, invstd, train, dgamma, dbeta, coef, stream));
        return vt_bn_keep_bwd_apply(dy, lddy, z, ldz, shift, coef, keep, add, lda, HW, dz, lddz, M, C, act, dtype, stream);
    }
    const int groups = C / Cg;
    const RowMap rm = fin_rowmap(Cg, groups, vt_epc(dtype), M);
    const VtFinBwd f = make_fin_bwd(sums, C, count, pscale, scale, mean, invstd, train, dgamma, dbeta, coef);
#define VT_KEEP_FIN_APPLY(ADD)                                                                                                        \
    VT_DISPATCH_T(dtype, "vt_bn_keep_bwd_finalize_apply",                                                                             \
                  hipLaunchKernelGGL((bn_keep_bwd_apply_kernel<T, true, ADD>), dim3(rm.blocks(M), groups), dim3(kThreads), 0,           \
                                     (hipStream_t)stream, f, (const float*)nullptr, shift, (const T*)dy, lddy, (const T*)z, ldz, keep, \
                                     (const T*)add, lda, (unsigned)HW, (T*)dz, lddz, (long)M, C, rm, Cg, act))
    if (add) VT_KEEP_FIN_APPLY(true);
    else VT_KEEP_FIN_APPLY(false);
#undef VT_KEEP_FIN_APPLY
    VT_CHECK_LAUNCH("vt_bn_keep_bwd_finalize_apply");
    return VT_OK;
}

int64_t vt_bn_act_avgpool_scratch_bytes(int32_t B, int32_t HW, int32_t C, int32_t dtype) {
    if (B <= 0 || HW <= 0 || C <= 0 || (dtype != VT_F32 && dtype != VT_BF16) || C % vt_epc(dtype)) return -1;
    return pool_plan(B, HW, C, vt_epc(dtype)).S > 1 ? (int64_t)B * C * 16 : 0;
}

int vt_bn_act_avgpool_apply(const void* z, int32_t ldz, const float* scale, const float* shift, void* y, int32_t ldy, void* pooled,
                            int32_t ldp, void* scratch, int32_t B, int32_t HW, int32_t C, int32_t act, int32_t dtype,
                            void* stream) {
    VT_REQUIRE(scale && shift, VT_ERR_INVALID, "vt_bn_act_avgpool_apply: bad argument");
    VT_TRY(check_pool("vt_bn_act_avgpool_apply", z, ldz, y, ldy, pooled, ldp, B, HW, C, act, dtype));
    const VtFinFwd f{};
    return launch_pool<false>("vt_bn_act_avgpool_apply", f, scale, shift, z, ldz, y, ldy, pooled, ldp, scratch, B, HW, C, act, dtype,
                              (hipStream_t)stream);
}

int vt_bn_act_avgpool_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                                     float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                     float* scale, float* shift, float* mean, float* invstd, const void* z, int32_t ldz, void* y,
                                     int32_t ldy, void* pooled, int32_t ldp, void* scratch, int32_t B, int32_t HW, int32_t act,
                                     int32_t dtype, void* stream) {
    VT_REQUIRE(stats && scale && shift && mean && invstd && C > 0 && count > 0, VT_ERR_INVALID,
               "vt_bn_act_avgpool_finalize_apply: bad argument");
    VT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), VT_ERR_INVALID,
               "vt_bn_act_avgpool_finalize_apply: running_mean/var must both be given or both NULL");
    VT_TRY(check_pool("vt_bn_act_avgpool_finalize_apply", z, ldz, y, ldy, pooled, ldp, B, HW, C, act, dtype));
    if (!fin_in_launch(fin_group(C, vt_epc(dtype)))) {
        VT_TRY(vt_bn_finalize(stats, C, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, scale,
                              shift, mean, invstd, stream));
        return vt_bn_act_avgpool_apply(z, ldz, scale, shift, y, ldy, pooled, ldp, scratch, B, HW, C, act, dtype, stream);
    }
    const VtFinFwd f = make_fin_fwd(stats, C, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, scale,
                                    shift, mean, invstd);
    return launch_pool<true>("vt_bn_act_avgpool_finalize_apply", f, nullptr, nullptr, z, ldz, y, ldy, pooled, ldp, scratch, B, HW, C,
                             act, dtype, (hipStream_t)stream);
}

}  // extern "C"
