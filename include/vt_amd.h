/*
 * vt_amd.h -- C-ABI of libvt_amd.so: the MI355X (gfx950) hot path of the
 * Darknet / CSPDarknet / VoVNet backbones.
 *
 * The reference (gau-nernst/vision-toolbox) has NO native layer: every entry
 * point below replaces a torch.nn / ATen call made from the reference's Python.
 * The call site it replaces is cited per function as `file:line` relative to
 * the reference checkout.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching
 *     allocator in our host code); the library allocates nothing persistent.
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it,
 *     no entry point synchronises.
 *   - activations are NHWC ("channels_last"): element (b,h,w,c) of a tensor
 *     with pixel stride `ld` lives at ((b*H + h)*W + w)*ld + c.  `ld >= C`
 *     lets a tensor be a channel slice of a wider concat buffer.
 *   - dtype: VT_F32 (exact-f32 MFMA, parity mode) or VT_BF16 (bf16 storage,
 *     f32 accumulate).  Channel counts / strides / offsets must be multiples
 *     of 16 bytes' worth of elements (4 for f32, 8 for bf16).
 *   - conv weights are [Cout][taps][Cin] ("KRSC"), i.e. the memory image of a
 *     torch OIHW weight held in channels_last format.
 *   - return value: VT_OK or a VT_ERR_* code; vt_last_error() gives the text.
 *     Nothing aborts.  Stateless and re-entrant apart from that thread-local
 *     error string.
 */
#ifndef VT_AMD_H
#define VT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VT_OK 0
#define VT_ERR_INVALID 1     /* bad argument: null pointer, misalignment, size  */
#define VT_ERR_UNSUPPORTED 2 /* shape / dtype this library has no kernel for    */
#define VT_ERR_HIP 3         /* HIP runtime reported an error                   */

#define VT_F32 0
#define VT_BF16 1
#define VT_I64 2 /* collectives only (vt_allreduce_bucket): the fixed-point BatchNorm sums */

#define VT_MAX_TAPS 36 /* 6x6 stem of DarknetYOLOv5 (darknet.py:109) */

/* epilogue flags of vt_conv_igemm */
#define VT_CONV_RELU 1     /* y = max(y, 0) after scale/shift                   */
#define VT_CONV_STATS 2    /* accumulate per-channel sum / sum-of-squares       */
#define VT_CONV_RESIDUAL 4 /* y += residual (after relu)                        */
#define VT_CONV_AFFINE 8   /* y = y*scale[c] + shift[c]; scale==NULL means 1    */
#define VT_CONV_NOSTORE 32 /* with VT_CONV_STATS: only the statistics -- of the f32 accumulator, not of a rounded copy --,
                            * y is not written (y may be NULL); RGB stem only */
#define VT_CONV_D2S 16     /* depth-to-space 2x2: the Cout = 4*C' columns of grid pixel (i, j) are the output pixels
                            * (2i+a, 2j+b) x C' channels, column = (2a+b)*C' + c; needs oHs = oWs = 2, oh0 = ow0 = 0,
                            * oH = 2*Ho, oW = 2*Wo, no STATS / AFFINE / RELU.  One launch then forms the whole data
                            * gradient of a 3x3 stride-2 convolution (the four parity classes as column blocks of a
                            * 2x2-tap filter image, zero where a class has no tap) and reads dz once. */

#define VT_STAT_REPLICAS 16
/* A statistics buffer (`stats` of vt_conv_igemm, `sums` of the BatchNorm-backward reductions) is
 * int64[VT_STAT_REPLICAS][2][C][2], VT_STAT_BYTES(C) bytes, zeroed by the caller and passed as float*: fixed point,
 * value = hi*2^12 + lo/2^33, accumulated with integer atomics.  Integer addition is associative, so the statistics --
 * and with them every activation, loss and data gradient -- are bit-identical from run to run;
 * vt_bn_finalize / vt_bn_bwd_finalize sum the replicas exactly.  SyncBatchNorm all-reduces the buffer as int64.
 *
 * The marker.  A legitimate sum has |sum| < 2^50 (1.1e15), i.e. |hi| < 2^38.  A contribution that is NaN, +-Inf or has
 * |v| >= 2^50 is not accumulated: it adds 2^40 to the hi limb instead, and EVERY decoder of the format -- vt_bn_finalize,
 * vt_bn_finalize_apply, vt_bn_bwd_finalize, vt_bn_bwd_finalize_apply and the passes that finalize for themselves,
 * vt_fixed_to_f32, vt_channel_sums_to_f32, vt_wfuse_finalize, vt_stem_bn_bwd_s2 / _combine / _combine_y -- returns NaN
 * for an entry whose hi limb, summed over the replicas, has |hi| >= 2^38 (the marker carries no sign: -Inf gives NaN too).
 * Legitimate contributions that together leave the range decode as NaN as well, never as a wrapped finite value.  The
 * replicas are summed as integers, so vt_stat_fold and the int64 all-reduce preserve the marker of any replica or rank;
 * other entries of the buffer are not affected.  A diverged activation thus shows up as NaN statistics, coefficients and
 * parameter gradients, as it would with float sums. */
#define VT_STAT_BYTES(C) ((int64_t)VT_STAT_REPLICAS * 2 * (C) * 16)

/*
 * Geometry of one implicit-GEMM convolution launch.  One descriptor covers the
 * forward conv, the data gradient (run on dz with a re-packed filter) and the
 * per-parity-class data gradient of stride-2 convs.
 *
 *   out(b, i*oHs+oh0, j*oWs+ow0, n) =
 *       sum_{t<ntaps} sum_{c<Cin} in(b, i*sh+h0+dh[t], j*sw+w0+dw[t], c) * w[n][t][c]
 *   for i<Ho, j<Wo; taps that fall outside [0,Hi)x[0,Wi) read zero.
 */
typedef struct vt_conv_desc {
    int32_t dtype;
    int32_t B, Hi, Wi, Cin, ldx; /* gather source                              */
    int32_t Ho, Wo;              /* output grid iterated (GEMM M = B*Ho*Wo)    */
    int32_t sh, sw, h0, w0;      /* input step / origin                        */
    int32_t Cout, ldy;           /* GEMM N and output pixel stride             */
    int32_t oH, oW;              /* extent of the tensor written               */
    int32_t oHs, oWs, oh0, ow0;  /* placement of grid point (i,j) in it        */
    int32_t ldw;                 /* weight row stride, elements (>= ntaps*Cin) */
    int32_t ldr;                 /* residual pixel stride                      */
    int32_t flags;               /* VT_CONV_*                                  */
    int32_t ntaps;
    int8_t dh[VT_MAX_TAPS];
    int8_t dw[VT_MAX_TAPS];
} vt_conv_desc;

/* ---- library ------------------------------------------------------------ */
int vt_version(void);
const char* vt_last_error(void);
/* name (template instantiation) of the convolution / filter-gradient kernel the calling thread's most
 * recent vt_conv_igemm / vt_conv_wgrad dispatch chose; bench.py labels its roofline entry with it. */
const char* vt_last_kernel_name(void);
/* number of kernel launches issued by this process through the library; the
 * GPU tests assert it advances, i.e. that the HIP path is what ran. */
uint64_t vt_launch_count(void);
/* Experiment / test switch of the kernel dispatchers (the names INTEGRATION.md lists, e.g. "VT_SPAN6"): each is read
 * from the environment variable of the same name ONCE per process; this call sets it afterwards (the GPU tests force a
 * kernel with it).  No switch changes results beyond summation order. */
int vt_set_knob(const char* name, int32_t value);
int vt_memset(void* ptr, int value, uint64_t bytes, void* stream);

/* ---- convolution --------------------------------------------------------
 * Replaces nn.Conv2d inside ConvNormAct (components.py:26-35) and, with the
 * AFFINE/RELU/RESIDUAL epilogue, the eval-mode BatchNorm2d + ReLU that follow
 * it (components.py:36-44) and DarknetBlock's add (darknet.py:28).  With
 * VT_CONV_STATS it also produces the batch statistics BatchNorm2d needs in
 * training mode.  The same entry point computes conv data gradients.
 * `stats` is a statistics buffer of VT_STAT_BYTES(Cout) bytes (see VT_STAT_REPLICAS), zeroed by the caller. */
int vt_conv_igemm(const vt_conv_desc* d, const void* x, const void* w, void* y,
                  const float* scale, const float* shift, const void* residual,
                  float* stats, void* stream);

/* A data gradient that also REDUCES the BatchNorm backward of the unit whose output it differentiates (round 6).
 * `d` describes a convolution run on dz with the re-packed filter (as vt_conv_igemm is called for a data gradient: flags
 * 0, every pixel of the output tensor produced: oHs = oWs = 1, oH = Ho, oW = Wo); its result dy = d(y) is the gradient of
 * the output y = act(z * scale + shift) of a ConvNormAct unit (components.py:26-44) that has no other consumer.  Besides
 * storing dy the call adds that unit's backward sums -- exactly what vt_bn_act_bwd_reduce(dy, z, ...) adds:
 *   sums[0][c] += sum g,  sums[1][c] += invstd[c] * sum g * (z - mean[c]),   g = dy (as stored) * [z * scale + shift > 0]
 * (`relu` 0: no mask) -- so that the separate reduction pass, which reads dy and z once more, disappears: where the
 * two-group persistent 3x3 kernel takes the launch the sums come out of its epilogue (dy in registers, z read like a
 * residual operand); everywhere else the call is the two launches it replaces.  `sums` is a statistics buffer
 * (VT_STAT_REPLICAS), fixed point: the result does not depend on the order in which workgroups finish.
 * Replaces the autograd backward of nn.Conv2d (components.py:26-35) with respect to its input + the reductions of
 * the autograd backward of nn.BatchNorm2d / nn.ReLU (components.py:36-44) of the unit in front of it. */
int vt_conv_dgrad_bnred(const vt_conv_desc* d, const void* dz, const void* w, void* dy, const void* z, int32_t ldz,
                        const float* scale, const float* shift, const float* mean, const float* invstd,
                        int32_t relu, float* sums, void* stream);

/* Depthwise convolution (round 6): nn.Conv2d(C, C, k, stride s, padding pad, dilation dil, groups=C, bias=False) inside a
 * ConvNormAct (components.py:26-35 with `groups = in_channels`) -- forward, data gradient, filter gradient.  x / dx are
 * [B][Hi][Wi][C], z / dz [B][Ho][Wo][C] with Ho = (Hi + 2 pad - dil (k-1) - 1) / s + 1; `w` / `dw` are the f32 [C][k*k]
 * image of the torch [C, 1, k, k] weight (bf16 launches round the filter as the convolution kernels' bf16 mirror does).
 *   vt_dwconv_fwd:   z = conv(x, w); `stats` non-NULL: also the per-channel sum / sum of squares of the STORED z (a
 *                    statistics buffer, VT_STAT_REPLICAS: the contract of vt_conv_igemm's VT_CONV_STATS)
 *   vt_dwconv_dgrad: dx = conv_transpose(dz, w) (+ residual, which may alias dx)
 *   vt_dwconv_wgrad: dw[c][t] += sum_pixels dz * x_shifted  (f32 atomics)
 * C a multiple of 8 (bf16) / 4 (f32), k <= 7.  Off the Darknet / VoVNet path; streaming kernels, no matrix pipe. */
int vt_dwconv_fwd(const void* x, int32_t ldx, const float* w, void* z, int32_t ldz, float* stats, int32_t B, int32_t Hi,
                  int32_t Wi, int32_t C, int32_t k, int32_t s, int32_t pad, int32_t dil, int32_t dtype, void* stream);
int vt_dwconv_dgrad(const void* dz, int32_t lddz, const float* w, void* dx, int32_t lddx, const void* residual, int32_t ldr,
                    int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t k, int32_t s, int32_t pad, int32_t dil,
                    int32_t dtype, void* stream);
int vt_dwconv_wgrad(const void* x, int32_t ldx, const void* dz, int32_t lddz, float* dw, int32_t B, int32_t Hi, int32_t Wi,
                    int32_t C, int32_t k, int32_t s, int32_t pad, int32_t dil, int32_t dtype, void* stream);

/* LayerNorm over the channel axis of an NHWC map and LayerScale + residual (ConvNeXt: reference backbones/convnext.py:48,
 * 53, 58, 74, 84, 101 -- nn.LayerNorm(C) on (B, H, W, C), `x + gamma * layers(x)`).  Operands are [M][C] rows with a pixel
 * stride ld >= C (channel slices work), C a multiple of 8 (bf16) / 4 (f32) and at most 6144 (bf16) / 3072 (f32); gamma / beta /
 * pre_bias are f32 masters.  Streaming kernels: a row is owned by a group of lanes of one wave, statistics in f32, two-pass
 * over the row held in registers (mean, then sum (u - mean)^2; biased variance).
 *   vt_layernorm_fwd:  y = (u - mean) rstd gamma + beta, u = x (+ pre_bias: the bias of the convolution in front, which the
 *                      depthwise kernels do not add themselves)
 *   vt_layernorm_bwd:  dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)) (+ residual, which may alias dx), g = dy gamma; mean
 *                      and rstd are recomputed from x.  `sums` (VT_CHANNEL_SUMS_BYTES(3, C) bytes, zeroed by the caller):
 *                      row 0 += sum_m dy xhat (d gamma), row 1 += sum_m dy (d beta), row 2 += sum_m dx without the
 *                      residual (d pre_bias; only when pre_bias is given)
 *   vt_scale_residual_fwd:  y = residual + gamma t (gamma NULL: y = residual + t)
 *   vt_scale_residual_bwd:  dt = dy gamma; `sums` (VT_CHANNEL_SUMS_BYTES(1, C)): row 0 += sum_m dy t (d gamma)
 *   vt_channel_sums_to_f32: dst_k[c] += sum over the replicas of row k (k < rows <= 3; a NULL dst_k is skipped)
 * A channel-sums buffer is int64[VT_STAT_REPLICAS][rows][C][2], the fixed-point format of the statistics buffers
 * (VT_STAT_REPLICAS): integer atomics, so these parameter gradients are bit-identical from run to run. */
#define VT_CHANNEL_SUMS_BYTES(rows, C) ((int64_t)VT_STAT_REPLICAS * (rows) * (C) * 16)
int vt_layernorm_fwd(const void* x, int32_t ldx, const float* pre_bias, const float* gamma, const float* beta, void* y,
                     int32_t ldy, int64_t M, int32_t C, float eps, int32_t dtype, void* stream);
int vt_layernorm_bwd(const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* pre_bias, const float* gamma,
                     void* dx, int32_t lddx, const void* residual, int32_t ldr, float* sums, int64_t M, int32_t C, float eps,
                     int32_t dtype, void* stream);
int vt_scale_residual_fwd(const void* t, int32_t ldt, const float* gamma, const void* residual, int32_t ldr, void* y,
                          int32_t ldy, int64_t M, int32_t C, int32_t dtype, void* stream);
int vt_scale_residual_bwd(const void* dy, int32_t lddy, const void* t, int32_t ldt, const float* gamma, void* dt,
                          int32_t lddt, float* sums, int64_t M, int32_t C, int32_t dtype, void* stream);
int vt_channel_sums_to_f32(const float* sums, int32_t rows, int32_t C, float* dst0, float* dst1, float* dst2, void* stream);

/* Token mixing (MLP-Mixer: reference backbones/mlp_mixer.py:28,34 -- a Linear over the TOKEN axis) and the patch gather of
 * the patch embedding (mlp_mixer.py:52,60), vt_token_mix.hip.  Maps are [B][tokens][C] rows with a row stride ld >= C, C a
 * multiple of 8 (bf16) / 4 (f32); the token counts K and M are arbitrary positive integers.
 *   vt_token_mix_fwd:    out[b][m][c] = sum_k A[m][k] x[b][k][c] (+ bias[m]) (+ residual[b][m][c], which may alias z);
 *                        A[m][k] = w[m * ldw + k], or w[k * ldw + m] with `transw` (the data gradient: the same weight,
 *                        K and M exchanged).  w has the map's dtype (bf16 launches read the bf16 mirror), bias is f32.
 *                        `z` receives out, `a` (optional) act(z) for activation code 0 / 4 (exact GELU) of the stored z;
 *                        either may be NULL.  bf16: mfma_f32_16x16x32_bf16 over x tiles read with ds_read_b64_tr_b16, a
 *                        64-row slice of W resident in LDS (K <= ~1000); f32: exact f32 FMA.
 *   vt_token_mix_wgrad:  dw[m][k] += sum_{b,c} dz[b][m][c] x[b][k][c] (dense [M][K]), dbias[m] += sum_{b,c} dz[b][m][c]
 *                        (either may be NULL).  Partial tiles are stored into slabs of `scratch`
 *                        (vt_token_mix_wgrad_scratch_bytes; a smaller scratch gets fewer, longer splits) and added in split
 *                        order: no float atomics, bit-identical from run to run.
 *   vt_patchify_fwd:     out[b][gy][gx][(py p + px) Cin + c] = img[b][gy p + py][gx p + px][c] -- the row order of the
 *                        channels_last filter image [d_model][p][p][Cin], so the embedding is a Linear over these rows
 *   vt_patchify_bwd:     the scatter back into the (channel padded) image gradient, pad channels zero (+ residual) */
int vt_token_mix_fwd(const void* x, int32_t ldx, const void* w, int32_t ldw, int32_t transw, const float* bias,
                     const void* residual, int32_t ldr, void* z, int32_t ldz, void* a, int32_t lda, int32_t act, int32_t B,
                     int32_t K, int32_t M, int32_t C, int32_t dtype, void* stream);
int64_t vt_token_mix_wgrad_scratch_bytes(int32_t B, int32_t K, int32_t M, int32_t C, int32_t dtype);
int vt_token_mix_wgrad(const void* dz, int32_t lddz, const void* x, int32_t ldx, float* dw, float* dbias, void* scratch,
                       int64_t scratch_bytes, int32_t B, int32_t K, int32_t M, int32_t C, int32_t dtype, void* stream);
int vt_patchify_fwd(const void* img, int32_t ldi, void* out, int32_t ldo, int32_t B, int32_t H, int32_t W, int32_t Cin,
                    int32_t p, int32_t dtype, void* stream);
int vt_patchify_bwd(const void* dout, int32_t lddo, void* dimg, int32_t ldg, const void* residual, int32_t ldr, int32_t B,
                    int32_t H, int32_t W, int32_t Cin, int32_t Cpad, int32_t p, int32_t dtype, void* stream);

/* Multi-head self-attention (ViT: reference backbones/vit.py:34-46 -- F.scaled_dot_product_attention over (B, heads, L,
 * head_dim) views) and a ViT's token bookkeeping (vit.py:145-151), vt_attention.hip.  Q, K, V, O and their gradients are
 * [B][L][heads * head_dim] token-major rows with a row stride each (a multiple of 8 (bf16) / 4 (f32), like heads * head_dim);
 * head h is the channel slice [h head_dim, (h + 1) head_dim), so the three operands may be channel slices of one [B][L][3 d]
 * buffer and nothing is transposed in memory.  head_dim is 32 or 64 (VT_ERR_UNSUPPORTED otherwise), L is arbitrary.
 *   vt_attn_fwd:   o = softmax(scale q k^T) v per (image, head); lse[B][heads][L] (f32) = log sum_k exp(scale q.k), for the
 *                  backward.  The L x L scores never reach memory: 64-query tiles against 64-key tiles with the running row
 *                  maximum subtracted.  bf16: mfma_f32_16x16x32_bf16 for both products, softmax in f32, P rounded to bf16
 *                  only as the operand of P v, V tiles read with ds_read_b64_tr_b16; f32: exact f32 FMA.
 *   vt_attn_bwd:   dq, dk, dv (each may be NULL) from q, k, v, o, dout and lse: P is recomputed from the scores and lse,
 *                  delta = rowsum(dout o) goes through `scratch` (vt_attn_bwd_scratch_bytes).  One kernel owns a key tile
 *                  and loops over query tiles (dk, dv), one owns a query tile and loops over key tiles (dq): no atomics,
 *                  bit-identical from run to run.
 *   vt_vit_tokens_fwd:   out[b][0] = cls (cls not NULL: c0 = 1, else c0 = 0), out[b][c0 + t] = embed[b][t] + pe[t];
 *                        embed is [B][T][C], out [B][c0 + T][C]; pe [T][C] and cls [C] are f32 masters
 *   vt_vit_tokens_bwd:   dembed[b][t] = dout[b][has_cls + t], dpe[t] += sum_b dout[b][has_cls + t], dcls += sum_b dout[b][0]
 *                        (f32, summed over the images in order by the one thread that owns the element; each may be NULL)
 *   vt_token_select_fwd: out[b] = x[b][t0]: row t0 of every image of [B][T][C] to [B][C]
 *   vt_token_select_bwd: dx[b][t0] = dout[b], every other row zero; with `accumulate` dx[b][t0] += dout[b] and the other rows
 *                        stay */
int vt_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                float* lse, float scale, int32_t B, int32_t heads, int32_t L, int32_t head_dim, int32_t dtype, void* stream);
int64_t vt_attn_bwd_scratch_bytes(int32_t B, int32_t heads, int32_t L);
int vt_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o, int32_t ldo,
                const void* dout, int32_t lddo, const float* lse, void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv,
                int32_t lddv, void* scratch, int64_t scratch_bytes, float scale, int32_t B, int32_t heads, int32_t L,
                int32_t head_dim, int32_t dtype, void* stream);
int vt_vit_tokens_fwd(const void* embed, int32_t lde, const float* pe, const float* cls, void* out, int32_t ldo, int32_t B,
                      int32_t T, int32_t C, int32_t dtype, void* stream);
int vt_vit_tokens_bwd(const void* dout, int32_t lddo, void* dembed, int32_t lde, float* dpe, float* dcls, int32_t has_cls,
                      int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream);
int vt_token_select_fwd(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t B, int32_t T, int32_t t0, int32_t C,
                        int32_t dtype, void* stream);
int vt_token_select_bwd(const void* dout, int32_t lddo, void* dx, int32_t ldx, int32_t accumulate, int32_t B, int32_t T,
                        int32_t t0, int32_t C, int32_t dtype, void* stream);

/* Shifted-window attention with a learned relative-position bias (Swin: reference backbones/swin.py:32-86 -- roll, window
 * partition, MHA with attn_bias = table[index] (+ the -100 region mask), un-partition, roll back), vt_window_attention.hip.
 * Q, K, V, O and their gradients are [B][H][W][heads * head_dim] pixel-major rows of an NHWC map with a pixel stride each (a
 * multiple of 8 (bf16) / 4 (f32)); head h is the channel slice [h head_dim, (h + 1) head_dim), so q | k | v may be channel
 * slices of one [B][H][W][3 C] buffer.  The partition and both rolls are index arithmetic in the loads and stores
 * (vt_window_index.h): token t = i ws + j of window (wy, wx) is pixel ((wy ws + i + shift) mod H, (wx ws + j + shift) mod W),
 * and o goes back to that pixel; no map is gathered, rolled or copied.  `table` is the f32 master [heads][(2 ws - 1)^2], read
 * at (i_q - i_k + ws - 1)(2 ws - 1) + (j_q - j_k + ws - 1); with shift > 0, -100.0 is added where query and key lie in
 * different regions of the rolled map (3 per axis: [0, n - ws), [n - ws, n - shift), [n - shift, n)).
 * head_dim is 32, ws^2 <= 64 (a window is one 64-row tile; ws = 14 is VT_ERR_UNSUPPORTED), 0 <= shift < ws, H and W
 * multiples of ws (VT_ERR_INVALID otherwise).
 *   vt_win_attn_fwd:  o = softmax(scale q k^T + bias + mask) v per (window, head), one workgroup each;
 *                     lse[B][heads][H W] (f32, at the pixel) = the log-sum-exp of the row.  bf16: mfma_f32_16x16x32_bf16 for
 *                     both products, softmax in f32 with the row maximum subtracted after bias and mask; f32: exact f32 FMA.
 *   vt_win_attn_bwd:  dq, dk, dv, dtable (each may be NULL) in ONE kernel per (window, head): P and dS = P o (dout v^T - delta)
 *                     are formed once, delta = rowsum(dout o) inside the kernel.  dtable[h][idx] += the sum over images,
 *                     windows and (q, k) pairs with that index of dS (the gradient of the pre-softmax score, unscaled):
 *                     every workgroup stores its share into `scratch` (vt_win_attn_bwd_scratch_bytes) and a second kernel
 *                     adds the shares in a fixed order.  No atomics: bit-identical from run to run.  `scratch` is read and
 *                     checked only where dtable is given; with dtable NULL it may be NULL. */
int vt_win_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                    float* lse, const float* table, float scale, int32_t B, int32_t H, int32_t W, int32_t heads, int32_t head_dim,
                    int32_t ws, int32_t shift, int32_t dtype, void* stream);
int64_t vt_win_attn_bwd_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t heads, int32_t ws);
int vt_win_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o,
                    int32_t ldo, const void* dout, int32_t lddo, const float* lse, const float* table, void* dq, int32_t lddq,
                    void* dk, int32_t lddk, void* dv, int32_t lddv, float* dtable, void* scratch, int64_t scratch_bytes,
                    float scale, int32_t B, int32_t H, int32_t W, int32_t heads, int32_t head_dim, int32_t ws, int32_t shift,
                    int32_t dtype, void* stream);

/* The two attention forms of CaiT (reference backbones/cait.py:16-51) and the token bookkeeping of its class-attention
 * stage, vt_talking_attention.hip.  Layout as vt_attn_*: [B][L][heads * head_dim] token-major rows with a row stride each (a
 * multiple of 8 (bf16) / 4 (f32)), head h is a channel slice, q | k | v may be slices of one buffer.
 * Talking heads, per image, s = scale, Wl / Ww the [heads][heads] f32 masters of the two 1x1 mixes, bl / bw their [heads]
 * biases (may be NULL = 0):
 *     A_h = s q_h k_h^T    M_g = sum_h Wl[g,h] A_h + bl[g]    P_g = softmax_j M_g    R_g = sum_h Ww[g,h] P_h + bw[g]
 *     O_g = R_g v_g        lse[B][heads][L] (f32) = logsumexp_j M_g
 * head_dim is 48 and 1 <= heads <= 16 (VT_ERR_UNSUPPORTED otherwise), L is arbitrary.  The L x L planes never reach memory:
 * a workgroup owns a 16-row tile of an image and ALL heads, a thread owns one (query, key) pair and mixes the heads in
 * registers; two passes over the key tiles (lse of M, then the normalised P mixed to R and R v).  f32: exact f32 FMA.  bf16
 * forward: mfma_f32_16x16x32_bf16 (second k-step zero-padded from 48) for the scores, the mixes on the accumulator tiles, R
 * rounded to bf16 as the operand of mfma_f32_16x16x16_bf16 for R v.  The backward computes in f32 FMA in both dtypes (bf16
 * operands are widened when staged: the loads and stores are its only rounding points).
 *   vt_talk_attn_bwd: dq, dk, dv, dwl, dbl, dww, dbw (each may be NULL; the parameter gradients accumulate with += in f32)
 *                     from q, k, v, dout, lse and the parameters; P is recomputed from lse.  delta_h = sum_j dP_h P_h (not
 *                     rowsum(dout o)) takes a pass of its own over the keys.  One kernel owns query tiles (delta, dq and the
 *                     workgroup's share of the parameter gradients), one owns key tiles (dk, dv); a third adds the shares in
 *                     a fixed order.  No atomics: bit-identical from run to run.
 *                     scratch bytes = 4 (B heads L + B ceil(L / 16) (2 heads^2 + 2 heads)): delta, then the shares.
 * Class attention: plain softmax attention of ONE query row per image.  q, o, dout, dq are [B][heads * head_dim] rows; k, v,
 * dk, dv are [B][Lk][heads * head_dim]; lse is [B][heads].  head_dim 32, 48 or 64.  One wave per (image, head), vector FMA,
 * k and v read once; the backward (delta = dout . o) writes every row of dk and dv with plain stores, no scratch, no
 * atomics; dq, dk, dv may each be NULL, not all.
 *   vt_token_prepend_fwd: out[b][0] = first[b] ([B][C] activation) or first_param ([C] f32 master, broadcast); exactly one
 *                         of the two is non-NULL; out[b][1 + t] = x[b][t].  x is [B][T][C], out [B][1 + T][C].
 *   vt_token_prepend_bwd: dx[b][t] (+)= dout[b][1 + t] (`accumulate`), dfirst[b] = dout[b][0] or dfirst_param += sum_b
 *                         dout[b][0] in image order; each may be NULL, not all. */
int vt_talk_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                     float* lse, const float* wl, const float* bl, const float* ww, const float* bw, float scale, int32_t B,
                     int32_t heads, int32_t L, int32_t head_dim, int32_t dtype, void* stream);
int64_t vt_talk_attn_bwd_scratch_bytes(int32_t B, int32_t heads, int32_t L);
int vt_talk_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* dout,
                     int32_t lddo, const float* lse, const float* wl, const float* bl, const float* ww, const float* bw, void* dq,
                     int32_t lddq, void* dk, int32_t lddk, void* dv, int32_t lddv, float* dwl, float* dbl, float* dww, float* dbw,
                     void* scratch, int64_t scratch_bytes, float scale, int32_t B, int32_t heads, int32_t L, int32_t head_dim,
                     int32_t dtype, void* stream);
int vt_cls_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                    float* lse, float scale, int32_t B, int32_t heads, int32_t Lk, int32_t head_dim, int32_t dtype, void* stream);
int vt_cls_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o, int32_t ldo,
                    const void* dout, int32_t lddo, const float* lse, void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv,
                    int32_t lddv, float scale, int32_t B, int32_t heads, int32_t Lk, int32_t head_dim, int32_t dtype,
                    void* stream);
int vt_token_prepend_fwd(const void* x, int32_t ldx, const void* first, int32_t ldf, const float* first_param, void* out,
                         int32_t ldo, int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream);
int vt_token_prepend_bwd(const void* dout, int32_t lddo, void* dx, int32_t ldx, int32_t accumulate, void* dfirst, int32_t ldf,
                         float* dfirst_param, int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream);

/* PatchConvNet (reference backbones/patchconvnet.py:25-103; vt_patchconv.hip).  bf16 and f32, f32 arithmetic from
 * storage-rounded operands, pixel strides ld >= C, C a multiple of a 16-byte chunk.  No float atomics: a workgroup owns one
 * image and one slab of channels and walks all its pixels, so every sum has one owner and a fixed order and every result is
 * bit-identical from run to run.
 *   vt_dw3_gelu_pool_fwd: a = GELU(dwconv3x3_pad1(u, w) + bias) (exact GELU; stored in the compute dtype) and
 *                         pooled[b][c] = mean over the pixels of the STORED a, a [B][C] row in the compute dtype (the
 *                         contract of vt_global_avgpool_fwd).  u, a are [B][H][W][C]; w is the f32 master [C][9] (bf16
 *                         launches round it as vt_dwconv_fwd does), bias the f32 master [C] or NULL.  The slab's u plane is
 *                         staged with its halo in LDS.
 *   vt_dw3_gelu_pool_bwd: the whole backward of that column in one kernel: z is recomputed (never stored),
 *                         dz = (da + dpooled / HW) * GELU'(z) is formed into an LDS plane, du = conv_transpose(dz, w)
 *                         (+ residual, which may alias du), and the image's share of dw[c][9] and dbias[c] goes to
 *                         scratch [B][C][10] f32; a second small kernel adds the shares over the images in image order
 *                         into the f32 gradients (+=).  da or dpooled may be NULL (zero), du / dw / dbias too (not all).
 *   Both return VT_ERR_UNSUPPORTED for a map whose planes ((H + 2)(W + 2) cells of one 16-byte chunk, plus 4 bytes per
 *   element for dz in the backward) exceed the 160 KiB of LDS; vt_dw3_gelu_pool_supported(H, W, dtype) tells (1 / 0).
 *   vt_se_gate_fwd:       y = a * sigmoid(s[b][c]); a, y are [B][HW][C], s is [B][C] in the compute dtype
 *   vt_se_gate_bwd:       da (+)= dy * sigmoid(s) (`accumulate`), ds[b][c] = sigmoid'(s) * sum_pixels dy * a, f32 [B][C]
 *   vt_channel_stats:     per-channel sum and sum of squares of a stored [M][C] map into a statistics buffer: exactly the
 *                         contract of VT_CONV_STATS (fixed point, VT_STAT_REPLICAS; zeroed by the caller).  For a BatchNorm
 *                         in front of its convolution, which has no producing conv epilogue.
 *   vt_pool_attn_fwd/bwd: softmax attention of ONE query row per image with ONE head of width C (any multiple of a 16-byte
 *                         chunk up to 256 chunks).  q, o, dout, dq are [B][C]; k, v, dk, dv are [B][Lk][C]; lse is [B].  One
 *                         workgroup per image; the backward (delta = dout . o) writes dq and every row of dk and dv with
 *                         plain stores; each may be NULL, not all. */
int vt_dw3_gelu_pool_supported(int32_t H, int32_t W, int32_t dtype);
int vt_dw3_gelu_pool_fwd(const void* u, int32_t ldu, const float* w, const float* bias, void* a, int32_t lda, void* pooled,
                         int32_t ldp, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
int64_t vt_dw3_gelu_pool_bwd_scratch_bytes(int32_t B, int32_t C);
int vt_dw3_gelu_pool_bwd(const void* u, int32_t ldu, const void* da, int32_t ldda, const void* dpooled, int32_t lddp,
                         const float* w, const float* bias, void* du, int32_t lddu, const void* residual, int32_t ldr, float* dw,
                         float* dbias, void* scratch, int64_t scratch_bytes, int32_t B, int32_t H, int32_t W, int32_t C,
                         int32_t dtype, void* stream);
int vt_se_gate_fwd(const void* a, int32_t lda, const void* s, int32_t lds, void* y, int32_t ldy, int32_t B, int32_t HW, int32_t C,
                   int32_t dtype, void* stream);
int vt_se_gate_bwd(const void* dy, int32_t lddy, const void* a, int32_t lda, const void* s, int32_t lds, void* da, int32_t ldda,
                   float* ds, int32_t B, int32_t HW, int32_t C, int32_t accumulate, int32_t dtype, void* stream);
int vt_channel_stats(const void* x, int32_t ldx, int64_t M, int32_t C, int32_t dtype, float* stats, void* stream);
int vt_pool_attn_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                     float* lse, float scale, int32_t B, int32_t Lk, int32_t C, int32_t dtype, void* stream);
int vt_pool_attn_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, const void* o, int32_t ldo,
                     const void* dout, int32_t lddo, const float* lse, void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv,
                     int32_t lddv, float scale, int32_t B, int32_t Lk, int32_t C, int32_t dtype, void* stream);

/* The token bookkeeping of DeiT (reference backbones/deit.py:37-41 -- cat([cls_token, dist_token, patches + pe], 1) in front
 * of the blocks, norm(out[:, :2]).mean(1) behind them), general in the number of prefix rows P, vt_prefix_tokens.hip.  bf16
 * and f32, f32 arithmetic from storage-rounded operands, one rounding at the store.  Rows are [B][rows][C] with a row stride
 * each (ld >= C, a multiple of 8 (bf16) / 4 (f32), like C: VT_ERR_UNSUPPORTED / VT_ERR_INVALID otherwise); 1 <= P <= 4.  Every
 * global access is a 16-byte chunk per lane; no float atomics: every sum has one owner or goes through the fixed-point
 * channel-sums buffer, so every result is bit-identical from run to run.
 *   vt_prefix_tokens_fwd: out[b][p] = prefix[p] (p < P; `prefix` is a HOST array of P device pointers to f32 masters of C
 *                         values each, broadcast over the batch; no position is added), out[b][P + t] = embed[b][t] + pe[t];
 *                         embed is [B][T][C], out [B][P + T][C], pe the f32 master [T][C]
 *   vt_prefix_tokens_bwd: dembed[b][t] = dout[b][P + t], dpe[t] += sum_b dout[b][P + t], dprefix[p] += sum_b dout[b][p]
 *                         (f32, summed over the images in order by the one thread that owns the chunk).  dembed, dpe, the
 *                         array dprefix and each of its P entries may be NULL, not all of them.
 *   vt_prefix_pool_fwd:   y[b] = (1 / P) sum_{p < P} LayerNorm_C(x[b][p]; gamma, beta, eps); x is [B][L][C] (L >= P), y is
 *                         [B][C]; C <= 3072 (a wave holds a row in registers)
 *   vt_prefix_pool_bwd:   dx[b][p] (= | +=, `accumulate`) the LayerNorm backward of dy[b] / P through row p, mean and rstd
 *                         recomputed from x; rows t >= P of dx are written ZERO with accumulate = 0 and left alone with
 *                         accumulate = 1 (the gradient is rounded to the storage type before it is added).  `sums`
 *                         (VT_CHANNEL_SUMS_BYTES(2, C) bytes, zeroed by the caller; vt_channel_sums_to_f32 folds it):
 *                         row 0 += sum_{b,p} (dy[b] / P) xhat[b][p] (d gamma), row 1 += sum_b dy[b] (d beta) */
int vt_prefix_tokens_fwd(const void* embed, int32_t lde, const float* pe, const float* const* prefix, int32_t P, void* out,
                         int32_t ldo, int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream);
int vt_prefix_tokens_bwd(const void* dout, int32_t lddo, void* dembed, int32_t lde, float* dpe, float* const* dprefix, int32_t P,
                         int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream);
int vt_prefix_pool_fwd(const void* x, int32_t ldx, const float* gamma, const float* beta, void* y, int32_t ldy, int32_t B,
                       int32_t L, int32_t P, int32_t C, float eps, int32_t dtype, void* stream);
int vt_prefix_pool_bwd(const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* gamma, void* dx, int32_t lddx,
                       int32_t accumulate, float* sums, int32_t B, int32_t L, int32_t P, int32_t C, float eps, int32_t dtype,
                       void* stream);

/* Filter gradient: dw[n][t][c] += sum_pixels dz(pix,n) * x_gathered(pix,t,c),
 * fp32 accumulation straight into the (channels_last) .grad of the weight.
 * `d` is the forward descriptor (ldy = pixel stride of dz).  Replaces the
 * autograd backward of nn.Conv2d (components.py:26-35). */
int vt_conv_wgrad(const vt_conv_desc* d, const void* x, const void* dz, float* dw,
                  int32_t ldgw, void* stream);

/* The same filter gradient in two stages: every (tile, pixel split) workgroup stores its partial tile into its own slab of
 * `scratch` (plain stores) and a second kernel adds the slabs to dw in split order -- no atomics, and a result that does
 * not depend on the order in which workgroups finish.  One scratch of ~40 MB serves every layer (launches on one stream
 * reuse it, so it stays in the memory-side cache); a scratch too small for a layer's usual split gets fewer, longer splits,
 * never atomics across splits.  (Deterministic mode.) */
int vt_conv_wgrad_slabs(const vt_conv_desc* d, const void* x, const void* dz, float* dw, int32_t ldgw,
                        void* scratch, int64_t scratch_bytes, void* stream);

/* n filter gradients of ONE descriptor -- same-shape layers, e.g. the 3x3 convs of a stage's DarknetBlocks
 * (darknet.py:20-28) or of an OSA chain (vovnet.py:41-44) -- in as few launches as the kernels allow: the CU-owning
 * stride-1 3x3 kernel takes up to 8 layers per launch and pays its prologue and its f32 atomic flush once per launch
 * (a filter gradient has no consumer before the optimiser, so a caller may hold the layers of a stage back until the
 * last one's dz exists).  Shapes that kernel does not cover run one by one, exactly as vt_conv_wgrad -- except, with
 * the knob VT_WGRAD_GROUP_1X1=1, 1x1 stride-1 layers, which then share launches of the general kernel (up to 8 layers,
 * one atomic flush; off by default).  x / dz / dw are HOST arrays of n device pointers. */
int vt_conv_wgrad_group(const vt_conv_desc* d, int32_t n, const void* const* x, const void* const* dz,
                        float* const* dw, int32_t ldgw, void* stream);

/* dst[i] (+)= hi[i]*2^12 + lo[i]/2^33 for a fixed-point buffer q = int64[n][2] (vt_colsum_fixed); a marked entry
 * (|hi| >= 2^38, see VT_STAT_REPLICAS: a non-finite or out-of-range contribution) yields NaN. */
int vt_fixed_to_f32(const void* q, float* dst, int64_t n, int32_t accumulate, void* stream);

/* Re-pack a [Cout][ntaps][Cin] filter (f32 master or dtype mirror) into the
 * [Cin][nsel][Cout] image the data-gradient launch reads; sel[i] is the source
 * tap of packed tap i (-1: a zero tap, for the column blocks of a VT_CONV_D2S filter image). */
int vt_pack_dgrad_filter(const void* w, int32_t src_dtype, int32_t ldw, void* out,
                         int32_t dst_dtype, const int32_t* sel_host, int32_t nsel,
                         int32_t Cout, int32_t ntaps, int32_t Cin, void* stream);
/* The same for n filters in ceil(n / VT_PACK_BATCH) launches (bf16 -> bf16 only): a train step re-packs every filter
 * once, 73 launches of ~6 us for CSPDarknet-53, which cost 0.3 ms of the step through the launches alone.  The
 * executor (vt_run_ops*) gathers consecutive VT_OP_PACK_DGRAD ops of one stream into this call by itself. */
#define VT_PACK_BATCH 40
typedef struct vt_pack_item {
    const void* w;
    void* out;
    int32_t ldw, nsel, Cout, ntaps, Cin;
    int8_t sel[VT_MAX_TAPS];
} vt_pack_item;
int vt_pack_dgrad_filter_batch(const vt_pack_item* items, int32_t n, void* stream);

/* ---- BatchNorm2d + ReLU (components.py:36-44) --------------------------- */
/* training: stats -> batch mean/var, running-stat update (momentum, unbiased
 * var), scale = gamma*invstd, shift = beta - mean*scale. */
int vt_bn_finalize(const float* stats, int32_t C, double count, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean,
                   float* running_var, int64_t* num_batches_tracked, float* scale,
                   float* shift, float* mean, float* invstd, void* stream);
/* Fold the VT_STAT_REPLICAS replicas of a statistics / sums buffer into replica 0 (exact integer adds) and zero the
 * others: SyncBatchNorm then all-reduces 32*C bytes per layer instead of the whole buffer.  The marker of a non-finite
 * contribution (see VT_STAT_REPLICAS) is part of the hi limb and is folded with it. */
int vt_stat_fold(float* stats, int32_t C, void* stream);
/* eval: coefficients from the running statistics. */
int vt_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int32_t C, float* scale,
                      float* shift, float* mean, float* invstd, void* stream);
/* n of them in ceil(n / VT_PACK_BATCH) launches (the executor gathers consecutive VT_OP_BN_EVAL_COEFFS ops itself) */
typedef struct vt_bn_eval_item {
    const float *gamma, *beta, *running_mean, *running_var;
    float *scale, *shift, *mean, *invstd;
    int32_t C;
    float eps;
} vt_bn_eval_item;
int vt_bn_eval_coeffs_batch(const vt_bn_eval_item* items, int32_t n, void* stream);
/* y = act(z*scale + shift) [+ residual].  `relu` here and in vt_bn_act_bwd_reduce / _bwd_apply is an ACTIVATION CODE
 * (ConvNormAct's `act`, components.py:37-44): 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 SiLU ("swish"), 4 GELU (exact), 5 ReLU6, 6 Hardswish
 * (torchvision's MobileNets; derivatives as torch: ReLU6' = 1 on 0 < u < 6, Hardswish' = (2u + 3) / 6 on -3 <= u <= 3).  Codes 0 / 1
 * are the Darknet / VoVNet path; 2-6 run generic instantiations of the same kernels (round 5). */
int vt_bn_act_apply(const void* z, int32_t ldz, const float* scale, const float* shift,
                    const void* residual, int32_t ldr, void* y, int32_t ldy, int64_t M,
                    int32_t C, int32_t relu, int32_t dtype, void* stream);
/* sums (statistics buffer, see VT_STAT_REPLICAS): [0][c] += sum g, [1][c] += sum g*xhat, g = dy*[z*scale+shift>0] */
int vt_bn_act_bwd_reduce(const void* dy, int32_t lddy, const void* z, int32_t ldz,
                         const float* scale, const float* shift, const float* mean,
                         const float* invstd, int64_t M, int32_t C, int32_t relu,
                         int32_t dtype, float* sums, void* stream);
/* dgamma += pscale * sum g*xhat; dbeta += pscale * sum g; coef[3][C] for vt_bn_act_bwd_apply.
 * train!=0: full batch-norm gradient; train==0: statistics are constants.
 * SyncBatchNorm (configs/base.yaml:22): `sums` then hold the all-reduced sums and `count` the
 * global sample count; pscale = 1/world keeps the parameter gradients rank-local in size, so
 * the gradient all-reduce(mean) that follows yields the same values as torch's SyncBatchNorm. */
int vt_bn_bwd_finalize(const float* sums, int32_t C, double count, double pscale,
                       const float* scale, const float* mean, const float* invstd, int32_t train,
                       float* dgamma, float* dbeta, float* coef, void* stream);
/* dz = coef0[c]*g - coef1[c]*z + coef2[c], g = dy * act'(z*scale + shift).
 * scale, shift and coef ALL NULL: dz = dy * act'(z) -- the activation of a ConvNormAct built with norm="none"
 * (reference components.py:36: nn.Identity between the biased conv and the activation). */
int vt_bn_act_bwd_apply(const void* dy, int32_t lddy, const void* z, int32_t ldz,
                        const float* scale, const float* shift, const float* coef,
                        void* dz, int32_t lddz, int64_t M, int32_t C, int32_t relu,
                        int32_t dtype, void* stream);

/* The three calls above in ONE launch where the operands fit the register file (round 6, vt_bn_bwd_fused.hip): every
 * thread keeps its rows of dy and z packed in registers between the reduction and the apply pass, two device-scope grid
 * barriers (at most one workgroup per CU: all resident) separate reduce | finalize | apply -- dy and z are read once instead
 * of twice and two launches disappear.  bf16, activation code 0 / 1, C <= 4096, up to 13 x 16 bytes per thread and tensor
 * (256 channels @14x14 and smaller at batch 256); any other call runs vt_bn_act_bwd_reduce, vt_bn_bwd_finalize and
 * vt_bn_act_bwd_apply, with identical arguments and results that differ by the order of the f32 partial sums only.
 * `sums`: a zeroed statistics buffer; `sync`: 16 zeroed bytes (two barrier counters, one error flag).  A barrier that does not
 * complete within ~4 ms of wall clock gives up (no hang) and is counted: vt_bn_bwd_fused_timeouts must read 0.
 * Replaces the autograd backward of nn.BatchNorm2d + nn.ReLU (components.py:36-44). */
int vt_bn_act_bwd_fused(const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* scale, const float* shift,
                        const float* mean, const float* invstd, int64_t M, int32_t C, int32_t relu, int32_t dtype,
                        double count, double pscale, int32_t train, float* sums, void* sync, float* dgamma, float* dbeta,
                        float* coef, void* dz, int32_t lddz, void* stream);
int vt_bn_bwd_fused_timeouts(uint32_t* count);
/* vt_bn_finalize + vt_bn_act_apply, and vt_bn_bwd_finalize + vt_bn_act_bwd_apply, as ONE launch each (round 6).  The sums
 * are complete when the streaming launch starts, so nothing is handed over inside it: EVERY workgroup finalizes the (at most
 * 128) channels of its own channel group for itself -- a thread per (channel, sum), the 16 replicas x 2 limbs in one round
 * of loads, the same arithmetic bit for bit -- and keeps the coefficients in LDS; the workgroups of row block 0 also store
 * them, the running statistics and d(gamma) / d(beta).  The single-workgroup finalize launch between a producer of
 * statistics and the pass that needs the coefficients (9 - 13 us of the step each, 134 per CSPDarknet-53 step) disappears;
 * the grid is cut for ~1536 workgroups (knob VT_BN_FIN_APPLY_WGS) so that the redundant reads stay small.  Same arguments,
 * same results (bit-identical) as the two calls each replaces.  Those two calls run for activation codes >= 2, for channel
 * counts without a divisor in [32, 128] that is a multiple of the 16-byte chunk (other than C itself), and with the knob
 * VT_BN_FIN_APPLY = 0.  (The first form of these launches -- the first workgroups finalize and publish, all others poll a
 * counter -- measured 2.3 ms slower per step, NOTEBOOK R6.6.) */
int vt_bn_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                         float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* scale,
                         float* shift, float* mean, float* invstd, const void* z, int32_t ldz,
                         const void* residual, int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t relu, int32_t dtype,
                         void* stream);
int vt_bn_bwd_finalize_apply(const float* sums, int32_t C, double count, double pscale, const float* scale,
                             const float* shift, const float* mean, const float* invstd, int32_t train, float* dgamma,
                             float* dbeta, float* coef, const void* dy, int32_t lddy, const void* z, int32_t ldz,
                             void* dz, int32_t lddz, int64_t M, int32_t relu, int32_t dtype, void* stream);

/* ---- BatchNorm passes whose residual joins BEFORE the activation (vt_resnet.hip) ------------------------------------
 * The last unit of a torchvision BasicBlock / Bottleneck: y = relu(bn(conv(h)) + identity).  The passes above implement
 * relu(bn(conv)) + residual (a DarknetBlock): their mask is z*scale + shift > 0 and the residual's gradient is dy.  Here
 * the mask depends on the sum and the identity's gradient is the masked dy:
 *   vt_bn_add_act_apply                y  = relu(z*scale + shift + r)                        (r may alias y)
 *   vt_bn_add_act_bwd_reduce           g  = dy * [y > 0]; sums[0][c] += sum g, sums[1][c] += sum g*xhat (statistics buffer)
 *   vt_bn_add_act_bwd_apply            dz = coef0*g - coef1*z + coef2; dr = g, or dr += g with `accumulate`
 * The mask is read from the STORED y in its own dtype (what torch's in-place ReLU does): exact against the forward's
 * decision.  vt_bn_add_act_finalize_apply / vt_bn_add_act_bwd_finalize_apply run the finalize step inside the launch, with
 * the arguments, the arithmetic (vt_bn_finalize / vt_bn_bwd_finalize, bit for bit) and the fall-back to two launches of
 * vt_bn_finalize_apply / vt_bn_bwd_finalize_apply.  bf16 and f32, channel-last rows of ld* elements; dz and dr are two
 * tensors; no float atomics: two runs give bit-identical results. */
int vt_bn_add_act_apply(const void* z, int32_t ldz, const float* scale, const float* shift, const void* r, int32_t ldr, void* y,
                        int32_t ldy, int64_t M, int32_t C, int32_t dtype, void* stream);
int vt_bn_add_act_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                                 float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                 float* scale, float* shift, float* mean, float* invstd, const void* z, int32_t ldz, const void* r,
                                 int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t dtype, void* stream);
int vt_bn_add_act_bwd_reduce(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                             const float* mean, const float* invstd, int64_t M, int32_t C, int32_t dtype, float* sums,
                             void* stream);
int vt_bn_add_act_bwd_apply(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                            const float* coef, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate, int64_t M,
                            int32_t C, int32_t dtype, void* stream);
int vt_bn_add_act_bwd_finalize_apply(const float* sums, int32_t C, double count, double pscale, const float* scale,
                                     const float* mean, const float* invstd, int32_t train, float* dgamma, float* dbeta,
                                     float* coef, const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z,
                                     int32_t ldz, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate, int64_t M,
                                     int32_t dtype, void* stream);

/* The same five passes with a per-image keep factor: stochastic depth of a ResNet block as timm's ResNet places it, behind
 * the last BatchNorm and in front of the shortcut,  y = relu(keep[b] * bn(conv(h)) + identity).  `keep` is a device
 * float[M / HW] of any values (0, or 1 / (1 - p) for a kept image); image b = row / HW, M = B * HW < 2^31 rows.
 *   forward   y = relu(keep[b] * (z*scale + shift) + r); where keep[b] == 0 the rows of z are not read and y = relu(r)
 *   backward  g = dy * [y > 0] from the stored y.  The identity receives g (written, or accumulated).  The BatchNorm side
 *             sees u = keep[b] * g: sums[0][c] += sum u, sums[1][c] += sum u*xhat (a dropped image's rows are not read),
 *             dz = coef0*u - coef1*z + coef2 (a dropped image's z IS read: under batch statistics its dz is
 *             -coef1*z + coef2; with the coefficients of a frozen BatchNorm it is 0)
 * With keep[b] == 1 everywhere every output has the bits of the pass without `keep`.  No float atomics. */
int vt_bn_add_act_keep_apply(const void* z, int32_t ldz, const float* scale, const float* shift, const void* r, int32_t ldr, void* y,
                             int32_t ldy, const float* keep, int32_t HW, int64_t M, int32_t C, int32_t dtype, void* stream);
int vt_bn_add_act_keep_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                                      float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                      float* scale, float* shift, float* mean, float* invstd, const void* z, int32_t ldz,
                                      const void* r, int32_t ldr, void* y, int32_t ldy, const float* keep, int32_t HW, int64_t M,
                                      int32_t dtype, void* stream);
int vt_bn_add_act_keep_bwd_reduce(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                                  const float* mean, const float* invstd, const float* keep, int32_t HW, int64_t M, int32_t C,
                                  int32_t dtype, float* sums, void* stream);
int vt_bn_add_act_keep_bwd_apply(const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z, int32_t ldz,
                                 const float* coef, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate,
                                 const float* keep, int32_t HW, int64_t M, int32_t C, int32_t dtype, void* stream);
int vt_bn_add_act_keep_bwd_finalize_apply(const float* sums, int32_t C, double count, double pscale, const float* scale,
                                          const float* mean, const float* invstd, int32_t train, float* dgamma, float* dbeta,
                                          float* coef, const void* dy, int32_t lddy, const void* y, int32_t ldy, const void* z,
                                          int32_t ldz, void* dz, int32_t lddz, void* dr, int32_t lddr, int32_t accumulate,
                                          const float* keep, int32_t HW, int64_t M, int32_t dtype, void* stream);

/* ---- the ResNet stem Conv2d(3, Cout, 7, stride 2, padding 3) as a 4x4 stride-1 convolution (vt_resnet.hip) -----------
 * 49 taps do not fit VT_MAX_TAPS.  Padded to 8x8 with a zero first row and column the filter is a 4x4 stride-1 filter over
 * the space-to-depth image xs[b][hs][ws][(py, px, c)] = x[b][2hs + py][2ws + px][c] (12 channels, padded with zeros to
 * vt_stem7_s2d_channels(dtype): 16 for bf16, 12 for f32), the sixteen taps at row / column offsets -2 .. +1: a vt_conv_desc
 * with Hi = Ho = ceil(H / 2), h0 = w0 = -2, dh = t / 4, dw = t % 4, which vt_conv_igemm and vt_conv_wgrad run.  Odd H or W: a
 * zero row / column at the far edge, which is what the convolution's own padding holds there.
 *   vt_stem7_s2d           the image gather; x has its 3 channels in one 16-byte chunk per pixel (ldx elements apart)
 *   vt_stem7_pack_filter   w [Cout][7][7][3] (f32 or bf16) -> out [Cout][4][4][Cs] (dst_dtype)
 *   vt_stem7_unpack_wgrad  dw [Cout][7][7][3] += dws [Cout][4][4][Cs], both f32 (the transpose of the repack) */
int32_t vt_stem7_s2d_channels(int32_t dtype);
int vt_stem7_s2d(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t B, int32_t H, int32_t W, int32_t dtype,
                 void* stream);
int vt_stem7_pack_filter(const void* w, int32_t src_dtype, void* out, int32_t dst_dtype, int32_t Cout, void* stream);
int vt_stem7_unpack_wgrad(const float* dws, int32_t Cs, float* dw, int32_t Cout, void* stream);

/* ---- grouped 3x3 convolution of the RegNet blocks, and their Squeeze-Excitation MLP (vt_gconv.hip) --------------------
 * 3x3, padding 1, dilation 1, stride 1 or 2, Cin = Cout = C in C / gw groups of gw channels; gw a multiple of 8 from 8 to 64
 * (VT_ERR_UNSUPPORTED otherwise).  x, z, dz, dx are channel-last maps with pixel strides ld >= C (channel slices of wider
 * buffers work); Ho = (Hi - 1) / stride + 1.  The filter is [C][3][3][gw] in the compute dtype (torch's grouped OIHW weight
 * with the taps in front of the group's input channels).  bf16 (matrix unit, f32 accumulation) and f32 (exact FMA over the
 * same index maps).  ONE launch over the whole map each; no float atomics: two runs give bit-identical results.
 *   vt_gconv3_fwd    z = conv(x, w); `stats` (or NULL): per-channel sum and sum of squares of the STORED z into a
 *                    statistics buffer, the contract of VT_CONV_STATS (fixed point, zeroed by the caller)
 *   vt_gconv3_dgrad  dx = conv_transpose(dz, w) [+ residual, which may alias dx]; every pixel of dx is written, also the
 *                    ones no tap reaches under stride 2
 *   vt_gconv3_wgrad  dw [C][3][3][gw] f32 += sum over the pixels of dz (x) x: the pixels are cut into slabs, a workgroup
 *                    stores its slab's partial filter into `scratch` (vt_gconv3_wgrad_scratch_bytes), a second kernel adds
 *                    the slabs in slab order with one owner per filter element
 *   vt_se_mlp_fwd    per image: hidden = relu(W1 pooled + b1) (S values, any S >= 1; kept as f32 [B][S] holding the
 *                    values rounded to the compute dtype), logits = W2 hidden + b2, a [B][C] row in the compute dtype: the
 *                    operand `s` of vt_se_gate_fwd.  W1 [S][C], W2 [C][S], b1, b2 are the f32 masters (bf16 launches round
 *                    the weights as the bf16 mirror does).  C <= 8192, S <= 2048.
 *   vt_se_mlp_bwd    from d(logits): d(pooled) (or NULL), and dW1, db1, dW2, db2 (f32, +=; each may be NULL) with one owner
 *                    per parameter element adding the images in image order.  `dhidden` is f32 [B][S] scratch. */
int vt_gconv3_fwd(const void* x, int32_t ldx, const void* w, void* z, int32_t ldz, float* stats, int32_t B, int32_t Hi, int32_t Wi,
                  int32_t C, int32_t gw, int32_t stride, int32_t dtype, void* stream);
int vt_gconv3_dgrad(const void* dz, int32_t lddz, const void* w, void* dx, int32_t lddx, const void* residual, int32_t ldr,
                    int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t gw, int32_t stride, int32_t dtype, void* stream);
int64_t vt_gconv3_wgrad_scratch_bytes(int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t gw, int32_t stride);
int vt_gconv3_wgrad(const void* x, int32_t ldx, const void* dz, int32_t lddz, float* dw, void* scratch, int64_t scratch_bytes,
                    int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t gw, int32_t stride, int32_t dtype, void* stream);
int vt_se_mlp_fwd(const void* pooled, int32_t ldp, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden,
                  void* logits, int32_t ldl, int32_t B, int32_t C, int32_t S, int32_t dtype, void* stream);
int vt_se_mlp_bwd(const void* dlogits, int32_t ldg, const void* pooled, int32_t ldp, const float* w1, const float* w2,
                  const float* hidden, float* dhidden, void* dpooled, int32_t lddp, float* dw1, float* db1, float* dw2, float* db2,
                  int32_t B, int32_t C, int32_t S, int32_t dtype, void* stream);
/* The same MLP with the squeeze activation given by code: `act` = 1 ReLU (exactly the two entry points above) or 3 SiLU
 * (EfficientNet).  SiLU's backward needs the pre-activation: with act = 3 `hidden` is f32 [2][B][S], the rounded hidden values
 * (the operand of dW2) followed by the f32 pre-activations W1 pooled + b1 (the operand of silu'). */
int vt_se_mlp_act_fwd(const void* pooled, int32_t ldp, const float* w1, const float* b1, const float* w2, const float* b2,
                      float* hidden, void* logits, int32_t ldl, int32_t B, int32_t C, int32_t S, int32_t act, int32_t dtype,
                      void* stream);
int vt_se_mlp_act_bwd(const void* dlogits, int32_t ldg, const void* pooled, int32_t ldp, const float* w1, const float* w2,
                      const float* hidden, float* dhidden, void* dpooled, int32_t lddp, float* dw1, float* db1, float* dw2,
                      float* db2, int32_t B, int32_t C, int32_t S, int32_t act, int32_t dtype, void* stream);

/* ---- what an EfficientNet block needs beyond the MobileNet kernels (vt_mbconv.hip) --------------------------------------
 * BatchNorm passes with a per-image keep factor -- stochastic depth in "row" mode, x + keep[b] * f(x), on the Conv ->
 * BatchNorm [-> act] unit that closes f.  z, r, y, dy, dz are [M][C] channel-last with row strides ld >= C, M = B * HW rows,
 * image b = m / HW; `keep` is a device float[B] of any values; `act` is an activation code 0 .. 6 of vt_bn_act_apply.
 *   vt_bn_keep_apply               y = keep[b] * act(z*scale + shift) + r (r may alias y).  Where keep[b] == 0 the rows of z
 *                                  are not read and y = r bit for bit
 *   vt_bn_keep_finalize_apply      the same with vt_bn_finalize inside the launch (the arguments of vt_bn_finalize_apply)
 *   vt_bn_keep_bwd_reduce          sums (the fixed-point buffer of vt_bn_act_bwd_reduce) += sum g, sum g * xhat with
 *                                  g = keep[b] * dy * act'(z*scale + shift); a dropped image's dy and z are not read
 *   vt_bn_keep_bwd_apply           dz = coef0*g - coef1*z + coef2 from the coefficients of vt_bn_bwd_finalize (coef0 is the
 *                                  scale); a dropped image's z IS read (dz = -coef1*z + coef2 under batch statistics)
 *   vt_bn_keep_bwd_finalize_apply  the same with vt_bn_bwd_finalize inside the launch
 * The three backward entries also take `add` (or NULL), a [M / HW][C] row of stride lda in the compute dtype: g = (keep[b] * dy +
 * add[b][c] / HW) * act'(.), the gradient of a per-image average pool of y joining d(y) in f32; with `add` given `keep` may be NULL
 * (factor 1), and a dropped image's z is read.
 * The residual's gradient is dy itself.  No float atomics: two runs of any launch are bit-identical.
 * Normalise + activation + per-image average pool in one pass (the Squeeze-Excitation pool over the expanded map):
 *   vt_bn_act_avgpool_apply           y = act(z*scale + shift), bit-identical to vt_bn_act_apply's, and pooled[b][c] = the
 *                                     mean over the HW rows of image b of y as stored (rounded to dtype): a [B][C] row of
 *                                     stride ldp in the compute dtype.  `scratch`: vt_bn_act_avgpool_scratch_bytes bytes,
 *                                     zeroed by the caller (0 bytes: may be NULL) -- where an image is cut into several row
 *                                     slabs their sums meet there in fixed point
 *   vt_bn_act_avgpool_finalize_apply  the same with vt_bn_finalize inside the launch */
int vt_bn_keep_apply(const void* z, int32_t ldz, const float* scale, const float* shift, const void* r, int32_t ldr, void* y,
                     int32_t ldy, const float* keep, int32_t HW, int64_t M, int32_t C, int32_t act, int32_t dtype, void* stream);
int vt_bn_keep_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* scale,
                              float* shift, float* mean, float* invstd, const void* z, int32_t ldz, const void* r, int32_t ldr,
                              void* y, int32_t ldy, const float* keep, int32_t HW, int64_t M, int32_t act, int32_t dtype,
                              void* stream);
int vt_bn_keep_bwd_reduce(const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* keep, const void* add, int32_t lda, int32_t HW,
                          int64_t M, int32_t C, int32_t act, int32_t dtype, float* sums, void* stream);
int vt_bn_keep_bwd_apply(const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* shift, const float* coef,
                         const float* keep, const void* add, int32_t lda, int32_t HW, void* dz, int32_t lddz, int64_t M, int32_t C,
                         int32_t act, int32_t dtype, void* stream);
int vt_bn_keep_bwd_finalize_apply(const float* sums, int32_t C, double count, double pscale, const float* scale, const float* shift,
                                  const float* mean, const float* invstd, int32_t train, float* dgamma, float* dbeta, float* coef,
                                  const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* keep, const void* add,
                                  int32_t lda, int32_t HW, void* dz, int32_t lddz, int64_t M, int32_t act, int32_t dtype,
                                  void* stream);
int64_t vt_bn_act_avgpool_scratch_bytes(int32_t B, int32_t HW, int32_t C, int32_t dtype); /* < 0: bad geometry */
int vt_bn_act_avgpool_apply(const void* z, int32_t ldz, const float* scale, const float* shift, void* y, int32_t ldy, void* pooled,
                            int32_t ldp, void* scratch, int32_t B, int32_t HW, int32_t C, int32_t act, int32_t dtype,
                            void* stream);
int vt_bn_act_avgpool_finalize_apply(const float* stats, int32_t C, double count, const float* gamma, const float* beta, float eps,
                                     float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                     float* scale, float* shift, float* mean, float* invstd, const void* z, int32_t ldz, void* y,
                                     int32_t ldy, void* pooled, int32_t ldp, void* scratch, int32_t B, int32_t HW, int32_t act,
                                     int32_t dtype, void* stream);

/* ---- tiled depthwise convolution of the MobileNet Conv-BN-act units (vt_dwtile.hip) -------------------------------------
 * k in {3, 5}, stride s in {1, 2}, padding (k - 1) / 2, dilation 1; C a multiple of 8 (bf16) / 4 (f32); any Hi, Wi >= 1 whose
 * one-row tile fits 64 KiB of LDS (Wi up to ~400 at k = 5); x, z, dz, dx channel-last with pixel strides ld >= C (channel
 * slices of wider buffers work); Ho = (Hi - 1) / s + 1.  The filter is the f32 master [C][k*k] of vt_dwconv_*, rounded for
 * bf16 launches as vt_dwconv_fwd rounds it.  Anything else: VT_ERR_UNSUPPORTED with the argument named.  A workgroup owns
 * (image, band of output rows, slab of channels) and stages its inputs with their halo in LDS once; no float atomics.
 *   vt_dwt_fwd           z = conv(x, w), f32 accumulation from 0 in ascending tap order: bit-identical to vt_dwconv_fwd on
 *                        the same operands.  `stats` (or NULL): the VT_CONV_STATS contract (fixed point, zeroed by the caller)
 *   vt_dwt_bwd           ONE launch: dx = conv_transpose(dz, w) [+ residual, which may alias dx; the sum is rounded to the
 *                        storage type first], every input pixel written; and the workgroup's filter-gradient share, f32
 *                        [k*k][slab channels], into shares[image][band][tap][c] (vt_dwt_shares_bytes; every element the
 *                        reducer reads is written)
 *   vt_dwt_wgrad_reduce  dw[c][t] += the shares of that element added in (image, band) order by one owner thread (the +=
 *                        contract of vt_dwconv_wgrad).  Takes the dtype of the vt_dwt_bwd launch: the band height, and with
 *                        it the share count, follows from the tile, which depends on the bytes per channel
 *   vt_dwt_tile          the tile all three use for a geometry: output rows per band, channels per slab */
int vt_dwt_fwd(const void* x, int32_t ldx, const float* w, void* z, int32_t ldz, float* stats, int32_t B, int32_t Hi, int32_t Wi,
               int32_t C, int32_t k, int32_t s, int32_t dtype, void* stream);
int vt_dwt_bwd(const void* dz, int32_t lddz, const void* x, int32_t ldx, const float* w, void* dx, int32_t lddx, const void* residual,
               int32_t ldr, float* shares, int64_t shares_bytes, int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t k, int32_t s,
               int32_t dtype, void* stream);
int vt_dwt_wgrad_reduce(const float* shares, int64_t shares_bytes, float* dw, int32_t B, int32_t Hi, int32_t Wi, int32_t C,
                        int32_t k, int32_t s, int32_t dtype, void* stream);
int64_t vt_dwt_shares_bytes(int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t k, int32_t s, int32_t dtype); /* < 0: refused */
int vt_dwt_tile(int32_t Hi, int32_t Wi, int32_t C, int32_t k, int32_t s, int32_t dtype, int32_t* rows_per_band,
                int32_t* channels_per_slab);

/* Backward of the stem unit Conv3x3(3 -> C, s1, pad 1) -> BatchNorm2d -> ReLU in one streaming pass
 * (darknet.py:75 `ConvNormAct(3, 32, 3, 1)`; autograd backward of components.py:26-44 with respect to the
 * conv weight and the BatchNorm parameters -- the unit's input is the image, no data gradient exists).
 * vt_stem_bn_bwd_reduce reads x [B*H*W][8] (3 real channels), dy and z ONCE and accumulates
 *   sums  (a statistics buffer, see VT_STAT_REPLICAS) as vt_bn_act_bwd_reduce, and
 *   gzx   vt_stem_bn_bwd_scratch_bytes(C) bytes: the correlations of g, z and 1 with the tap-shifted x, as f32
 *         (fixed = 0: f32 atomics, the first quarter of the buffer) or as fixed-point int64 pairs (fixed = 1: integer
 *         atomics, order-free -- the deterministic mode)
 * (both zeroed by the caller); after vt_bn_bwd_finalize, vt_stem_bn_bwd_combine (same `fixed`) adds
 *   dw[n][t][c] += coef0[n]*G - coef1[n]*Z + coef2[n]*X,  dw float[C][9][cin]
 * i.e. the filter gradient of dz = coef0*g - coef1*z + coef2 without forming dz.  bf16, C = 32 (the stems of the reference's models). */
int64_t vt_stem_bn_bwd_scratch_bytes(int32_t C);
int vt_stem_bn_bwd_reduce(int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, const void* x,
                          const void* dy, int32_t lddy, const void* z, int32_t ldz, const float* scale,
                          const float* shift, const float* mean, const float* invstd, int32_t relu,
                          float* sums, float* gzx, int32_t fixed, void* stream);
int vt_stem_bn_bwd_combine(int32_t C, int32_t cin, const float* gzx, const float* coef, float* dw,
                           int32_t fixed, void* stream);
/* `fixed` bit 1 of vt_stem_bn_bwd_reduce: `z` holds the unit's OUTPUT y = relu(z*scale + shift) (the pre-activation was
 * never stored: forward = a VT_CONV_STATS|VT_CONV_NOSTORE pass + a pass with the affine/ReLU epilogue).  The mask is
 * y > 0; the reduction then leaves `sums` entry 1 (sum g * xhat) ZERO, and vt_stem_bn_bwd_s2 fills it from the
 * correlations before vt_bn_bwd_finalize: z is linear in the 27 im2col patch values, so sum g*z = sum_i w[n][i] G[n][i]
 * exactly -- nothing is recovered from the rounded y.  The 32 z rows of gzx hold the correlations of the patch values
 * with the tap-shifted x instead; vt_stem_bn_bwd_combine_y then forms Z = W P with `w` the bf16 filter image [C][9][8]
 * the forward conv read, and adds dW like vt_stem_bn_bwd_combine.
 * Order: reduce(fixed | 2) -> s2 -> vt_bn_bwd_finalize -> combine_y. */
int vt_stem_bn_bwd_s2(int32_t C, const float* gzx, const void* w, const float* mean, const float* invstd, float* sums,
                      int32_t fixed, void* stream);
int vt_stem_bn_bwd_combine_y(int32_t C, int32_t cin, const float* gzx, const float* coef, const void* w, float* dw,
                             int32_t fixed, void* stream);

/* ---- pointwise (1x1) ConvNormAct unit without materialised pre-activations (vt_pointwise.hip) ---------------
 * A 1x1 `ConvNormAct` (components.py:26-44: nn.Conv2d(k=1, bias=False) -> nn.BatchNorm2d -> nn.ReLU) and its autograd
 * backward as four streaming passes that RECOMPUTE z = W x from the unit's input instead of storing z and dz:
 *   vt_pw_fwd_stats   x            -> batch statistics of z                       (then vt_bn_finalize)
 *   vt_pw_fwd_apply   x (+ res)    -> y = relu(z*scale + shift) (+ residual)
 *   vt_pw_bwd_reduce  dy, x        -> sums of g and g*xhat, g = dy*[y>0]          (then vt_bn_bwd_finalize)
 *   vt_pw_bwd_apply   dy, x (+add) -> dx = W^T dz (+ addend), dW += dz^T x, dz = coef0*g - coef1*z + coef2 in registers
 * z is rounded to bf16 where the unfused path stores it, so values agree with vt_conv_igemm + vt_bn_* to summation
 * order.  Up to two OUTPUT GROUPS share a launch -- CSPDarknetStage.conv1 / conv2 (darknet.py:46-47,53) read the same
 * tensor: one GEMM with N = C[0] + C[1] whose halves have their own filters, BatchNorm coefficients, statistics and
 * destinations.  bf16; K and every C[g] multiples of 32; vt_pw_supported() says whether a shape has a kernel:
 *   0 no;  2 yes;  1 yes, but the filter gradient does not fit the kernel's accumulators: vt_pw_bwd_apply then WRITES dz
 *   (pass `dz`) and the caller runs vt_conv_wgrad on it, `dw` must be NULL.
 * `coef` is float[4][N] = scale | shift | mean | invstd over all N = C[0] + C[1] channels (group 1 after group 0);
 * statistics / sums buffers and the vt_bn_bwd_finalize coefficients `bcoef` (float[3][C[g]]) are per group;
 * residual operands of vt_pw_fwd_apply: one for every group or none.
 * Arrays of per-group values have `ngroups` entries. */
typedef struct vt_pw_desc {
    int32_t dtype; /* VT_BF16 */
    int32_t K;     /* input channels */
    int32_t ngroups;
    int32_t relu;
    int64_t M;     /* pixels (B*H*W) */
    const void* x; /* [M][K], pixel stride ldx */
    int32_t ldx;
    int32_t C[2];       /* output channels per group */
    const void* w[2];   /* filters [C[g]][K], row stride ldw[g] */
    int32_t ldw[2];
    /* Producer fold (NULL / 0: none, the behaviour above).  `x` then holds the stored PRE-activation z0 of the training-mode
     * BatchNorm unit that produces this unit's input, `pcoef` is float[4][K] = scale | shift | mean | invstd of that
     * BatchNorm and `pact` its activation code (0 none, 1 ReLU): every pass applies y0 = act(z0*scale + shift), rounded to
     * bf16, to what it loads -- bit for bit the values vt_bn_act_apply / vt_bn_finalize_apply would have stored, so every
     * result equals that of the same call on the stored y0, which then need not exist.  Only shapes with
     * vt_pw_supported() == 2 (anything else: VT_ERR_UNSUPPORTED). */
    const float* pcoef;
    int32_t pact;
    /* vt_pw_bwd_apply[_finalize] with a producer operand and WITHOUT an addend (the call is then the only writer of
     * dx = d(y0)): also accumulate the producer's backward sums into this zeroed statistics buffer of K channels, as
     * vt_bn_act_bwd_reduce(dx, z0, pcoef rows, M, K, pact) would from the stored dx -- [0][c] += sum g, [1][c] += sum g*xhat,
     * g = dx * [y0 > 0] -- so that pass is not needed.  With an addend: VT_ERR_UNSUPPORTED.  NULL: not wanted. */
    float* psums;
} vt_pw_desc;
int vt_pw_supported(int32_t dtype, int32_t K, int32_t C0, int32_t C1);
/* the apply pass ALONE (inference: folded running statistics), one output group: additionally the 80-channel shapes of
 * YOLOv5x's first stage (80 -> 80, 160 -> 80), which are no multiples of 32 (darknet.py:124-133 at width 1.25) */
int vt_pw_apply_supported(int32_t dtype, int32_t K, int32_t C0);
int vt_pw_fwd_stats(const vt_pw_desc* d, float* const* stats, void* stream);
int vt_pw_fwd_apply(const vt_pw_desc* d, const float* coef, void* const* y, const int32_t* ldy,
                    const void* const* res, const int32_t* ldr, void* stream);
int vt_pw_bwd_reduce(const vt_pw_desc* d, const float* coef, const void* const* dy, const int32_t* lddy,
                     float* const* sums, void* stream);
int vt_pw_bwd_apply(const vt_pw_desc* d, const float* coef, const void* const* dy, const int32_t* lddy,
                    const float* const* bcoef, void* dx, int32_t lddx, const void* addend, int32_t ldadd,
                    float* const* dw, const int32_t* lddw, void* const* dz, const int32_t* lddz, void* stream);
/* The two apply passes with the BatchNorm finalize step of every group INSIDE them (round 6; as vt_bn_finalize_apply): a
 * workgroup stages the coefficients in LDS anyway, so every workgroup computes them itself from the complete sums of the pass
 * before, and workgroup 0 stores what the later passes read.  Same values bit for bit as
 *   vt_bn_finalize(fin[g].stats, C[g], fin[g].count, gamma, beta, eps, momentum, running_mean, running_var,
 *                  num_batches_tracked, coef + off_g, coef + N + off_g, coef + 2N + off_g, coef + 3N + off_g) per group, then
 *   vt_pw_fwd_apply(d, coef, ...)                                              (off_g = 0 | C[0], N = C[0] + C[1]);
 *   vt_bn_bwd_finalize(fin[g].sums, C[g], fin[g].count, fin[g].pscale, coef + off_g, coef + 2N + off_g, coef + 3N + off_g,
 *                      fin[g].train, fin[g].dgamma, fin[g].dbeta, bcoef[g]) per group, then vt_pw_bwd_apply(d, coef, ...).
 * Those calls run where N > 128 or with the knob VT_BN_FIN_APPLY = 0.  `fin` has ngroups entries. */
typedef struct vt_bn_fin_fwd {
    const float* stats; /* statistics buffer of the group (vt_pw_fwd_stats) */
    double count;
    const float *gamma, *beta; /* NULL: 1 / 0 */
    float eps, momentum;
    float *running_mean, *running_var; /* both or neither */
    int64_t* num_batches_tracked;      /* optional */
} vt_bn_fin_fwd;
typedef struct vt_bn_fin_bwd {
    const float* sums; /* sums buffer of the group (vt_pw_bwd_reduce) */
    double count, pscale;
    int32_t train;
    float *dgamma, *dbeta; /* optional, accumulated */
} vt_bn_fin_bwd;
int vt_pw_fwd_apply_finalize(const vt_pw_desc* d, const vt_bn_fin_fwd* fin, float* coef, void* const* y, const int32_t* ldy,
                             const void* const* res, const int32_t* ldr, void* stream);
int vt_pw_bwd_apply_finalize(const vt_pw_desc* d, const float* coef, const void* const* dy, const int32_t* lddy,
                             const vt_bn_fin_bwd* fin, float* const* bcoef, void* dx, int32_t lddx, const void* addend,
                             int32_t ldadd, float* const* dw, const int32_t* lddw, void* const* dz, const int32_t* lddz,
                             void* stream);
/* vt_pw_fwd_stats of a descriptor with a producer operand, with the PRODUCER's BatchNorm finalize step in its prologue: the
 * producer's statistics `pfin->stats` (K channels) are complete when this launch starts, so every workgroup computes
 * scale | shift for itself and workgroup 0 stores the four rows of d->pcoef (which the later passes read) and the running
 * statistics.  Same values bit for bit as vt_bn_finalize(pfin->stats, K, ...) into the rows of d->pcoef followed by
 * vt_pw_fwd_stats; those two calls run with the knob VT_BN_FIN_APPLY = 0. */
int vt_pw_fwd_stats_finalize(const vt_pw_desc* d, const vt_bn_fin_fwd* pfin, float* const* stats, void* stream);

/* ---- pooling ------------------------------------------------------------ */
/* The normalise pass fused with the MaxPool2d(3, 2, 1) that reads its output (VoVNet: `stage.max_pool` on the previous
 * stage's last ConvNormAct, vovnet.py:94 after components.py:36-44): writes y, the pooled map and the arg-max taps in one
 * pass over z; and the unit's BatchNorm-backward passes reading the POOLED gradient through the arg-max taps instead of
 * a materialised d(y) (only when the pool is y's sole consumer).  Same values as the separate calls. */
int vt_bn_act_apply_pool(const void* z, int32_t ldz, const float* scale, const float* shift, const void* residual,
                         int32_t ldr, void* y, int32_t ldy, void* pooled, int32_t ldp, uint8_t* argmax, int32_t B,
                         int32_t H, int32_t W, int32_t C, int32_t relu, int32_t dtype, void* stream);
int vt_bn_act_bwd_reduce_pool(const void* dp, int32_t lddp, const uint8_t* argmax, const void* z, int32_t ldz,
                              const float* scale, const float* shift, const float* mean, const float* invstd, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t relu, int32_t dtype, float* sums, void* stream);
int vt_bn_act_bwd_apply_pool(const void* dp, int32_t lddp, const uint8_t* argmax, const void* z, int32_t ldz,
                             const float* scale, const float* shift, const float* coef, void* dz, int32_t lddz, int32_t B,
                             int32_t H, int32_t W, int32_t C, int32_t relu, int32_t dtype, void* stream);

/* nn.MaxPool2d(3, 2, 1) at the head of every VoVNet stage (vovnet.py:94). */
int vt_maxpool3x3s2_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, uint8_t* argmax,
                        int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype,
                        void* stream);
int vt_maxpool3x3s2_bwd(const void* dy, int32_t lddy, const uint8_t* argmax, void* dx,
                        int32_t lddx, int32_t B, int32_t H, int32_t W, int32_t C,
                        int32_t accumulate, int32_t dtype, void* stream);
/* nn.AdaptiveAvgPool2d((1,1)) of the classifier head (classifier.py:61) and of
 * ESEBlock (vovnet.py:23). y is [B][C] with row stride ldy.  The sum over the pixels is 2^-32 fixed point (bit-identical
 * from run to run); a cell (b, c) whose pixels hold a NaN, an Inf or partial sums of 2^22 and more yields NaN, other cells
 * are not affected. */
int vt_global_avgpool_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t B,
                          int32_t HW, int32_t C, int32_t dtype, void* stream);
int vt_global_avgpool_bwd(const void* dy, int32_t lddy, void* dx, int32_t lddx, int32_t B,
                          int32_t HW, int32_t C, int32_t accumulate, int32_t dtype,
                          void* stream);

/* ---- nearest-neighbour resampling of the necks (necks.py:66, 70-81) -------- */
/* The `nn.Upsample(scale_factor=2.0 | 0.5, mode="nearest")` of FPN / PAN fused with the `sum`
 * that follows it (`aggregate_sum`, necks.py:19-23):
 *   mode 0 (top-down):  dst[b][i][j] = src[b][i/2][j/2] (+ other[b][i][j]);  src is [B][Hd/2][Wd/2][C]
 *   mode 1 (bottom-up): dst[b][i][j] = src[b][2i][2j]   (+ other[b][i][j]);  src is [B][2Hd][2Wd][C]
 * dst / other are [B][Hd][Wd][C]; `other` may be NULL.
 * Round 6: `mode="bilinear"` (align_corners False, what nn.Upsample computes):
 *   mode 2 (x2):   destination index d reads source coordinate d/2 - 1/4: taps (k-1, k) with weights (1/4, 3/4) for d = 2k,
 *                  (k, k+1) with (3/4, 1/4) for d = 2k+1, indices clamped to the map, rows and columns alike
 *   mode 3 (x0.5): dst[b][i][j] = mean of src[b][2i..2i+1][2j..2j+1] */
int vt_resample2x_add_fwd(const void* src, int32_t lds, const void* other, int32_t ldo, void* dst,
                          int32_t ldd, int32_t B, int32_t Hd, int32_t Wd, int32_t C, int32_t mode,
                          int32_t dtype, void* stream);
/* gradient w.r.t. src of the above (the `other` branch is the identity):
 *   mode 0: dsrc[b][i][j] (+)= sum of the 2x2 block dy[b][2i..2i+1][2j..2j+1]
 *   mode 1: dsrc[b][i][j] (+)= (i, j both even) ? dy[b][i/2][j/2] : 0
 *   mode 2 / 3: the transposes of the bilinear maps above (mode 3: a quarter of dy[b][i/2][j/2])
 * dy is [B][Hd][Wd][C]. */
int vt_resample2x_bwd(const void* dy, int32_t lddy, void* dsrc, int32_t lds, int32_t B, int32_t Hd,
                      int32_t Wd, int32_t C, int32_t mode, int32_t accumulate, int32_t dtype,
                      void* stream);

/* ---- BiFPN's weighted fusion node (necks.py:197-215) ---------------------- */
/* out = (sum_i relu(w)_i R_i(x_i)) / (sum_i relu(w)_i + eps) over n in {2, 3} inputs (x2 is ignored for n = 2).  out is
 * [B][H][W][C]; code_i says how input i relates to that grid: 0 same size, 1 nearest x2 (x_i is [B][H/2][W/2][C], read at
 * (i/2, j/2); H and W even), 2 nearest x0.5 (x_i is [B][2H][2W][C], read at (2i, 2j)) -- the index maps of
 * vt_resample2x_add_fwd modes 0 and 1.  `weights` is the RAW parameter, a device float[n]: the kernels apply the ReLU and
 * form 1 / (sum + eps) themselves.  f32 accumulation, one rounding at the store; out must not alias an input.  C is a
 * whole number of 16-byte chunks.
 * vt_wfuse_bwd, one launch per node, given g = d(out):
 *   dx_i (=|+= with acc_i) relu(w)_i / (sum + eps) * R_i^T(g): code 1 sums the 2x2 block of g; code 2 writes the
 *   even/even pixel and zeroes the other three (with acc_i nothing outside the even/even pixels is touched); a NULL dx_i
 *   skips that input;
 *   sums (VT_CHANNEL_SUMS_BYTES(1, n) bytes, zeroed by the caller): entry i += sum g * (R_i(x_i) - out), out recomputed in
 *   f32 from the inputs; fixed point, integer atomics, so every run is bit-identical.
 * vt_wfuse_finalize: dweights[i] += [w_i > 0] * sums_i / (sum + eps) -- BOTH scalar factors are applied here, in double;
 *   an entry whose weight is not positive is left untouched (torch: relu'(0) = 0). */
int vt_wfuse_fwd(int32_t n, const void* x0, int32_t ld0, int32_t code0, const void* x1, int32_t ld1, int32_t code1,
                 const void* x2, int32_t ld2, int32_t code2, const float* weights, float eps, void* out, int32_t ldo, int32_t B,
                 int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
int vt_wfuse_bwd(int32_t n, const void* g, int32_t ldg, const void* x0, int32_t ld0, int32_t code0, const void* x1, int32_t ld1,
                 int32_t code1, const void* x2, int32_t ld2, int32_t code2, const float* weights, float eps, void* dx0,
                 int32_t lddx0, int32_t acc0, void* dx1, int32_t lddx1, int32_t acc1, void* dx2, int32_t lddx2, int32_t acc2,
                 float* sums, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
int vt_wfuse_finalize(const float* sums, const float* weights, float eps, int32_t n, float* dweights, void* stream);

/* ---- SPPBlock: cascaded stride-1 pooling (components.py:139-152) ---------- */
/* p_1 = pool(x), p_s = pool(p_{s-1}), pool = MaxPool2d / AvgPool2d(k, 1, (k-1)/2); y = cat(p_1 .. p_repeats) over channels (x
 * itself is not part of it).  x is [B][H][W][C] with pixel stride ldx >= C, y is [B][H][W] with ldy >= repeats*C and stage s
 * (0-based) in channels [s*C, (s+1)*C); C is a whole number of 16-byte chunks.  Geometry (vt_spp_supported): k odd, 3 <= k <= 15
 * (a tap is one byte), repeats in 1..4, repeats*(k-1)/2 <= 8; any H, W >= 1.  Anything else returns VT_ERR_UNSUPPORTED.
 * vt_spp_fwd, ONE launch for all stages:
 *   pool 0 (max): positions outside the image never win; exact in the compute dtype.  With taps != NULL it also writes
 *     taps[repeats][B][H][W][C] (uint8, 16-byte aligned): the window tap dy*k + dx of the winner, the FIRST maximum of the
 *     clipped window in row-major order (torch's rule, which its backward sends the whole gradient to).
 *   pool 1 (avg): f32 sums times 1/k^2 with zeros outside the image at EVERY stage (count_include_pad); stage s+1 reads the
 *     stored (rounded) values of stage s.  taps is ignored.
 *   Inputs are finite by contract: what a NaN in x does is not specified.
 * vt_spp_bwd, ONE launch, gather form, no atomics, bit-identical runs: dy is the gradient of the whole y (lddy >=
 *   repeats*C); dx (=|+= with accumulate) the gradient of x; max needs the taps of the forward launch, avg ignores them. */
int vt_spp_supported(int32_t k, int32_t repeats);
int vt_spp_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, uint8_t* taps, int32_t B, int32_t H, int32_t W, int32_t C,
               int32_t k, int32_t repeats, int32_t pool, int32_t dtype, void* stream);
int vt_spp_bwd(const void* dy, int32_t lddy, const uint8_t* taps, void* dx, int32_t lddx, int32_t accumulate, int32_t B, int32_t H,
               int32_t W, int32_t C, int32_t k, int32_t repeats, int32_t pool, int32_t dtype, void* stream);

/* ---- DeformableConv2d: modulated deformable convolution (components.py:77-135) ---------- */
/* torchvision's deform_conv2d with one offset group and groups = 1, NHWC:
 *   y[b][ho][wo][co] = bias[co] + sum_{t = i*k + j} sum_ci w[co][t][ci] * m_t * bilinear(x[b], py, px)[ci]
 *   py = ho*stride - padding + i*dilation + offset[2t], px = wo*stride - padding + j*dilation + offset[2t + 1]
 * bilinear over floor and floor + 1; a corner outside [0, H-1] x [0, W-1] contributes zero; at an exactly integer position the
 * floor cell is used (d(offset) is the right-hand derivative).  m_t = mask_act(mask[t]): mask_act 0 identity, 1 sigmoid; mask
 * NULL: m = 1.  x is [B][H][W][Cin] (pixel stride ldx), y / dy [B][Ho][Wo][Cout], Ho = (H + 2 padding - dilation (k-1) - 1) /
 * stride + 1; offset [B][Ho][Wo] x 2k^2 (ldo >= 2k^2) and mask [B][Ho][Wo] x k^2 (ldm >= k^2) in the compute dtype: every map
 * may be a channel slice of a wider buffer; the offset / mask maps and their gradients need element alignment only.  w is the
 * filter image [Cout][k][k][Cin] in the compute dtype, bias f32 or NULL.  vt_deform_supported: k 1 or 3, stride 1 or 2, Cin
 * and Cout whole 16-byte chunks; anything else returns VT_ERR_UNSUPPORTED.  Positions, bilinear weights and the sigmoid are
 * f32 in both dtypes; bf16 products run on MFMA with the blended sample rounded once to bf16, f32 is an exact FMA chain.
 * vt_deform_fwd: ONE launch, no column matrix in memory.
 * vt_deform_bwd: doffset and dmask (ignored with mask NULL) are WRITTEN (their 2k^2 / k^2 channels only), each by the one wave
 *   that owns the pixel, in a fixed order: bit-identical runs.  dx != NULL: d(x) is scattered with f32 atomics into `plane`
 *   (f32 [B][H][W][Cin], cleared here) and a flush pass writes (accumulate 0) or adds (1) the rounded plane to dx: d(x) is the
 *   one output that is not bit-reproducible.  dx NULL: no scatter, plane ignored.
 * vt_deform_wgrad: dw[Cout][k][k][Cin] += dy^T col and, with dbias != NULL, dbias[Cout] += column sums of dy (f32): partial
 *   tiles per pixel slab in `scratch` (vt_deform_wgrad_scratch_bytes), then an ordered reducer inside the same call: no float
 *   atomics, bit-identical runs. */
int vt_deform_supported(int32_t k, int32_t stride, int32_t Cin, int32_t Cout, int32_t dtype);
int vt_deform_fwd(const void* x, int32_t ldx, const void* offset, int32_t ldo, const void* mask, int32_t ldm, const void* w,
                  const float* bias, void* y, int32_t ldy, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k,
                  int32_t stride, int32_t padding, int32_t dilation, int32_t mask_act, int32_t dtype, void* stream);
int vt_deform_bwd(const void* dy, int32_t lddy, const void* x, int32_t ldx, const void* offset, int32_t ldo, const void* mask,
                  int32_t ldm, const void* w, void* doffset, int32_t lddo, void* dmask, int32_t lddm, void* dx, int32_t lddx,
                  int32_t accumulate, float* plane, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k,
                  int32_t stride, int32_t padding, int32_t dilation, int32_t mask_act, int32_t dtype, void* stream);
int64_t vt_deform_wgrad_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k, int32_t stride,
                                      int32_t padding, int32_t dilation);
int vt_deform_wgrad(const void* dy, int32_t lddy, const void* x, int32_t ldx, const void* offset, int32_t ldo, const void* mask,
                    int32_t ldm, float* dw, float* dbias, void* scratch, int64_t scratch_bytes, int32_t B, int32_t H, int32_t W,
                    int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t padding, int32_t dilation, int32_t mask_act,
                    int32_t dtype, void* stream);

/* ---- Input pipeline: crop-resize-flip-erase from uint8 (reference data.py) ---------- */
/* ONE launch turns a ragged batch of decoded uint8 HWC images into out[B][3][S_h][S_w] (f32, NCHW, the trainer's input batch).
 * Every pointer is a device pointer; the geometry is read from the tables by the kernel, the grid depends on (B, S_h, S_w) only.
 *   raw     all images packed, each [H][W][3] uint8
 *   table   int64 [B][3] = (byte offset of the image in raw, H, W); trusted: it says where the images are.  H, W <= 2^20.
 *           A row with H < 1, W < 1 or a negative offset names no image: nothing is read for it and its output is all zeros.
 *   params  int32 [B][16] = top, left, h, w, OH, OW, oy, ox, flip, ei, ej, eh, ew, erase mode, seed, constant (f32 bits)
 * Per image: the crop box (top, left, h, w) is resized to a virtual (OH, OW) image and the (S_h, S_w) window at (oy, ox) of it is
 * produced (training: OH, OW = S_h, S_w and oy = ox = 0; validation: the whole image to the Resize size, the window is the
 * centre crop).  The filter is torch's F.interpolate(mode="bilinear", antialias = antialias != 0, align_corners=False): along an
 * axis of n source and `out` virtual pixels, with s = n / out, support = max(s, 1) (antialias) or 1, c = s (i + 0.5), the taps
 * of output i are j in [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n)) with weight max(0, 1 - |j + 0.5 - c| /
 * support) over the sum of the weights; separable, never leaving the crop box, no rounding to 8 bits in between.  Then: flip
 * != 0 mirrors the columns of the window; the value is multiplied by 1/255; with mean_std != NULL (f32 [6] = mean[3], std[3])
 * it becomes (v - mean[c]) / std[c]; last, with erase mode 1 or 2 and eh > 0, the box rows [ei, ei + eh) x columns [ej, ej + ew)
 * of the OUTPUT is overwritten with the constant (mode 1) or with standard-normal values (mode 2) of the counter-based generator
 *   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16            (uint32)
 *   k = mix(seed + 0x9e3779b9); k = mix(k + b); k = mix(k + c); k = mix(k + y); k = mix(k + x)     (output coordinates)
 *   h1 = mix(k ^ 0x68bc21eb), h2 = mix(k ^ 0x02e5be93); u1 = ((h1 >> 8) + 1) / 2^24, u2 = (h2 >> 8) / 2^24
 *   z = sqrtf(-2 logf(u1)) * cosf(6.2831855f * u2)                                                  (accurate f32 functions)
 * which is part of the interface: the same (seed, b) gives the same values in every run.
 * Whatever params holds is clamped into its image before it forms an address (a bad box cannot read outside its image); what
 * such a box produces is not specified.  No atomics, a fixed summation order: repeated launches are bit-identical.
 * lds_bytes caps the LDS plan (tables + the plane of horizontally filtered source rows); 0: the default (64 KiB); values above
 * 160 KiB mean 160 KiB.  A band that needs more source rows than the plane holds runs in chunks, with the same bits.
 * VT_ERR_INVALID: a null raw / table / params / out, B, S_h or S_w <= 0, a misaligned table, lds_bytes < 0 or too small for the
 * tables and one source row. */
int vt_augment_batch(const uint8_t* raw, const int64_t* table, const int32_t* params, float* out, int32_t B, int32_t S_h,
                     int32_t S_w, int32_t antialias, const float* mean_std, int32_t lds_bytes, void* stream);

/* ---- Input pipeline: TrivialAugmentWide on 8-bit levels (reference data.py:44-52, its third stage) ---------- */
/* With TrivialAugmentWide the image between resize / flip and ToTensor is 8-bit, as in the reference.  Two calls:
 *
 * vt_augment_batch_u8: the arguments of vt_augment_batch without mean_std, the SAME kernel body with another epilogue.  The
 *   filtered value of vt_augment_batch on the 0 .. 255 scale, before the 1/255, is rounded half up (floorf(v + 0.5f), the
 *   product rounded before the sum) and clamped to 0 .. 255: out is uint8 [B][S_h][S_w][3], the LEVELS.  No mean / std, no
 *   erase (the erase fields of params are ignored).  A table row that names no image gives zeros.  out needs no alignment.
 *
 * vt_trivial_augment: u8 = those levels, ta = f64 [B][8] = (op, m0..m5, arg) per image, params = the table of
 *   vt_augment_batch (only its erase fields ei, ej, eh, ew, mode, seed, constant are read), out f32 [B][3][S_h][S_w],
 *   workspace u32 [B][4][256] (the three channel histograms and the gray histogram; cleared inside the call).  Per image the
 *   op is applied to the levels, then out = float32(level) * (1.0f / 255.0f), then mean / std and the erase exactly as in
 *   vt_augment_batch (same fields, same generator).  The ops, torchvision's TrivialAugmentWide order, with `a` the levels of
 *   an image, H = S_h, W = S_w, and every result the level PIL 12 computes on an 8-bit RGB image:
 *     0 Identity.
 *     1 ShearX, 2 ShearY, 3 TranslateX, 4 TranslateY, 5 Rotate: PIL's Image.transform(AFFINE, (m0..m5), BILINEAR), fill 0.
 *       For output pixel (x, y), in f64 with every product and sum rounded on its own (no FMA), left to right:
 *         xin = m0 (x + .5) + m1 (y + .5) + m2,  yin = m3 (x + .5) + m4 (y + .5) + m5;
 *         0 unless 0 <= xin < W and 0 <= yin < H;  xin -= .5, yin -= .5;  x0 = floor(xin), dx = xin - x0 (likewise y);
 *         the neighbours (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) with their indices clamped into the image;
 *         v1 = p00 + (p01 - p00) dx, v2 = p10 + (p11 - p10) dx, v = v1 + (v2 - v1) dy, truncated.
 *       The matrix (output -> input) is the host's: torchvision's inverse affine matrix, or PIL's Image.rotate matrix.
 *     6 Brightness, 7 Color, 8 Contrast, 9 Sharpness: blend(deg, a, f) with f = float32(arg):
 *         t = f32(deg) + f * (f32(a) - f32(deg)) (a product, then a sum);  0 if t <= 0, 255 if t >= 255, else t truncated.
 *       gray g = (19595 R + 38470 G + 7471 B + 32768) >> 16.  Brightness: deg = 0.  Color: deg = g on all three channels.
 *       Contrast: deg = int(mean of g over the image (f64: the integer sum over H W) + 0.5).  Sharpness: deg = PIL's SMOOTH,
 *       floor((sum of the 3 x 3 + 4 centre) / 13 + 0.5) inside, the first and last row and column copied.
 *     10 Posterize: a & (256 - (1 << (8 - k))), k = arg.      11 Solarize: a if a < arg (f64) else 255 - a.
 *     12 AutoContrast, per channel: lo, hi = the lowest and highest level present; identity if hi <= lo; else in f64
 *         scale = 255 / (hi - lo), offset = -lo scale, lut[i] = clamp(int(i scale + offset), 0, 255).
 *     13 Equalize, per channel with histogram h: identity if at most one bin is non-zero; step = (H W - h[highest non-zero
 *         bin]) / 255 (integer); identity if 0; n = step / 2; for i in 0 .. 255: lut[i] = min(n / step, 255), n += h[i].
 *   The histograms are built with integer atomics only (no float atomics anywhere): repeated launches are bit-identical.
 *   The op differs per image inside one launch; any S_h x S_w with S_h S_w < 2^31 runs (no image has to fit in LDS).
 *   ta ON THE DEVICE IS NOT VALIDATED: an op that is not a number in [0, 14) is Identity (NaN included), a fractional op is
 *   truncated; Posterize's k is truncated and clamped into 1 .. 8 (NaN: 1); a matrix with NaNs or huge coefficients fills
 *   with 0 wherever the coordinate tests fail; a factor or threshold that is not a number gives unspecified levels.  No
 *   value of ta or params forms an address outside u8, workspace or out.
 *   VT_ERR_INVALID: a null u8 / ta / params / out / workspace, B, S_h or S_w <= 0, S_h S_w >= 2^31, a misaligned ta (8),
 *   params, out, workspace or mean_std (4). */
int vt_augment_batch_u8(const uint8_t* raw, const int64_t* table, const int32_t* params, uint8_t* out, int32_t B, int32_t S_h,
                        int32_t S_w, int32_t antialias, int32_t lds_bytes, void* stream);
int vt_trivial_augment(const uint8_t* u8, const double* ta, const int32_t* params, float* out, uint32_t* workspace, int32_t B,
                       int32_t S_h, int32_t S_w, const float* mean_std, void* stream);

/* ---- Input pipeline: baseline JPEG decoding (reference classifier.py:22-25, image_loader) ---------- */
/* Two launches turn the compressed files of a batch into the packed uint8 HWC images (`raw` of vt_augment_batch):
 *   vt_jpeg_entropy   Huffman-decodes every entropy segment into the coefficient scratch, one wave per segment;
 *   vt_jpeg_idct_rgb  dequantises, runs libjpeg's accurate integer IDCT, the "fancy" chroma upsampling and the 16-bit
 *                     fixed-point YCbCr -> RGB conversion, and writes the pixels.
 * The result is the level libjpeg's default decode gives (PIL's Image.open(...).convert("RGB")), integer arithmetic throughout.
 * As in libjpeg, a chroma plane is filtered only if it is more than two samples wide (ceil(W / 2) > 2) and replicated otherwise.
 * The IDCT forms its sums and products modulo 2^32: jidctint on the coefficients of any real image, and a defined function (no
 * signed overflow) of whatever a damaged stream leaves in the scratch.
 * Scope: baseline sequential DCT (SOF0, SOF1 with 8-bit tables), 8-bit samples, Huffman coding, ONE interleaved scan of 1 or 3
 * components, sampling 4:4:4, 4:2:2 (2x1) or 4:2:0 (2x2) with the chroma components at 1x1; any W, H >= 1; restart intervals
 * of any length.  The HOST parses the markers, refuses everything else and builds the tables; every pointer below is a device
 * pointer, and all geometry is read from the tables by the kernels.
 *
 *   data      the bytes of all files, packed.
 *   images    int64 [B][VT_JPEG_IMG_FIELDS]:
 *               0 H   1 W   2 components (1 or 3)   3 h_max (1 or 2)   4 v_max (1 or 2)   5 MCUs per row   6 MCU rows
 *               7, 8, 9     quantisation table index of component 0, 1, 2
 *               10 .. 15    Huffman table index: DC0, AC0, DC1, AC1, DC2, AC2
 *               16 first block of the image in the coefficient scratch   17 byte offset of the image in raw
 *               18 first row of the image in `segments`   19 its segment count   20 restart interval in MCUs (0: none)
 *               21 .. 23    unused (0)
 *             A gray image uses the entries of component 0 only; its MCU is one block.  An MCU of a colour image is h_max x
 *             v_max luma blocks (rows of blocks, left to right) followed by one Cb and one Cr block.
 *   segments  int64 [S][VT_JPEG_SEG_FIELDS] = image, first byte in data, one past the last byte, first MCU, MCU count, 0.
 *             A segment is the entropy-coded data between two markers of the scan; the markers themselves are outside it.
 *   qtabs     uint8 [NQ][64]: quantisation tables in NATURAL (row-major) order, de-duplicated over the batch.
 *   hufftabs  uint8 [NH][VT_JPEG_HUFF_BYTES]: T.81's BITS (16 bytes) then HUFFVAL (256 bytes, zero padded), de-duplicated.
 *   coef      int16 [blocks][64], 16-byte aligned: per image, component after component (Y, Cb, Cr), each a raster of
 *             (MCUs per row x h_c) x (MCU rows x v_c) blocks; a block is 64 coefficients in natural order, the DC prediction
 *             resolved.  vt_jpeg_scratch_bytes(blocks) is its size.  EVERY coefficient of every block that a segment names
 *             is written (zeros included), so the scratch needs no clearing.
 *   status    int32 [S], one entry per SEGMENT, always written: 0 clean, 1 a bit pattern that is no code of its table (or a
 *             DC size above 15), 2 a zero run that passes coefficient 63, 3 the blocks needed bits past the end of the segment
 *             (or past a marker inside it; such reads yield zero bits, as libjpeg pads), 4 a row of `segments` / `images`
 *             that is out of range (nothing but the status is written for such a segment) or a Huffman table that
 *             over-subscribes its code space (all blocks of the segment are written as zeros), 5 all blocks decoded but 8 or
 *             more bits of the segment were left over.  On 1, 2 and 3 the block in which it happened and all later blocks of
 *             the segment are written as zeros.  An image's status is the largest of its segments'.
 *   raw       uint8, the output: image b is [H][W][3] at its byte offset; no alignment is needed.
 * UNTRUSTED BYTES.  `data` may hold anything.  A byte is read only inside its segment's [begin, end), itself checked against
 * data_bytes; the number of symbols a wave decodes is at most 64 per block and its blocks are MCU count x blocks per MCU, both
 * known before the loop starts; block indices are re-checked against coef_blocks and pixel addresses against raw_bytes on
 * entry, and a row that fails writes nothing.  `images` / `segments` come from the host and are checked all the same.
 * No atomics; repeated launches are bit-identical.  The result does not depend on band_mcu_rows.
 *   band_mcu_rows  MCU rows a workgroup of vt_jpeg_idct_rgb owns: 0 (the default, 4) or 1 .. 4.
 *   max_mcus_x/y   the largest fields 5 / 6 of the batch (they size the grid; an image with more is cut off there).
 * VT_ERR_INVALID: a null pointer, B / S / NQ / NH / blocks / bytes <= 0, a misaligned table (8), status (4) or coef (16),
 * band_mcu_rows outside 0 .. 4, max_mcus_x / max_mcus_y < 1 or a grid beyond 2^31 workgroups (B > 65535). */
#define VT_JPEG_IMG_FIELDS 24
#define VT_JPEG_SEG_FIELDS 6
#define VT_JPEG_HUFF_BYTES 272
int64_t vt_jpeg_scratch_bytes(int64_t blocks);
int vt_jpeg_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* images, int32_t B, const int64_t* segments,
                    int32_t S, const uint8_t* hufftabs, int32_t NH, int16_t* coef, int64_t coef_blocks, int32_t* status,
                    void* stream);
int vt_jpeg_idct_rgb(const int16_t* coef, int64_t coef_blocks, const int64_t* images, int32_t B, const uint8_t* qtabs,
                     int32_t NQ, uint8_t* raw, int64_t raw_bytes, int32_t max_mcus_x, int32_t max_mcus_y,
                     int32_t band_mcu_rows, void* stream);

/* ---- ESEBlock gate (vovnet.py:20-28) ------------------------------------ */
/* y = x * hardsigmoid(s[b][c]) [+ residual]; s is [B][C] (the biased 1x1 conv
 * of the pooled map, computed with vt_conv_igemm). */
int vt_ese_gate_fwd(const void* x, int32_t ldx, const void* s, int32_t lds,
                    const void* residual, int32_t ldr, void* y, int32_t ldy, int32_t B,
                    int32_t HW, int32_t C, int32_t dtype, void* stream);
/* dx (=|+=) dy*hsig(s);  ds[b][c] = hsig'(s) * sum_hw dy*x  (f32 [B][C]; the sum as in vt_global_avgpool_fwd: NaN for a
 * cell with a non-finite or out-of-range (2^22) partial sum) */
int vt_ese_gate_bwd(const void* dy, int32_t lddy, const void* x, int32_t ldx, const void* s,
                    int32_t lds, void* dx, int32_t lddx, float* ds, int32_t B, int32_t HW,
                    int32_t C, int32_t accumulate, int32_t dtype, void* stream);

/* ---- classifier head / loss (classifier.py:58-64, 92) ------------------- */
/* per-column sums of a [M][C] matrix into out[C] (+=): bias gradients. */
int vt_colsum(const void* a, int32_t lda, int64_t M, int32_t C, int32_t dtype, float* out,
              void* stream);
/* the same sums into a zeroed fixed-point buffer q = int64[C][2] (deterministic mode; vt_fixed_to_f32 folds it in) */
int vt_colsum_fixed(const void* a, int32_t lda, int64_t M, int32_t C, int32_t dtype, void* q, void* stream);
/* F.cross_entropy(logits, labels, label_smoothing) with mean reduction and its
 * gradient times grad_scale; loss_sum[0] += sum_b loss_b / B. */
int vt_softmax_xent(const void* logits, int32_t ldl, const int64_t* labels,
                    float label_smoothing, float grad_scale, float* loss, void* dlogits,
                    int32_t lddl, int32_t B, int32_t N, int32_t dtype, void* stream);

/* MixUp / CutMix of the training step (classifier.py:86-87, extras.py:14-109), on device.
 * `mix` is a device float[8] the host refreshes per step (so captured graphs stay valid):
 *   mix[0] mode: 0 none, 1 mixup, 2 cutmix;  mix[1] lambda (for cutmix: 1 - box area / image area,
 *   extras.py:88);  mix[2..5] = x1, y1, x2, y2 of the cutmix box (extras.py:81-84).
 * The partner of sample b is sample b-1 (mod B): `batch.roll(1, 0)`, extras.py:34,69.
 * vt_softmax_xent_mix: loss / gradient against the soft target
 *   lambda * onehot(labels[b]) + (1 - lambda) * onehot(labels[b-1]), then label smoothing --
 *   what F.cross_entropy(logits, mixed_onehot, label_smoothing) computes (classifier.py:92).
 * vt_mix_nchw_to_nhwc: vt_nchw_to_nhwc of the mixed images (mixup: lambda*x[b] + (1-lambda)*x[b-1];
 *   cutmix: x[b-1] inside the box, x[b] outside). */
int vt_softmax_xent_mix(const void* logits, int32_t ldl, const int64_t* labels,
                        float label_smoothing, float grad_scale, float* loss, void* dlogits,
                        int32_t lddl, int32_t B, int32_t N, int32_t dtype, const float* mix,
                        void* stream);
/* Validation step (classifier.py:97-109): out3[0] += sum of the rows' cross entropy WITHOUT label smoothing, out3[1] +=
 * rows whose arg-max (first maximum, as torch.argmax) equals the label, out3[2] += rows.  The caller zeroes out3 or keeps
 * accumulating over an epoch's batches; data parallel it all-reduces the three sums (`sync_dist=True`, classifier.py:104). */
int vt_softmax_xent_eval(const void* logits, int32_t ldl, const int64_t* labels, float* out3, int32_t B, int32_t N,
                         int32_t dtype, void* stream);
int vt_mix_nchw_to_nhwc(const float* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W,
                        int32_t Cpad, int32_t dtype, const float* mix, void* stream);

/* Binary cross-entropy of the training step (loss="bce"): the loss of the "ResNet strikes back" and DeiT III recipes, in the
 * form of timm.loss.BinaryCrossEntropy behind timm's Mixup.  timm is no dependency; THIS statement is the definition.
 * For B rows, N classes, logits x, labels y and the `mix` block above (NULL or mode 0: lam = 1, no partner is read):
 *   mixed one-hot  m[b][c] = lam * [c == y_b] + (1 - lam) * [c == y_{(b-1) mod B}]     (equal labels: the two terms add)
 *   smoothing      t = (1 - s) * m + s / N                                               (s = label_smoothing)
 *   threshold      with VT_BCE_THRESHOLD:  t = (t > target_threshold) ? 1 : 0
 *   element loss   l = max(x, 0) - x * t + log1p(exp(-|x|))       (= F.binary_cross_entropy_with_logits(x, t, "none"))
 *   batch loss     loss[0] += sum_b sum_c l / D,   D = B * N (a mean over elements), or D = B with VT_BCE_SUM_CLASSES
 *   gradient       dlogits = (sigmoid(x) - t) * grad_scale * (VT_BCE_SUM_CLASSES ? 1 : 1 / N)      (NULL: loss only)
 * A label outside [0, N) makes the loss NaN; a label is compared with column indices and never forms an address.  Only
 * columns [0, N) of a row of dlogits are written.  Every finite logit gives finite results.
 * `rows` is scratch of B doubles (8-byte aligned): the first launch stores each row's sum of l there, one workgroup per
 * row; a second one-workgroup launch adds rows[0], rows[1], .. in that order in double.  No float atomic: the loss is a
 * fixed-order sum, the same bits on every run (vt_softmax_xent's is not). */
#define VT_BCE_SUM_CLASSES 1
#define VT_BCE_THRESHOLD 2
int vt_sigmoid_bce(const void* logits, int32_t ldl, const int64_t* labels, float label_smoothing, float grad_scale,
                   float* loss, void* dlogits, int32_t lddl, int32_t B, int32_t N, int32_t dtype, const float* mix,
                   int32_t flags, float target_threshold, double* rows, void* stream);

/* ---- optimiser (classifier.py:161-169: torch.optim.SGD, momentum) -------- */
/* g' = g*grad_scale + wd*p; m = mu*m + g'; p -= lr*m; mirror = cast(p).
 * lr_dev (optional, device float[1]) overrides `lr`, so a captured graph can
 * follow the warm-up/cosine schedule (classifier.py:171-190) without re-capture. */
int vt_sgd_momentum(float* p, const float* g, float* m, void* mirror, int32_t mirror_dtype,
                    int64_t n, float lr, float momentum, float weight_decay,
                    float grad_scale, const float* lr_dev, void* stream);
/* torch.optim.AdamW (decoupled != 0) / torch.optim.Adam (decoupled == 0), single tensor, amsgrad = False, over the same
 * flat buffers plus the second moment v; g' = g*grad_scale:
 *   AdamW: p *= 1 - lr*wd            Adam: g' += wd*p
 *   m = beta1*m + (1-beta1)*g';  v = beta2*v + (1-beta2)*g'*g'
 *   p -= (lr / (1-beta1^t)) * m / (sqrt(v) / sqrt(1-beta2^t) + eps);  mirror = cast(p)
 * `hyper` (required, device float[8], 16-byte aligned like every buffer here): [0] the learning rate, [4] the step
 * count t as an int32, [5] 1-beta1^t, [6] sqrt(1-beta2^t).  vt_adam_tick advances t by one and refreshes [5] and [6]
 * (in double, one thread); it runs ONCE per step in front of that step's vt_adamw launches, which only read the
 * three values -- so every segment of a step sees the same t, and a replayed hipGraph counts by itself.  The betas
 * are doubles because 1-beta is rounded to f32 from the double value, as torch does. */
int vt_adam_tick(float* hyper, double beta1, double beta2, void* stream);
int vt_adamw(float* p, const float* g, float* m, float* v, void* mirror, int32_t mirror_dtype,
             int64_t n, double beta1, double beta2, float eps, float weight_decay,
             float grad_scale, int32_t decoupled, const float* hyper, void* stream);

/* ---- gradient norm, clipping, LAMB ----------------------------------------------------------------------------------
 * Notation: g the flat gradient as backward left it, s = grad_scale (1 / world), N = s * sqrt(sum g^2) the norm of the
 * averaged gradient; t, bc1 = 1 - beta1^t, sqrt(bc2) = sqrt(1 - beta2^t) as vt_adam_tick keeps them in `hyper`.
 *
 * A flat buffer is reduced in ITEMS of VT_OPT_ITEM elements: a workgroup turns an item into one double, written with a
 * plain store, so no sum depends on the grid or the CU count and none uses a float atomic; results are bit-identical
 * from run to run.  Whoever needs a total adds the partials of an earlier launch, in index order per lane and a fixed
 * tree over the lanes, in double.
 *
 * vt_grad_sumsq:  partials[i] = sum of g^2 over item i, i < VT_OPT_ITEMS(n).  16-byte loads; any n > 0.
 * vt_clip_coef:   one workgroup.  ctl is a device float[8] (16-byte aligned):
 *     ctl[VT_CTL_CLIP]     C, the trainer-level threshold    (in)   a value <= 0, infinite or NaN means "off"
 *     ctl[VT_CTL_LAMB_MAX] M, LAMB's max_grad_norm           (in)   likewise
 *     ctl[VT_CTL_FACTOR]   s * c1 / c2                       (out)  what every consumer below multiplies g by
 *     ctl[VT_CTL_NORM]     N                                 (out)
 *   c1 = min(1, C / (N + 1e-6)) -- torch.nn.utils.clip_grad_norm_, i.e. Lightning's gradient_clip_val with the "norm"
 *   algorithm; a NaN N gives a NaN c1, as torch does.  LAMB's own clip sees the clipped gradient: N' = c1 * N,
 *   c2 = N' / M if N' > M else 1 (a false comparison, NaN included, gives 1).  Both off: the factor is exactly s.
 * vt_sgd_momentum_clip / vt_adamw_clip: vt_sgd_momentum / vt_adamw with the device scalar coef[0] in the place of the
 *   immediate grad_scale (coef = ctl + VT_CTL_FACTOR), same kernel bodies.
 *
 * LAMB, in the form of timm.optim.Lamb(bias_correction=True, grad_averaging=True).  timm is not a dependency and was
 * not at hand: the form below was written down from memory of timm/optim/lamb.py and IS the definition for this
 * library.  Per element, with g' = coef[0] * g:
 *     m = beta1*m + (1-beta1)*g';   v = beta2*v + (1-beta2)*g'^2
 *     u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd*p
 * per parameter tensor, if wd != 0 or VT_LAMB_ALWAYS_ADAPT:  r = ||p|| / ||u|| where both norms are > 0, else 1;
 * r = min(r, 1) with VT_LAMB_TRUST_CLIP; otherwise r = 1.  Then p -= lr * r * u and mirror = cast(p).
 * (timm's default eps is 1e-6, not torch.optim.Adam's 1e-8.)
 *
 * The tensors come from a device table the host builds once: int32[n_segs][4] = (element offset, elements, first item,
 * weight decay as float bits), followed by int32[n_items] = the segment of each item; 16-byte aligned.  Offsets and
 * lengths are multiples of 64 (the flat store's slots), a segment of n elements owns VT_OPT_ITEMS(n) consecutive
 * items, so an item never straddles two tensors.  The kernels check every entry against n_total, the length of the
 * flat buffers, before they address anything with it; an unusable entry gets NaN partials and no update.
 * vt_lamb_moments: reads p g m v, writes m v and partials[2*i], partials[2*i + 1] = sum p^2, sum u^2 of item i.
 * vt_lamb_apply:   re-forms u from the new m, v and the unchanged p (the same inline function), adds the tensor's
 *   partials in its prologue (every workgroup for itself), applies r, writes p and the mirror.  g is left alone.
 * 42 bytes of traffic per parameter with a bf16 mirror (vt_adamw: 30).
 * VT_ERR_INVALID: a null or misaligned p / g / m / v / table / partials, a null hyper / coef / ctl, counts <= 0. */
#define VT_OPT_ITEM 4096
#define VT_OPT_ITEMS(n) (((n) + VT_OPT_ITEM - 1) / VT_OPT_ITEM)
#define VT_CTL_CLIP 0
#define VT_CTL_LAMB_MAX 1
#define VT_CTL_FACTOR 2
#define VT_CTL_NORM 3
#define VT_LAMB_TRUST_CLIP 1
#define VT_LAMB_ALWAYS_ADAPT 2
int32_t vt_opt_item(void); /* VT_OPT_ITEM of the built library */
int vt_grad_sumsq(const float* g, int64_t n, double* partials, void* stream);
int vt_clip_coef(const double* partials, int64_t n_items, float grad_scale, float* ctl, void* stream);
int vt_sgd_momentum_clip(float* p, const float* g, float* m, void* mirror, int32_t mirror_dtype, int64_t n, float lr,
                         float momentum, float weight_decay, const float* coef, const float* lr_dev, void* stream);
int vt_adamw_clip(float* p, const float* g, float* m, float* v, void* mirror, int32_t mirror_dtype, int64_t n,
                  double beta1, double beta2, float eps, float weight_decay, const float* coef, int32_t decoupled,
                  const float* hyper, void* stream);
int vt_lamb_moments(const float* p, const float* g, float* m, float* v, const int32_t* table, int32_t n_segs,
                    int64_t n_items, int64_t n_total, double* partials, const float* coef, double beta1, double beta2,
                    float eps, int32_t flags, const float* hyper, void* stream);
int vt_lamb_apply(float* p, const float* m, const float* v, void* mirror, int32_t mirror_dtype, const int32_t* table,
                  int32_t n_segs, int64_t n_items, int64_t n_total, const double* partials, float eps, int32_t flags,
                  const float* hyper, void* stream);

/* ---- exponential moving average of the weights ------------------------------------------------------------------------
 * The shadow copy e of a flat f32 buffer p that torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d),
 * use_buffers=True) (torchvision's ExponentialMovingAverage) and timm.utils.ModelEmaV2 keep.  Neither package is a
 * dependency; the statement below is the definition for this library.
 *
 * Optimiser steps are numbered s = 0, 1, 2, ..; updates of the average are numbered u = 0, 1, 2, ..  With the period k
 * (torchvision's --model-ema-steps; 1 = every step) step s updates the average iff s % k == 0, as the reference loop's
 * `if i % model_ema_steps == 0` does.  Update 0 is a copy, every later one a blend:
 *     u == 0:  e <- p
 *     u >= 1:  e <- e + alpha * (p - e)          one subtraction, one fused multiply-add, both in f32
 * alpha = 1 - decay is formed in DOUBLE on the host and handed over as an f32; the decay itself never exists as an f32
 * (for decay = 0.99998, rounding the decay to f32 first moves alpha by 3e-3 of its value).  On a step that does not
 * update, e keeps its bits.  Floating-point buffers (parameters, BatchNorm running statistics) are averaged; integer
 * buffers (num_batches_tracked) are copied on the steps that update.
 *
 * ctl is a device buffer of 8 four-byte words, 16-byte aligned:
 *     ctl[VT_EMA_ALPHA]   float  alpha                                  (in)
 *     ctl[VT_EMA_MODE]    int32  VT_EMA_SKIP / _COPY / _BLEND           (out of vt_ema_tick, in of the others)
 *     ctl[VT_EMA_COUNT]   int32  updates made so far, u                 (in / out of vt_ema_tick)
 *     ctl[VT_EMA_PERIOD]  int32  k; a value < 1 counts as 1             (in)
 *     ctl[VT_EMA_STEP]    int32  optimiser steps seen so far, s         (in / out of vt_ema_tick)
 * vt_ema_tick:   one thread.  Leaves this step's mode, then advances s (and u where the step updates).  It runs ONCE per
 *   optimiser step in front of that step's vt_ema_update / vt_ema_copy launches, which only read the mode and alpha: the
 *   launch list is the same on every step, and a replayed hipGraph counts by itself.
 * vt_ema_update: one streaming pass, 16-byte accesses, any n > 0.  Reads e and p, writes e, and where ema_mirror is given
 *   the bf16 (round-to-nearest-even) cast of the NEW e in the same pass: 14 bytes per element (12 without a mirror; a copy
 *   does not read e).  In skip mode every workgroup returns behind its read of ctl: neither e nor p is touched.
 * vt_ema_copy:   dst <- src for `bytes` (a multiple of 16) unless the mode is skip.
 * vt_ema_grid_cap: the element count above which every workgroup of vt_ema_update takes more than one round.
 * VT_ERR_INVALID: a null or misaligned ema / p / dst / src / ctl (16 bytes; the mirror: 8), ema == p, n or bytes <= 0. */
#define VT_EMA_ALPHA 0
#define VT_EMA_MODE 1
#define VT_EMA_COUNT 2
#define VT_EMA_PERIOD 3
#define VT_EMA_STEP 4
#define VT_EMA_SKIP 0
#define VT_EMA_COPY 1
#define VT_EMA_BLEND 2
int64_t vt_ema_grid_cap(void);
int vt_ema_tick(float* ctl, void* stream);
int vt_ema_update(float* ema, const float* p, void* ema_mirror, int64_t n, const float* ctl, void* stream);
int vt_ema_copy(void* dst, const void* src, int64_t bytes, const float* ctl, void* stream);

/* ---- layout / precision plumbing ---------------------------------------- */
/* rows x cols block copy with dtype conversion: dst (=|+=) src */
int vt_copy2d(const void* src, int32_t src_dtype, int64_t lds, void* dst, int32_t dst_dtype,
              int64_t ldd, int64_t rows, int32_t cols, int32_t accumulate, void* stream);
/* images: NCHW f32 -> NHWC dtype with channels zero-padded to Cpad
 * (the `images.to(memory_format=channels_last)` of classifier.py:88-89). */
int vt_nchw_to_nhwc(const float* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W,
                    int32_t Cpad, int32_t dtype, void* stream);
/* dx[B][C][H][W] f32 (=) dy NHWC[..., :C] */
int vt_nhwc_to_nchw(const void* y, int32_t ldy, float* x, int32_t B, int32_t C, int32_t H,
                    int32_t W, int32_t dtype, void* stream);

/* ---- native executor -----------------------------------------------------
 * A step of the backbone is a static list of the calls above.  The host builds
 * the list once per (model, input shape) and replays it with one call, or as a
 * captured hipGraph.  Pointers are (base, byte offset) pairs so one list serves
 * any arena placement. */
#define VT_OP_MAX_PTR 24
#define VT_OP_MAX_INT 110
#define VT_OP_MAX_FLT 8
#define VT_MAX_BASES 16

enum vt_op_kind {
    VT_OP_MEMSET = 1,
    VT_OP_CONV_IGEMM,
    VT_OP_CONV_WGRAD,
    VT_OP_PACK_DGRAD,
    VT_OP_BN_FINALIZE,
    VT_OP_BN_EVAL_COEFFS,
    VT_OP_BN_ACT_APPLY,
    VT_OP_BN_BWD_REDUCE,
    VT_OP_BN_BWD_FINALIZE,
    VT_OP_BN_BWD_APPLY,
    VT_OP_MAXPOOL_FWD,
    VT_OP_MAXPOOL_BWD,
    VT_OP_AVGPOOL_FWD,
    VT_OP_AVGPOOL_BWD,
    VT_OP_ESE_FWD,
    VT_OP_ESE_BWD,
    VT_OP_COLSUM,
    VT_OP_XENT,
    VT_OP_SGD,
    VT_OP_COPY2D,
    VT_OP_NCHW_TO_NHWC,
    VT_OP_NHWC_TO_NCHW,
    VT_OP_FORK, /* side stream waits for everything enqueued on the main stream so far */
    VT_OP_JOIN, /* main stream waits for everything enqueued on the side stream so far */
    VT_OP_RESAMPLE_FWD,
    VT_OP_RESAMPLE_BWD,
    VT_OP_FORK_MARK, /* remember the main stream's position (an event record), nothing waits yet */
    VT_OP_FORK_WAIT, /* side stream waits for the last FORK_MARK: FORK split in two, so that the host can enqueue main-stream
                        work between the mark and the side-stream ops that depend on it */
    VT_OP_STEM_BWD_REDUCE,  /* vt_stem_bn_bwd_reduce */
    VT_OP_STEM_BWD_COMBINE, /* vt_stem_bn_bwd_combine */
    VT_OP_FIXED_TO_F32,     /* vt_fixed_to_f32 */
    VT_OP_PW_STATS,         /* vt_pw_fwd_stats */
    VT_OP_PW_APPLY,         /* vt_pw_fwd_apply */
    VT_OP_PW_REDUCE,        /* vt_pw_bwd_reduce */
    VT_OP_PW_BWD,           /* vt_pw_bwd_apply */
    VT_OP_STEM_BWD_S2,      /* vt_stem_bn_bwd_s2 */
    VT_OP_ALLREDUCE,        /* vt_allreduce_bucket (a gradient bucket, in place) */
    VT_OP_STAT_SYNC,        /* vt_stat_sync (one BatchNorm layer's sums over all ranks) */
    VT_OP_XENT_EVAL,        /* vt_softmax_xent_eval (validation: loss sum, top-1 hits, rows) */
    VT_OP_CONV_DGRAD_BNRED, /* vt_conv_dgrad_bnred (a data gradient + the BatchNorm-backward sums of the producing unit) */
    VT_OP_BN_BWD_FUSED,     /* vt_bn_act_bwd_fused (BatchNorm backward of a unit: reduce, finalize, apply in one launch) */
    VT_OP_BN_FIN_APPLY,     /* vt_bn_finalize_apply */
    VT_OP_BN_BWD_FIN_APPLY, /* vt_bn_bwd_finalize_apply */
    VT_OP_DWCONV_FWD,       /* vt_dwconv_fwd */
    VT_OP_DWCONV_DGRAD,     /* vt_dwconv_dgrad */
    VT_OP_DWCONV_WGRAD,     /* vt_dwconv_wgrad */
    VT_OP_PW_APPLY_FIN,      /* vt_pw_fwd_apply_finalize */
    VT_OP_PW_BWD_FIN,        /* vt_pw_bwd_apply_finalize */
    VT_OP_LAYERNORM_FWD,     /* vt_layernorm_fwd */
    VT_OP_LAYERNORM_BWD,     /* vt_layernorm_bwd */
    VT_OP_SCALE_RES_FWD,     /* vt_scale_residual_fwd */
    VT_OP_SCALE_RES_BWD,     /* vt_scale_residual_bwd */
    VT_OP_CHANNEL_SUMS,      /* vt_channel_sums_to_f32 */
    VT_OP_ADAM_TICK,         /* vt_adam_tick (the optimiser step count, once per step) */
    VT_OP_ADAMW,             /* vt_adamw */
    VT_OP_TOKEN_MIX,         /* vt_token_mix_fwd (forward and, with transw, the data gradient) */
    VT_OP_TOKEN_WGRAD,       /* vt_token_mix_wgrad */
    VT_OP_PATCHIFY_FWD,      /* vt_patchify_fwd */
    VT_OP_PATCHIFY_BWD,      /* vt_patchify_bwd */
    VT_OP_ATTN_FWD,          /* vt_attn_fwd */
    VT_OP_ATTN_BWD,          /* vt_attn_bwd */
    VT_OP_VIT_TOKENS_FWD,    /* vt_vit_tokens_fwd */
    VT_OP_VIT_TOKENS_BWD,    /* vt_vit_tokens_bwd */
    VT_OP_TOKEN_SELECT_FWD,  /* vt_token_select_fwd */
    VT_OP_TOKEN_SELECT_BWD,  /* vt_token_select_bwd */
    VT_OP_WIN_ATTN_FWD,      /* vt_win_attn_fwd */
    VT_OP_WIN_ATTN_BWD,      /* vt_win_attn_bwd */
    VT_OP_TALK_ATTN_FWD,     /* vt_talk_attn_fwd */
    VT_OP_TALK_ATTN_BWD,     /* vt_talk_attn_bwd */
    VT_OP_CLS_ATTN_FWD,      /* vt_cls_attn_fwd */
    VT_OP_CLS_ATTN_BWD,      /* vt_cls_attn_bwd */
    VT_OP_TOKEN_PREPEND_FWD, /* vt_token_prepend_fwd */
    VT_OP_TOKEN_PREPEND_BWD, /* vt_token_prepend_bwd */
    VT_OP_DW3_GELU_POOL_FWD, /* vt_dw3_gelu_pool_fwd */
    VT_OP_DW3_GELU_POOL_BWD, /* vt_dw3_gelu_pool_bwd */
    VT_OP_SE_GATE_FWD,       /* vt_se_gate_fwd */
    VT_OP_SE_GATE_BWD,       /* vt_se_gate_bwd */
    VT_OP_CHANNEL_STATS,     /* vt_channel_stats */
    VT_OP_POOL_ATTN_FWD,     /* vt_pool_attn_fwd */
    VT_OP_POOL_ATTN_BWD,     /* vt_pool_attn_bwd */
    VT_OP_PREFIX_TOKENS_FWD, /* vt_prefix_tokens_fwd */
    VT_OP_PREFIX_TOKENS_BWD, /* vt_prefix_tokens_bwd */
    VT_OP_PREFIX_POOL_FWD,   /* vt_prefix_pool_fwd */
    VT_OP_PREFIX_POOL_BWD,   /* vt_prefix_pool_bwd */
    VT_OP_BN_ADD_ACT_APPLY,         /* vt_bn_add_act_apply */
    VT_OP_BN_ADD_ACT_FIN_APPLY,     /* vt_bn_add_act_finalize_apply */
    VT_OP_BN_ADD_ACT_BWD_REDUCE,    /* vt_bn_add_act_bwd_reduce */
    VT_OP_BN_ADD_ACT_BWD_APPLY,     /* vt_bn_add_act_bwd_apply */
    VT_OP_BN_ADD_ACT_BWD_FIN_APPLY, /* vt_bn_add_act_bwd_finalize_apply */
    VT_OP_STEM7_S2D,                /* vt_stem7_s2d */
    VT_OP_STEM7_PACK_FILTER,        /* vt_stem7_pack_filter */
    VT_OP_STEM7_UNPACK_WGRAD,       /* vt_stem7_unpack_wgrad */
    VT_OP_GCONV3_FWD,               /* vt_gconv3_fwd */
    VT_OP_GCONV3_DGRAD,             /* vt_gconv3_dgrad */
    VT_OP_GCONV3_WGRAD,             /* vt_gconv3_wgrad */
    VT_OP_SE_MLP_FWD,               /* vt_se_mlp_fwd */
    VT_OP_SE_MLP_BWD,               /* vt_se_mlp_bwd */
    VT_OP_DWT_FWD,                  /* vt_dwt_fwd */
    VT_OP_DWT_BWD,                  /* vt_dwt_bwd */
    VT_OP_DWT_WGRAD_REDUCE,         /* vt_dwt_wgrad_reduce */
    VT_OP_BN_KEEP_APPLY,            /* vt_bn_keep_apply */
    VT_OP_BN_KEEP_FIN_APPLY,        /* vt_bn_keep_finalize_apply */
    VT_OP_BN_KEEP_BWD_REDUCE,       /* vt_bn_keep_bwd_reduce */
    VT_OP_BN_KEEP_BWD_APPLY,        /* vt_bn_keep_bwd_apply */
    VT_OP_BN_KEEP_BWD_FIN_APPLY,    /* vt_bn_keep_bwd_finalize_apply */
    VT_OP_BN_ACT_AVGPOOL_APPLY,     /* vt_bn_act_avgpool_apply */
    VT_OP_BN_ACT_AVGPOOL_FIN_APPLY, /* vt_bn_act_avgpool_finalize_apply */
    VT_OP_WFUSE_FWD,                /* vt_wfuse_fwd */
    VT_OP_WFUSE_BWD,                /* vt_wfuse_bwd */
    VT_OP_WFUSE_FIN,                /* vt_wfuse_finalize */
    VT_OP_SPP_FWD,                  /* vt_spp_fwd */
    VT_OP_SPP_BWD,                  /* vt_spp_bwd */
    VT_OP_DEFORM_FWD,               /* vt_deform_fwd */
    VT_OP_DEFORM_BWD,               /* vt_deform_bwd */
    VT_OP_DEFORM_WGRAD,             /* vt_deform_wgrad */
    VT_OP_GRAD_SUMSQ,               /* vt_grad_sumsq */
    VT_OP_CLIP_COEF,                /* vt_clip_coef */
    VT_OP_SGD_CLIP,                 /* vt_sgd_momentum_clip */
    VT_OP_ADAMW_CLIP,               /* vt_adamw_clip */
    VT_OP_LAMB_MOMENTS,             /* vt_lamb_moments */
    VT_OP_LAMB_APPLY,               /* vt_lamb_apply */
    VT_OP_BCE,                      /* vt_sigmoid_bce */
    VT_OP_BN_ADD_ACT_KEEP_APPLY,         /* vt_bn_add_act_keep_apply */
    VT_OP_BN_ADD_ACT_KEEP_FIN_APPLY,     /* vt_bn_add_act_keep_finalize_apply */
    VT_OP_BN_ADD_ACT_KEEP_BWD_REDUCE,    /* vt_bn_add_act_keep_bwd_reduce */
    VT_OP_BN_ADD_ACT_KEEP_BWD_APPLY,     /* vt_bn_add_act_keep_bwd_apply */
    VT_OP_BN_ADD_ACT_KEEP_BWD_FIN_APPLY, /* vt_bn_add_act_keep_bwd_finalize_apply */
    VT_OP_EMA_TICK,                 /* vt_ema_tick (the EMA step mode, once per optimiser step) */
    VT_OP_EMA_UPDATE,               /* vt_ema_update */
    VT_OP_EMA_COPY,                 /* vt_ema_copy */
    VT_OP_KIND_END
};

/* OR-ed into vt_op.kind: enqueue this op on the side stream.  Filter gradients depend only
 * on a layer's input and dz, nothing downstream waits for them before the optimiser, so they
 * run beside the (HBM-bound) rest of backward instead of in line with it. */
#define VT_OP_SIDE_STREAM 0x10000

typedef struct vt_ptr {
    int32_t base; /* index into the bases[] passed at run time; -1 = NULL */
    int32_t pad;
    int64_t offset; /* bytes */
} vt_ptr;

typedef struct vt_op {
    int32_t kind;
    int32_t tag; /* host-defined id (layer index), echoed in error messages */
    vt_ptr ptr[VT_OP_MAX_PTR];
    int32_t i[VT_OP_MAX_INT];
    double f[VT_OP_MAX_FLT];
} vt_op;

/* run ops[0..n) in order on `stream`; argument order per kind is documented in
 * vt_runtime.hip next to each case. */
int vt_run_ops(const vt_op* ops, int32_t n, void* const* bases, int32_t nbases, void* stream);
/* same, with a side stream for ops flagged VT_OP_SIDE_STREAM (FORK / JOIN order the two).
 * side == NULL or side == stream runs everything in line. */
int vt_run_ops_streams(const vt_op* ops, int32_t n, void* const* bases, int32_t nbases, void* stream,
                       void* side);
/* same, for a list that is run in SEGMENTS (the data-parallel trainer issues a gradient bucket's collective between
 * two segments, reference configs/base.yaml:17-19 = DDP's per-bucket hooks): with VT_RUN_LEAVE_SIDE_OPEN the call
 * does not order `stream` behind the side stream on return -- the caller joins them itself (a later segment's JOIN
 * op, or vt_stream_wait) -- so cutting a list does not serialise the filter-gradient stream. */
#define VT_RUN_LEAVE_SIDE_OPEN 1
int vt_run_ops_streams_ex(const vt_op* ops, int32_t n, void* const* bases, int32_t nbases, void* stream,
                          void* side, int32_t flags);
/* order `waiter` behind everything enqueued on `signaller` so far (a pooled event; no host synchronisation) */
int vt_stream_wait(void* waiter, void* signaller);

/* hipGraph capture of an op list (side-stream ops become parallel graph branches): capture
 * once, replay with one launch. */
int vt_graph_create(const vt_op* ops, int32_t n, void* const* bases, int32_t nbases,
                    void** graph_out);
int vt_graph_launch(void* graph, void* stream);
int vt_graph_destroy(void* graph);

/* ---- data-parallel collectives (RCCL over xGMI, bound at run time) ------------------------------------------------
 * The reference leaves these to DistributedDataParallel / SyncBatchNorm (`strategy: ddp`, `sync_batchnorm: true`,
 * configs/base.yaml:17-22).  Here they are stream-ordered entry points, so a launch list carries them as ops
 * (VT_OP_ALLREDUCE, VT_OP_STAT_SYNC) between the kernels that produce and consume their operands.  One communicator per
 * process (= per GPU): rank 0 draws an id, the host side hands it to every rank (any out-of-band channel), every rank
 * calls vt_comm_init with the device current.  The RCCL image already mapped into the process is used when there is
 * one (PyTorch's), else librccl.so.1 is loaded. */
#define VT_COMM_ID_BYTES 128
int vt_comm_unique_id(void* id128);
int vt_comm_init(const void* id128, int32_t rank, int32_t world);
/* Optional second communicator over the same ranks (a second id, drawn and carried like the first), used by
 * vt_stat_sync only: RCCL serialises the operations of ONE communicator in issue order across streams, so the per-layer
 * statistics exchanges (main stream) would otherwise queue behind the bucket all-reduces (filter-gradient stream). */
int vt_comm_init_stat(const void* id128);
int vt_comm_has_stat(void);
int vt_comm_world(void); /* ranks of this process's communicator, 0 without one */
int vt_comm_destroy(void);
/* in-place sum all-reduce of `count` elements (VT_F32 / VT_BF16 gradients, VT_I64 fixed-point sums) on `stream` */
int vt_allreduce_bucket(void* buf, int64_t count, int32_t dtype, void* stream);
/* SyncBatchNorm exchange of one layer: vt_stat_fold, then the int64 all-reduce of the folded 32*C bytes */
int vt_stat_sync(float* stats, int32_t C, void* stream);

/* ---- timing helpers for bench.py (HIP events on the launch stream) ------- */
int vt_event_create(void** ev);
int vt_event_record(void* ev, void* stream);
int vt_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
int vt_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* VT_AMD_H */
