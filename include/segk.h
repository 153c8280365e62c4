/* segk -- C ABI of the MI355X (gfx950) segmentation hot-path kernels.
 *
 * This is the drop-in boundary of the project: a shared library
 * (image_segmentation_amd/csrc/libsegk.so) with plain-C entry points -- raw device pointers, ints and a
 * HIP stream handle; no torch/C++ types cross it.  The reference (in5omnia/Image_Segmentation) has no
 * FFI of its own: its hot path is a chain of stock torch.nn layers.  Each entry below names the
 * reference layer(s) it replaces (file:line under the reference repo) so a maintainer can bind it from
 * any host (ctypes stub in INTEGRATION.md; image_segmentation_amd/_lib.py is the binding we ship).
 *
 * Conventions
 *  - every function returns 0 on success, a negative code on failure; segk_last_error() returns a
 *    thread-local message.  Nothing throws, allocates device memory, or synchronises the device:
 *    all launches are asynchronous on `stream` (graph-capture safe); all buffers are caller-owned.
 *  - activations are NHWC, channel count padded to a multiple of 32 ("Cp"); padded channels are zero.
 *  - dtype: SEGK_F32 (exact fp32 MFMA, parity mode) or SEGK_BF16 (bf16 storage/MFMA, fp32 accumulate).
 *  - parameters and their gradients stay in the reference layout and fp32 (OIHW conv weights, IOHW
 *    transposed-conv weights, per-channel vectors); segk_pack_* convert them to the MFMA layout.
 */
#ifndef SEGK_H
#define SEGK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SEGK_F32 0
#define SEGK_BF16 1
#define SEGK_MAX_CLASSES 8

typedef void* segk_stream_t; /* hipStream_t */

/* ABI version and the number of entry points this header declares: segk_version() / segk_entry_count() of a library
 * must equal them (image_segmentation_amd/_lib.py refuses a library whose values differ from the table it binds) */
#define SEGK_ABI_VERSION 340
#define SEGK_ENTRY_COUNT 125
int segk_version(void);
int segk_entry_count(void);
/* first 16 hex digits of the sha256 over the sources this library was built from (image_segmentation_amd/build.py:
 * source_hash) -- lets a host check that a shipped libsegk.so matches the sources beside it */
const char* segk_build_id(void);
const char* segk_last_error(void);

/* ---- layout ------------------------------------------------------------------------------------ */
/* NCHW fp32 [B,C,H,W] -> NHWC dtype [B,H,W,Cp] (zero padded).  Input edge of model(X), training.py:45-46 */
int segk_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int Cp, int dtype, segk_stream_t s);
/* NHWC dtype [B,H,W,Cp] -> NCHW fp32 [B,C,H,W] */
int segk_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int Cp, int dtype, segk_stream_t s);

/* Conv2d weight OIHW fp32 [Cout][CA+CB][taps] -> MFMA layout [Kp/CH][taps][Np][CH] (CH = 16 fp32 / 32 bf16).
 * The input channels may come from two NHWC sources (the skip concat of unet.py:63 / clipunet.py:102):
 * CA/CB logical, CAp/CBp padded.  mode 0: forward weights; mode 1: data-gradient weights (flipped taps,
 * in/out swapped).  taps = 9 (3x3) or 1 (1x1).  dst holds (CAp+CBp)*taps*Coutp elements. */
int segk_pack_conv_weight(const float* w, void* dst, int Cout, int CA, int CB, int Coutp, int CAp, int CBp,
                          int taps, int mode, int dtype, segk_stream_t s);
/* 3x3 weights: the forward (mode 0) and data-gradient (mode 1) layouts of segk_pack_conv_weight in one pass over the
 * fp32 parameter (training re-packs after every optimizer step); dst_dgrad may be NULL */
int segk_pack_conv3x3_both(const float* w, void* dst_fwd, void* dst_dgrad, int Cout, int CA, int CB, int Coutp, int CAp,
                           int CBp, int dtype, segk_stream_t s);
/* Up to 64 packed copies refreshed by ONE launch (everything a model re-packs after an optimizer step).
 * table: device array of n 64-byte entries { const float* w; void* dst_fwd; void* dst_dgrad; int32 Cout, CA, CB, Coutp,
 * CAp, CBp; int32 block0; int32 kind; int32 pad[2] } sorted by block0 = first block of the tensor; total_blocks = the sum
 * of the entries' block counts.  The table must stay valid until the launch has run.
 *   kind 0: segk_pack_conv3x3_both (blocks (CAp+CBp)/32 * Coutp/32);
 *   kind 1: segk_pack_convt_weight, mode 0 into dst_fwd and mode 1 into dst_dgrad (may be NULL), CA = Cin, CAp = Cinp
 *           (blocks ceil(Cinp*4*Coutp / segk_pack_convt_chunk()));
 *   kind 2: bias w [Cout] -> dst_fwd fp32 [reps][Coutp] (1 block), reps = CA, 0 meaning 4: the bias4 operand of
 *           segk_convt2x2_fwd; reps 1: the padded bias operand of segk_conv1x1;
 *   kind 3: Conv2d 1x1 weight w [Cout][CA] -> segk_pack_conv_weight(taps 1) mode 0 into dst_fwd and mode 1 into dst_dgrad
 *           (may be NULL) (blocks ceil(CAp*Coutp / segk_pack_convt_chunk())). */
int segk_pack_multi(const void* table, int n, int total_blocks, int dtype, segk_stream_t s);
int segk_pack_convt_chunk(void);
/* ConvTranspose2d(k=2,s=2) weight IOHW fp32 [Cin][Cout][2][2] -> MFMA layout; mode 0 forward, 1 data-gradient */
int segk_pack_convt_weight(const float* w, void* dst, int Cin, int Cout, int Cinp, int Coutp, int mode, int dtype,
                           segk_stream_t s);

/* ---- Conv2d 3x3 pad 1 (unet/unet.py:16,19; clip/clipunet.py:87,90), forward and data-gradient -----
 * out[B,H,W,CO1] (| out2[B,H,W,CO2]) = conv3x3( [srcA | srcB] , wpacked ) (+ bias).
 * scale/shift != NULL: the producer layer's BatchNorm+ReLU is applied to srcA on load (fused prologue).
 * stats != NULL: per-tile per-channel (sum, sumsq) partials [segk_conv_tiles()][CO1+CO2][2] for
 * training-mode BatchNorm (finish with segk_bn_finalize).  For the data gradient pass mode-1 weights. */
/* Second conv of a DoubleConv block with its fused BN+ReLU prologue, additionally writing the prologue's result
 * act_out[B,H,W,CA] = relu(srcA * scale + shift) (the hidden activation nn.Sequential would have materialised,
 * unet.py:17-18): the weight-gradient pass then reads it directly instead of re-deriving it per fragment.
 * Only for layers where segk_conv_writes_act_q(CA, CO, dtype) != 0; act_out may be NULL. */
int segk_conv_writes_act_q(int Cin, int Cout, int dtype);
int segk_conv3x3_act(const void* srcA, const void* wpacked, const float* scale, const float* shift, void* out,
                     void* act_out, float* stats, int B, int H, int W, int CA, int CO, int dtype, segk_stream_t s);

/* The stem: Conv2d(Cin <= 3, 64, k=3, p=1) (unet/unet.py:16, first conv of down1) applied directly to the NCHW fp32 input
 * batch of utils/training.py:45 -- an im2col GEMM with K = 9 Cin <= 27 (one MFMA step), bf16 operands rounded exactly as the
 * layout pass + packed weights would round them, bias-free like segk_conv3x3.  x_nchw [B,Cin,H,W] fp32, w_oihw the fp32
 * parameter itself [64][Cin][3][3]; z NHWC bf16 [B,H,W,64]; stats (may be NULL): segk_stem3x3_rows() rows of [64][2]
 * partial sums for segk_bn_finalize; x_nhwc (may be NULL): the padded NHWC bf16 copy of the input [B,H,W,32] the
 * weight-gradient pass reads (what segk_nchw_to_nhwc would have written).  segk_stem3x3_rows() is 0 where the kernel does
 * not apply (bf16 only, W % 16 == 0, Cout == 64): use segk_nchw_to_nhwc + segk_conv3x3 there. */
int segk_stem3x3_rows(int B, int H, int W, int Cin, int Cout, int dtype);
int segk_stem3x3(const float* x_nchw, const float* w_oihw, void* z, void* x_nhwc, float* stats, int B, int H, int W, int Cin,
                 int Cout, int dtype, segk_stream_t s);
/* ... and its weight gradient from the same NCHW fp32 batch and dz NHWC bf16 [B,H,W,64]: segk_stem3x3_wgrad_slabs() slabs of
 * [64][32] fp32 (column k = ci * 9 + tap, the OIHW order; columns >= 9 Cin are zero), summed by
 * segk_wgrad_reduce(slabs, S, grad, 64, 9 * Cin, 0, 64, 32, 0, 1).  0 slabs: not served (use segk_wgrad on the padded copy). */
int segk_stem3x3_wgrad_slabs(int B, int H, int W, int Cin, int Cout, int dtype);
int segk_stem3x3_wgrad(const float* x_nchw, const void* dz, float* slabs, int B, int H, int W, int Cin, int Cout, int dtype,
                       segk_stream_t s);
/* The same weight gradient with dz never stored (unet/unet.py:16-18, first conv + BatchNorm + ReLU of down1: the stem has no
 * data gradient, so dz has this one consumer): da NHWC bf16 [B,H,W,64] is the gradient of the hidden activation, z the first
 * conv's pre-activation, coef the [64][2] output of segk_bn_relu_bwd_stats; dz = scale * (g - c1 - xhat * c2) is formed per
 * element with the formula of segk_bn_relu_bwd and rounded to bf16 as that entry stores it: the slabs are bit-identical to
 * segk_bn_relu_bwd + segk_stem3x3_wgrad. */
int segk_stem3x3_wgrad_bn(const float* x_nchw, const void* da, const void* z, const float* scale, const float* shift,
                          const float* mean, const float* rstd, const float* coef, float* slabs, int B, int H, int W, int Cin,
                          int Cout, int dtype, segk_stream_t s);
int segk_conv_tiles(int B, int H, int W, int Cin, int Cout, int dtype);   /* padded CA+CB and CO1+CO2 of the call */
/* floats to allocate for `stats`: the [tiles][Cp][2] partials plus the scratch segk_bn_finalize reduces through */
int segk_bn_stats_floats(int tiles, int Cp);
int segk_conv3x3(const void* srcA, const void* srcB, const void* wpacked, const float* bias, const float* scale,
                 const float* shift, void* out, void* out2, float* stats, int B, int H, int W, int CA, int CB,
                 int CO1, int CO2, int dtype, segk_stream_t s);
/* Conv2d 1x1 (clip/clipunet.py:84,122): same contract, taps = 1 */
int segk_conv1x1(const void* srcA, const void* wpacked, const float* bias, void* out, int B, int H, int W, int CA,
                 int CO, int dtype, segk_stream_t s);
/* ConvTranspose2d(k=2,s=2) forward (unet.py:59; clipunet.py:83): in [B,H,W,Cin] -> out [B,2H,2W,Cout];
 * bias4 = the layer bias tiled over the four taps (length 4*Cout, zero in padded channels) or NULL */
int segk_convt2x2_fwd(const void* in, const void* wpacked, const float* bias4, void* out, int B, int H, int W,
                      int Cin, int Cout, int dtype, segk_stream_t s);
/* ... its data gradient: dout [B,2H,2W,Cout] -> din [B,H,W,Cin]  (H,W are the INPUT grid) */
int segk_convt2x2_dgrad(const void* dout, const void* wpacked, void* din, int B, int H, int W, int Cin, int Cout,
                        int dtype, segk_stream_t s);

/* ---- weight gradients ---------------------------------------------------------------------------
 * slabs [S][CD][taps][CA+CB] fp32 = split-K partials of  sum_p dz[p][n] * a[p+tap][k]; then
 * segk_wgrad_reduce sums them in fixed order into the reference-layout gradient (fp32, overwritten; the
 * slabs are read only).
 * geo 0: Conv2d 3x3 (grad OIHW [N][CA+CB][9]);  geo 1: Conv2d 1x1;  geo 2: ConvTranspose2d(k=2,s=2) with
 * dz := layer input [B,H,W,CD], srcA := output gradient [B,2H,2W,CA], grad IOHW [CD][CA][2][2].
 * scale/shift: BatchNorm+ReLU prologue on srcA (the conv input is relu(bn(z)) of the previous conv). */
int segk_wgrad_tiles(int B, int H, int W, int geo, int dtype);
/* split-K factor S the host sizes the slab buffer with ([S][CD][taps][CA+CB] fp32) for `tiles` = segk_wgrad_tiles():
 * enough workgroups to fill the chip for this layer's (n, k) tiling, never more slabs than tiles; 0 for invalid input.
 * The value is advice, not a requirement: segk_wgrad accepts ANY S in [1, 65535] for every kernel form.  Slab s sums the
 * spatial tiles s, s + S, s + 2S, ...; every element of all S slabs is written by the call (the caller need not clear the
 * buffer), a slab whose index is at or above the form's tile count is written as zeros, and nothing beyond slab S - 1 is
 * touched (tests/test_gpu_wgrad_matrix.py runs S below, at and above the tile count on NaN-filled buffers). */
int segk_wgrad_split(int tiles, int CD, int CA, int CB, int geo, int dtype);
int segk_wgrad(const void* dz, const void* srcA, const void* srcB, const float* scale, const float* shift,
               float* slabs, const void* zeros64, int S, int B, int H, int W, int CD, int CA, int CB, int geo,
               int dtype, segk_stream_t s);   /* zeros64: >= 64 zero bytes in device memory (halo source of the
                                                  LDS-DMA path); NULL selects the register-staged kernel */
/* slabs [S][Np][taps][CAp+CBp] -> grad [N][CA+CB][taps]: rows n >= N and the padding columns of either source are skipped.
 * CAp + CBp must be a multiple of 32 (refused otherwise); S <= 16 stages one gradient row of (CA+CB)*taps floats in LDS
 * (at most 64 KiB), S > 16 takes the slab-parallel form. */
int segk_wgrad_reduce(const float* slabs, int S, float* grad, int N, int CA, int CB, int Np, int CAp, int CBp,
                      int taps, segk_stream_t s);
/* Up to four such reductions in ONE launch -- the two weight gradients of a DoubleConv block (unet.py:16,19), the
 * ConvTranspose2d weight gradient of the Up block around it (unet.py:59) and that layer's bias gradient: jobs is a HOST
 * array (read during the call).  kind 0: segk_wgrad_reduce(src = slabs, S, dst = grad, N, CA, CB, Np, CAp, CBp, taps);
 * kind 1: column sums dst[c] = sum over rows r < S of src[(r * N + CA + c) * 2], c < CB (N = channels per row of the
 * [rows][N][2] BatchNorm-style partials segk_conv3x3 writes: the bias gradient of the ConvTranspose whose output is the
 * second concat operand is the channel sum of the concat data gradient).  Results equal the single launches bit for bit. */
typedef struct segk_reduce_job {
  const float* src;
  float* dst;
  int kind, S, N, CA, CB, Np, CAp, CBp, taps, pad_;
} segk_reduce_job;
int segk_wgrad_reduce_multi(const segk_reduce_job* jobs, int n, segk_stream_t s);

/* ---- BatchNorm2d + ReLU (unet.py:17-18,20-21; clipunet.py:88-89,91-92) ---------------------------
 * training: stats partials -> scale = gamma*rstd, shift = beta - mean*scale, batch mean/rstd saved for
 * backward, running stats updated (momentum, unbiased var; conv_bias only shifts running_mean: the
 * kernels work on the bias-free conv output because the bias cancels inside BatchNorm).
 * eval: scale/shift from running statistics. */
int segk_bn_finalize(const float* stats, int tiles, int Cp, int C, double count, const float* conv_bias,
                     const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, int training, float* scale, float* shift, float* mean, float* rstd, segk_stream_t s);
/* y = relu(z*scale + shift) over P pixels */
int segk_bn_relu_apply(const void* z, void* y, const float* scale, const float* shift, long P, int Cp, int dtype,
                       segk_stream_t s);
/* ... and the MaxPool2d(2,2) of y in the same pass (unet.py:20-21 followed by :40 of the next Down block):
 * pooled [B,H/2,W/2,Cp]; bit-identical to segk_bn_relu_apply + segk_maxpool2x2_fwd */
int segk_bn_relu_apply_pool(const void* z, void* y, void* pooled, const float* scale, const float* shift, int B, int H, int W,
                            int Cp, int dtype, segk_stream_t s);
/* backward of y = relu(bn(z)): dz (may alias dy) and dgamma/dbeta.  part: segk_bn_bwd_blocks()*Cp*2 floats,
 * coef: 2*Cp floats of scratch. */
int segk_bn_bwd_blocks(long P, int Cp, int dtype);
int segk_bn_relu_bwd(const void* dy, const void* z, void* dz, const float* scale, const float* shift,
                     const float* mean, const float* rstd, long P, int Cp, int C, float* part, float* dgamma,
                     float* dbeta, float* coef, int dtype, segk_stream_t s);

/* per-channel sum over P pixels of an NHWC tensor: the bias gradient of ConvTranspose2d (unet.py:59) and of the
 * 1x1 convs (clipunet.py:84,122).  part: segk_bn_bwd_blocks(P,Cp,dtype)*Cp floats of scratch. */
int segk_channel_sum(const void* x, long P, int Cp, int C, float* part, float* out, int dtype, segk_stream_t s);

/* ---- MaxPool2d(2,2) (unet.py:40) ---------------------------------------------------------------- */
int segk_maxpool2x2_fwd(const void* x, void* y, int B, int H, int W, int Cp, int dtype, segk_stream_t s);
/* dx (+)= route(dy) to the first maximum of each window; accumulate=1 adds into dx (skip gradient) */
int segk_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int B, int H, int W, int Cp, int accumulate,
                        int dtype, segk_stream_t s);

/* Pooling backward of a DoubleConv block's output y = relu(bn(z)) (unet.py:40 behind :20-21) that ALSO accumulates that
 * BatchNorm's backward reductions sum(g), sum(g*xhat) over the complete gradient it writes (xhat recovered from y where the
 * ReLU is active): part holds segk_maxpool_bwd_stat_blocks() rows of [Cp][2] floats, finished by
 * segk_bn_relu_bwd_from_part (finalize + apply, no reduce pass).  segk_maxpool_bwd_stat_blocks returns 0 when the shape
 * is not served (Cp / vector width must be a power of two). */
int segk_maxpool_bwd_stat_blocks(int B, int H, int W, int Cp, int dtype);
int segk_maxpool2x2_bwd_bnstat(const void* x, const void* dy, void* dx, int B, int H, int W, int Cp, int accumulate,
                               const float* scale, const float* shift, const float* mean, const float* rstd, float* part,
                               const void* z, int dtype, segk_stream_t s);
/* z (may be NULL): the block's pre-activation [B,H,W,Cp].  xhat is recovered from x = relu(z*scale+shift) itself except
 * for channels where that is impossible or ill-conditioned (scale == 0, |scale| < |shift|/16): the threads owning such a
 * channel read z and take xhat = (z - mean) * rstd, exactly like segk_bn_relu_bwd's own reduction; with z == NULL those
 * channels get xhat = -mean * rstd (wrong dgamma for them). */
int segk_bn_relu_bwd_from_part(const void* dy, const void* z, void* dz, const float* scale, const float* shift,
                               const float* mean, const float* rstd, long P, int Cp, int C, const float* part, int nb,
                               float* dgamma, float* dbeta, float* coef, int dtype, segk_stream_t s);

/* The reduce and finalize steps of segk_bn_relu_bwd alone (unet/unet.py:17-18 of down1): dgamma, dbeta and coef [Cp][2] as that
 * entry returns them, no dz -- for a consumer that forms dz itself (segk_stem3x3_wgrad_bn).  part: segk_bn_bwd_blocks() rows. */
int segk_bn_relu_bwd_stats(const void* dy, const void* z, const float* scale, const float* shift, const float* mean,
                           const float* rstd, long P, int Cp, int C, float* part, float* dgamma, float* dbeta, float* coef,
                           int dtype, segk_stream_t s);

/* ---- bilinear resize, align_corners=False (clip/clipunet.py:99-100: skip features 14x14 -> decoder grid) ----
 * x [B,IH,IW,Cp] -> y [B,OH,OW,Cp]; backward is a deterministic gather dy -> dx */
int segk_bilinear_fwd(const void* x, void* y, int B, int IH, int IW, int OH, int OW, int Cp, int dtype,
                      segk_stream_t s);
/* scratch: B*OH*IW*Cp floats for the separable two-pass form (x then y; about 3x the up-sampling factor of work per
 * element instead of its square), or NULL for the single-pass 2-D gather */
int segk_bilinear_bwd(const void* dy, void* dx, float* scratch, int B, int IH, int IW, int OH, int OW, int Cp, int dtype,
                      segk_stream_t s);

/* ---- CLIP vision transformer, frozen feature extractor (clip/clipunet.py:25-46,48-63 drive transformers'
 * CLIPVisionModel -- third party; algorithm: modeling_clip.py CLIPVisionEmbeddings / CLIPEncoderLayer / CLIPAttention /
 * CLIPMLP).  Token tensors are row matrices [Mp][C], Mp = B*T rounded up to 16 rows; the residual stream is fp32. */
/* nn.Linear / patch-projection GEMM on MFMA: out[M][N] = rows[M][K] . W^T (+ bias) (act 1: quick_gelu, CLIPMLP).
 * wpacked = segk_pack_conv_weight(W viewed as [N][K][1][1], taps 1, mode 0); K, N multiples of 32; M multiple of 16. */
int segk_linear(const void* rows, const void* wpacked, const float* bias, void* out, long M, int K, int N, int act,
                int dtype, segk_stream_t s);
/* image NCHW fp32 [B,C,H,W] -> patch rows [B*(H/ps)*(W/ps)][Kp], k = c*ps*ps + i*ps + j (zero beyond C*ps*ps):
 * the im2col of CLIPVisionEmbeddings.patch_embedding (Conv2d(C, D, ps, stride ps, bias=False)) */
int segk_vit_patchify(const float* x, void* rows, int B, int C, int H, int W, int ps, int Kp, int dtype, segk_stream_t s);
/* h[b][t] = LayerNorm_pre( (t == 0 ? class_embedding : proj[b][t-1]) + position_embedding[t] ); h fp32 [B*T][D] */
int segk_vit_embed_ln(const void* proj, const float* cls, const float* pos, const float* gamma, const float* beta,
                      float eps, float* h, int B, int T, int D, int Dp, int dtype, segk_stream_t s);
/* residual add + LayerNorm: h[M][D] += delta[M][Dp] (delta may be NULL); out[M][Dp] = LN(h)*gamma+beta (out may be
 * NULL: add only) -- CLIPEncoderLayer's residual connections fused with the next layer_norm1/2 */
int segk_add_layernorm(float* h, const void* delta, const float* gamma, const float* beta, float eps, void* out, long M,
                       int D, int Dp, int dtype, segk_stream_t s);
/* split-K forms for GEMMs too small to fill 256 CUs (ViT out_proj / fc2 at B = 16: 78 output tiles): `ksplit` partial
 * products out_parts[ksplit][M][N] (bf16, bias on split 0), summed in fixed order by the residual add that follows */
int segk_linear_splitk(const void* rows, const void* wpacked, const float* bias, void* out_parts, long M, int K, int N,
                       int ksplit, int dtype, segk_stream_t s);
int segk_add_layernorm_parts(float* h, const void* delta, int nparts, long part_stride, const float* gamma,
                             const float* beta, float eps, void* out, long M, int D, int Dp, int dtype, segk_stream_t s);
/* CLIPAttention: qkv [B*T][ldq] = [q | k | v] (heads*head_dim each) -> ctx [B*T][ldo] = softmax(q k^T * scale) v per
 * head; head_dim 32 or 64; the head's K and V must fit the 160 KiB LDS (T <= 320 fp32 / 640 bf16 at head_dim 64) */
int segk_attention(const void* qkv, void* ctx, int B, int T, int heads, int head_dim, int ldq, int ldo, float scale,
                   int dtype, segk_stream_t s);
/* drop CLS, residual stream -> NHWC feature grid [B,G,G,Dp] in dtype (clipunet.py:48-51,54-63) */
int segk_vit_tokens_to_grid(const float* h, void* out, int B, int T, int D, int Dp, int dtype, segk_stream_t s);

/* ---- eval-time pre/post-processing on device (utils/utils.py:13-115; training.py:87-99) ---------------------------
 * one image [C,H,W] -> its slot [C,T,T] of the network batch: resize to (nh,nw) + zero padding (utils.py:13-49).
 * mode 0: anti-aliased bilinear = F.interpolate(bilinear, align_corners=False, antialias=True), what torchvision's
 * tensor TF.resize computes from 0.17 on; mode 2: plain two-tap bilinear (antialias=False: torchvision < 0.17 on
 * tensors; the reference pins no version); mode 1: nearest.  elem 0: float32, 1: int64 (labels; mode 1 only). */
int segk_resize_pad(const void* img, void* out, int C, int H, int W, int nh, int nw, int T, int pad_top, int pad_left,
                    int mode, int elem, segk_stream_t s);
/* slot [C,T,T] fp32 -> crop the (nh,nw) window at (pad_top,pad_left) -> [C,oh,ow]: F.interpolate bilinear
 * (align_corners=False; mode 0) or nearest (mode 1) (utils.py:51-75) */
int segk_crop_resize(const float* slot, float* out, int C, int T, int pad_top, int pad_left, int nh, int nw, int oh,
                     int ow, int mode, segk_stream_t s);
/* prediction pre-processing (segmentation_webapp/app.py:266-273: TF.to_tensor + process_batch_forward): an 8-bit
 * interleaved image [H,W,Cin], Cin 1 / 3 / 4 (alpha dropped; 4-channel images 4-byte aligned), -> its float slot
 * [min(Cin,3),T,T].  Every tap is (float)u8 / 255.0f fed to the tap / weight code of segk_resize_pad, so the slot equals
 * bit for bit what segk_resize_pad makes of the converted image.  mode as in segk_resize_pad (0 / 1 / 2). */
int segk_resize_pad_u8(const uint8_t* img_hwc, float* out, int Cin, int H, int W, int nh, int nw, int T, int pad_top,
                       int pad_left, int mode, segk_stream_t s);
/* prediction post-processing in one pass (app.py:291-326; utils.py:51-75): slot [C,T,T] fp32 (logits or probabilities) ->
 * crop + resize with the arithmetic, geometry arguments and modes of segk_crop_resize -> argmax over the classes (first
 * maximum, NaN maximal: torch.argmax / segk_confusion) -> mask [oh,ow] uint8.  The full-size logits are never stored.
 * Optional outputs: color [oh,ow,3] uint8 = palette[C][3] looked up per pixel (color and palette come together);
 * counts[8] += pixels per class; M[pred*8 + label] += 1 as segk_confusion does, for labels [oh,ow] inside [0,C) (labels
 * and M come together; the caller zeroes counts and M).  1 <= C <= 8; mask and color 4-byte aligned. */
int segk_predict_mask(const float* slot, uint8_t* mask, uint8_t* color, const uint8_t* palette, uint64_t* counts,
                      const int64_t* labels, uint64_t* M, int C, int T, int pad_top, int pad_left, int nh, int nw, int oh,
                      int ow, int mode, segk_stream_t s);

/* segk_resize_pad / segk_resize_pad_u8 of the FLIPPED image (test-time augmentation): bit 0 of flip reverses
 * x, bit 1 reverses y, in the image's own pixels; only the source fetch changes (it reads (H-1-y, W-1-x)), so the slot
 * equals bit for bit what the entries above make of the flipped image, and flip 0 equals them.  0 <= flip <= 3. */
int segk_resize_pad_flip(const void* img, void* out, int C, int H, int W, int nh, int nw, int T, int pad_top, int pad_left,
                         int mode, int elem, int flip, segk_stream_t s);
int segk_resize_pad_u8_flip(const uint8_t* img_hwc, float* out, int Cin, int H, int W, int nh, int nw, int T, int pad_top,
                            int pad_left, int mode, int flip, segk_stream_t s);

/* ---- multi-view prediction: test-time augmentation and ensembling (the reference holds no code for it) ----
 * One view of an (oh, ow) image: the network output for one model, one target size and one flip of the image. */
#define SEGK_MAX_VIEWS 16
#define SEGK_MERGE_PROB 0            /* acc += weight * (kind 0: softmax(z); kind 1: z) */
#define SEGK_MERGE_LOGIT 1           /* acc += weight * z (kind is not read) */
typedef struct segk_view_desc {      /* one view; 48 bytes, 16-byte aligned */
  uint64_t slot;                     /* device address of the view's fp32 slot [C][T][T] */
  int32_t T, pad_top, pad_left, nh, nw; /* the slot's side and the (nh, nw) window of the flipped image in it; T T < 2^30 */
  int32_t flip;                      /* bit 0: the view saw the image reversed in x, bit 1: in y */
  int32_t kind;                      /* 0: the slot holds logits, 1: probabilities */
  float weight;                      /* w_v / sum of the weights, rounded once from float64 */
  int32_t pad_[2];
} segk_view_desc;
/* views_dev: a DEVICE table of V descriptors (1 <= V <= SEGK_MAX_VIEWS), 16-byte aligned; the host never reads it, so its
 * contents are the caller's to get right (image_segmentation_amd/tta.py: view_table checks them).  Per output pixel (oy, ox),
 * for v = 0..V-1 in table order: z = the view sampled at (flip & 2 ? oh-1-oy : oy, flip & 1 ? ow-1-ox : ox) with the
 * arithmetic of segk_crop_resize (mode 0 bilinear, 1 nearest), then the accumulation above in fp32.  mask = argmax of acc
 * (first maximum, NaN maximal: segk_predict_mask's rule); color, palette, counts, labels and M as in segk_predict_mask.
 * Optional: conf [oh,ow] uint8 = (uint8)(255 p_best + 0.5) and scores fp32 [C,oh,ow] = p, with p = acc / sum_k acc
 * (merge 0) or softmax(acc) (merge 1); a NaN confidence is stored as 0.  No float atomics: bit-stable from run to run.
 * 1 <= C <= 8; mask, color and conf 4-byte aligned; oh ow < 2^31 - 4.  Only the scalar arguments and the output pointers
 * are validated (-2 before any launch). */
int segk_predict_merge(const void* views_dev, int V, int C, int merge, int mode, int oh, int ow, uint8_t* mask,
                       uint8_t* color, const uint8_t* palette, uint64_t* counts, const int64_t* labels, uint64_t* M,
                       uint8_t* conf, float* scores, segk_stream_t s);

/* ---- tiled full-resolution prediction: tile gather and blend (the reference holds no code for it) ----
 * The image is cut at its own resolution into T x T tiles, the tiles run through the network as batches, and the overlapping
 * outputs are blended into one mask; nothing is resampled.  The tile plan is derived INSIDE the kernels from the scalars (no
 * descriptor table, no host-read array); image_segmentation_amd/tiles.py: tile_axis is the same arithmetic.  Per axis of
 * length L, with stride s = T - overlap (0 <= overlap <= T / 2):
 *   L <= T: one tile at origin -((T - L) / 2) (the image centred, the odd pixel after it);
 *   L >  T: n = ceil((L - T) / s) + 1 tiles at origins min(i s, L - T) (the last tile pulled back inside the image).
 * A pixel is covered by 1..3 tiles per axis; tiles are numbered row-major, t = iy nx + ix.
 *
 * segk_tile_gather_u8 / segk_tile_gather: tiles tile0 .. tile0 + ntiles - 1 of an 8-bit interleaved [H,W,Cin] image (Cin 1,
 * 3 or 4; alpha dropped; value (float)u8 / 255.0f, segk_resize_pad_u8's expression) or a float [C,H,W] image (values
 * unchanged) -> out fp32 [ntiles][min(Cin,3) or C][T][T].  Tile pixel (ty, tx) of tile (iy, ix) is image pixel (y_iy + ty,
 * x_ix + tx); outside the image (an axis with L < T only) it is 0 (SEGK_TILE_PAD_ZERO) or the pixel at r(g, L)
 * (SEGK_TILE_PAD_REFLECT): r = 0 for L == 1, else m = 2 L - 2, j = g mod m (non-negative), r = j < L ? j : m - j.
 * 1 <= T <= 4096; tile0 >= 0, ntiles >= 1, tile0 + ntiles <= ny nx; ntiles c T ceil(T/4) < 2^31 per call (split the range
 * otherwise); out 4-byte aligned (16-byte stores when T % 4 == 0 and out is 16-byte aligned); a 4-channel image 4-byte
 * aligned. */
#define SEGK_TILE_PAD_ZERO 0
#define SEGK_TILE_PAD_REFLECT 1
#define SEGK_TILE_WINDOW_FLAT 0      /* wa(u) = 1 */
#define SEGK_TILE_WINDOW_TRIANGLE 1  /* wa(u) = min(u, T - 1 - u) + 1 */
int segk_tile_gather_u8(const uint8_t* img_hwc, float* out, int Cin, int H, int W, int T, int overlap, int pad, int tile0,
                        int ntiles, segk_stream_t s);
int segk_tile_gather(const float* img_chw, float* out, int C, int H, int W, int T, int overlap, int pad, int tile0, int ntiles,
                     segk_stream_t s);
/* Y fp32 [ny nx][C][T][T]: the network outputs of ALL tiles of the plan, kind 0 logits / 1 probabilities.  Per output pixel
 * (oy, ox), for the covering tiles in row-major tile order: z = Y[t][.][oy - y_iy][ox - x_ix], w = wa(ty) wa(tx) (an
 * integer below 2^24: exact in fp32), s = softmax(z) (segk_predict_merge's) when merge is SEGK_MERGE_PROB and kind is 0,
 * else z; acc_k = acc_k + w s_k (a multiply, then an add), Wtot = Wtot + w.  SEGK_MERGE_PROB: mask = argmax acc, p = acc /
 * sum_k acc.  SEGK_MERGE_LOGIT (kind 0 only): a = acc / Wtot, mask = argmax a, p = softmax(a).  Argmax rule, color, palette,
 * counts, labels, M, conf and scores as in segk_predict_merge.  Positions of Y that no pixel maps to (the padded border of
 * a short axis) are never used: a NaN there reaches no output.  No float atomics: bit-stable from run to run.
 * 1 <= C <= 8; ny nx C T T < 2^30; H W < 2^31 - 4; Y, mask, color, conf and scores 4-byte aligned; every scalar and pointer
 * pairing is validated (-2 before any launch). */
int segk_predict_tiles(const float* Y, int C, int kind, int merge, int window, int H, int W, int T, int overlap, uint8_t* mask,
                       uint8_t* color, const uint8_t* palette, uint64_t* counts, const int64_t* labels, uint64_t* M,
                       uint8_t* conf, float* scores, segk_stream_t s);

/* ---- confidence calibration: reliability histograms and the temperature sweep (the reference holds no code
 * for it).  Integer sums only, accumulated with += into caller-zeroed uint64 buffers (a data set is a sequence of calls into
 * one set of buffers): order-independent and bit-stable, no float atomics, no finalize pass.
 * A pixel is VALID when 0 <= label < C and label != ignore_index (ignore_index -1: none).
 *
 * segk_calib_hist: conf uint8 [H,W] (Prediction.confidence), mask uint8 [H,W], labels int64 [H,W] ->
 * hist uint64 [SEGK_MAX_CLASSES][256][2]: every valid pixel adds 1 to hist[m][q][0], and 1 to hist[m][q][1] when m == l.  The
 * maps are device data, so a mask value m >= C cannot be refused: it is counted under class C - 1 (and, being no label, is
 * never correct).  H W < 2^31 - 4; labels and hist 8-byte aligned. */
#define SEGK_MAX_TEMPS 32
#define SEGK_CALIB_NLL_MAX 262144.0f /* 2^18 nat: a per-pixel NLL at or above it (NaN and inf included) counts as non-finite */
int segk_calib_hist(const uint8_t* conf, const uint8_t* mask, const int64_t* labels, int H, int W, int C, int ignore_index,
                    uint64_t* hist, segk_stream_t s);
/* segk_calib_temps: one view's slot [C,T,T] fp32 of LOGITS, the geometry arguments and modes of segk_predict_mask, labels
 * int64 [oh,ow] and a DEVICE table inv_T_dev of K floats 1/T_j (1 <= K <= SEGK_MAX_TEMPS; the host never reads it).  Per valid
 * pixel: z = the slot sampled with the arithmetic of segk_predict_mask, best = its argmax (first maximum, NaN maximal; the
 * same for every j); per j: s = z inv_T[j], mx = max s, e_k = expf(s_k - mx), S = sum_k e_k in class order, p = e / S, then
 * p = p / sum_k p (a one-view SEGK_MERGE_PROB merge of weight 1: at inv_T = 1.0f the confidence is segk_predict_merge's bit
 * for bit), q = (uint8)(255 p_best + 0.5) clamped, NaN -> 0, nll = logf(S) - (s_l - mx).
 *   hist uint64 [K][256][2]: hist[j][q][0] += 1, hist[j][q][1] += (best == l)
 *   nll_fx[j] += (uint64)((double)max(nll, 0) 65536 + 0.5) when nll < SEGK_CALIB_NLL_MAX, else nonfinite[j] += 1
 *   valid[0] += 1 once per valid pixel
 * The 2^-16 nat fixed point errs by at most 2^-17 nat per pixel; 2^30 pixels at the cap stay inside uint64.  T T < 2^30,
 * oh ow < 2^31 - 4; labels and the outputs 8-byte aligned.  Every scalar and pointer is validated (-2 before any launch). */
int segk_calib_temps(const float* slot, int C, int T, int pad_top, int pad_left, int nh, int nw, int oh, int ow, int mode,
                     const int64_t* labels, int ignore_index, const float* inv_T_dev, int K, uint64_t* hist, uint64_t* nll_fx,
                     uint64_t* nonfinite, uint64_t* valid, segk_stream_t s);

/* ---- mask clean-up: connected components, boxes, blob removal (the reference has no such code: this
 * replaces a mask.cpu() + scipy.ndimage.label post-process).  Integer arithmetic only: results are unique and bit-stable.
 * No launch waits for another workgroup; several launches per call, in stream order.
 *
 * Workspace: ws holds SEGK_CC_WS_INTS(H, W) 32-bit words, 16-byte aligned, uninitialised; segk_cc_label fills it and
 * segk_cc_clean reads it (and uses its vote words), so it must stay untouched between the two.  Layout, in words:
 * best[8] as uint64 (16) | votes [H*W][8] | parent [H*W] | area [H*W] | id [H*W] | row counts [H] | row bases [H]. */
#define SEGK_CC_TILE_W 64
#define SEGK_CC_TILE_H 32
#define SEGK_CC_MAX_PIXELS (1L << 28)
#define SEGK_CC_WS_INTS(H, W) (16L + 11L * (long)(H) * (long)(W) + 2L * (long)(H))
/* DESIGN.md 3.3 "components and ids", "what is recorded": mask [H,W] uint8 -> labels [H,W] int32 (0: unlabelled, else the
 * id 1..K in ascending order of the component's first pixel), num[1] = K, and for the ids 1..min(K, max_components) the rows
 * cls / area / first [max_components] and box [max_components][4] = (y0, x0, y1, x1), y1 and x1 exclusive; the rows past
 * K are zeroed.  A pixel is labelled if its value is < 8 and bit `value` of class_mask is set.  connectivity 4 or 8.
 * box and ws 16-byte aligned; H*W <= SEGK_CC_MAX_PIXELS.  The mask is only read. */
int segk_cc_label(const uint8_t* mask, int32_t* labels, int32_t* num, int32_t* cls, int32_t* area, int32_t* box,
                  int32_t* first, int32_t* ws, int H, int W, int connectivity, int class_mask, int max_components,
                  segk_stream_t s);
/* DESIGN.md 3.3 "removal", "new class of a removed component": after segk_cc_label on the same mask and ws.  A component
 * is removed if area < min_area, or if bit `class` of keep_mask is set and it is not the largest of its class (tie: lowest
 * id); its pixels take the class most of its standing 4-neighbours have (lowest class on a tie, its own with no votes).
 * out [H,W] uint8 (not the mask itself) = the cleaned mask; kept / new_cls [max_components] for the reported ids, zero past
 * K.  May be called again with other min_area / keep_mask on the same ws. */
int segk_cc_clean(const uint8_t* mask, uint8_t* out, int32_t* ws, int32_t* kept, int32_t* new_cls, int H, int W,
                  int min_area, int keep_mask, int max_components, segk_stream_t s);
/* DESIGN.md 3.3 "finish from a mask": the optional outputs of segk_predict_mask, with its pointer rules, from a finished
 * mask [H,W] uint8: color [H,W,3] = palette[mask], counts[8] += pixels per class, M[mask*8 + label] += 1 for labels inside
 * [0,C) (the caller zeroes counts and M).  A mask value >= C is coloured black and counted nowhere.  1 <= C <= 8; mask and
 * color 4-byte aligned; at least one output. */
int segk_mask_finish(const uint8_t* mask, uint8_t* color, const uint8_t* palette, uint64_t* counts, const int64_t* labels,
                     uint64_t* M, int C, int H, int W, segk_stream_t s);

/* ---- mask vectorisation: run table, contour rings, corner vertices (the reference has no such code: this
 * replaces a mask.cpu() + cv2.findContours / pycocotools encode).  Integer arithmetic only: results are unique and bit-stable.
 * No launch waits for another workgroup, the host reads no count back, and every device loop is bounded by an argument; the
 * counts the later launches need are read from device memory.
 *
 * Workspace: SEGK_VEC_WS_INTS(H, W, max_edges) 32-bit words, 16-byte aligned, uninitialised, scratch of ONE call (either
 * entry; nothing has to survive between calls).  With HW = H*W, ME = max_edges and R4(n) = n rounded up to a multiple of 4,
 * in words: 16 | ring areas uint64 [ME/4 + 1] | block partials uint64 [ceil(ME/2048)] | two jump buffers int2 [ME] each |
 * edge keys [ME] | successors, later the ring order [ME] | ring heads [ME] | edge base per pixel [HW] | block partials
 * [ceil(HW/2048)] | corner flags, bytes [ME] | side masks, bytes [HW].  segk_vec_runs uses the first W * ceil(H/128) words. */
#define SEGK_VEC_CHUNK 2048
#define SEGK_VEC_RUN_ROWS 128
#define SEGK_VEC_MAX_CAP (1L << 30)
#define SEGK_VEC_R4(n) (((long)(n) + 3L) / 4L * 4L)
#define SEGK_VEC_WS_INTS(H, W, ME)                                                                                              \
  (16L + SEGK_VEC_R4(2L * ((long)(ME) / 4L + 1L)) + SEGK_VEC_R4(2L * (((long)(ME) + SEGK_VEC_CHUNK - 1L) / SEGK_VEC_CHUNK)) + \
   7L * SEGK_VEC_R4(ME) + SEGK_VEC_R4((long)(H) * (long)(W)) +                                                                  \
   SEGK_VEC_R4(((long)(H) * (long)(W) + SEGK_VEC_CHUNK - 1L) / SEGK_VEC_CHUNK) + SEGK_VEC_R4(((long)(ME) + 3L) / 4L) +          \
   SEGK_VEC_R4(((long)(H) * (long)(W) + 3L) / 4L))
/* DESIGN.md 3.17 "run table": obj [H,W] int32 (0: nothing, else an id >= 1; Components.labels) read in column-major order
 * t = x*H + y.  A run starts at t = 0 and wherever obj differs from the element before; run_start / run_obj [max_runs] hold
 * the first min(runs, max_runs) runs in ascending t (runs of id 0 included), totals[0] = runs.  Nothing at or past max_runs or
 * the run count is written.  H*W <= SEGK_CC_MAX_PIXELS, 1 <= max_runs <= SEGK_VEC_MAX_CAP. */
int segk_vec_runs(const int32_t* obj, int32_t* run_start, int32_t* run_obj, int32_t* totals, int32_t* ws, int H, int W,
                  int max_runs, segk_stream_t s);
/* DESIGN.md 3.17 "boundary edges", "successor", "ring record", "vertices", "capacities": totals[1] = E, the directed unit
 * boundary edges of all objects.  With E <= max_edges: totals[2] = R rings, totals[3] = V corner vertices; ring_obj / ring_head
 * / ring_len [max_rings] and ring_area2 int64 [max_rings] hold the first min(R, max_rings) rings in ascending head key,
 * ring_offset [max_rings + 1] the first min(R, max_rings) + 1 entries of the CSR offsets into xy, xy [max_vertices][2] = (x, y)
 * the first min(V, max_vertices) vertices.  With E > max_edges: totals[2] = totals[3] = -1 and no ring array is touched.
 * Nothing at or past a capacity or a total is written.  connectivity 4 or 8: which of two diagonal pixels of one object a
 * ring joins -- the connectivity obj was labelled with.  1 <= every capacity <= SEGK_VEC_MAX_CAP; ring_area2 8-byte aligned. */
int segk_vec_rings(const int32_t* obj, int32_t* ring_obj, int32_t* ring_head, int32_t* ring_len, int64_t* ring_area2,
                   int32_t* ring_offset, int32_t* xy, int32_t* totals, int32_t* ws, int H, int W, int connectivity,
                   int max_edges, int max_rings, int max_vertices, segk_stream_t s);

/* ---- label rasterisation: polygons and run-length codes -> uint8 label maps (the reference has no such code:
 * this replaces a host rasteriser plus one upload per image).  Integer arithmetic only: the result is unique and bit-stable.
 * One launch serves a ragged batch, one workgroup per tile of SEGK_RAST_TILE_H rows x SEGK_RAST_TILE_W columns; the host
 * builds every table and all of them are DEVICE pointers, so the entry validates the arguments only and the kernel clamps
 * every index it reads from a table to its argument.  No workgroup waits for another; no atomics on global memory. */
#define SEGK_RAST_TILE_H 64
#define SEGK_RAST_TILE_W 256
#define SEGK_RAST_MAX_SIDE 8192
#define SEGK_RAST_POLYGON 0          /* begin / end: rows of edges; inside = odd number of counting crossings (even-odd) */
#define SEGK_RAST_RLE 1              /* begin / end: entries of run_start; inside = odd run index */
typedef struct segk_rast_shape {     /* one shape; 32 bytes */
  int32_t kind;                      /* SEGK_RAST_POLYGON | SEGK_RAST_RLE */
  int32_t value;                     /* 0..255, painted where the shape is inside */
  int32_t begin, end;                /* its rows of edges, or its entries of run_start */
  int32_t H;                         /* height of its image: t = x*H + y */
  int32_t pad_[3];
} segk_rast_shape;
typedef struct segk_rast_tile {      /* one tile; 32 bytes, 8-byte aligned */
  int64_t out_off;                   /* byte offset of the image (uint8 [H][W], dense) in out */
  int32_t H, W;                      /* 1..SEGK_RAST_MAX_SIDE */
  int32_t y0, x0;                    /* first row and column of the tile */
  int32_t list0, list1;              /* its entries of shape_list */
} segk_rast_tile;
/* every pixel of every tile = fill, then the shapes shape_list[list0:list1) of the tile in that order, a
 * later shape over an earlier one.  edges int32 [n_edges][4] = (X0, Y0, X1, Y1) with 8 fractional bits, |X| <= 2^22, 16-byte
 * aligned; run_start int32 [n_runs] cumulative run starts, ascending inside a shape.  The tiles of an image must cover it
 * exactly once for its bytes to be written once; a tile record that does not lie inside out[0, out_bytes) writes nothing.
 * n_tiles >= 1, out_bytes >= n_tiles, 0 <= fill <= 255; the table lengths may be 0 but no pointer may be NULL. */
int segk_raster_labels(const segk_rast_tile* tiles, int n_tiles, const segk_rast_shape* shapes, int n_shapes,
                       const int32_t* shape_list, int list_len, const int32_t* edges, int n_edges, const int32_t* run_start,
                       int n_runs, uint8_t* out, long out_bytes, int fill, segk_stream_t s);

/* ---- object-level evaluation: overlap table, IoU > 0.5 matching, Panoptic Quality statistics (the reference
 * has no such code: this replaces a mask.cpu() + labelling + np.unique of combined ids).  Integer arithmetic only, integer
 * atomics only, no float on the device: the result is unique and bit-stable.  No launch waits for another workgroup, the host
 * reads no count back, every device loop is bounded by an argument.
 *
 * A segment id is 0 (nothing), 1..max_components (a labelled component: row id - 1 of its cls array) or max_components + 1 + c
 * (stuff class c); a target segment may also be -1 (void).  Per-segment arrays hold max_components + 8 rows, row r = segment
 * r + 1; the rows in use are 0..num-1 and max_components..max_components+7, the rows between are never read or written.
 *
 * Workspace of segk_pq_pairs: SEGK_PQ_WS_INTS(H, W, max_pairs, max_components) 32-bit words, 16-byte aligned, uninitialised,
 * scratch of one call (segk_pq_match needs none; max_components is part of the macro so that it may).  In words, with
 * S = SEGK_PQ_SLOTS(max_pairs) and B = ceil(H*W / 32): 16 (word 0: the overflow flag) | keys uint64 [S] | counts [S] | first
 * pixels [S] | leader bitmap [R4(B)] | leaders before each bitmap word [R4(B)] | leaders per chunk [R4(ceil(B / 1024))]. */
#define SEGK_PQ_BLOCK_PIXELS 2048    /* pixels one workgroup of the insert pass collapses */
#define SEGK_PQ_LDS_SLOTS 256        /* slots of its LDS table */
#define SEGK_PQ_CHUNK 1024           /* bitmap words (32 pixels each) one workgroup counts and scans */
#define SEGK_PQ_MIN_SLOTS 1024
#define SEGK_PQ_STAT_COLS 16
#define SEGK_PQ_MAX_PAIRS (1L << 28)
#define SEGK_PQ_SLOTS(MP) (2L * (long)(MP) + SEGK_PQ_MIN_SLOTS)
#define SEGK_PQ_WS_INTS(H, W, MP, MC)                                                                            \
  (16L + 4L * SEGK_PQ_SLOTS(MP) + 2L * SEGK_VEC_R4(((long)(H) * (long)(W) + 31L) / 32L) +                       \
   SEGK_VEC_R4((((long)(H) * (long)(W) + 31L) / 32L + SEGK_PQ_CHUNK - 1L) / SEGK_PQ_CHUNK) + 0L * (long)(MC))
/* DESIGN.md 3.19 "segments", "void", "pair table": pred / target uint8 [H,W] masks with their label maps int32 [H,W] and
 * component counts num[1] (segk_cc_label with the thing classes, or instance ids given by the caller; a label outside 1..num
 * counts as 0).  A pixel with label 0 whose value is a class of stuff_mask belongs to that stuff segment.  A target pixel whose
 * value is ignore_index (-1: none) or >= 8 is void.  pair_g / pair_p / pair_n [max_pairs]: every distinct (target segment,
 * predicted segment) with its pixel count, in ascending order of the pair's first pixel; totals[0] = P.  If P > max_pairs or
 * either num > max_components: totals[0..3] = -1 and no pair array is touched.  Nothing at or past P is written.
 * H*W <= SEGK_CC_MAX_PIXELS, 1 <= max_components <= 2^24, 1 <= max_pairs <= SEGK_PQ_MAX_PAIRS.  The inputs are only read. */
int segk_pq_pairs(const uint8_t* pred, const int32_t* pred_labels, const int32_t* pred_num, const uint8_t* target,
                  const int32_t* target_labels, const int32_t* target_num, int32_t* pair_g, int32_t* pair_p, int32_t* pair_n,
                  int32_t* totals, int32_t* ws, int H, int W, int stuff_mask, int ignore_index, int max_components,
                  int max_pairs, segk_stream_t s);
/* DESIGN.md 3.19 "areas", "match", "statistics", "totals": from the pair table of segk_pq_pairs (same totals, capacities and
 * num words) and the cls arrays [max_components] of both labellings.  area_g / match_g / inter_g / union_g and area_p / void_p
 * / match_p [max_components + 8]: match is the matched segment id of the other side (0: none), inter and union those of the
 * match (0: none).  totals[1..3] = target segments, predicted segments, matches (segments with area > 0).  stats int64 [8][16],
 * 8-byte aligned, is ADDED to and never zeroed: row = class, columns TP, FP, FN, sum of floor(inter 2^32 / union), TP at
 * IoU >= 0.50 + 0.05 k (k = 0..9), target segments, predicted segments.  A segment whose class is outside 0..7 matches nothing
 * and is counted nowhere.  Returns at once, touching nothing, when totals[0] < 0. */
int segk_pq_match(const int32_t* pair_g, const int32_t* pair_p, const int32_t* pair_n, int32_t* totals, const int32_t* pred_cls,
                  const int32_t* pred_num, const int32_t* target_cls, const int32_t* target_num, int32_t* area_g,
                  int32_t* match_g, int32_t* inter_g, int32_t* union_g, int32_t* area_p, int32_t* void_p, int32_t* match_p,
                  int64_t* stats, int max_components, int max_pairs, segk_stream_t s);

/* ---- mask morphology: erode, dilate, open, close, void band, capped boundary distance, hole fill (the
 * reference has no such code: this replaces a mask.cpu() + scipy.ndimage / cv2 post-process).  Integer arithmetic only: results
 * are unique and bit-stable.  No workgroup waits for another, no atomics on global memory in segk_morph, the host reads nothing
 * back, every device loop is bounded by an argument.  No entry needs a workspace; segk_morph uses SEGK_MORPH_LDS_BYTES(radius)
 * bytes of dynamic LDS: 16-bit keys of the tile with its halo, a byte of column distance per cell of the tile's rows, the tile's
 * own bytes (69632 at radius 32: the entry raises the kernel's limit, two workgroups still share a CU). */
#define SEGK_MORPH_TILE_H 64
#define SEGK_MORPH_TILE_W 128
#define SEGK_MORPH_MAX_RADIUS 32
#define SEGK_MORPH_SQUARE 0          /* dist(dx, dy) = max(|dx|, |dy|), fires at <= r */
#define SEGK_MORPH_DIAMOND 1         /* |dx| + |dy|, fires at <= r */
#define SEGK_MORPH_DISK 2            /* dx dx + dy dy, fires at <= r r */
#define SEGK_MORPH_WILD 0xFFFFu      /* the key that differs from nothing (and that pixels outside the image have) */
#define SEGK_MORPH_FAR 0xFFFF        /* dist of a pixel that does not fire */
#define SEGK_MORPH_LDS_BYTES(r) \
  ((SEGK_MORPH_TILE_H + 2 * (r)) * (SEGK_MORPH_TILE_W + 2 * (r)) * 2 + SEGK_MORPH_TILE_H * (SEGK_MORPH_TILE_W + 2 * (r)) + \
   SEGK_MORPH_TILE_H * SEGK_MORPH_TILE_W)
/* DESIGN.md 3.21 "the primitive", "write rule": mask [H,W] uint8; key uint16 [256] and fire uint8 [256] are DEVICE tables
 * indexed by a pixel's byte.  D(p) = the minimum of dist(p, q) over the pixels q inside the image with key[mask[q]] !=
 * key[mask[p]], neither key being SEGK_MORPH_WILD; p fires when D(p) <= radius (disk: radius squared).
 *   out  [H,W] uint8 (may be NULL): without paint, `value` where p fires and fire[mask[p]] is set, else mask[p]; with paint
 *        [H,W] uint8, paint[p] where p fires, fire[mask[p]] is set and key[paint[p]] != key[mask[p]], else mask[p]
 *   dist [H,W] uint16 (may be NULL): D(p) (squared for the disk) where p fires, else SEGK_MORPH_FAR
 * At least one of out and dist; out is neither mask nor paint; 1 <= radius <= SEGK_MORPH_MAX_RADIUS; H*W <=
 * SEGK_CC_MAX_PIXELS; 0 <= value <= 255; key and dist 2-byte aligned.  The inputs are only read. */
int segk_morph(const uint8_t* mask, const uint8_t* paint, uint8_t* out, uint16_t* dist, const uint16_t* key,
               const uint8_t* fire, int value, int metric, int radius, int H, int W, segk_stream_t s);
/* dst[i] = lut[src[i]] for n bytes; lut uint8 [256] on the device; 1 <= n <= SEGK_CC_MAX_PIXELS; dst is not src. */
int segk_byte_lut(const uint8_t* src, uint8_t* dst, const uint8_t* lut, long n, segk_stream_t s);
/* DESIGN.md 3.21 "holes": after segk_cc_label (same H, W, max_components; labels, num, area, box, first are its outputs) on the
 * map in which the complement of the class set is one class.  out [H,W] uint8 (not the mask) = value where the pixel's
 * component id is in 1..min(num, max_components), its box touches no image border (y0 > 0, x0 > 0, y1 < H, x1 < W) and its area
 * is <= max_area; else mask[p].  filled[0] += the number of such components (the caller zeroes it).  box 16-byte aligned. */
int segk_fill_holes(const uint8_t* mask, const int32_t* labels, const int32_t* num, const int32_t* area, const int32_t* box,
                    const int32_t* first, uint8_t* out, int32_t* filled, int value, int max_area, int H, int W,
                    int max_components, segk_stream_t s);

/* ---- mixed-sample augmentation: CutMix, ClassMix, object copy-paste (the reference only puts two images side
 * by side).  Every output value is a copy of one input value and the paste bit m(y, x) is defined in integers, so results are
 * unique and bit-stable.  The host reads nothing back.  One descriptor per sample lives in DEVICE memory where the entries cannot
 * see it: the kernels clamp the partner to 0..n-1 and the slot to 0..n_slots-1 and treat an unknown mode as SEGK_MIX_NONE; every
 * address is formed from an entry argument that was checked. */
#define SEGK_MIX_NONE 0
#define SEGK_MIX_BOX 1
#define SEGK_MIX_CLASS 2
#define SEGK_MIX_OBJECT 3
#define SEGK_MIX_TILE_H 16           /* segk_mix_apply: one workgroup per tile, a thread takes four pixels of a row */
#define SEGK_MIX_TILE_W 64
#define SEGK_MIX_MAX_OBJECTS 32
#define SEGK_MIX_MAX_COMPONENTS 65536    /* ids fit the low 24 bits of a key */
#define SEGK_MIX_ROW_INTS(cap) (4 + 2 * (cap))   /* one slot of cc_rows: num, three unused words, cls [cap], area [cap] */
#define SEGK_MIX_STAGE_BYTES 0
#define SEGK_MIX_STAGE_SELECT 1
typedef struct segk_mix_desc {   /* one sample; 64 bytes */
  uint64_t seed;                 /* of the selection keys */
  int32_t mode;                  /* SEGK_MIX_* */
  int32_t partner;               /* sample that is pasted from; may be the sample itself */
  int32_t flip;                  /* 0 | 1: the partner is mirrored horizontally */
  int32_t dy, dx;                /* output (y, x) looks at partner (y - dy, flip ? W - 1 - (x - dx) : x - dx) */
  int32_t y0, x0, y1, x1;        /* SEGK_MIX_BOX, output coordinates, y1 and x1 exclusive */
  int32_t slot;                  /* SEGK_MIX_OBJECT: which id map and cc_rows slot hold the partner's components */
  int32_t pad_[4];
} segk_mix_desc;
/* DESIGN.md 3.22 "selection".  y: labels [n][H][W] of label_bytes 1 (uint8) or 8 (int64); a value outside 0..255 is "outside".
 * stage SEGK_MIX_STAGE_BYTES: descs is a table of n_desc slot owners (mode SEGK_MIX_OBJECT); bytes [n_slots][H][W] of slot
 *   descs[i].slot = the partner's labels as bytes, outside -> 255 (what segk_cc_label then reads).  Slots are distinct.
 * stage SEGK_MIX_STAGE_SELECT: one workgroup per sample i < n_desc = n writes select[i * select_stride ..]:
 *   SEGK_MIX_CLASS   256 bytes: candidates = the byte values that occur in the partner's labels and have exclude[v] == 0 (exclude
 *                    uint8 [256] on the device); k = n_classes > 0 ? min(count, n_classes) : ceil(count / 2); byte v = 1 for the
 *                    k candidates with the smallest key(v) = (splitmix(seed, v) & ~0xFFFFFF) | v, else 0
 *   SEGK_MIX_OBJECT  max_components bytes: cc_rows int32 [n_slots][SEGK_MIX_ROW_INTS(max_components)] holds num / cls / area of
 *                    segk_cc_label per slot; candidates = the ids 1..min(num, max_components) with bit cls of things_mask set and
 *                    min_area <= area <= max_area; k = min(count, max_objects); byte id - 1 = 1 for the k smallest key(id)
 *   other modes      nothing is written
 * No atomics on global memory, no workgroup waits for another, loops are bounded by H W and max_components.  n <= 65535, H W <=
 * SEGK_CC_MAX_PIXELS, select_stride >= 256 (and >= max_components when n_slots > 0), 1 <= max_objects <= SEGK_MIX_MAX_OBJECTS,
 * 1 <= max_components <= SEGK_MIX_MAX_COMPONENTS. */
int segk_mix_select(const segk_mix_desc* descs, int n_desc, int n, const void* y, int label_bytes, int H, int W,
                    const uint8_t* exclude, int n_classes, const int32_t* cc_rows, int n_slots, int things_mask, int min_area,
                    int max_area, int max_objects, int max_components, uint8_t* bytes, uint8_t* select, int select_stride,
                    int stage, segk_stream_t s);
/* DESIGN.md 3.22 "geometry", "paste bit", "write rule".  X: images, elem_bytes 4 or 2: [n][C][H][W]; elem_bytes 1: [n][H][W][C]
 * (uint8); 1 <= C <= 4.  y / y_out: labels [n][H][W] of label_bytes 1 or 8.  ids int32 [n_slots][H][W]: labels of segk_cc_label
 * (may be NULL when n_slots == 0).  m(y, x) = 0 where the partner pixel lies outside the image, else BOX: the box test; CLASS:
 * select[label byte]; OBJECT: select[id - 1] for 1 <= id <= max_components.  X_out / y_out at (y, x) = the partner's at the source
 * pixel where m = 1, else the sample's own; with has_seam, y_out = seam_value where a 4-neighbour inside the image has another m.
 * pasted int32 [n] += sum of m (the caller zeroes it; one add per workgroup).  Every output element is written once.  The outputs
 * overlap no input and not each other; X, X_out aligned to elem_bytes, y, y_out to label_bytes, pasted and ids to 4. */
int segk_mix_apply(const segk_mix_desc* descs, int n, const void* X, const void* y, void* X_out, void* y_out, int32_t* pasted,
                   int C, int H, int W, int elem_bytes, int label_bytes, const uint8_t* select, int select_stride,
                   const int32_t* ids, int n_slots, int max_components, int has_seam, long seam_value, segk_stream_t s);

/* ---- boundary quality: Boundary IoU, band IoU, contour distances, HD95 (the reference has none of it).  Built
 * on the primitive of 3.21 and nothing wider: every quantity is an integer count, the result is unique and bit-stable (integer
 * atomics only, a few per workgroup).  No workgroup waits for another, the host reads nothing back, every device loop is bounded
 * by an argument or the tile, no float on the device. */
#define SEGK_BOUNDARY_TILE_H 64
#define SEGK_BOUNDARY_TILE_W 128
#define SEGK_BOUNDARY_MAX_WIDTH 32        /* of width and of max_distance */
#define SEGK_BOUNDARY_BINS 34             /* distance bins 0..32 and room for the overflow bin max_distance + 1 */
#define SEGK_BOUNDARY_HIST_WORDS (2 * SEGK_MAX_CLASSES * SEGK_BOUNDARY_BINS)   /* [2][8][34]: pred->label, label->pred */
/* the statistics: int64 words, [8] per class unless said */
#define SEGK_BOUNDARY_BAND_G 0            /* #{G = c, Dg <= width} */
#define SEGK_BOUNDARY_BAND_P 8            /* #{P = c, Dp <= width} */
#define SEGK_BOUNDARY_BAND_I 16           /* #{G = c = P, Dg <= width, Dp <= width} */
#define SEGK_BOUNDARY_CONF 24             /* [8][8]: #{G = g, P = p, Dg <= width} */
#define SEGK_BOUNDARY_HD_SUM 88           /* sum over images of the per-image HD95 (whole pixels) */
#define SEGK_BOUNDARY_HD_IMAGES 96        /* images that sum is over */
#define SEGK_BOUNDARY_HD_CAPPED 104       /* images whose HD95 fell in the overflow bin */
#define SEGK_BOUNDARY_HIST 112            /* [2][8][34] */
#define SEGK_BOUNDARY_STAT_WORDS (SEGK_BOUNDARY_HIST + SEGK_BOUNDARY_HIST_WORDS)
#define SEGK_BOUNDARY_HALO(width, max_distance) (((width) > (max_distance) ? (width) : (max_distance)) + 1)
/* dynamic LDS of segk_boundary_stats: 2 C class planes, 2 non-void planes and 2 contour planes of 64-bit words, four words per
 * staged row */
#define SEGK_BOUNDARY_LDS_BYTES(C, halo) ((2 * (C) + 4) * (SEGK_BOUNDARY_TILE_H + 2 * (halo)) * 32)
/* DESIGN.md 3.23 "void", "band distance", "band counts", "band confusion", "contours", "contour distance histogram" for one
 * image pair.  pred, label [H,W] uint8, only read.  A label >= num_classes or with its bit of ignore_mask (bits 0..7) set is
 * void in both maps; a pred >= num_classes is void in pred.  The band counts and the confusion are ADDED to stats (int64
 * [SEGK_BOUNDARY_STAT_WORDS]), the histogram to image_hist (int64 [SEGK_BOUNDARY_HIST_WORDS], zero before the image's first
 * call; segk_boundary_finish clears it).  1 <= num_classes <= SEGK_MAX_CLASSES; metric SEGK_MORPH_SQUARE / _DIAMOND / _DISK;
 * 1 <= width, max_distance <= SEGK_BOUNDARY_MAX_WIDTH; image_border 0 | 1; H*W <= SEGK_CC_MAX_PIXELS; stats and image_hist
 * 8-byte aligned and distinct. */
int segk_boundary_stats(const uint8_t* pred, const uint8_t* label, int64_t* stats, int64_t* image_hist, int num_classes,
                        int ignore_mask, int metric, int width, int max_distance, int image_border, int H, int W,
                        segk_stream_t s);
/* DESIGN.md 3.23 "per-image HD95": from image_hist per class c < num_classes, n = both directions' total over bins
 * 0..max_distance + 1; if n > 0, t = the smallest bin with 20 cum >= 19 n: t == max_distance + 1 adds 1 to HD_CAPPED[c], else t
 * to HD_SUM[c] and 1 to HD_IMAGES[c].  Then stats' histogram += image_hist and image_hist = 0.  One workgroup. */
int segk_boundary_finish(int64_t* stats, int64_t* image_hist, int num_classes, int max_distance, segk_stream_t s);

/* ---- superpixels: SLIC in the pixel-centric integer form, and snapping a mask to a segmentation by a per-segment vote
 * (the reference has none of it: this replaces an image.cpu() + skimage.segmentation.slic pass and a host
 * loop over segments).  Integer arithmetic only, ties go to the lowest index, the sums are integer atomics (a few per
 * workgroup): results are unique and bit-stable.  No workgroup waits for another, the host reads nothing back, no float on
 * the device, every device loop is bounded by the step, the tile or 9. */
#define SEGK_SLIC_TILE 64                 /* segk_slic_assign / segk_snap_vote: one workgroup of 256 per tile_rows x 64 pixels;
                                             tile_rows is 4, 16 or SEGK_SLIC_TILE and never shows in a result: the host takes
                                             fewer rows for a small image, so that it still fills the device */
#define SEGK_SLIC_MAX_CELLS 18            /* cells per side a tile and its one-cell ring touch (at step 4) */
#define SEGK_SLIC_MIN_STEP 4
#define SEGK_SLIC_MAX_STEP 64
#define SEGK_SLIC_MAX_COMPACTNESS 255
#define SEGK_SLIC_MAX_ITERATIONS 20
#define SEGK_SLIC_MAX_SIDE (1 << 27)      /* 16 H and 16 W fit an int32 centre */
#define SEGK_SLIC_RGB 0
#define SEGK_SLIC_YCC 1
#define SEGK_SLIC_CENTRE_WORDS 5          /* Y, X, C0, C1, C2 in 1/16 units */
#define SEGK_SLIC_SUM_WORDS 8             /* n, sum of y - (i - 1) S, of x - (j - 1) S, of c0, c1, c2, two unused words */
#define SEGK_SNAP_NONE 255                /* paint[k] of a segment that is not painted */
/* DESIGN.md 3.24 "features", "grid", "start centre".  image [H,W,C] uint8, C in {1, 3, 4} (a fourth channel is ignored), only
 * read.  K = ceil(H / step) ceil(W / step).  centres int32 [K][5] = the start centres; sums int32 [K][8] = 0.  space
 * SEGK_SLIC_RGB | _YCC; SEGK_SLIC_MIN_STEP <= step <= SEGK_SLIC_MAX_STEP; H*W <= SEGK_CC_MAX_PIXELS; H, W <=
 * SEGK_SLIC_MAX_SIDE; centres 4-byte, sums 16-byte aligned. */
int segk_slic_start(const uint8_t* image, int32_t* centres, int32_t* sums, int C, int space, int step, int H, int W, int K,
                    segk_stream_t s);
/* DESIGN.md 3.24 "assignment", "sums": round `round` (0 .. iterations - 1) of `iterations` (1 .. SEGK_SLIC_MAX_ITERATIONS).
 * Every pixel takes the candidate of smallest D, the lowest index on a tie; n and the sums of its pixels are ADDED to
 * sums[k] (positions as offsets from the origin of the cell before the home cell, so they fit 32 bits).  labels int32 [H,W]
 * is written in the last round only.  1 <= compactness <= SEGK_SLIC_MAX_COMPACTNESS; tile_rows 4, 16 or SEGK_SLIC_TILE; the
 * rest as segk_slic_start; labels 4-byte aligned.  Uses no dynamic LDS. */
int segk_slic_assign(const uint8_t* image, const int32_t* centres, int32_t* sums, int32_t* labels, int C, int space, int step,
                     int compactness, int round, int iterations, int tile_rows, int H, int W, int K, segk_stream_t s);
/* DESIGN.md 3.24 "update": counts[k] = n; with n > 0 every component of centres[k] = floor((32 sum + n) / (2 n)) of the
 * true sum, else it stays; sums[k] = 0.  K threads. */
int segk_slic_update(int32_t* centres, int32_t* sums, int32_t* counts, int step, int H, int W, int K, segk_stream_t s);
/* DESIGN.md 3.24 "vote": hist int64 [K][8] (the caller zeroes it): hist[labels[p]][mask[p]] += weights ? weights[p] : 1 for
 * the pixels with 0 <= labels[p] < K and mask[p] < 8 with its bit of classes_mask (1..255) set.  labels int32 [H,W], mask
 * and weights (may be NULL) uint8 [H,W], only read.  1 <= K <= SEGK_CC_MAX_PIXELS >= H*W; tile_rows 4, 16 or SEGK_SLIC_TILE;
 * hist 8-byte, labels 4-byte aligned. */
int segk_snap_vote(const int32_t* labels, const uint8_t* mask, const uint8_t* weights, int64_t* hist, int classes_mask,
                   int tile_rows, int H, int W, int K, segk_stream_t s);
/* DESIGN.md 3.24 "winner", "snap".  winner int32 [K] = the class of the largest entry of hist[k], the lowest on a tie, -1 for
 * a row of zeros; paint uint8 [K] (scratch) = winner[k] when 256 hist[k][winner] >= min_share sum_c hist[k][c], else
 * SEGK_SNAP_NONE.  out [H,W] uint8 = paint[labels[p]] where 0 <= labels[p] < K, that is not SEGK_SNAP_NONE and bit mask[p] of
 * the 256-bit set allow0..allow3 (allow0 bit 0 = value 0) is set; else mask[p].  0 <= min_share <= 256; out is neither mask
 * nor paint; hist 8-byte, labels and winner 4-byte aligned.  Two launches. */
int segk_snap_paint(const int32_t* labels, const uint8_t* mask, const int64_t* hist, int32_t* winner, uint8_t* paint,
                    uint8_t* out, long allow0, long allow1, long allow2, long allow3, int min_share, int H, int W, int K,
                    segk_stream_t s);

/* ---- output head: Conv2d(C, ncls, 1) (unet.py:91,105; clipunet.py:181,187) ----------------------- */
/* y NHWC [B,H,W,Cp] -> logits NCHW fp32 [B,ncls,H,W];  w fp32 [ncls][C], bias [ncls] */
int segk_head_fwd(const void* y, const float* w, const float* bias, float* logits, int B, int H, int W, int Cp,
                  int C, int ncls, int dtype, segk_stream_t s);
int segk_head_part_floats(long P, int Cp);
int segk_head_bwd(const float* dlogits, const void* y, const float* w, void* dy, float* part, float* dw, float* db,
                  int B, int H, int W, int Cp, int C, int ncls, int dtype, segk_stream_t s);

/* segk_head_bwd that also accumulates the BatchNorm backward reductions of the DoubleConv block whose output y the head
 * reads (unet.py:103-105: up4 -> output): bnpart holds segk_head_bwd_blocks(P) rows of [Cp][2] floats for
 * segk_bn_relu_bwd_from_part */
int segk_head_bwd_blocks(long P);
int segk_head_bwd_bnstat(const float* dlogits, const void* y, const float* w, void* dy, float* part, float* dw, float* db,
                         int B, int H, int W, int Cp, int C, int ncls, const float* scale, const float* shift,
                         const float* mean, const float* rstd, float* bnpart, int dtype, segk_stream_t s);

/* The same head reading the block's PRE-ACTIVATION z instead of its output (unet.py:103-105: the output of up4 is
 * consumed by the head alone, so relu(z * scale + shift) -- rounded to `dtype` exactly as segk_bn_relu_apply stores it --
 * is re-formed inside both kernels and never written): forward, and backward writing the gradient of that (virtual)
 * output to dy; bnpart (may be NULL) receives the BatchNorm backward reductions with xhat = (z - mean) * rstd. */
int segk_head_fwd_bn(const void* z, const float* scale, const float* shift, const float* w, const float* bias, float* logits,
                     int B, int H, int W, int Cp, int C, int ncls, int dtype, segk_stream_t s);
int segk_head_bwd_bn(const float* dlogits, const void* z, const float* w, void* dy, float* part, float* dw, float* db,
                     int B, int H, int W, int Cp, int C, int ncls, const float* scale, const float* shift,
                     const float* mean, const float* rstd, float* bnpart, int dtype, segk_stream_t s);

/* The output layer's backward without a stored gradient of the block output (unet.py:20-21 of up4 behind :91,105; that
 * gradient is Wt . dlogits, three multiply-adds per channel, and has one consumer).  segk_head_bwd_bn_stats is segk_head_bwd_bn
 * minus the store of dy: the dW / db partials and the BatchNorm partial rows bnpart are the same values in the same order.
 * segk_head_bn_bwd_apply finishes bnpart (nb = segk_head_bwd_blocks(P) rows) into dgamma, dbeta, coef like
 * segk_bn_relu_bwd_from_part and writes dz [B,H,W,Cp], re-forming each dy element from dlogits and w exactly as
 * segk_head_bwd_bn computes and rounds it: dz is bit-identical to the two-entry sequence.  dz must not alias z. */
int segk_head_bwd_bn_stats(const float* dlogits, const void* z, const float* w, float* part, float* dw, float* db, int B, int H,
                           int W, int Cp, int C, int ncls, const float* scale, const float* shift, const float* mean,
                           const float* rstd, float* bnpart, int dtype, segk_stream_t s);
int segk_head_bn_bwd_apply(const float* dlogits, const void* z, const float* w, void* dz, const float* scale, const float* shift,
                           const float* mean, const float* rstd, int B, int H, int W, int Cp, int C, int ncls,
                           const float* bnpart, int nb, float* dgamma, float* dbeta, float* coef, int dtype, segk_stream_t s);

/* ---- per-pixel CrossEntropy + soft Dice (training.py:47; utils/weighted_loss.py:31-98,140-166) ----
 * logits NCHW fp32 [N,C,HW], labels int64 [N,HW].  state (segk_loss_state_floats() floats):
 * [0]=dice_weight*dice+ce_weight*ce, [1]=ce, [2]=dice, rest = saved statistics for backward.
 * ignore_index < 0: none.  class_weights may be NULL. */
int segk_loss_part_floats(long P);
int segk_loss_state_floats(void);
int segk_loss_fwd(const float* logits, const int64_t* labels, const float* class_weights, int N, int C, long HW,
                  int ignore_index, float smooth, float dice_weight, float ce_weight, float* part, float* state,
                  float* loss_out, segk_stream_t s);   /* loss_out (may be NULL): one float, a copy of state[0] (the value the
                                                          nn.Module returns, in a buffer of its own); the block of the
                                                          launch that finishes last turns the partials into the state */
int segk_loss_bwd(const float* logits, const int64_t* labels, const float* class_weights, const float* state,
                  const float* grad_out, int N, int C, long HW, int ignore_index, float dice_weight, float ce_weight,
                  float* dlogits, segk_stream_t s);

/* ---- distillation: fused multi-teacher soft-target loss (the reference holds no code for it) ----
 * student fp32 [N,C,H,W] logits; V teacher tensors fp32 [N,C,H,W] named by a DEVICE table of V descriptors (16-byte aligned;
 * the host never reads it, so its contents are the caller's to get right: image_segmentation_amd/distill.py: teacher_table);
 * labels int64 [N,H,W] or NULL. */
typedef struct segk_teacher_desc {   /* one teacher view; 32 bytes, 16-byte aligned */
  uint64_t ptr;                      /* device address of the teacher's fp32 [N,C,H,W] output */
  int32_t flip;                      /* bit 0: the view saw the batch reversed in x, bit 1: in y */
  int32_t kind;                      /* 0: logits, 1: probabilities, taken as z = logf(fmaxf(t, 2^-126)) */
  float weight;                      /* w_v / sum of the weights, rounded once from float64 */
  int32_t pad_[3];
} segk_teacher_desc;
/* Per pixel (b, y, x), for v = 0..V-1 in table order and in fp32: z_v = teacher v at (flip & 2 ? H-1-y : y, flip & 1 ? W-1-x : x),
 * q += weight_v * softmax(z_v * inv_T), q1 += weight_v * softmax(z_v) (the same numbers as q when inv_T == 1.0f); p = softmax(s *
 * inv_T).  The pixel COUNTS when (labels == NULL or label != ignore_index) and max_k q1_k >= min_conf.  KL = sum_k q_k (logf(q_k)
 * - log p_k), terms with q_k == 0 being 0.  state (segk_loss_state_floats() floats): [0] = soft = T_sq * sum KL / n, [1] = n, the
 * number of counted pixels, [2] = sum KL, [3] = n_agree, the counted pixels with argmax p == argmax q (first maximum, NaN maximal),
 * the rest 0; n == 0 gives soft = 0 exactly.  loss_out (may be NULL): a copy of state[0].  part: segk_loss_part_floats(N H W)
 * floats of scratch.  No float atomics: the block that finishes last sums the block partials in float64 in one fixed order.
 * 1 <= C <= 8, 1 <= V <= SEGK_MAX_VIEWS, N H W < 2^31, inv_T and T_sq positive and finite, min_conf finite; every scalar and
 * every host-visible pointer is validated (-2 before any launch). */
int segk_distill_fwd(const float* student, const void* teachers_dev, int V, const int64_t* labels, int N, int C, int H, int W,
                     int ignore_index, float inv_T, float T_sq, float min_conf, float* part, float* state, float* loss_out,
                     segk_stream_t s);
/* dstudent [N,C,H,W] = grad_out[0] * T_sq * inv_T / n * (p - q) at counted pixels, exactly 0 elsewhere (and everywhere when
 * n == 0); q is formed again by the code the forward pass ran, from the same arguments.  Teachers get no gradient. */
int segk_distill_bwd(const float* student, const void* teachers_dev, int V, const int64_t* labels, const float* state,
                     const float* grad_out, int N, int C, int H, int W, int ignore_index, float inv_T, float T_sq, float min_conf,
                     float* dstudent, segk_stream_t s);

/* ---- hard-pixel losses: label smoothing, focal modulation, OHEM selection ----------------------------
 * logits fp32 [N,C,HW], 1 <= C <= 8; labels int64 [N,HW]; N HW < 2^31; class_weights [C] or NULL (all 1); ignore_index < 0: none.
 * A pixel COUNTS when 0 <= y < C and y != ignore_index; n = the counted pixels.  Per counted pixel, in fp32, classes in order:
 * m = max z, e_k = expf(z_k - m), se = sum e_k, lse = logf(se), nl_k = lse - (z_k - m), p_k = e_k * (1 / se);
 *   key   kappa = nl_t, a negative value clamped to 0, a NaN kept;
 *   ce    = sum_k a_k nl_k with a_k = [k = t] ((1 - eps) w_t) + (eps / C) w_k, eps = label_smoothing in [0, 1); for eps == 0
 *           exactly w_t nl_t, segk_loss_fwd's term;
 *   l     = powf(u, gamma) ce with u = sum_{k != t} p_k, gamma == 0 or in [1, 8] (gamma == 0: l = ce, no powf).
 * select != 0 keeps the pixels with kappa >= tau = min(theta, k-th largest key), k = min(n, max(min_kept, ceil(f n))) with
 * f = min_frac_q16 / 65536 and the ceiling as (n q + 65535) >> 16 in 64-bit integers (k == 0: tau = theta); theta >= 0 is
 * -log(thresh), +inf for none; ties at the k-th key are all kept and a NaN key orders above +inf.  select == 0 keeps every
 * counted pixel.  loss = (float)(S / D), S = sum of l and D = sum of w_t over the kept pixels, summed in segk_loss_fwd's order
 * and finished in float64 by the block that arrives last; D == 0: NaN when n == 0, else exactly 0.  With everything off
 * state[0] carries segk_loss_fwd's bits (dice_weight 0, ce_weight 1).
 * keys [N HW] uint32, needed iff select != 0 and saved for backward: bits(kappa) + 1 of a counted pixel, 0x7FC00001 for a NaN
 * key, 0 for a pixel that does not count (non-negative floats order as their bits).  hist: SEGK_HARD_HIST_WORDS uint32 of
 * scratch, 16-byte aligned, needed iff select != 0, zeroed by the entry on the stream.  part: segk_loss_part_floats(N HW),
 * state: segk_loss_state_floats() floats: [0] loss, [1] S, [3] D, [4] tau, [5] the word of tau, [6] n, [7] the kept pixels
 * ([5..7] as uint32 bits; select == 0: tau = 0, word 1), the rest 0.  loss_out (may be NULL): a copy of state[0].
 * The selection is exact (three histogram passes over the words, 11 + 11 + 10 bits): no sort, no host sync, no float atomics.
 * Every scalar and every host-visible pointer is validated (-2 before any launch). */
#define SEGK_HARD_HIST_WORDS 5136   /* 2048 + 2048 + 1024 bins and 16 control words; a constant, not a query */
int segk_hard_loss_fwd(const float* logits, const int64_t* labels, const float* class_weights, int N, int C, long HW,
                       int ignore_index, float label_smoothing, float gamma, int select, float theta, int min_kept,
                       int min_frac_q16, uint32_t* keys, uint32_t* hist, float* part, float* state, float* loss_out,
                       segk_stream_t s);
/* dlogits_j = (grad_out[0] / D) g_j at kept pixels (saved word >= the word in state[5]), g_j = mod (A p_j - a_j) - gamma
 * powf(u, gamma - 1) p_t ([j = t] - p_j) ce with A = sum_k a_k and mod = powf(u, gamma) (second term absent for gamma == 0);
 * gamma == 0 and eps == 0: segk_loss_bwd's grad_out ((w_t / D) (p_j - [j = t])).  Exactly 0 at every other pixel and
 * everywhere when D == 0.  Same scalars as the forward call; keys NULL iff select == 0. */
int segk_hard_loss_bwd(const float* logits, const int64_t* labels, const float* class_weights, const uint32_t* keys,
                       const float* state, const float* grad_out, int N, int C, long HW, int ignore_index,
                       float label_smoothing, float gamma, int select, float* dlogits, segk_stream_t s);

/* ---- Lovasz-Softmax loss: device segmented sort, Jaccard scan -----------------------------------------
 * logits fp32 [N,C,HW], 1 <= C <= 8; labels int64 [N,HW]; P = N HW < 2^31; class_weights [C] or NULL (all 1); ignore_index < 0:
 * none.  A pixel COUNTS when 0 <= y < C and y != ignore_index.  per_image 1: S = N segments of L = HW pixels; 0: S = 1, L = P.
 * Per counted pixel, in fp32: m = max z, e_k = expf(z_k - m), se = sum e_k, p_k = e_k * (1 / se); for every class c, fg =
 * [y = c] and err_c = fg ? sum_{k != c} p_k (class order from 0.f, never 1 - p_c) : p_c.  Sort word: bits(err_c) + 1, 0x3FFFFFFF
 * for a NaN error, 0 for a pixel that does not count; payload (fg << 31) | index-in-segment.  Inside every (segment s, class c)
 * the slots are ordered by word descending, ties by index ascending (a stable sort: the permutation is unique).  With G = the fg
 * slots of (s, c) and F_i = the fg slots among the sorted positions 1..i, in float64 from integers: J_i = 1 - (G - F_i) /
 * (G + i - F_i), J_0 = 0, g_i = J_i - J_{i-1}; L_{s,c} = sum_i (double)err_i g_i over the counted slots, err_i the value of the
 * word (NaN for the NaN word), summed per tile of SEGK_LOVASZ_TILE sorted slots and over the tiles in one fixed order.
 * Class c ENTERS segment s iff s has a counted pixel and (classes == SEGK_LOVASZ_ALL or G_{s,c} > 0).  loss_s = sum_{c enters}
 * w_c L_{s,c} / sum_{c enters} w_c (0 when no class enters or the weights sum to 0); loss = (float)((1 / S) sum_s loss_s): exactly
 * 0 when no pixel counts (not CrossEntropy's NaN), NaN when an error is NaN.
 * coef fp32 [C][P] (class-major, pixel order), written everywhere: (float)g_i, negated when fg, at the pixel sorted to position i;
 * exactly 0 at pixels that do not count.  state: SEGK_LOVASZ_STATE_DOUBLES(C, S) float64: [0] loss, [1] the counted pixels, then
 * four [S][C] tables -- L_{s,c}; a_{s,c} = (float)(w_c / (S sum_{c' enters} w_c')) for entering classes, else 0; G_{s,c}; 1 where
 * c enters -- then n_s [S].  loss_out (may be NULL): the loss.
 * scratch: SEGK_LOVASZ_SCRATCH_BYTES(C, P, S) bytes, 16-byte aligned, nothing in it needs a value before the call; a smaller
 * scratch_bytes is refused.  With T = SEGK_LOVASZ_TILE, TS = ceil(L / T), NT = C S TS, as uint32 words in this order: the float64
 * tile sums [2 NT]; sorted words [C P] and sorted payloads [C P] (segment (s, c) at slot (c S + s) L); their second copies
 * [C P], [C P]; the tile digit tables [256 NT]; the segment digit totals [256 C S]; the tile fg counts, exclusive over a segment
 * [NT]; the tile counted slots [NT]; G [C S] and the counted slots [C S] by segment c S + s.
 * Kernels: keys, four radix passes (8 bits: tile histogram, scan over the tiles, ranked scatter), count, scan, terms; the block of
 * the terms pass that arrives last finishes.  No workgroup waits for another, no host sync, no float atomics.
 * Every scalar and every host-visible pointer is validated (-2 before any launch). */
#define SEGK_LOVASZ_TILE 2048
#define SEGK_LOVASZ_PRESENT 0
#define SEGK_LOVASZ_ALL 1
#define SEGK_LOVASZ_SCRATCH_WORDS(C, P, S) (4 * (C) * (P) + 260 * (C) * (S) * (((P) / (S) + SEGK_LOVASZ_TILE - 1) / SEGK_LOVASZ_TILE) + 258 * (C) * (S))
#define SEGK_LOVASZ_SCRATCH_BYTES(C, P, S) (4 * SEGK_LOVASZ_SCRATCH_WORDS(C, P, S))   /* 64-bit arguments */
#define SEGK_LOVASZ_STATE_DOUBLES(C, S) (2 + 4 * (C) * (S) + (S))
int segk_lovasz_fwd(const float* logits, const int64_t* labels, const float* class_weights, int N, int C, long HW,
                    int ignore_index, int per_image, int classes, void* scratch, long scratch_bytes, float* coef,
                    double* state, float* loss_out, segk_stream_t s);
/* With t_c = (a_{s,c} coef_c) p_c and A = sum_c t_c (class order from 0.f), all fp32, p formed again by the forward's code:
 * dlogits_j = grad_out[0] (t_j - p_j A) at counted pixels -- the sum over c of a_{s,c} coef_c p_c ([j = c] - p_j) -- and
 * exactly 0 at every other pixel.  coef and state as segk_lovasz_fwd left them; same N, C, HW, ignore_index, per_image. */
int segk_lovasz_bwd(const float* logits, const int64_t* labels, const float* coef, const double* state, const float* grad_out,
                    int N, int C, long HW, int ignore_index, int per_image, float* dlogits, segk_stream_t s);

/* ---- prompt model (prompt_based/prompt.py:33-56; utils/weighted_loss.py:170-343) ---------------------------
 * remix of the frozen 4-class CLIP-UNet softmax with the sigmoid of the 1-channel mask U-Net, fp32 NCHW:
 * final[0] = 1-m; final[1] = m*(p0+p3); final[2] = m*p1; final[3] = m*p2.  Backward: gradient of the mask logit only
 * (the CLIP branch is frozen, prompt.py:30-31). */
int segk_prompt_mix_fwd(const float* clip_logits, const float* mask_logit, float* final_probs, int N, long HW,
                        segk_stream_t s);
int segk_prompt_mix_bwd(const float* clip_logits, const float* mask_logit, const float* dfinal, float* dmask_logit, int N,
                        long HW, segk_stream_t s);
/* WeightedDiceNLLLoss on class probabilities (apply_softmax=False): soft Dice on the values themselves +
 * NLLLoss(weight, ignore_index) of log(p + eps) (nll_log = 1; prompt.ipynb's stable_log) or of p itself (nll_log = 0).
 * part/state sized like segk_loss_fwd's. */
int segk_prob_loss_fwd(const float* probs, const int64_t* labels, const float* class_weights, int N, int C, long HW,
                       int ignore_index, float smooth, float dice_weight, float nll_weight, int nll_log, float eps,
                       float* part, float* state, float* loss_out, segk_stream_t s);
int segk_prob_loss_bwd(const float* probs, const int64_t* labels, const float* class_weights, const float* state,
                       const float* grad_out, int N, int C, long HW, int ignore_index, float dice_weight,
                       float nll_weight, int nll_log, float eps, float* dprobs, segk_stream_t s);

/* ---- point prompts (utils/augmentation.ipynb, cell "Prompt Augmentation": create_gaussian_heatmap, select_dominant_class
 * and the retry loop; prompt_based/prompt.py reads what that cell wrote) ----------------------------------------------------
 * Two host-built tables carry every value that decides a result, indexed by the integer squared distance d2 = dy*dy + dx*dx:
 * w[d2] = exp(-d2 / (2 sigma^2)) in float64 (nw entries) and q[d2] = (uint8)(255 * w[d2]) (nq entries, the non-zero head).
 * labels int64 [B,H,W]; lut (may be NULL): uint8[256] applied to the labels first -- labels outside 0..255 and table results
 * >= SEGK_MAX_CLASSES count as class 0; without a table the labels are the classes.  H, W <= 32768.  Centres, classes and
 * points are device data: a centre outside the image scores nothing, gets class 0, is never taken and makes no heat; every
 * table index is bounded by nw / nq.
 *
 * scores[B,K,8] float64 = per-class sums of w over the window |dy|, |dx| <= R around centers[B,K,2] (int32, y then x) clipped
 * to the image, summed in a fixed order; cls[B,K] int32 = the class 1..7 with the largest sum (the lowest on a tie), 0 when
 * every sum is < 1e-9 (select_dominant_class). */
int segk_prompt_scores(const int64_t* labels, const uint8_t* lut, const int32_t* centers, const double* w, int nw, int R,
                       double* scores, int32_t* cls, int B, int K, int H, int W, segk_stream_t s);
/* the retry loop and the files it writes: per image, candidate k is taken if cls[b][k] is non-zero and not taken yet, until
 * per_image (1..7) are taken.  For the j-th taken candidate: heat[B,per_image,1,H,W] fp32 = (float)q[d2] / 255.0f (0 beyond
 * nq), target[B,per_image,H,W] int64 = label == class ? class : 0, classes[B,per_image] int32, out_centers[B,per_image,2]
 * int32, valid[B] uint8 = 1.  An image with fewer distinct classes gets valid = 0 and zeros everywhere (the reference skips
 * it).  H*W % 4 == 0 takes the 16-byte path (labels, heat, target 16-byte aligned). */
int segk_prompt_make(const int64_t* labels, const uint8_t* lut, const int32_t* centers, const int32_t* cls, const uint8_t* q,
                     int nq, float* heat, int64_t* target, int32_t* classes, int32_t* out_centers, uint8_t* valid, int B, int K,
                     int per_image, int H, int W, segk_stream_t s);
/* prediction side: P points [P,2] (int32, y then x; 1 <= P <= 1024) -> heat[1,H,W] fp32 = (float)q[min over the points of
 * d2] / 255.0f, the maximum of the points' Gaussians; one point gives the training form */
int segk_prompt_heatmap(const int32_t* points, int P, const uint8_t* q, int nq, float* heat, int H, int W, segk_stream_t s);

/* ---- training augmentation and dataset preparation (utils/augmentation.ipynb: the eight imgaug augmenters, each followed by
 * "pad to square, resize to 256"; cell 17 combine_images_preserve_aspect_ratio; utils/utils.py:201-250
 * convert_rgb_label_to_classes; utils/utils.py:117-198 calculate_class_weights) ------------------------------------------------
 * All arithmetic is integer and every deciding value comes from a host-built table, so results are bit-stable; the exact
 * definition is DESIGN.md 3 (and, as NumPy, tests/augment_reference.py).  One launch serves a whole batch of differently sized
 * samples through a descriptor table in DEVICE memory; the entry points cannot see it, so the kernels clamp every coordinate to
 * its buffer and every table row to the table length, and treat an unknown op as SEGK_AUG_RESIZE.  Sides are 1..8192. */
#define SEGK_AUG_RESIZE 0
#define SEGK_AUG_CENTER_CROP 1
#define SEGK_AUG_RANDOM_CROP 2
#define SEGK_AUG_ROTATION 3      /* stage A: bilinear (image) / nearest (label) gather through the Q16 inverse map A */
#define SEGK_AUG_MASKING 4       /* CoarseDropout: cell grid gh x gw, a cell is dropped by the hash of (seed, cell) */
#define SEGK_AUG_GRAYSCALE 5
#define SEGK_AUG_LAPLACE 6       /* per-element noise: row `aux` of the Laplace tables, indexed by the hash of (seed, element) */
#define SEGK_AUG_BLUR 7          /* stage A: 12 x 12 box, reflect-101 borders, image only */
#define SEGK_AUG_CONTRAST 8      /* row `aux` of the contrast tables */
#define SEGK_AUG_LAPLACE_ENTRIES 4096
typedef struct segk_aug_desc {   /* one sample; 160 bytes */
  const uint8_t* img;            /* source image uint8 [H][W][img_c], img_c 3 | 4 (the fourth channel is ignored) */
  const uint8_t* lab;            /* source label uint8 [H][W][lab_c], lab_c 1 (class ids / trimap) | 3 (colour), or NULL */
  uint8_t* a_img;                /* stage-A image [Ha][Wa][3] in caller scratch (rotation, blur), else NULL */
  uint8_t* a_lab;                /* stage-A label [Ha][Wa], colour labels already as classes (rotation), else NULL */
  int64_t A[6];                  /* rotation: SX = A[0] x + A[1] y + A[2], SY = A[3] x + A[4] y + A[5], Q16 */
  uint64_t seed;                 /* per-image seed of the hash (masking, Laplace) */
  int32_t H, W, img_c, lab_c;
  int32_t Ha, Wa;                /* stage-A output size */
  int32_t op;                    /* SEGK_AUG_* */
  int32_t wy, wx, wh, ww;        /* window of stage B in its input (stage-A output if there is one, else the source) */
  int32_t tab, aux;              /* row of the cubic tables (the one built for S = max(wh, ww)); row of the op's own table */
  int32_t gh, gw;                /* masking grid */
  int32_t label_fill;            /* rotation: label value outside the source */
  int32_t pad_[2];
} segk_aug_desc;
/* stage A for `n` samples (only those that have one need to be in the table): a_img (and a_lab) of each are written.
 * max_tiles = the largest ceil(Ha/16) * ceil(Wa/16) of the table.  Rotation: image (sum of w p + 32768) >> 16 with the four
 * integer weights of the 8-bit fractions (SX >> 8) & 255, taps outside the source read 0; label (SX + 32768) >> 16, outside
 * label_fill.  Blur: (sum of rows y-6..y+5, columns x-6..x+5 + 72) / 144. */
int segk_aug_prefilter(const segk_aug_desc* descs, int n, int max_tiles, segk_stream_t s);
/* stage B for `n` samples: window -> pointwise op on every tap -> pad to the square S = max(wh, ww) (centred, 0) -> resize to
 * T x T.  Image: separable cubic from cub_idx int32 [n_cub][T] (floor of the source coordinate) and cub_coef int16
 * [n_cub][T][4] (rows sum to 2048), clamp((sum_r c[r] sum_c c[c] p + 2^21) >> 22, 0, 255), written as X fp32 [n,3,T,T] = u8 /
 * 255.0f (utils/dataset.py:39) and / or X8 uint8 [n,T,T,3] (either may be NULL, not both).  Label: nearest (dst S) / T, the
 * colour -> class map, then label_lut uint8[256] (may be NULL) -> y int64 [n,1,T,T] (may be NULL).  contrast uint8
 * [n_contrast][256], laplace int16 [n_laplace][4096]. */
int segk_aug_resample(const segk_aug_desc* descs, int n, int T, const int32_t* cub_idx, const int16_t* cub_coef, int n_cub,
                      const uint8_t* contrast, int n_contrast, const int16_t* laplace, int n_laplace, const uint8_t* label_lut,
                      float* X, uint8_t* X8, int64_t* y, segk_stream_t s);
typedef struct segk_merge_desc { /* one pair; 64 bytes */
  const uint8_t* img[2];         /* uint8 [H][W][img_c] */
  const uint8_t* lab[2];         /* uint8 [H][W][lab_c]; a one-channel label counts as grey RGB (cell 17 loads RGB); or NULL */
  int32_t H[2], W[2], img_c[2], lab_c[2];
} segk_merge_desc;
/* cell 17 for `n` pairs: tables int32 [n][4][T] = source row of image 0 per canvas row, source column of image 0 per canvas
 * column, the same two for image 1 (-1: none); image 1 is pasted over image 0, the rest of the canvas is 0.  Outputs as
 * segk_aug_resample; the label canvas goes through the colour -> class map, then label_lut. */
int segk_aug_merge(const segk_merge_desc* descs, const int32_t* tables, int n, int T, const uint8_t* label_lut, float* X,
                   uint8_t* X8, int64_t* y, segk_stream_t s);
/* utils.py:166-177: counts[c] += number of labels with clamp(label, 0, num_classes - 1) == c among those != ignore_index (when
 * has_ignore).  labels: n elements of elem_bytes 1 (uint8) or 8 (int64); counts uint64 [num_classes <= 256], caller-zeroed,
 * accumulates across calls; integer sums, so the result does not depend on the order. */
int segk_label_hist(const void* labels, long n, int elem_bytes, int num_classes, int has_ignore, long ignore_index,
                    uint64_t* counts, segk_stream_t s);
/* utils.py:201-250: rgb uint8 [n][3] -> out uint8 [n]: black or white 0, (128,0,0) 1, (0,128,0) 2, else 255 */
int segk_rgb_label_to_classes(const uint8_t* rgb, uint8_t* out, long n, segk_stream_t s);

/* ---- robustness perturbations (report section 4.1 / figure 6; the reference holds no code for them: DESIGN.md 3.x) --------
 * 8-bit interleaved images at their own sizes in, uint8 [H][W][3] out; integer arithmetic and host-built tables only, so the
 * result is bit-stable and independent of the launch shape.  One launch serves a ragged batch: the device table has one
 * entry per image, sorted by tile0, and total_tiles is the sum of the images' tile counts.  A launch applies ONE kind (or one
 * number of blur passes) to all its images: the table lives in device memory, so what the host must validate is an argument. */
#define SEGK_PERTURB_LUT 0           /* out = lut[v]; table: uint8 [256] (contrast, brightness) */
#define SEGK_PERTURB_GAUSS_NOISE 1   /* out = clip(v + tab[hash(seed, e) >> 52], 0, 255), e = (y W + x) 3 + c; table: int16 [4096] */
#define SEGK_PERTURB_SALT_PEPPER 2   /* h = hash(seed, e); (h >> 40) < p0 ? ((h >> 39) & 1 ? 255 : 0) : v; p0 = floor(amount 2^24) */
#define SEGK_PERTURB_OCCLUDE 3       /* rows [p0, p0 + p2) x columns [p1, p1 + p2) become 0 in every channel */
#define SEGK_PERTURB_GAUSS_ENTRIES 4096
#define SEGK_PERTURB_POINT_TILE 4096 /* output bytes per tile of segk_perturb_point: ceil(H W 3 / 4096) tiles per image */
#define SEGK_PERTURB_BLUR_TH 32      /* output rows and columns per tile of segk_perturb_blur: */
#define SEGK_PERTURB_BLUR_TW 64      /*   ceil(H / 32) ceil(W / 64) tiles per image */
#define SEGK_PERTURB_BLUR_MAX 9      /* most passes one launch runs (the halo the tile in LDS is sized for) */
typedef struct segk_perturb_desc {   /* one image; 56 bytes */
  const uint8_t* src;                /* uint8 [H][W][src_c], src_c 3 | 4 (the fourth channel is ignored) */
  uint8_t* dst;                      /* uint8 [H][W][3]; must not overlap src */
  uint64_t seed;                     /* per-image seed of the hash (noise, salt and pepper) */
  int32_t H, W, src_c;               /* H W 3 < 2^31 */
  int32_t tile0;                     /* first tile of this image in the launch */
  int32_t p0, p1, p2;                /* the kind's parameters (above) */
  int32_t pad_;
} segk_perturb_desc;
/* hash = the splitmix64 finaliser of e + seed 0x9E3779B97F4A7C15 (the one of SEGK_AUG_LAPLACE).  table: see the kinds (NULL
 * for salt and pepper and occlusion).  total_tiles == 0 launches nothing. */
int segk_perturb_point(const segk_perturb_desc* descs, int n, int total_tiles, int kind, const void* table, segk_stream_t s);
/* k passes (0..SEGK_PERTURB_BLUR_MAX; 0 copies) of the mask [1 2 1; 2 4 2; 1 2 1] / 16, each (sum + 8) >> 4 on 8-bit values
 * with reflect-101 borders (index i mod 2 (n - 1), folded; 0 for n = 1).  All passes run in LDS: the tile is loaded with a
 * halo of k reflected once, which equals reflecting at every pass because the mask is symmetric. */
int segk_perturb_blur(const segk_perturb_desc* descs, int n, int total_tiles, int k, segk_stream_t s);

/* ---- reconstruction head and MSE loss (autoencoder/autoencoder.py:188-191; nn.MSELoss as autoencoder.ipynb cell 0
 * constructs it and utils/training.py:141,234 call it) ---------------------------------------------------------------
 * rec NCHW fp32 [B,Cout,H,W] = sigmoid(bias + conv3x3_pad1(x)) with x an act tensor [B,H,W,Cp] (Cin <= Cp, zero halo) and
 * the fp32 parameters themselves: w OIHW [Cout][Cin][3][3], bias [Cout] (may be NULL).  fp32: fp32 FMAs on the operands as
 * given; bf16: the weights are rounded to bf16 and channel pairs are multiplied with fp32 accumulation.  Any Cout >= 1. */
int segk_recon_head_fwd(const void* x, const float* w, const float* bias, float* rec, int B, int H, int W, int Cp, int Cin,
                        int Cout, int dtype, segk_stream_t s);
/* its Sigmoid backward into the act layout: dz [B,H,W,Cp] = drec * (1 - rec) * rec (ATen's sigmoid_backward order) in
 * dtype, padding channels zeroed; drec, rec NCHW fp32 [B,C,H,W].  dx / dW / db follow from segk_conv3x3 (mode-1 weights),
 * segk_wgrad (geo 0) and segk_channel_sum on dz. */
int segk_recon_sigmoid_bwd(const float* drec, const float* rec, void* dz, int B, int H, int W, int C, int Cp, int dtype,
                           segk_stream_t s);
/* out[0] = scale * sum((a - b)^2) over n fp32 elements, scale = 1/n (mean = 1) or 1 (mean = 0): fixed per-block fp64
 * partials in part (8-byte aligned, part_floats >= SEGK_MSE_PART_FLOATS suffices for every n), then a one-block
 * fixed-order finalize -- the value depends on the data only, never on timing or the device.  Two launches. */
#define SEGK_MSE_PART_FLOATS 1024
int segk_mse_fwd(const float* a, const float* b, float* part, int part_floats, float* out, long n, int mean, segk_stream_t s);
/* da = (norm * (a - b)) * grad_out[0] with norm = (float)(2/n) (mean) or 2 (ATen's mse_loss_backward); grad_out is read on
 * the device.  db (may be NULL) = -da, the gradient of the target. */
int segk_mse_bwd(const float* a, const float* b, const float* grad_out, float* da, float* db, long n, int mean,
                 segk_stream_t s);

/* ---- optimizer step: global-norm clipping + AdamW + weight EMA ------------------------------------------------------------
 * Replaces the notebooks' `optimizer = torch.optim.AdamW(model.parameters(), weight_decay=0.01)` cell and its
 * optimizer.step() (utils/training.py), plus what trainers compose around it (clip_grad_norm_, an EMA of the weights).
 * The arithmetic is defined in DESIGN.md section 3.13 (float32, every operation rounded once).
 *
 * table: device array of n records sorted by block0; tensor i owns ceil(numel / SEGK_OPTIM_CHUNK) consecutive blocks from
 * block0, total_blocks is their sum (tensors of 0 elements are left out).  All tensors are dense fp32.  The 16-byte vector
 * path runs where every pointer of a record is 16-byte aligned, a per-element path elsewhere.
 * groups: device array of ngroups records, uploaded by the host every step (lr may move between steps).
 * state: 32 + 2 * (8 + 16 * ngroups) bytes of device memory that persist across steps:
 *   { double norm; float clip; int32 finite; int32 skipped; int32 pad[3] } then two slots { int32 t; int32 pad;
 *   double pow[ngroups][2] } (beta1^t, beta2^t as running products).  A step reads slot `parity` and writes slot parity ^ 1:
 *   the host flips parity with every step it launches.  Initial content: clip 1, finite 1, slot pow 1.0, everything else 0.
 * The table, the groups and the state must stay valid until the launch has run. */
#define SEGK_OPTIM_CHUNK 4096            /* elements per block */
#define SEGK_OPTIM_MAX_GROUPS 1024
#define SEGK_OPTIM_CLIP 1                /* grad_norm: clip = min(1, max_norm / (norm + 1e-6)); otherwise clip = 1 */
#define SEGK_OPTIM_SKIP_NONFINITE 2      /* both: a step whose gradients hold an inf or a NaN writes nothing */
#define SEGK_OPTIM_NORMED 1              /* adamw: segk_optim_grad_norm ran for this step (same parity) on this stream */
#define SEGK_OPTIM_EMA_WARMUP 4          /* adamw: d = min(ema_decay, (1 + t) / (10 + t)) in float32 instead of omd */
#define SEGK_OPTIM_SWAP 8                /* adamw: exchange p and shadow of every record that has one; nothing else is read */
typedef struct {
  float* p;                          /* parameter */
  const float* g;                    /* its gradient */
  float* m;                          /* exp_avg */
  float* v;                          /* exp_avg_sq */
  float* shadow;                     /* EMA of p, or NULL */
  int64_t numel;
  int32_t block0;                    /* first block of this tensor in the launch */
  int32_t group;                     /* index into groups */
  int32_t pad_[2];
} segk_optim_rec;                    /* 64 bytes */
typedef struct {
  float lr;                          /* float32(lr) */
  float decay;                       /* float32(1 - lr * weight_decay), formed in float64 */
  float omb1, b2, omb2;              /* float32(1 - beta1), float32(beta2), float32(1 - beta2) */
  float eps;
  float omd;                         /* float32(1 - ema_decay), formed in float64 */
  float ema_decay;                   /* float32(ema_decay): read with SEGK_OPTIM_EMA_WARMUP only */
  double beta1, beta2;               /* multipliers of the running products */
  int32_t pad_[4];
} segk_optim_group;                  /* 64 bytes */
/* Sum of squares of every gradient of the table in float64 with a fixed assignment of elements to threads and fixed
 * reduction trees (no float atomics: identical gradients give identical bits, run to run and rank to rank).  part: scratch of
 * total_blocks doubles.  The last block to arrive writes state->norm, clip (rounded once to float32) and finite, and the next
 * slot of the step state: t + 1 and pow * beta when the step will be applied (finite, or no SEGK_OPTIM_SKIP_NONFINITE), a
 * copy and skipped + 1 otherwise. */
int segk_optim_grad_norm(const segk_optim_rec* table, int n, int total_blocks, const segk_optim_group* groups, int ngroups,
                         void* state, double* part, double max_norm, int flags, int parity, segk_stream_t s);
/* One pass per element: reads g, p, m, v (and shadow), writes p, m, v (and shadow).  With SEGK_OPTIM_NORMED the gradient is
 * scaled by state->clip and the step state is read from slot parity ^ 1; without it every block derives t + 1 and pow * beta
 * from slot parity and block 0 stores them to slot parity ^ 1.  SEGK_OPTIM_SWAP: groups and state may be NULL. */
int segk_optim_adamw(const segk_optim_rec* table, int n, int total_blocks, const segk_optim_group* groups, int ngroups,
                     void* state, int flags, int parity, segk_stream_t s);

/* ---- diagnostics (not on the product path) ---------------------------------------------------------
 * The shader clock held under a dense bf16 MFMA load: `blocks` workgroups of four waves (one per SIMD) run `iters` rounds of
 * 16 v_mfma_f32_32x32x16_bf16 (shape 0; shape 1: the same work as 32 v_mfma_f32_16x16x32_bf16) each and write, per wave w, out[2w] = elapsed shader cycles (s_memtime) and out[2w+1] =
 * elapsed ticks of the constant 100 MHz counter (s_memrealtime): clock = out[2w] / out[2w+1] x 100 MHz.  bench.py puts
 * the median into its line so that box-to-box spread is explained by a number. */
int segk_clock_probe(uint64_t* out, int blocks, int iters, int shape, segk_stream_t s);
/* Overwrites every counter of the device's ticket ring with the low 32 bits of `pattern` and waits for the copy.  The ring
 * holds the arrival counters of the kernels that finish a reduction in the launch that produced its partials
 * (segk_bn_finalize above 1024 partial rows, segk_loss_fwd / segk_prob_loss_fwd); the host zeroes the counters a launch will
 * use on that launch's stream right before it, so ANY content is a valid starting state.  Tests use this entry to leave
 * behind what an aborted launch or a stray store would (tests/test_gpu_kernels.py). */
int segk_debug_poison_tickets(uint64_t pattern, segk_stream_t s);

/* ---- metric: argmax + confusion matrix (utils/MetricsHistory.py:65-75) ---------------------------
 * M[pred*8 + label] += count (uint64, caller zeroes); TP/FP/FN/TN follow on the host. */
int segk_confusion(const float* logits, const int64_t* labels, int N, int C, long HW, uint64_t* M, segk_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
