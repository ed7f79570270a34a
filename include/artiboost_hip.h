/* artiboost_hip.h -- C ABI of libartiboost_hip.so (hand-written HIP kernels for gfx950 / MI355X).
 *
 * The reference (lixiny/ArtiBoost) is 100 % Python and has no FFI of its own; every "kernel" it runs lives in a
 * third-party wheel (cuDNN via torch, pyrender/OpenGL, manotorch).  Each entry point below therefore names the
 * reference *call site* whose arithmetic it replaces (paths relative to the reference root).  INTEGRATION.md shows
 * the ctypes stub a maintainer would add on the reference side.
 *
 * Conventions
 *  - plain pointers + sizes only; all pointers are DEVICE pointers unless the name ends in _host
 *  - every function enqueues work on `stream` (a hipStream_t passed as void*) and returns immediately
 *  - return value: 0 on success, >0 = hipError_t from the launch, <0 = argument error (AB_E*)
 *  - no global state; re-entrant per stream
 *  - activations are NHWC ("pixels x channels"); `dtype`: 0 = float32, 1 = bfloat16 (raw uint16 bits)
 */
#ifndef ARTIBOOST_HIP_H
#define ARTIBOOST_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AB_DT_F32 0
#define AB_DT_BF16 1
#define AB_DT_U8N 2         /* loaders only (`out_dtype` of ab_render_batch / ab_augment_batch): the padded image as ONE bf16 plane of the odd integers
                             * 2 v - 255 (v = the uint8 pixel after the jitter chain); the network input v / 255 - 0.5 (hodata.py:446) is that plane / 510.
                             * ab_conv2d_stem_fwd_x3 / _stem_wgrad_x3 take it as xpad_hi with xpad_lo == NULL: two MFMA passes, no rounding of the image */
#define AB_EINVAL (-1)
#define AB_ESHAPE (-2)
#define AB_EALIGN (-3)

/* library / device info: returns ABI version (integer, bumped on any signature change) */
int ab_abi_version(void);

/* measurement aid (no reference counterpart; bench.py's roofline leg): a one-thread launch that writes the device's constant-rate wall clock to
 * *slot (device int64); ab_wall_clock_khz(): its rate.  Captured into a hipGraph around a kernel, the slot difference is that kernel's
 * duration inside the replay.                                                                                                          */
int ab_wall_stamp(int64_t* slot, void* stream);
int ab_wall_clock_khz(void);

/* ---- M3: fused softmax + 3-D integral (soft-argmax) head ------------------------------------------------------
 * replaces: norm_heatmap('softmax') + max + renorm + view_to_bcdhw + integral_heatmap3d
 *           anakin/models/simplebaseline.py:16-40, 43-71, 183-189
 * logits : [B, H, W, C*DP] (NHWC of the reference's (B, C*D, H, W); channel = c*DP + d, d < D; DP >= D is the
 *          padded depth pitch -- the model uses DP = 32 so every class is one aligned 64/128-byte run), f32|bf16
 * part   : workspace, float [B, ntile, C, 8]  (ntile from ab_softargmax3d_ntiles)
 * uvd    : float [B, C, 3]  (u = width, v = height, d = depth, each in [0,1))
 * conf   : float [B, C]     (max softmax probability)
 * stat   : float [B, C, 2]  (global max, sum exp(x - max)) kept for backward                                  */
int ab_softargmax3d_ntiles(int H, int W);
/* Host only, launches nothing: which kernel instantiation an entry point runs for (dtype, C, D, DP, norm = norm_type) -- the launchers switch
 * on this very function.  entry: 0 = forward stage 1, 1 = ab_softargmax3d_bwd[_norm], 2 = ab_softargmax3d_bwd_x3 (split planes),
 * 3 = ab_softargmax3d_bwd_x3_bias (split planes + bias gradient).  Returns
 *   entry 0:    10 = scalar kernel (C*DP odd);  100 + 10*KP + m = pair kernel walking KP in {2, 4, 6, 8} groups of 128 channels,
 *               m = 1: depth bins merged by 32 lanes per class (D <= 32), m = 0: by one thread per class (D > 32)
 *   entry 1:    20 = scalar kernel (C*DP odd);  PIX*100 + V*10 + KV = pair kernel, PIX pixels per workgroup, KV groups of V channels (1628)
 *   entry 2, 3: 10000 + PIX*100 + V*10 + KV  (PIX = 16 | 64;  V, KV = 4, 3 for C*DP % 4 == 0 up to 768;  4, 4 above;  2, 8 otherwise)
 * or the AB_E* code with which the entry point refuses these arguments (AB_ESHAPE: DP < D, C*DP > 1024, odd C*DP on entries 2 and 3).  */
int ab_softargmax3d_form(int entry, int dtype, int C, int D, int DP, int norm);
int ab_softargmax3d_fwd(const void* logits, int dtype, int B, int C, int D, int DP, int H, int W,
                        float* part, float* uvd, float* conf, float* stat, void* stream);
/* dlogits[b,h,w,c*D+d] = p * ( g_uvd . (coord - uvd) ) / (1+1e-7) + g_conf * conf * (argmax? 1 : 0 - p)
 * g_conf may be NULL.  dlogits has the dtype/layout of logits (may alias logits: in-place is allowed).        */
int ab_softargmax3d_bwd(const void* logits, int dtype, int B, int C, int D, int DP, int H, int W,
                        const float* uvd, const float* conf, const float* stat,
                        const float* g_uvd, const float* g_conf, void* dlogits, void* stream);
/* fp32 logits in, dlogits out as split-bf16 planes (what the final layer's bf16x3 data / weight gradients consume)      */
int ab_softargmax3d_bwd_x3(const float* logits, int B, int C, int D, int DP, int H, int W, const float* uvd,
                           const float* conf, const float* stat, const float* g_uvd, const float* g_conf,
                           void* dl_hi, void* dl_lo, void* stream);
/* ... and dbias [C*DP] = column sums of dlogits over all B*H*W rows: the bias gradient of the final 1x1 layer that produced the
 * logits (anakin/models/simplebaseline.py:148, final_layer), reduced in the same pass in fixed order.
 * colpart: ab_softargmax3d_bwd_x3_bias_rows(B, H, W) x C*DP floats of scratch.                                              */
int ab_softargmax3d_bwd_x3_bias_rows(int B, int H, int W);
int ab_softargmax3d_bwd_x3_bias(const float* logits, int B, int C, int D, int DP, int H, int W, const float* uvd,
                                const float* conf, const float* stat, const float* g_uvd, const float* g_conf, void* dl_hi,
                                void* dl_lo, float* colpart, float* dbias, void* stream);
/* NORM_TYPE of IntegralDeconvHead (anakin/models/simplebaseline.py:16-40): norm_type 0 = "softmax" (the entry points above),
 * 1 = "sigmoid": w = sigmoid(x), conf = max w, uvd = sum(w * coord) / (sum(w) + 1e-7) -- evaluated in the log domain with the same
 * kernels (x' = log sigmoid(x); `stat` holds (log w_max, sum w / w_max)).  g_conf must be NULL for the sigmoid head.
 * Its backward is dlogits = w (1 - w) ( g_uvd . (coord - uvd) ) / (sum w + 1e-7): the 1e-7 is absolute, as in the forward.
 * ("divide_sum" is not implemented: raw weights can be negative, and the reference's own docstring advises against it.)
 * _bwd_x3_norm: dlogits as split planes; colpart + dbias non-NULL: also the bias gradient (scratch as for _bwd_x3_bias). */
int ab_softargmax3d_fwd_norm(const void* logits, int dtype, int B, int C, int D, int DP, int H, int W, int norm_type, float* part,
                             float* uvd, float* conf, float* stat, void* stream);
int ab_softargmax3d_bwd_norm(const void* logits, int dtype, int B, int C, int D, int DP, int H, int W, int norm_type, const float* uvd,
                             const float* conf, const float* stat, const float* g_uvd, const float* g_conf, void* dlogits,
                             void* stream);
int ab_softargmax3d_bwd_x3_norm(const float* logits, int B, int C, int D, int DP, int H, int W, int norm_type, const float* uvd,
                                const float* conf, const float* stat, const float* g_uvd, void* dl_hi, void* dl_lo, float* colpart,
                                float* dbias, void* stream);

/* ---- M1/M2: convolution stack (implicit GEMM on MFMA) ----------------------------------------------------------
 * replaces cuDNN behind nn.Conv2d / nn.ConvTranspose2d / nn.Linear:
 *   anakin/models/resnet.py:154 (stem), :41-44 conv3x3 in BasicBlock (:85-101), :181-184 (1x1 downsample)
 *   anakin/models/simplebaseline.py:161-170 (ConvTranspose2d 4x4 s2 p1), :95-101 (final 1x1 conv + bias)
 *   anakin/models/mlp.py:15-22 (Linear + ReLU)
 * Layouts: activations NHWC; weights "OHWI" = [Cout][kh][kw][Cin] (K-contiguous) in the activation dtype;
 * data-gradient weights "IHWO" = [Cin][kh][kw][Cout].  Cin (fwd) / Cout (dgrad) must be a multiple of 32 (bf16)
 * or 16 (f32).  stats (optional): float [ab_conv2d_stat_rows(...)][Cout][2] per-tile (sum, sum^2) partials of
 * the OUTPUT for the following training-mode BatchNorm (finalised by ab_bn_finalize).                           */
int ab_conv2d_stat_rows(int dtype, int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int stem);
int ab_conv2d_fwd(const void* x, const void* w, void* y, int dtype, int N, int H, int W, int Cin, int Cout,
                  int kh, int kw, int stride, int pad, const float* bias, float* stats, int relu, void* stream);
/* stem 7x7/2 pad 3 on a zero-bordered NHWC4 image [N, H+6, W+8, 4] (see ab_image_pad_nhwc4); w [Cout][7][8][4]  */
int ab_conv2d_stem_fwd(const void* xpad, const void* w, void* y, int dtype, int N, int H, int W, int Cout,
                       float* stats, void* stream);
/* dx of conv2d(x,w,stride,pad) (also == ConvTranspose2d forward).  H,W,Cin describe dx.  addend (optional, dx-shaped)
 * is added in the epilogue.  stats must be NULL.                                                                 */
/* rows of BatchNorm partials [rows][Cin][2] ab_conv2d_dgrad writes when `stats` is given (the forward of a transposed
 * convolution is this data gradient: simplebaseline.py:95-101); 0: not available for the shape, pass stats = NULL. */
int ab_conv2d_dgrad_stat_rows(int dtype, int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad);
int ab_conv2d_dgrad(const void* dy, const void* wt, void* dx, int dtype, int N, int H, int W, int Cin, int Cout,
                    int kh, int kw, int stride, int pad, const void* addend, float* stats, void* stream);
/* dw (float, OHWI) of conv2d; workspace of ab_conv2d_wgrad_workspace(N*Ho*Wo, Cout, kh*kw*Cin) bytes           */
long ab_conv2d_wgrad_workspace(int M, int Cout, int jtot);
int ab_conv2d_wgrad(const void* x, const void* dy, float* dw, int dtype, int N, int H, int W, int Cin, int Cout,
                    int kh, int kw, int stride, int pad, void* workspace, int accumulate, void* stream);
/* Deferred slab reduction: the *_deferred variants run the slab kernel and record the fixed-order reduction they would
 * launch; ab_wgrad_reduce_batch runs the recorded reductions of many layers in one launch (bit-identical results).  The
 * workspace of a deferred call must stay untouched until its descriptor has been consumed.  A split-bf16 launch of 2^21 or
 * more output pixels runs as two half-batches over one workspace: its *_x3_deferred call reduces both halves itself, in stream
 * order, and returns pending->nslices == 0 (dw is then complete without ab_wgrad_reduce_batch).                      */
#define AB_WGRAD_BATCH_MAX 48
typedef struct ab_wgrad_reduce_desc {
    const float* slabs;    /* [nslices][slab_elems] partial weight gradients */
    float* dst;            /* dW */
    long slab_elems;
    int nslices;           /* 0: nothing pending */
    int src_j, dst_j;      /* row lengths of a slab row and of the destination row (padded taps dropped) */
    int accumulate, stem_mask;
} ab_wgrad_reduce_desc;
int ab_conv2d_wgrad_deferred(const void* x, const void* dy, float* dw, int dtype, int N, int H, int W, int Cin, int Cout,
                             int kh, int kw, int stride, int pad, void* workspace, int accumulate,
                             ab_wgrad_reduce_desc* pending, void* stream);
int ab_conv2d_stem_wgrad_deferred(const void* xpad, const void* dy, float* dw, int dtype, int N, int H, int W, int Cout,
                                  void* workspace, ab_wgrad_reduce_desc* pending, void* stream);
int ab_conv2d_wgrad_x3_deferred(const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, float* dw, int N, int H,
                                int W, int Cin, int Cout, int kh, int kw, int stride, int pad, void* workspace, int accumulate,
                                ab_wgrad_reduce_desc* pending, void* stream);
int ab_conv2d_stem_wgrad_x3_deferred(const void* xpad_hi, const void* xpad_lo, const void* dy_hi, const void* dy_lo, float* dw,
                                     int N, int H, int W, int Cout, void* workspace, ab_wgrad_reduce_desc* pending, void* stream);
int ab_wgrad_reduce_batch(const ab_wgrad_reduce_desc* desc, int n, void* stream);
/* Grouped weight gradient (round 6): G <= AB_WGRAD_GROUP_MAX convolutions of ONE shape (3x3 / stride 1 / pad 1, split-bf16 operands: the
 * layers of a ResNet stage, anakin/models/resnet.py:85-101,158-161) as one slab launch + one reduction launch.  items_host[p]: the planes of
 * x [N,H,W,Cin] and dy [N,H,W,Cout] and the destination dW [Cout,3,3,Cin] fp32 of problem p (device pointers in a HOST array).  Equal to G
 * ab_conv2d_wgrad_x3 calls up to the (fixed) summation order over pixel slices.  workspace >= ab_conv2d_wgrad_x3_group_workspace(...) bytes
 * (0: shape not handled: call ab_conv2d_wgrad_x3 per layer).                                                                              */
#define AB_WGRAD_GROUP_MAX 8
typedef struct ab_wgrad_group_item {
    const void* x_hi; const void* x_lo; const void* dy_hi; const void* dy_lo;
    float* dw;
} ab_wgrad_group_item;
long ab_conv2d_wgrad_x3_group_workspace(int G, int N, int H, int W, int Cin, int Cout);
int ab_conv2d_wgrad_x3_group(const ab_wgrad_group_item* items_host, int G, int N, int H, int W, int Cin, int Cout, void* workspace,
                             int accumulate, void* stream);
long ab_conv2d_stem_wgrad_workspace(int N, int H, int W, int Cout);
int ab_conv2d_stem_wgrad(const void* xpad, const void* dy, float* dw, int dtype, int N, int H, int W, int Cout,
                         void* workspace, void* stream);

/* ---- M1/M2 at the reference's precision: split-bf16 ("bf16x3") convolutions ------------------------------------
 * The reference runs these convolutions in fp32 (train/train_artiboost.py:39-41,91-96 -- no autocast; cuDNN fp32 behind
 * anakin/models/resnet.py:41-44,154,181-184 and simplebaseline.py:95-101,161-170).  Every fp32 operand v is given as
 * two bf16 planes hi = bf16(v), lo = bf16(v - hi) (ab_split_f32 makes them) and a product is hi*hi + hi*lo + lo*hi on the
 * bf16 MFMA with fp32 accumulation: 2^-17 operand precision instead of bf16's 2^-9, at 1/3 of the bf16 matrix peak
 * (the f32-input MFMA runs at 1/16).  Outputs, addends, BatchNorm partials and weight gradients are fp32.
 * Same layouts and meanings as ab_conv2d_fwd / _dgrad / _wgrad; Cin (fwd) / Cout (dgrad) % 32 == 0, wgrad: both % 64.
 * w_lo must lie 0 .. 2^31-1 bytes after w_hi (both planes of one allocation).                                       */
int ab_split_f32(const float* src, long n, void* hi, void* lo, void* stream);          /* n % 8 == 0 */
/* rows of BatchNorm partials a forward WITHOUT bias / relu writes for this shape (the specialised 3x3/s1, 3x3/s2 and 4x4/s2 kernels write one
 * row per tile of theirs).  ab_conv2d_fwd_x3 with stats AND a bias or ReLU runs the generic kernel, whose row count may differ on those
 * shapes: it then returns AB_EINVAL instead of writing past a buffer sized by this function.                                            */
int ab_conv2d_x3_stat_rows(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad);
int ab_conv2d_fwd_x3(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, float* y, int N, int H, int W,
                     int Cin, int Cout, int kh, int kw, int stride, int pad, const float* bias, float* stats, int relu,
                     void* stream);
/* The final layer of IntegralDeconvHead and the first stage of its soft-argmax in ONE launch -- replaces final_layer (nn.Conv2d(256,
 * NCLASSES * DEPTH, 1): anakin/models/simplebaseline.py:95-101,173-175) followed by the softmax statistics of norm_heatmap / integral_heatmap3d
 * (:16-40, 43-71, 183-189).  x (hi, lo) [B,H,W,Cin]; w (hi, lo) [C*32][Cin] (channel = c*32 + d, d < D valid: DEPTH_PITCH 32, padding bins
 * carry zero weights); bias [C*32] or NULL; logits fp32 [B,H,W,C*32]; part fp32 [B, H*W/64, C, 8] = the rows ab_softargmax3d_stage2 merges
 * into uvd / conf / stat (same meaning as ab_softargmax3d_fwd's workspace).  _ok(): 1 when the register-resident GEMM takes the shape
 * (Cin % 64 == 0, Cin <= 256, H*W % 64 == 0, D <= 32); otherwise AB_ESHAPE and the caller runs ab_conv2d_fwd_x3 + ab_softargmax3d_fwd.  */
int ab_conv1x1_sam_fwd_x3_ok(int B, int H, int W, int Cin, int C, int D);
int ab_conv1x1_sam_fwd_x3(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias, float* logits,
                          int B, int H, int W, int Cin, int C, int D, float* part, void* stream);
int ab_softargmax3d_stage2(const float* part, int B, int C, int ntile, float* uvd, float* conf, float* stat, void* stream);
/* Eval-mode BasicBlock convolutions (anakin/models/resnet.py:85-101 under model.eval(): train/submit_reload.py:26-79, the TEST
 * pass of train/train_artiboost.py:224-240): 3x3 / stride 1 / pad 1 convolution with the BatchNorm that follows folded into the
 * epilogue -- bnp = [scale Cout | shift Cout | ..] from ab_bn_eval_params; out = relu?(conv * scale + shift + residual) as (hi, lo)
 * planes (+ fp32 copy when out_f32 != NULL); residual = (res_hi, res_lo) planes, or fp32 res_f32, or none.  _ok(): 1 when the
 * shape is taken (otherwise run ab_conv2d_fwd_x3 + ab_bn_apply_x3: same bits). */
int ab_conv2d_fwd_x3_evalbn_ok(int N, int H, int W, int Cin, int Cout);
int ab_conv2d_fwd_x3_evalbn(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, int N, int H, int W, int Cin,
                            int Cout, const float* bnp, const void* res_hi, const void* res_lo, const float* res_f32, int relu,
                            void* out_hi, void* out_lo, float* out_f32, void* stream);
/* ... and of the generic convolutions (strided 3x3, 1x1 downsample: resnet.py:85-101,181-184) / the head's ConvTranspose2d
 * (simplebaseline.py:161-172; dgrad form as ab_conv2d_dgrad_x3): out = relu?(conv * scale + shift) as fp32 `out_f32` OR as planes
 * (out_hi, out_lo) -- exactly one of the two; bit-identical to the conv followed by ab_bn_apply / ab_bn_apply_x3. */
int ab_conv2d_fwd_x3_affine(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, int N, int H, int W, int Cin,
                            int Cout, int kh, int kw, int stride, int pad, const float* scale, const float* shift, int relu,
                            float* out_f32, void* out_hi, void* out_lo, void* stream);
int ab_conv2d_dgrad_x3_affine(const void* dy_hi, const void* dy_lo, const void* wt_hi, const void* wt_lo, int N, int H, int W, int Cin,
                              int Cout, int kh, int kw, int stride, int pad, const float* scale, const float* shift, int relu,
                              float* out_f32, void* out_hi, void* out_lo, void* stream);
int ab_conv2d_dgrad_x3_stat_rows(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad);
int ab_conv2d_dgrad_x3(const void* dy_hi, const void* dy_lo, const void* wt_hi, const void* wt_lo, float* dx, int N, int H,
                       int W, int Cin, int Cout, int kh, int kw, int stride, int pad, const float* addend, float* stats,
                       void* stream);
/* The two data gradients that leave the input of a down-sampling BasicBlock (anakin/models/resnet.py:85-101 backwards: conv1 3x3/s2
 * and downsample.0 1x1/s2 read the same x) in one launch: dx = dgrad(dy, wt; kh x kw / 2 / pad) + dgrad(dy2, wt2; 1x1 / 2 / 0)
 * [+ addend].  dy2 planes [N,H/2,W/2,Cout], wt2 planes [Cin][1][1][Cout]; kh, kw <= 3, H, W even.                            */
int ab_conv2d_dgrad_x3_pair(const void* dy_hi, const void* dy_lo, const void* wt_hi, const void* wt_lo, const void* dy2_hi,
                            const void* dy2_lo, const void* wt2_hi, const void* wt2_lo, float* dx, int N, int H, int W, int Cin,
                            int Cout, int kh, int kw, int pad, const float* addend, void* stream);
/* ab_conv2d_dgrad_x3_pair whose result arrives at relu(bn(bn_y) [+ residual]) -- the output of the stage below (anakin/models/resnet.py:85-101,
 * 178-192 backwards): dz = the MASKED gradient, bn_part[rows][Cin][2] = per-tile (sum dz, sum dz*xhat) for ab_bn_bwd_x3(part, rows); mask as
 * in ab_conv2d_dgrad_x3_bn.  rows = ab_conv2d_dgrad_x3_pair_bn_rows(...); 0 = not handled (ab_conv2d_dgrad_x3_pair + the full ab_bn_bwd_x3). */
int ab_conv2d_dgrad_x3_pair_bn_rows(int N, int H, int W, int Cin, int Cout, int kh, int kw, int pad);
int ab_conv2d_dgrad_x3_pair_bn(const void* dy_hi, const void* dy_lo, const void* wt_hi, const void* wt_lo, const void* dy2_hi,
                               const void* dy2_lo, const void* wt2_hi, const void* wt2_lo, float* dz, int N, int H, int W, int Cin,
                               int Cout, int kh, int kw, int pad, const float* bn_y, const void* bn_out_hi, const float* bnp,
                               float* bn_part, void* stream);
/* Data gradient of a 3x3/s1 conv whose result arrives at relu(bn(bn_y) [+ residual]) (BasicBlock, anakin/models/resnet.py:85-101,
 * backwards): dz = the MASKED gradient (mask: sign of bn_out_hi, the hi bf16 plane of the stored activation, or recomputed from
 * bn_y and bnp when bn_out_hi is NULL), bn_part[rows][Cin][2] = per-tile (sum dz, sum dz*xhat) for ab_bn_bwd_x3(part, rows).
 * rows = ab_conv2d_dgrad_x3_bn_rows(...); 0 = shape not handled here (use ab_conv2d_dgrad_x3 + the full ab_bn_bwd_x3).  Also taken: 1x1 / s1 / p0
 * with addend = bn_out_hi = NULL (final_layer of the head, simplebaseline.py:173-175 backwards, arriving at relu(bn(deconv_layers.3 output))).  */
int ab_conv2d_dgrad_x3_bn_rows(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad);
int ab_conv2d_dgrad_x3_bn(const void* dy_hi, const void* dy_lo, const void* wt_hi, const void* wt_lo, float* dz, int N, int H,
                          int W, int Cin, int Cout, int kh, int kw, int stride, int pad, const float* addend,
                          const float* bn_y, const void* bn_out_hi, const float* bnp, float* bn_part, void* stream);
/* workspace: ab_conv2d_wgrad_x3_workspace(...) bytes (the split-bf16 kernels slice the pixels differently from the bf16 ones) */
long ab_conv2d_wgrad_x3_workspace(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad);
int ab_conv2d_wgrad_x3(const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, float* dw, int N, int H,
                       int W, int Cin, int Cout, int kh, int kw, int stride, int pad, void* workspace, int accumulate,
                       void* stream);

/* stem 7x7/2 on split planes of the zero-bordered NHWC4 image (ab_conv2d_stem_fwd / _wgrad at bf16x3 precision)        */
int ab_conv2d_stem_x3_stat_rows(int N, int H, int W);
int ab_conv2d_stem_fwd_x3(const void* xpad_hi, const void* xpad_lo, const void* w_hi, const void* w_lo, float* y, int N, int H,
                          int W, int Cout, float* stats, void* stream);
int ab_conv2d_stem_wgrad_x3(const void* xpad_hi, const void* xpad_lo, const void* dy_hi, const void* dy_lo, float* dw, int N,
                            int H, int W, int Cout, void* workspace, void* stream);
/* fp32 elementwise passes that write a convolution operand directly as split planes (no separate ab_split_f32 pass):
 * ab_bn_apply_x3 = ab_bn_apply on fp32 with out (optional fp32 copy, may be NULL) + planes; ab_bn_bwd_x3 = ab_bn_bwd /
 * ab_bn_bwd_apply on fp32 with dy as planes (nparts_given = 0: run the reduction into `part`; > 0: `part` holds that many
 * already reduced rows).  resnet.py:85-101, simplebaseline.py:171-172.  ab_bn_apply_x3 / _respl take C % 4 == 0 (8 channels per
 * thread, 4 where C % 8 == 4: the same bits); the other forms C % 8 == 0.                                            */
int ab_bn_apply_x3(const float* y, const float* res, const float* bnp, long M, int C, int relu, float* out, void* out_hi,
                   void* out_lo, void* stream);
/* ... the residual given as the raw output res_y of the block's downsample conv and ITS BatchNorm parameters res_bnp
 * (anakin/models/resnet.py:95-99: identity = downsample(x)): out = [relu]( bn(y) + bn_ds(res_y) ), bn_ds(res_y) never stored. */
int ab_bn_apply_x3_resbn(const float* y, const float* res_y, const float* bnp, const float* res_bnp, long M, int C, int relu,
                         float* out, void* out_hi, void* out_lo, void* stream);
/* ... the residual given as its (hi, lo) bf16 planes (a block input that exists only as the planes its producer wrote). */
int ab_bn_apply_x3_respl(const float* y, const void* res_hi, const void* res_lo, const float* bnp, long M, int C, int relu,
                         float* out, void* out_hi, void* out_lo, void* stream);
/* BatchNorm finalize + apply in ONE launch for the training forward (round 4; nn.BatchNorm2d in train mode, resnet.py:85-101 /
 * simplebaseline.py:152-175): part [nparts][C][2] = the per-tile (sum, sum of squares) of a convolution's epilogue, count = elements per
 * channel.  Writes bnp [4][C] and updates the running statistics exactly like ab_bn_finalize, then applies like ab_bn_apply_x3
 * (res fp32 or NULL), ab_bn_apply_x3_respl (res_hi / res_lo) or ab_bn_apply_x3_resbn (res + res_bnp).  Taken when
 * ab_bn_fin_apply_x3_ok(nparts, C) (nparts <= 64, C % 64 == 0); AB_ESHAPE otherwise (run ab_bn_finalize + ab_bn_apply_x3*).
 * ab_bn_bwd_x3 takes the same route internally for its finalize.                                                              */
int ab_bn_fin_apply_x3_ok(int nparts, int C);
int ab_bn_fin_apply_x3(const float* part, int nparts, long count, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, float* bnp, const float* y, const float* res, const void* res_hi,
                       const void* res_lo, const float* res_bnp, long M, int C, int relu, float* out, void* out_hi, void* out_lo,
                       void* stream);
/* out (relu == 1): the stored activation as fp32, or -- out_is_hi_plane != 0 -- the hi plane (bf16) of its split form: the
 * ReLU mask only needs the sign, and the plane is half the bytes                                                     */
int ab_bn_bwd_x3(const float* dout, const void* out, int out_is_hi_plane, const float* y, const float* bnp, long M, int C,
                 int relu, float* part, int nparts_given, float* bwdp, float* dgamma, float* dbeta, void* dy_hi, void* dy_lo,
                 float* dz_out, void* stream);

/* ---- M1/M2: training-mode BatchNorm, ReLU, residual, pooling (HBM-bound NHWC kernels) ---------------------------
 * replaces nn.BatchNorm2d / ReLU / MaxPool2d / mean-pool: anakin/models/resnet.py:85-101,155-157,219;
 * anakin/models/simplebaseline.py:171-172.
 * bnp: float [4][C] = (gamma*invstd, beta-mean*gamma*invstd, mean, invstd).                                     */
int ab_col_stats_nparts(long M);
int ab_col_stats(const void* x, int dtype, long M, int C, float* part, void* stream);
int ab_bn_finalize(const float* part, int nparts, int C, long count, const float* gamma, const float* beta,
                   float eps, float momentum, float* running_mean, float* running_var, float* bnp, void* stream);
int ab_bn_eval_params(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                      float* bnp, void* stream);
/* ... for EVERY BatchNorm of a network in one launch (eval mode re-derives them at each forward: the running statistics may have
 * moved): desc_dev = device int32 [n][6] = (gamma, beta element offset in `flat`; running_mean, running_var offset in `stats`;
 * bnp offset in `out`; C).  max_c = the largest C. */
int ab_bn_eval_params_batch(const float* flat, const float* stats, const int32_t* desc_dev, int n, int max_c, float eps, float* out,
                            void* stream);
int ab_bn_apply(const void* y, const void* res, const float* bnp, int dtype, long M, int C, int relu, void* out,
                void* stream);
/* part: float [ab_col_stats_nparts(M)][C][2]; bwdp: float [2][C]; dz_out optional (gradient of the residual branch).
 * relu: 0 = no activation followed the BN; 1 = ReLU, mask taken from the stored activation `out` (needed when a residual
 * was added before the ReLU); 2 = ReLU, mask recomputed as y*bnp[0]+bnp[1] > 0 (`out` may be NULL and is not read).   */
int ab_bn_bwd(const void* dout, const void* out, const void* y, const float* bnp, int dtype, long M, int C, int relu,
              float* part, float* bwdp, float* dgamma, float* dbeta, void* dy, void* dz_out, void* stream);
int ab_relu_bwd(const void* dout, const void* out, int dtype, long n, void* dz, void* stream);
int ab_col_sum(const void* x, int dtype, long M, int C, float* part, float* out, void* stream);
int ab_col_sum_x3(const void* hi, const void* lo, long M, int C, float* part, float* out, void* stream);   /* of hi + lo */
int ab_add(const void* a, const void* b, int dtype, long n, void* out, void* stream);
/* idx: uint8 [N,H/2,W/2,C] winning tap (0..8, first maximum in row-major order); H,W describe the pool INPUT          */
int ab_maxpool3x3s2_fwd(const void* x, int dtype, int N, int H, int W, int C, void* out, void* idx, void* stream);
/* BatchNorm-backward reduction fused into the producer of its input gradient.  ab_conv2d_dgrad_bnstats is
 * ab_conv2d_dgrad (3x3 / stride 1 / pad 1, bf16) whose epilogue also accumulates, over the dx tile it stores, the sums
 * (sum dz, sum dz*xhat) of the BatchNorm that produced this conv's INPUT activation: bn_y = that BN's input (the conv
 * output it normalised), bnp = its (scale, shift, mean, invstd), dz = dx masked by the ReLU that followed (mask from the
 * stored activation bn_out when non-NULL -- required if a residual was added before the ReLU -- else recomputed from
 * bn_y).  bn_part: float [rows][Cin][2] with rows = ab_conv2d_dgrad_bnstats_rows(...) (0: no fused path for this shape;
 * use ab_conv2d_dgrad + ab_bn_bwd).  ab_bn_bwd_apply is the rest of ab_bn_bwd (finalize + apply) from such partials. */
int ab_conv2d_dgrad_bnstats_rows(int dtype, int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad);
int ab_conv2d_dgrad_bnstats(const void* dy, const void* wt, void* dx, int dtype, int N, int H, int W, int Cin, int Cout,
                            int kh, int kw, int stride, int pad, const void* addend, const void* bn_y, const void* bn_out,
                            const float* bnp, float* bn_part, void* stream);
int ab_bn_bwd_apply(const void* dout, const void* out, const void* y, const float* bnp, int dtype, long M, int C, int relu,
                    const float* part, int nparts, float* bwdp, float* dgamma, float* dbeta, void* dy, void* dz_out,
                    void* stream);
/* Stem fusion: out = maxpool3x3/2(relu(y*bnp[0]+bnp[1])) without materialising the activation, and its backward through
 * both BN passes (dpool: pooled gradient; part/bwdp as in ab_bn_bwd with M = N*H*W).                                 */
int ab_bn_relu_maxpool3x3s2_fwd(const void* y, const float* bnp, int dtype, int N, int H, int W, int C, void* out,
                                void* idx, void* stream);
int ab_bn_relu_maxpool3x3s2_fwd_x3(const float* y, const float* bnp, int N, int H, int W, int C, float* out, void* out_hi,
                                   void* out_lo, void* idx, void* stream);      /* fp32 + (hi, lo) bf16 planes of the pooled tensor */
int ab_bn_relu_maxpool_bwd(const void* dpool, const void* idx, const void* y, const float* bnp, int dtype, int N, int H,
                           int W, int C, float* part, float* bwdp, float* dgamma, float* dbeta, void* dy, void* stream);
/* ... for the split-bf16 path: ONE pass scatters the pooled gradient to full resolution, masks it with the recomputed ReLU and
 * reduces it (dz: fp32 [N,H,W,C] scratch; part: [ab_bn_relu_maxpool_bwd_x3_nparts(N,H,W,C)][C][2]), then finalize + a mask-free
 * apply pass that writes dy as planes.  nparts == 0: shape not handled (use ab_maxpool3x3s2_bwd + ab_bn_bwd_x3).               */
int ab_bn_relu_maxpool_bwd_x3_nparts(int N, int H, int W, int C);
int ab_bn_relu_maxpool_bwd_x3(const float* dpool, const void* idx, const float* y, const float* bnp, int N, int H, int W,
                              int C, float* part, float* bwdp, float* dgamma, float* dbeta, float* dz, void* dy_hi,
                              void* dy_lo, void* stream);
/* The same pair with the backward's BatchNorm reduction run over the POOLED elements (the masked gradient is non-zero at window
 * winners only): the forward also writes ywin [N,H/2,W/2,C] fp32, the raw conv output at each winner; the backward reduces
 * (dpool, ywin) -- a quarter of the full-resolution tensors -- into part[ab_col_stats_nparts(N*H/2*W/2)][C][2].
 * fwd: `out` may be NULL (the pooled activation as planes only).                                                            */
int ab_bn_relu_maxpool3x3s2_fwd_x3w(const float* y, const float* bnp, int N, int H, int W, int C, float* out, void* out_hi,
                                    void* out_lo, void* idx, float* ywin, void* stream);
int ab_bn_relu_maxpool_bwd_x3w(const float* dpool, const void* idx, const float* ywin, const float* y, const float* bnp, int N, int H,
                               int W, int C, float* part, float* bwdp, float* dgamma, float* dbeta, void* dy_hi, void* dy_lo,
                               void* stream);
int ab_maxpool3x3s2_bwd(const void* idx, const void* dout, int dtype, int N, int H, int W, int C, void* dx, void* stream);
int ab_avgpool_fwd(const void* x, int dtype, int N, int HW, int C, float* out, void* stream);
int ab_avgpool_bwd(const float* g, int dtype, int N, int HW, int C, void* dx, int accumulate, void* stream);
int ab_cast_f32_bf16(const float* src, long n, void* dst, void* stream);
int ab_transpose_oki(const float* src, int O, int K, int I, int dtype, void* dst, void* stream);
/* The same re-layout for many tensors in one launch.  desc_dev: DEVICE array of ntensors descriptors; tensor t owns the
 * workgroups [tile_begin, tile_begin + ceil(O/64)*K*ceil(I/64)); total_tiles = end of the last range.  Requires
 * I % 4 == 0 and O % 8 == 0 (16-byte vectors).                                                                      */
typedef struct ab_transpose_desc {
    const void* src;   /* float [O][K][I] */
    void* dst;         /* dtype [I][K][O] */
    int32_t O, K, I;
    int32_t tile_begin;
} ab_transpose_desc;
int ab_transpose_oki_batch(const ab_transpose_desc* desc_dev, int ntensors, long total_tiles, int dtype, void* stream);
/* bf16 outputs as split planes (hi at desc.dst, lo = bf16(v - hi) at desc.dst + lo_offset_elems): the IHWO weight copies of
 * the bf16x3 data gradients */
int ab_transpose_oki_batch_x3(const ab_transpose_desc* desc_dev, int ntensors, long total_tiles, long lo_offset_elems, void* stream);
int ab_image_pad_nhwc4(const float* img_nchw, int dtype, int N, int H, int W, void* out, void* stream);

/* ---- T1: global-norm clip + Adam on the flat parameter buffer ---------------------------------------------------
 * replaces torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step: train/train_artiboost.py:91-96,
 * anakin/utils/netutils.py:26-33.  part: float[1024] workspace, total_norm: float[1] (device).  hyper (optional):
 * device float[3] = {lr, 1-beta1^step, sqrt(1-beta2^step)} overriding lr/step (per-step values under graph replay). */
int ab_grad_norm(const float* grad, long n, float* part, float* total_norm, void* stream);
/* x[0..n) *= s in place: the 1 / world_size after a SUM all-reduce of the flat gradient -- the averaging torch's
 * DistributedDataParallel does around train/train_artiboost.py:88 `final_loss.backward()` (the reference wraps the model in DDP at :249-257).
 * Kept in this library because RCCL's ReduceOp.AVG kernels use packed fp32. */
int ab_scale_f32(float* x, long n, float s, void* stream);
int ab_clip_adam(float* param, const float* grad, float* m, float* v, long n, const float* total_norm,
                 float max_norm, float lr, float beta1, float beta2, float eps, int step, const float* hyper,
                 void* lp, void* stream);
/* ab_clip_adam that also refreshes the split-bf16 weight planes (hi = bf16(p), lo = bf16(p - hi)) in the same pass */
int ab_clip_adam_x3(float* param, const float* grad, float* m, float* v, long n, const float* total_norm,
                    float max_norm, float lr, float beta1, float beta2, float eps, int step,
                    const float* hyper, void* lp_hi, void* lp_lo, void* stream);

/* ---- M4 + L1-L3 + V1: fused pose assembly + criterion, forward and backward --------------------------------------
 * replaces (one wave per sample, deterministic): anakin/models/hybridbaseline.py:49-96 (uvd->xyz, 6D->R, corners),
 * anakin/criterions/jointloss.py:25-67, ordinal.py:144-227, 262-306, criterion.py:57-67 and the per-sample EPE of
 * anakin/metrics/val_metric.py:84-106.  Random draws are inputs (host RNG, reference order): views [nv,3] float,
 * pair index lists int64.  weights8_host (HOST pointer) = {LAMBDA_JOINTS_3D, LAMBDA_CORNERS_3D, LAMBDA_JOINTS_LEVEL,
 * LAMBDA_PART_LEVEL, LAMBDA_SCENE_LEVEL, LAMBDAS[JointsLoss], LAMBDAS[HandOrdLoss], LAMBDAS[SceneOrdLoss]}.
 * outputs: joints_abs [B,21,3], corners_abs [B,8,3], rotmat [B,3,3], uvd2d [B,30,3] (optional), sample_part [B,8]
 * (per-sample partial sums; [5],[6] = joint / corner EPE in mm), losses float[8] = joints_3d_loss, corners_3d_loss,
 * joint_ord_loss, part_ord_loss, scene_ord_loss, final_loss, mean EPE joints, mean EPE corners;
 * g_kp3d [B,22,3], g_box6d [B,6] = d final_loss / d input (NULL g_kp3d: forward only).                          */
/* M4 alone -- the pose assembly of an EVAL-mode forward (no targets, no criterion): anakin/models/hybridbaseline.py:49-96
 * (uvd -> xyz with the crop intrinsics, 6-D -> R, canonical corners -> camera frame, 2-D re-projection).  One launch instead of the
 * ~50 small tensor ops of the module's forward.  joints_abs [B,21,3], corners_abs [B,8,3], rotmat [B,3,3]; optional: uvd2d
 * [B,30,3] (hybridbaseline.py:80-84), joints_rel / corners_rel (minus the predicted joint `center_idx`), boxroot [B,3]. */
int ab_pose_assemble(const float* kp3d, const float* box6d, int box_stride, const float* root_joint, const float* cam_intr,
                     const float* corners_can, int B, int center_idx, float res_w, float res_h, float* joints_abs,
                     float* corners_abs, float* rotmat, float* uvd2d, float* joints_rel, float* corners_rel, float* boxroot,
                     void* stream);
int ab_pose_loss(const float* kp3d, const float* box6d, int box_stride, const float* root_joint,
                 const float* cam_intr, const float* corners_can, const float* joints_3d, const float* corners_3d,
                 const float* joints_vis, const float* corners_vis, const float* hand_views, int nvh,
                 const int64_t* j0, const int64_t* j1, int njp, const int64_t* p0, const int64_t* p1, int npp,
                 const float* scene_views, int nvs, const int64_t* s0, const int64_t* s1, int nsp, int B,
                 int center_idx, float res_w, float res_h, const float* weights8_host, float* joints_abs,
                 float* corners_abs, float* rotmat, float* uvd2d, float* sample_part, float* losses, float* g_kp3d,
                 float* g_box6d, void* stream);
/* ab_pose_loss with SymCornerLoss (anakin/criterions/symcornerloss.py:49-102, use_ho3d_ycb = False) in the same kernel:
 * loss = mean_b min_k mean((sym_k(corners_gt) - pred)^2) over the object's symmetry set, vis-masked; its value goes to
 * loss_out[0], losses[5] (final) and the corner gradients include weight * lambda * loss.  sym == NULL or K == 0: absent. */
typedef struct ab_symcorner {
    const float* R;            /* device [nobj][K][3][3] (identity-padded)                       */
    const float* t;            /* device [nobj][K][3], metres                                     */
    int32_t K;
    const int64_t* obj_idx;    /* device [B], 1-based                                             */
    const float* obj_transf;   /* device [B][4][4]                                                */
    float lambda;              /* LAMBDA_SYM_CORNERS_3D                                           */
    float weight;              /* the Criterion LAMBDA of this loss                               */
    float* loss_out;           /* device [1], may be NULL                                         */
} ab_symcorner;
int ab_pose_loss_sym(const float* kp3d, const float* box6d, int box_stride, const float* root_joint,
                     const float* cam_intr, const float* corners_can, const float* joints_3d, const float* corners_3d,
                     const float* joints_vis, const float* corners_vis, const float* hand_views, int nvh,
                     const int64_t* j0, const int64_t* j1, int njp, const int64_t* p0, const int64_t* p1, int npp,
                     const float* scene_views, int nvs, const int64_t* s0, const int64_t* s1, int nsp, int B,
                     int center_idx, float res_w, float res_h, const float* weights8_host, const ab_symcorner* sym,
                     float* joints_abs, float* corners_abs, float* rotmat, float* uvd2d, float* sample_part, float* losses,
                     float* g_kp3d, float* g_box6d, void* stream);
/* The criterion of the regression-based model (HOPRegNet) in the same kernel, one launch + the finalize pass, deterministic:
 * replaces anakin/models/hpregnet.py:112-147 (joints_3d_abs = MANO joints + the TARGET's root_joint; corners_3d_abs =
 * ortho6d_to_rotmat(transf[3:9]) * corners_can + root_joint + transf[0:3]), anakin/criterions/honetloss.py:12-73 (ManoLoss: mean(shape^2),
 * mean(pose[:, 3:]^2), unmasked joint MSE), jointloss.py:25-67, ordinal.py:144-227, 262-306, criterion.py:57-67, the per-sample EPE of
 * anakin/metrics/val_metric.py:84-106, and their autograd backward.  joints_pred [B,21,3] (root-relative), mano_pca_pose [B,3+ncomps],
 * mano_shape [B,10], transf rows of 9 with pitch transf_stride >= 9.  An ordinal loss is present exactly when its draw buffers are passed.
 * weights12_host (HOST pointer) = the eight of ab_pose_loss, then LAMBDA_SHAPE_REG, LAMBDA_POSE_REG, ManoLoss's LAMBDA_JOINTS_3D,
 * LAMBDAS[ManoLoss].  outputs: joints_abs [B,21,3], corners_abs [B,8,3], rotmat [B,3,3], sample_part [B,8] ([5],[6] = joint / corner EPE in
 * mm, [7] = the sample's unmasked squared joint error), losses float[16] = the eight of ab_pose_loss, [8] mano_shape, [9] mano_pca_pose,
 * [10] ManoLoss's joints_3d_loss, [11] joints_loss_output, [12] hand_ord_loss_output, [13..15] zero; gradients of final_loss: g_joints
 * [B,21,3], g_pose [B,3+ncomps], g_shape [B,10], g_transf (pitch transf_stride; 9 values per row written).  NULL g_joints: forward only. */
int ab_reg_pose_loss(const float* joints_pred, const float* mano_pca_pose, const float* mano_shape, const float* transf,
                     int transf_stride, const float* root_joint, const float* cam_intr, const float* corners_can,
                     const float* joints_3d, const float* corners_3d, const float* joints_vis, const float* corners_vis,
                     const float* hand_views, int nvh, const int64_t* j0, const int64_t* j1, int njp, const int64_t* p0,
                     const int64_t* p1, int npp, const float* scene_views, int nvs, const int64_t* s0, const int64_t* s1,
                     int nsp, int B, int ncomps, const float* weights12_host, float* joints_abs, float* corners_abs,
                     float* rotmat, float* sample_part, float* losses, float* g_joints, float* g_pose, float* g_shape,
                     float* g_transf, void* stream);

/* ---- R3/R4/R5: batched online synthesis (rasterise + z-buffer + shade + background + colour jitter + crop) --------
 * replaces: anakin/utils/renderer.py:101-136 (Renderer.__call__: pyrender/OpenGL draw, background putmask),
 *           anakin/utils/frender_utils.py:36-46,116-118 (per-frame vertex upload, stale normals),
 *           anakin/artiboost/render_infra.py:14-59 (render server + two queue hops per image),
 *           anakin/artiboost/rendered_dataset.py:256-270 + anakin/utils/img_augment.py:6-80 (PIL jitter, affine, to_tensor)
 * ab_scene: HOST struct of DEVICE pointers to the immutable assets (one packed table for all object meshes).
 *   The hand mesh has V_dup >= 778 render vertices (UV-seam duplicates, as a textured trimesh has): hand_faces int32 [1538,3]
 *   index them, hand_uv [V_dup,2] / hand_normals [V_dup,3] are per render vertex, hand_map int32 [V_dup] gives the MANO
 *   vertex whose position a render vertex takes (renderer.py:17-28 get_mapping, :107 update_verts); NULL = identity.
 * samples : device array of 96-byte records {int32 obj_id, hand_tex_id, bg_id, bg_x0, bg_y0, bg_w, bg_h; float light;
 *           float obj_pose[16] (row-major 4x4)}.  hand_verts: float [B,778,3] camera frame.
 * The background is the record's crop rectangle resized to the render size with cv2.resize's INTER_LINEAR fixed-point
 * arithmetic (renderer.py:136); ab_scene.bg holds RGBX texels, uint8 [nbg, bgs, bgs, 4].
 * order/factor: int32/float [B,4] colour-jitter op ids (0 brightness, 1 saturation, 2 hue, 3 contrast) and factors in
 * application order.  inv_affine: float [B,6] output-pixel-centre -> render-pixel map (PIL AFFINE data).
 * blur_radius: float [B] (device) or NULL: PIL ImageFilter.GaussianBlur radius applied to the composited render before
 * the jitter (rendered_dataset.py:257-258, radius = U(0,1) * 0.1); each radius must be < 1.41 (box radius < 1 px).
 * out_pad: zero-bordered NHWC4 [B, oh+6, ow+8, 4] in out_dtype (interior written; border must already be zero);
 * out_chw: optional float [B,3,oh,ow] (the reference's `image` tensor).  keys_out (optional) uint64 [B,H,W]:
 * depth24<<32 | face id, ~0 = background.  rgbx_out (optional) uint8 [B,H,W,4] pre-jitter render.
 * ab_scene.srgb2lin: float [256], lin2srgb: uint8 [4096] (4-byte aligned: a tile with triangles copies it to LDS as words). */
typedef struct ab_scene {
    const void* hand_faces; const void* hand_normals; const void* hand_uv; const void* hand_map; const void* hand_tex; int hts;
    const void* obj_verts; const void* obj_normals; const void* obj_uv; const void* obj_faces;
    const void* obj_vert_off; const void* obj_face_off; const void* obj_tex; int ots;
    const void* bg; int bgs; const void* srgb2lin; const void* lin2srgb;
    float fx, fy, cx, cy; int W, H;
} ab_scene;
long ab_render_workspace_bytes(int B, int W, int H, int max_faces);
int ab_render_batch(const ab_scene* scene_host, const void* samples, const float* hand_verts, const int32_t* order,
                    const float* factor, const float* inv_affine, const float* blur_radius, int B, int max_faces,
                    int ow, int oh, int out_dtype, void* out_pad, float* out_chw, void* workspace, void* keys_out,
                    void* rgbx_out, void* stream);
/* The GaussianBlur stage of ab_render_batch on its own (PIL ImageFilter.GaussianBlur on the RGB bytes of B RGBX images,
 * W and H multiples of 32): radius float [B] on the device, each < 1.41; out must not alias rgbx.                  */
int ab_gaussian_blur(const void* rgbx, int B, int W, int H, const float* radius, void* out, void* stream);
/* SURVEY section 8f-3, the real-data half of MixedDataset: the augmentation chain of HOdata.__getitem__
 * (anakin/datasets/hodata.py:336-337,435-446) for B decoded frames of one size, RGBX uint8 [B,H,W,4] on the device:
 * optional Image.FLIP_LEFT_RIGHT (flip uint8 [B] or NULL), GaussianBlur (blur_radius [B] or NULL; needs W, H % 32 == 0),
 * colour jitter (order / factor as ab_render_batch), inverse-affine nearest crop to ow x oh, to_tensor - 0.5.
 * Outputs as ab_render_batch (zero-bordered NHWC4 in out_dtype and/or float CHW).                                   */
long ab_augment_workspace_bytes(int B, int W, int H);
int ab_augment_batch(const void* rgbx, int B, int W, int H, const int32_t* order, const float* factor,
                     const float* inv_affine, const float* blur_radius, const uint8_t* flip, int ow, int oh,
                     int out_dtype, void* out_pad, float* out_chw, void* workspace, void* stream);
/* SURVEY section 8f-3, the decode in front of that chain: baseline JPEG files -> RGB(X) frames on the device, bit-identical to what
 * `Image.open(path).convert("RGB")` returns in the reference's DataLoader workers (anakin/datasets/ho3d.py:228-231, dexycb.py:226-229,
 * fhb.py:257-260: Pillow / libjpeg-turbo defaults, JDCT_ISLOW + fancy up-sampling).  Huffman decode (self-synchronising, one thread per
 * `sub_bytes` of scan data, 16 <= sub_bytes <= 128), de-quantisation + integer IDCT, chroma up-sampling and colour conversion all run on the device; the host
 * only reads the marker segments (artiboost_amd/jpeg.py) into:
 *   data   the files' bytes (device; each image's scan is addressed through its descriptor)
 *   desc   int32 [n][AB_JPEG_DESC_INTS]: 0 scan offset in data, 1 scan bytes, 2 width, 3 height, 4 components (1 | 3), 5 hmax, 6 vmax,
 *          7.. per component (h, v, quant table, DC table, AC table) x 3, 22 restart interval (MCUs), 23 first row of `segs`, 24 segments,
 *          25 first subsequence, 26 subsequences, 27 first block, 28 blocks, 29 byte offset of its sample planes in the workspace,
 *          30 output offset (pixels), 31 output row pitch (pixels), 32 MCUs per row, 33 MCU rows, 34 blocks per MCU,
 *          35 index of its 4 quantisation tables in qtabs, 36 index of its 8 Huffman tables in htabs
 *   segs   int32 [.][4] per restart interval (one per image without restart markers): byte offset in the scan, bytes, first subsequence,
 *          first block (both relative to the image)
 *   qtabs  uint16 [.][4][64] in natural (row-major) order;  htabs  uint8 [.][8][16 + 256]: DC tables 0-3, AC tables 0-3 as in the DHT segment
 * max_blocks / max_width / max_height: the largest descriptor fields 28 / 2 / 3 of the batch.
 * out: uint8, out_channels 3 (RGB) or 4 (RGBX, X = 0).  Supported files: SOF0 / SOF1, 8 bit, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, restart
 * intervals; anything else is refused by the host parser (the caller keeps Pillow for those files, as the reference does for all).      */
#define AB_JPEG_DESC_INTS 40
/* workspace: coefficients, per-subsequence states, sample planes, the unstuffed scans, decode tables.  n_tables: sets of 8 Huffman tables in
 * htabs; data_bytes: bytes of `data`; total_segs: rows of segs; max_subseq: the largest descriptor field 26.                              */
long ab_jpeg_workspace_bytes(long total_blocks, long total_subseq, long plane_bytes, long data_bytes, long total_segs, int n, int n_tables);
int ab_jpeg_decode_batch(const void* data, const int32_t* desc, const int32_t* segs, const void* qtabs, const void* htabs, int n,
                         int n_tables, int sub_bytes, long total_blocks, long total_subseq, long plane_bytes, long data_bytes,
                         long total_segs, int max_blocks, int max_width, int max_height, int max_subseq, int out_channels, void* out,
                         void* workspace, void* stream);
/* SURVEY section 8f-3, the same decode for .png frames -- HO3D v2, the dataset of BASELINE.json's configs[1..3], stores rgb/NNNN.png
 * (anakin/datasets/ho3d.py:181, decoded at :228-231 by `Image.open(path).convert("RGB")`): the scanline reconstruction of the PNG
 * specification (filter types None / Sub / Up / Average / Paeth, what Pillow's libImaging/ZipDecode.c applies behind zlib) and the sample
 * selection of convert("RGB"), bit-identical.  The zlib inflate of the IDAT streams stays on the host (a thread pool, artiboost_amd/png.py).
 *   raw    the inflated scanlines of the n images (device): per image `height` lines of 1 filter byte + width * bpp sample bytes;
 *          the buffer must be readable for 8 bytes past the last line (samples are fetched 4 / 8 bytes at a time)
 *   desc   int32 [n][AB_PNG_DESC_INTS]: 0 / 1 byte offset of the image in raw (low / high word), 2 width, 3 height, 4 bytes per pixel
 *          (3 RGB8, 4 RGBA8, 6 RGB16, 8 RGBA16, 1 grey8), 5 byte offsets of the R, G, B samples inside a pixel as c0 | c1 << 8 | c2 << 16
 *          (16-bit samples: the high byte, as Pillow keeps), 6 output offset (pixels), 7 output row pitch (pixels)
 *   max_width / max_bpp: the largest descriptor fields 2 / 4 of the batch
 *   out    uint8, out_channels 3 (RGB) or 4 (RGBX, X = 0);  status (device int32 or NULL): bit 0 <- a filter byte above 4 was met
 * Interlaced, palette, 1/2/4-bit, 16-bit grey and grey + alpha files are refused by the host parser (the caller keeps Pillow for those).  */
#define AB_PNG_DESC_INTS 8
int ab_png_unfilter_batch(const void* raw, const int32_t* desc, int n, int max_width, int max_bpp, int out_channels, void* out, int* status,
                          void* stream);
/* Small-batch fp32 linear layers (the box-rotation MLP, anakin/models/mlp.py:11-25; nn.Linear weights [N][K]):
 *   fwd   y[M][N]  = act(x[M][K] W^T + bias)            (relu != 0: ReLU)
 *   dgrad gx[M][K] = (g[M][N] W) masked by act_out > 0   (act_out NULL: no mask); takes wt = W transposed, [K][N]
 *   wgrad dw[N][K] = g^T x, db[N] = column sums of g     (db may be NULL)      reduction lengths % 4 == 0.          */
int ab_linear_fwd(const float* x, const float* w, const float* bias, int M, int N, int K, int relu, float* y, void* stream);
int ab_linear_dgrad(const float* g, const float* wt, const float* act_out, int M, int N, int K, float* gx, void* stream);
int ab_linear_wgrad(const float* g, const float* x, int M, int N, int K, float* dw, float* db, void* stream);

/* ---- grasp refiner (anakin/artiboost/refiner.py) ------------------------------------------------
 * ab_nearest_dist replaces point2point_signed(hand_verts, verts_object) (refiner.py:21-83; nearest neighbour from the
 * third-party chamfer_distance CUDA extension) together with the rotated-object temporary of refiner.py:196-199:
 *   dist[b][i] = min_j || x[b][i] - rot[b] * y[j] ||   (+ per-vertex affine dist * scale[i] + shift[i], the eval-mode
 *   BatchNorm1d(778) of refiner.py:267, when scale != NULL), idx_out[b][i] = arg min (first minimum; optional).
 * x [B,P1,3]; ypts [nobj,P2,3] selected by obj_idx [B] (int64), or [B,P2,3] when obj_idx == NULL; rot [B,3,3] or NULL;
 * dist has row pitch ld >= P1.
 * ab_linear_fused: one layer of the RefineNet MLP (refiner.py:227-319, ResBlock :286-319), fp32:
 *   y[m][n] = act(((x W^T + bias) * scale[n] + shift[n]) + residual[m][n]), act 0 none / 1 ReLU / 2 leaky(slope);
 *   W [N][K], K % 4 == 0 (pad the features), scale/shift/residual/bias may be NULL, ldr / ldy = row pitches.        */
int ab_nearest_dist(const float* x, const float* ypts, const int64_t* obj_idx, const float* rot, int B, int P1, int P2,
                    const float* scale, const float* shift, float* dist, int ld, int32_t* idx_out, void* stream);
int ab_linear_fused(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                    const float* residual, int ldr, int M, int N, int K, int act, float slope, float* y, int ldy,
                    void* stream);
/* The colour-jitter chain of ab_render_batch on its own (anakin/utils/img_augment.py:6-80 on a PIL image): B RGBX images of
 * npix pixels, order int32 [B][4] (0 brightness, 1 saturation, 2 hue, 3 contrast), factor float [B][4]; out (RGBX, X =
 * 255) may alias rgbx; lsum_ws: B x 8 bytes of device scratch.                                                        */
int ab_color_jitter(const void* rgbx, int B, int npix, const int32_t* order, const float* factor, void* out,
                    void* lsum_ws, void* stream);

/* ---- R1: MANO linear-blend skinning ------------------------------------------------------------------------------
 * replaces manotorch.manolayer.ManoLayer.forward (third party, un-pinned git dependency, requirements.txt:178) at
 * anakin/artiboost/preprocessor.py:25,62, refiner.py:138,193,216,265, grasp_engine.py:90-95; maths as in the in-tree
 * anakin/postprocess/iknet/manolayer.py:182-276 (center_idx=None).  pose [B,48] axis-angle, betas [B,10];
 * model tables: v_template [778,3], shapedirs [778,3,10], posedirs [778,3,135], J_regressor [16,778],
 * weights [778,16], hands_mean [45].  Outputs verts [B,778,3], joints [B,21,3], T_abs [B,16,4,4] (optional).     */
int ab_mano_lbs(const float* pose, const float* betas, const float* v_template, const float* shapedirs,
                const float* posedirs, const float* J_regressor, const float* weights, const float* hands_mean,
                int B, float* verts, float* joints, float* T_abs, void* stream);

/* ---- MANO from PCA coefficients, forward and backward (the regression model's hand layer) ---------------------------
 * anakin/models/mano.py:46-137 (ManoBranch: ManoLayer(use_pca=True, ncomps, center_idx, flat_hand_mean=False)) and
 * anakin/models/hpregnet.py:75-104 (its call on the pose / shape regressions).  pose_coeffs [B,3+ncomps] (root axis-angle +
 * PCA coefficients), betas [B,10], comps [ncomps,45] (the first ncomps rows of hands_components), hands_mean [45], and the
 * tables of ab_mano_lbs.  full = [root | hands_mean + pca . comps] -> the maths of ab_mano_lbs (same Rodrigues, chain and
 * skinning code) -> verts [B,778,3], joints [B,21,3], both minus joint center_idx (-1: no centring); full_pose [B,48]
 * (optional).  1 <= ncomps <= 45.
 * ab_mano_pca_bwd: the exact reverse, from g_verts [B,778,3], g_joints [B,21,3] and g_full_pose [B,48] (optional) to
 * g_pose_coeffs [B,3+ncomps] and g_betas [B,10] (overwritten).  It recomputes the forward state itself; every reduction
 * runs in a fixed order (no atomics): the gradient is bit-reproducible.                                              */
int ab_mano_pca_fwd(const float* pose_coeffs, const float* betas, const float* comps, const float* hands_mean,
                    const float* v_template, const float* shapedirs, const float* posedirs, const float* J_regressor,
                    const float* weights, int ncomps, int center_idx, int B, float* verts, float* joints, float* full_pose,
                    void* stream);
int ab_mano_pca_bwd(const float* pose_coeffs, const float* betas, const float* comps, const float* hands_mean,
                    const float* v_template, const float* shapedirs, const float* posedirs, const float* J_regressor,
                    const float* weights, int ncomps, int center_idx, int B, const float* g_verts, const float* g_joints,
                    const float* g_full_pose, float* g_pose_coeffs, float* g_betas, void* stream);

/* ---- HoNet's recovery stage, forward and backward (the hand-mesh + object-vertices model's per-vertex stage) ------------------------
 * anakin/models/honetMANO.py:113-253 (recover_3d_proj, recover_mano, recover_object, forward).  hand_st: B rows of (scale, tx, ty),
 * obj_st: B rows of (scale, tx, ty, axis-angle 3), each addressed through its row pitch in floats (the first columns of padded head
 * outputs); cam_intr [B,9]; joints_3d [B,21,3] and hand_verts_3d [B,778,3] (MANO's, centred); obj_verts_can [B,N,3]; corners_can
 * [B,8,3] or NULL (then the three corner outputs are not touched).  Placement of both (honetMANO.py:126-139), focal = cam_intr[0]:
 *   Z0 = focal * scale * scale_factor + off_z,  XY0 = (trans * trans_factor + (img_w, img_h) / 2 - (cam_intr[2], cam_intr[5])) * Z0 / focal
 * root_joint / obj_center [B,3] = (XY0, Z0) of the hand / object; rotmat [B,9] = Rodrigues of the axis-angle (the device function of the
 * MANO kernels); *_abs = point + root_joint (hand) or rotmat . canonical + obj_center (object, corners); *_2d = cam_intr . p over its
 * depth; corners_3d / obj_verts_3d = *_abs - root_joint (obj_verts_3d may be NULL: not written).  N >= 1, any value.
 * ab_honet_recover_bwd: the exact reverse.  g_<output>: the gradient of each forward output, NULL = zero; the forward's inputs are read
 * again (nothing is saved between the launches).  Writes (overwrites) g_hand_st B rows of 3, g_obj_st B rows of 6 (row pitches
 * g_hand_pitch / g_obj_pitch), g_joints_3d [B,21,3], g_hand_verts_3d [B,778,3].  workspace: ab_honet_recover_workspace(B, N) bytes.
 * The vertices of a sample are split over ab_honet_recover_chunks(N) workgroups (+ one for the hand and the corners); the per-chunk sums
 * are added in chunk order by a second launch.  No float atomics, fixed-order reductions: bit-reproducible.                            */
int ab_honet_recover_chunks(int N);
long ab_honet_recover_workspace(int B, int N);
int ab_honet_recover_fwd(const float* hand_st, int hand_pitch, const float* obj_st, int obj_pitch, const float* cam_intr,
                         const float* joints_3d, const float* hand_verts_3d, const float* obj_verts_can, const float* corners_can,
                         int B, int N, float trans_factor, float scale_factor, float img_w, float img_h, float off_z,
                         float* root_joint, float* joints_3d_abs, float* hand_verts_3d_abs, float* joints_2d, float* hand_verts_2d,
                         float* obj_center, float* rotmat, float* obj_verts_3d_abs, float* obj_verts_2d, float* corners_3d_abs,
                         float* corners_2d, float* corners_3d, float* obj_verts_3d, void* stream);
int ab_honet_recover_bwd(const float* hand_st, int hand_pitch, const float* obj_st, int obj_pitch, const float* cam_intr,
                         const float* joints_3d, const float* hand_verts_3d, const float* obj_verts_can, const float* corners_can,
                         int B, int N, float trans_factor, float scale_factor, float img_w, float img_h, float off_z,
                         const float* g_root_joint, const float* g_joints_3d_abs, const float* g_hand_verts_3d_abs,
                         const float* g_joints_2d, const float* g_hand_verts_2d, const float* g_obj_center, const float* g_rotmat,
                         const float* g_obj_verts_3d_abs, const float* g_obj_verts_2d, const float* g_corners_3d_abs,
                         const float* g_corners_2d, const float* g_corners_3d, const float* g_obj_verts_3d, float* g_hand_st,
                         int g_hand_pitch, float* g_obj_st, int g_obj_pitch, float* g_joints_3d, float* g_hand_verts_3d,
                         void* workspace, void* stream);

/* ---- HoNet's mesh queries and fused mesh criterion (csrc/honet_loss.hip): what a captured HoNet training step runs around the network ----
 * ab_mesh_queries: artiboost_amd/synth.py add_mesh_queries in one launch.  table [n_obj,n,3] (synth.mesh_vertex_table), obj_id int64 [B],
 * obj_transf [B,4,4] (R | t), root_joint [B,3], hand_verts [B,778,3] (the epoch's un-augmented camera-frame vertices); the object pose is
 * read in place from the 96-byte render records: `samples` is their byte base, sample_pitch the record pitch and pose_offset the offset of
 * the row-major 4x4 `obj_pose` field, both in bytes and multiples of 4.  Writes, in full,
 *   obj_verts_can [B,n,3] = table[clamp(obj_id, 0, n_obj - 1)]   (bit copies; an id outside the table never reads outside it)
 *   obj_verts_3d  [B,n,3] = R . can + t - root
 *   hand_verts_3d [B,778,3] = (R . Rpose^T) . hand_verts - root
 * No allocation, no host read, no atomics; any n >= 1, B >= 1.
 * ab_honet_loss: anakin/criterions/honetloss.py:12-97 (ManoLoss: mean(shape^2), mean(pose[:, 3:]^2), joint MSE, hand-vertex MSE; ObjLoss:
 * object-vertex MSE), criterion.py:57-67, the per-sample EPE of anakin/metrics/val_metric.py:84-106, and their autograd backward.
 * Predictions: joints_3d_abs [B,21,3], hand_verts_3d_abs [B,778,3], obj_verts_3d_abs [B,N,3] (NULL with N = 0: no object term),
 * corners_3d_abs [B,8,3] or NULL, mano_pca_pose [B,3+ncomps], mano_shape [B,10].  Targets, root-relative (the kernel adds root_joint
 * [B,3], the TARGET's root): joints_3d, hand_verts_3d, obj_verts_3d, corners_3d; a NULL target drops its term (value 0, zero gradient).
 * weights7_host (HOST pointer) = LAMBDA_SHAPE_REG, LAMBDA_POSE_REG, ManoLoss's LAMBDA_JOINTS_3D, LAMBDA_HAND_VERTS_3D, LAMBDA_OBJ_VERTS_3D,
 * LAMBDAS[ManoLoss], LAMBDAS[ObjLoss].  The means are over B*10, B*ncomps, B*63, B*2334, B*N*3 elements.
 * Outputs: losses float[8] = mano_shape, mano_pca_pose, joints_3d_loss, hand_verts_3d_loss, obj_verts_3d_loss, final_loss, batch-mean joint
 * EPE, batch-mean corner EPE (mm); sample_part [B,8] = the sample's five squared sums, [5] / [6] its joint / corner EPE in mm (0 without
 * the target or the corners), [7] zero.  Gradients of final_loss, each written (overwritten) when its pointer is not NULL: g_joints_3d_abs,
 * g_hand_verts_3d_abs, g_obj_verts_3d_abs, g_mano_pca_pose (root-rotation columns zero), g_mano_shape.  workspace:
 * ab_honet_loss_workspace(B, N) bytes.  A sample's object vertices are split over ab_honet_loss_chunks(N) workgroups (+ one for the hand);
 * each reduces in a fixed order into its own row, a finalize launch adds the rows in chunk order and the samples in double.  No float
 * atomics: two calls give the same bits, and the loss bits do not depend on which gradients are asked for.
 * ab_real_mesh_queries: the same three queries for REAL frames (artiboost_amd/realdata.py RealBatcher).  The reference
 * has the getters (anakin/datasets/ho3d.py:253-262 get_hand_verts_3d, :376-385 get_obj_verts_can, :401-413 get_obj_verts_transf) but
 * HOdata.__getitem__ (hodata.py:315-450) never samples them; the definition is the per-point chain it applies to JOINTS_3D / CORNERS_3D
 * (flip :336-343, in-plane rotation :364-368, root subtraction :371-381).  table [n_rows,n,3] (datasets.HO3D.mesh_vertex_table), row int64
 * [B] (clamped into the table), obj_map / hand_map [B,3,4] row-major affine maps composed on the host in float64
 * (realdata.real_mesh_maps), mano_verts [B,778,3] (ab_mano_lbs on the frame's handPose / handBeta).  Writes, in full,
 *   obj_verts_can [B,n,3] = table[clamp(row, 0, n_rows - 1)]   (bit copies)
 *   obj_verts_3d  [B,n,3] = obj_map . [can; 1]         hand_verts_3d [B,778,3] = hand_map . [mano_verts; 1]
 * each coordinate ((m0 x + m1 y) + m2 z) + m3, unfused.  Grid and block of ab_mesh_queries.  B == 0 returns 0 without a launch; no
 * allocation, no host read, no atomics: two calls give the same bits.                                                                  */
int ab_mesh_queries(const float* table, int n_obj, int n, const int64_t* obj_id, const float* obj_transf, const float* root_joint,
                    const float* hand_verts, const uint8_t* samples, long sample_pitch, long pose_offset, int B, float* obj_verts_can,
                    float* obj_verts_3d, float* hand_verts_3d, void* stream);
int ab_real_mesh_queries(const float* table, int n_rows, int n, const int64_t* row, const float* obj_map, const float* hand_map,
                         const float* mano_verts, int B, float* obj_verts_can, float* obj_verts_3d, float* hand_verts_3d, void* stream);
int ab_honet_loss_chunks(int N);
long ab_honet_loss_workspace(int B, int N);
int ab_honet_loss(const float* joints_3d_abs, const float* hand_verts_3d_abs, const float* obj_verts_3d_abs, const float* corners_3d_abs,
                  const float* mano_pca_pose, const float* mano_shape, const float* root_joint, const float* joints_3d,
                  const float* hand_verts_3d, const float* obj_verts_3d, const float* corners_3d, int B, int N, int ncomps,
                  const float* weights7_host, float* sample_part, float* losses, float* g_joints_3d_abs, float* g_hand_verts_3d_abs,
                  float* g_obj_verts_3d_abs, float* g_mano_pca_pose, float* g_mano_shape, void* workspace, void* stream);

/* ---- Hand-mesh fitting of the submission pass (IKNet initialisation + 20 Adam steps of a MANO fit, all hands in one launch) -----
 * anakin/postprocess/iknet/fittingunit.py:112-225 (FittingUnit.__call__: residuals :63-80, geo :43-60, mano_de :83-97) and
 * utils.py:13-41 (quaternion -> axis-angle).  quat [B,64]: the raw IKNet output (16 quaternions, normalised here); pred_joints
 * [B,21,3]: the predicted absolute joints (root = joint 9).  MANO tables as ab_mano_lbs (flat hand mean) plus J_template [16,3] =
 * J_regressor . v_template and J_shapedirs [16,3,10] = J_regressor . shapedirs.  State in / out, [B,59] each (so3 48 | beta 10 |
 * bone 1): params and the Adam moments adam_m / adam_v; init != 0 starts from so3 = the hand's own IKNet pose, beta = 0, bone = the
 * predicted bone and zero moments (what the submit pass does), init == 0 reads them.  Runs n_iter Adam steps (lr 0.03, b1 = b2 =
 * 0.5, eps 1e-8) with step indices n = step0 .. step0 + n_iter - 1 (bias correction 1 - 0.5^(n+1)); the pose regulariser pulls
 * towards the mean of the WHOLE batch's IKNet poses, as in the reference.  Optional outputs: verts [B,778,3], joints [B,21,3] (the
 * fitted mesh, scaled by the predicted bone and moved to the predicted root), loss [B,n_iter] (the objective before each step),
 * grad [B,59] (the gradient of the last step).  0 <= n_iter, 0 <= step0, step0 + n_iter <= 120.  Fixed-order reductions only:
 * bit-reproducible.                                                                                                                   */
int ab_mano_fit(const float* quat, const float* pred_joints, const float* v_template, const float* shapedirs, const float* posedirs,
                const float* J_regressor, const float* weights, const float* J_template, const float* J_shapedirs, int B, int n_iter,
                int step0, int init, float* params, float* adam_m, float* adam_v, float* verts, float* joints, float* loss, float* grad,
                void* stream);

/* ---- Qualitative drawings of the submission pass (`--postprocess_draw`): two views of fitted hand + posed object per sample ----------
 * anakin/viztools/draw.py:400-449 (save_a_image_with_mesh_joints_objects), opendr_renderer.py:137-170 (three Lambertian point lights),
 * draw.py:236-276 (mayavi view azimuth -50, elevation 50, distance 0.6).  The reference draws with OpenDR / mayavi on the host, one
 * sample at a time; their pixels are not reproduced -- DESIGN.md section 18 defines this build's, tests/draw_oracle.py restates them.
 * out: uint8 [B, H, 4W, 3], the contact sheet; panels 2 (columns W .. 2W-1: the hand alone over the frame, the sample's cam_intr
 * [B,3,3] with identity extrinsic) and 3 (columns 2W .. 3W-1: hand and object on white from the orbit camera) are written, every pixel
 * of them; panels 1 and 4 are not touched.  image: the batch's float [B,3,H,W] tensor (frame - 0.5); an uncovered pixel of panel 2 is
 * floor(255 (image + 0.5) + 0.5) clamped to a byte.
 * hand_verts [B,778,3] (what ab_mano_fit returns), hand_faces [nhf,3], adj_off [779] / adj_face [nadj]: the faces around each hand
 * vertex (CSR, ascending face index; vertex normals are gathered in that order, no atomics).  Object library in canonical coordinates:
 * obj_verts / obj_normals [nov,3] and obj_faces [nof,3] (indices local to the object) packed, obj_vert_off / obj_face_off [n_obj+1];
 * max_obj_verts / max_obj_faces >= the largest object's counts (they size the vertex records and the grid; an object larger than that is
 * drawn without the faces that reach past it).  Per sample: obj_id [B] (>= 0 library object, -1 no object, -2 the 12-triangle box over
 * corners[b], eight points indexed 4 ix + 2 iy + iz), obj_rot [B,3,3] and obj_tsl [B,3] (X = R v + t), corners [B,8,3] (may be NULL when no
 * sample asks for the box).  The library pointers may be NULL with n_obj == 0.
 * workspace: ab_draw_workspace_bytes(B, W, H, max_obj_verts) bytes.  After the call it holds, from byte 0, the vertex records
 * [B, 778 + max(max_obj_verts, 8), 12] (int32 words: sx0 sy0 zq0 sx1 sy1 zq1 | float zv0 zv1 r g b | flags; view 0 = camera, 1 = orbit;
 * screen positions in 1/256 px, zq the 24-bit inverse depth, flags bit v = usable in view v) and, from byte
 * ab_draw_workspace_keys_offset(B, max_obj_verts), the depth keys uint64 [B, 2, H, W] (zq << 32 | face, hand faces first; all ones =
 * uncovered) -- the stage outputs the tests compare.  W, H <= 4096.  Integer atomicMin only: bit-reproducible.                      */
long ab_draw_workspace_bytes(int B, int W, int H, int max_obj_verts);
long ab_draw_workspace_keys_offset(int B, int max_obj_verts);
int ab_draw_meshes(const float* hand_verts, const int32_t* hand_faces, int nhf, const int32_t* adj_off, const int32_t* adj_face, int nadj,
                   const float* obj_verts, const float* obj_normals, const int32_t* obj_faces, const int32_t* obj_vert_off,
                   const int32_t* obj_face_off, int n_obj, int nov, int nof, int max_obj_verts, int max_obj_faces, const int32_t* obj_id,
                   const float* obj_rot, const float* obj_tsl, const float* corners, const float* cam_intr, const float* image, int B, int W,
                   int H, uint8_t* out, void* workspace, void* stream);

/* ---- Maximum symmetry-aware surface distance of the evaluator (csrc/mssd.hip) -----------------------------------
 * anakin/metrics/bopAR.py:131-175 (MSSD.feed) and val_metric.py:272-320: what AR and ValMetricAR2 accumulate.  Per sample b, with the
 * symmetry set S = sym[clamp(obj_idx[b] - 1, 0, n_obj - 1)] at its TRUE length sym_count[obj] (clamped to 0 .. Kmax),
 *   mssd[b] = min over k < sym_count of max over v < V of || R_gt (S_k.R can_v + S_k.t) + t_gt - pred_v - c_b ||      (metres)
 * can [B,V,3]; obj_transf [B,4,4] row-major (R_gt | t_gt in its first three rows; the fourth is not read); obj_idx int64 [B], 1-based, an
 * id outside the table is clamped into it (as ab_mesh_queries does); sym_R [n_obj,Kmax,9] row-major, sym_t [n_obj,Kmax,3] in metres,
 * sym_count int32 [n_obj]: entries of a table row at or past its count are never read.  An empty set (count < 1) gives +inf.
 *   rigid mode  (pred_pts NULL): pred_v = pred_R[b] can_v + pred_t[b] with pred_R [B,9] (box_rot_rotmat), pred_t [B,3] (boxroot_3d_abs);
 *                                the residual is one 3x4 affine map per (b, k) applied to can_v.
 *   points mode (pred_pts [B,V,3], pred_R and pred_t NULL): pred_v read from memory (MSSD_USE_CORNERS: corners_3d_abs).
 * center [B,3] or NULL (zero): c_b = root_joint - joints_3d_abs[:, center_idx] of MSSD_USE_CENTER_IDX.  USE_HO3D_YCB needs no mode: the
 * sign flips fold into the table (ext S.R ext, ext S.t), exactly.
 * mssd [B] is written in full.  workspace: ab_mssd_workspace(B, Kmax, V) bytes (one partial per sample and chunk of 64 symmetries).
 * Squared lengths are compared and ONE square root is taken at the end.  No atomics; a vertex's residual does not depend on where the
 * vertex or the sample sits and max / min are order-independent, so the bits are the same across calls, for a sample alone or inside a
 * batch, and under repetition padding of the vertices.  1 <= B <= 65535, V >= 1, n_obj >= 1, 1 <= Kmax <= 64 * 65535.                  */
long ab_mssd_workspace(int B, int Kmax, int V);
int ab_mssd(const float* can, const float* obj_transf, const int64_t* obj_idx, const float* sym_R, const float* sym_t,
            const int32_t* sym_count, int n_obj, int Kmax, const float* pred_R, const float* pred_t, const float* pred_pts,
            const float* center, int B, int V, float* mssd, void* workspace, void* stream);

/* ---- Mesh-level registry losses, eager route only (csrc/mesh_align.hip) --------------------------------------------
 * ab_chamfer_rigid: anakin/criterions/chamferloss.py:11-52 over the brute-force nearest neighbour of criterions.chamfer_distance_torch.
 * can [B,N,3], rot [B,9] row-major (box_rot_rotmat), tsl [B,3] (boxroot_3d_abs), targ [B,M,3] (obj_verts_3d), root [B,3] (root_joint, added
 * to targ), corners_vis [B,8] fp32: keep = any(corners_vis != 0) is formed in the kernel.  Per sample
 *   x_i = keep (R can_i + t),  y_j = keep (targ_j + root),  dist_xy[i] = min_j |x_i - y_j|^2,  dist_yx[j] = min_i |x_i - y_j|^2
 * as sums of squared differences (never |x|^2 + |y|^2 - 2 x.y: that form cancels at 0.5 m depth and millimetre distances); the first
 * minimum wins on ties, as in argmin and ab_nearest_dist.
 *   loss[1] = sum dist_xy / (B N) + sum dist_yx / (B M)
 * dist_xy [B,N], dist_yx [B,M], idx_xy int32 [B,N] (into y), idx_yx int32 [B,M] (into x): each optional (NULL).  g_rot [B,9] and g_tsl [B,3]
 * (both or neither): the gradient of loss, the nine rotation entries free variables as autograd treats them,
 *   g_i = (2 / (B N)) (x_i - y_i*) + sum over j with j* = i of (2 / (B M)) (x_i - y_j),   g_tsl = keep sum g_i,   g_rot = keep sum g_i can_i^T,
 * each target's term folded straight into the two sums: no [B,N,3] and no [N,M] is materialised.  A masked sample (keep = 0) writes zero
 * distances, zero indices and zero gradients without scanning and still counts in both means (the reference's behaviour, kept on purpose).
 * Meshes padded by repetition hold exact duplicates; which duplicate wins a tie does not change g_rot or g_tsl: duplicates share can_i.
 * workspace: ab_chamfer_rigid_workspace(B, N, M) bytes (16 floats per sample and chunk of 256 query points of either cloud).  No atomics:
 * partial sums are added in a fixed order by a second small launch, so two calls give the same bits, and a sample's distances, indices
 * and B-fold gradients (B a power of two) do not depend on the batch around it.  1 <= B <= 65535, N, M >= 1.
 *
 * ab_procrustes_loss: anakin/criterions/alignloss.py:52-80 plus the MSE; one wave per sample, one launch for the batch and a small one for
 * the mean.  pred [B,n,3] (joints_3d_abs), targ [B,n,3] (joints_3d), root [B,3] (added to targ), n >= 3 (the model: 21).  With Xh, Ph the
 * centred clouds over (their Frobenius norm + 1e-8), c the target's norm term, M = Xh^T Ph = u w v^T, R = u v^T (NO determinant correction:
 * a mirrored hand aligns by a reflection, as in the reference) and s = sum w:
 *   aligned [B,n,3] (optional) = s c R Ph_i + centroid(targ + root);   sample_loss [B] = c^2 sum_i |s R Ph_i - Xh_i|^2 / (3 n), computed from
 *   the residual (1 - s^2 loses its digits for a near-perfect prediction);   loss[1] = mean of sample_loss, summed in a fixed order;
 *   g_pred [B,n,3] (optional) = d loss / d pred: R is the optimum, so d loss / d M = -2 c^2 s R / (3 n B) without an SVD backward, then
 *   through Ph = Pc / p and the centring.
 * A rank-deficient M (coplanar or collinear joints) gives finite numbers everywhere; the gradient there is unspecified (the reference's
 * torch.svd backward is not finite there either).  Deterministic; sample_loss, aligned and B-fold g_pred (B a power of two) do not depend
 * on the batch around the sample.  B >= 1, 3 <= n <= 2^24.
 * Neither entry point is captured in a hipGraph anywhere in this project: TrainStep refuses such a step.          */
long ab_chamfer_rigid_workspace(int B, int N, int M);
int ab_chamfer_rigid(const float* can, const float* rot, const float* tsl, const float* targ, const float* root, const float* corners_vis,
                     int B, int N, int M, float* loss, float* dist_xy, float* dist_yx, int32_t* idx_xy, int32_t* idx_yx, float* g_rot,
                     float* g_tsl, void* workspace, void* stream);
int ab_procrustes_loss(const float* pred, const float* targ, const float* root, int B, int n, float* sample_loss, float* loss,
                       float* aligned, float* g_pred, void* stream);

/* ---- Leaderboard mesh metrics of the evaluator, eager only (csrc/mesh_metrics.hip) ----------------------------------
 * What HO3D / DexYCB results are published in: the Procrustes-aligned and root-relative errors, the mesh F-scores and ADD-S.
 * pred [B,N,3], targ [B,M,3] fp32; root [B,3] or NULL (zero), added to targ; center_idx: the centre point of the root-relative error, or
 * < 0 (none); thresholds_host: T <= AB_MM_MAX_THRESHOLDS F-score thresholds in metres, a HOST array read during the call; flags: which
 * groups to compute.  AB_MM_PAIRED and AB_MM_PROCRUSTES need N == M, AB_MM_PROCRUSTES N >= 3, center_idx < N: AB_EINVAL otherwise.
 * Per sample, with P = pred[b] and G = targ[b] + root[b]:
 *   AB_MM_PAIRED      epe = mean_i |P_i - G_i|;  ra_epe = mean_i |(P_i - P_c) - (G_i - G_c)|, c = center_idx (NaN when center_idx < 0)
 *   AB_MM_PROCRUSTES  the similarity of ab_procrustes_loss, formed as that entry point forms `aligned` (same normalisation by the Frobenius
 *                     norms + 1e-8, same one-sided Jacobi, finite numbers for rank-deficient clouds): with Pc, Gc the centred clouds and
 *                     K = Gc^T Pc = U S V^T,  R = U V^T with NO determinant correction (a mirrored prediction aligns by a reflection, as
 *                     in AlignLoss and the public FreiHAND / HO3D scoring scripts),  s = tr S / |Pc|^2,  P'_i = s R Pc_i + centroid(G);
 *                     pa_epe = mean_i |P'_i - G_i|,  scale = s.  The two entry points agree on P' to rounding.
 *   AB_MM_NN          for Q = P and, with AB_MM_PROCRUSTES, Q = P':  d_pg[i] = min_j |Q_i - G_j|,  d_gp[j] = min_i |Q_i - G_j|  as sums of
 *                     squared differences (never |x|^2 + |y|^2 - 2 x.y), squared lengths compared, one square root per point;
 *                     mean_pg, mean_gp their means (mean_gp is ADD-S: the mean over the posed ground-truth points of the distance to the
 *                     nearest predicted point);  per threshold t:  precision = #{d_pg < t} / N,  recall = #{d_gp < t} / M  (strict <; the
 *                     points of a cloud padded by repetition each count),  F = 2 p r / (p + r), 0 when p + r = 0.
 * rows [B, AB_MM_ROW] fp32, written in full: the AB_MM_* slots below; a group that was not asked for, ra_epe without a centre and the
 * F slots at or past T are NaN.  counts int32 [B, T, 4]: per threshold #{d_pg < t}, #{d_gp < t}, then the same two of the aligned scan
 * (zero where the scan was not asked for).  d_pg [B,N], d_gp [B,M], pa_d_pg [B,N], pa_d_gp [B,M]: the per-point distances in metres,
 * each optional (NULL).  workspace: ab_mesh_metrics_workspace(B, N, M) bytes (the similarity of each sample, one partial per sample, scan
 * and chunk of 256 query points).  Three launches: one wave per sample for the paired sums and the similarity; one workgroup per (sample,
 * scan, direction, chunk), applying the similarity as it stages or forms the points, so no aligned [B,N,3] is written; one thread per
 * sample adding its chunks in turn.  No atomics: two calls give the same bits, and a sample's row, counts and distances do not depend on
 * the batch around it.  1 <= B <= 65535, 1 <= N, M <= 2^24.
 * Like the two mesh losses above, this entry point is not captured in a hipGraph anywhere in this project (DESIGN.md sections 19 and 23):
 * the evaluator is fed outside the replayed graphs.                                                                                      */
#define AB_MM_PAIRED 1
#define AB_MM_PROCRUSTES 2
#define AB_MM_NN 4
#define AB_MM_MAX_THRESHOLDS 4
#define AB_MM_ROW 16           /* floats per sample row: */
#define AB_MM_EPE 0
#define AB_MM_RA_EPE 1
#define AB_MM_PA_EPE 2
#define AB_MM_SCALE 3
#define AB_MM_MEAN_PG 4
#define AB_MM_MEAN_GP 5        /* ADD-S */
#define AB_MM_PA_MEAN_PG 6
#define AB_MM_PA_MEAN_GP 7
#define AB_MM_F 8              /* [AB_MM_MAX_THRESHOLDS] */
#define AB_MM_PA_F 12          /* [AB_MM_MAX_THRESHOLDS] */
long ab_mesh_metrics_workspace(int B, int N, int M);
int ab_mesh_metrics(const float* pred, const float* targ, const float* root, int B, int N, int M, int center_idx,
                    const float* thresholds_host, int T, int flags, float* rows, int32_t* counts, float* d_pg, float* d_gp, float* pa_d_pg,
                    float* pa_d_gp, void* workspace, void* stream);

/* ---- Hand-object interaction measures of the evaluator, eager only (csrc/interact.hip) ------------------------------
 * Whether the predicted hand is inside the predicted object or never touches it: maximum / mean penetration depth, smallest distance,
 * contact, and the intersection volume of the two meshes on a lattice.  Definitions, for a mesh of triangles (a, b, c) and a query q, with
 * A = a - q, B = b - q, C = c - q:
 *   solid angle     num = A . (B x C),  den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|,  Omega = 2 atan2(num, den), 0 when both are 0
 *   winding number  w(q) = sum_f Omega_f / (4 pi)
 *   orientation     o = sign(sum_f a . (b x c)), the sign of the mesh's signed volume, computed by the HOST per mesh in float64 and passed
 *                   in (hand_orient, obj_orient [n_obj], each +-1); the kernel assumes no sign
 *   inside          o w(q) > 0.5 (the meshes need not be watertight: the winding number degrades gracefully where a ray parity is undefined)
 *   distance        d(q) = min_f |q - cp_f(q)|, cp_f the closest point of triangle f by the region form, every division guarded (a zero
 *                   denominator gives parameter 0); sums of squared differences, squared lengths compared, one square root per query
 * Faces with a repeated index are dropped by the host when it builds the face tables.
 * hand_verts [B,Nh,3] fp32; hand_faces int32 [Fh,3] (needed with AB_IA_VOLUME only).  The objects are one packed table: obj_verts [*,3],
 * obj_faces int32 [*,3] with indices LOCAL to the object, vert_off / face_off int32 [n_obj + 1]; obj_row int64 [B] selects the object
 * (clamped into the table); rot [B,3,3], tsl [B,3]: the object mesh of sample b is rot[b] can + tsl[b].  A query is taken into the
 * canonical frame once, q' = rot[b]^T (q - tsl[b]), and the canonical triangles are scanned from the table; no posed face list is written.
 *   AB_IA_VERTS    hand vertex i against the object: inside_i, d_i;  pen_max = max over inside vertices of d_i (0 when none), pen_mean their
 *                  mean (0 when none), min_dist = min_i d_i, inside_frac = n_inside / Nh, contact = 1 when n_inside > 0 or
 *                  min_dist <= contact_thr, else 0.  sdf [B,Nh]: -d_i inside, +d_i outside; wind [B,Nh]: o w; each optional (NULL).
 *   AB_IA_VOLUME   the lattice points p = voxel (i + 1/2, j + 1/2, k + 1/2), integer i, j, k, of the CAMERA frame (so a sample's value does
 *                  not depend on the batch around it) inside the intersection of the axis-aligned boxes of the hand vertices and of the
 *                  posed object vertices: n_lattice of them; n_both are inside the object AND inside the hand mesh (hand_orient);
 *                  volume = n_both voxel^3.  More than max_voxels lattice points: nothing is scanned, volume NaN, capped = 1.
 * rows [B, AB_IA_ROW] fp32, written in full: the slots below, metres and cubic metres; a group that was not asked for and the two
 * reserved slots are NaN.  counts int32 [B,4]: n_inside, n_lattice, n_both, capped (zero where not asked for).  workspace:
 * ab_interaction_workspace(B, Nh, max_voxels) bytes.  Launches: one workgroup of 256 threads per (sample, chunk of 256 hand vertices), the
 * triangles through LDS in SoA tiles; one workgroup per sample for the boxes and index ranges; a FIXED grid of ceil(max_voxels / 256)
 * chunks per sample whose workgroups leave at once past n_lattice or when the sample is capped (the host reads nothing back between the
 * launches); one thread per sample adding its chunks in turn.  No atomics: two calls give the same bits, and a sample's row, counts, sdf
 * and wind do not depend on the batch around it.  1 <= B <= 65535, 1 <= Nh, Fh <= 2^24, 1 <= max_voxels <= 2^24, voxel > 0,
 * contact_thr >= 0, every object >= 1 face: AB_EINVAL otherwise (the tables' contents are trusted; indices are clamped into their mesh).
 * Like the three mesh entry points above, this one is not captured in a hipGraph anywhere in this project (DESIGN.md sections 19, 23, 24):
 * the evaluator is fed outside the replayed graphs.                                                                                      */
#define AB_IA_VERTS 1
#define AB_IA_VOLUME 2
#define AB_IA_ROW 8            /* floats per sample row: */
#define AB_IA_PEN_MAX 0
#define AB_IA_PEN_MEAN 1
#define AB_IA_MIN_DIST 2
#define AB_IA_INSIDE_FRAC 3
#define AB_IA_CONTACT 4
#define AB_IA_VOL 5            /* m^3; slots 6, 7 reserved (NaN) */
long ab_interaction_workspace(int B, int Nh, int max_voxels);
int ab_interaction(const float* hand_verts, const int32_t* hand_faces, int Nh, int Fh, float hand_orient, const float* obj_verts,
                   const int32_t* obj_faces, const int32_t* vert_off, const int32_t* face_off, const float* obj_orient, int n_obj,
                   const int64_t* obj_row, const float* rot, const float* tsl, int B, float contact_thr, float voxel, int max_voxels, int flags,
                   float* rows, int32_t* counts, float* sdf, float* wind, void* workspace, void* stream);

/* ---- Contact loss: hand-object repulsion and attraction with their gradient, eager only (csrc/contact_loss.hip) ------
 * The contact loss of Hasson et al. (CVPR 2019) on the quantities of ab_interaction, for training: hand vertices inside the posed object
 * are pushed out, contact zones that do not touch it are pulled in.  The object of sample b is rot[b] can + tsl[b] from the packed table
 * of ab_interaction (same arguments); a hand vertex q is taken into the canonical frame once, q' = rot[b]^T (q - tsl[b]).
 *   distance     d(q) and the closest point cp'(q) by the triangle region form of ab_interaction, the first minimum in face order winning;
 *                the residual r' = q' - cp' is the sum of differences that form leaves, d = |r'|.
 *   box          obj_box [n_obj,6] (lo xyz | hi xyz): the closed axis-aligned box of each object's canonical vertices, exact in fp32,
 *                formed once per object by the host.
 *   inside(q)    q' in box AND o w(q) > 0.5 (w the generalised winding number, o the table's orientation).  A vertex outside the box is
 *                outside by definition and its winding number is not computed.
 *   candidates   q' in box, or zone_id >= 0: the vertices that can contribute; only they are scanned.
 *   repulsion    rep[b] = (1 / Nh) sum over inside vertices of rho tanh(d / rho)
 *   attraction   zone_id int32 [Nh] (shared by the batch; NULL allowed when Z == 0): -1, or any value outside 0 .. Z-1, = no zone.  For zone
 *                z, among its vertices that are NOT inside, d_z is the smallest d, the lowest vertex index winning ties; a zone without
 *                such a vertex contributes 0.  The box does not limit attraction.  att[b] = (1 / max(Z, 1)) sum_z alpha tanh(d_z / alpha)
 *   loss         loss[0] = (lambda_r sum_b m_b rep[b] + lambda_a sum_b m_b att[b]) / B;  m_b = 0 for a sample whose obj_row is outside
 *                [0, n_obj) or whose mask (fp32 [B], optional) is 0: it still counts in B, nothing of it is scanned, rep[b] = att[b] = 0,
 *                its counts are 0, its sdf NaN and its gradients 0.
 *   gradient     analytic, cp' held fixed (it minimises the distance): d = |q - (rot[b] cp' + tsl[b])|.  With n = rot[b] r' / d and
 *                s = sech^2(d / scale), a contributing vertex gets g_q = weight s n, 0 when d == 0: weight lambda_r m_b / (B Nh) and scale
 *                rho for an inside vertex, weight lambda_a m_b / (B max(Z, 1)) and scale alpha for a zone's winner.  The two sets are
 *                disjoint; every other vertex gets exactly 0.  g_tsl[b] = -sum g_q;  g_rot[b] = -sum g_q cp'^T, the nine rotation entries
 *                free variables (the convention of ab_chamfer_rigid).  g_hand [B,Nh,3], g_rot [B,9], g_tsl [B,3]: all three or none.
 * counts int32 [B,2]: n_inside, n_candidates.  sdf [B,Nh] (optional): NaN for a vertex that is no candidate, -d for an inside vertex, +d
 * for any other candidate.  AB_CL_SCAN_ALL scans every vertex of an unmasked sample instead of its candidates; what it scans beyond them
 * is dropped, so every output has the same bits with and without it (the A/B of tools/bench_contact_loss.py).
 * workspace: ab_contact_loss_workspace(B, Nh) bytes.  Launches: classify and compact (one workgroup per sample; the candidates as an
 * ascending index list by ballots and prefix counts), scan (a FIXED grid of ceil(Nh / 256) chunks of 256 candidates per sample; a
 * workgroup past the list leaves at once, the host reads nothing back; triangles through LDS in tiles of 512), finalize (one workgroup per
 * sample: zone winners, terms, gradients, the 12 pose sums), one workgroup for the batch.  No atomics: two calls give the same bits, and a
 * sample's rep, att, sdf, counts and B x its gradients do not depend on the batch around it for B a power of two.
 * 1 <= B <= 65535, 1 <= Nh <= 2^24, 0 <= Z <= 16, rho > 0, alpha > 0: AB_EINVAL otherwise (the tables' contents are trusted).
 * Like the mesh losses above, this entry point is not captured in a hipGraph anywhere in this project (DESIGN.md sections 19, 26).       */
#define AB_CL_SCAN_ALL 1
long ab_contact_loss_workspace(int B, int Nh);
int ab_contact_loss(const float* hand_verts, const int32_t* zone_id, int Nh, int Z, const float* obj_verts, const int32_t* obj_faces,
                    const int32_t* vert_off, const int32_t* face_off, const float* obj_orient, const float* obj_box, int n_obj,
                    const int64_t* obj_row, const float* rot, const float* tsl, const float* mask, int B, float rho, float alpha,
                    float lambda_r, float lambda_a, int flags, float* loss, float* rep, float* att, int32_t* counts, float* sdf,
                    float* g_hand, float* g_rot, float* g_tsl, void* workspace, void* stream);

/* ---- Symmetric interaction measures: object vertices inside the hand mesh, eager only (csrc/interact_sym.hip) --------
 * The reverse direction of ab_interaction: the vertices of the sample's object are the queries, the posed hand's triangles the mesh.  A
 * small or pointed object pressed into the palm has no hand vertex inside it while dozens of its vertices are inside the hand.  Solid
 * angle, winding number w, orientation o, "inside <=> o w > 0.5", the closest point by the region form and the first minimum in face order
 * are those of the comment block of ab_interaction above, computed by the same functions (csrc/ia_tile.h): a distance has the same bits.
 * hand_verts [B,Nh,3] fp32, hand_faces int32 [Fh,3] (indices clamped into [0, Nh) while staging), hand_orient +-1 from the host.  The
 * objects are the packed table of ab_interaction, of which only obj_verts [*,3] and vert_off int32 [n_obj + 1] are read (the object's
 * faces and orientation play no part in this direction); r = obj_row[b] clamped into [0, n_obj), No_r = min(vert_off[r+1] - vert_off[r],
 * No_max) canonical vertices c_i.
 *   frame          each hand vertex is taken into the object's canonical frame once, v' = rot[b]^T (v - tsl[b]) (the arithmetic of
 *                  ab_interaction's queries); the queries are the canonical vertices c_i straight from the table.  No posed object vertex
 *                  is formed, and coordinates stay within the object's extent.
 *   per vertex     inside_i <=> hand_orient w_hand'(c_i) > 0.5;  d_i = the distance of c_i to the hand's triangles
 *   per sample     obj_pen_max = max over inside vertices of d_i (0 when none), obj_pen_mean their mean (0 when none),
 *                  obj_min_dist = min_i d_i, obj_inside_frac = n_obj_inside / No_r, obj_contact = 1 when n_obj_inside > 0 or
 *                  obj_min_dist <= contact_thr, else 0
 *   optional       sdf_obj [B,No_max]: -d_i inside, +d_i outside; wind_obj [B,No_max]: o w; entries at i >= No_r are NaN (each may be NULL)
 * No query is culled by the hand's box: on a mesh that is not watertight (the stand-in hand's kept face list has boundary loops and
 * non-manifold edges) a vertex outside the box can still have o w > 0.5, and the definition does not depend on a shortcut.
 * rows [B, AB_IAS_ROW] fp32, written in full, metres: the slots below, the reserved ones NaN.  counts int32 [B,2]: n_obj_inside, No_r.
 * workspace: ab_interaction_sym_workspace(B, Nh, No_max) bytes (the canonical hand vertices [B,Nh,3] and four words per chunk).
 * Launches: (1) one thread per (sample, hand vertex) writes the canonical hand; (2) a FIXED grid of ceil(No_max / 256) chunks x B samples,
 * 256 threads, one object vertex per thread, the hand's triangles through LDS in SoA tiles of 512: a workgroup whose chunk starts at or
 * past No_r fills its slots of sdf_obj / wind_obj with NaN and leaves before any barrier, lanes past No_r of the last live chunk compute
 * on a clamped vertex and are masked out of every reduction; a chunk leaves n_inside, the sum and maximum of the inside depths and the
 * smallest distance in the workspace (ballot and popcount, wave butterflies, the four waves in turn); (3) one thread per sample adds its
 * live chunks in turn and writes the row and the counts.  The host reads nothing back between the launches.  No atomics:
 * two calls give the same bits, and a sample's row, counts, sdf_obj and wind_obj do not depend on the batch around it.  1 <= B <= 65535, 1 <= Nh, Fh, No_max <= 2^24, n_obj >= 1, contact_thr >= 0, hand_orient +-1, rows and counts
 * non-NULL: AB_EINVAL otherwise (the tables' contents are trusted).
 * Like ab_interaction, this entry point is not captured in a hipGraph anywhere in this project (DESIGN.md sections 19, 24, 27).          */
#define AB_IAS_ROW 8           /* floats per sample row: */
#define AB_IAS_OBJ_PEN_MAX 0
#define AB_IAS_OBJ_PEN_MEAN 1
#define AB_IAS_OBJ_MIN_DIST 2
#define AB_IAS_OBJ_INSIDE_FRAC 3
#define AB_IAS_OBJ_CONTACT 4   /* slots 5..7 reserved (NaN) */
long ab_interaction_sym_workspace(int B, int Nh, int No_max);
int ab_interaction_sym(const float* hand_verts, const int32_t* hand_faces, int Nh, int Fh, float hand_orient, const float* obj_verts,
                       const int32_t* vert_off, int n_obj, const int64_t* obj_row, const float* rot, const float* tsl, int B, int No_max,
                       float contact_thr, float* rows, int32_t* counts, float* sdf_obj, float* wind_obj, void* workspace, void* stream);

/* ---- BOP pose errors of the evaluator, eager only (ab_mspd: csrc/mssd.hip, ab_vsd: csrc/bop_recall.hip) ---------------
 * The two errors of bop_toolkit's pose_error.py that, with ab_mssd, make the BOP average recall: MSPD and VSD.
 *
 * ab_mspd: per sample b, with the symmetry set of ab_mssd (same table layout, same sym_count semantics, same clamping of obj_idx),
 *   mspd[b] = min over k < sym_count of max over v < V of || proj(pred_v) - proj(R_gt (S_k.R can_v + S_k.t) + t_gt) ||      (pixels)
 *   proj(X, Y, Z) = (fx X / Z + cx, fy Y / Z + cy) with cam_intr [B,9] row-major (fx, cx, fy, cy read from slots 0, 2, 4, 5; no skew).
 * Rigid mode (pred_pts NULL): pred_v = pred_R[b] can_v + pred_t[b]; points mode (pred_pts [B,V,3], pred_R and pred_t NULL): read from
 * memory.  A point whose camera-space Z is <= 0 in either pose makes the sample's error +inf (bop_toolkit divides by Z regardless and
 * mirrors such a point through the principal point; here it is reported as what it is).  An empty set gives +inf.  fp32 throughout; squared
 * distances are compared and ONE square root is taken at the end.  workspace: ab_mspd_workspace(B, Kmax, V) bytes.  No atomics: the bits are
 * the same across calls and for a sample alone or inside a batch.  1 <= B <= 65535, V >= 1, n_obj >= 1, 1 <= Kmax <= 64 * 65535.
 *
 * ab_vsd: Visible Surface Discrepancy (pose_error.vsd, cost_type "step", visibility mode bop19) of a whole batch, fused: the three depth
 * images live in LDS, one 32 x 32 tile at a time, and reach memory only through depth_out.
 * The object is row clamp(rows[b], 0, n_obj - 1) of the packed table of ab_interaction (obj_verts [*,3], obj_faces int32 [*,3] with LOCAL
 * indices, vert_off / face_off int32 [n_obj + 1]); max_obj_verts is the largest vertex count of the table (a mesh with more keeps its
 * first max_obj_verts vertices; a face with an index outside its mesh is dropped).  rot_est / rot_gt [B,9], tsl_est / tsl_gt [B,3]: the
 * estimated and the ground-truth pose; cam_intr [B,9]; depth_test [B,H,W] fp32 or NULL (all zero), 0 = no measurement; the occluder
 * (both or neither): occ_verts [B,Nv,3] in the CAMERA frame, occ_faces int32 [Nf,3].  All lengths in one unit (the project's: metres):
 * delta, diameter fp32 [n_obj] (per table row), taus_host: T <= AB_VSD_MAX_TAUS fp32 values in a HOST array read during the call.
 * With an occluder, the test depth of a pixel is the nearest of the occluder, the object under the ground truth and depth_test where
 * that is > 0 (what a depth sensor would have seen); without one it is depth_test as given.
 * The stages are the contract that makes the result checkable bit for bit (restated in tests/bop_raster_ref.py):
 *   A  fp32, this operation order, no FMA (the library is built with -ffp-contract=off):  camera point ((r0 x + r1 y) + r2 z) + t per row;
 *      u = fx (X / Z) + cx, v = fy (Y / Z) + cy;  snapped to 1/256 px by floorf(u 256 + 0.5).  Pixel (x, y) is sampled AT (x, y) -- BOP's
 *      convention (depth_im_to_dist_im_fast: pre_Xs = (x - cx) / fx) --, not at x + 1/2.  A triangle is dropped when a vertex has
 *      Z <= AB_VSD_NEAR, when a snapped coordinate lies outside [-AB_VSD_RANGE, AB_VSD_RANGE] (with W, H <= 8192 every edge product stays
 *      below 2^48), or when its area is zero.  No back-face culling; a clockwise triangle has its second and third vertex swapped.
 *   B  integers: E0 = edge(v1, v2, p), E1 = edge(v2, v0, p), E2 = edge(v0, v1, p) in int64, edge(a, b, p) = (bx - ax)(py - ay) - (by - ay)(px - ax);
 *      covered when all are >= 0 and every zero one belongs to a top or left edge (dy > 0, or dy == 0 and dx < 0): render.hip's rule.
 *   C  float64, this order:  l_i = (double)E_i / (double)A, A = E0 + E1 + E2;  Z = 1 / ((l0 / Z0 + l1 / Z1) + l2 / Z2);  rounded to fp32; the
 *      nearest surface wins by an unsigned minimum over the bit patterns (positive floats): order-independent, so the image is the same
 *      on every call.  A pixel no triangle covers has depth 0.
 *   D  float64 per pixel, the order of bop_toolkit:  pX = ((double)x - cx) / fx, pY likewise;  L = sqrt(((pX d)^2 + (pY d)^2) + d^2) for
 *      each of the three depths d;  visible(L) = ((float)L - (float)L_test <= delta or L_test == 0) and L > 0;  vis_gt = visible(L_gt),
 *      vis_est = visible(L_est) or (vis_gt and L_est > 0);  per tau: cost = |L_gt - L_est| (/ diameter when normalized_by_diameter) >= tau
 *      over the intersection.
 * counts int32 [B, 2 + T]: union pixels, complement pixels (union minus intersection), the cost count per tau.  err fp32 [B,T]:
 * (cost_t + complement) / union formed in float64 and rounded, 1.0 where the union is empty.  depth_out [B,3,H,W] or NULL: the est, gt
 * and test depth images.  workspace: ab_vsd_workspace(B, max_obj_verts, Nv, W, H, T) bytes (a 16-byte record per projected vertex, 2 + T
 * partial counts per tile).  Three launches (vertex setup; one workgroup per (sample, tile); one workgroup per sample adding its tiles in
 * turn).  The only atomics are the LDS minima of stage C; counts are integers added in a fixed order: two calls give the same bits and a
 * sample does not depend on the batch around it.  1 <= B <= 65535, 1 <= W, H <= 8192, 1 <= T <= AB_VSD_MAX_TAUS, delta >= 0.
 * Neither entry point is captured in a hipGraph anywhere in this project: the evaluator is fed outside the replayed graphs.              */
#define AB_VSD_MAX_TAUS 16
#define AB_VSD_NEAR 0.01f      /* metres */
#define AB_VSD_RANGE 4194304   /* 2^22 snapped units = 16 384 px */
long ab_mspd_workspace(int B, int Kmax, int V);
int ab_mspd(const float* can, const float* obj_transf, const int64_t* obj_idx, const float* sym_R, const float* sym_t,
            const int32_t* sym_count, int n_obj, int Kmax, const float* pred_R, const float* pred_t, const float* pred_pts,
            const float* cam_intr, int B, int V, float* mspd, void* workspace, void* stream);
long ab_vsd_workspace(int B, int max_obj_verts, int Nv, int W, int H, int T);
int ab_vsd(const float* obj_verts, const int32_t* obj_faces, const int32_t* vert_off, const int32_t* face_off, int n_obj,
           int max_obj_verts, const int64_t* rows, const float* rot_est, const float* tsl_est, const float* rot_gt, const float* tsl_gt,
           const float* cam_intr, int B, int W, int H, const float* depth_test, const float* occ_verts, const int32_t* occ_faces, int Nv,
           int Nf, float delta, const float* taus_host, int T, const float* diameter, int normalized_by_diameter, int32_t* counts,
           float* err, float* depth_out, void* workspace, void* stream);

/* ---- Argument contracts of the dispatcher ops (torch.ops.artiboost_hip.*, libartiboost_torch.so) ------------------------------------------
 * The C entry points above take raw pointers and trust their caller.  Their PyTorch-dispatcher form (ops that "validate
 * with TORCH_CHECK") is generated from this header by artiboost_amd/gen_torch_ops.py and checks, before the C call, for EVERY op:
 *   - a tensor passed for a device pointer is a contiguous HIP tensor of the current device; one passed for a host pointer (`*_host`, the
 *     ab_* descriptor structs) is a contiguous CPU tensor;
 *   - a typed pointer fixes the dtype: float* float32, int32_t* / int* int32, int64_t* int64, uint8_t* uint8;
 * and, per op, the clauses of its `@check` line below (C expressions over the op's integer arguments; co() = convolution output size):
 *   names >= expr        every named tensor holds at least `expr` elements (a wrong B / H / C no longer overruns a buffer: RuntimeError)
 *   bytes names >= expr  ... at least `expr` bytes (workspaces)
 *   bf16|u8|i32|f32: names     dtype of `void*` arguments
 *   dt(code): names            dtype given by the op's AB_DT_* argument `code`
 *   strided: names             arguments the op addresses through a row-pitch argument (ld*, *_stride): non-contiguous views are accepted
 * A violated clause raises RuntimeError naming the op, the argument and both sizes; nothing is launched.
 * @check ab_softargmax3d_fwd: dt(dtype): logits; logits >= B*H*W*C*DP; part >= B*ab_softargmax3d_ntiles(H,W)*C*8; uvd >= B*C*3; conf >= B*C; stat >= B*C*2
 * @check ab_softargmax3d_bwd: dt(dtype): logits dlogits; logits dlogits >= B*H*W*C*DP; uvd g_uvd >= B*C*3; conf g_conf >= B*C; stat >= B*C*2
 * @check ab_softargmax3d_bwd_x3: bf16: dl_hi dl_lo; logits dl_hi dl_lo >= B*H*W*C*DP; uvd g_uvd >= B*C*3; conf g_conf >= B*C; stat >= B*C*2
 * @check ab_split_f32: bf16: hi lo; src hi lo >= n
 * @check ab_cast_f32_bf16: bf16: dst; src dst >= n
 * @check ab_conv2d_fwd_x3: bf16: x_hi x_lo w_hi w_lo; x_hi x_lo >= N*H*W*Cin; w_hi w_lo >= Cout*kh*kw*Cin; y >= N*co(H,kh,stride,pad)*co(W,kw,stride,pad)*Cout; bias >= Cout; stats >= ab_conv2d_x3_stat_rows(N,H,W,Cin,Cout,kh,kw,stride,pad)*Cout*2
 * @check ab_conv1x1_sam_fwd_x3: bf16: x_hi x_lo w_hi w_lo; x_hi x_lo >= B*H*W*Cin; w_hi w_lo >= C*32*Cin; bias >= C*32; logits >= B*H*W*C*32; part >= B*(H*W/64)*C*8
 * @check ab_softargmax3d_stage2: part >= B*ntile*C*8; uvd >= B*C*3; conf >= B*C; stat >= B*C*2
 * @check ab_conv2d_fwd_x3_evalbn: bf16: x_hi x_lo w_hi w_lo res_hi res_lo out_hi out_lo; x_hi x_lo >= N*H*W*Cin; w_hi w_lo >= Cout*9*Cin; bnp >= 2*Cout; res_hi res_lo res_f32 out_hi out_lo out_f32 >= N*H*W*Cout
 * @check ab_conv2d_fwd_x3_affine: bf16: x_hi x_lo w_hi w_lo out_hi out_lo; x_hi x_lo >= N*H*W*Cin; w_hi w_lo >= Cout*kh*kw*Cin; scale shift >= Cout; out_f32 out_hi out_lo >= N*co(H,kh,stride,pad)*co(W,kw,stride,pad)*Cout
 * @check ab_conv2d_dgrad_x3: bf16: dy_hi dy_lo wt_hi wt_lo; dy_hi dy_lo >= N*co(H,kh,stride,pad)*co(W,kw,stride,pad)*Cout; wt_hi wt_lo >= Cin*kh*kw*Cout; dx addend >= N*H*W*Cin
 * @check ab_conv2d_dgrad_x3_pair: bf16: dy_hi dy_lo wt_hi wt_lo dy2_hi dy2_lo wt2_hi wt2_lo; dy_hi dy_lo dy2_hi dy2_lo >= N*(H/2)*(W/2)*Cout; wt_hi wt_lo >= Cin*kh*kw*Cout; wt2_hi wt2_lo >= Cin*Cout; dx addend >= N*H*W*Cin
 * @check ab_conv2d_dgrad_x3_pair_bn: bf16: dy_hi dy_lo wt_hi wt_lo dy2_hi dy2_lo wt2_hi wt2_lo bn_out_hi; dy_hi dy_lo dy2_hi dy2_lo >= N*(H/2)*(W/2)*Cout; wt_hi wt_lo >= Cin*kh*kw*Cout; wt2_hi wt2_lo >= Cin*Cout; dz bn_y bn_out_hi >= N*H*W*Cin; bnp >= 4*Cin; bn_part >= ab_conv2d_dgrad_x3_pair_bn_rows(N,H,W,Cin,Cout,kh,kw,pad)*Cin*2
 * @check ab_conv2d_dgrad_x3_bn: bf16: dy_hi dy_lo wt_hi wt_lo bn_out_hi; dy_hi dy_lo >= N*co(H,kh,stride,pad)*co(W,kw,stride,pad)*Cout; wt_hi wt_lo >= Cin*kh*kw*Cout; dz addend bn_y bn_out_hi >= N*H*W*Cin; bnp >= 4*Cin; bn_part >= ab_conv2d_dgrad_x3_bn_rows(N,H,W,Cin,Cout,kh,kw,stride,pad)*Cin*2
 * @check ab_conv2d_wgrad_x3: bf16: x_hi x_lo dy_hi dy_lo; x_hi x_lo >= N*H*W*Cin; dy_hi dy_lo >= N*co(H,kh,stride,pad)*co(W,kw,stride,pad)*Cout; dw >= Cout*kh*kw*Cin; bytes workspace >= ab_conv2d_wgrad_x3_workspace(N,H,W,Cin,Cout,kh,kw,stride,pad)
 * @check ab_conv2d_stem_fwd_x3: bf16: xpad_hi xpad_lo w_hi w_lo; xpad_hi xpad_lo >= N*(H+6)*(W+8)*4; w_hi w_lo >= Cout*7*8*4; y >= N*(H/2)*(W/2)*Cout; stats >= ab_conv2d_stem_x3_stat_rows(N,H,W)*Cout*2
 * @check ab_conv2d_wgrad_x3_group: bytes workspace >= ab_conv2d_wgrad_x3_group_workspace(G,N,H,W,Cin,Cout)
 * @check ab_conv2d_stem_wgrad_x3: bf16: xpad_hi xpad_lo dy_hi dy_lo; xpad_hi xpad_lo >= N*(H+6)*(W+8)*4; dy_hi dy_lo >= N*(H/2)*(W/2)*Cout; dw >= Cout*7*8*4
 * @check ab_conv2d_fwd: dt(dtype): x w y; x >= N*H*W*Cin; w >= Cout*kh*kw*Cin; y >= N*co(H,kh,stride,pad)*co(W,kw,stride,pad)*Cout; bias >= Cout
 * @check ab_conv2d_dgrad: dt(dtype): dy wt dx addend; dy >= N*co(H,kh,stride,pad)*co(W,kw,stride,pad)*Cout; wt >= Cin*kh*kw*Cout; dx addend >= N*H*W*Cin
 * @check ab_bn_apply_x3: bf16: out_hi out_lo; y res out out_hi out_lo >= M*C; bnp >= 2*C
 * @check ab_bn_apply_x3_respl: bf16: res_hi res_lo out_hi out_lo; y res_hi res_lo out out_hi out_lo >= M*C; bnp >= 2*C
 * @check ab_bn_fin_apply_x3: bf16: res_hi res_lo out_hi out_lo; part >= nparts*C*2; gamma beta running_mean running_var >= C; bnp >= 4*C; res_bnp >= 2*C; y res res_hi res_lo out out_hi out_lo >= M*C
 * @check ab_bn_bwd_x3: bf16: dy_hi dy_lo; dout y dy_hi dy_lo dz_out >= M*C; bnp >= 4*C; dgamma dbeta >= C
 * @check ab_bn_finalize: part >= nparts*C*2; gamma beta running_mean running_var >= C; bnp >= 4*C
 * @check ab_bn_eval_params: gamma beta rm rv >= C; bnp >= 4*C
 * @check ab_col_stats: dt(dtype): x; x >= M*C; part >= ab_col_stats_nparts(M)*C*2
 * @check ab_bn_relu_maxpool3x3s2_fwd_x3w: bf16: out_hi out_lo; y >= N*H*W*C; bnp >= 2*C; out out_hi out_lo ywin >= N*(H/2)*(W/2)*C; bytes idx >= N*(H/2)*(W/2)*C
 * @check ab_avgpool_fwd: dt(dtype): x; x >= N*HW*C; out >= N*C
 * @check ab_image_pad_nhwc4: dt(dtype): out; img_nchw >= N*3*H*W; out >= N*(H+6)*(W+8)*4
 * @check ab_grad_norm: grad >= n; total_norm >= 1
 * @check ab_scale_f32: x >= n
 * @check ab_clip_adam: bf16: lp; param grad m v lp >= n; total_norm >= 1
 * @check ab_clip_adam_x3: bf16: lp_hi lp_lo; param grad m v lp_hi lp_lo >= n; total_norm >= 1
 * @check ab_pose_assemble: strided: box6d; kp3d >= B*22*3; root_joint >= B*3; cam_intr >= B*9; corners_can >= B*24; joints_abs joints_rel >= B*63; corners_abs corners_rel >= B*24; rotmat >= B*9; uvd2d >= B*90
 * @check ab_pose_loss: strided: box6d g_box6d; kp3d g_kp3d >= B*22*3; root_joint >= B*3; cam_intr >= B*9; corners_can corners_3d >= B*24; joints_3d >= B*63; joints_vis >= B*21; corners_vis >= B*8; hand_views >= nvh*3; scene_views >= nvs*3; j0 j1 >= njp; p0 p1 >= npp; s0 s1 >= nsp; weights8_host >= 8
 * @check ab_render_batch: bytes samples >= B*96; hand_verts >= B*778*3; order factor >= B*4; inv_affine >= B*6; blur_radius >= B; dt(out_dtype): out_pad; out_pad >= B*(oh+6)*(ow+8)*4; out_chw >= B*3*oh*ow
 * @check ab_gaussian_blur: u8: rgbx out; rgbx out >= B*W*H*4; radius >= B
 * @check ab_augment_batch: u8: rgbx; rgbx >= B*W*H*4; order factor >= B*4; inv_affine >= B*6; blur_radius flip >= B; dt(out_dtype): out_pad; out_pad >= B*(oh+6)*(ow+8)*4; out_chw >= B*3*oh*ow; bytes workspace >= ab_augment_workspace_bytes(B,W,H)
 * @check ab_color_jitter: u8: rgbx out; rgbx out >= B*npix*4; order factor >= B*4; bytes lsum_ws >= B*8
 * @check ab_jpeg_decode_batch: u8: data out; bytes data >= data_bytes; desc >= n*AB_JPEG_DESC_INTS; segs >= total_segs*4; bytes qtabs >= n*4*64*2; bytes htabs >= n_tables*8*272; bytes workspace >= ab_jpeg_workspace_bytes(total_blocks,total_subseq,plane_bytes,data_bytes,total_segs,n,n_tables)
 * @check ab_png_unfilter_batch: u8: raw out; desc >= n*AB_PNG_DESC_INTS; status >= 1
 * @check ab_linear_fwd: x >= M*K; w >= N*K; bias >= N; y >= M*N
 * @check ab_linear_dgrad: g act_out >= M*N; wt >= K*N; gx >= M*K
 * @check ab_linear_wgrad: g >= M*N; x >= M*K; dw >= N*K; db >= N
 * @check ab_nearest_dist: strided: dist; x >= B*P1*3; rot >= B*9; obj_idx >= B; scale shift >= P1; idx_out >= B*P1
 * @check ab_pose_loss_sym: strided: box6d g_box6d; kp3d g_kp3d >= B*22*3; root_joint >= B*3; cam_intr >= B*9
 * @check ab_reg_pose_loss: strided: transf g_transf; joints_pred joints_3d joints_abs g_joints >= B*63; mano_pca_pose g_pose >= B*(3+ncomps); mano_shape g_shape >= B*10; root_joint >= B*3; cam_intr >= B*9; corners_can corners_3d corners_abs >= B*24; joints_vis >= B*21; corners_vis >= B*8; rotmat >= B*9; sample_part >= B*8; losses >= 16; hand_views >= nvh*3; scene_views >= nvs*3; j0 j1 >= njp; p0 p1 >= npp; s0 s1 >= nsp; weights12_host >= 12
 * @check ab_linear_fused: strided: residual y; x >= M*K; w >= N*K; bias scale shift >= N
 * @check ab_mano_lbs: pose >= B*48; betas >= B*10; v_template >= 778*3; shapedirs >= 778*3*10; posedirs >= 778*3*135; J_regressor >= 16*778; weights >= 778*16; hands_mean >= 45; verts >= B*778*3; joints >= B*21*3; T_abs >= B*16*16
 * @check ab_mano_pca_fwd: pose_coeffs >= B*(3+ncomps); betas >= B*10; comps >= ncomps*45; hands_mean >= 45; v_template >= 778*3; shapedirs >= 778*3*10; posedirs >= 778*3*135; J_regressor >= 16*778; weights >= 778*16; verts >= B*778*3; joints >= B*21*3; full_pose >= B*48
 * @check ab_mano_pca_bwd: pose_coeffs g_pose_coeffs >= B*(3+ncomps); betas g_betas >= B*10; comps >= ncomps*45; hands_mean >= 45; v_template >= 778*3; shapedirs >= 778*3*10; posedirs >= 778*3*135; J_regressor >= 16*778; weights >= 778*16; g_verts >= B*778*3; g_joints >= B*21*3; g_full_pose >= B*48
 * @check ab_honet_recover_fwd: strided: hand_st obj_st; cam_intr rotmat >= B*9; joints_3d joints_3d_abs >= B*63; hand_verts_3d hand_verts_3d_abs >= B*778*3; obj_verts_can obj_verts_3d_abs obj_verts_3d >= B*N*3; corners_can corners_3d_abs corners_3d >= B*24; root_joint obj_center >= B*3; joints_2d >= B*42; hand_verts_2d >= B*778*2; obj_verts_2d >= B*N*2; corners_2d >= B*16
 * @check ab_honet_recover_bwd: strided: hand_st obj_st g_hand_st g_obj_st; cam_intr g_rotmat >= B*9; joints_3d g_joints_3d_abs g_joints_3d >= B*63; hand_verts_3d g_hand_verts_3d_abs g_hand_verts_3d >= B*778*3; obj_verts_can g_obj_verts_3d_abs g_obj_verts_3d >= B*N*3; corners_can g_corners_3d_abs g_corners_3d >= B*24; g_root_joint g_obj_center >= B*3; g_joints_2d >= B*42; g_hand_verts_2d >= B*778*2; g_obj_verts_2d >= B*N*2; g_corners_2d >= B*16; bytes workspace >= ab_honet_recover_workspace(B,N)
 * @check ab_mesh_queries: table >= n_obj*n*3; obj_id >= B; obj_transf >= B*16; root_joint >= B*3; hand_verts hand_verts_3d >= B*778*3; bytes samples >= (B-1)*sample_pitch+pose_offset+64; obj_verts_can obj_verts_3d >= B*n*3
 * @check ab_real_mesh_queries: table >= n_rows*n*3; row >= B; obj_map hand_map >= B*12; mano_verts hand_verts_3d >= B*778*3; obj_verts_can obj_verts_3d >= B*n*3
 * @check ab_honet_loss: joints_3d_abs joints_3d g_joints_3d_abs >= B*63; hand_verts_3d_abs hand_verts_3d g_hand_verts_3d_abs >= B*778*3; obj_verts_3d_abs obj_verts_3d g_obj_verts_3d_abs >= B*N*3; corners_3d_abs corners_3d >= B*24; mano_pca_pose g_mano_pca_pose >= B*(3+ncomps); mano_shape g_mano_shape >= B*10; root_joint >= B*3; weights7_host >= 7; sample_part >= B*8; losses >= 8; bytes workspace >= ab_honet_loss_workspace(B,N)
 * @check ab_mano_fit: quat >= B*64; pred_joints >= B*63; v_template >= 778*3; shapedirs >= 778*3*10; posedirs >= 778*3*135; J_regressor >= 16*778; weights >= 778*16; J_template >= 48; J_shapedirs >= 480; params adam_m adam_v grad >= B*59; verts >= B*778*3; joints >= B*63; loss >= B*n_iter
 * @check ab_draw_meshes: hand_verts >= B*778*3; hand_faces >= nhf*3; adj_off >= 779; adj_face >= nadj; obj_verts obj_normals >= nov*3; obj_faces >= nof*3; obj_vert_off obj_face_off >= n_obj+1; obj_id >= B; obj_rot >= B*9; obj_tsl >= B*3; corners >= B*24; cam_intr >= B*9; image >= B*3*H*W; out >= B*H*4*W*3; bytes workspace >= ab_draw_workspace_bytes(B,W,H,max_obj_verts)
 * @check ab_mssd: can pred_pts >= B*V*3; obj_transf >= B*16; obj_idx mssd >= B; sym_R >= n_obj*Kmax*9; sym_t >= n_obj*Kmax*3; sym_count >= n_obj; pred_R >= B*9; pred_t center >= B*3; bytes workspace >= ab_mssd_workspace(B,Kmax,V)
 * @check ab_chamfer_rigid: can >= B*N*3; rot g_rot >= B*9; tsl root g_tsl >= B*3; targ >= B*M*3; corners_vis >= B*8; loss >= 1; dist_xy idx_xy >= B*N; dist_yx idx_yx >= B*M; bytes workspace >= ab_chamfer_rigid_workspace(B,N,M)
 * @check ab_procrustes_loss: pred targ aligned g_pred >= B*n*3; root >= B*3; sample_loss >= B; loss >= 1
 * @check ab_mesh_metrics: pred >= B*N*3; targ >= B*M*3; root >= B*3; thresholds_host >= T; rows >= B*AB_MM_ROW; counts >= B*T*4; d_pg pa_d_pg >= B*N; d_gp pa_d_gp >= B*M; bytes workspace >= ab_mesh_metrics_workspace(B,N,M)
 * @check ab_interaction: hand_verts >= B*Nh*3; hand_faces >= Fh*3; vert_off face_off >= n_obj+1; obj_verts >= 3; obj_faces >= 3; obj_orient >= n_obj; obj_row >= B; rot >= B*9; tsl >= B*3; rows >= B*AB_IA_ROW; counts >= B*4; sdf wind >= B*Nh; bytes workspace >= ab_interaction_workspace(B,Nh,max_voxels)
 * @check ab_contact_loss: hand_verts g_hand >= B*Nh*3; zone_id >= Nh; vert_off face_off >= n_obj+1; obj_verts >= 3; obj_faces >= 3; obj_orient >= n_obj; obj_box >= n_obj*6; obj_row mask rep att >= B; rot g_rot >= B*9; tsl g_tsl >= B*3; loss >= 1; counts >= B*2; sdf >= B*Nh; bytes workspace >= ab_contact_loss_workspace(B,Nh)
 * @check ab_interaction_sym: hand_verts >= B*Nh*3; hand_faces >= Fh*3; vert_off >= n_obj+1; obj_verts >= 3; obj_row >= B; rot >= B*9; tsl >= B*3; rows >= B*AB_IAS_ROW; counts >= B*2; sdf_obj wind_obj >= B*No_max; bytes workspace >= ab_interaction_sym_workspace(B,Nh,No_max)
 * @check ab_mspd: can pred_pts >= B*V*3; obj_transf >= B*16; obj_idx mspd >= B; sym_R >= n_obj*Kmax*9; sym_t >= n_obj*Kmax*3; sym_count >= n_obj; pred_R cam_intr >= B*9; pred_t >= B*3; bytes workspace >= ab_mspd_workspace(B,Kmax,V)
 * @check ab_vsd: obj_verts >= 3; obj_faces >= 3; vert_off face_off >= n_obj+1; rows >= B; rot_est rot_gt cam_intr >= B*9; tsl_est tsl_gt >= B*3; depth_test >= B*H*W; occ_verts >= B*Nv*3; occ_faces >= Nf*3; taus_host >= T; diameter >= n_obj; counts >= B*(2+T); err >= B*T; depth_out >= B*3*H*W; bytes workspace >= ab_vsd_workspace(B,max_obj_verts,Nv,W,H,T)
 */

#ifdef __cplusplus
}
#endif
#endif
