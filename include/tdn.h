/*
 * tdn.h — C ABI of libtdn.so, the MI355X (gfx950) native hot path behind the
 * Torch_Detection module registry.
 *
 * The reference (TCGGroup/Torch_Detection) has NO native interface: every hot
 * operation is a torch.nn call made from Python.  Each entry point below names
 * the reference call site (file:line, relative to the reference root) whose
 * arithmetic it replaces.  The only intended binder is ctypes from
 * torch_detection_amd/_lib.py (see INTEGRATION.md for the stub a reference
 * maintainer would add).
 *
 * Conventions
 *   - All tensors are caller-owned device memory (PyTorch allocations).  The
 *     library never allocates, frees or synchronises; every kernel is enqueued
 *     on the hipStream_t passed as `stream` (void*; NULL = default stream).
 *   - Activations / gradients are NHWC ("channels last"), 2-byte elements: the
 *     `dtype` argument says which — TDN_BF16 (bfloat16) or TDN_F16 (IEEE half;
 *     the reference's model.half()).  Every 16-bit operand of one call has that
 *     type; accumulation, BN/bias constants and all parameter gradients are fp32.
 *     Weights are pre-packed K-major in the same type by tdn_pack_conv_weight.
 *   - Return value: 0 = ok, negative = error; tdn_last_error() returns a
 *     thread-local message.  Nothing throws across the boundary.
 *   - Re-entrant: no global mutable state besides the thread-local error text.
 */
#ifndef TDN_H_
#define TDN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDN_VERSION 100 /* 0.1.0 */

enum { TDN_BF16 = 0, TDN_F16 = 1 };

/* epilogue addend modes */
enum {
  TDN_ADD_NONE = 0,
  TDN_ADD_SAME = 1,     /* addend has the output's shape (residual `out += residual`, resnet.py:57,117) */
  TDN_ADD_UP2X = 2,     /* addend is the 2x coarser map, nearest-upsampled (fpn.py:99-101)                */
  TDN_ADD_SUMPOOL2 = 3  /* addend is the 2x finer map, 2x2 sum-pooled (adjoint of fpn.py:99-101)         */
};

/* Fused epilogue applied to the fp32 accumulator of a conv / dgrad GEMM:
 *   v = acc * scale[c] + shift[c]          (eval-mode BatchNorm2d folded, layers.py:50-54; or conv bias, layers.py:93)
 *   v += addend(...)                        (see modes above)
 *   if relu:      v = max(v, 0)             (nn.ReLU, resnet.py:35,90,217); relu == 2: v = min(v, 6) as well
 *                                           (nn.ReLU6, layers.py:117-118), values under 6 stay under 6 when stored
 *   if mask_src:  v = mask_src > 0 ? v : 0  (adjoint of that ReLU, from the saved forward output)
 *   out = (bf16) v          (or fp32 when out_f32 != 0: pre-rounding value, used for 1e-3 parity checks
 *                             and for fp32 module outputs)
 */
typedef struct tdn_epilogue {
  const float* scale;    /* [Cout] or NULL (= 1) */
  const float* shift;    /* [Cout] or NULL (= 0) */
  const void* addend;    /* NHWC, Cout channels, or NULL */
  int32_t addend_mode;   /* TDN_ADD_* */
  int32_t addend_h;      /* spatial size of the addend tensor (UP2X / SUMPOOL2) */
  int32_t addend_w;
  int32_t relu;          /* 0 none / 1 ReLU / 2 ReLU6 */
  const void* mask_src;  /* NHWC, same shape as the output, or NULL */
  int32_t out_f32;       /* 0: out is bf16 NHWC; 1: out is float32 NHWC */
  int32_t reserved;
} tdn_epilogue;

const char* tdn_last_error(void);
int tdn_version(void);

/* ---- weight / norm preparation ------------------------------------------------ */

/* Eval-mode BatchNorm2d folded to a per-channel affine (layers.py:50-54, resnet.py:270-276):
 *   invstd = 1/sqrt(var+eps); scale = gamma*invstd; shift = beta - mean*scale. */
int tdn_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                float eps, int C, float* scale, float* shift, float* invstd, void* stream);

/* Pack an nn.Conv2d weight (layers.py:12,25,40,93) for the GEMM kernels.
 *   w: fp32, logical [Cout][Cin][kh][kw] with element strides (s_o, s_i, s_h, s_w).
 *   w_fwd:   bf16 [Cout][kh][kw][Cin]                       (forward / wgrad-finalize operand)
 *   w_dgrad: bf16 [Cin][kh][kw][Cout] = scale[co] * w      (may be NULL; dgrad operand, BN scale folded)
 */
int tdn_pack_conv_weight(const float* w, int64_t s_o, int64_t s_i, int64_t s_h, int64_t s_w,
                         int Cout, int Cin, int kh, int kw, const float* scale,
                         void* w_fwd, void* w_dgrad, int dtype, void* stream);

/* Stem variant (conv7x7_group(3,64,stride=2), resnet.py:214): w fp32 [64][3][7][7] contiguous ->
 * bf16 [Cout][7][8][4] (kw padded 7->8, channels padded 3->4, pads zero). */
int tdn_pack_stem_weight(const float* w, int Cout, void* w_fwd, int dtype, void* stream);

/* ---- convolution (nn.Conv2d.forward via resnet.py:42-59,97-119,253-258; fpn.py:92-108) ---- */

/* y[N][Ho][Wo][Cout] = epilogue(conv(x[N][H][W][Cin], w_fwd)), square kernel k in {1,3},
 * stride in {1,2}; "same" padding: k = 1: pad 0; k = 3: pad = dilation in 1..32, exactly as conv3x3_group builds its
 * convs (padding = dilation, models/utils/layers.py:20-32; ResNet(dilations=...), resnet.py:187-233) — the dilation of
 * a 3x3 conv is read from `pad` in every tdn_*conv2d_* entry point.
 * Requires Cin % 64 == 0 and Cout % 64 == 0. */
int tdn_conv2d_fwd(const void* x, const void* w_fwd, void* y, int N, int H, int W, int Cin,
                   int Cout, int k, int stride, int pad, const tdn_epilogue* ep, int dtype,
                   void* stream);

/* dx[N][H][W][Cin] = epilogue(conv_transpose(g[N][Ho][Wo][Cout], w_dgrad)) — input gradient of
 * the conv above (autograd of nn.Conv2d; no explicit reference line: the reference never calls
 * backward). */
int tdn_conv2d_dgrad(const void* g, const void* w_dgrad, void* dx, int N, int H, int W, int Cin,
                     int Cout, int k, int stride, int pad, const tdn_epilogue* ep, int dtype,
                     void* stream);

/* Workspace bytes tdn_conv2d_wgrad needs for this shape. */
int64_t tdn_conv2d_wgrad_workspace(int N, int H, int W, int Cin, int Cout, int k, int stride,
                                    int pad);

/* Weight / affine gradients of  y = (conv(x, w)) * scale + shift  given g = dL/d(y pre-activation):
 *   dw[Cout][kh][kw][Cin] (fp32; channels_last view of the nn.Conv2d grad)  = beta*dw + scale * (g^T im2col(x))
 *   BN mode (mean, invstd != NULL): dgamma = beta*dgamma + invstd*(sum_k w*G - mean*sum_m g), dbeta = beta*dbeta + sum_m g
 *   bias mode (mean == NULL):       dbeta (= dbias) = beta*dbeta + sum_m g ; dgamma ignored (may be NULL)
 * scale may be NULL (= 1). */
int tdn_conv2d_wgrad(const void* x, const void* g, const void* w_fwd, const float* scale,
                     const float* mean, const float* invstd, float* dw, float* dgamma,
                     float* dbeta, float beta, int N, int H, int W, int Cin, int Cout, int k,
                     int stride, int pad, void* workspace, int64_t workspace_bytes, int dtype,
                     void* stream);

/* Grouped launch: the weight / affine gradients of SEVERAL convs (e.g. every conv of one ResNet stage, or of the
 * FPN) in as few launches as the tile shapes allow — autograd of the nn.Conv2d / BatchNorm2d parameters created at
 * models/backbone/resnet.py:74-91,214-216 and models/necks/fpn.py:44-58, which the reference leaves to one autograd
 * node per layer.  Members are independent; each is described like one tdn_conv2d_wgrad / tdn_stem_conv_wgrad /
 * tdn_gconv2d_wgrad call.  The library cuts every member's pixel range (the GEMM's reduction index) into splits
 * sized so that the GROUP fills the chip — a member that can be reduced by one workgroup per tile writes its
 * gradient directly (no fp32 partial slabs) — and reduces the rest, plus every member's BN / bias gradients, in ONE
 * finalize launch, in a fixed order (bit-reproducible run to run).  items / n: HOST array. */
enum { TDN_WGRAD_CONV = 0, TDN_WGRAD_STEM = 1, TDN_WGRAD_GCONV = 2 };
typedef struct tdn_wgrad_item {
  const void* x;       /* conv input, NHWC 16-bit [N][H][W][Cin]; TDN_WGRAD_STEM: the staged image xp (tdn_stage_image) */
  const void* g;       /* dL/d(pre-activation output), NHWC 16-bit [N][Ho][Wo][Cout] */
  const void* w_fwd;   /* packed forward weights (tdn_pack_conv_weight / _stem_ / _gconv_); read for dgamma */
  const float* scale;  /* BN scale or NULL (= 1) */
  const float* mean;   /* BN mean, or NULL: bias mode */
  const float* invstd; /* BN 1/sqrt(var + eps), or NULL */
  float* dw;           /* as in the single-layer call of the member's kind */
  float* dgamma;       /* may be NULL in bias mode */
  float* dbeta;        /* may be NULL */
  float beta;          /* 0: overwrite, else accumulate beta * old + new */
  int32_t kind;        /* TDN_WGRAD_* */
  int32_t N, H, W;     /* input size (STEM: the image size, even) */
  int32_t Cin, Cout;   /* GCONV: Cin = Cout = C */
  int32_t k, stride, pad;   /* ignored for STEM */
  int32_t groups;      /* GCONV only */
  int32_t reserved;
} tdn_wgrad_item;
int64_t tdn_wgrad_group_workspace(const tdn_wgrad_item* items, int n, int dtype);
int tdn_wgrad_group(const tdn_wgrad_item* items, int n, void* workspace, int64_t workspace_bytes, int dtype,
                    void* stream);
/* Host-only: the decomposition tdn_wgrad_group would use.  per_item[n][8] = {kernel (0 tap-per-tile, 1 / 2 nine-tap
 * with 128- / 64-wide tiles), tile_co, tile_ci, splits, pixels per split, direct (1: no slabs), workgroups, fp32 slab
 * bytes / 1024};
 * totals[4] = {gradient-kernel launches, finalize launches, workgroups, slab KiB}. */
int tdn_wgrad_group_plan(const tdn_wgrad_item* items, int n, int dtype, int32_t* per_item, int32_t* totals);

/* ---- operand preparation of many conv units in one launch -----------------------------------------------------
 * What tdn_bn_fold + tdn_pack_conv_weight do per layer (the eval-mode BN fold of models/utils/layers.py:50-54 as the
 * reference's default bn_eval=True makes it, resnet.py:270-276, and the 16-bit copies of nn.Conv2d.weight), for a
 * whole list of plain convolutions (groups = 1, channels multiples of 64) at once: a training step re-derives every
 * operand after the optimizer update, and 113 launches become ceil(n / 30).  Results are bit-identical to the
 * per-layer calls.  gamma == NULL: no norm (scale 1, `fold` untouched).  items / n: HOST array. */
typedef struct tdn_prep_item {
  const float* w;            /* fp32 logical [Cout][Cin][kh][kw], element strides s_o, s_i, s_h, s_w */
  void* w_fwd;               /* 16-bit [Cout][kh][kw][Cin] */
  void* w_dgrad;             /* 16-bit [Cin][kh][kw][Cout] = elem(elem(w) * scale[co]); may be NULL */
  const float* gamma;        /* BatchNorm2d weight / bias / running_mean / running_var, or all NULL */
  const float* beta;
  const float* mean;
  const float* var;
  float* fold;               /* fp32 [3][Cout]: scale, shift, invstd (written when gamma != NULL) */
  int64_t s_o, s_i, s_h, s_w;
  int32_t Cout, Cin, kh, kw;
  float eps;
  int32_t reserved;
} tdn_prep_item;
int tdn_prepare_group(const tdn_prep_item* items, int n, int dtype, void* stream);

/* ---- one residual Bottleneck per launch (models/backbone/resnet.py:97-119) ------------------
 * Stride-1 Bottleneck without a downsample branch (resnet.py:110-118), C mid channels, 4C in / out:
 *   forward   out1 = relu(bn1(conv1(in)));  out2 = relu(bn2(conv2(out1)));  out3 = relu(bn3(conv3(out2)) + in)
 *   dgrad     out1 = mask1 . conv3^T(in);   out2 = mask2 . conv2^T(out1);   out3 = mask3 . (conv1^T(out2) + in)
 *             (in = dL/d(block output before its ReLU), already masked; mask_k . v keeps v where mask_k > 0;
 *              mask1 = saved conv2 output, mask2 = saved conv1 output, mask3 = the block input, NULL = no mask)
 * in ONE launch: the intermediate tensors are handed from GEMM to GEMM through LDS (a workgroup owns 8 x 16 output
 * pixels and recomputes conv1 on the one-pixel halo) and are only WRITTEN to out1 / out2 (the weight gradients read
 * them later).  Bit-identical to the three tdn_conv2d_fwd / tdn_conv2d_dgrad launches it replaces.
 *   forward: w1 / w2 / w3 = w_fwd of conv1 / conv2 / conv3, scale_k / shift_k their folded BN (NULL = 1 / 0)
 *   dgrad:   w1 / w2 / w3 = w_dgrad of conv3 / conv2 / conv1 (BN scale folded), scale / shift unused
 * tdn_bottleneck_supported: 1 if this build has a kernel for (C, stride, dilation); callers fall back to per-conv
 * launches otherwise. */
typedef struct tdn_bottleneck_args {
  const void* in;       /* NHWC 16-bit [N][H][W][4C] */
  const void* w1;       /* [C][1][1][4C] */
  const void* w2;       /* [C][3][3][C] */
  const void* w3;       /* [4C][1][1][C] */
  const float* scale1; const float* shift1;   /* [C] */
  const float* scale2; const float* shift2;   /* [C] */
  const float* scale3; const float* shift3;   /* [4C] */
  const void* mask1;    /* [N][H][W][C] */
  const void* mask2;    /* [N][H][W][C] */
  const void* mask3;    /* [N][H][W][4C] */
  void* out1;           /* [N][H][W][C] */
  void* out2;           /* [N][H][W][C] */
  void* out3;           /* [N][H][W][4C] */
  int32_t N, H, W, C;
  /* ReLU bit planes, optional (all NULL = off): 1 bit per element, bit c % 32 of the 32-bit word c / 32 of the pixel.
   *   forward: written —  bits1 = out1 > 0, bits2 = out2 > 0, bits3 = in > 0 (any subset)
   *   dgrad:   read INSTEAD of mask1 / mask2 / mask3 (all three or none): bits2 masks out1, bits1 masks out2, bits3
   *            masks out3 — i.e. the three planes the forward call of the same block wrote.  1/16 of the mask bytes. */
  void* bits1;          /* [N][H][W][C / 32]  uint32 */
  void* bits2;          /* [N][H][W][C / 32]  uint32 */
  void* bits3;          /* [N][H][W][4C / 32] uint32 */
} tdn_bottleneck_args;
int tdn_bottleneck_supported(int H, int W, int C, int stride, int dilation);
int tdn_bottleneck_fwd(const tdn_bottleneck_args* a, int dtype, void* stream);
int tdn_bottleneck_dgrad(const tdn_bottleneck_args* a, int dtype, void* stream);

/* The stage's FIRST Bottleneck where it keeps the resolution (layer1.0: models/backbone/resnet.py:130-136 builds a
 * 1x1 conv + BN `downsample` because inplanes != planes * 4; :113-114 adds it instead of x): the block input has Cin
 * channels and the residual branch is downsample(x).  Built for Cin == C == 64, stride 1.
 *   forward:  b.in [N][H][W][Cin]; b.w1 [C][1][1][Cin]; b.out3 [N][H][W][4C] = relu(bn3(conv3(out2)) + addend) with
 *             addend [N][H][W][4C] = the downsample branch (a tdn_conv2d_fwd launch of the caller's), or computed in
 *             the launch from wd / scale_d / shift_d (see below);
 *             bits1 / bits2 optional, bits3 must be NULL
 *   dgrad:    b.in = g [N][H][W][4C]; b.w3 = conv1 w_dgrad [Cin][1][1][C]; b.out3 = dx [N][H][W][Cin] =
 *             conv1^T(out2) + addend with addend [N][H][W][Cin] = the downsample conv's input gradient; the block input
 *             comes from the max pool: no mask3 / bits3; bits1 and bits2 (both or none) replace mask2 / mask1
 * Bit-identical to the three tdn_conv2d_fwd / tdn_conv2d_dgrad launches it replaces. */
typedef struct tdn_bottleneck_head_args {
  tdn_bottleneck_args b;
  const void* addend;
  /* INSTEAD of addend: the downsample conv's own operands — forward: w_fwd [4C][1][1][Cin] and folded BN [4C]
   * (NULL = 1 / 0); dgrad: w_dgrad [Cin][1][1][4C] (scale_d / shift_d unused).  The branch is then computed inside the
   * launch (same K order, affine and 16-bit rounding as its own launch would apply: still bit-identical) and never
   * travels through HBM */
  const void* wd;
  const float* scale_d; const float* shift_d;
} tdn_bottleneck_head_args;
int tdn_bottleneck_head_supported(int H, int W, int Cin, int C, int stride, int dilation);
int tdn_bottleneck_head_fwd(const tdn_bottleneck_head_args* a, int dtype, void* stream);
int tdn_bottleneck_head_dgrad(const tdn_bottleneck_head_args* a, int dtype, void* stream);

/* ---- grouped convolution (ResNeXt) -----------------------------------
 * conv3x3_group(..., groups=cardinality) of models/backbone/resnext.py:26-28,82-83: C channels in and out,
 * `groups` groups.  Computed in block-diagonal form: every 64-channel block of the output multiplies only the same
 * 64 input channels, with zeros outside the true groups — requires C % 64 == 0 and (C / groups) | 64.
 *   tdn_pack_gconv_weight: w fp32 logical [C][C/groups][kh][kw] (element strides) ->
 *       w_fwd [C][kh][kw][64], w_dgrad [C][kh][kw][64] (BN scale folded; may be NULL)
 *   tdn_gconv2d_fwd / _dgrad: as tdn_conv2d_fwd / _dgrad (same epilogue) on those operands
 *   tdn_gconv2d_wgrad: dw fp32 [C][kh][kw][C/groups] (= channels_last bytes of the grouped parameter); dgamma / dbeta /
 *       scale / mean / invstd / beta as in tdn_conv2d_wgrad */
int tdn_pack_gconv_weight(const float* w, int64_t s_o, int64_t s_i, int64_t s_h, int64_t s_w, int C, int groups,
                          int kh, int kw, const float* scale, void* w_fwd, void* w_dgrad, int dtype, void* stream);
int tdn_gconv2d_fwd(const void* x, const void* w_fwd, void* y, int N, int H, int W, int C, int groups, int k,
                    int stride, int pad, const tdn_epilogue* ep, int dtype, void* stream);
int tdn_gconv2d_dgrad(const void* g, const void* w_dgrad, void* dx, int N, int H, int W, int C, int groups, int k,
                      int stride, int pad, const tdn_epilogue* ep, int dtype, void* stream);
int64_t tdn_gconv2d_wgrad_workspace(int N, int H, int W, int C, int groups, int k, int stride, int pad);
int tdn_gconv2d_wgrad(const void* x, const void* g, const void* w_fwd, const float* scale, const float* mean,
                      const float* invstd, float* dw, float* dgamma, float* dbeta, float beta, int N, int H, int W,
                      int C, int groups, int k, int stride, int pad, void* workspace, int64_t workspace_bytes,
                      int dtype, void* stream);

/* ---- stem (resnet.py:214-218,254-258) ------------------------------------------ */

/* NCHW image (fp32, arbitrary element strides) -> zero-padded NHWC4 bf16 staging buffer
 * xp[N][H+6][W+8][4] (3 px halo top/left/bottom, 3+2 right; channel 3 = 0).  This is the
 * device-side form of the pad/transpose of dataset_transforms.py:37-44. */
int tdn_stage_image(const float* img, int64_t s_n, int64_t s_c, int64_t s_h, int64_t s_w, int N,
                    int H, int W, void* xp, int dtype, void* stream);

/* y[N][H/2][W/2][64] = relu(bn(conv7x7 s2 p3 (img)))  from the staged image. H, W even. */
int tdn_stem_conv_fwd(const void* xp, const void* w_stem, void* y, int N, int H, int W, int Cout,
                      const tdn_epilogue* ep, int dtype, void* stream);

/* The stem in one launch: conv7x7/s2 (tdn_stem_conv_fwd) + eval-mode BN (scale, shift: tdn_bn_fold) + ReLU +
 * MaxPool2d(3, 2, 1) (tdn_maxpool3x3s2_fwd) — resnet.py:214-218, 254-258.  y[N][Ho][Wo][64] and idx (window
 * position of the first maximum) are bit-identical to the two separate calls; the stem's full-size activation is
 * never written (backward: tdn_maxpool3x3s2_relu_bwd reads the ReLU mask from y).  Cout must be 64; H, W even. */
int tdn_stem_pool_fwd(const void* xp, const void* w_stem, const float* scale, const float* shift,
                      void* y, uint8_t* idx, int N, int H, int W, int Cout, int dtype, void* stream);

int64_t tdn_stem_conv_wgrad_workspace(int N, int H, int W, int Cout);

/* dw fp32 [Cout][3][7][7] contiguous (+ BN grads as in tdn_conv2d_wgrad). */
int tdn_stem_conv_wgrad(const void* xp, const void* g, const void* w_stem, const float* scale,
                        const float* mean, const float* invstd, float* dw, float* dgamma,
                        float* dbeta, float beta, int N, int H, int W, int Cout, void* workspace,
                        int64_t workspace_bytes, int dtype, void* stream);

/* ---- pooling / resampling -------------------------------------------------------- */

/* nn.MaxPool2d(3, stride=2, padding=1) (resnet.py:218,258) on NHWC; idx[N][Ho][Wo][C] (uint8) records
 * the window position (kh*3+kw) of the first maximum, PyTorch's tie rule. C % 8 == 0. */
int tdn_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C,
                         int dtype, void* stream);

/* dx[N][H][W][C] = relu_mask(x) * scatter(dy by idx): adjoint of maxpool (and, when mask_src != NULL,
 * of the in-place ReLU before it, resnet.py:257). */
int tdn_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, const void* mask_src, void* dx, int N,
                         int H, int W, int C, int dtype, void* stream);

/* The same adjoint of ReLU -> maxpool (resnet.py:257-258) with the ReLU mask taken from the pool's OUTPUT
 * y_pooled[N][Ho][Wo][C] instead of its full-size input: a window's value is the value of the element it
 * selected, so the gradient of a window passes where y_pooled > 0.  Same dx bit for bit; reads a tensor a
 * quarter of the size, and the stem's activation need not be kept for backward. */
int tdn_maxpool3x3s2_relu_bwd(const void* dy, const uint8_t* idx, const void* y_pooled, void* dx, int N,
                              int H, int W, int C, int dtype, void* stream);

/* F.max_pool2d(x, 1, stride=2) (fpn.py:116): y[N][ceil(H/2)][ceil(W/2)][C] = x[:, ::2, ::2, :]. */
int tdn_subsample2_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype,
                       void* stream);

/* dx = dx_in (may be NULL = 0) + scatter(dy) : adjoint of the above, fused with the accumulation. */
int tdn_subsample2_bwd(const void* dy, const void* dx_in, void* dx, int N, int H, int W, int C,
                       int dtype, void* stream);

/* out = (a (+ b)) masked by mask_src > 0  (b, mask_src may be NULL). Element-wise, n elements, n % 8 == 0. */
int tdn_add_relu_mask(const void* a, const void* b, const void* mask_src, void* out, int64_t n,
                      int dtype, void* stream);

/* bf16 NHWC <-> fp32 NCHW (logical, element strides) boundary converters. */
/* ConvModule activation / pre-activation pieces (models/utils/layers.py:57-135: activation='relu6',
 * activate_last=False).  tdn_clamp_max: y = min(y, hi) in place (the upper clamp of nn.ReLU6 after a ReLU epilogue).
 * tdn_act_mask: out = g where 0 < y < hi, else 0 — the activation's backward from its saved OUTPUT y (hi = +inf:
 * ReLU, 6: ReLU6).  n % 8 == 0. */
int tdn_clamp_max(void* y, float hi, int64_t n, int dtype, void* stream);
int tdn_act_mask(const void* g, const void* y, void* out, float hi, int64_t n, int dtype, void* stream);
/* Pre-activation order (layers.py:129-134: norm -> activate -> conv): BatchNorm2d in eval mode on the conv's INPUT,
 * folded to y = act(x * scale[c] + shift[c]) (tdn_bn_fold), act 0 none / 1 ReLU / 2 ReLU6; NHWC [npix][C], C % 8 == 0.
 * Backward, from g = dL/dy already masked by the activation (tdn_act_mask): dx = g * scale[c],
 * dbeta[c] = sum g, dgamma[c] = invstd[c] * sum g * (x - mean[c]); beta != 0 accumulates into dgamma / dbeta.
 * Deterministic (per-chunk partial sums in the workspace, added in order). */
int tdn_channel_affine_fwd(const void* x, const float* scale, const float* shift, void* y, int64_t npix, int C,
                           int act, int dtype, void* stream);
int64_t tdn_channel_affine_bwd_workspace(int64_t npix, int C);
int tdn_channel_affine_bwd(const void* g, const void* x, const float* scale, const float* mean, const float* invstd,
                           void* dx, float* dgamma, float* dbeta, float beta, int64_t npix, int C, void* workspace,
                           int64_t workspace_bytes, int dtype, void* stream);

int tdn_nchw_f32_to_nhwc(const float* src, int64_t s_n, int64_t s_c, int64_t s_h, int64_t s_w,
                         int N, int C, int H, int W, void* dst, int dtype, void* stream);
/* 16-bit source (bf16 or fp16 bits, element strides of the logical NCHW tensor) -> contiguous NHWC of the same type */
int tdn_nchw16_to_nhwc(const void* src, int64_t s_n, int64_t s_c, int64_t s_h, int64_t s_w, int N, int C, int H,
                       int W, void* dst, void* stream);
int tdn_nhwc_to_nchw_f32(const void* src, int N, int C, int H, int W, float* dst, int dtype,
                         void* stream);

/* ---- prepared launch lists -----------------------------------------------------------------------------------------
 * One C call that enqueues a whole recorded step (the launches behind ResNet.forward, models/backbone/resnet.py:253-268,
 * FPN.forward, models/necks/fpn.py:88-125, and their backward) for callers that cannot capture a hipGraph.
 *   tdn_plan_begin()            start recording: every launch the library makes from now on is also kept (stream,
 *                               kernel, arguments by value); one recording at a time, process-wide
 *   tdn_plan_event_record(s)    the host recorded an event on stream s here -> plan-local event id (-1: not recording)
 *   tdn_plan_stream_wait(s, id) the host made stream s wait for that event here
 *   tdn_plan_end()              stop recording -> plan handle (NULL on error)
 *   tdn_plan_run(plan)          enqueue everything again, same streams, same order, same dependencies; no sync
 *   tdn_plan_stats(plan, out)   out[3] = {launches, event records, stream waits}; RETURNS the number of launches that were
 *                               made by OTHER threads while the plan was being recorded and were therefore NOT kept
 *                               (0 = the plan holds every launch of the recorded step; < 0: bad handle)
 *   tdn_plan_free(plan)
 * Pointers held by the recorded arguments must still refer to the same buffers when the plan runs (the host keeps the
 * recorded step's tensors alive in a private pool, like a captured graph does). */
int tdn_plan_begin(void);
void* tdn_plan_end(void);
int tdn_plan_event_record(void* stream);
int tdn_plan_stream_wait(void* stream, int event_id);
int tdn_plan_run(void* plan);
int tdn_plan_stats(void* plan, int32_t* out3);
int tdn_plan_free(void* plan);

/* ---- box ops (absent from the reference: core/__init__.py is empty; semantics = SURVEY Appendix B,
 *      conventions pinned by datasets/utils/bbox.py:39,375-377 and dataset_transforms.py:120-131) ---- */

/* anchors[(y*featW + x)*A + a][4] = base[a] + (x*stride, y*stride, x*stride, y*stride);
 * valid[...] = x < valid_w && y < valid_h (uint8, may be NULL). */
int tdn_anchor_grid(const float* base_anchors, int A, int featH, int featW, int stride,
                    int valid_h, int valid_w, float* anchors, uint8_t* valid, void* stream);

/* The whole pyramid in one launch: `nlevels` (<= 8) levels, outputs concatenated level after level — anchors fp32
 * [sum_l featH_l*featW_l*A_l][4], valid (may be NULL) one byte per anchor; inside a level exactly what tdn_anchor_grid
 * writes.  levels: HOST array; base_anchors: device pointers. */
typedef struct tdn_anchor_level {
  const float* base_anchors;   /* device, fp32 [A][4] */
  int32_t A, featH, featW, stride, valid_h, valid_w;
} tdn_anchor_level;
int tdn_anchor_pyramid(const tdn_anchor_level* levels, int nlevels, float* anchors, uint8_t* valid, void* stream);

/* iou[N][M] (fp32) of inclusive-pixel xyxy boxes, '+1' convention, IEEE fp32 (no contraction). */
int tdn_bbox_iou_pairwise(const float* a, int N, const float* b, int M, float* iou, void* stream);

int64_t tdn_nms_workspace(int N);

/* Greedy NMS: stable sort by score desc (ties: lower index first), suppress iou > thr.
 *   keep[N] uint8 (original order), kept_idx[N] int64 (score order, first *num_kept valid),
 *   num_kept: device int32. */
int tdn_nms(const float* boxes, const float* scores, int N, float iou_thr, uint8_t* keep,
            int64_t* kept_idx, int32_t* num_kept, void* workspace, int64_t workspace_bytes,
            void* stream);

/* Box delta (de)normalisation (reference: datasets/utils/bbox.py:118-166).
 *   normalize:   bbox[rows][4] <- (bbox - means) / stds, IN PLACE like `bbox.sub_(means).div_(stds)` (bbox.py:140)
 *   denormalize: out[rows][cols] = bbox * stds + means, means/stds tiled over cols = 4C (bbox.py:161-165)
 * means4 / stds4 are HOST arrays of 4 floats. Separate IEEE sub/div and mul/add: bit-identical to PyTorch-CPU. */
int tdn_bbox_normalize(float* bbox, int64_t rows, const float* means4, const float* stds4, void* stream);
int tdn_bbox_denormalize(const float* bbox, float* out, int64_t rows, int cols, const float* means4,
                         const float* stds4, void* stream);

/* ---- box delta encode / decode, segmented NMS, RPN proposals (the project's own spec in the
 *      mmdetection-v0.x lineage of SURVEY Appendix B; '+1' boxes, strict IEEE fp32 in the spec's operation order) ---- */

/* deltas[N][4] = (encode(proposals, gt) - means) / stds:  dx = (gx - px) / pw, dw = log(gw / pw), ... */
int tdn_bbox2delta(const float* proposals, const float* gt, int64_t N, const float* means4, const float* stds4,
                   float* deltas, void* stream);
/* out[N][4C] = rois[N][4] decoded by deltas[N][4C] * stds + means; dw, dh clamped to +-|log(wh_ratio_clip)| (fp32);
 * max_shape: HOST int32 (h, w) to clip x to [0, w-1] and y to [0, h-1], or NULL. */
int tdn_delta2bbox(const float* rois, const float* deltas, int64_t N, int C, const float* means4,
                   const float* stds4, const int32_t* max_shape, double wh_ratio_clip, float* out, void* stream);

/* Greedy NMS of S contiguous segments in one call: segment s = rows [seg_offsets[s], seg_offsets[s+1]) (device int64),
 * at most TDN_NMS_SEG_MAX rows; rows of different segments never suppress each other.  Order inside a segment: score
 * desc, ties lower index first; suppress iou > thr.  keep[N] uint8 (input order, 0 outside every segment),
 * kept_idx[N] int64: in each segment's row range its kept indices in score order, padded with -1; counts[S] int32
 * (device): kept per segment, -1 for a segment whose offsets are out of order / range or that is too long (its rows
 * are then left unkept).  No host synchronisation.  workspace: tdn_batched_nms_workspace(N, S) bytes, 256-aligned. */
#define TDN_NMS_SEG_MAX 4096
int64_t tdn_batched_nms_workspace(int N, int S);
int tdn_batched_nms(const float* boxes, const float* scores, int N, const int64_t* seg_offsets, int S, float iou_thr,
                    uint8_t* keep, int64_t* kept_idx, int32_t* counts, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* RPN proposals (sigmoid classification, NMS per level) of B images and `nlevels` pyramid levels in 4 launches.
 * Level l: logits (B, A, H, W) and deltas (B, 4A, H, W) in TDN_F32 or TDN_BF16, read through their element strides
 * (n, c, h, w) — NCHW, channels_last or anything else; anchors (H*W*A, 4) fp32 in (y, x, a) order, shared by all
 * images.  levels: HOST array.  img_shapes: device int32 [B][2] = (h, w).
 * Outputs (device): proposals [B][max_num][5] = x1, y1, x2, y2, sigmoid(logit), anchor_idx [B][max_num] int64 (row of
 * the concatenated pyramid), counts [B] int32; unused rows 0 / -1.  Limits: 1..8 levels, 1 <= B <= 64, every segment
 * entering NMS <= TDN_NMS_SEG_MAX boxes (nms_pre, or the level's anchors when nms_pre = 0), max_num <= 8192.
 * workspace: tdn_rpn_proposals_workspace() bytes, 256-aligned. */
enum { TDN_F32 = 2 };
#define TDN_RPN_MAX_LEVELS 8
#define TDN_RPN_MAX_NUM 8192
typedef struct tdn_rpn_level {
  const void* logits;          /* device, (B, A, H, W) */
  const void* deltas;          /* device, (B, 4A, H, W): channel 4a+j = coordinate j of anchor a */
  const float* anchors;        /* device, fp32 [H*W*A][4] */
  int64_t logit_strides[4];    /* elements: n, c, h, w */
  int64_t delta_strides[4];
  int32_t dtype;               /* TDN_F32 or TDN_BF16, both tensors */
  int32_t H, W, A;
} tdn_rpn_level;
typedef struct tdn_rpn_config {
  int32_t nms_pre;             /* > 0: top nms_pre anchors per level by logit; 0: all */
  int32_t nms_post;            /* > 0: survivors kept per level */
  int32_t max_num;             /* 1..8192: proposals per image */
  float nms_thr;
  float min_bbox_size;         /* > 0: drop boxes with x2-x1+1 or y2-y1+1 below it */
  float means[4], stds[4];     /* target_means / target_stds of the deltas */
  int32_t reserved;
} tdn_rpn_config;
int64_t tdn_rpn_proposals_workspace(const tdn_rpn_level* levels, int nlevels, int B, const tdn_rpn_config* cfg);
int tdn_rpn_proposals(const tdn_rpn_level* levels, int nlevels, int B, const int32_t* img_shapes,
                      const tdn_rpn_config* cfg, float* proposals, int64_t* anchor_idx, int32_t* counts,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- multi-level RoIAlign, the FPN RoI extractor (the project's own spec in the mmdetection-v1
 *      lineage, SingleRoIExtractor + RoIAlign with aligned=False and the '+1' end; strict IEEE fp32 in the spec's
 *      operation order) ----
 * rois: device fp32 [R][5] = (batch_idx, x1, y1, x2, y2) in input-image pixels.  A row whose (int)batch_idx is not
 * in [0, B) is invalid: zero output, no gradient (padded rows of tdn_rpn_proposals with index -1 pass straight in).
 * Level of a row: floor(log2(sqrt((x2-x1+1)*(y2-y1+1)) / finest_scale + 1e-6)) from the exponent of the fp32 value,
 * clamped to [0, nlevels-1].  Level l of B images, C channels: (B, C, H, W) 16-bit in memory addressed by the element
 * strides (n, c, h, w); the channel stride must be 1 (NHWC memory), the others multiples of 8, data 16-byte aligned.
 * Limits: 1..8 levels of one dtype, C % 8 == 0, 1 <= out_size <= 16, 0 <= sampling_ratio <= 512 (0: ceil(bin size)
 * samples per bin side, capped at 512).  No host synchronisation, no allocation, no float atomics. */
#define TDN_ROI_MAX_LEVELS 8
#define TDN_ROI_MAX_OUT 16
#define TDN_ROI_MAX_SAMPLES 512
typedef struct tdn_roi_level {
  void* data;                  /* device: features (fwd, read) or their gradient (bwd, written in full) */
  int64_t strides[4];          /* elements: n, c, h, w (c must be 1) */
  int32_t H, W;
  int32_t dtype;               /* TDN_BF16 or TDN_F16, the same on every level */
  int32_t reserved;
} tdn_roi_level;
typedef struct tdn_roi_config {
  int32_t out_size;            /* S: output bins per side */
  int32_t sampling_ratio;      /* > 0: samples per bin side; 0: adaptive */
  float finest_scale;          /* > 0 (mmdetection: 56) */
  int32_t reserved;
  float scales[TDN_ROI_MAX_LEVELS];   /* spatial_scale of level l = 1 / featmap_stride_l (fp32), > 0 */
} tdn_roi_config;
/* levels[R] int64 = the level of every row (batch index ignored), as above. */
int tdn_roi_map_levels(const float* rois, int64_t R, int nlevels, float finest_scale, int64_t* levels, void* stream);
/* out: device 16-bit (R, S, S, C) contiguous (channels_last (R, C, S, S)); one launch. */
int tdn_roi_align_fwd(const tdn_roi_level* feats, int nlevels, int B, int C, const float* rois, int64_t R,
                      const tdn_roi_config* cfg, void* out, void* stream);
/* dout: device 16-bit (R, S, S, C) contiguous.  grads[l].data: every element of every level is written (pixels no
 * valid row touches get 0), fp32 sums rounded once; bitwise reproducible.  Two launches (per-row geometry, then one
 * workgroup per 4x16-pixel tile x 256 channels summing its rows in row order).  workspace:
 * tdn_roi_align_bwd_workspace(R) bytes, 256-aligned. */
int64_t tdn_roi_align_bwd_workspace(int64_t R);
int tdn_roi_align_bwd(const tdn_roi_level* grads, int nlevels, int B, int C, const float* rois, int64_t R,
                      const tdn_roi_config* cfg, const void* dout, void* workspace, int64_t workspace_bytes,
                      void* stream);
/* rois[B*M][5] from tdn_rpn_proposals' proposals[B][M][5]: row b*M+m = (b, x1, y1, x2, y2) when m < counts[b], else
 * (-1, x1, y1, x2, y2) — an invalid row for tdn_roi_align_*.  No host synchronisation. */
int tdn_rois_from_proposals(const float* proposals, const int32_t* counts, int B, int M, float* rois, void* stream);

/* ---- training targets: max-IoU assignment, random sampling, RPN and RoI-head targets (the project's
 *      own spec in the mmdetection-v0.x/v1 lineage of MaxIoUAssigner / RandomSampler / anchor_target / bbox_target;
 *      IoU is tdn_bbox_iou_pairwise's value bit for bit, encode is tdn_bbox2delta's arithmetic) ----
 * Common to all four: B images (1..64), boxes fp32 xyxy '+1'; box_stride = floats between the boxes of consecutive
 * images (0: one set of N boxes shared by all images, else >= 4N); gt: device fp32 [B][G][4], rows at or beyond
 * gt_counts[b] (device int32 [B], clamped to 0..G) are padding and never read; G <= TDN_TARGET_MAX_GT,
 * N <= TDN_TARGET_MAX_BOXES, num <= TDN_TARGET_MAX_NUM.  The (N, G) IoU matrix is never stored: pass 1 keeps the row
 * maximum / argmax per box and merges the per-ground-truth column maxima with integer atomicMax on the IoU's bit
 * pattern, pass 2 recomputes the IoUs against them.  No float atomics, no host synchronisation, no allocation; the
 * first launch of a call clears what the call's workspace needs cleared.  Workspaces: the *_workspace_bytes() query of
 * the entry point, 256-aligned. */
#define TDN_TARGET_MAX_GT 256
#define TDN_TARGET_MAX_BOXES (1 << 20)
#define TDN_TARGET_MAX_NUM 8192
typedef struct tdn_target_config {
  float pos_iou_thr, neg_iou_thr, min_pos_iou;   /* compared in fp32 */
  int32_t gt_max_assign_all;   /* step 6: 1 = every box attaining a ground truth's maximum, 0 = the lowest such box */
  int32_t num;                 /* samples per image, 0..TDN_TARGET_MAX_NUM */
  int32_t num_pos_expected;    /* int(num * pos_fraction), evaluated by the caller in double; 0..num */
  int32_t allowed_border;      /* tdn_anchor_target: >= 0 drops anchors leaving the image by more than this; < 0: off */
  int32_t add_gt_as_proposals; /* tdn_sample_rois */
  double neg_pos_ub;           /* >= 0: negatives <= int(neg_pos_ub * max(1, positives)); < 0: no bound */
  float means[4], stds[4];     /* target_means / target_stds of the deltas */
  uint32_t seed;               /* of the generated keys (keys == NULL) */
  int32_t reserved;
} tdn_target_config;
/* assigned[B][N] int32: -1 ignored / not taking part, 0 negative, j+1 ground truth j; max_overlaps[B][N] fp32 (0 for a
 * box that does not take part, may be NULL).  valid: uint8 [N] shared by all images (valid_stride 0) or [B][N]
 * (valid_stride N) whatever box_stride is, or NULL.  Three launches (four with gt_max_assign_all = 0). */
int64_t tdn_assign_max_iou_workspace_bytes(int B, int G);
int tdn_assign_max_iou(const float* boxes, int64_t box_stride, const uint8_t* valid, int64_t valid_stride, const float* gt,
                       const int32_t* gt_counts, int B, int N, int G, const tdn_target_config* cfg, int32_t* assigned,
                       float* max_overlaps, void* workspace, int64_t workspace_bytes, void* stream);
/* The pos / neg smallest (key, index) among assigned > 0 / == 0 of every image: pos = min(#positives,
 * num_pos_expected), neg = min(#negatives, num - pos [, neg_pos_ub bound]).  keys: device int32 [B][N], non-negative, or
 * NULL for key = tdn_target_key(seed, b, i).  pos_mask / neg_mask uint8 [B][N], num_pos / num_neg int32
 * [B].  One launch, two workgroups per image; no workspace. */
int tdn_sample_assigned(const int32_t* assigned, int B, int N, const tdn_target_config* cfg, const int32_t* keys,
                        uint8_t* pos_mask, uint8_t* neg_mask, int32_t* num_pos, int32_t* num_neg, void* stream);
/* RPN targets: assignment (valid flags [N] or [B][N] or NULL, and allowed_border against img_shapes int32 [B][2] =
 * (h, w)), sampling, encode.  labels int64 [B][N] (1 on sampled positives), label_weights fp32 [B][N] (1 on sampled
 * positives and negatives), bbox_targets / bbox_weights fp32 [B][N][4], num_pos / num_neg int32 [B], assigned int32
 * [B][N].  Five launches (six with gt_max_assign_all = 0). */
int64_t tdn_anchor_target_workspace_bytes(int B, int N, int G);
int tdn_anchor_target(const float* anchors, int64_t box_stride, const uint8_t* valid, int64_t valid_stride, const float* gt,
                      const int32_t* gt_counts, const int32_t* img_shapes, int B, int N, int G,
                      const tdn_target_config* cfg, const int32_t* keys, int64_t* labels, float* label_weights,
                      float* bbox_targets, float* bbox_weights, int32_t* num_pos, int32_t* num_neg, int32_t* assigned,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* RoI-head targets from tdn_rpn_proposals' padded output: proposals [B][P][5], counts [B].  Candidates of image b: its
 * gt_counts[b] ground truths first (add_gt_as_proposals), then its counts[b] proposals; keys int32 [B][G + P] (or
 * [B][P] without the ground truths) or NULL.  Image b owns rows [b*num, (b+1)*num): sampled positives in ascending
 * candidate index, then sampled negatives likewise, then padding (batch index -1, zeros, weight 0, gt index -1).
 * rois fp32 [B*num][5] = (b, x1, y1, x2, y2), labels int64 (gt_labels[b][assigned-1] on positives, gt_labels int64
 * [B][G]), label_weights fp32, bbox_targets / bbox_weights fp32 [B*num][4], pos_gt_inds int32 [B*num].  Five launches
 * (six with gt_max_assign_all = 0). */
int64_t tdn_sample_rois_workspace_bytes(int B, int P, int G, int add_gt_as_proposals);
int tdn_sample_rois(const float* proposals, const int32_t* counts, const float* gt, const int64_t* gt_labels,
                    const int32_t* gt_counts, int B, int P, int G, const tdn_target_config* cfg, const int32_t* keys,
                    float* rois, int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights,
                    int32_t* pos_gt_inds, int32_t* num_pos, int32_t* num_neg, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* IoU-balanced negative sampling (Libra R-CNN): tdn_sample_assigned and tdn_sample_rois with ONLY the
 * choice of negatives replaced; assignment, positives, row layout, labels, targets, weights and the launch counts are
 * theirs.  "Choose k of a set at random" is "the k smallest (key, index) of the set" with tdn_sample_assigned's keys.
 * Per image, o_i = max_overlaps of candidate i, n = the number of negatives tdn_sample_assigned would take at most:
 *   at most n negatives: all of them.  Else among the negatives F = {o < floor_thr}, S = {o >= floor_thr}, t0 = floor_thr
 *   (floor_thr > 0); F = {o == 0}, S = {o > 0}, t0 = 0 (floor_thr == 0); F empty, S all, t0 = 0 (floor_thr < 0).
 *   n_S = (int)((double)n * (1.0 - (double)floor_fraction)).  |S| <= n_S: all of S.  Else, num_bins >= 2: m = the maximum
 *   of o over ALL candidates of the image, w = (m - t0) / num_bins, per = n_S / num_bins (integers); from each bin
 *   {i in S: t0 + k w <= o_i < t0 + (k + 1) w} (fp32, product and sum rounded separately), k = 0 .. num_bins - 1, its
 *   per smallest (all if it has no more); then the n_S - taken smallest of the rest of S.  num_bins == 1: the n_S smallest
 *   of S.  Then from F the n - taken smallest (all if it has no more), then from the remaining negatives up to n.
 * num_bins 1..8, floor_fraction in [0, 1], floor_thr < 1.  max_overlaps fp32 [B][N] as tdn_assign_max_iou writes it. */
typedef struct tdn_balanced_config {
  float floor_thr;
  float floor_fraction;
  int32_t num_bins;
  int32_t reserved;
} tdn_balanced_config;
int tdn_sample_assigned_balanced(const int32_t* assigned, const float* max_overlaps, int B, int N,
                                 const tdn_target_config* cfg, const tdn_balanced_config* bal, const int32_t* keys,
                                 uint8_t* pos_mask, uint8_t* neg_mask, int32_t* num_pos, int32_t* num_neg, void* stream);
int64_t tdn_sample_rois_balanced_workspace_bytes(int B, int P, int G, int add_gt_as_proposals);
int tdn_sample_rois_balanced(const float* proposals, const int32_t* counts, const float* gt, const int64_t* gt_labels,
                             const int32_t* gt_counts, int B, int P, int G, const tdn_target_config* cfg,
                             const tdn_balanced_config* bal, const int32_t* keys, float* rois, int64_t* labels,
                             float* label_weights, float* bbox_targets, float* bbox_weights, int32_t* pos_gt_inds,
                             int32_t* num_pos, int32_t* num_neg, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- losses of the dense anchor heads (RPN, RetinaNet) and of the RoI box head, with their gradients (DESIGN.md §4e:
 *      sigmoid BCE / focal + smooth L1 over the level-major anchors of tdn_anchor_target; softmax CE + smooth L1 over
 *      the rows of tdn_sample_rois) ----
 * Head outputs are TDN_F32 / TDN_BF16 / TDN_F16, read in place; targets are the fp32 / int64 tensors the target entry
 * points write.  Per-element work is fp32, sums are fp64 in an order fixed by the shapes (no float atomics: block
 * partials in the workspace, added in index order by the last launch).  An element whose weight is exactly 0 is never
 * evaluated: loss 0, gradient 0, whatever its logit.  The divisor is read on the device (tdn_loss_avg), so nothing
 * synchronises with the host.  losses fp32 [2] = (loss_cls, loss_bbox); avg_out fp32 [1] = the divisor, which the
 * backward entry points take back as avg_in together with the cotangent g fp32 [2].  Forward: two launches; backward:
 * one.  Workspaces: the *_workspace_bytes() query, 256-aligned. */
#define TDN_LOSS_MAX_LEVELS 8
#define TDN_LOSS_MAX_CLASSES 1024
#define TDN_LOSS_MAX_ROWS (1 << 20)     /* anchors per image / RoI rows */
#define TDN_LOSS_MAX_AVG 64             /* elements per avg_factor tensor */
typedef struct tdn_loss_level {
  const void* cls;            /* (B, A*C, H, W) logits: class channel a*C + c */
  const void* reg;            /* (B, 4A, H, W) deltas: box channel 4a + j */
  void* dcls;                 /* backward only: gradients, laid out as cls / reg */
  void* dreg;
  int32_t H, W;
  int32_t cls_nhwc, reg_nhwc; /* 0: NCHW-contiguous memory, 1: channels_last (N, H, W, C) memory */
} tdn_loss_level;
typedef struct tdn_loss_config {
  int32_t dtype;              /* TDN_BF16 / TDN_F16 / TDN_F32, of every head output and gradient */
  int32_t num_anchors;        /* A */
  int32_t num_classes;        /* C: label k in 1..C is one-hot on class channel k-1, 0 is background */
  int32_t focal;              /* 0: binary cross entropy, 1: focal with gamma, alpha */
  float beta;                 /* smooth L1 knee, > 0 */
  float gamma, alpha;
  int32_t reserved;
} tdn_loss_config;
typedef struct tdn_loss_avg {
  const int32_t* a;           /* mode 1: divisor = max(1, sum a[0..na) + sum b[0..nb)) as fp32, summed on the device */
  const int32_t* b;
  int32_t na, nb;             /* 0..TDN_LOSS_MAX_AVG each */
  int32_t mode;               /* 0: value; 1: the tensors; 2 (RoI head only): rows with label_weights > 0, at least 1 */
  float value;                /* mode 0: finite and > 0 */
} tdn_loss_avg;
/* labels int64 [B][N], label_weights fp32 [B][N], bbox_targets / bbox_weights fp32 [B][N][4], N = sum H*W*A over the
 * levels in order, anchor (h*W + w)*A + a within a level; one level tensor holds fewer than 2^31 elements. */
int64_t tdn_loss_dense_workspace_bytes(const tdn_loss_level* levels, int num_levels, int B, const tdn_loss_config* cfg);
int tdn_loss_dense_fwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_loss_config* cfg,
                       const int64_t* labels, const float* label_weights, const float* bbox_targets,
                       const float* bbox_weights, const tdn_loss_avg* avg, float* losses, float* avg_out,
                       void* workspace, int64_t workspace_bytes, void* stream);
int tdn_loss_dense_bwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_loss_config* cfg,
                       const int64_t* labels, const float* label_weights, const float* bbox_targets,
                       const float* bbox_weights, const float* g, const float* avg_in, void* stream);
/* cls [R][C] softmax logits (class 0 background), reg [R][reg_cols], reg_cols = 4C (row r regresses columns
 * 4*labels[r] ..) or 4; labels int64 [R], label_weights fp32 [R], bbox_targets / bbox_weights fp32 [R][4].  A row whose
 * label is outside [0, C) counts as weight 0. */
int64_t tdn_loss_roi_workspace_bytes(int R);
int tdn_loss_roi_fwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols, const int64_t* labels,
                     const float* label_weights, const float* bbox_targets, const float* bbox_weights, float beta,
                     const tdn_loss_avg* avg, float* losses, float* avg_out, void* workspace, int64_t workspace_bytes,
                     void* stream);
int tdn_loss_roi_bwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols, const int64_t* labels,
                     const float* label_weights, const float* bbox_targets, const float* bbox_weights, float beta,
                     const float* g, const float* avg_in, void* dcls, void* dreg, void* stream);
/* The same two entry points with balanced L1 (Libra R-CNN) in place of smooth L1 as the box term; the
 * classification term, the divisor, the weight-0 rule, the column rule, the reduction and the workspace
 * (tdn_loss_roi_workspace_bytes) are the same.  Per element, fp32, in the order written, d = pred - target, a = |d|:
 *   a <  beta:  t = log1pf((b a) / beta);  l = ((alpha / b) (b a + 1)) t - alpha a;
 *               dl = sign(d) (alpha t + (alpha (1 - beta)) / (b a + beta))      (the second term is +0 at beta = 1)
 *   a >= beta:  l = gamma a + (gamma / b - alpha beta);                              dl = sign(d) gamma
 * b = e^(gamma / alpha) - 1, alpha / b, gamma / b - alpha beta and alpha (1 - beta) are formed on the host in double and
 * rounded once to fp32.  alpha, gamma finite and > 0, b finite in fp32; beta is the knee.  a = 0: loss 0 and gradient 0
 * exactly. */
int tdn_loss_roi_balanced_fwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols,
                              const int64_t* labels, const float* label_weights, const float* bbox_targets,
                              const float* bbox_weights, float beta, float alpha, float gamma, const tdn_loss_avg* avg,
                              float* losses, float* avg_out, void* workspace, int64_t workspace_bytes, void* stream);
int tdn_loss_roi_balanced_bwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols,
                              const int64_t* labels, const float* label_weights, const float* bbox_targets,
                              const float* bbox_weights, float beta, float alpha, float gamma, const float* g,
                              const float* avg_in, void* dcls, void* dreg, void* stream);

/* ---- test-time detections of the RoI box head: softmax + decode, per-class NMS, per-image top-k (the
 *      project's own spec in the mmdetection-v0.x lineage of multiclass_nms / get_det_bboxes; NMS is tdn_batched_nms's
 *      arithmetic, decode is tdn_delta2bbox's, the softmax row is tdn_loss_roi_fwd's) ----
 * scores fp32 [N][C], column 0 background; boxes fp32 [N][box_cols], box_cols = 4 (C - 1) (class c reads columns
 * 4 (c - 1) ..) or 4 (class-agnostic).  batch_idx: device int32 (batch_idx_bytes 4) or int64 (8) [N], or NULL for one
 * image (B = 1); a row whose index is outside [0, B) takes no part.  Candidates of (image b, class c >= 1): the image's
 * rows with score > score_thr; per segment greedy NMS (score desc, row asc; iou > nms_thr) as tdn_batched_nms; per image
 * the best min(max_num, survivors) by (score desc, class asc, row asc), always in that order.
 * Outputs (device): dets fp32 [B][max_num][5] = x1, y1, x2, y2, score; labels int64 [B][max_num] = c - 1; row_idx int64
 * [B][max_num] = the source row; counts int32 [B]; unused rows 0 / -1 / -1.  An image with a segment of more than
 * TDN_NMS_SEG_MAX candidates gets counts[b] = -1 and empty rows.  NaN scores are unsupported.
 * Limits: 1 <= B <= 64, 2 <= C <= TDN_DET_MAX_CLASSES, N <= TDN_DET_MAX_ROWS, 1 <= max_num <= TDN_RPN_MAX_NUM, finite
 * thresholds, B (C - 1) min(N, TDN_NMS_SEG_MAX) < 2^31.  Four launches; no host synchronisation, no memset, no float
 * atomics.  workspace: tdn_multiclass_nms_workspace_bytes() bytes, 256-aligned.  Soft-NMS in place of the greedy NMS:
 * the _soft entry points further down. */
#define TDN_DET_MAX_CLASSES 1024
#define TDN_DET_MAX_ROWS (1 << 18)
int64_t tdn_multiclass_nms_workspace_bytes(int N, int C, int B);
int tdn_multiclass_nms(const float* boxes, int box_cols, const float* scores, const void* batch_idx, int batch_idx_bytes,
                       int N, int C, int B, float score_thr, float nms_thr, int max_num, float* dets, int64_t* labels,
                       int64_t* row_idx, int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
/* The box head's outputs to detections in five launches.  rois fp32 [R][5] = (batch_idx, x1, y1, x2, y2) as
 * tdn_roi_align_fwd takes them (a row whose (int)batch_idx is not in [0, B) takes no part); cls [R][C] softmax logits,
 * reg [R][reg_cols], reg_cols = 4C (class c reads columns 4c ..) or 4, both TDN_F32 / TDN_BF16 / TDN_F16; img_shapes
 * device int32 [B][2] = (h, w): the decode's clip; scale_factors device fp32 [B] or NULL, then scale_factor (0: none):
 * every clipped coordinate is divided by its image's factor.  dense_scores fp32 [R][C] and dense_boxes fp32
 * [R][4 (C - 1)] (or [R][4]) are written by the first launch (rows that take no part: 0) and are what the selection
 * reads: tdn_multiclass_nms on them with batch_idx = the rois' first column gives the same outputs bit for bit.
 * workspace: tdn_bbox_detections_workspace_bytes() bytes, 256-aligned. */
int64_t tdn_bbox_detections_workspace_bytes(int R, int C, int B);
int tdn_bbox_detections(const float* rois, const void* cls, const void* reg, int dtype, int R, int C, int reg_cols, int B,
                        const int32_t* img_shapes, const float* scale_factors, float scale_factor, const float* means4,
                        const float* stds4, double wh_ratio_clip, float score_thr, float nms_thr, int max_num,
                        float* dense_scores, float* dense_boxes, float* dets, int64_t* labels, int64_t* row_idx,
                        int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Cascade R-CNN: box refinement between the stages and detections from the stages' averaged scores (DESIGN.md
 *      §4q: mmdetection v1's BBoxHead.refine_bboxes / regress_by_class and CascadeRCNN.simple_test; decode is
 *      tdn_delta2bbox's arithmetic, everything after the averaged logit is tdn_bbox_detections itself) ----
 * tdn_cascade_detections: tdn_bbox_detections with cls a HOST array of num_stages = 1..TDN_CASCADE_MAX_STAGES device
 * matrices [R][C] of one dtype; the logit of (r, c) is (((x_0 + x_1) + ...) + x_{S-1}) / (float)S, fp32 additions in
 * stage order and one fp32 division; reg is the last stage's.  Same five launches, outputs, limits and workspace
 * (tdn_bbox_detections_workspace_bytes) as tdn_bbox_detections; with one stage the outputs are its outputs bit for bit. */
#define TDN_CASCADE_MAX_STAGES 8
int tdn_cascade_detections(const float* rois, const void* const* cls, int num_stages, const void* reg, int dtype, int R,
                           int C, int reg_cols, int B, const int32_t* img_shapes, const float* scale_factors,
                           float scale_factor, const float* means4, const float* stds4, double wh_ratio_clip,
                           float score_thr, float nms_thr, int max_num, float* dense_scores, float* dense_boxes,
                           float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* tdn_refine_bboxes: rois fp32 [R][5] = (batch_idx, x1, y1, x2, y2) (a row whose (int)batch_idx is not in [0, B) is
 * padding); bbox_pred [R][reg_cols] of dtype TDN_F32 / TDN_BF16 / TDN_F16, reg_cols = 4C (row r reads columns
 * 4*label .., label 0 the background's, as regress_by_class does) or 4.  Exactly one of labels (int64 [R], as
 * tdn_sample_rois writes them) and cls_score ([R][C] of dtype: the label is the arg-max over all C columns, ties to the
 * lowest column, as cls_score.argmax(dim=1)) is non-NULL; with reg_cols = 4C a given label outside [0, C) makes the row
 * padding.  The new box is tdn_delta2bbox's decode of the row against img_shapes[b] (int32 [B][2] = (h, w)).
 *   max_per_img = 0, row-aligned (test time): rois_out fp32 [R][5], row r = (b, box) of input row r, padding rows
 *     (-1, 0, 0, 0, 0).  One launch, no workspace.
 *   max_per_img = P in 1..TDN_RPN_MAX_NUM, compacted (training): proposals fp32 [B][P][5] = (x1, y1, x2, y2, 0) and
 *     counts int32 [B], the form tdn_sample_rois reads: image b's kept rows in ascending input row, the first P of them,
 *     counts[b] = min(kept, P), rows past it 0.  Padding rows are dropped, and with pos_gt_inds (int32 [R]) and
 *     gt_bboxes (fp32 [B][G][4]) also every row with 0 <= pos_gt_inds[r] < G whose four coordinates are bitwise those
 *     of gt_bboxes[b][pos_gt_inds[r]] (refine_bboxes' pos_is_gt).  Two launches; workspace: TDN_REFINE_WS_BYTES(R, B)
 *     bytes, 256-aligned (none for R = 0).
 * Limits: 1 <= B <= 64, R <= TDN_DET_MAX_ROWS, 1 <= C <= TDN_DET_MAX_CLASSES.  No host synchronisation, no memset, no
 * float atomics; NaN logits are unsupported. */
#define TDN_REFINE_CHUNK 1024           /* rows per workgroup */
#define TDN_REFINE_WS_BYTES(R, B) \
  (((((int64_t)(R) + TDN_REFINE_CHUNK - 1) / TDN_REFINE_CHUNK) * (int64_t)(B) * 4 + 255) & ~(int64_t)255)
int tdn_refine_bboxes(const float* rois, const void* bbox_pred, int dtype, int R, int reg_cols, int B,
                      const int32_t* img_shapes, const int64_t* labels, const void* cls_score, int C,
                      const int32_t* pos_gt_inds, const float* gt_bboxes, int G, const float* means4,
                      const float* stds4, double wh_ratio_clip, int max_per_img, float* rois_out, float* proposals,
                      int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- single-stage (RetinaNet-style) dense anchor heads: test-time detections from sigmoid class logits, and unsampled
 *      class-labelled anchor targets (the project's own spec in the mmdetection-v1 lineage of
 *      AnchorHead.get_bboxes / anchor_target with sampling off; decode is tdn_delta2bbox's arithmetic, the sigmoid is
 *      tdn_rpn_proposals', the selection is tdn_multiclass_nms itself, the assignment is tdn_anchor_target's) ----
 * Level l of B images: cls (B, A*C, H, W) logits, class channel a*C + c, and reg (B, 4A, H, W) deltas, box channel
 * 4a + j, both of cfg->dtype (TDN_F32 / TDN_BF16 / TDN_F16), read in place through their element strides (n, c, h, w);
 * anchors fp32 [H*W*A][4] in (y, x, a) order.  levels: HOST array.  The key of anchor i = (h*W + w)*A + a of (image,
 * level) is the maximum of its C logits (-0 == +0; NaN unsupported).  A level of n_l > nms_pre > 0 anchors keeps the
 * nms_pre first by (key desc, anchor asc), any other level all n_l; k_l kept, K = sum k_l, off_l their prefix sum.
 * (image b, level l) owns dense rows [b*K + off_l, b*K + off_l + k_l), its kept anchors there in ascending anchor order:
 * dense_scores fp32 [B*K][C+1] (column 0 = 0, column 1+c = 1 / (1 + expf(-x))), dense_boxes fp32 [B*K][4] (the decode
 * clipped to img_shapes[b] = (h, w), device int32 [B][2]; then divided by scale_factors[b] (device fp32 [B]) or, when
 * that is NULL, by cfg->scale_factor (0: none)), batch_idx int32 [B*K], dense_anchor_idx int64 [B*K] (row of the
 * concatenated pyramid).  Then tdn_multiclass_nms on those four, class-agnostic boxes: dets, labels, row_idx, counts as
 * there, and anchor_idx int64 [B][max_num] = dense_anchor_idx[row_idx], -1 on unused rows.
 * Limits: 1..TDN_DENSE_MAX_LEVELS levels, 1 <= B <= 64, 1 <= C <= TDN_DET_MAX_CLASSES - 1, A >= 1, 0 <= nms_pre <=
 * TDN_NMS_SEG_MAX, B*K <= TDN_DET_MAX_ROWS, B*A*C*H*W < 2^31 per level, and tdn_multiclass_nms's.
 * Launches, whatever B, the number of levels and C: 1 class maximum of every anchor of the levels that select (grid
 * grows with the anchors; none if no level selects), 1 per (image, level) threshold, ordered compaction, sigmoid and
 * decode, tdn_multiclass_nms's 4, 1 anchor_idx gather: 7 (6).  No host synchronisation, no allocation, no memset, no
 * float atomics.  tdn_dense_detections_plan is host-only: out16 = {K, B*K, anchors per image, launches, workgroups of
 * the class-maximum launch, levels that select, key words of the workspace, 0, k_0 .. k_7}.
 * workspace: tdn_dense_detections_workspace_bytes() bytes, 256-aligned. */
#define TDN_DENSE_MAX_LEVELS 8
typedef struct tdn_dense_level {
  const void* cls;             /* device, (B, A*C, H, W) */
  const void* reg;             /* device, (B, 4A, H, W) */
  const float* anchors;        /* device, fp32 [H*W*A][4] */
  int64_t cls_strides[4];      /* elements: n, c, h, w */
  int64_t reg_strides[4];
  int32_t H, W;
} tdn_dense_level;
typedef struct tdn_dense_config {
  double wh_ratio_clip;        /* in (0, 1) */
  int32_t dtype;               /* TDN_F32 / TDN_BF16 / TDN_F16, every head output */
  int32_t num_anchors;         /* A */
  int32_t num_classes;         /* C */
  int32_t nms_pre;             /* > 0: anchors kept per level; 0: all */
  int32_t max_num;             /* 1..TDN_RPN_MAX_NUM detections per image */
  float score_thr, nms_thr;
  float scale_factor;          /* used when scale_factors == NULL; 0: no rescale */
  float means[4], stds[4];     /* target_means / target_stds of the deltas */
} tdn_dense_config;
int tdn_dense_detections_plan(const tdn_dense_level* levels, int nlevels, int B, const tdn_dense_config* cfg,
                              int32_t* out16);
int64_t tdn_dense_detections_workspace_bytes(const tdn_dense_level* levels, int nlevels, int B,
                                             const tdn_dense_config* cfg);
int tdn_dense_detections(const tdn_dense_level* levels, int nlevels, int B, const int32_t* img_shapes,
                         const float* scale_factors, const tdn_dense_config* cfg, float* dense_scores,
                         float* dense_boxes, int32_t* batch_idx, int64_t* dense_anchor_idx, float* dets,
                         int64_t* labels, int64_t* row_idx, int64_t* anchor_idx, int32_t* counts, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* Unsampled anchor targets: tdn_anchor_target's assignment (valid flags, allowed_border, the six steps), then every
 * anchor is used.  labels int64 [B][N] = gt_labels[b][assigned - 1] where assigned > 0 (gt_labels int64 [B][G]; NULL:
 * 1), else 0; label_weights fp32 [B][N] = 1 where assigned >= 0; bbox_targets / bbox_weights fp32 [B][N][4] = the
 * encode / 1 where assigned > 0, else 0; num_pos / num_neg int32 [B] = anchors with assigned > 0 / == 0; assigned int32
 * [B][N].  N >= 1.  cfg: the thresholds, gt_max_assign_all, allowed_border, means, stds; the sampling fields are not
 * read.  The assignment's three launches (four with gt_max_assign_all = 0) plus one that writes every output element
 * and, from one integer atomic add per workgroup on a word the first launch cleared, the counts. */
int64_t tdn_anchor_target_all_workspace_bytes(int B, int N, int G);
int tdn_anchor_target_all(const float* anchors, int64_t box_stride, const uint8_t* valid, int64_t valid_stride,
                          const float* gt, const int64_t* gt_labels, const int32_t* gt_counts,
                          const int32_t* img_shapes, int B, int N, int G, const tdn_target_config* cfg, int64_t* labels,
                          float* label_weights, float* bbox_targets, float* bbox_weights, int32_t* num_pos,
                          int32_t* num_neg, int32_t* assigned, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- FCOS: points, point targets, focal + IoU + centre-ness loss, detections (the project's own spec in
 *      the mmdetection-v1 lineage of FCOSHead; '+1' boxes, strict fp32 in the spec's operation order) ----
 * The pyramid has L levels (HOST array) of H x W points and an integer stride s; point i = h*W + w of a level sits at
 * (x, y) = (w*s + s/2, h*s + s/2) (integer division, exact in fp32: W*s, H*s < 2^24), points are level-major,
 * N = sum H*W <= TDN_TARGET_MAX_BOXES.  Head outputs (loss, detections): cls (B, C, H, W), reg (B, 4, H, W), ctr
 * (B, 1, H, W) of one dtype (TDN_F32 / TDN_BF16 / TDN_F16), each NCHW-contiguous (nhwc flag 0) or channels_last (1)
 * memory, read in place; one level tensor holds fewer than 2^31 elements.  scales: device fp32 [L] or NULL (all 1): the
 * distance of a point in direction j is expf(scales[l] * reg_j), one fp32 product. */
#define TDN_FCOS_MAX_LEVELS 8
typedef struct tdn_fcos_level {
  const void* cls;             /* device; loss and detections only */
  const void* reg;
  const void* ctr;
  void* dcls;                  /* backward only: gradients, laid out as cls / reg / ctr */
  void* dreg;
  void* dctr;
  int32_t H, W;
  int32_t stride;              /* 1..2^15 */
  int32_t cls_nhwc, reg_nhwc;  /* 0: NCHW-contiguous memory, 1: channels_last memory */
  int32_t reserved;
  float lo, hi;                /* targets only: the level's regress range, lo <= hi, hi may be +inf */
} tdn_fcos_level;
/* points fp32 [N][4] = (x, y, stride, level).  One launch. */
int tdn_fcos_points(const tdn_fcos_level* levels, int nlevels, float* points, void* stream);
/* Point targets.  gt fp32 [B][G][4] xyxy, gt_labels int64 [B][G] (NULL: 1), gt_counts int32 [B] (clamped to 0..G),
 * G <= TDN_TARGET_MAX_GT.  For point (x, y) of level l and ground truth j < gt_counts[b], ascending j:
 * l = x - x1, t = y - y1, r = x2 - x, b = y2 - y; inside: min(l, t, r, b) > 0, or with radius > 0 the same test against
 * (max(cx - radius*s, x1), max(cy - radius*s, y1), min(cx + radius*s, x2), min(cy + radius*s, y2)), cx = (x1 + x2)*0.5,
 * cy = (y1 + y2)*0.5; range: lo <= max(l, t, r, b) <= hi; the smallest area (x2 - x1 + 1)*(y2 - y1 + 1) among those that
 * pass both wins, ties to the lowest j.  labels int64 [B][N] (0: none), bbox_targets fp32 [B][N][4] = the winner's
 * (l, t, r, b) or 0, assigned int32 [B][N] = j + 1 or 0, num_pos int32 [B].  radius 0: no centre sampling.  Two launches
 * (targets with one integer count per workgroup; the counts' sum): no atomics at all. */
int64_t tdn_fcos_target_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B, int G);
int tdn_fcos_target(const tdn_fcos_level* levels, int nlevels, int B, const float* gt, const int64_t* gt_labels,
                    const int32_t* gt_counts, int G, float radius, int64_t* labels, float* bbox_targets,
                    int32_t* assigned, int32_t* num_pos, void* workspace, int64_t workspace_bytes, void* stream);
/* The FCOS loss over all B*N points.  labels int64 [B][N] (0: background, k in 1..C: class channel k-1; > 0: positive),
 * bbox_targets fp32 [B][N][4] = (l*, t*, r*, b*) as tdn_fcos_target writes them.
 *   loss_cls: the focal term of tdn_loss_dense_fwd (A = 1, every weight 1), sum / (positives + B).
 *   positives only, d_j = expf(scale_l * reg_j):  c* = sqrtf((min(l*,r*)/max(l*,r*)) * (min(t*,b*)/max(t*,b*)));
 *     areas (l+r+1)*(t+b+1), intersection (min(l,l*)+min(r,r*)+1)*(min(t,t*)+min(b,b*)+1), iou = inter/(area+area*-inter);
 *     giou 0: -logf(max(iou, eps)) (gradient 0 where iou < eps); giou 1: 1 - (iou - (enc - union)/enc), enc the same
 *     product with max in place of min.  loss_bbox = sum c* loss / sum c* (0 without positives); loss_centerness =
 *     sum (softplus(z) - c* z) / max(positives, 1), z the centre-ness logit.  min selects the prediction where
 *     d <= d*, max where d >= d*: these masks carry the gradient.
 * A point that is not positive has its reg / ctr elements never read and gets gradient exactly 0.
 * Forward (two launches): losses fp32 [3] = (loss_cls, loss_bbox, loss_centerness); norm fp32 [3] = the three divisors;
 * scale_sums fp64 [L] (NULL iff scales is NULL) = per level sum over positives and j of c* (dloss/dd_j) d_j reg_j.
 * Backward (one launch) takes the cotangent g fp32 [3], norm and scale_sums back, writes every element of dcls / dreg /
 * dctr in the head dtype and dscales fp32 [L] = (g[1] / norm[1]) * scale_sums[l] (NULL iff scales is NULL).
 * Sums are fp64 in an order fixed by the shapes; no float atomics, no memset, no host synchronisation.
 * Limits: B 1..64, C 1..TDN_LOSS_MAX_CLASSES, gamma >= 0, alpha in [0, 1], eps in (0, 1). */
typedef struct tdn_fcos_loss_config {
  int32_t dtype;               /* TDN_BF16 / TDN_F16 / TDN_F32, of every head output and gradient */
  int32_t num_classes;         /* C */
  int32_t giou;                /* 0: -log(iou), 1: GIoU */
  int32_t reserved;
  float gamma, alpha, eps;
  int32_t reserved2;
} tdn_fcos_loss_config;
int64_t tdn_fcos_loss_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B, const tdn_fcos_loss_config* cfg);
int tdn_fcos_loss_fwd(const tdn_fcos_level* levels, int nlevels, int B, const tdn_fcos_loss_config* cfg,
                      const int64_t* labels, const float* bbox_targets, const float* scales, float* losses,
                      float* norm, double* scale_sums, void* workspace, int64_t workspace_bytes, void* stream);
int tdn_fcos_loss_bwd(const tdn_fcos_level* levels, int nlevels, int B, const tdn_fcos_loss_config* cfg,
                      const int64_t* labels, const float* bbox_targets, const float* scales, const float* g,
                      const float* norm, const double* scale_sums, float* dscales, void* stream);
/* FCOS test-time detections: tdn_dense_detections' architecture and limits with A = 1 and points in place of anchors.
 * sg(v) = 1 / (1 + expf(-v)).  The key of point i of (image, level) is sg(max_c cls_c) * sg(ctr), one fp32 product; a
 * level of n_l > nms_pre > 0 points keeps the nms_pre first by (key desc, point asc), any other level all n_l; k_l kept,
 * K = sum k_l.  (image b, level l) owns dense rows [b*K + off_l, b*K + off_l + k_l), its kept points there in ascending
 * point order: dense_scores fp32 [B*K][C+1] (column 0 = 0, column 1+c = sg(cls_c) * sg(ctr)), dense_boxes fp32 [B*K][4]
 * = (x - d_l, y - d_t, x + d_r, y + d_b), d_j = expf(scales[l] * reg_j), clipped to [0, w-1] / [0, h-1] of img_shapes[b]
 * = (h, w) (device int32 [B][2]), then divided by scale_factors[b] (device fp32 [B]) or, when that is NULL, by
 * cfg->scale_factor (0: none); batch_idx int32 [B*K]; dense_point_idx int64 [B*K] (row of the pyramid).  Then
 * tdn_multiclass_nms on those four: dets, labels, row_idx, counts as there, and point_idx int64 [B][max_num] =
 * dense_point_idx[row_idx], -1 on unused rows.  Launches: 1 key (none if no level selects), 1 select + decode,
 * tdn_multiclass_nms's 4, 1 gather: 7 (6).  tdn_fcos_detections_plan is host-only: out16 = {K, B*K, points per image,
 * launches, workgroups of the key launch, levels that select, key words of the workspace, 0, k_0 .. k_7}.
 * workspace: tdn_fcos_detections_workspace_bytes() bytes, 256-aligned.  NaN logits are unsupported. */
typedef struct tdn_fcos_det_config {
  int32_t dtype;               /* TDN_F32 / TDN_BF16 / TDN_F16, every head output */
  int32_t num_classes;         /* C, 1..TDN_DET_MAX_CLASSES - 1 */
  int32_t nms_pre;             /* > 0: points kept per level; 0: all */
  int32_t max_num;             /* 1..TDN_RPN_MAX_NUM detections per image */
  float score_thr, nms_thr;
  float scale_factor;          /* used when scale_factors == NULL; 0: no rescale */
  int32_t reserved;
} tdn_fcos_det_config;
int tdn_fcos_detections_plan(const tdn_fcos_level* levels, int nlevels, int B, const tdn_fcos_det_config* cfg,
                             int32_t* out16);
int64_t tdn_fcos_detections_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B,
                                            const tdn_fcos_det_config* cfg);
int tdn_fcos_detections(const tdn_fcos_level* levels, int nlevels, int B, const int32_t* img_shapes,
                        const float* scale_factors, const float* scales, const tdn_fcos_det_config* cfg,
                        float* dense_scores, float* dense_boxes, int32_t* batch_idx, int64_t* dense_point_idx,
                        float* dets, int64_t* labels, int64_t* row_idx, int64_t* point_idx, int32_t* counts,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---- soft-NMS in place of the greedy NMS of the five test-time entry points above (the project's own
 *      spec in the lineage of mmdetection v1's soft_nms_cpu; '+1' boxes, strict fp32 in the spec's operation order) ----
 * One (image, class) segment of candidates (score > score_thr, as above), repeated until no candidate is alive:
 *   select  the alive candidate with the largest current score, ties to the lowest source row; it is retired and is the
 *           segment's next survivor, with its current score;
 *   decay   for every other alive candidate j, with w, h, inter, uni and ov = inter / uni formed as tdn_nms forms the IoU
 *           of (selected, j): if w > 0 and h > 0, score_j = weight * score_j (one fp32 product), and j is dropped for
 *           good if the product is < min_score.
 * weight: TDN_SOFT_LINEAR ov > iou_thr ? 1 - ov : 1; TDN_SOFT_NAIVE ov > iou_thr ? 0 : 1 (greedy NMS when
 * 0 < min_score <= score_thr); TDN_SOFT_GAUSSIAN soft_exp(-(ov * ov) / sigma), soft_exp the library's own fp32
 * exponential on [-64, 0] (range reduction, degree-7 polynomial, exact scaling; relative error <= 4 * 2^-24), the same
 * bits on every run and in the CPU oracle.  A segment's survivors keep their selection order; per image the best
 * min(max_num, survivors) by (final score desc, class asc, selection order).  dets[..][4] is the final score; every
 * other output, limit and the counts = -1 rule are those of the entry point without _soft.
 * Refused (-1, tdn_last_error): method not one of the three; a non-finite iou_thr, sigma or min_score; sigma outside
 * [1/64, 64]; min_score < 0.  Each entry point takes the arguments of its namesake with `soft` in place of nms_thr (the
 * config structs' nms_thr is not read) and has a workspace query of its own: there is no suppression mask, so the
 * workspace is smaller.  One launch fewer than the namesake: the segment launch, one workgroup per segment for the whole
 * soft-NMS, the merge.  No host synchronisation, no memset, no float atomics, no inter-workgroup waits. */
#define TDN_SOFT_NAIVE 0
#define TDN_SOFT_LINEAR 1
#define TDN_SOFT_GAUSSIAN 2
typedef struct tdn_soft_nms_config {
  int32_t method;              /* TDN_SOFT_NAIVE / TDN_SOFT_LINEAR / TDN_SOFT_GAUSSIAN */
  float iou_thr;               /* linear and naive: pairs with ov > iou_thr decay */
  float sigma;                 /* gaussian; in [1/64, 64] */
  float min_score;             /* >= 0: a decayed score below it drops the candidate */
} tdn_soft_nms_config;
int64_t tdn_multiclass_nms_soft_workspace_bytes(int N, int C, int B);
int tdn_multiclass_nms_soft(const float* boxes, int box_cols, const float* scores, const void* batch_idx,
                            int batch_idx_bytes, int N, int C, int B, float score_thr, const tdn_soft_nms_config* soft,
                            int max_num, float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts,
                            void* workspace, int64_t workspace_bytes, void* stream);
int64_t tdn_bbox_detections_soft_workspace_bytes(int R, int C, int B);
int tdn_bbox_detections_soft(const float* rois, const void* cls, const void* reg, int dtype, int R, int C, int reg_cols,
                             int B, const int32_t* img_shapes, const float* scale_factors, float scale_factor,
                             const float* means4, const float* stds4, double wh_ratio_clip, float score_thr,
                             const tdn_soft_nms_config* soft, int max_num, float* dense_scores, float* dense_boxes,
                             float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                             int64_t workspace_bytes, void* stream);
int64_t tdn_cascade_detections_soft_workspace_bytes(int R, int C, int B);
int tdn_cascade_detections_soft(const float* rois, const void* const* cls, int num_stages, const void* reg, int dtype,
                                int R, int C, int reg_cols, int B, const int32_t* img_shapes,
                                const float* scale_factors, float scale_factor, const float* means4,
                                const float* stds4, double wh_ratio_clip, float score_thr,
                                const tdn_soft_nms_config* soft, int max_num, float* dense_scores, float* dense_boxes,
                                float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                                int64_t workspace_bytes, void* stream);
int64_t tdn_dense_detections_soft_workspace_bytes(const tdn_dense_level* levels, int nlevels, int B,
                                                  const tdn_dense_config* cfg);
int tdn_dense_detections_soft(const tdn_dense_level* levels, int nlevels, int B, const int32_t* img_shapes,
                              const float* scale_factors, const tdn_dense_config* cfg,
                              const tdn_soft_nms_config* soft, float* dense_scores, float* dense_boxes,
                              int32_t* batch_idx, int64_t* dense_anchor_idx, float* dets, int64_t* labels,
                              int64_t* row_idx, int64_t* anchor_idx, int32_t* counts, void* workspace,
                              int64_t workspace_bytes, void* stream);
int64_t tdn_fcos_detections_soft_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B,
                                                 const tdn_fcos_det_config* cfg);
int tdn_fcos_detections_soft(const tdn_fcos_level* levels, int nlevels, int B, const int32_t* img_shapes,
                             const float* scale_factors, const float* scales, const tdn_fcos_det_config* cfg,
                             const tdn_soft_nms_config* soft, float* dense_scores, float* dense_boxes,
                             int32_t* batch_idx, int64_t* dense_point_idx, float* dets, int64_t* labels,
                             int64_t* row_idx, int64_t* point_idx, int32_t* counts, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ---- gradient-harmonised losses of the dense anchor heads: GHM-C and GHM-R with their gradients (the
 *      project's own spec in the lineage of mmdetection v1's GHMC / GHMR; tests/ghm_ref.py restates it) ----
 * levels, labels, label_weights, bbox_targets and bbox_weights are tdn_loss_dense_fwd's.  A class element (b, n, c) is
 * valid iff label_weights[b][n] > 0, a box element (b, n, j) iff bbox_weights[b][n][j] > 0; a weight's value is used for
 * nothing else and an invalid element is never evaluated (loss 0, gradient exactly 0, whatever its logit).  Rows: with
 * TDN_GHM_SCOPE_LEVEL every level is a row, with TDN_GHM_SCOPE_BATCH all levels are one; tot[r] = max(valid elements of
 * row r, 1).  Per valid element, fp32 in the order written:
 *   GHM-C  e = soft_exp(-|x|) (the library's own fp32 exponential, as in tdn_multiclass_nms_soft); sigma(z) = z >= 0 ?
 *          1 / (1 + e) : e / (1 + e); g = t ? sigma(-x) : sigma(x); l = max(t ? -x : x, 0) + log1pf(e); dl = t ? -g : g
 *   GHM-R  d = pred - target; q = sqrt(d d + mu2), mu2 = fp32(mu mu in double); g = |d| / q; l = (d d) / (q + mu);
 *          dl = d / q
 *   bin    the i in [0, bins) with edge[i] <= g < edge[i + 1], edge[i] = fp32(i) / fp32(bins), the last bin closed above;
 *          a NaN g lies in no bin: the element counts in tot and its loss term and gradient are that NaN
 * Weights, per kind, rows in order, bins in order, skipping bins with cnt[r][i] == 0: with momentum > 0
 * acc[i] = momentum acc[i] + (1 - momentum) float(cnt) and w = float(tot) / acc[i], else w = float(tot) / float(cnt);
 * beta[r][i] = w / float(non-empty bins of row r).  acc_cls fp32 [bins_cls] / acc_reg fp32 [bins_reg] are the caller's
 * state, updated in place row after row by every forward call (NULL allowed iff that momentum is 0).
 * losses fp32 [2] = per kind sum over rows of (fp64 sum of fp32 beta l) / tot[r], in an order fixed by the shapes,
 * rounded once.  table fp32 [2][TDN_LOSS_MAX_LEVELS][TDN_GHM_TABLE_STRIDE], written in full by the forward and read by
 * the backward: per (kind, row) beta [64], float(cnt) [64], float(tot), the number of non-empty bins, the number of valid
 * elements in no bin, zeros.  Backward: d x = (beta dl) (g[kind] / float(tot[r])), rounded to nearest even into the
 * head's dtype; it touches neither the counts nor acc.  Forward: four launches, backward: one; no float atomics, no
 * host synchronisation.  Limits: tdn_loss_dense_fwd's, bins 1..TDN_GHM_MAX_BINS, momentum in [0, 1), mu finite and > 0.
 * workspace: tdn_ghm_workspace_bytes() bytes, 256-aligned. */
#define TDN_GHM_MAX_BINS 64
#define TDN_GHM_TABLE_STRIDE 136
#define TDN_GHM_SCOPE_LEVEL 0
#define TDN_GHM_SCOPE_BATCH 1
typedef struct tdn_ghm_config {
  int32_t dtype;               /* TDN_BF16 / TDN_F16 / TDN_F32, of every head output and gradient */
  int32_t num_anchors;         /* A */
  int32_t num_classes;         /* C: label k in 1..C is one-hot on class channel k-1, 0 is background */
  int32_t bins_cls, bins_reg;  /* 1..TDN_GHM_MAX_BINS */
  int32_t scope;               /* TDN_GHM_SCOPE_LEVEL / TDN_GHM_SCOPE_BATCH */
  float momentum_cls, momentum_reg; /* in [0, 1) */
  float mu;                    /* GHM-R's knee, finite and > 0 */
  int32_t reserved;
} tdn_ghm_config;
int64_t tdn_ghm_workspace_bytes(const tdn_loss_level* levels, int num_levels, int B, const tdn_ghm_config* cfg);
int tdn_ghm_fwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_ghm_config* cfg, const int64_t* labels,
                const float* label_weights, const float* bbox_targets, const float* bbox_weights, float* acc_cls,
                float* acc_reg, float* losses, float* table, void* workspace, int64_t workspace_bytes, void* stream);
int tdn_ghm_bwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_ghm_config* cfg, const int64_t* labels,
                const float* label_weights, const float* bbox_targets, const float* bbox_weights, const float* g,
                const float* table, void* stream);

/* ---- Guided Anchoring: location targets, shape targets, the location + shape loss, the guided anchors (DESIGN.md §4w:
 *      the project's own spec in the lineage of mmdetection v1's GuidedAnchorHead; tests/ga_ref.py restates it) ----
 * A pyramid is 1..TDN_LOSS_MAX_LEVELS levels; locations are level-major, (y*W + x) within a level, N = sum H*W <=
 * TDN_TARGET_MAX_BOXES.  Head outputs: loc (B, 1, H, W) logits, shape (B, 2, H, W) = (dw, dh), TDN_F32 / TDN_BF16 /
 * TDN_F16, NCHW-contiguous or channels_last, read in place.  Boxes are fp32 '+1' xyxy; ground truths gt fp32 [B][G][4]
 * with gt_counts int32 [B] (clamped to 0..G, rows past it never read), G <= TDN_TARGET_MAX_GT.  Nothing synchronises with
 * the host; the only atomics are integer maxima / minima, every output is a pure function of the inputs. */
#define TDN_GA_MAX_APPROX 16
typedef struct tdn_ga_level {
  const void* loc;             /* (B, 1, H, W) */
  const void* shape;           /* (B, 2, H, W) */
  void* dloc;                  /* backward only: gradients, laid out as loc / shape */
  void* dshape;
  int32_t H, W;
  int32_t stride;              /* tdn_ga_loc_target only: 1..32768, H*stride and W*stride below 2^24 */
  int32_t shape_nhwc;          /* 0: NCHW-contiguous memory, 1: channels_last */
} tdn_ga_level;
/* Location targets, one launch.  The level of a ground truth: #{k in 1..L-1 : area >= area_thr[k-1]}, area the fp32
 * product of its '+1' sides.  A region of ratio pair (r, c) on level l: g = gt / stride_l, x1 = rint(c g.x1 + r g.x2),
 * x2 = rint(r g.x1 + c g.x2), the same for y, fp32 with one rounding per operation, rint to even, clamped to the map.
 * Per location, ground truths in ascending j, from t = 0, w = -1, ig = 0: j on the location's level: inside the ignore
 * region w = 0, then inside the centre region t = 1, w = 1; j one level above or below: inside its ignore region at this
 * level's stride ig = 1.  At the end w < 0 becomes ig ? 0 : 0.1.  loc_targets int64 [B][N], loc_weights fp32 [B][N]. */
typedef struct tdn_ga_loc_config {
  float area_thr[TDN_LOSS_MAX_LEVELS]; /* [0, L-1): finite, positive, ascending */
  float center_r, center_c;    /* fp32((1 - center_ratio) / 2), fp32(1 - that) */
  float ignore_r, ignore_c;    /* the same of ignore_ratio */
} tdn_ga_loc_config;
int tdn_ga_loc_target(const tdn_ga_level* levels, int nlevels, int B, const float* gt, const int32_t* gt_counts, int G,
                      const tdn_ga_loc_config* cfg, int64_t* loc_targets, float* loc_weights, void* stream);
/* Shape targets: tdn_anchor_target's assignment and sampling (cfg: its thresholds, gt_max_assign_all, num,
 * num_pos_expected, neg_pos_ub, allowed_border, seed) with the overlap of location i and ground truth j = max over a of
 * IoU(approxs[i][a], gt[j]), approxs fp32 [N][A][4], A <= TDN_GA_MAX_APPROX.  valid uint8 [N*A] (valid_stride 0) or
 * [B][N*A] (valid_stride N*A) or NULL; a location takes part iff one of its approxs is flagged valid and, with
 * allowed_border >= 0, inside the image by tdn_anchor_target's rule; the maximum runs over all A.  sampling == 0: every
 * positive and every negative.  On sampled positives bbox_anchors fp32 [B][N][4] = squares[i] (squares fp32 [N][4]),
 * bbox_gts = the assigned ground truth, bbox_weights = 1; zeros elsewhere.  num_pos / num_neg int32 [B], assigned int32
 * [B][N], max_overlaps fp32 [B][N].  Launches: clear, two assign passes, the first-index pass (gt_max_assign_all = 0),
 * select, fill.  workspace: tdn_ga_shape_target_workspace_bytes() bytes, 256-aligned. */
int64_t tdn_ga_shape_target_workspace_bytes(int B, int N, int G);
int tdn_ga_shape_target(const float* approxs, int A, const float* squares, const uint8_t* valid, int64_t valid_stride,
                        const float* gt, const int32_t* gt_counts, const int32_t* img_shapes, int B, int N, int G,
                        const tdn_target_config* cfg, int sampling, const int32_t* keys, float* bbox_anchors,
                        float* bbox_gts, float* bbox_weights, int32_t* num_pos, int32_t* num_neg, int32_t* assigned,
                        float* max_overlaps, void* workspace, int64_t workspace_bytes, void* stream);
/* Guided anchors, one launch: anchors fp32 [B][N][4] = tdn_delta2bbox's decode of squares[i] with deltas (0, 0, dw, dh),
 * wh_ratio_clip 1e-6, no clipping to an image; loc_mask uint8 [B][N] = 1, or with use_loc (loc logit >= loc_thr_logit). */
int tdn_guided_anchors(const tdn_ga_level* levels, int nlevels, int B, int dtype, const float* squares,
                       const float* means4, const float* stds4, int use_loc, float loc_thr_logit, float* anchors,
                       uint8_t* loc_mask, void* stream);
/* The loss.  losses fp32 [2] = (loss_loc, loss_shape); norm fp32 [2] = their divisors, which the backward takes back.
 *   loss_loc    sum over (b, n) with loc_weights != 0 of loc_weights * focal(loc logit, loc_targets == 1) (the focal
 *               element of tdn_loss_dense_fwd), divided by loc_avg_factor; a location of weight 0 is never evaluated
 *   loss_shape  over the rows with bbox_weights[b][n][0] > 0: the box p = tdn_delta2bbox's decode of bbox_anchors with
 *               (0, 0, dw, dh), means, stds and wh_ratio_clip 1e-6; per axis, with centres (x1 + x2) / 2 and sizes
 *               x2 - x1 + 1 of p and of bbox_gts, D = 2 |ct - cp|:  l_c = 1 - max((st - D) / (st + D + eps), 0),
 *               l_s = 1 - min(st / (sp + eps), sp / (st + eps)); each l shaped as l < beta ? 0.5 l l / beta :
 *               l - 0.5 beta and weighted by its bbox_weights element (x, y, w, h); divided by avg (tdn_loss_avg mode 0
 *               or 1).  Other rows never have their shape outputs, anchors or ground truths read.
 * Gradients reach only dw, dh, through the size terms; min's tie takes half of each side and the clamp passes the
 * gradient on [-R, R] inclusive, as torch does.  Forward: two launches, backward: one; sums are fp64 in an order fixed by
 * the shapes.  workspace: tdn_ga_loss_workspace_bytes() bytes, 256-aligned. */
typedef struct tdn_ga_loss_config {
  int32_t dtype;               /* TDN_BF16 / TDN_F16 / TDN_F32, of every head output and gradient */
  float gamma, alpha;          /* focal: gamma >= 0, alpha in [0, 1] */
  float beta;                  /* the knee, > 0 */
  float eps;                   /* in (0, 1) */
  float loc_avg_factor;        /* finite and > 0 */
  float means[4], stds[4];     /* the anchoring normalisation */
} tdn_ga_loss_config;
int64_t tdn_ga_loss_workspace_bytes(const tdn_ga_level* levels, int nlevels, int B, const tdn_ga_loss_config* cfg);
int tdn_ga_loss_fwd(const tdn_ga_level* levels, int nlevels, int B, const tdn_ga_loss_config* cfg,
                    const int64_t* loc_targets, const float* loc_weights, const float* bbox_anchors,
                    const float* bbox_gts, const float* bbox_weights, const tdn_loss_avg* avg, float* losses, float* norm,
                    void* workspace, int64_t workspace_bytes, void* stream);
int tdn_ga_loss_bwd(const tdn_ga_level* levels, int nlevels, int B, const tdn_ga_loss_config* cfg,
                    const int64_t* loc_targets, const float* loc_weights, const float* bbox_anchors,
                    const float* bbox_gts, const float* bbox_weights, const float* g, const float* norm, void* stream);
/* Guided RPN proposals: tdn_rpn_proposals (levels, cfg, outputs, padding rules, limits, launch count: its four, the
 * first one replaced) with one anchor per location (every level's A must be 1; the levels' own anchors pointers are
 * ignored), anchors fp32 [B][N][4] that differ per image and loc_mask uint8 [B][N], N = sum H*W over the levels in
 * order, both as tdn_guided_anchors writes them.  A location whose mask byte is 0 is absent: level l of image b sends
 * the min(nms_pre, locations in) highest logits of its locations that are in to NMS (all of them with nms_pre = 0).
 * With anchors repeated for every image and a mask of ones the outputs are tdn_rpn_proposals' bit for bit.  NaN logits
 * are unsupported.  workspace: tdn_ga_rpn_proposals_workspace_bytes() bytes (tdn_rpn_proposals' own size),
 * 256-aligned. */
int64_t tdn_ga_rpn_proposals_workspace_bytes(const tdn_rpn_level* levels, int nlevels, int B,
                                             const tdn_rpn_config* cfg);
int tdn_ga_rpn_proposals(const tdn_rpn_level* levels, int nlevels, int B, const float* anchors, const uint8_t* loc_mask,
                         const int32_t* img_shapes, const tdn_rpn_config* cfg, float* proposals, int64_t* anchor_idx,
                         int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the mask branch of Mask R-CNN: polygon mask targets, mask loss, mask paste (the project's own
 *      spec in the mmdetection-v1 lineage of mask_target / FCNMaskHead.loss / get_seg_masks) ----
 * Polygons: poly_xy fp32 [P][2] vertices in the network-input frame; poly_offsets int32 [Q + 1]: polygon q owns vertices
 * [poly_offsets[q], poly_offsets[q + 1]); gt_poly_offsets int32 [B][G + 1]: ground truth j of image b owns polygons
 * [gt_poly_offsets[b][j], gt_poly_offsets[b][j + 1]).  Every offset read on the device is clamped to its array.
 * tdn_mask_target, one launch: row r of rois fp32 [R][5] = (batch_idx, x1, y1, x2, y2) with gt_inds int32 [R] is valid
 * iff its truncated batch index is in [0, B) and 0 <= gt_inds[r] < G; targets uint8 [R][M][M] = 1 where the cell centre
 * of the truncated box lies inside any polygon of the instance (even-odd per polygon, union across polygons), weights
 * fp32 [R] = 1; an invalid row gets zeros and weight 0.  1 <= M <= TDN_MASK_MAX_SIZE, R <= TDN_LOSS_MAX_ROWS. */
#define TDN_MASK_MAX_SIZE 56
int tdn_mask_target(const float* rois, const int32_t* gt_inds, int R, const float* poly_xy, int P,
                    const int32_t* poly_offsets, int Q, const int32_t* gt_poly_offsets, int B, int G, int M,
                    uint8_t* targets, float* weights, void* stream);
/* pred [R][C][M][M] logits, TDN_F32 / TDN_BF16 / TDN_F16, nhwc 0: NCHW-contiguous memory, 1: channels_last memory; row r
 * reads channel labels[r] (int64, 1..C-1; C == 1: channel 0) against targets uint8 [R][M][M] with weights fp32 [R];
 * loss fp32 [1] = sum_r w_r sum_ij bce / (D M^2), D from avg as tdn_loss_roi_fwd takes it (mode 2: rows with w > 0);
 * avg_out fp32 [1] = D, which the backward takes as avg_in with the cotangent g fp32 [1].  A row whose weight is exactly
 * 0 is never read; a row whose label is outside its range counts as weight 0.  dpred has pred's layout and is written
 * in full.  Forward two launches, backward one.  R <= TDN_LOSS_MAX_ROWS, C <= TDN_LOSS_MAX_CLASSES, R C M^2 < 2^31.
 * workspace: tdn_mask_loss_workspace_bytes() bytes, 256-aligned. */
int64_t tdn_mask_loss_workspace_bytes(int R);
int tdn_mask_loss_fwd(const void* pred, int dtype, int nhwc, int R, int C, int M, const uint8_t* targets,
                      const int64_t* labels, const float* weights, const tdn_loss_avg* avg, float* loss, float* avg_out,
                      void* workspace, int64_t workspace_bytes, void* stream);
int tdn_mask_loss_bwd(const void* pred, int dtype, int nhwc, int R, int C, int M, const uint8_t* targets,
                      const int64_t* labels, const float* weights, const float* g, const float* avg_in, void* dpred,
                      void* stream);
/* dets fp32 [B][max_num][5] and counts int32 [B] of tdn_multiclass_nms -> rois fp32 [B * max_num][5] =
 * (b, x1 s, y1 s, x2 s, y2 s) for rows below counts[b], (-1, 0, 0, 0, 0) for the rest; s = scale_factors[b] (device
 * fp32 [B]) or, when that is NULL, scale_factor. */
int tdn_rois_from_detections(const float* dets, const int32_t* counts, int B, int max_num, const float* scale_factors,
                             float scale_factor, float* rois, void* stream);
/* pred [B * max_num][C][M][M] as above, in the row order of tdn_rois_from_detections; dets in the frame of the H x W
 * canvas, labels int64 [B][max_num] 0-based foreground labels (channel label + 1, or 0 when C == 1), img_shapes device
 * int32 [B][2] = (h, w) or NULL.  out uint8 [B * max_num][H][W] (packed 0) = bilinear sample of sigmoid(pred) > thr
 * inside the truncated box, the canvas and the image, 0 elsewhere; packed 1: [B * max_num][H][8 ceil(W / 64)], bit
 * x % 8 of byte x / 8 is pixel x.  Every byte is written.  One launch. */
int tdn_mask_paste(const void* pred, int dtype, int nhwc, int B, int max_num, int C, int M, const float* dets,
                   const int64_t* labels, const int32_t* counts, const int32_t* img_shapes, int H, int W, float thr,
                   int packed, uint8_t* out, void* stream);

/* ---- Mask Scoring R-CNN around the MaskIoUHead's layers (mmdetection v1's MaskIoUHead.get_target,
 *      its MSELoss on the positive targets and get_mask_scores) ----
 * tdn_mask_iou_target, one launch: rois, gt_inds and the polygon arrays are tdn_mask_target's and so is the validity of
 * a row; pred / dtype / nhwc / C / labels are tdn_mask_loss_fwd's (row r reads channel labels[r]); targets uint8
 * [R][M][M] are tdn_mask_target's; img_shapes int32 [B][2] = (h, w), each clamped to 0..TDN_MASK_IOU_MAX_CANVAS on the
 * device.  The instance's bitmap has pixel (x, y) of the h x w canvas set iff (x + 0.5, y + 0.5) is inside any of its
 * polygons by §4g's crossing test; full = its population count, in = the count over x in [max(x1, 0), min(x2, w - 1)],
 * y alike (the truncated box; an empty range counts 0); pa = #{logit > thr}, ts = #{target == 1}, ov = #{both}.
 *   ratio = in / (full + 1e-7f);  gf = ts / (ratio + 1e-7f);  den = (pa + gf) - ov;  iou = den > 0 ? ov / den : 0
 * in fp32, one rounding per operation.  iou fp32 [R]; an invalid row or a label without a channel gives 0 and neither
 * its logits nor its polygons are read. */
#define TDN_MASK_IOU_MAX_CANVAS 8192
int tdn_mask_iou_target(const float* rois, const int32_t* gt_inds, int R, const float* poly_xy, int P,
                        const int32_t* poly_offsets, int Q, const int32_t* gt_poly_offsets, int B, int G,
                        const void* pred, int dtype, int nhwc, int C, int M, const int64_t* labels,
                        const uint8_t* targets, const int32_t* img_shapes, float thr, float* iou, void* stream);
/* pred [R][C] TDN_F32 / TDN_BF16 / TDN_F16; row r is live iff targets[r] > 0 and labels[r] (int64) is in 1..C-1; a row
 * that is not live is never read.  loss fp32 [1] = loss_weight sum_live (pred[r][labels[r]] - targets[r])^2 / D with
 * D = max(#live, 1) counted on the device; avg_out fp32 [1] = D, which the backward takes as avg_in with the cotangent
 * g fp32 [1]: dpred [R][C] = (pred - target) ((2 loss_weight g) / D) at [r][labels[r]] of a live row, 0 elsewhere,
 * written in full in pred's dtype.  Forward two launches, backward one.  workspace:
 * tdn_mask_iou_loss_workspace_bytes() bytes, 256-aligned. */
int64_t tdn_mask_iou_loss_workspace_bytes(int R);
int tdn_mask_iou_loss_fwd(const void* pred, int dtype, int R, int C, const int64_t* labels, const float* targets,
                          float loss_weight, float* loss, float* avg_out, void* workspace, int64_t workspace_bytes,
                          void* stream);
int tdn_mask_iou_loss_bwd(const void* pred, int dtype, int R, int C, const int64_t* labels, const float* targets,
                          float loss_weight, const float* g, const float* avg_in, void* dpred, void* stream);
/* scores fp32 [B][max_num] = (float)pred[b max_num + d][labels[b][d] + 1] * dets[b][d][4] (one fp32 product) for
 * d < counts[b] and 0 <= labels[b][d] + 1 < C, 0 elsewhere (every row under the overflow marker counts[b] = -1).  One
 * launch. */
int tdn_mask_scores(const void* pred, int dtype, int B, int max_num, int C, const float* dets, const int64_t* labels,
                    const int32_t* counts, float* scores, void* stream);

/* The mask channel of the MaskIoUHead's first 3x3 conv over cat(feats, maxpool2x2(sigmoid(pred[r][ch_r]))): by
 * linearity the layer is conv_Cf(feats) + conv_1(P), and these form the second term as the epilogue addend of the
 * library's own conv launch.  pred [R][C][2S][2S] as tdn_mask_loss_fwd takes it; row r reads channel
 * labels[r] + label_offset (1..C-1; C == 1: channel 0), a row without a channel has P = 0, is never read and gets no
 * gradient.  weight fp32 [Cout][Cf + 1][3][3] contiguous (only its last input channel is read); Cf and Cout multiples
 * of 64, Cout <= TDN_MASK_IOU_MAX_COUT, 1 <= S <= TDN_MASK_MAX_SIZE / 2, R >= 1.
 * tdn_mask_iou_stem_fwd, one launch: P fp32 [R][S][S] = the FIRST maximum in row-major order of each 2x2 window of
 * sigmoid(pred) (replaced on strict >), idx uint8 [R][S][S] = its place 2 dy + dx in the window (255: no channel),
 * a [R][S][S][Cout] in out_dtype (TDN_BF16 / TDN_F16) = sum over the nine taps in (ky, kx) order of
 * weight[co][Cf][ky][kx] P[i + ky - 1][j + kx - 1] (P = 0 outside the map), fp32 products and adds, rounded once.
 * tdn_mask_iou_stem_bwd, two launches, from gz [R][S][S][Cout] (gz_dtype) = the layer's cotangent behind its ReLU:
 * dP fp32 [R][S][S] = sum_taps sum_co weight[co][Cf][ky][kx] gz[i - ky + 1][j - kx + 1][co]; dpred (pred's layout and
 * dtype, written in full) = dP sigmoid(x) sigmoid(-x) at each window's first maximum, 0 elsewhere; dw1 fp32
 * [Cout][3][3] = sum_{r,i,j} gz[r][i][j][co] P[r][i + ky - 1][j + kx - 1] (fp32 products, fp64 sums in a fixed order).
 * workspace: tdn_mask_iou_stem_bwd_workspace_bytes() bytes, 256-aligned. */
#define TDN_MASK_IOU_MAX_COUT 512
int tdn_mask_iou_stem_fwd(const void* pred, int dtype, int nhwc, int R, int C, int S, const int64_t* labels,
                          int label_offset, const float* weight, int Cf, int Cout, void* a, int out_dtype, float* P,
                          uint8_t* idx, void* stream);
int64_t tdn_mask_iou_stem_bwd_workspace_bytes(int R, int S, int Cout);
int tdn_mask_iou_stem_bwd(const void* gz, int gz_dtype, const float* P, const uint8_t* idx, const float* weight, int Cf,
                          int Cout, const void* pred, int dtype, int nhwc, int R, int C, int S, const int64_t* labels,
                          int label_offset, float* dP, void* dpred, float* dw1, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- fused SGD step: gradient-norm clip, loss unscaling, momentum update (no reference counterpart:
 *      SURVEY row 25) ----
 * One item per parameter: p, g and buf are fp32 device pointers to the lowest address of a dense, non-overlapping
 * tensor of `shape` (fewer than 4 dims: leading 1s); p_stride / g_stride are element strides, buf has p's strides and
 * is NULL when the item's group has momentum 0.  Fewer than 2^31 elements per item.  Three access paths, chosen from the
 * strides (tdn_sgd_plan reports them):
 *   TDN_SGD_PATH_LINEAR      p and g share one layout: 16-byte loads and stores when all three pointers are aligned
 *   TDN_SGD_PATH_TRANSPOSED  p contiguous [O][I][kh][kw], g stored [O][kh][kw][I] (the gradient views of a reducer):
 *                            per output channel a kh kw x I block is transposed through LDS
 *   TDN_SGD_PATH_GENERAL     any other pair of dense permutations, element by element */
typedef struct {
  float* p;
  const float* g;
  float* buf;
  int64_t shape[4];
  int64_t p_stride[4];
  int64_t g_stride[4];
  int32_t group;             /* row of the hyper-parameter array */
  int32_t reserved;
} tdn_sgd_item;
#define TDN_SGD_MAX_ITEMS (1 << 20)
#define TDN_SGD_MAX_GROUPS 1024
#define TDN_SGD_PATH_LINEAR 0
#define TDN_SGD_PATH_TRANSPOSED 1
#define TDN_SGD_PATH_GENERAL 2
/* flags */
#define TDN_SGD_NESTEROV 1
#define TDN_SGD_SKIP_NONFINITE 2
#define TDN_SGD_DYNAMIC_SCALE 4
/* fstate: device fp32 [TDN_SGD_F_COUNT]; istate: device int32 [TDN_SGD_I_COUNT].  The caller initialises
 * fstate[F_SCALE] (1 without loss scaling) and zeroes the rest; I_BUF_INIT != 0 says that the momentum buffers hold
 * values (a loaded checkpoint), 0 makes the next taken step copy instead of accumulate. */
#define TDN_SGD_F_SCALE 0
#define TDN_SGD_F_NORM 1
#define TDN_SGD_F_COEF 2
#define TDN_SGD_F_SNAP_SCALE 3
#define TDN_SGD_F_COUNT 4
#define TDN_SGD_I_TRACKER 0
#define TDN_SGD_I_TAKEN 1
#define TDN_SGD_I_SKIPPED 2
#define TDN_SGD_I_LAST_SKIPPED 3
#define TDN_SGD_I_BUF_INIT 4
#define TDN_SGD_I_SNAP_FIRST 5
#define TDN_SGD_I_COUNT 8
/* Host only.  plan8 = {table bytes, workspace bytes, workgroups of pass 1, workgroups of pass 2, norm chunks, update
 * chunks, n, n_groups}.  table_host NULL: the size query; else a 16-byte aligned HOST buffer of table_bytes >= plan8[0]
 * bytes that receives the table (item descriptors and the two chunk -> (item, offset) maps), which the caller copies
 * to 256-aligned device memory once.  paths: NULL or int32 [n], the access path of every item.  Overlapping or
 * non-dense tensors are refused. */
int tdn_sgd_plan(const tdn_sgd_item* items, int n, int n_groups, int64_t* plan8, void* table_host, int64_t table_bytes,
                 int32_t* paths);
/* The step, two launches, no host synchronisation, no atomics; table (device) and plan8 (host) of one tdn_sgd_plan call.
 * hyper: device fp32 [n_groups][3] = lr, weight decay, momentum.  Pass 1: S = sum of g^2 over all items in float64 (one
 * partial per norm chunk in the workspace), and the snapshot of fstate[F_SCALE] / !istate[I_BUF_INIT].  Pass 2, with
 * inv = 1 / scale, n = (float)(sqrt(S) * inv), coef = max_norm > 0 ? min(1, max_norm / (n + 1e-6)) : 1, m = coef * inv,
 * per element, each operation rounded to fp32 on its own:
 *   gh = g * m;  d = wd != 0 ? fma(wd, p, gh) : gh;  buf' = first step ? d : buf * mom + d;
 *   u = nesterov ? fma(mom, buf', d) : buf'  (no buf: u = d);  p' = fma(-lr, u, p)
 * which is torch.optim.SGD(foreach=False) bit for bit.  g is never written.  S not finite (an Inf or NaN gradient) with
 * TDN_SGD_SKIP_NONFINITE: p and buf are left untouched, istate[I_SKIPPED] advances instead of istate[I_TAKEN].  With
 * TDN_SGD_DYNAMIC_SCALE fstate[F_SCALE] and istate[I_TRACKER] follow torch._amp_update_scale_(growth, backoff,
 * interval).  fstate[F_NORM] = n, fstate[F_COEF] = coef, istate[I_LAST_SKIPPED] = 0 / 1.
 * workspace: plan8[1] bytes, 256-aligned. */
int tdn_sgd_step(const void* table, const int64_t* plan8, const float* hyper, float* fstate, int32_t* istate,
                 void* workspace, int64_t workspace_bytes, int flags, float max_norm, float growth, float backoff,
                 int interval, void* stream);

/* ---- fully connected layers ---------------------------------------------------------------------------
 * nn.Linear as the box head uses it (shared_fcs, fc_cls, fc_reg of the mmdetection-v1 SharedFCBBoxHead): 16-bit
 * operands, fp32 accumulation on the matrix cores, one rounding of the result.  K is a multiple of 64, O is any value in
 * 1..65536, M any value in 0..2^18; Op = O rounded up to 64.  ld* are row strides in ELEMENTS.  Nothing past row M or
 * column O is written and nothing outside an operand's rows is read.
 *
 * splits: 0 lets the library cut the reduction (see tdn_linear_plan); 1..K/64 (wgrad: 1..ceil(M/64), at least 1) forces
 * a slice count — a value above the number of 64-element chunks of the product's reduction (dgrad reduces over Op) means
 * one chunk per slice; anything else is an error.  With more than one slice every workgroup stores an fp32 partial slab
 * into the workspace and a finalize launch adds the slabs in slice order, then applies the epilogue: the result does not
 * depend on the run.  workspace: tdn_linear_workspace_bytes(kind, M, O, K, splits) bytes (may be 0, then NULL is taken),
 * 256-byte aligned; its regions, in order: the padded cotangent (dgrad / wgrad with O % 64 != 0: M x Op elements), the
 * slabs, wgrad's column-sum slabs.  kind: 0 forward, 1 dgrad, 2 wgrad.
 *
 * tdn_pack_linear_weight: w fp32 [O][K] with element strides (s_o, s_k) -> w_fwd [Op][K] and, unless NULL, w_dgrad
 *   [K][Op], each value rounded once to `dtype`, the rows / columns O..Op-1 zero.  C == K: the columns as they are;
 *   otherwise (C | K, C % 8 == 0, hw = K / C) logical column c * hw + p goes to packed column p * C + c, so that the
 *   forward reads a channels_last (R, S, S, C) RoI feature buffer and the dgrad writes its gradient in place.
 * tdn_linear_plan (host only): out[0..15] = {BM, BN, BK, row tiles, column tiles, tiles, slices, chunks per slice, chunks,
 *   workgroups of the GEMM launch, launches, 1 if a pad launch runs + 2 if the product is handed to the conv GEMM, slab bytes low 31 bits, slab bytes >> 31, workspace
 *   bytes low 31 bits, workspace bytes >> 31}.
 * With splits == 0, an unsplit forward / dgrad of a layer with O % 64 == 0 and dense rows (ld == row length) is computed
 * by tdn_conv2d_fwd / tdn_conv2d_dgrad as a 1x1 conv over M pixels (same operands, same arithmetic contract; measured
 * faster); any splits >= 1 keeps it in csrc/linear.hip.
 * tdn_linear_fwd:   y[m][o] = act(sum_k x[m][k] * w_fwd[o][k] + bias[o]);  bias fp32 or NULL, act = ReLU if relu, y
 *   16-bit, or fp32 if out_f32.
 * tdn_linear_dgrad: dx[m][k] = sum_o g[m][o] * w_dgrad[k][o], then 0 where mask_src[m][k] <= 0 (mask_src: the layer's own
 *   input, i.e. the previous layer's ReLU output, or NULL).  g rows need no alignment when O % 64 != 0 (one pad launch
 *   copies them); otherwise g and ldg must keep rows 16-byte aligned.
 * tdn_linear_wgrad: dw[o][j] = beta * dw[o][j] + sum_m g[m][o] * x[m][packed(j)] in fp32, dw contiguous [O][K] in the
 *   parameter's LOGICAL column order (C as in the pack); dbias[o] = beta * dbias[o] + sum_m g[m][o] (NULL: skipped).
 *   beta == 0 never reads dw / dbias.  M == 0 leaves beta * old.
 * tdn_linear_relu_bwd: out[m][o] = y[m][o] > 0 ? g[m][o] : 0 on contiguous (M, O) operands: the cotangent behind a
 *   layer's own ReLU, from its stored output y (16-bit; fp32 if y_f32).  Only a stand-alone layer needs it: in a chain
 *   the next layer's tdn_linear_dgrad applies this mask through mask_src. */
int tdn_pack_linear_weight(const float* w, int64_t s_o, int64_t s_k, int O, int K, int C, void* w_fwd, void* w_dgrad,
                           int dtype, void* stream);
int64_t tdn_linear_workspace_bytes(int kind, int M, int O, int K, int splits);
int tdn_linear_relu_bwd(const void* g, const void* y, int y_f32, void* out, int M, int O, int dtype, void* stream);
int tdn_linear_plan(int kind, int M, int O, int K, int splits, int32_t* out16);
int tdn_linear_fwd(const void* x, int64_t ldx, const void* w_fwd, const float* bias, void* y, int64_t ldy, int M, int O,
                   int K, int relu, int out_f32, int splits, void* workspace, int64_t workspace_bytes, int dtype,
                   void* stream);
int tdn_linear_dgrad(const void* g, int64_t ldg, const void* w_dgrad, const void* mask_src, int64_t ld_mask, void* dx,
                     int64_t lddx, int M, int O, int K, int splits, void* workspace, int64_t workspace_bytes, int dtype,
                     void* stream);
int tdn_linear_wgrad(const void* x, int64_t ldx, const void* g, int64_t ldg, float* dw, float* dbias, float beta, int M,
                     int O, int K, int C, int splits, void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* ---- 2x2 stride-2 transposed convolution ------------------------------------------------------------------
 * nn.ConvTranspose2d(Cin, Cout, 2, stride=2) as the mask head's upsampling layer uses it: 16-bit operands, fp32
 * accumulation on the matrix cores, one rounding of the result.  The taps do not overlap:
 *     y[r][2i+a][2j+b][o] = act(bias[o] + sum_c x[r][i][j][c] * W[c][o][a][b])
 * i.e. one GEMM with M = R*H*W input pixels, K = Cin and N = 4*Cout columns n = (a*2+b)*Cout + o whose rows are
 * scattered into (forward) or gathered from (dgrad, wgrad) the 2H x 2W map.  x is NHWC memory (R, H, W, Cin); y and its
 * cotangent g are NHWC memory (R, 2H, 2W, Cout); all of them dense and 16-byte aligned.  weight (Cin, Cout, 2, 2) and
 * bias (Cout) stay fp32.  Limits, checked on the host: Cin and Cout multiples of 64 in 64..65536, H >= 1, W >= 1,
 * R >= 0 (R == 0 is legal: nothing is launched but wgrad's finalize), R*H*W < 2^29, R*2H*2W*Cout < 2^31 and
 * R*H*W*Cin < 2^31.  kind: 0 forward, 1 dgrad, 2 wgrad.
 *
 * tdn_pack_deconv2x2_weight: w fp32 (Cin, Cout, 2, 2) with element strides (s_c, s_o, s_a, s_b) -> w_fwd [4*Cout][Cin],
 *   row (a*2+b)*Cout + o, and, unless NULL, w_dgrad [Cin][4*Cout]; each value rounded once to `dtype`.  One launch.
 * tdn_deconv2x2_fwd: y = act(x . w_fwd^T + bias) with the scatter in the epilogue; bias fp32 or NULL, act = ReLU if relu.
 *   Every element of y is written exactly once, nothing else is written.  One launch.
 * tdn_deconv2x2_dgrad: dx[r][i][j][c] = sum_{a,b,o} g[r][2i+a][2j+b][o] * W[c][o][a][b], rounded once to `dtype`.  The
 *   reduction runs over 4*Cout in 64-element chunks, each read from the output pixel of its tap.  g is taken as it is: a
 *   layer with a ReLU masks its cotangent first (tdn_linear_relu_bwd on the (R*2H*2W, Cout) matrix that y is in memory,
 *   or the mask_src of the next layer's tdn_linear_dgrad).  One launch.
 * tdn_deconv2x2_wgrad: dw[c][o][a][b] = beta * dw + sum_m x[m][c] * g[pix(m,a,b)][o] and dbias[o] = beta * dbias[o] + the
 *   sum of g[.][o] over all R*2H*2W pixels, in fp32; dw contiguous in the parameter's own (Cin, Cout, 2, 2) layout;
 *   dbias NULL: skipped.  beta == 0 never reads dw / dbias; R == 0 leaves beta * old.  The reduction over the pixels is
 *   cut into `slices` runs of whole 64-pixel chunks (splits: 0 lets the library choose — as tdn_linear_wgrad does: up to
 *   256 workgroups, at least 4 chunks per slice —, 1..ceil(M/64) forces a count; forward and dgrad are never cut and
 *   take splits 0 or 1 in the queries).  Every workgroup stores its fp32 partial slab into the workspace with plain
 *   stores; a finalize launch adds the slabs in slice order, the four taps' column sums in tap order, and writes dw and
 *   dbias: no atomics, no counters, no memset, the same bits on every run.  Two launches (one if R == 0).
 * tdn_deconv2x2_workspace_bytes: the workspace of that kind (forward / dgrad: 0; wgrad: slices * (4*Cout*Cin + 4*Cout)
 *   floats, each region from a 256-byte boundary), 256-byte aligned; -1 on a refused shape.
 * tdn_deconv2x2_plan (host only): out[0..15] = {BM, BN, BK, row tiles, column tiles, tiles, slices, chunks per slice,
 *   chunks, workgroups of the GEMM launch, launches, 0, slab bytes low 31 bits, slab bytes >> 31, workspace bytes low 31
 *   bits, workspace bytes >> 31}.  Rows x columns: forward M x 4*Cout, dgrad M x Cin, wgrad 4*Cout x Cin. */
int tdn_pack_deconv2x2_weight(const float* w, int64_t s_c, int64_t s_o, int64_t s_a, int64_t s_b, int Cin, int Cout,
                              void* w_fwd, void* w_dgrad, int dtype, void* stream);
int64_t tdn_deconv2x2_workspace_bytes(int kind, int R, int H, int W, int Cin, int Cout, int splits);
int tdn_deconv2x2_plan(int kind, int R, int H, int W, int Cin, int Cout, int splits, int32_t* out16);
int tdn_deconv2x2_fwd(const void* x, const void* w_fwd, const float* bias, void* y, int R, int H, int W, int Cin,
                      int Cout, int relu, int dtype, void* stream);
int tdn_deconv2x2_dgrad(const void* g, const void* w_dgrad, void* dx, int R, int H, int W, int Cin, int Cout, int dtype,
                        void* stream);
int tdn_deconv2x2_wgrad(const void* x, const void* g, float* dw, float* dbias, float beta, int R, int H, int W, int Cin,
                        int Cout, int splits, void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* ---- dense head predictors over a pyramid -----------------------------------------------------------------
 * The two 1x1 predictors of the RPN head (rpn_cls: A channels, rpn_reg: 4A channels; mmdetection-v1 RPNHead) on the
 * hidden maps of ALL pyramid levels in one launch per product: 16-bit operands, fp32 accumulation on the matrix cores,
 * one rounding of each result.  The weights are shared by the levels.  levels: HOST array of 1..TDN_PRED_MAX_LEVELS
 * entries.  h is the level's hidden map, NHWC memory seen as a dense (rows, C) matrix, 16-byte aligned; cls and reg are
 * dense (rows, A) and (rows, 4A) matrices of their own (2-byte aligned, nothing more): the outputs of the forward, the
 * cotangents of dgrad and wgrad; dh (dgrad only) is the dense (rows, C) gradient of h, 16-byte aligned.  rows in
 * 0..2^31-1 (row offsets are 64-bit); a level with rows == 0 is skipped and its pointers are not looked at.  C is a
 * multiple of 64 in 64..512, A is in 1..12.  The stacked weight has O = 5A rows, the A cls rows first; Op = O rounded up to
 * 16, Kp = O rounded up to 32.  kind: 0 forward, 1 dgrad, 2 wgrad.  With every rows == 0 nothing is launched but wgrad's
 * finalize, which writes zeros.
 *
 * tdn_pack_pred_weight: w_cls fp32 (A, C) and w_reg fp32 (4A, C) with element strides (s_o, s_c) each -> w_fwd [Op][C]
 *   and, unless NULL, w_dgrad [C][Kp]; each value rounded once to `dtype`, pad rows / columns zero.  One launch.
 * tdn_pred_fwd:   cls_l[m][a] = sum_c h_l[m][c] * w_cls[a][c] + bias_cls[a], reg_l[m][j] likewise with w_reg, bias_reg
 *   (fp32, not NULL).  Every element of cls_l and reg_l is written exactly once, nothing else is written.  One launch.
 * tdn_pred_dgrad: dh_l[m][c] = h_l[m][c] > 0 ? sum_a cls_l[m][a] * w_cls[a][c] + sum_j reg_l[m][j] * w_reg[j][c] : 0; both
 *   products are added in the fp32 accumulator, in the order of the stacked rows, and rounded once.  One launch.
 * tdn_pred_wgrad: dw_cls (A, C), dw_reg (4A, C), dbias_cls (A), dbias_reg (4A), contiguous fp32, none NULL:
 *   dw[o][c] = sum over all levels and rows of g_l[m][o] * h_l[m][c], dbias[o] = sum of g_l[m][o].  The rows are cut into
 *   slices of slice_rows rows — ceil(total rows / 64) rounded up to whole 128-row steps, a function of the shapes alone
 *   —, each level on its own, the slice list being the levels' slices in level order.  Every workgroup (slice x
 *   64-channel tile) stores an fp32 partial slab into the workspace with plain stores; the finalize launch adds the slabs
 *   in slice order: no atomics, no counters, no memset, the same bits on every run and on every device.
 * tdn_pred_workspace_bytes: forward / dgrad 0; wgrad slices * (Op * C + Op) floats, each region from a 256-byte boundary;
 *   256-byte aligned; -1 on a refused shape.  rows: HOST array of num_levels row counts.
 * tdn_pred_plan (host only): out[0..15] = {rows per workgroup (forward / dgrad) = rows per wgrad step, workgroups of the
 *   main launch, slices, rows per slice, launches, Op, Kp, channel tiles, LDS bytes, 0, 0, 0, slab bytes low 31 bits,
 *   slab bytes >> 31, workspace bytes low 31 bits, workspace bytes >> 31}. */
#define TDN_PRED_MAX_LEVELS 8
typedef struct tdn_pred_level {
  const void* h;
  void* cls;
  void* reg;
  void* dh;
  int64_t rows;
} tdn_pred_level;
int tdn_pack_pred_weight(const float* w_cls, int64_t c_so, int64_t c_sc, const float* w_reg, int64_t r_so, int64_t r_sc,
                         int A, int C, void* w_fwd, void* w_dgrad, int dtype, void* stream);
int64_t tdn_pred_workspace_bytes(int kind, const int64_t* rows, int num_levels, int C, int A);
int tdn_pred_plan(int kind, const int64_t* rows, int num_levels, int C, int A, int32_t* out16);
int tdn_pred_fwd(const tdn_pred_level* levels, int num_levels, const void* w_fwd, const float* bias_cls,
                 const float* bias_reg, int C, int A, int dtype, void* stream);
int tdn_pred_dgrad(const tdn_pred_level* levels, int num_levels, const void* w_dgrad, int C, int A, int dtype,
                   void* stream);
int tdn_pred_wgrad(const tdn_pred_level* levels, int num_levels, float* dw_cls, float* dbias_cls, float* dw_reg,
                   float* dbias_reg, int C, int A, void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* ---- 3x3 conv with shared weights over a pyramid, ragged Cout ---------------------------------------------
 * The tower layers and the two predictors of a single-stage head (mmdetection-v1 RetinaHead: retina_cls has A * C, retina_reg
 * 4A output channels) on ALL pyramid levels in one launch per product: 3x3, stride 1, pad 1, 16-bit operands, fp32
 * accumulation on the matrix cores, one rounding of each result.  levels: HOST array of 1..TDN_PYR_MAX_LEVELS entries of
 * one batch size B (>= 0) and a map size (H, W) each.  x is the level's input, dense NHWC (B, H, W, Cin), 16-byte aligned;
 * y is the dense NHWC (B, H, W, Cout) map — the output of the forward, the cotangent of dgrad and wgrad — whose rows are
 * 2 * Cout bytes: 2-byte aligned, nothing more; dx (dgrad only) is the dense (B, H, W, Cin) gradient of x, mask_src and
 * addend (dgrad only, each may be NULL) have dx's shape; the three are 16-byte aligned.  Cin is a multiple of 64 in
 * 64..512, Cout is ANY integer in 1..1024, B * H * W < 2^31 per level (pixel offsets are 64-bit).  A level with
 * B * H * W == 0 is skipped and its pointers are not looked at.  A tap outside the map contributes zero and is not read:
 * no launch reads a neighbouring image, a neighbouring level or memory outside a map.  kind: 0 forward, 1 dgrad, 2 wgrad.
 * Cp = Cout rounded up to 64, the column granularity of the kernels.
 *
 * tdn_pack_pyr_weight: w fp32 (Cout, Cin, 3, 3) with element strides (s_o, s_c, s_h, s_w) ->
 *   w_fwd [Cp][9][Cin], w_fwd[o][3 kh + kw][c] = w[o][c][kh][kw], and, unless NULL,
 *   w_dgrad [Cin][9][Cp], w_dgrad[c][3 th + tw][o] = w[o][c][2 - th][2 - tw];
 *   each value rounded once to `dtype`, rows / columns o >= Cout zero.  One launch.
 * tdn_pyr_conv_fwd: y_l[b][h][w][o] = relu?(sum_{kh,kw,c} x_l[b][h + kh - 1][w + kw - 1][c] * w[o][c][kh][kw] + bias[o]);
 *   bias fp32 (Cout) or NULL, added to the fp32 sum before the rounding.  Every element of y_l is written exactly once,
 *   with 16-, 8- or 2-byte stores as its address allows; nothing else is written.  One launch.
 * tdn_pyr_conv_dgrad: dx_l = sum_{kh,kw,o} y_l[b][h - kh + 1][w - kw + 1][o] * w[o][c][kh][kw] (+ addend_l, in fp32 before
 *   the rounding), then exactly 0 where mask_src_l <= 0.  The cotangent is read where it lies; the reduction over Cout is
 *   padded to Cp with zero weight columns and zero operand registers.  One launch.
 * tdn_pyr_conv_wgrad: dw fp32 written through the element strides (s_o, s_c, s_h, s_w) — the parameter's own layout —,
 *   dbias fp32 (Cout), neither NULL: dw[o][c][kh][kw] = sum over levels and pixels of y_l[b][h][w][o] *
 *   x_l[b][h + kh - 1][w + kw - 1][c], dbias[o] = sum of y_l[b][h][w][o].  The pixels are cut into slices of slice_rows
 *   pixels, each level on its own, the slice list being the levels' slices in level order; slice_rows =
 *   ceil(total pixels / S) rounded up to whole 128-pixel steps, S = min(64, ceil(1024 / units)), units = (Cp / 64) * 9 *
 *   (Cin / 64): a function of the shapes alone.  Every workgroup (slice x unit) stores an fp32 partial slab into the
 *   workspace with plain stores; the finalize launch adds the slabs in slice order: no atomics, no counters, no memset,
 *   the same bits on every run and on every device.  With no pixels at all only the finalize runs and writes zeros.
 * tdn_pyr_workspace_bytes: forward / dgrad 0; wgrad slices * (Cp * 9 * Cin + Cp) floats, each of the two regions from a
 *   256-byte boundary; the workspace is 256-byte aligned; -1 on a refused shape.  hw: HOST int32 [num_levels][2] = (H, W).
 * tdn_pyr_plan (host only): out[0..15] = {pixels per workgroup (forward / dgrad) = pixels per wgrad step, workgroups of the
 *   main launch, slices, pixels per slice, launches, columns per workgroup (64), Cp, padded reduction length per tap,
 *   LDS bytes, column tiles (forward / dgrad) or units per slice (wgrad), pixel tiles, 0, slab bytes low 31 bits, slab
 *   bytes >> 31, workspace bytes low 31 bits, workspace bytes >> 31}. */
#define TDN_PYR_MAX_LEVELS 8
typedef struct tdn_pyr_level {
  const void* x;
  void* y;
  void* dx;
  const void* mask_src;
  const void* addend;
  int32_t H;
  int32_t W;
} tdn_pyr_level;
int tdn_pack_pyr_weight(const float* w, int64_t s_o, int64_t s_c, int64_t s_h, int64_t s_w, int Cout, int Cin,
                        void* w_fwd, void* w_dgrad, int dtype, void* stream);
int64_t tdn_pyr_workspace_bytes(int kind, int B, const int32_t* hw, int num_levels, int Cin, int Cout);
int tdn_pyr_plan(int kind, int B, const int32_t* hw, int num_levels, int Cin, int Cout, int32_t* out16);
int tdn_pyr_conv_fwd(const tdn_pyr_level* levels, int num_levels, int B, const void* w_fwd, const float* bias, int Cin,
                     int Cout, int relu, int dtype, void* stream);
int tdn_pyr_conv_dgrad(const tdn_pyr_level* levels, int num_levels, int B, const void* w_dgrad, int Cin, int Cout,
                       int dtype, void* stream);
int tdn_pyr_conv_wgrad(const tdn_pyr_level* levels, int num_levels, int B, float* dw, int64_t s_o, int64_t s_c,
                       int64_t s_h, int64_t s_w, float* dbias, int Cin, int Cout, void* workspace,
                       int64_t workspace_bytes, int dtype, void* stream);

/* ---- GroupNorm (+ ReLU) with shared affine parameters over a pyramid ---------------------------------------
 * The conv -> GroupNorm -> ReLU tower layers of a single-stage head with norm_cfg GN (mmdetection-v1 FCOSHead) on ALL
 * pyramid levels: three launches forward and three backward for the whole pyramid.  levels: HOST array of
 * 1..TDN_PYR_MAX_LEVELS entries of one batch size B (>= 0) and a map size (H, W) each, H, W >= 0.  All maps are dense NHWC
 * (B, H, W, C), 16-bit, 16-byte aligned: z the raw conv output, y the output of the forward and the ReLU mask source of
 * the backward (may be NULL there when relu == 0), g = dL/dy UNMASKED, dz = dL/dz.  A level with B * H * W == 0 is skipped
 * and its pointers are not looked at.  C is 64, 128, 256 or 512, G divides C, at most 256 channels per group;
 * B * H * W < 2^31 per level (offsets are 64-bit), B <= 8191.  gamma, beta fp32 (C), shared by every level.  Statistics are
 * per (level, image, group), biased variance; they are formed as in tdn_gn_fwd: fp32 sums about the pivot K_c = the
 * channel's value at pixel 0 of the (level, image), pivots put back in double, y = (z - K) a + b' with b' formed in double.
 * relu is 0 or 1.  kind: 0 forward, 1 backward.
 *
 * tdn_pyr_gn_fwd: y_l = relu?((z_l - mu) rstd gamma + beta); stats fp32 [level][B][C][2] = (mu, rstd) of the channel's
 *   group, kept for the backward; the rows of a skipped level are zero (with no pixels at all nothing is launched).
 * tdn_pyr_gn_bwd: with g'_l = g_l where y_l > 0 (or everywhere when relu == 0) and exactly 0 elsewhere, and
 *   xhat = (z - mu) rstd: dz_l = rstd (gamma g' - mean_group(gamma g') - xhat mean_group(gamma g' xhat)), rounded once;
 *   dgamma[c] = sum over ALL levels, images and pixels of g' xhat, dbeta[c] = sum of g', fp32 (C), 16-byte alignment not
 *   needed; acc = 0 overwrites them, else they become acc * old + sum.  stats must be 16-byte aligned.  With no pixels at
 *   all one launch writes the (zero) sums.
 * The pixels of a (level, image) are cut into chunks by tdn_gn_fwd's rule applied to that level alone — min(ceil(1024 / B),
 * ceil(H W / (4 * pixel lanes))) chunks, pixel lanes = 2048 / C —, a function of (B, H W, C): a level gives the same bits
 * alone and inside a pyramid.  Partials are plain stores into the workspace and every reduction runs in a fixed order (chunk
 * order within an image; images within a level, levels finest first for dgamma / dbeta): no atomics, no counters, no
 * memset, the same bits on every run.
 * tdn_pyr_gn_workspace_bytes: part [workgroup][2][C] | coef [level][B][3][C] | backward: sums [level][B][2][C], fp32, each
 *   region from a 256-byte boundary; the workspace is 256-byte aligned; 0 with no pixels; -1 on a refused shape.
 *   hw: HOST int32 [num_levels][2] = (H, W).
 * tdn_pyr_gn_plan (host only): out32[0..7] chunks per image of each level (0: skipped), out32[8..15] pixels per chunk,
 *   out32[16..18] workgroups of the three launches, out32[19] launches, out32[20] 16-byte lanes per workgroup of the third
 *   launch, out32[21] channels per block of the second, out32[22] workspace bytes low 31 bits, out32[23] workspace bytes
 *   >> 31, the rest 0. */
typedef struct tdn_pyr_gn_level {
  const void* z;
  void* y;
  const void* g;
  void* dz;
  int32_t H;
  int32_t W;
} tdn_pyr_gn_level;
int64_t tdn_pyr_gn_workspace_bytes(int kind, int B, const int32_t* hw, int num_levels, int C, int G);
int tdn_pyr_gn_plan(int kind, int B, const int32_t* hw, int num_levels, int C, int G, int32_t* out32);
int tdn_pyr_gn_fwd(const tdn_pyr_gn_level* levels, int num_levels, int B, const float* gamma, const float* beta, int C,
                   int G, float eps, int relu, float* stats, void* workspace, int64_t workspace_bytes, int dtype,
                   void* stream);
int tdn_pyr_gn_bwd(const tdn_pyr_gn_level* levels, int num_levels, int B, const float* stats, const float* gamma, int C,
                   int G, int relu, float* dgamma, float* dbeta, float acc, void* workspace, int64_t workspace_bytes,
                   int dtype, void* stream);

/* ---- Balanced Feature Pyramid, Libra R-CNN's BFP neck (csrc/bfp.hip) ------------------------------------------
 * levels: HOST array of 1..TDN_PYR_MAX_LEVELS entries of one batch size B (1..64), one channel count C (a multiple of 8 in
 * 8..1024) and a map size (H, W) each, 1 <= H, W <= 32767 and B H W C < 2^31, in ANY relation to one another.  All maps
 * are dense NHWC (B, H, W, C), 16-bit, 16-byte aligned, finite.  (Hg, Wg) is the size of level refine_level; bsf and dbsf
 * are (B, Hg, Wg, C).  An axis map sends destination index d to a window [lo, hi) of n_src source indices:
 *   pool     lo = floor(d n_src / n_dst), hi = ceil((d + 1) n_src / n_dst)   (adaptive_max_pool2d; windows may overlap)
 *   nearest  lo = min((int)floorf((float)d * ((float)n_src / (float)n_dst)), n_src - 1), hi = lo + 1, fp32 (interpolate)
 * and a destination element is the FIRST maximum of its 2-D window in row-major order.  M_l (level -> refine grid) is the
 * pool for l < refine_level and nearest otherwise; N_l (refine grid -> level) is nearest for l < refine_level and the pool
 * otherwise.  Sums are fp32, in the order written, starting from +0; every result is rounded once to the dtype.
 *   tdn_bfp_gather_fwd:  reads x.   bsf[q] = (M_0(x_0)[q] + M_1(x_1)[q] + ...) / L, one fp32 division.
 *   tdn_bfp_scatter_fwd: reads x, writes out.   out_l[p] = N_l(bsf)[p] + x_l[p]   (bsf: the refined map).
 *   tdn_bfp_scatter_bwd: reads g.   dbsf[q] = s_0 + s_1 + ..., s_l = the sum, in row-major order of p, of g_l[p] over the
 *                        p whose window under N_l contains q and has its first maximum, recomputed from bsf, at q.
 *   tdn_bfp_gather_bwd:  reads x, g, writes dx.   dx_l[p] = g_l[p] + s / L, s = the sum, in row-major order of q, of
 *                        dbsf[q] over the q whose window under M_l contains p and has its first maximum, recomputed from
 *                        x_l, at p.
 * One launch each, no workspace, no atomics: every element is written once by one lane; the same bits on every run. */
typedef struct tdn_bfp_level {
  const void* x;
  void* out;
  const void* g;
  void* dx;
  int32_t H;
  int32_t W;
} tdn_bfp_level;
int tdn_bfp_gather_fwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C, void* bsf, int dtype,
                       void* stream);
int tdn_bfp_scatter_fwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C, const void* bsf,
                        int dtype, void* stream);
int tdn_bfp_scatter_bwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C, const void* bsf,
                        void* dbsf, int dtype, void* stream);
int tdn_bfp_gather_bwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C, const void* dbsf,
                       int dtype, void* stream);

/* ---- deformable convolution, DCN v1 / v2 (csrc/deform.hip) ---------------------------------------------
 * y = conv1x1(cols, W) with cols[n, ho, wo, k, c] the bilinear sample of x (N, H, W, C NHWC, 16-bit) at
 * (ho stride - pad + i pad + dy, wo stride - pad + j pad + dx), tap k = 3 i + j of a 3x3 kernel with dilation == pad,
 * (dy, dx) = offset channels 2 (g 9 + k), 2 (g 9 + k) + 1 of deformable group g = c / (C / deformable_groups), times the
 * mask channel g 9 + k when mask != NULL (mask_is_logit: times 1 / (1 + exp(-mask)), fp32).  offset (N, Ho, Wo, >= 18 dg)
 * and mask (N, Ho, Wo, >= 9 dg) are NHWC with offset_pitch / mask_pitch ELEMENTS between pixels, fp32 (TDN_F32) or the
 * compute dtype.  A sample is valid iff -1 < py < H and -1 < px < W, tested on the floats (NaN, inf: invalid); an invalid
 * sample is 0 and has zero gradients; a corner outside the map contributes exactly 0.  fp32 arithmetic in the order of
 * DESIGN.md §4p, one rounding to the compute dtype.  C a multiple of 64, (C / dg) a multiple of 8, stride 1 or 2, pad 1..32,
 * H, W <= 32766, N Ho Wo 9 dg < 2^30.
 *   tdn_deform_sample:      cols (N Ho Wo, 9 C) compute dtype, K index k C + c; 16-byte aligned.
 *   tdn_pack_deform_weight: fp32 (Cout, C, 3, 3) of any element strides -> w_fwd [Cout][9 C] (the 1x1 forward operand over
 *                           cols) and w_dgrad [9 C][Cout] (its tdn_conv2d_dgrad operand; may be NULL), one launch.
 *   tdn_deform_coord_grad:  doffset / dmask in the offset's / mask's own dtype and pitch from dcol (N Ho Wo, 9 C):
 *                           d dy = m sum_c dcol ((v3 - v1) hx + (v4 - v2) lx), d dx = m sum_c dcol ((v2 - v1) hy + (v4 - v3) ly),
 *                           d m = sum_c dcol val (times s (1 - s) = t / (1 + t)^2, t = exp(-|m|), for a logit), sums over the group's channels in fp32: each
 *                           of L = min(64, 2^ceil(log2(C / dg / 8))) lanes its 8-channel groups in order, then a fixed xor
 *                           tree.  Channels of a pixel past 18 dg / 9 dg are not written.
 *   tdn_deform_input_grad:  dx (N, H, W, C) compute dtype, every pixel written once: the fp32 sum of dcol m w_corner over
 *                           the valid samples' corners landing on it, in sample order ((ho, wo), g, k), rounded once.  Two
 *                           launches, no atomics: the same bits on every run.  x of the descriptor is not read.
 *   tdn_deform_workspace_bytes (host only): bytes of tdn_deform_input_grad's workspace (256-byte aligned): records
 *                           [N][chunks][256] of 16 bytes | boxes [N][chunks] of 16 bytes, chunks = ceil(Ho Wo dg 9 / 256),
 *                           each region from a 256-byte boundary; -1 on a refused shape. */
typedef struct tdn_deform_desc {
  const void* x;
  const void* offset;
  const void* mask;            /* NULL: DCN v1 */
  int64_t offset_pitch;
  int64_t mask_pitch;
  int32_t N, H, W, C;
  int32_t stride, pad, deformable_groups;
  int32_t dtype, offset_dtype, mask_dtype;
  int32_t mask_is_logit;
  int32_t reserved;
} tdn_deform_desc;
int64_t tdn_deform_workspace_bytes(int N, int H, int W, int stride, int pad, int deformable_groups);
int tdn_deform_sample(const tdn_deform_desc* d, void* cols, void* stream);
int tdn_pack_deform_weight(const float* w, int64_t s_o, int64_t s_i, int64_t s_h, int64_t s_w, int Cout, int C,
                           void* w_fwd, void* w_dgrad, int dtype, void* stream);
int tdn_deform_coord_grad(const tdn_deform_desc* d, const void* dcol, void* doffset, void* dmask, void* stream);
int tdn_deform_input_grad(const tdn_deform_desc* d, const void* dcol, void* dx, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* ---- CARAFE content-aware upsampling (csrc/carafe.hip) ------------------------------------------------
 * out[n, c, ph, pw] = sum over taps t = i k + j, in that order, of w[n, gi k^2 + t, ph, pw] * x[n, c, h - r + i, w - r + j],
 * h = ph / s, w = pw / s, gi = c / (C / g), r = (k - 1) / 2; a tap whose source pixel lies outside the map is skipped.
 * x (N, H, W, C), out / gout / addend (N, out_h, out_w, C) and dx are NHWC in the compute dtype (16-byte aligned).
 * `weights` is NHWC with weight_pitch ELEMENTS between pixels, fp32 (TDN_F32) or the compute dtype: the stored masks
 * (N, sH, sW, >= g k^2), or with weights_are_logits the content encoder's output (N, H, W, >= g k^2 s^2) whose channel
 * (gi k^2 + t) s^2 + dy s + dx is the logit of tap t at output pixel (s h + dy, s w + dx); the kernels then use
 * p_t = exp(l_t - max) / sum_u exp(l_u - max) (fp32, the sum in tap order).  (out_h, out_w) in (sH - s + 1 .. sH,
 * sW - s + 1 .. sW) crops the output top-left: only those pixels are computed, gout counts as zero outside.  fp32
 * accumulation, one rounding per output.  C a multiple of 64, C / g a multiple of 8, k odd in 1..7, s in 1..4,
 * g k^2 s^2 <= 1024, H, W <= 32766, N sH sW < 2^30.  No workspace, no atomics: the same bits on every run.
 *   tdn_carafe_forward:       out = addend (when non-NULL) + the sum above, one launch.
 *   tdn_carafe_feature_grad:  dx[n, c, h, w] = sum over the source pixels (h2, w2) of the window, row-major, and their s^2
 *                             sub-pixels, row-major, of gout * w; one thread per element, one launch.  x is not read.
 *   tdn_carafe_mask_grad:     dweights in the dtype, layout and pitch of `weights`: d mask[t] = sum over the group's
 *                             channels of gout * x (0 for a tap outside the map; each of L lanes its 8-channel vectors in
 *                             order, then a fixed xor tree); for logits p_t (dm_t - sum_u p_u dm_u).  Every channel of
 *                             every pixel below g k^2 (s^2) is written; one launch. */
typedef struct tdn_carafe_desc {
  const void* x;
  const void* weights;
  const void* addend;          /* forward only; may be NULL */
  int64_t weight_pitch;
  int32_t N, H, W, C;
  int32_t kernel_size, group_size, scale_factor;
  int32_t out_h, out_w;
  int32_t dtype, weight_dtype;
  int32_t weights_are_logits;
} tdn_carafe_desc;
int tdn_carafe_forward(const tdn_carafe_desc* d, void* out, void* stream);
int tdn_carafe_feature_grad(const tdn_carafe_desc* d, const void* gout, void* dx, void* stream);
int tdn_carafe_mask_grad(const tdn_carafe_desc* d, const void* gout, void* dweights, void* stream);

/* ---- GroupNorm ----------------------------------------------------
 * nn.GroupNorm(get_group_gn(planes), planes) — models/utils/layers.py:50-54,138-154 (32 groups, eps 1e-5, biased
 * variance) — after a conv of ResNet(use_gn=True) (models/backbone/resnet.py:42-59,97-119,254-257) or of a
 * ConvModule with GN (layers.py:122-135), fused with the residual add and ReLU that follow it.
 *   (relu: 0 none, 1 ReLU, 2 ReLU6 — as in the conv epilogue; the same for tdn_bn_train_fwd)
 *   tdn_gn_fwd: z (N,H,W,C) raw conv output -> y = relu?((z - mu) * rstd * gamma + beta (+ addend)); addend_mode
 *               TDN_ADD_SAME (same shape: the residual) or TDN_ADD_UP2X ((N,H/2,W/2,C): FPN top-down, fpn.py:98-100);
 *               stats (N,C,2) float = per-channel (mu, rstd) of the channel's group, kept for the backward.
 *   tdn_gn_bwd: g = dL/dy (already ReLU-masked) -> dz = dL/dz (16-bit, feeds tdn_conv2d_dgrad / _wgrad with no BN
 *               fold), dgamma, dbeta (float; acc = 1 accumulates into them, 0 overwrites).
 * C a power of two in 64..2048, G | C.  workspace: tdn_gn_workspace() bytes, 16-byte aligned. */
int64_t tdn_gn_workspace(int N, int H, int W, int C, int G);
int tdn_gn_fwd(const void* z, const float* gamma, const float* beta, int N, int H, int W, int C, int G, float eps,
               const void* addend, int addend_mode, int relu, void* y, float* stats, void* workspace,
               int64_t workspace_bytes,
               int dtype, void* stream);
int tdn_gn_bwd(const void* g, const void* z, const float* stats, const float* gamma, int N, int H, int W, int C,
               int G, void* dz, float* dgamma, float* dbeta, float acc, void* workspace, int64_t workspace_bytes,
               int dtype, void* stream);

/* ---- BatchNorm2d with batch statistics (training mode) ------------------------------------
 * nn.BatchNorm2d as norm_layer builds it (models/utils/layers.py:50-54) when the backbone is NOT told to keep BN in eval
 * mode — ResNet(bn_eval=False), models/backbone/resnet.py:270-276.  Same passes as GroupNorm with the statistics taken
 * per channel over (N, H, W); running_mean / running_var (may both be NULL) are updated in place:
 * r = (1 - momentum) r + momentum * batch value, unbiased variance.  stats (N,C,2) as in tdn_gn_fwd.
 * Workspace: tdn_gn_workspace(N, H, W, C, C). */
int tdn_bn_train_fwd(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, int N, int H, int W, int C, float eps, const void* addend, int addend_mode,
                     int relu, void* y, float* stats, void* workspace, int64_t workspace_bytes, int dtype,
                     void* stream);
int tdn_bn_train_bwd(const void* g, const void* z, const float* stats, const float* gamma, int N, int H, int W, int C,
                     void* dz, float* dgamma, float* dbeta, float acc, void* workspace, int64_t workspace_bytes,
                     int dtype, void* stream);

/* ---- image batch staging -------------------------------------------
 * One launch for what the reference does per image on the host and then in collate():
 *   img_normalize            datasets/utils/image.py:87-105     (img - mean) / std, float32
 *   img_flip (horizontal)    datasets/utils/image.py:220-249
 *   img_pad_size_divisor     datasets/utils/image.py:300-347    zero pad bottom/right
 *   HWC -> CHW               datasets/dataset_transforms.py:44
 *   collate (stack, pad 0)   datasets/loader/collate.py:42-63   pad every sample to the batch maximum
 * imgs: HOST array of N device pointers to H_i x W_i x 3 pixels (src_kind 0 = uint8, 1 = float32), already resized;
 * hw: HOST int32 [N][2] = (H_i, W_i); flip: HOST [N] flags or NULL; mean3 / std3: HOST float[3], in the images'
 * channel order.  Hb x Wb = batch size (>= every image, normally rounded up to the size divisor by the caller).
 * out_kind 0: float32 (N, 3, Hb, Wb), bit-identical to the reference chain (two IEEE operations per element).
 * out_kind 1: the stem's staged input (N, Hb+6, Wb+8, 4) in `dtype` — exactly tdn_stage_image of the out_kind-0
 *             batch, without the float32 round trip.  N <= TDN_COLLATE_MAX per call. */
#define TDN_COLLATE_MAX 16
int tdn_collate_images(const void* const* imgs, const int32_t* hw, const uint8_t* flip, int N, int src_kind,
                       const float* mean3, const float* std3, int Hb, int Wb, void* out, int out_kind, int dtype,
                       void* stream);

/* ---- host-only introspection (no GPU needed; used by CPU tests) --------------------- */

/* Describes the GEMM decomposition the library would launch for a conv: fills out[0..15] with
 * {M, Ngemm, Kgemm, BM, BN, BK, grid_x, grid_y, grid_z, nclasses, ntaps(class0), 1 (GEMM route), ...}.
 * kind: 0 = fwd, 1 = dgrad, 2 = wgrad.  A shape taken by the LDS-resident patch kernel (csrc/conv_halo.hip: 3x3
 * stride-1 convs) reports grid_z = 100 + its configuration id, out[11] = patch rows * 1000 + patch columns and
 * out[12] = chunk images held in LDS * 100 + output-channel passes per workgroup. */
int tdn_conv2d_plan(int kind, int N, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                    int32_t* out16);

#ifdef __cplusplus
}
#endif
#endif /* TDN_H_ */
