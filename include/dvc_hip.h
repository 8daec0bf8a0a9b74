/*
 * dvc_hip.h — C-ABI of libdvc_hip.so: hand-written gfx950 (MI355X / CDNA4) HIP kernels for the
 * inference hot path of Deep-Exemplar-based-Video-Colorization
 *   VGG19 features -> WarpNet dense exemplar<->frame correlation -> ColorVidNet generator.
 *
 * The reference (/root/reference) has NO native / FFI layer: every op on this path is a stock ATen
 * op reached through torch.nn.  The drop-in boundary is therefore the Python module
 * surface that /root/reference/test.py:17-19 imports; this header is the thin native layer underneath
 * it, and each entry point cites the reference call site(s) whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C: raw device pointers (fp32, NCHW, contiguous unless a batch stride is given), sizes,
 *     and a hipStream_t passed as void*.  No torch types.  No allocation, no synchronisation: every
 *     call only enqueues kernels on `stream` (so a caller may capture calls into a hipGraph).
 *   - return 0 on success; non-zero on error, with a message retrievable via dvc_last_error().
 *   - scratch memory is supplied by the caller (sizes via the *_workspace_bytes helpers).
 */
#ifndef DVC_HIP_H
#define DVC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported. */
#pragma GCC visibility push(default)

typedef void* dvcStream; /* hipStream_t */

#define DVC_ABI_VERSION 20

int dvc_abi_version(void);
/* Thread-local description of the last failure (empty string if none). */
const char* dvc_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Convolution engine: im2col-free implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).
 * Replaces every nn.Conv2d (+ the padding / upsample / norm / activation modules wrapped around it):
 *   VGG19_pytorch.forward            models/NonlocalNet.py:235-254  (conv3x3 p1 + ReLU)
 *   WarpNet heads / ResidualBlock    models/NonlocalNet.py:364-410, 341-352
 *                                    (ReflectionPad2d + conv3x3 s1/s2; IN+PReLU folded into the
 *                                     consumer's load; Upsample folded into the index map)
 *   WarpNet.theta / .phi             models/NonlocalNet.py:418-423  (1x1)
 *   ColorVidNet.forward              models/ColorVidNet.py:98-141   (conv3x3 d1/d2, InstanceNorm and
 *                                     the depthwise stride-2 `*_ss` scale folded into the load,
 *                                     nearest-up folded into the index map, skip-add + ReLU epilogue)
 *
 * y[n,co,oy,ox] = act( bias[co] + residual[n,co,oy,ox]
 *                      + sum_{ci,ky,kx} w[co,ci,ky,kx] * T(x)[n,ci, oy*stride+ky*dil-pad, ox*stride+kx*dil-pad] )
 * where T(x) is the *virtual* input: the stored tensor x[N,Cin,H,W], optionally subsampled
 * (x[:, :, ::2, ::2]) or nearest-upsampled x2, with the per-(n,ci) affine v*in_scale+in_shift and an
 * optional PReLU applied to in-bounds values; out-of-bounds taps read 0 (zero pad) or the mirrored
 * position (reflect pad, applied in the virtual domain exactly like ReflectionPad2d after Upsample).
 *
 * Weights are pre-packed as w_packed[ci][ky*ks+kx][co] (co contiguous), Cout % 4 == 0.
 *
 * Layers too small to fill the 1024 SIMDs are split over input-channel chunks (split-K): partial sums
 * go to `workspace` ([S][N][Cout][OH][OW] floats) and a second tiny kernel adds them in a fixed order and
 * applies bias / residual / activation.  Without a workspace split-K is off.
 * Alternatively (cfg 32 + k) the layer is decomposed stream-K style: the (tile, channel-chunk) units are dealt in
 * equal contiguous ranges to a grid that exactly fills the chip; tiles that a range boundary splits go through
 * per-workgroup slots in `workspace` and a fixed-order fixup kernel (csrc/conv_sk_kernel.h).
 */
enum { DVC_ACT_NONE = 0, DVC_ACT_RELU = 1, DVC_ACT_PRELU = 2, DVC_ACT_LEAKY = 3, DVC_ACT_TANH128 = 4 };
enum { DVC_PAD_ZERO = 0, DVC_PAD_REFLECT = 1 };

typedef struct DvcConvDesc {
    int32_t N, Cin, H, W;       /* stored input tensor */
    int32_t Cout;
    int32_t ksize;              /* 1 or 3 (4: dvc_gan_conv4s2 / _dgrad only) */
    int32_t stride;             /* 1 or 2 */
    int32_t dil;                /* 1 or 2 */
    int32_t pad;                /* 0..2 */
    int32_t pad_mode;           /* DVC_PAD_* */
    int32_t in_up;              /* 1 | 2 : nearest upsample of the stored input */
    int32_t in_sub;             /* 1 | 2 : keep every 2nd row/col of the stored input */
    int32_t act;                /* DVC_ACT_* */
    float   act_slope;          /* PReLU/LeakyReLU slope when act_slope_ptr == NULL */
    int32_t in_prelu;           /* apply PReLU (slope *in_slope_ptr) to the affine-transformed input */
    int32_t cfg;                /* tile configuration 0..4; -1 = choose automatically; 16 + k = configuration k
                                   with register staging forced (layers without a fused input transform
                                   otherwise stage through LDS-DMA); 32 + k (k = 2, 3, 4) = stream-K decomposition
                                   of a plain stride-1 layer with tile configuration k (needs a workspace) */
    int32_t split_k;            /* 0 = automatic, 1 = off, 2..8 = forced (needs a workspace); with cfg >= 32:
                                   workgroups per CU (0 -> 2) */
    int64_t x_batch_stride;     /* elements; 0 => Cin*H*W */
    int64_t y_batch_stride;     /* elements; 0 => Cout*OH*OW  (lets y be a channel slice) */
    int64_t res_batch_stride;   /* elements; 0 => Cout*OH*OW */
    int32_t flags;              /* DVC_CONV_* bits (0 = none) */
    int64_t w_batch_stride;     /* dvc_conv2d only, elements; 0 => the N images share one filter set (a convolution); != 0 =>
                                   image n uses w_packed + n * w_batch_stride: with ksize 1 that is a BATCHED GEMM
                                   y[n] = w[n]^T x[n] (K = Cin, M = Cout, N = H*W) — the N x N affinity products of the
                                   training-side callers (models/ContextualLoss.py:97-126, train.py:402-427), one launch for
                                   the whole batch.  Multiple of 4 (16-byte aligned slices); general engine only (cfg < 32) */
} DvcConvDesc;
/* dvc_conv2d_winograd only: when the layer is split over input channels (dvc_conv2d_winograd_split > 1), leave the partial
 * sums [split][N][Cout][OH*OW] in the workspace instead of launching the reduce — bias, activation and `y` are then NOT applied /
 * written; the consumer sums them (dvc_instnorm_apply_partials).  No effect when the layer is not split. */
#define DVC_CONV_DEFER_REDUCE 1
/* dvc_conv2d_winograd / _pool / _dual / _split: plan the launch for the WHOLE batch (workgroups of all N images fill the chip
 * together, so layers that would be split over input channels for one image need a smaller split or none) instead of per
 * image.  Default (bit clear): the plan is that of a single image and a batch of N is bit-identical to N single-image calls
 * (train.py:402 calls the path with B = 16).  With the bit set the result is deterministic per (layer, N) but the fp32
 * summation order over input channels — hence the last-place rounding — depends on N.  Used where N images MUST run together
 * anyway: the R references of one clip (/root/reference/test.py:169-181), whose ColorVidNet recurrences advance in lock step. */
#define DVC_CONV_BATCH_PLAN 2
/* dvc_conv2d, the 3 -> 64 image-input layer only (VGG19 conv1_1): the stored input is ONE plane per image — the centred
 * luminance L, x_batch_stride elements apart (0 => H*W) — and every one of the three virtual input channels reads
 * (L + 50) / 100, i.e. gray2rgb_batch(uncenter_l(L)) (utils/util.py:63-64,97-101, FrameColor.py:9) folded into the load:
 * bit-identical to dvc_gray2rgb followed by the plain call, one launch and a 1 MB tensor less per frame.  The input affine
 * (vgg_preprocess) applies to that value as usual. */
#define DVC_CONV_GRAY_INPUT 4

/* Output spatial size implied by a descriptor. */
int dvc_conv2d_out_hw(const DvcConvDesc* d, int32_t* OH, int32_t* OW);

int dvc_conv2d(const DvcConvDesc* d,
               const float* x, const float* w_packed, const float* bias /* may be NULL */,
               const float* in_scale /* [N*Cin] or NULL */, const float* in_shift /* [N*Cin] or NULL */,
               const float* in_slope_ptr /* device scalar, used when in_prelu */,
               const float* act_slope_ptr /* device scalar or NULL */,
               const float* residual /* or NULL */, float* y,
               void* workspace /* or NULL: scratch for split-K partial sums */, size_t workspace_bytes,
               dvcStream stream);

/* The same 3x3 convolution (every 3x3 stride-1 nn.Conv2d of models/ColorVidNet.py:14-81, models/NonlocalNet.py:200-215,
 * 330-339, 359-420 whose input needs no fused per-element transform) in Winograd F(2x2,3x3) form: 2.25x fewer
 * multiplies, fp32 throughout, result within fp32 rounding of the direct sum (what cuDNN selects for these layers under
 * the reference's cudnn.benchmark = True, test.py:140).  Requirements: ksize 3, stride 1, dil 1|2 with pad == dil,
 * Cin % 8 == 0, Cout % 64 == 0, in_prelu == 0.  Descriptor fields as for dvc_conv2d except
 *   cfg      -1 = automatic | tile-block shape (0: 1x32, 1: 2x16, 2: 4x8, 3: 8x4 tiles) + 4 * workgroup shape
 *            (0: 128 channels x 32 tiles, 1: 64 channels x 64 tiles — 8 waves, one workgroup per CU; 2: 64 channels x
 *            32 tiles — 4 waves and 64 KB of LDS, two workgroups per CU)
 *   split_k  0 = automatic | 1..8 = split over input-channel chunks (needs the workspace, as dvc_conv2d)
 * u_packed: the filters in the transform domain, U = G g G^T, laid out [Cout/32][Cin][4][32][4]
 * (dvc_winograd_weight_floats(Cout, Cin) floats, written by dvc_winograd_pack_weight). */
size_t dvc_winograd_weight_floats(int32_t Cout, int32_t Cin);
/* w: [Cout][Cin][3][3] (the nn.Conv2d weight as stored in the reference's checkpoints) -> u_packed, evaluated in double
 * and rounded once.  Cout % 32 == 0. */
int dvc_winograd_pack_weight(const float* w, int32_t Cout, int32_t Cin, float* u_packed, dvcStream stream);
/* the split over input channels dvc_conv2d_winograd uses for this descriptor and workspace size (1 = none) and the number of
 * images one launch of it covers (workspace capacity at that split, 65535-workgroup cap); a pure function.  A caller that
 * wants DVC_CONV_DEFER_REDUCE must check images_per_launch >= d->N first. */
int dvc_conv2d_winograd_split(const DvcConvDesc* d, size_t workspace_bytes, int32_t* split, int32_t* images_per_launch);
int dvc_conv2d_winograd(const DvcConvDesc* d, const float* x, const float* u_packed,
                        const float* bias /* may be NULL */, const float* act_slope_ptr /* device scalar or NULL */,
                        const float* residual /* or NULL */, float* y,
                        void* workspace /* or NULL */, size_t workspace_bytes, dvcStream stream);
/* dvc_conv2d_winograd with nn.MaxPool2d(2, 2) of the activated output fused (VGG19: relu1_2 -> pool, relu2_2 -> pool, relu3_4 ->
 * pool, relu4_4 -> pool, /root/reference/models/NonlocalNet.py:240-254): y_pool [N][Cout][OH/2][OW/2] (floor mode;
 * pool_batch_stride in elements, 0 = dense) is written by the convolution's epilogue — a lane's 2x2 Winograd output tile is a
 * pooling window — or, when the layer is split over its input channels, by the reduce kernel.  y may be NULL when only the pooled
 * tensor is wanted.  Both outputs are bit-identical to dvc_conv2d_winograd followed by dvc_maxpool2x2.  Dilation 1, no residual. */
int dvc_conv2d_winograd_pool(const DvcConvDesc* d, const float* x, const float* u_packed, const float* bias /* may be NULL */,
                             const float* act_slope_ptr /* device scalar or NULL */, float* y /* or NULL */, float* y_pool,
                             int64_t pool_batch_stride, void* workspace /* or NULL */, size_t workspace_bytes, dvcStream stream);
/* TWO 3x3 convolutions whose outputs are added, as ONE launch: y = act(conv(T_A(xA), W_A) + conv(T_B(xB), W_B) + bias).
 * ColorVidNet.py:124-139 adds a skip convolution to the first convolution of every decoder block
 * (conv8_1(up(norm(c7_3))) + conv3_3_short(norm(c3_3)), likewise conv9_1 / conv10_1): the reduction simply runs over the
 * channels of both inputs, each with its own index map (dA / dB: Cin, H, W, in_up, in_sub; batch, Cout, dilation, padding
 * mode, activation and output geometry from dA and equal in dB), so the pair costs one set of per-launch / per-workgroup
 * fixed costs, one pass over the output and no residual read.  u_packed_cat: the two packed filter sets concatenated along
 * the input-channel axis ([Cout/32][CinA + CinB][4][32][4]); bias: the SUM of the two biases (or NULL).  Cin % 8 == 0 for
 * both, Cout % 64 == 0.  Rounding differs from the two-launch form only by the order of the fp32 accumulation. */
int dvc_conv2d_winograd_dual(const DvcConvDesc* dA, const DvcConvDesc* dB, const float* xA, const float* xB,
                             const float* u_packed_cat, const float* bias /* may be NULL */,
                             const float* act_slope_ptr /* device scalar or NULL */, float* y,
                             void* workspace /* or NULL */, size_t workspace_bytes, dvcStream stream);

/* r06 — weights-in-registers direct convolution (csrc/conv_ws.hip) for the large-map, few-channel 3x3 layers of ColorVidNet's
 * encoder (models/ColorVidNet.py:98-103: conv1_1[2] 32 -> 64 and conv1_2 64 -> 64 at full frame size, conv2_1 64 -> 128 at half
 * size): same arithmetic class as dvc_conv2d (exact fp32 products, blocked fp32 accumulation: chains of 8 channels x 9 taps
 * added to a running total), another decomposition — a wave keeps its 32 x 32 x 9 filter block in 144 VGPRs for the whole
 * launch and walks down a 32-pixel column strip whose input rows stream through an LDS ring.
 * Eligible (dvc_conv2d_ws_eligible != 0): ksize 3, stride 1, dil 1, pad 1, zero padding, no up / sub-sampling, no fused input
 * transform, Cin 32, 64 or 128, Cout % 64 == 0, act NONE / RELU / PRELU / LEAKY; no residual.  `u_packed`: Cout * Cin * 9 floats
 * written by dvc_conv2d_ws_pack_weight from the module's [Cout][Cin][3][3] weight (fragment order, 16-byte aligned).
 * x_batch_stride / y_batch_stride of the descriptor are honoured; cfg / split_k / flags are ignored (one plan per geometry,
 * per image: a batch of N is bit-identical to N calls). */
int dvc_conv2d_ws_eligible(const DvcConvDesc* d);
int dvc_conv2d_ws_pack_weight(const float* w, int32_t Cout, int32_t Cin, float* u_packed, dvcStream stream);
int dvc_conv2d_ws(const DvcConvDesc* d, const float* x, const float* u_packed, const float* bias /* may be NULL */,
                  const float* act_slope_ptr /* may be NULL */, float* y, dvcStream stream);

/* r06 — several INDEPENDENT 3x3 layers in ONE launch: the first (and the second) convolutions of WarpNet's four heads
 * (models/NonlocalNet.py:364-410; NonlocalNet.py:451-458 runs the heads on four different VGG taps, nothing connects them).
 * Item i is exactly dvc_conv2d_winograd(&d, x, u_packed, bias, act_slope_ptr, residual, y, workspace, workspace_bytes): the
 * same plan, the same kernel body, the same (deferred or launched) split-K reduce — results are bit-identical to the per-item
 * calls.  The items' workgroups form one grid when every item gets the 64-channel x 32-tile workgroup shape and a single
 * launch (every head layer at the path's sizes does); otherwise the call degrades to one launch per item.  The items must not
 * depend on each other; outputs and workspaces must be disjoint.  1 .. 4 items. */
typedef struct DvcConvGroupItem {
    DvcConvDesc d;
    const float* x;
    const float* u_packed;
    const float* bias;            /* or NULL */
    const float* act_slope_ptr;   /* or NULL */
    const float* residual;        /* or NULL */
    float* y;
    void* workspace;              /* this item's own split-K scratch (may be NULL: no split) */
    size_t workspace_bytes;
} DvcConvGroupItem;
int dvc_conv2d_winograd_group(const DvcConvGroupItem* items, int32_t n_items, dvcStream stream);

/* conv 1x1 with tiny Cout (<= 4) + optional tanh*128: ColorVidNet.conv10_ab, ColorVidNet.py:142-144.
 * w is the unpacked [Cout][Cin] matrix. */
int dvc_conv1x1_small(const float* x, const float* w, const float* bias, int32_t N, int32_t Cin,
                      int32_t HW, int32_t Cout, int32_t act, float* y, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * InstanceNorm2d (eps, no affine, biased variance), split as "statistics" + "apply":
 *   models/NonlocalNet.py:335,339,368,...   models/ColorVidNet.py:85-94
 * stats: for every plane p=(n,c) of HW elements computes mean/var (fp64 accumulation, like ATen's CPU
 *   batch-norm statistics) and writes scale[p] = rstd * (chan_scale ? chan_scale[c] : 1),
 *   shift[p] = -mean * scale[p].  chan_scale carries the depthwise `*_ss` weights (ColorVidNet.py:12).
 */
int dvc_instnorm_stats(const float* x, int32_t N, int32_t C, int32_t HW, int64_t x_batch_stride,
                       float eps, const float* chan_scale, float* scale, float* shift,
                       dvcStream stream);

/* apply: y = prelu_or_id( x*scale + shift + residual ), optional nearest x`up` upsample and `rpad`
 * replicated rows on top and bottom (F.pad(...,(0,0,1,1),'replicate'), NonlocalNet.py:461-463).
 * slope_ptr == NULL => no activation.  y is [N][C][(H*up)+2*rpad][W*up] with its own batch stride. */
int dvc_affine_act(const float* x, const float* scale, const float* shift, const float* residual,
                   const float* slope_ptr, int32_t N, int32_t C, int32_t H, int32_t W, int32_t up,
                   int32_t rpad, int64_t x_batch_stride, int64_t res_batch_stride,
                   int64_t y_batch_stride, float* y, dvcStream stream);

/* InstanceNorm and what follows it in ONE launch: the statistics of every (n,c) plane as dvc_instnorm_stats,
 * then y = prelu_or_id( x*scale + shift + residual ) as dvc_affine_act, applied by the workgroup that reduced
 * the plane (its second read hits L2).  sub = 2 keeps every 2nd row/column (the stride-2 depthwise `*_ss`
 * convs, ColorVidNet.py:12,16,21; chan_scale = their weights); up / rpad as in dvc_affine_act; up and sub
 * exclude each other.  y is [N][C][VH + 2*rpad][VW], VH = H*up or ceil(H/2); y may be x itself when
 * up == sub == 1 and rpad == 0.  scale_out / shift_out (both or neither; may be NULL) receive the affine.
 * y2 (optional) is a second consumer's view of the same statistics: y2 = InstanceNorm(x) * chan_scale2 at stride
 * sub2, contiguous [N][C][ceil(H/sub2)][ceil(W/sub2)] (ColorVidNet normalises conv1_2 / conv2_2 / conv3_3 once for
 * the skip convolution and once, scaled and subsampled, for the next block).
 * The convolution that consumes y then needs no fused input transform and stages through LDS-DMA. */
int dvc_instnorm_apply(const float* x, const float* residual /* or NULL */, const float* slope_ptr /* or NULL */,
                       const float* chan_scale /* [C] or NULL */, float eps, int32_t N, int32_t C, int32_t H,
                       int32_t W, int32_t up, int32_t sub, int32_t rpad, int64_t x_batch_stride,
                       int64_t res_batch_stride, int64_t y_batch_stride, float* y,
                       float* scale_out, float* shift_out,
                       const float* chan_scale2 /* [C] or NULL */, int32_t sub2, float* y2 /* or NULL */,
                       dvcStream stream);
/* dvc_instnorm_apply on x = act(sum_s part[s] + bias): `part` = the [S][N][C][H*W] partial sums a convolution left in its
 * workspace (DVC_CONV_DEFER_REDUCE), bias [C] or NULL, act / act_slope / act_slope_ptr as DvcConvDesc.  Bit-identical to
 * reduce -> dvc_instnorm_apply; one launch and three passes over the tensor less.  H*W <= 16384 (the plane is built in LDS). */
int dvc_instnorm_apply_partials(const float* part, int32_t S, const float* bias, int32_t act, float act_slope,
                                const float* act_slope_ptr, const float* residual, const float* slope_ptr,
                                const float* chan_scale, float eps, int32_t N, int32_t C, int32_t H, int32_t W, int32_t up,
                                int32_t sub, int32_t rpad, int64_t res_batch_stride, int64_t y_batch_stride, float* y,
                                float* scale_out, float* shift_out, const float* chan_scale2, int32_t sub2, float* y2,
                                dvcStream stream);

/* r06 — several INDEPENDENT InstanceNorm launches as one: the norms of WarpNet's four heads
 * (models/NonlocalNet.py:364-410, run side by side by NonlocalNet.py:451-458).  Item i is dvc_instnorm_apply (S == 0: `x` is
 * the tensor, x_batch_stride elements per image, 0 => C*H*W) or dvc_instnorm_apply_partials (S >= 1: `x` is the [S][N][C][H*W]
 * partial sums, with bias / act / act_slope / act_slope_ptr; H*W <= 16384) without the second output; 1 .. 4 items.
 * Bit-identical to the per-item calls. */
typedef struct DvcInstNormItem {
    const float* x;
    int32_t S;
    const float* bias;            /* S >= 1 only, [C] or NULL */
    int32_t act;                  /* S >= 1 only, DVC_ACT_* of the convolution that left the partial sums */
    float act_slope;
    const float* act_slope_ptr;   /* or NULL */
    const float* residual;        /* or NULL */
    const float* slope_ptr;       /* PReLU slope of the norm's own activation, or NULL */
    const float* chan_scale;      /* [C] or NULL */
    float eps;
    int32_t N, C, H, W, up, sub, rpad;
    int64_t x_batch_stride, res_batch_stride, y_batch_stride;   /* elements; 0 => dense */
    float* y;
} DvcInstNormItem;
int dvc_instnorm_apply_group(const DvcInstNormItem* items, int32_t n_items, dvcStream stream);

/* nn.MaxPool2d(2,2) floor mode, NonlocalNet.py:237-255. planes = N*C.
 * NaN: the window maximum is taken with fmaxf, which DROPS a NaN (the maximum of the other elements; NaN only when all four
 * are), where ATen lets a NaN take the window.  The fused epilogue of dvc_conv2d_winograd_pool is tied to this bit for bit. */
int dvc_maxpool2x2(const float* x, int32_t planes, int32_t H, int32_t W, float* y, dvcStream stream);
/* nn.AvgPool2d(2,2): the pool="avg" variant of VGG19_pytorch, NonlocalNet.py:221-226; also, bit for bit,
 * F.interpolate(x, scale_factor=0.5, mode="bilinear") — full-resolution Lab -> network resolution, test.py:58,71. */
int dvc_avgpool2x2(const float* x, int32_t planes, int32_t H, int32_t W, float* y, dvcStream stream);
/* F.avg_pool2d(x, 4), NonlocalNet.py:491. */
int dvc_avgpool4x4(const float* x, int32_t planes, int32_t H, int32_t W, float* y, dvcStream stream);
/* nn.Upsample(scale_factor=f) nearest, NonlocalNet.py:425,499-500. */
int dvc_upsample_nearest(const float* x, int32_t planes, int32_t H, int32_t W, int32_t f, float* y,
                         dvcStream stream);
/* feature_normalize: x / (||x||_2 over C + eps), utils/util.py:155-158. */
int dvc_channel_l2norm(const float* x, int32_t N, int32_t C, int32_t HW, float eps, float* y,
                       dvcStream stream);
/* The same for up to DVC_L2NORM_MAX_TENSORS feature maps of one batch in ONE launch (FrameColor.py:16-23 normalises relu2_1 ..
 * relu5_1 of a frame back to back; the small maps alone are a handful of workgroups each).  x / y / C / HW: host arrays of
 * `count` entries; every map needs H*W % 4 == 0 and 16-byte aligned pointers.  Same arithmetic per pixel as
 * dvc_channel_l2norm up to the summation order of the channel groups. */
#define DVC_L2NORM_MAX_TENSORS 8
int dvc_channel_l2norm_multi(const float* const* x, float* const* y, const int32_t* C, const int32_t* HW,
                             int32_t count, int32_t N, float eps, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Colour / glue elementwise ops.
 */
/* gray2rgb_batch (utils/util.py:97-101): y[n,0..2] = (L+50)/100. */
int dvc_gray2rgb(const float* l, int32_t N, int32_t HW, int64_t l_batch_stride, float* y,
                 dvcStream stream);
/* tensor_lab2rgb (utils/util.py:379-414): Lab (L in [0,100], i.e. already uncentred when
 * l_offset == 0; pass l_offset = 50 to fold uncenter_l, utils/util.py:63-64) -> sRGB [0,1]. */
int dvc_lab2rgb(const float* lab, int32_t N, int32_t HW, float l_offset, float* rgb,
                dvcStream stream);
/* cat((IA_l, nonlocal_BA_lab[:,1:3], similarity_map, IA_last_lab), 1): models/FrameColor.py:63-64 -> out7 [N][7][HW].
 * IA_l: the luminance plane of the current frame (element stride between images `ia_batch_stride`, 0 = HW; 3 HW when it
 * is channel 0 of a Lab tensor).  IA_last_lab arrives as its two parts, so that the clip loop never materialises
 * test.py:96's cat((IA_l, ab_predict)) between frames: last_l = luminance plane of the previous frame, last_ab = the
 * previous [N][2][HW] prediction (batch strides 0 = HW / 2 HW); for an existing Lab tensor pass (lab, 3 HW, lab + HW, 3 HW).
 * warped_lab: [N][3][HW] (channels 1, 2 are read); sim: [N][1][HW].
 * A NEGATIVE batch stride means "the same plane for every image" (stride 0): one frame against the R references of a clip
 * (/root/reference/test.py:169-181), whose R ColorVidNet inputs share the frame's luminance. */
int dvc_pack_color_input(const float* IA_l, int64_t ia_batch_stride, const float* warped_lab, const float* sim,
                         const float* last_l, int64_t last_l_batch_stride, const float* last_ab,
                         int64_t last_ab_batch_stride, int32_t N, int32_t HW, float* out7, dvcStream stream);

/* ---- clip-driver tail, test.py:98-116 ------------------------------------------------
 * F.interpolate(x, scale_factor=2, mode="bilinear") * mul on `planes` planes of H x W (test.py:100-102; ATen's
 * align_corners=False source index and its fma evaluation order, bit-exact for the sizes the path uses). */
int dvc_upsample_bilinear2x(const float* x, int32_t planes, int32_t H, int32_t W, float mul, float* y,
                            dvcStream stream);
/* (uncenter_l(L) * 255 / 100).astype(uint8): the guide image of the WLS filter, test.py:106-109. */
int dvc_lum_guide_u8(const float* L_centered, int64_t n, uint8_t* guide, dvcStream stream);
/* cv2.ximgproc.createFastGlobalSmootherFilter(guide, lambda, sigma_color).filter(src) on `planes` float planes
 * (test.py:107-111): Min et al. 2014, Alg. 1 — num_iter x {row solve, column solve}, lambda_t = 1.5 * 4^(T-t) /
 * (4^T - 1) * lambda, weights exp(-|dg| / sigma_color).  OpenCV's defaults: num_iter 3, attenuation 0.25.
 * Several frames (guides) are filtered by one call: planes g*planes_per_guide.. use guide g.  dst may be src.
 * Parity unpinned (opencv-contrib is absent from the build image; see oracle/tail_oracle.py). */
size_t dvc_fgs_workspace_bytes(int32_t H, int32_t W, int32_t n_guides, int32_t planes_per_guide, int32_t num_iter);
int dvc_fgs_filter(const uint8_t* guide /* [n_guides][H][W] */, const float* src /* [n_guides*planes_per_guide][H][W] */,
                   int32_t n_guides, int32_t planes_per_guide, int32_t H, int32_t W, float lambda, float sigma_color,
                   int32_t num_iter, float lambda_attenuation, float* dst, void* workspace, size_t workspace_bytes,
                   dvcStream stream);
/* batch_lab2rgb_transpose_mc for one image (utils/util.py:134-151): Lab (L centred) -> skimage lab2rgb (float64)
 * -> clip -> *255 -> uint8, H x W x 3.  ab = [2][H][W].  Parity unpinned (skimage absent). */
int dvc_lab2rgb_u8(const float* L_centered, const float* ab, int32_t H, int32_t W, uint8_t* rgb_hwc,
                   dvcStream stream);
/* Frame ingest, colour part: RGB2Lab() -> ToTensor() -> Normalize(),
 * utils/util_distortion.py:18-23,85-100: skimage rgb2lab (float64) of an 8-bit H x W x 3 image, .float(), L - 50;
 * lab = [3][H][W].  Parity unpinned (skimage absent); round trip with dvc_lab2rgb_u8 tested. */
int dvc_rgb8_to_lab(const uint8_t* rgb_hwc, int32_t H, int32_t W, float* lab, dvcStream stream);
/* Frame ingest, geometric half: CenterPad(image_size)(image), utils/util_distortion.py:217-258 — skimage's
 * anti-aliased resize (Gaussian pre-filter + bilinear sampling, mirror boundaries, float64) to the target width or
 * height, centre crop, astype(uint8).  img = [H0][W0][3], out = [H][W][3].  Parity unpinned (skimage absent; the
 * restatement is checked against the SciPy calls skimage makes).
 * r06: workspace == NULL selects the FUSED kernel (one launch: a workgroup stages the 8-bit source window of its 8 x 32 output
 * tile in LDS, every thread filters only the values its bilinear sample reads — same arithmetic in the same order, the same
 * bytes); it applies when dvc_center_pad_is_fused() says so (down-scaling with a Gaussian radius <= 4 on both axes: factors
 * up to 3.25; also the same-size copy).  With a workspace of dvc_center_pad_workspace_bytes the three full-frame passes of
 * r01 run (any factor up to 21). */
size_t dvc_center_pad_workspace_bytes(int32_t H0, int32_t W0);
int dvc_center_pad_is_fused(int32_t H0, int32_t W0, int32_t H, int32_t W);
int dvc_center_pad(const uint8_t* img, int32_t H0, int32_t W0, int32_t H, int32_t W, uint8_t* out, void* workspace,
                   size_t workspace_bytes, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Dense correlation (the north-star kernel).  Replaces models/NonlocalNet.py:469-500:
 *   centre + normalise theta/phi -> f = theta^T phi (P x P) -> similarity = rowmax f ->
 *   softmax(f / T) -> y = softmax @ avgpool4(B_lab) -> nearest x4 upsample of y and similarity.
 * The P x P affinity is never written to memory: query rows live in registers, exemplar ("key")
 * tiles stream through LDS, the 256-deep dot products run on v_mfma_f32_32x32x2_f32, and the row
 * softmax is an online (running max / running sum) recurrence kept per lane.
 */
/* t_raw[B][C][P] (output of the 1x1 theta/phi conv) -> t[b,c,p] = (t_raw - mean_p) / (||.||_C + eps)
 * mean_scratch: B*C floats. */
int dvc_corr_prepare(const float* t_raw, int32_t B, int32_t C, int32_t P, float eps,
                     float* mean_scratch, float* t_out, dvcStream stream);

size_t dvc_corr_workspace_bytes(int32_t B, int32_t P);

/* theta, phi: [B][C][P] centred+normalised (C must be 256).  blab: [B][3][P] pooled exemplar Lab.
 * temperature > 0.  wta_scale == 1 disables the winner-take-all rescale (NonlocalNet.py:486);
 * otherwise f' = (f == rowmax f) ? f : f * wta_scale (WTA_scale.forward, NonlocalNet.py:295-309).
 * Outputs (any may be NULL): y_small [B][3][h][w], sim_small [B][1][h][w] with h*w == P,
 * y_up [B][3][4h][4w], sim_up [B][1][4h][4w], argmax [B][P] (index of the largest affinity per row,
 * lowest index on exact ties).
 * With EVERY output NULL (B == 1, wta_scale == 1) the merge of the per-workgroup partial softmax states is left to the
 * consumer: they stay in `workspace` (dvc_corr_workspace_bytes(1, P) bytes, which the caller then must not reuse) for
 * dvc_corr_merge_pack. */
int dvc_corr_fwd(const float* theta, const float* phi, const float* blab, float temperature,
                 float wta_scale, int32_t B, int32_t C, int32_t h, int32_t w, float* y_small,
                 float* sim_small, float* y_up, float* sim_up, int32_t* argmax, void* workspace,
                 size_t workspace_bytes, dvcStream stream);

/* The merge of a deferred dvc_corr_fwd (same temperature, h, w; `workspace` as that call left it) fused with the consumer of
 * its results, cat((IA_l, nonlocal_BA_lab[:,1:3], similarity_map, IA_last_lab), 1) of models/FrameColor.py:63-64 (see
 * dvc_pack_color_input) for ONE image: out7 [7][16 P]; IA_l, last_l: [16 P] planes; last_ab: [2][16 P].  The warped colours and
 * the similarity map go straight into channels 1..3 (x4 nearest, NonlocalNet.py:499-500) and are additionally written to
 * y_up [3][16 P] / sim_up [16 P] when those are not NULL (FrameColor.py:41-67 returns nonlocal_BA_lab).  Same arithmetic, same
 * order as the merge inside dvc_corr_fwd: bit-identical values.  Every pointer 16-byte aligned. */
int dvc_corr_merge_pack(const void* workspace, size_t workspace_bytes, float temperature, int32_t h, int32_t w,
                        const float* IA_l, const float* last_l, const float* last_ab, float* out7,
                        float* y_up /* or NULL */, float* sim_up /* or NULL */, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 mixed-precision correlation (BASELINE.json configs[4]).  Same reference lines as dvc_corr_fwd
 * (models/NonlocalNet.py:469-500); bf16 MFMA affinities are used as a candidate filter and every key
 * within 2*2^-8 of the bf16 row maximum is re-scored in exact fp32, which provably contains the fp32
 * argmax (unit-norm columns => |f_bf16 - f| <= 2^-8).  Exact for temperature <= 1e-4 (test.py:94 uses
 * 1e-10); larger temperatures are rejected (use dvc_corr_fwd).
 */
/* t_raw[B][C][P] -> centred + normalised copies in [B][P][C] layout: fp32 and bf16 (round-to-nearest-even). */
int dvc_corr_prepare_bf16(const float* t_raw, int32_t B, int32_t C, int32_t P, float eps,
                          float* mean_scratch, float* t_f32_pc, void* t_bf16_pc, dvcStream stream);
size_t dvc_corr_bf16_workspace_bytes(int32_t B, int32_t P);
int dvc_corr_fwd_bf16(const void* theta_bf16_pc, const void* phi_bf16_pc, const float* theta_f32_pc,
                      const float* phi_f32_pc, const float* blab, float temperature, int32_t B, int32_t C,
                      int32_t h, int32_t w, float* y_small, float* sim_small, float* y_up, float* sim_up,
                      int32_t* argmax, void* workspace, size_t workspace_bytes, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Contextual loss (models/ContextualLoss.py:29-126: `ContextualLoss_forward` :88-126 and `ContextualLoss` :29-77; called by
 * train.py:649-668 on relu3_1 / relu4_1 / relu5_1 features of the prediction and of the exemplar).  Per image, X = predicted,
 * Y = exemplar features [C][N]:   mu = mean_j Y;  Xn, Yn = (. - mu) / (||.||_C + eps);  S = Xn^T Yn;  d = 1 - S;
 * a_i = min_j d_ij + 1e-5;  A = softmax_j((1 - d / a_i) / h);  CX = mean_i max_j A_ij  (_forward)  |  mean_j max_i A_ij;
 * loss = -log CX.  The GEMMs run as 1x1 convolutions with per-image filters — batched GEMMs, DvcConvDesc::w_batch_stride —
 * (dvc_conv2d) from the host (dvc_amd/contextual.py) in blocks of rows of S, all images of the batch per launch; these entries are the pieces in between, forward and backward (gradient w.r.t. X; Y is data, as in train.py). */
/* x [B][C][P] -> out = (x - mean) / (||x - mean||_C + eps).  centre == 0: no mean.  mean_in != NULL: use it ([B*C], e.g. the
 * exemplar's, ContextualLoss.py:49-51); otherwise the own per-channel mean is computed into mean_out.  norm_out [B][P] (or
 * NULL) receives ||x - mean||_C (needed by dvc_cx_normalize_bwd). */
int dvc_cx_prepare(const float* x, const float* mean_in, int32_t centre, int32_t B, int32_t C, int32_t P, float eps,
                   float* mean_out, float* norm_out, float* out, dvcStream stream);
/* The entries below take a BATCH of nb images in one launch (r04; the products in between are batched GEMMs, DvcConvDesc::
 * w_batch_stride): S_bs = elements between the images' S blocks, row_bs = elements between their per-row arrays (a, jstar, l,
 * r, e: [nb][Nx] slices starting at the block's first row), tq_bs = between their t / q arrays; cmax / cargi are [nb][N],
 * gscale / loss [nb], dST [nb][N][ld_t]. */
/* S [nb][rows][N] (a block of rows of Xn^T Yn per image) -> per row: a = (1 - max_j S) + 1e-5, jstar = arg max_j S (lowest index
 * on ties), l = sum_j w, r = max_j A = w_jstar / l, e = sum_j A_ij d_ij, with w = exp((1 - d / a) / h). */
int dvc_cx_rows(const float* S, int32_t nb, int64_t S_bs, int64_t row_bs, int32_t rows, int32_t N, float h, float* a, int32_t* jstar,
                float* l, float* r, float* e, dvcStream stream);
/* ContextualLoss only: running column maxima of A over row blocks (cmax initialised below 0, cargi = the winning global row,
 * row0 = global index of the block's first row). */
int dvc_cx_colmax(const float* S, int32_t nb, int64_t S_bs, int64_t row_bs, const float* a, const float* l, int32_t rows, int32_t N,
                  int32_t row0, float h, float* cmax, int32_t* cargi, dvcStream stream);
/* per image b of v [nb][n]: loss[b] = -log(mean(v[b])),  gscale[b] = d loss / d v_k = -1 / (n mean(v[b])) */
int dvc_cx_finish(const float* v, int32_t nb, int32_t n, float* loss, float* gscale, dvcStream stream);
/* ContextualLoss backward: per row i of the block, t = sum of A_ik over the columns k whose maximum sits in row i
 * (cargi[k] == row0 + i), q = the same sum weighted by d_ik. */
int dvc_cx_rows_tq(const float* S, int32_t nb, int64_t S_bs, int64_t row_bs, int64_t tq_bs, const float* a, const float* l,
                   const int32_t* cargi, int32_t rows, int32_t N, int32_t row0, float h, float* t, float* q, dvcStream stream);
/* d loss / d S for a block of rows, row-major (dS, may be NULL) and transposed (dST [nb][N][ld_t], rows >= `rows` zero-filled:
 * the K-major operand of d Xn = Yn dS^T; may be NULL since r06 when dS is given).  mode 0 = ContextualLoss_forward, 1 = ContextualLoss (needs cargi, t, q).
 * gscale: [nb] device values from dvc_cx_finish (times the upstream gradient of each image's loss); gout: a common factor. */
int dvc_cx_ds(const float* S, int32_t nb, int64_t S_bs, int64_t row_bs, int64_t tq_bs, const float* a, const float* l, const float* r,
              const float* e, const int32_t* jstar, const int32_t* cargi, const float* t, const float* q, const float* gscale,
              float gout, int32_t mode, int32_t rows, int32_t N, int32_t row0, int32_t ld_t, float h, float* dS, float* dST,
              dvcStream stream);
/* backward of xn = xc / (||xc|| + eps) per position: dx = dxn / (n + eps) - xn (xn . dxn) / n. */
int dvc_cx_normalize_bwd(const float* xn, const float* norm, const float* dxn, int32_t B, int32_t C, int32_t P, float eps,
                         float* dx, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the fused correlation (training-side callers: train.py:402-427 runs frame_colorization, hence
 * WarpNet.forward, models/NonlocalNet.py:477-500, under autograd at temperature 0.01).  The host walks the query rows
 * in blocks (dvc_amd/corr_autograd.py); for one block of `rows` queries this entry turns the block's affinities
 * f_blk[rows][P] (= theta_blk^T phi, produced by dvc_conv2d as a 1x1 convolution) into
 *     dS[i][j] = p_ij * (g_i . B_j - g_i . y_i) / T  (+ gsim[i] at j == argmax[i]),   p = softmax_j(f / T)
 * written row-major (dS[rows][P]) and transposed (dST[P][ld_t], rows >= `rows` zero-filled) — the two K-major operands
 * of the 1x1-convolution GEMMs that follow (d phi += theta_blk dS, d theta_blk = phi dS^T).  dST may be NULL (r06): the
 * transposed copy is not written — for a caller whose GEMM takes dS transposed as it is (rocBLAS through torch.bmm).
 * gy, y: [3][.] with `chan_stride` elements between channels, already offset to the block's first query; sim, gsim,
 * argmax likewise (gsim / argmax may both be NULL: no gradient through the similarity map).  The softmax is re-evaluated
 * around the row maximum of f_blk ITSELF (the block is recomputed by another GEMM order than the forward kernel's, so the
 * saved similarity is not guaranteed to bound it: at T <= 1e-7 a 1e-7 excess would overflow the exponential); `sim` is
 * not read and is kept for the signature.  rowstat_scratch: [3][ld_t] floats (row maxima, row sums, raw row maxima).
 * wta_scale != 1 (r05): WTA_scale of NonlocalNet.py:288-327 ahead of the temperature — f' = (f == max_j f) ? f : f * wta_scale, and its
 * backward's factor (1 at the row maximum, the reference's constant 1e-4 elsewhere); gsim (similarity from f BEFORE it) unscaled.
 * batch (r05): images per call, dense: f_blk / dS [batch][ld_t][P], dST [batch][P][ld_t], blab / gy / y [batch][3][chan_stride]
 * (gy, y offset to the block's first row), gsim / argmax [batch][chan_stride], rowstat_scratch [batch][3][ld_t]. */
int dvc_corr_softmax_bwd(const float* f_blk, const float* blab, const float* gy, const float* y, const float* sim,
                         const float* gsim, const int32_t* argmax, float temperature, float wta_scale, int32_t batch, int32_t rows, int32_t P,
                         int64_t chan_stride, int32_t ld_t, float* rowstat_scratch, float* dS, float* dST,
                         dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Non-local weighted average (models/NonlocalNet.py:86-111, NonlocalWeightedAverage; find_local_patch :12-17), the
 * training-side smoothness term: per image, with x_lab and feature nearest-resized to H x W (N = H W),
 *     U = find_local_patch(feature, k)  [C k k][N];   A = softmax_j(U^T U / alpha);   out[2][N] = (A ab^T)^T
 * as one fused pass (dvc_amd/nonlocal_avg.py): nothing N x N and nothing k*k-times unfolded is materialised.
 * x_lab [B][Cx][Hx][Wx] (channels 1..2 are read), feature [B][C][Hf][Wf], out [B][2][H][W], all fp32 contiguous.
 * scale_x* / scale_f*: the source-index scales of the two nearest resizes, src = min(floor(dst * scale), in - 1) — the
 * float ATen derives (1 / scale_factor when a factor is given, in / out when a size is).  patch_size odd >= 1, alpha > 0.
 * workspace: dvc_nlwa_workspace_bytes(B, C, patch_size, H, W) bytes, 256-byte aligned; it holds, at 256-byte aligned offsets,
 * the zero-bordered resized feature F_pad [B][Cp][H + 2 (k/2)][W + 2 (k/2)] (Cp = C rounded up to 32, zero planes), then the
 * resized ab [B][2][N], then the partial softmax states.  Deterministic; an image's result does not depend on B. */
size_t dvc_nlwa_workspace_bytes(int32_t B, int32_t C, int32_t patch_size, int32_t H, int32_t W);
int dvc_nlwa_fwd(const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* feature, int32_t C, int32_t Hf, int32_t Wf,
                 int32_t B, int32_t H, int32_t W, float scale_xh, float scale_xw, float scale_fh, float scale_fw, int32_t patch_size,
                 float alpha, float* out, void* workspace, size_t workspace_bytes, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Local weighted average (models/NonlocalNet.py, WeightedAverage_color; find_local_patch :12-17), the local half of the
 * training-side smoothness term, forward and backward — csrc/local_avg.hip, one launch each.  With r = patch_size / 2,
 * g = (L + l_offset, a, b) of the nearest-resized x_lab and v = (a', b') of pred, both zero outside the image, per pixel p
 * and offset d in [-r, r]^2:
 *     w_d(p) = softmax_d(-|g(p + d) - g(p)|^2 / alpha)   (over all k*k offsets)      y_c(p) = sum_d w_d(p) v_c(p + d)
 * x_lab [B][Cx >= 3][Hx][Wx] (channels 0..2 are read), scale_x*: the source-index scales of its nearest resize to H x W as
 * for dvc_nlwa_fwd (1.0 and Hx == H, Wx == W: no resize).  pred [B][Cp][H][W]: channels ab_ch, ab_ch + 1 are a', b' (1 for
 * a Lab tensor, 0 for a bare [B][2][H][W] ab tensor).  l_offset: 50 folds uncenter_l.  patch_size odd, 1..7; alpha > 0 and
 * finite.  y [B][2][H][W].  All fp32 contiguous; no workspace, nothing k*k-times unfolded is materialised.
 * dvc_lwa_bwd: for G [B][2][H][W] and the forward's y, d_pred_ab [B][2][H][W] = dy/dv^T G and, unless d_guide is NULL,
 * d_guide [B][3][H][W] = the gradient of x_lab's channels 0..2 (the offset's derivative is 1); it is refused unless x_lab is
 * unresized (Hx == H, Wx == W, both scales 1.0): a caller that wants it through a resize resizes first.
 * Deterministic (gather form, no atomics); an image's result does not depend on B.  Bad arguments are reported before
 * any launch. */
int dvc_lwa_fwd(const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* pred, int32_t Cp, int32_t ab_ch, int32_t B,
                int32_t H, int32_t W, float scale_xh, float scale_xw, float l_offset, int32_t patch_size, float alpha, float* y,
                dvcStream stream);
int dvc_lwa_bwd(const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* pred, int32_t Cp, int32_t ab_ch, int32_t B,
                int32_t H, int32_t W, float scale_xh, float scale_xw, float l_offset, int32_t patch_size, float alpha,
                const float* G, const float* y, float* d_pred_ab, float* d_guide, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Flow warp (utils/warping.py, WarpingLayer: get_grid + F.grid_sample, bilinear, zeros padding), the temporal-consistency
 * term's warp, forward and backward — csrc/flow_warp.hip.  x [B][C][H][W], flow [B][2][H][W] (channel 0 = x displacement,
 * channel 1 = y displacement, in pixels), y [B][C][H][W], all fp32 contiguous.  Per output pixel (y, x) the sample position is
 *     align_corners = 1:  px = x + u,                         py = y + v
 *     align_corners = 0:  px = (x + u) W / (W - 1) - 0.5,     py = (y + v) H / (H - 1) - 0.5     (F.grid_sample's default)
 * and the output is the bilinear mix of the four corners around it, a corner outside the image counting as 0.  Coordinates
 * and weights are computed in double.  A NaN / inf coordinate gives NaN in every channel of that pixel, adds nothing to dx and
 * gives a NaN dflow; a finite one of any size is range-checked before it becomes an index.
 * dvc_flow_warp_bwd: for G [B][C][H][W], dx [B][C][H][W] and dflow [B][2][H][W], each optional (NULL = not wanted, not both).
 * dflow is a gather.  dx is a scatter done in exact integer arithmetic: per image, contributions are quantised to
 * 2^(e - 40), 2^e the smallest power of two above max |G| of that image, and added with 64-bit integer atomics, so dx is
 * bitwise reproducible, does not depend on B, and is within H W 2^-41 max |G| of exact before its one rounding to fp32.
 * max |G| == 0 gives dx = 0; a NaN / inf in an image's G gives a NaN dx for that image.  workspace (only read when dx is
 * wanted): dvc_flow_warp_bwd_workspace_bytes(B, C, H, W) bytes, 8-byte aligned, contents arbitrary (it is zeroed on the
 * stream).  B, C >= 1; H, W >= 2; H W <= 2^22.  Bad arguments are reported before any launch. */
size_t dvc_flow_warp_bwd_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int dvc_flow_warp_fwd(const float* x, const float* flow, int32_t B, int32_t C, int32_t H, int32_t W, int32_t align_corners,
                      float* y, dvcStream stream);
int dvc_flow_warp_bwd(const float* x, const float* flow, const float* G, int32_t B, int32_t C, int32_t H, int32_t W,
                      int32_t align_corners, float* dx, float* dflow, void* workspace, size_t workspace_bytes, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Batched fp32 GEMM on strided views — csrc/bgemm.hip: the products of the training side's row-block loops
 * (dvc_amd/block_products.py) without a vendor library.
 *     C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n],   b < batch, m < M, n < N, k < K   (all >= 1; M = 1 and K = 1 are legal)
 * Strides are in elements: A[b][m][k] at A + b a_sb + m a_sm + k a_sk, B[b][k][n] at B + b b_sb + k b_sk + n b_sn, C[b][m][n] at
 * C + b c_sb + m ldc + n with ldc >= N.  One of (a_sm, a_sk) and one of (b_sk, b_sn) must be 1: transposed and column-sliced
 * views of contiguous tensors.  No alignment beyond 4 bytes is needed (16-byte reads are used where pointer and strides allow).
 * accumulate = 0: C is written and never read (a NaN in the old C does not leak, elements between N and ldc are untouched);
 * accumulate = 1: C += A B.  Products and sums are exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), each element a k-ordered fma
 * chain; no atomics: results are bit-identical from run to run and an image's bits do not depend on the batch around it.
 * dvc_bgemm never splits K.  dvc_bgemm_splitk cuts K into slices when the output has too few 128 x 128 tiles to fill the chip
 * (the slice count depends on M, N, K only): partial sums go to `workspace` (dvc_bgemm_workspace_bytes(batch, M, N, K) bytes,
 * 0 = these sizes are not split and workspace may be NULL; contents arbitrary) and a second launch adds them in slice order.
 * Its bits differ from dvc_bgemm's where it splits, and are as reproducible.  Bad arguments (a null pointer, a non-positive
 * size, ldc < N, neither inner stride 1, a negative stride, a missing or short workspace) are reported before any launch. */
size_t dvc_bgemm_workspace_bytes(int32_t batch, int32_t M, int32_t N, int32_t K);
int dvc_bgemm(const float* A, const float* B, float* C, int32_t batch, int32_t M, int32_t N, int32_t K, int64_t a_sb, int64_t a_sm,
              int64_t a_sk, int64_t b_sb, int64_t b_sk, int64_t b_sn, int64_t c_sb, int64_t ldc, int32_t accumulate,
              dvcStream stream);
int dvc_bgemm_splitk(const float* A, const float* B, float* C, int32_t batch, int32_t M, int32_t N, int32_t K, int64_t a_sb,
                     int64_t a_sm, int64_t a_sk, int64_t b_sb, int64_t b_sk, int64_t b_sn, int64_t c_sb, int64_t ldc,
                     int32_t accumulate, void* workspace, size_t workspace_bytes, dvcStream stream);

/* dvc_bgemm_splitk's contract, argument for argument, on the bf16 matrix pipes — csrc/bgemm_split3.hip (opt-in: ops.bgemm's
 * engine="split3", block_products' backend "split3").  Every fp32 operand element is split exactly into three bf16 terms
 * (round to nearest, clamped so that no finite value rounds to infinity), eight of the nine term products run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulators — a1 b1 in one, the seven low-order products in another, added once at the
 * end — and a3 b3 alone is dropped (at most 2^-32 |a||b| per product).  Same strides, tails, ldc margin,
 * accumulate flag, refusals, split-K policy (dvc_bgemm_split3_workspace_bytes == dvc_bgemm_workspace_bytes) and
 * reproducibility; the error bound tests hold it to is the fp32 kernel's, (K + 2) 2^-24 (|A||B| + |C0|).  Special values:
 * zeros stay exact; a non-finite input makes the same output elements non-finite as the fp32 kernel does, though an Inf may
 * arrive as a NaN; inputs below 2^-100 in magnitude are outside the bound (their low terms may underflow in bf16) and give
 * finite results. */
size_t dvc_bgemm_split3_workspace_bytes(int32_t batch, int32_t M, int32_t N, int32_t K);
int dvc_bgemm_split3(const float* A, const float* B, float* C, int32_t batch, int32_t M, int32_t N, int32_t K, int64_t a_sb,
                     int64_t a_sm, int64_t a_sk, int64_t b_sb, int64_t b_sk, int64_t b_sn, int64_t c_sb, int64_t ldc,
                     int32_t accumulate, void* workspace, size_t workspace_bytes, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Input gradient of VGG19_pytorch (frozen weights) and of tensor_lab2rgb — csrc/vgg_bwd.hip.  The 3x3 convolutions' input
 * gradients run on dvc_conv2d / dvc_conv2d_winograd / dvc_conv2d_ws with the transposed, flipped filters; these are the steps
 * between them.  Masks and routes follow ATen: threshold_backward(grad, relu_out, 0) zeroes the gradient where out <= 0;
 * max_pool2d sends a window's gradient to the first maximum in scan order (a NaN takes the window).  Deterministic.
 *
 * dvc_vgg_act_bwd:  dZ = (dX + g) * [R > 0] over n elements; dX or g may be NULL (not both; one alone passes unchanged).  dZ
 *   may be dX (in place), not R or g.
 * dvc_vgg_pool_act_bwd:  a 2x2 stride-2 pool (floor mode) between two layers, per plane [H][W] (R, gR, dZ) and [H/2][W/2]
 *   (dP, gP):  dZ = (route(dP + gP) + gR) * [R > 0], route = the arg-max (DVC_POOL_MAX) or a quarter to each element
 *   (DVC_POOL_AVG).  Any of dP, gP, gR may be NULL (not all three).  With odd H or W the last row / column gets gR * mask.
 * dvc_vgg_conv1_bwd:  dx[N][3][H][W] = zero-padded 3x3 convolution of dZ [N][C][H][W] with w_t [3][C][3][3] (OIHW); C % 8 == 0,
 *   C <= 256.  VGG19's conv1_1: w_t = W^T flipped (x255 and the BGR swap of vgg_preprocess folded in when it applies).
 * dvc_lab2rgb_bwd:  grad_lab [N][3][HW] of dvc_lab2rgb at lab (same l_offset) for grad_rgb [N][3][HW]: the forward's float
 *   arithmetic recomputed, ATen's derivatives of the reference's composition (clamps pass inclusively). */
#define DVC_POOL_MAX 0
#define DVC_POOL_AVG 1
int dvc_vgg_act_bwd(const float* dX, const float* g, const float* R, int64_t n, float* dZ, dvcStream stream);
int dvc_vgg_pool_act_bwd(const float* dP, const float* gP, const float* gR, const float* R, int32_t planes, int32_t H, int32_t W,
                         int32_t pool_mode, float* dZ, dvcStream stream);
int dvc_vgg_conv1_bwd(const float* dZ, const float* w_t, int32_t N, int32_t C, int32_t H, int32_t W, float* dx, dvcStream stream);
int dvc_lab2rgb_bwd(const float* lab, int32_t N, int32_t HW, float l_offset, const float* grad_rgb, float* grad_lab,
                    dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * ColorVidNet's backward (training mode) — csrc/cvn_bwd.hip.  The 3x3 input gradients run on the forward's engines with the
 * transposed, flipped filters; these are the other steps.  Every sum has a fixed order: results are bit-deterministic.
 *
 * dvc_cvn_wgrad:  weight and bias gradient of a 3x3 convolution, pad == dil, stride 1, on v_mfma_f32_32x32x2_f32:
 *   out[co][ci][ky][kx] = sum_{b,y,x} dZ[b][co][y][x] * X[b][ci][y+(ky-1)dil][x+(kx-1)dil]   (zero outside the H x W map),
 *   then out[Cout*Cin*9 + co] = sum_{b,y,x} dZ[b][co][y][x].  dZ is [N][Cout][H][W]; X is the layer's input [N][Cin][H][W], or
 *   with in_up = 2 the half-resolution map [N][Cin][H/2][W/2] read through nearest x2 indexing (H, W even).  The positions are
 *   split over S slots (1 <= S <= 65535; dvc_cvn_wgrad_splits gives the default, 0 on bad sizes); part holds
 *   S * (Cout*Cin*9 + Cout) floats of partial sums, added in slot order by a second launch.
 * dvc_cvn_head_bwd:  conv10_ab (1x1, 2 outputs) + tanh*128 at the saved output ab [N][2][HW] for grad_ab [N][2][HW]:
 *   dpre = grad_ab * 128 * (1 - (ab/128)^2);  dZ[N][C][HW] = (w_ab^T dpre) * (R > 0 ? 1 : slope), R the saved post-leaky input
 *   [N][C][HW];  out[2][C] = sum dpre R^T, out[2C + o] = sum dpre_o.  w_ab is [2][C]; part holds
 *   dvc_cvn_head_bwd_workspace_floats(N, C, HW) floats.
 * dvc_cvn_inorm_bwd:  InstanceNorm (no affine) backward per [H][W] plane, n the saved output and rstd [N*C] its 1/sigma:
 *   dn = g_full + [y, x even] ss_w[c] g_ss[y/2][x/2] + (2x2 sum of g_up at 2y, 2x);
 *   dZ = rstd (dn - mean(dn) - n mean(dn n)) * [R > 0], R the producing layer's post-ReLU output.  g_full [N][C][H][W], g_ss
 *   [N][C][ceil(H/2)][ceil(W/2)], g_up [N][C][2H][2W]: any may be NULL (not all three).  With g_ss, ss_part [N][C] receives
 *   sum_{even y, x} n g_ss per plane and ss_grad [C] their sum over images (the `_ss` depthwise weights' gradient). */
int dvc_cvn_wgrad_splits(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W);
int dvc_cvn_wgrad(const float* dZ, const float* X, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t dil,
                  int32_t in_up, int32_t S, float* part, size_t part_floats, float* out, dvcStream stream);
size_t dvc_cvn_head_bwd_workspace_floats(int32_t N, int32_t C, int32_t HW);
int dvc_cvn_head_bwd(const float* ab, const float* grad_ab, const float* w_ab, const float* R, int32_t N, int32_t C, int32_t HW,
                     float slope, float* dZ, float* part, size_t part_floats, float* out, dvcStream stream);
int dvc_cvn_inorm_bwd(const float* n, const float* rstd, const float* R, const float* g_full, const float* g_ss, const float* ss_w,
                      const float* g_up, int32_t N, int32_t C, int32_t H, int32_t W, float* dZ, float* ss_part, float* ss_grad,
                      dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * WarpNet's backward behind the trunk tensor (training mode) — csrc/warp_bwd.hip.  The residual blocks' 3x3 input gradients run
 * on the forward's engines (zero pad 1 on a zero-ringed map, transposed flipped filters), their weight gradients on
 * dvc_cvn_wgrad (zero-ringed dZ against a reflect-padded copy of the input); these are the other steps.  Every sum has a fixed
 * order: results are bit-deterministic.
 *
 * dvc_warp_up4_bwd:  out[planes][h][w] = the 4x4 block sums of g [planes][4h][4w] (backward of the x4 nearest upsample).
 * dvc_warp_prelu_fwd:  y = prelu(n + skip) over count elements (skip may be NULL; y may be n), slope read from device memory.
 * dvc_warp_cn_bwd:  backward of dvc_corr_prepare at t_raw [B][C][P] with its per-row means mean [B][C]: tc = t - mean,
 *   r = ||tc||_2 over channels, d tc = g / (r + eps) - tc (tc . g) / (r (r + eps)^2) (second term zero where r == 0), then
 *   dt = d tc - mean_P(d tc) per channel row (channel sums and row means in double, rounded once).
 * dvc_warp_k1_wgrad:  weight and bias gradient of a 1x1 convolution on v_mfma_f32_32x32x2_f32:
 *   out[co][ci] = sum_{n,p} dT[n][co][p] F[n][ci][p], then out[Cout*Cin + co] = sum_{n,p} dT[n][co][p] (in double).  The positions
 *   are split over S slots (1 <= S <= 65535; dvc_warp_k1_wgrad_splits gives the default, 0 on bad sizes); part holds
 *   S * (Cout*Cin + Cout) floats of partial sums, added in slot order (in double) by a second launch.
 * dvc_warp_norm_prelu_bwd:  per [H][W] plane, from the gradient g at a PReLU output whose input was u = n + skip (skip may be
 *   NULL), n an InstanceNorm output with 1/sigma rstd [planes]:  du = g * (u > 0 ? 1 : a);  slope_part[plane] =
 *   sum (u > 0 ? 0 : u g) (ATen's prelu backward);  dz = rstd (du - mean(du) - n mean(du n)) into the interior of the
 *   zero-ringed plane dz_ringed [planes][H+2][W+2] (the ring is written too).  du [planes][H][W] (may be NULL) receives du, the
 *   skip's gradient.
 * dvc_warp_slope_sum:  out[0] = the sum of count doubles in a fixed order, rounded once.
 * dvc_warp_reflect_pad:  x_padded [planes][H+2][W+2] = ReflectionPad2d(1) of x [planes][H][W]; H, W >= 2.
 * dvc_warp_fold:  the adjoint: dx [planes][H][W] = the interior of g_padded [planes][H+2][W+2] + its ring folded onto rows /
 *   columns 1 and H-2 / W-2 (+ skip [planes][H][W] when given; dx may be skip). */
int dvc_warp_up4_bwd(const float* g, int32_t planes, int32_t h, int32_t w, float* out, dvcStream stream);
int dvc_warp_prelu_fwd(const float* n, const float* skip, const float* slope, int64_t count, float* y, dvcStream stream);
int dvc_warp_cn_bwd(const float* t_raw, const float* mean, const float* g, int32_t B, int32_t C, int32_t P, float eps, float* dt,
                    dvcStream stream);
int dvc_warp_k1_wgrad_splits(int32_t N, int32_t Cin, int32_t Cout, int32_t P);
int dvc_warp_k1_wgrad(const float* dT, const float* F, int32_t N, int32_t Cin, int32_t Cout, int32_t P, int32_t S, float* part,
                      size_t part_floats, float* out, dvcStream stream);
int dvc_warp_norm_prelu_bwd(const float* g, const float* n, const float* skip, const float* rstd, const float* slope,
                            int32_t planes, int32_t H, int32_t W, float* dz_ringed, float* du, double* slope_part,
                            dvcStream stream);
int dvc_warp_slope_sum(const double* part, int64_t count, float* out, dvcStream stream);
int dvc_warp_reflect_pad(const float* x, int32_t planes, int32_t H, int32_t W, float* x_padded, dvcStream stream);
int dvc_warp_fold(const float* g_padded, const float* skip, int32_t planes, int32_t H, int32_t W, float* dx, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * WarpNet's backward through its four heads (training mode with WarpNet.set_head_training) — csrc/warp_head_bwd.hip.  The heads'
 * norm + PReLU sites, 3x3 input gradients and reflect-pad adjoints run on the entry points above; these are what the heads add.
 * Every sum has a fixed order: results are bit-deterministic.
 *
 * dvc_warp_head_wgrad:  weight and bias gradient of a 3x3 reflect-pad-1 convolution of stride s in {1, 2} on an H x W input
 *   (H, W >= 2; output Ho x Wo, Ho = (H - 1) / s + 1), on v_mfma_f32_32x32x2_f32:
 *   out[co][ci][ky][kx] = sum_{n,oy,ox} dz[n][co][oy][ox] x_padded[n][ci][s oy + ky][s ox + kx], then
 *   out[Cout*Cin*9 + co] = sum dz[n][co] (in double).  dz_ringed [N][Cout][Ho+2][Wo+2] is the zero-ringed map
 *   dvc_warp_norm_prelu_bwd writes (only its interior is read), x_padded [N][Cin][H+2][W+2] the output of dvc_warp_reflect_pad.
 *   Only the Ho x Wo output positions are multiplied.  The positions are split over S slots (1 <= S <= 65535;
 *   dvc_warp_head_wgrad_splits gives the default, 0 on bad sizes); part holds S * (Cout*Cin*9 + Cout) floats of partial sums,
 *   added in slot order (in double) by a second launch.
 * dvc_warp_dilate_ring:  out [planes][H+2][W+2] = 0 except out[1 + 2 oy][1 + 2 ox] = dz[oy][ox], dz the interior of
 *   dz_ringed [planes][Ho+2][Wo+2] with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1: the map whose zero-pad-1 3x3 convolution
 *   with the transposed flipped filters is the gradient at the reflect-padded input of a stride-2 layer (then dvc_warp_fold).
 * dvc_warp_up2_bwd:  out[planes][h][w] = the 2x2 block sums of g [planes][2h][2w] (backward of a x2 nearest upsample).
 * dvc_warp_rpad_rows_bwd:  backward of rpad replicated rows above and below: out [planes][h][w] = rows rpad .. rpad+h-1 of
 *   g [planes][h + 2 rpad][w], the rows above added onto row 0 and the rows below onto row h-1 (1 <= rpad <= 64). */
int dvc_warp_head_wgrad_splits(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t stride);
int dvc_warp_head_wgrad(const float* dz_ringed, const float* x_padded, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W,
                        int32_t stride, int32_t S, float* part, size_t part_floats, float* out, dvcStream stream);
int dvc_warp_dilate_ring(const float* dz_ringed, int32_t planes, int32_t Ho, int32_t Wo, int32_t H, int32_t W, float* out,
                         dvcStream stream);
int dvc_warp_up2_bwd(const float* g, int32_t planes, int32_t h, int32_t w, float* out, dvcStream stream);
int dvc_warp_rpad_rows_bwd(const float* g, int32_t planes, int32_t h, int32_t w, int32_t rpad, float* out, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Discriminator_x64 as a frozen critic (models/GAN_models.py:104-157, models/spectral_normalization.py): forward and the
 * gradient back to its input — csrc/gan.hip, walked by dvc_amd/gan.py.  Every sum has a fixed order and nothing is added
 * atomically: results are bit-deterministic.  W_bar is the stored filter [Cout][Cin][kh][kw], read as the matrix [Cout][K]; it
 * is never rewritten: each layer multiplies by the device scalar inv_sigma[0] = 1 / sigma in its epilogue.
 *
 * dvc_gan_spectral_sigma:  one power step of SpectralNorm on W_bar [Cout][K] (1 <= Cout, K):  v <- l2n(W_bar^T u),
 *   u <- l2n(W_bar v), l2n(z) = z / (|z| + eps), then inv_sigma[0] = 1 / (u^T W_bar v).  u [Cout] and v [K] are updated in place.
 *   workspace: at least (K + Cout) floats.  Three launches.
 * dvc_gan_sn_weight:  w_scaled[co][k] = W_bar[co][k] * inv_sigma[0] and (when w_scaled_t != NULL) w_scaled_t[k * ldt + co] the
 *   same, transposed: the filters of the attention block's 1x1 projections in the two layouts dvc_conv2d (ksize 1) takes for the
 *   forward and the input gradient; ldt >= Cout lets three projections share one stacked matrix.  w_scaled may be NULL.
 * dvc_gan_conv4s2:  y = act(conv4x4, stride 2, zero pad 1 (x, W_bar) * inv_sigma[0] + bias) as an implicit GEMM over K = 16 Cin
 *   on v_mfma_f32_32x32x2_f32.  d: N, Cin, H, W, Cout, ksize 4, stride 2, pad 1, dil 1, act NONE or LEAKY (act_slope), the batch
 *   strides of x and y; every other field at its default.  Output OH x OW = H / 2 x W / 2 (floor); H, W >= 2, any Cout >= 1.
 *   W_bar 16-byte aligned.
 * dvc_gan_conv4s2_dgrad:  the input gradient of that layer in gather form, d describing the FORWARD layer:
 *   dx[n][ci][iy][ix] = inv_sigma[0] * sum_{co} sum_{2x2 taps by the parity of iy, ix} W_bar[co][ci][ky][kx] dz[n][co][oy][ox],
 *   dz [N][Cout][OH][OW] (batch stride d->y_batch_stride) the gradient at the layer's PRE-activation output, dx [N][Cin][H][W]
 *   (batch stride d->x_batch_stride).  mask_act != NULL ([N][Cin][H][W], dense — the layer's input, i.e. the LeakyReLU output of
 *   the layer in front): dx is multiplied by (mask_act > 0 ? 1 : d->act_slope), which makes it the dz of that layer.
 * dvc_gan_last / dvc_gan_last_bwd:  out[n] = mean over the (H-2) x (W-5) positions of conv [3,6] valid (x, W_bar [1][Cin][3][6])
 *   * inv_sigma[0] + bias[0], x [N][Cin][H][W] with H >= 3, W >= 6; and its input gradient for g [N] = d loss / d out, times
 *   (mask_act > 0 ? 1 : slope) when mask_act != NULL (x itself, the LeakyReLU output of the layer in front).
 * dvc_gan_softmax_rows:  a[r][j] = exp(e[r][j] - max_j e[r]) / sum_j exp(...) for `rows` rows of P floats; a may be e.
 * dvc_gan_softmax_rows_bwd:  dE[r][j] = a[r][j] (dA[r][j] - sum_j a[r][j] dA[r][j]); dE may be dA.
 * dvc_gan_scale_add:  y[i] = gamma[0] * o[i] + x[i] (x == NULL: gamma[0] * o[i]) for count floats; gamma on the device.
 * dvc_gan_lrelu_bwd:  out[i] = (d[i] + g[i]) * (act[i] > 0 ? 1 : slope); d or g may be NULL (not both); out may be d or g. */
int dvc_gan_spectral_sigma(const float* w_bar, int32_t Cout, int32_t K, float eps, float* u, float* v, float* inv_sigma,
                           void* workspace, size_t workspace_bytes, dvcStream stream);
int dvc_gan_sn_weight(const float* w_bar, const float* inv_sigma, int32_t Cout, int32_t K, float* w_scaled, float* w_scaled_t,
                      int32_t ldt, dvcStream stream);
int dvc_gan_conv4s2(const DvcConvDesc* d, const float* x, const float* w_bar, const float* bias, const float* inv_sigma, float* y,
                    dvcStream stream);
int dvc_gan_conv4s2_dgrad(const DvcConvDesc* d, const float* dz, const float* w_bar, const float* inv_sigma,
                          const float* mask_act, float* dx, dvcStream stream);
int dvc_gan_last(const float* x, const float* w_bar, const float* bias, const float* inv_sigma, int32_t N, int32_t Cin, int32_t H,
                 int32_t W, int64_t x_batch_stride, float* out, dvcStream stream);
int dvc_gan_last_bwd(const float* g, const float* w_bar, const float* inv_sigma, const float* mask_act, float slope, int32_t N,
                     int32_t Cin, int32_t H, int32_t W, float* dx, dvcStream stream);
int dvc_gan_softmax_rows(const float* e, int64_t rows, int32_t P, float* a, dvcStream stream);
int dvc_gan_softmax_rows_bwd(const float* a, const float* dA, int64_t rows, int32_t P, float* dE, dvcStream stream);
int dvc_gan_scale_add(const float* o, const float* x, const float* gamma, int64_t count, float* y, dvcStream stream);
int dvc_gan_lrelu_bwd(const float* d, const float* g, const float* act, float slope, int64_t count, float* out, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Discriminator_x64: its own parameter gradients — csrc/gan_wgrad.hip, launched by dvc_amd/gan.py behind
 * `set_parameter_training()`.  SpectralNorm computes sigma = u'^T W_bar v' inside the graph with the vectors u', v' the power step
 * of THAT forward left (constants), and the layer uses W = W_bar / sigma; so with G = d loss / d W, the plain weight gradient,
 * d loss / d W_bar = G / sigma - (<G, W_bar> / sigma^2) u' v'^T.  Fixed orders, no atomics: bit-deterministic.
 *
 * dvc_gan_conv4s2_wgrad:  G and the bias gradient of the layer d describes (the fields dvc_gan_conv4s2 reads; act is not used):
 *   out[((co Cin + ci) 4 + ky) 4 + kx] = sum_{n,oy,ox} dz[n][co][oy][ox] x[n][ci][2 oy + ky - 1][2 ox + kx - 1] (out of range: 0),
 *   then out[Cout Cin 16 + co] = sum_{n,oy,ox} dz[n][co][oy][ox] (a double chain per slot).  dz [N][Cout][OH][OW] (batch stride
 *   d->y_batch_stride) is the gradient at the layer's PRE-activation output, x [N][Cin][H][W] (d->x_batch_stride) its input.
 *   On v_mfma_f32_32x32x2_f32; the pixels, numbered over the whole batch, are cut into chunks of 16 and the chunks into S
 *   contiguous ranges, 1 <= S <= 65535 (dvc_gan_conv4s2_wgrad_splits(d): the default; 0 for a descriptor that is refused).  part:
 *   S slots of ld = Cout Cin 16 + Cout floats (part_floats >= S ld), every float of which is written; out [ld] = the slots added
 *   in slot order in double, rounded once.  The bits depend on S and on nothing else.  out and part alias neither each other nor
 *   an input.  Two launches.
 * dvc_gan_sn_wgrad:  out[co][k] = (G[co][k] - c u[co] v[k]) * inv_sigma[0] with c = <G, W_bar> * inv_sigma[0], the inner product
 *   in double in a fixed order, every element computed in double and rounded once.  G, W_bar, out [Cout][K]; u [Cout], v [K] the
 *   vectors AFTER the forward's power step.  out is overwritten (accumulating into a .grad is the caller's business) and aliases
 *   no input.  workspace: dvc_gan_dot_workspace_bytes(Cout K) bytes, 8-byte aligned.  Two launches.
 * dvc_gan_last_wgrad:  for `last` (dvc_gan_last) on x [N][Cin][H][W], H >= 3, W >= 6, and g [N] = d loss / d out:
 *   out[(c 3 + ky) 6 + kx] = sum_n g[n] / cnt * sum_{oy,ox} x[n][c][oy + ky][ox + kx], cnt = (H-2)(W-5); out[Cin 18] = sum_n g[n].
 * dvc_gan_dot:  out[0] = sum_i a[i] b[i] over count >= 1 floats, in double in a fixed order that depends on count alone, rounded
 *   once.  workspace as for dvc_gan_sn_wgrad.  Two launches. */
int dvc_gan_conv4s2_wgrad_splits(const DvcConvDesc* d);
int dvc_gan_conv4s2_wgrad(const DvcConvDesc* d, const float* dz, const float* x, int32_t S, float* part, size_t part_floats,
                          float* out, dvcStream stream);
size_t dvc_gan_dot_workspace_bytes(int64_t count);
int dvc_gan_sn_wgrad(const float* G, const float* w_bar, const float* u, const float* v, const float* inv_sigma, int32_t Cout,
                     int32_t K, float* out, void* workspace, size_t workspace_bytes, dvcStream stream);
int dvc_gan_last_wgrad(const float* g, const float* x, int32_t N, int32_t Cin, int32_t H, int32_t W, int64_t x_batch_stride,
                       float* out, dvcStream stream);
int dvc_gan_dot(const float* a, const float* b, int64_t count, float* out, void* workspace, size_t workspace_bytes,
                dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Adam: every parameter tensor of an optimiser step in ONE launch — csrc/optim.hip, driven by dvc_amd/optim.py (a drop-in for
 * torch.optim.Adam).  The launch works from two DEVICE-resident tables the caller owns and fills: `tensors`, one DvcAdamTensor
 * per parameter tensor, and `chunks`, which cuts every tensor into pieces of at most DVC_ADAM_CHUNK elements (chunk k of tensor
 * i: {i, k * DVC_ADAM_CHUNK}); a workgroup walks chunks grid-stride, so a 1-element tensor and a 2.36 M-element one load the chip
 * evenly.  Per element, all in fp32 (torch.optim.Adam's single-tensor rule):
 *   g' = weight_decay != 0 ? fma(weight_decay, p, g) : g
 *   m  = fma(one_minus_beta1, g' - m, m)
 *   v  = fma(one_minus_beta2, g' * g', beta2 * v);   vmax != NULL:  vmax = max(vmax, v), and vmax takes v's place below
 *   p  = fma(-step_size, m / fma(sqrt(v), inv_sqrt_bc2, eps), p)          (sqrt and the division correctly rounded)
 * The scalars are per TENSOR (torch keeps `step` per parameter, and groups differ in lr): the caller evaluates them in double —
 * step_size = lr / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t), 1 - beta — and rounds each once.
 * A chunk whose p, g, m, v (and vmax) addresses are all 16-byte aligned moves as 16-byte vectors with a scalar tail; any other
 * chunk takes the scalar path, so tensors may be views that start on any 4-byte boundary.  No element outside [0, n) of any tensor
 * is read or written; a tensor with n == 0 needs no chunk.  Plain loads and stores, no atomics, no LDS: every element is
 * independent, the result is bit-reproducible and does not depend on what else is in the launch.  A chunk that names a tensor
 * outside [0, n_tensors) or a start outside [0, n) is skipped.  p, g, m, v, vmax of one tensor and of different tensors must not
 * overlap.
 * dvc_adam_step refuses before launching: a negative count, null tables (with tensors present), n_chunks == 0 with tensors
 * present.  n_tensors == 0 is a successful no-op.  One launch; nothing is allocated, copied or synchronised. */
#define DVC_ADAM_CHUNK 4096
typedef struct DvcAdamTensor {
    float* p;           /* parameter, updated in place */
    const float* g;     /* gradient */
    float* m;           /* exp_avg */
    float* v;           /* exp_avg_sq */
    float* vmax;        /* max_exp_avg_sq (amsgrad), or NULL */
    int64_t n;          /* elements */
    float step_size, inv_sqrt_bc2, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay;
    float reserved;     /* 0 */
} DvcAdamTensor;        /* 80 bytes */
typedef struct DvcAdamChunk {
    int32_t tensor;     /* index into the tensor table */
    int32_t reserved;   /* 0 */
    int64_t start;      /* first element of the chunk, a multiple of DVC_ADAM_CHUNK */
} DvcAdamChunk;         /* 16 bytes */
int dvc_adam_step(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks, dvcStream stream);

/* The step count and the two bias-correction columns kept on the DEVICE (dvc_amd.optim.CapturableAdam, torch's capturable=True
 * contract): one launch, ahead of dvc_adam_step on the same stream and the same tensor table, in which one thread per tensor does
 *   t = *step + 1;  *step = t;                      lr_i = lr_tensor ? *lr_tensor : lr
 *   tensors[i].step_size    = (float)(lr_i / (1 - pow(beta1, t)))          (double throughout, rounded once)
 *   tensors[i].inv_sqrt_bc2 = (float)(1 / sqrt(1 - pow(beta2, t)))
 * and touches nothing else of the record: the addresses, n and the other five scalar columns stay as the caller wrote them.  The
 * step therefore depends on nothing the host computes per step, and the pair of launches can be replayed from a captured graph.
 * `step` (and `lr_tensor`, when not NULL) are one-element fp32 device tensors; the `step` of different records must not alias.
 * dvc_adam_advance refuses before launching: a negative count, null tables (with tensors present).  n_tensors == 0 is a
 * successful no-op.  One launch; nothing is allocated, copied or synchronised. */
typedef struct DvcAdamAdvance {
    float* step;                /* the tensor's step count, advanced in place */
    const float* lr_tensor;     /* NULL: use `lr` */
    double lr, beta1, beta2;
} DvcAdamAdvance;       /* 40 bytes */
int dvc_adam_advance(const DvcAdamAdvance* advance, DvcAdamTensor* tensors, int32_t n_tensors, dvcStream stream);

/* The gradient guard (dvc_amd.optim.GuardedAdam, optim.grad_norm, optim.clip_grad_norm_): the global L2 norm of every gradient of
 * the tensor table, clip_grad_norm_'s coefficient and a non-finite flag, kept in a 24-byte DEVICE record that the guarded advance
 * and step obey — so a step replayed from a graph can clip its gradients and skip itself on a NaN or Inf with no host code.  All
 * four entry points work on the tensor and chunk tables of dvc_adam_step.
 * dvc_grad_norm, two launches; only g and n of a tensor record are read.  Stage 1 (256 threads, grid min(n_chunks, 2048),
 *   grid-stride over the chunks): thread j of a chunk adds (double)g * (double)g — exact: the square of an fp32 value fits a double —
 *   of its elements 4 (j + 256 r) + k (r = 0..3, k = 0..3) in that order, by 16-byte loads when g + start is 16-byte aligned and
 *   the four lie inside the chunk, by dword loads otherwise (same values, same order); block_sum (csrc/reduce.h: butterfly in the
 *   wave, the four waves in CHAIN order) combines the 256 doubles into partials[chunk], a function of the chunk's data alone.
 *   Stage 2, one workgroup: thread j adds partials j, j + 256, ..., block_sum gives S, and thread 0 writes, with ordinary stores,
 *     sumsq = S;  total_norm = (float)sqrt(S);  nonfinite = S is NaN or inf
 *     clip_coef = nonfinite ? 1.0f : (float)min(1.0, max_norm / (sqrt(S) + 1e-6))      (in double: clip_grad_norm_'s formula;
 *                                                                                      max_norm = +inf gives exactly 1.0f)
 *     found_inf = nonfinite && !(flags & DVC_GRAD_NORM_KEEP_NONFINITE);   skipped += found_inf
 *   The caller zeroes `skipped` once; every other field is overwritten.  With DVC_GRAD_NORM_KEEP_NONFINITE the flag stays 0 and the
 *   coefficient 1.0f on non-finite gradients: the guarded step then does what dvc_adam_step does with them.  Finite gradients
 *   whose norm exceeds the fp32 range report total_norm = inf with found_inf = 0, and clip_coef is still the finite value computed
 *   from the double.  No atomics; the record and every partial are bit-reproducible and independent of what else is in the table.
 *   `partials`: n_chunks doubles of scratch.
 * dvc_adam_advance_guarded: dvc_adam_advance, except that with guard->found_inf set it touches nothing — `step` is not advanced and
 *   the two columns are not rewritten.
 * dvc_adam_step_guarded: dvc_adam_step, except that with guard->found_inf set it returns before any load or store, and otherwise
 *   uses g' = clip_coef * g (one fp32 multiply, exact for 1.0f) in g's place.  g is never written.
 * dvc_grad_scale: g *= c in place (g is written through the table's const pointer: the gradients are the caller's), for the
 *   stand-alone clip_grad_norm_.  c = guard->clip_coef; with found_inf set it is what torch.nn.utils.clip_grad_norm_ (with
 *   error_if_nonfinite=False) multiplies by: NaN when the norm is NaN (every gradient becomes NaN), 0 when it is inf (Inf elements
 *   become NaN, the others 0).  One case differs from torch: max_norm = +inf with an infinite norm, where torch's inf / inf gives
 *   NaN and the record no longer knows max_norm; 0 is used.  c == 1.0f stores nothing.
 * All refuse before launching: a negative count; null tables or a null guard, or n_chunks == 0, with tensors present; dvc_grad_norm
 * also a max_norm that is NaN or <= 0, unknown flags and null partials.  n_tensors == 0 is a successful no-op (the record is not
 * written).  Nothing is allocated, copied or synchronised. */
#define DVC_GRAD_NORM_KEEP_NONFINITE 1u
typedef struct DvcGradGuard {
    float total_norm;   /* (float)sqrt(sumsq) */
    float clip_coef;    /* what the guarded step and dvc_grad_scale multiply g by */
    int32_t found_inf;  /* 1: sumsq is NaN or inf, and the step is to be skipped */
    int32_t skipped;    /* running count of found_inf */
    double sumsq;       /* sum of g^2 over every tensor, in double */
} DvcGradGuard;         /* 24 bytes */
int dvc_grad_norm(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks, double* partials,
                  double max_norm, uint32_t flags, DvcGradGuard* guard, dvcStream stream);
int dvc_adam_advance_guarded(const DvcAdamAdvance* advance, DvcAdamTensor* tensors, int32_t n_tensors, const DvcGradGuard* guard,
                             dvcStream stream);
int dvc_adam_step_guarded(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks,
                          const DvcGradGuard* guard, dvcStream stream);
int dvc_grad_scale(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks,
                   const DvcGradGuard* guard, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Pixel losses: every term scale * mean_i(w * |x_i - t_i|^p), p in {1, 2}, of a training step on one fused reduction —
 * csrc/loss.hip, driven by dvc_amd/losses.py (train.py's mse_loss / l1_loss / weighted_mse_loss / weighted_l1_loss).  As for Adam,
 * the launches work from two DEVICE-resident tables the caller owns: `terms`, one DvcLossTerm per term, and `chunks`, which cuts
 * every term into pieces of at most DVC_LOSS_CHUNK elements, terms in order, chunk j of term k at start j * DVC_LOSS_CHUNK.
 * `terms_host` is the caller's HOST copy of the term table (the staging buffer the device copy was sent from): every refusal below
 * is decided from it before anything is launched, and the kernels never see it.
 *   x: n contiguous floats.  t: n floats, or NULL for the scalar t_scalar.  w: NULL; n floats (cpl == 0); or a [B,1,H,W] mask
 *   broadcast over the channels of x [B,C,H,W] (plane = H*W, cpl = C*plane): element i reads w[(i / cpl) * plane + i % plane].
 * Per element, in fp32 and with no contraction: d = x - t, e = d*d or |d|, v = w*e (v = e without w; a NaN under a zero weight
 * stays a NaN).  Chunks whose x, t (dx, dt) addresses are 16-byte aligned move as 16-byte vectors, any other chunk element by
 * element; a full-shape w likewise from its own address, a broadcast w as vectors only when also plane % 4 == 0.
 * dvc_loss_fwd, two launches.  Stage 1: thread j of the 256 of a chunk adds the v of elements 4 (j + 256 r) + k (r = 0..3, k = 0..3)
 *   into a double, in that order whichever path loaded them; the 256 doubles are combined by block_sum (csrc/reduce.h: butterfly in
 *   the wave, the four waves in CHAIN order) and stored to partials[chunk] — a function of the chunk's data alone.  Stage 2, one
 *   workgroup: per term, thread j adds the term's partials j, j + 256, ..., block_sum gives S_k;
 *   values[k] = (float)(S_k * (double)scale_k / n_k), and values[n_terms] = (float) of those doubles added in term order.
 *   A term's value is therefore bit-identical alone and inside any table.  No atomics; nothing is allocated or synchronised.
 * dvc_loss_bwd, one launch: c_k = (float)(((double)grad_total[0] + grad_values[k]) * scale_k / n_k) from device memory (grad_values
 *   may be NULL: zeros); dx_i = (2 c_k * w_i) * d_i for p = 2, (c_k * w_i) * sgn(d_i) for p = 1 with sgn(0) = 0; dt_i = -dx_i; each
 *   is stored only where its pointer is non-NULL, and a term with neither is not touched.  Forward ignores dx and dt.
 * Both refuse before launching: a negative count; null tables, n_chunks == 0, or n_chunks != sum ceil(n_k / DVC_LOSS_CHUNK) with
 * terms present; p outside {1, 2}; n <= 0; null x; plane <= 0, cpl % plane != 0 or n % cpl != 0; null partials / values /
 * grad_total.  n_terms == 0 is a successful no-op.  A chunk that names a term outside [0, n_terms) or a start outside [0, n) is
 * skipped (its partial is 0).  dx and dt must not overlap x, t, w or each other. */
#define DVC_LOSS_CHUNK 4096
typedef struct DvcLossTerm {
    const float* x;     /* input */
    const float* t;     /* target of x's shape, or NULL: t_scalar */
    const float* w;     /* weights (see cpl), or NULL */
    float* dx;          /* backward: gradient to x, or NULL */
    float* dt;          /* backward: gradient to t, or NULL */
    int64_t n;          /* elements of x */
    int64_t plane;      /* H*W of a broadcast w; 1 otherwise */
    int64_t cpl;        /* C*H*W of a broadcast w; 0: w has x's shape */
    int32_t p;          /* 1: |d|, 2: d*d */
    int32_t reserved;   /* 0 */
    float t_scalar, scale;
} DvcLossTerm;          /* 80 bytes */
typedef struct DvcLossChunk {
    int32_t term;       /* index into the term table */
    int32_t reserved;   /* 0 */
    int64_t start;      /* first element of the chunk, a multiple of DVC_LOSS_CHUNK */
} DvcLossChunk;         /* 16 bytes */
int dvc_loss_fwd(const DvcLossTerm* terms, const DvcLossTerm* terms_host, int32_t n_terms, const DvcLossChunk* chunks,
                 int64_t n_chunks, double* partials, float* values, dvcStream stream);
int dvc_loss_bwd(const DvcLossTerm* terms, const DvcLossTerm* terms_host, int32_t n_terms, const DvcLossChunk* chunks,
                 int64_t n_chunks, const float* grad_total, const float* grad_values, dvcStream stream);

/* ------------------------------------------------------------------------------------------------
 * Loss plans: the terms above and two more kinds on RESIDENT tables, so that a call whose tensors did not move is launches and
 * nothing else and can be replayed from a captured graph — csrc/loss_plan.hip, driven by dvc_amd.losses.Plan.  The element and
 * chunk code of kinds 1 and 2 is the one dvc_loss_fwd / dvc_loss_bwd run (csrc/loss_chunk.h), so their values and gradients have
 * dvc_loss_fwd's bits.
 *   kind 1 (L1), 2 (MSE): scale * mean(w * |x - t|^p) with p == kind, exactly as above.
 *   kind 3 (MEAN): v_i = w_i * (x_i - t_i), signed; t and w as above; dx_i = c_k * w_i, dt_i = -dx_i.  p is 1.
 *   kind 4 (REL), the relativistic GAN term scale * mean_i(((x_i - mean(y)) - c)^2): y is n_y floats of its own (n_y != n allowed),
 *     t and w are NULL, p is 2.  m = (float)(S_y / n_y) with S_y the double sum of y in the order below; d_i = (x_i - m) - c, two
 *     fp32 subtractions; v_i = d_i * d_i.  dx_i = (2 c_k) * d_i;  dy_j = (float)(-(double)(2 c_k) * (sum_i d_i) / n_y), the same for
 *     every j, with sum_i d_i the double the FORWARD left in the scratch: the backward does not reduce again.
 * `chunks` holds n_chunks records that cut the x of every term, terms in order (as for dvc_loss_fwd), and behind them n_ychunks
 * records that cut the y of every REL term the same way, terms in order.  `scratch`, DVC_LOSS_PLAN_SCRATCH doubles the caller
 * owns, is [n_chunks partials | n_chunks partials of sum d | n_ychunks partials of y | per slot {m, sum d}]; a REL term names its
 * slot (0 <= slot < n_terms, no two REL terms the same one).
 * dvc_loss_plan_check, HOST only, nothing launched and no device touched: every refusal, decided from the host copy of the term
 * table at the time the tables are built — a resident table cannot be validated without a synchronising copy, so the launch
 * entry points take device tables only and check nothing but null pointers and counts.  It refuses what dvc_loss_fwd refuses
 * (negative counts, a null table, n_chunks == 0 or != sum ceil(n_k / DVC_LOSS_CHUNK), n <= 0, null x, the plane / cpl rules) and
 * kind outside 1..4; p that does not belong to the kind; REL with null y, n_y <= 0, a t or a w, or a slot outside [0, n_terms) or
 * used twice; another kind with a y, a dy or n_y != 0; n_ychunks != sum over REL terms of ceil(n_y / DVC_LOSS_CHUNK).
 * A C caller must have had dvc_loss_plan_check accept the host copy of exactly these tables with exactly these n_terms, n_chunks and
 * n_ychunks before it passes them to the two launch entry points: those take the counts on trust, size their grids from them and
 * index `chunks` ((n_chunks + n_ychunks) records) and `scratch` (DVC_LOSS_PLAN_SCRATCH doubles) by them.
 * dvc_loss_plan_fwd, two launches, four with a REL term (n_ychunks > 0), a straight line on `stream`:
 *   stage 0a  per y chunk, thread j adds (double)y of elements 4 (j + 256 r) + k in that order, block_sum (CHAIN) -> its partial;
 *   stage 0b  one workgroup: per REL term, thread j adds the term's y partials j, j + 256, ..., block_sum -> S_y; m -> its slot;
 *   stage 1   per x chunk as dvc_loss_fwd; a REL chunk reads m from its slot and accumulates two doubles, sum d^2 and sum d;
 *   stage 2   one workgroup: values[k] = (float)(S_k * scale_k / n_k) and values[n_terms] from the same doubles in term order,
 *             dvc_loss_fwd's rule; a REL term's sum d (its partials j, j + 256, ..., block_sum) -> its slot.
 *   Every partial depends on its chunk's data alone (a REL chunk's also on m, a function of y alone): a term's value is
 *   bit-identical alone and inside any plan.
 * dvc_loss_plan_bwd, one launch over the n_chunks + n_ychunks chunks; c_k from device memory as in dvc_loss_bwd.
 * No atomics; nothing is allocated, copied or synchronised.  n_terms == 0 is a successful no-op. */
#define DVC_LOSS_KIND_L1 1
#define DVC_LOSS_KIND_MSE 2
#define DVC_LOSS_KIND_MEAN 3
#define DVC_LOSS_KIND_REL 4
#define DVC_LOSS_PLAN_SCRATCH(n_terms, n_chunks, n_ychunks) (2 * (n_chunks) + (n_ychunks) + 2 * (n_terms))
typedef struct DvcPlanTerm {
    const float* x;     /* the first 80 bytes are DvcLossTerm's, with `kind` in the place of its reserved field */
    const float* t;
    const float* w;
    float* dx;
    float* dt;
    int64_t n;
    int64_t plane;
    int64_t cpl;
    int32_t p;          /* 1 for kinds 1 and 3, 2 for kinds 2 and 4 */
    int32_t kind;       /* DVC_LOSS_KIND_* */
    float t_scalar, scale;
    const float* y;     /* REL: the tensor whose mean is subtracted; NULL otherwise */
    float* dy;          /* backward, REL: gradient to y, or NULL */
    int64_t n_y;        /* REL: elements of y; 0 otherwise */
    float c;            /* REL: the constant */
    int32_t slot;       /* REL: index of the term's {m, sum d} pair in the scratch */
} DvcPlanTerm;          /* 112 bytes */
int dvc_loss_plan_check(const DvcPlanTerm* terms_host, int32_t n_terms, int64_t n_chunks, int64_t n_ychunks);
int dvc_loss_plan_fwd(const DvcPlanTerm* terms, int32_t n_terms, const DvcLossChunk* chunks, int64_t n_chunks, int64_t n_ychunks,
                      double* scratch, float* values, dvcStream stream);
int dvc_loss_plan_bwd(const DvcPlanTerm* terms, int32_t n_terms, const DvcLossChunk* chunks, int64_t n_chunks, int64_t n_ychunks,
                      const double* scratch, const float* grad_total, const float* grad_values, dvcStream stream);

#ifdef DVC_DEBUG
/* ------------------------------------------------------------------------------------------------
 * Diagnostics for the timing probes under tools/ — ONLY in a -DDVC_DEBUG build (`make -C csrc DEBUG=1` ->
 * dvc_amd/libdvc_hip_debug.so); the production library has neither these symbols nor the state behind them
 * (process-global switches, not thread-safe; all default to off and every probe switches them off again).
 *   dvc_debug_conv_trace     buf != NULL: LDS-DMA conv kernels record {entry, end of chunk loop, HW_ID, XCC_ID} per workgroup
 *   dvc_debug_conv_variant   1 / 2 / 3: skip all / patch / weight staging after the first chunk (timing only, wrong results)
 *   dvc_debug_corr_timeline  buf != NULL: per-tile s_memtime stamps of wave 0 of every correlation workgroup
 *   dvc_debug_corr_variant   1: skip the softmax arithmetic of dvc_corr_fwd (timing only, wrong results) */
void dvc_debug_conv_trace(long long* buf);
void dvc_debug_conv_variant(int v);
void dvc_debug_corr_timeline(long long* buf, int max_tiles);
void dvc_debug_corr_variant(int v);
#endif /* DVC_DEBUG */

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* DVC_HIP_H */
