// What gan.hip (forward, input gradient) and gan_wgrad.hip (parameter gradients) share: the 64 x 128 x 16 fp32-MFMA tile step
// with its blocked summation, and the descriptor check of the 4x4 stride-2 layer.  The library is built with -fno-gpu-rdc:
// everything here but GanConvArgs (a kernel parameter type: it stays global so that the kernels of gan.hip keep their symbol
// names) is in an anonymous namespace and each including file gets its own instance.
#pragma once
#include "common.h"

struct GanConvArgs {
    const float* x;          // forward: the input; dgrad: dz
    const float* w;
    const float* bias;       // forward only
    const float* inv_sigma;
    const float* mask_act;   // dgrad only, may be NULL
    float* y;                // forward: the output; dgrad: dx
    int N, Cin, H, W, Cout, OH, OW, act;
    float slope;
    long xbs, ybs;           // batch strides of the [N][Cin][H][W] and the [N][Cout][OH][OW] tensor
    long P;                  // N * OH * OW
};

namespace {

typedef float gan_f16v __attribute__((ext_vector_type(16)));

constexpr int kGanM = 64;            // channels per workgroup tile
constexpr int kGanN = 128;           // pixels (weight gradient: filter columns) per workgroup tile
constexpr int kGanK = 16;            // k per step
constexpr int kGanLdA = kGanM + 4;   // LDS row strides (floats)
constexpr int kGanLdB = kGanN + 4;
constexpr int kGanFlush = 16;        // steps (256 k) after which the running fma chain is closed into the block total

// one K step: 8 k-pairs, two MFMAs each; lane l reads row/pixel l & 31 of k = 2 kk + (l >> 5)
__device__ __forceinline__ void gan_mma_step(const float* sA, const float* sB, int wave, int l31, int hi, gan_f16v (&acc)[2]) {
    const float* pa = sA + hi * kGanLdA + l31;
    const float* pb = sB + hi * kGanLdB + wave * 32 + l31;
#pragma unroll
    for (int kk = 0; kk < kGanK / 2; ++kk) {
        const float a0 = pa[2 * kk * kGanLdA], a1 = pa[2 * kk * kGanLdA + 32];
        const float b = pb[2 * kk * kGanLdB];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
    }
}

__device__ __forceinline__ void gan_zero(gan_f16v (&acc)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// blocked summation: tot += acc, acc = 0
__device__ __forceinline__ void gan_flush(gan_f16v (&acc)[2], gan_f16v (&tot)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        tot[i] += acc[i];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    }
}

constexpr long kGanMaxBlocks = 0x7fffffffL;

static int gan_check_desc(const char* fn, const DvcConvDesc* d, GanConvArgs& a) {
    DVC_REQUIRE(d, "%s: null descriptor", fn);
    DVC_REQUIRE(d->ksize == 4 && d->stride == 2 && d->pad == 1 && d->dil == 1 && d->pad_mode == DVC_PAD_ZERO,
                "%s: the layer is a 4x4 stride-2 zero-pad-1 convolution (got ksize %d, stride %d, pad %d, dil %d, pad_mode %d)", fn,
                d->ksize, d->stride, d->pad, d->dil, d->pad_mode);
    DVC_REQUIRE(d->in_up == 1 && d->in_sub == 1 && d->in_prelu == 0 && d->flags == 0 && d->w_batch_stride == 0 && d->cfg == -1 &&
                    d->split_k == 0 && d->res_batch_stride == 0,
                "%s: no input transform, residual, flag, per-image filter, cfg or split_k is supported", fn);
    DVC_REQUIRE(d->act == DVC_ACT_NONE || d->act == DVC_ACT_LEAKY, "%s: act must be NONE or LEAKY (got %d)", fn, d->act);
    DVC_REQUIRE(d->N >= 1 && d->Cin >= 1 && d->Cout >= 1 && d->H >= 2 && d->W >= 2, "%s: bad shape (N %d, Cin %d, Cout %d, H %d, W %d)",
                fn, d->N, d->Cin, d->Cout, d->H, d->W);
    DVC_REQUIRE((long)d->Cin * 16 <= 0x7fffffffL && (long)d->Cout * d->Cin * 16 <= 0x7fffffffL, "%s: filter too large", fn);
    a.N = d->N, a.Cin = d->Cin, a.H = d->H, a.W = d->W, a.Cout = d->Cout, a.OH = d->H / 2, a.OW = d->W / 2;
    a.act = d->act, a.slope = d->act_slope;
    const long xdense = (long)d->Cin * d->H * d->W, ydense = (long)d->Cout * a.OH * a.OW;
    DVC_REQUIRE(d->x_batch_stride == 0 || d->x_batch_stride >= xdense, "%s: x_batch_stride (%ld) is below Cin*H*W (%ld)", fn,
                (long)d->x_batch_stride, xdense);
    DVC_REQUIRE(d->y_batch_stride == 0 || d->y_batch_stride >= ydense, "%s: y_batch_stride (%ld) is below Cout*OH*OW (%ld)", fn,
                (long)d->y_batch_stride, ydense);
    a.xbs = d->x_batch_stride ? d->x_batch_stride : xdense;
    a.ybs = d->y_batch_stride ? d->y_batch_stride : ydense;
    a.P = (long)d->N * a.OH * a.OW;
    a.bias = nullptr, a.mask_act = nullptr;
    return 0;
}

}  // namespace
