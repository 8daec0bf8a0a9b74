// Discriminator_x64 as a frozen critic (models/GAN_models.py:104-157 with models/spectral_normalization.py), for gfx950:
// forward and the gradient back to the input (its parameter gradients: gan_wgrad.hip).  dvc_amd/gan.py walks the layers;
// include/dvc_hip.h states every entry point.
//
// The 4x4 stride-2 convolution and its input gradient are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered
// fma chain per output element) in the tiling of bgemm.hip, cut to what these layers need: a workgroup of 4 waves owns
// 64 channels x 128 pixels, wave w the pixels [32 w, 32 w + 32) as two 32 x 32 MFMA tiles (32 accumulator registers).  Pixels
// are numbered over the whole batch, so the 3 x 6 and 6 x 12 maps of the last layers share tiles across images; K advances in
// steps of 16.  Both operands are staged k-major in LDS (row strides 68 and 132 floats); the MFMA loop reads one dword per lane
// per operand tile, each half wave from 32 consecutive banks.  The next step's operands are fetched into registers before the
// MFMA loop of the current one and stored after it (one LDS buffer, two barriers per step).  Neither kernel splits K and
// neither adds atomically: one output element is a sum of fma chains of 256 k each, closed in k order into a block total
// (kGanFlush — a blocked sum, whose rounding error grows with sqrt(256) + sqrt(K / 256) instead of sqrt(K)), whatever the batch.
//
//   forward  M = Cout, K = 16 Cin (one input channel per step: k = 16 ci + 4 ky + kx, which is W_bar's own row order, so the
//            filter tile is one float4 per thread), B[k][pixel] = x[n][ci][2 oy + ky - 1][2 ox + kx - 1] gathered with the eight
//            bounds predicates of a thread's pixel computed once, outside the K loop.  Epilogue: acc / sigma + bias, LeakyReLU.
//   dgrad    gather form.  An input pixel (iy, ix) is reached by the taps ky = 1 - py + 2 ty from the output rows
//            oy = (iy + py) / 2 - ty (py = iy & 1, ty in {0, 1}), and the same along x: 2 x 2 taps per output channel, which
//            ones decided by the pixel's parity.  blockIdx.z is the parity class; within a class M = Cin, K = 4 Cout (four
//            output channels per step: k = 4 co + 2 ty + tx), B[k][pixel] = dz[n][co][oy][ox].  Epilogue: acc / sigma, times
//            the LeakyReLU derivative of the layer in FRONT (its output is this layer's input) when the caller passes it — the
//            mask is fused into the store end, so a dgrad always reads a gradient at a pre-activation.
//
// Spectral normalisation: three launches (W^T u per column; the norm of that, v and W v per row; the norm of that, u and
// sigma).  Every sum goes through reduce.h: per-thread partial sums in a fixed order, then TREE or CHAIN across the waves.
#include "common.h"
#include "gan_common.h"   // the tile step, GanConvArgs, gan_check_desc: shared with gan_wgrad.hip
#include "reduce.h"

#include <cstdint>

// ---- forward: grid (pixel tiles, Cout tiles)
__global__ __launch_bounds__(256) void gan_conv4s2_kernel(GanConvArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[kGanK * kGanLdA];
    __shared__ __attribute__((aligned(16))) float sB[kGanK * kGanLdB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int m0 = blockIdx.y * kGanM;
    const long p0 = (long)blockIdx.x * kGanN;
    const long HW = (long)a.H * a.W, OHW = (long)a.OH * a.OW;
    const int K = a.Cin * 16;

    // B: thread -> pixel tid & 127, filter rows 2 bh and 2 bh + 1, all four kx
    const int bp = tid & 127, bh = tid >> 7;
    long xoff = 0;
    unsigned ok = 0;
    {
        const long p = p0 + bp;
        if (p < a.P) {
            const int n = (int)(p / OHW), rem = (int)(p - (long)n * OHW), oy = rem / a.OW, ox = rem - oy * a.OW;
            const int iy0 = 2 * oy - 1 + 2 * bh, ix0 = 2 * ox - 1;
            xoff = (long)n * a.xbs + (long)iy0 * a.W + ix0;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int kx = 0; kx < 4; ++kx)
                    if (iy0 + j >= 0 && iy0 + j < a.H && ix0 + kx >= 0 && ix0 + kx < a.W) ok |= 1u << (j * 4 + kx);
        }
    }
    // A: thread -> filter row m0 + (tid >> 2), k = 4 (tid & 3) .. + 3 of the step
    const int ar = tid >> 2, ak = (tid & 3) * 4;
    const bool a_ok = m0 + ar < a.Cout;
    const float* wrow = a.w + (long)(m0 + ar) * K + ak;

    gan_f16v acc[2], tot[2];
    gan_zero(acc);
    gan_zero(tot);
    float4 ra;
    float rb[8];
    auto load = [&](int ci) {
        ra = a_ok ? *reinterpret_cast<const float4*>(wrow + ci * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float* xc = a.x + xoff + (long)ci * HW;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) rb[j * 4 + kx] = (ok >> (j * 4 + kx)) & 1u ? xc[j * a.W + kx] : 0.f;
    };
    load(0);
    for (int ci = 0; ci < a.Cin; ++ci) {
        {
            float* d = sA + ak * kGanLdA + ar;
            d[0] = ra.x, d[kGanLdA] = ra.y, d[2 * kGanLdA] = ra.z, d[3 * kGanLdA] = ra.w;
#pragma unroll
            for (int j = 0; j < 8; ++j) sB[(bh * 8 + j) * kGanLdB + bp] = rb[j];
        }
        __syncthreads();
        if (ci + 1 < a.Cin) load(ci + 1);
        gan_mma_step(sA, sB, wave, l31, hi, acc);
        if (ci % kGanFlush == kGanFlush - 1) gan_flush(acc, tot);
        __syncthreads();
    }
    gan_flush(acc, tot);

    // C/D layout: column (pixel) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const long p = p0 + wave * 32 + l31;
    if (p >= a.P) return;
    const int n = (int)(p / OHW);
    float* yb = a.y + (long)n * a.ybs + (p - (long)n * OHW);
    const float inv = a.inv_sigma[0];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (co < a.Cout) {
                float v = tot[i][r] * inv + a.bias[co];
                if (a.act == DVC_ACT_LEAKY) v = v > 0.f ? v : v * a.slope;
                yb[(long)co * OHW] = v;
            }
        }
}

// ---- input gradient: grid (pixel tiles of the largest parity class, Cin tiles, 4 parity classes)
__global__ __launch_bounds__(256) void gan_conv4s2_dgrad_kernel(GanConvArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[kGanK * kGanLdA];
    __shared__ __attribute__((aligned(16))) float sB[kGanK * kGanLdB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int py = blockIdx.z >> 1, px = blockIdx.z & 1;
    const int HA = (a.H - py + 1) / 2, WB = (a.W - px + 1) / 2;   // rows / columns of this parity
    const long PA = (long)HA * WB, Pc = PA * a.N;
    const long p0 = (long)blockIdx.x * kGanN;
    if (p0 >= Pc) return;
    const int m0 = blockIdx.y * kGanM;
    const long HW = (long)a.H * a.W, OHW = (long)a.OH * a.OW;

    // B: thread -> pixel tid & 127, output channels 2 bh and 2 bh + 1 of the step, all four taps
    const int bp = tid & 127, bh = tid >> 7;
    long zoff[4] = {0, 0, 0, 0};
    unsigned ok = 0;
    {
        const long p = p0 + bp;
        if (p < Pc) {
            const int n = (int)(p / PA), rem = (int)(p - (long)n * PA), ay = rem / WB, ax = rem - ay * WB;
#pragma unroll
            for (int ty = 0; ty < 2; ++ty)
#pragma unroll
                for (int tx = 0; tx < 2; ++tx) {
                    const int oy = ay + py - ty, ox = ax + px - tx;
                    if (oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW) {
                        ok |= 1u << (ty * 2 + tx);
                        zoff[ty * 2 + tx] = (long)n * a.ybs + (long)oy * a.OW + ox;
                    }
                }
        }
    }
    // A: thread -> input channel m0 + (tid & 63), output channel tid >> 6 of the step, all four taps
    const int ac = tid & 63, ao = tid >> 6;
    const bool a_ok = m0 + ac < a.Cin;
    const float* wtap = a.w + (long)(m0 + ac) * 16 + (1 - py) * 4 + (1 - px);   // + co Cin 16 + 8 ty + 2 tx

    gan_f16v acc[2], tot[2];
    gan_zero(acc);
    gan_zero(tot);
    float ra[4], rb[8];
    auto load = [&](int st) {
        const int co_a = 4 * st + ao;
        const float* wc = wtap + (long)co_a * a.Cin * 16;
        const bool wa = a_ok && co_a < a.Cout;
#pragma unroll
        for (int t = 0; t < 4; ++t) ra[t] = wa ? wc[8 * (t >> 1) + 2 * (t & 1)] : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int co = 4 * st + 2 * bh + j;
            const float* zc = a.x + (long)co * OHW;
#pragma unroll
            for (int t = 0; t < 4; ++t) rb[j * 4 + t] = (co < a.Cout && ((ok >> t) & 1u)) ? zc[zoff[t]] : 0.f;
        }
    };
    const int steps = (a.Cout + 3) / 4;
    load(0);
    for (int st = 0; st < steps; ++st) {
#pragma unroll
        for (int t = 0; t < 4; ++t) sA[(ao * 4 + t) * kGanLdA + ac] = ra[t];
#pragma unroll
        for (int j = 0; j < 8; ++j) sB[(bh * 8 + j) * kGanLdB + bp] = rb[j];
        __syncthreads();
        if (st + 1 < steps) load(st + 1);
        gan_mma_step(sA, sB, wave, l31, hi, acc);
        if (st % kGanFlush == kGanFlush - 1) gan_flush(acc, tot);
        __syncthreads();
    }
    gan_flush(acc, tot);

    const long p = p0 + wave * 32 + l31;
    if (p >= Pc) return;
    const int n = (int)(p / PA), rem = (int)(p - (long)n * PA), ay = rem / WB, ax = rem - ay * WB;
    const long pix = (long)(py + 2 * ay) * a.W + (px + 2 * ax);
    float* xb = a.y + (long)n * a.xbs + pix;
    const float* mb = a.mask_act ? a.mask_act + (long)n * a.Cin * HW + pix : nullptr;
    const float inv = a.inv_sigma[0];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (ci < a.Cin) {
                float v = tot[i][r] * inv;
                if (mb) v *= mb[(long)ci * HW] > 0.f ? 1.f : a.slope;
                xb[(long)ci * HW] = v;
            }
        }
}

// ---- spectral normalisation
// t[k] = sum_i W[i][k] u[i]: a workgroup owns 64 columns; wave g sums the rows i = g (mod 4) into four partial sums by
// (i / 4) mod 4, combined as a tree, then the four waves' results as a tree
__global__ __launch_bounds__(256) void gan_sn_wtu_kernel(const float* __restrict__ Wm, const float* __restrict__ u, float* __restrict__ t,
                                                         int Cout, int K) {
    __shared__ float red[64 * 4];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6, k = blockIdx.x * 64 + c;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < K)
        for (int i0 = g; i0 < Cout; i0 += 16)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + 4 * q;
                if (i < Cout) s[q] += Wm[(long)i * K + k] * u[i];
            }
    red[c * 4 + g] = tree_sum4(s);
    __syncthreads();
    if (g == 0 && k < K) t[k] = tree_sum4(red + c * 4);
}

// s[i] = sum_k W[i][k] v[k] with v = t / (|t| + eps): one workgroup per row; every workgroup sums |t|^2 in the same order, the
// first one writes v
__global__ __launch_bounds__(256) void gan_sn_wv_kernel(const float* __restrict__ Wm, const float* __restrict__ t, float* __restrict__ v,
                                                        float* __restrict__ s, int K, float eps) {
    __shared__ float red[4];
    const int i = blockIdx.x;
    float q = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) q += t[k] * t[k];
    const float den = sqrtf(block_sum<float, 256>(q, red)) + eps;
    const float* wr = Wm + (long)i * K;
    float d = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float vk = t[k] / den;
        if (i == 0) v[k] = vk;
        d += wr[k] * vk;
    }
    d = block_sum<float, 256>(d, red);
    if (threadIdx.x == 0) s[i] = d;
}

// u = s / (|s| + eps), inv_sigma = 1 / (u . s): one workgroup
__global__ __launch_bounds__(256) void gan_sn_sigma_kernel(const float* __restrict__ s, float* __restrict__ u, float* __restrict__ inv_sigma,
                                                           int Cout, float eps) {
    __shared__ float red[4];
    float q = 0.f;
    for (int i = threadIdx.x; i < Cout; i += 256) q += s[i] * s[i];
    const float den = sqrtf(block_sum<float, 256>(q, red)) + eps;
    float d = 0.f;
    for (int i = threadIdx.x; i < Cout; i += 256) {
        const float ui = s[i] / den;
        u[i] = ui;
        d += ui * s[i];
    }
    d = block_sum<float, 256>(d, red);
    if (threadIdx.x == 0) inv_sigma[0] = 1.f / d;
}

__global__ __launch_bounds__(256) void gan_sn_weight_kernel(const float* __restrict__ Wm, const float* __restrict__ inv_sigma,
                                                            float* __restrict__ ws, float* __restrict__ wt, int Cout, int K, int ldt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Cout * K) return;
    const float v = Wm[e] * inv_sigma[0];
    if (ws) ws[e] = v;
    if (wt) {
        const int co = (int)(e / K), k = (int)(e - (long)co * K);
        wt[(long)k * ldt + co] = v;
    }
}

// ---- the last layer: [3, 6] valid convolution to one channel, then the mean over its positions.  One workgroup per image;
// thread-strided partial sums over the Cin * 18 filter taps, each tap times the sum of the inputs it meets, then CHAIN
__global__ __launch_bounds__(256) void gan_last_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ inv_sigma, int Cin, int H, int W, long xbs,
                                                       float* __restrict__ out) {
    __shared__ float red[4];
    const int n = blockIdx.x, OH = H - 2, OW = W - 5;
    const float* xn = x + (long)n * xbs;
    float s = 0.f;
    for (int e = threadIdx.x; e < Cin * 18; e += 256) {
        const int c = e / 18, r = e - c * 18, ky = r / 6, kx = r - ky * 6;
        const float* xc = xn + (long)c * H * W + ky * W + kx;
        float q = 0.f;
        for (int oy = 0; oy < OH; ++oy)
            for (int ox = 0; ox < OW; ++ox) q += xc[oy * W + ox];
        s += w[e] * q;
    }
    s = block_sum<float, 256>(s, red);
    if (threadIdx.x == 0) out[n] = s * inv_sigma[0] / (float)(OH * OW) + bias[0];
}

__global__ __launch_bounds__(256) void gan_last_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                           const float* __restrict__ inv_sigma, const float* __restrict__ mask_act,
                                                           float slope, int Cin, int H, int W, long total, float* __restrict__ dx) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int OH = H - 2, OW = W - 5;
    const int ix = (int)(e % W), iy = (int)((e / W) % H), c = (int)((e / ((long)W * H)) % Cin), n = (int)(e / ((long)W * H * Cin));
    float q = 0.f;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 6; ++kx)
            if (iy - ky >= 0 && iy - ky < OH && ix - kx >= 0 && ix - kx < OW) q += w[c * 18 + ky * 6 + kx];
    float v = g[n] * inv_sigma[0] / (float)(OH * OW) * q;
    if (mask_act) v *= mask_act[e] > 0.f ? 1.f : slope;
    dx[e] = v;
}

// ---- attention: row softmax and its backward, one wave per row (four rows per workgroup); a may be e and dE may be dA: a
// lane writes only the elements it alone reads, after its reductions
__global__ __launch_bounds__(256) void gan_softmax_rows_kernel(const float* e, long rows, int P, float* a) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* er = e + r * P;
    float* ar = a + r * P;
    float m = -INFINITY;
    for (int j = lane; j < P; j += 64) m = fmaxf(m, er[j]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < P; j += 64) s += expf(er[j] - m);
    s = wave_sum(s);
    for (int j = lane; j < P; j += 64) ar[j] = expf(er[j] - m) / s;
}

__global__ __launch_bounds__(256) void gan_softmax_rows_bwd_kernel(const float* __restrict__ a, const float* dA, long rows, int P, float* dE) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* ar = a + r * P;
    const float* gr = dA + r * P;
    float* dr = dE + r * P;
    float s = 0.f;
    for (int j = lane; j < P; j += 64) s += ar[j] * gr[j];
    s = wave_sum(s);
    for (int j = lane; j < P; j += 64) dr[j] = ar[j] * (gr[j] - s);
}

__global__ __launch_bounds__(256) void gan_scale_add_kernel(const float* __restrict__ o, const float* __restrict__ x, const float* __restrict__ gamma,
                                                            long count, float* __restrict__ y) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float v = gamma[0] * o[e];
    y[e] = x ? v + x[e] : v;
}

__global__ __launch_bounds__(256) void gan_lrelu_bwd_kernel(const float* d, const float* g, const float* __restrict__ act, float slope,
                                                            long count, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float v = d && g ? d[e] + g[e] : (d ? d[e] : g[e]);
    out[e] = v * (act[e] > 0.f ? 1.f : slope);
}

// ------------------------------------------------------------------------------------------------
extern "C" int dvc_gan_conv4s2(const DvcConvDesc* d, const float* x, const float* w_bar, const float* bias, const float* inv_sigma,
                               float* y, dvcStream stream) {
    const char* fn = "dvc_gan_conv4s2";
    GanConvArgs a;
    if (gan_check_desc(fn, d, a)) return 1;
    DVC_REQUIRE(x && w_bar && bias && inv_sigma && y, "%s: null argument", fn);
    DVC_REQUIRE(((uintptr_t)w_bar & 15) == 0, "%s: w_bar must be 16-byte aligned", fn);
    const long tiles = cdivl(a.P, kGanN);
    DVC_REQUIRE(tiles <= kGanMaxBlocks && cdiv(a.Cout, kGanM) <= 65535, "%s: too many tiles for one launch", fn);
    a.x = x, a.w = w_bar, a.bias = bias, a.inv_sigma = inv_sigma, a.y = y;
    hipLaunchKernelGGL(gan_conv4s2_kernel, dim3((unsigned)tiles, cdiv(a.Cout, kGanM)), dim3(256), 0, (hipStream_t)stream, a);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_conv4s2_dgrad(const DvcConvDesc* d, const float* dz, const float* w_bar, const float* inv_sigma,
                                     const float* mask_act, float* dx, dvcStream stream) {
    const char* fn = "dvc_gan_conv4s2_dgrad";
    GanConvArgs a;
    if (gan_check_desc(fn, d, a)) return 1;
    DVC_REQUIRE(dz && w_bar && inv_sigma && dx, "%s: null argument", fn);
    const long tiles = cdivl((long)a.N * ((a.H + 1) / 2) * ((a.W + 1) / 2), kGanN);
    DVC_REQUIRE(tiles <= kGanMaxBlocks && cdiv(a.Cin, kGanM) <= 65535, "%s: too many tiles for one launch", fn);
    a.x = dz, a.w = w_bar, a.inv_sigma = inv_sigma, a.mask_act = mask_act, a.y = dx;
    hipLaunchKernelGGL(gan_conv4s2_dgrad_kernel, dim3((unsigned)tiles, cdiv(a.Cin, kGanM), 4), dim3(256), 0, (hipStream_t)stream, a);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_spectral_sigma(const float* w_bar, int32_t Cout, int32_t K, float eps, float* u, float* v, float* inv_sigma,
                                      void* workspace, size_t workspace_bytes, dvcStream stream) {
    const char* fn = "dvc_gan_spectral_sigma";
    DVC_REQUIRE(w_bar && u && v && inv_sigma, "%s: null argument", fn);
    DVC_REQUIRE(Cout >= 1 && K >= 1 && Cout <= 65535 * 16, "%s: bad shape (Cout %d, K %d)", fn, Cout, K);
    DVC_REQUIRE(eps >= 0.f, "%s: eps must not be negative", fn);
    const size_t need = ((size_t)K + (size_t)Cout) * sizeof(float);
    DVC_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", fn, workspace ? workspace_bytes : 0,
                need);
    DVC_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", fn);
    float* t = (float*)workspace;
    float* s = t + K;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gan_sn_wtu_kernel, dim3(cdiv(K, 64)), dim3(256), 0, st, w_bar, (const float*)u, t, Cout, K);
    hipLaunchKernelGGL(gan_sn_wv_kernel, dim3(Cout), dim3(256), 0, st, w_bar, (const float*)t, v, s, K, eps);
    hipLaunchKernelGGL(gan_sn_sigma_kernel, dim3(1), dim3(256), 0, st, (const float*)s, u, inv_sigma, Cout, eps);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_sn_weight(const float* w_bar, const float* inv_sigma, int32_t Cout, int32_t K, float* w_scaled,
                                 float* w_scaled_t, int32_t ldt, dvcStream stream) {
    const char* fn = "dvc_gan_sn_weight";
    DVC_REQUIRE(w_bar && inv_sigma && (w_scaled || w_scaled_t), "%s: null argument", fn);
    DVC_REQUIRE(Cout >= 1 && K >= 1, "%s: bad shape (Cout %d, K %d)", fn, Cout, K);
    DVC_REQUIRE(!w_scaled_t || ldt >= Cout, "%s: ldt (%d) is below Cout (%d)", fn, ldt, Cout);
    const long blocks = cdivl((long)Cout * K, 256);
    DVC_REQUIRE(blocks <= kGanMaxBlocks, "%s: matrix too large for one launch", fn);
    hipLaunchKernelGGL(gan_sn_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w_bar, inv_sigma, w_scaled,
                       w_scaled_t, Cout, K, ldt);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

static int gan_last_check(const char* fn, int N, int Cin, int H, int W) {
    DVC_REQUIRE(N >= 1 && Cin >= 1 && (long)Cin * 18 <= 0x7fffffffL, "%s: bad shape (N %d, Cin %d)", fn, N, Cin);
    DVC_REQUIRE(H >= 3 && W >= 6, "%s: the map (%d x %d) is smaller than the 3 x 6 filter", fn, H, W);
    return 0;
}

extern "C" int dvc_gan_last(const float* x, const float* w_bar, const float* bias, const float* inv_sigma, int32_t N, int32_t Cin,
                            int32_t H, int32_t W, int64_t x_batch_stride, float* out, dvcStream stream) {
    const char* fn = "dvc_gan_last";
    DVC_REQUIRE(x && w_bar && bias && inv_sigma && out, "%s: null argument", fn);
    if (gan_last_check(fn, N, Cin, H, W)) return 1;
    const long dense = (long)Cin * H * W;
    DVC_REQUIRE(x_batch_stride == 0 || x_batch_stride >= dense, "%s: x_batch_stride (%ld) is below Cin*H*W (%ld)", fn,
                (long)x_batch_stride, dense);
    hipLaunchKernelGGL(gan_last_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, x, w_bar, bias, inv_sigma, Cin, H, W,
                       x_batch_stride ? (long)x_batch_stride : dense, out);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_last_bwd(const float* g, const float* w_bar, const float* inv_sigma, const float* mask_act, float slope,
                                int32_t N, int32_t Cin, int32_t H, int32_t W, float* dx, dvcStream stream) {
    const char* fn = "dvc_gan_last_bwd";
    DVC_REQUIRE(g && w_bar && inv_sigma && dx, "%s: null argument", fn);
    if (gan_last_check(fn, N, Cin, H, W)) return 1;
    const long total = (long)N * Cin * H * W, blocks = cdivl(total, 256);
    DVC_REQUIRE(blocks <= kGanMaxBlocks, "%s: tensor too large for one launch", fn);
    hipLaunchKernelGGL(gan_last_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, w_bar, inv_sigma, mask_act,
                       slope, Cin, H, W, total, dx);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

static int gan_rows_check(const char* fn, int64_t rows, int P) {
    DVC_REQUIRE(rows >= 1 && P >= 1, "%s: bad shape (rows %ld, P %d)", fn, (long)rows, P);
    DVC_REQUIRE(cdivl(rows, 4) <= kGanMaxBlocks, "%s: too many rows for one launch", fn);
    return 0;
}

extern "C" int dvc_gan_softmax_rows(const float* e, int64_t rows, int32_t P, float* a, dvcStream stream) {
    const char* fn = "dvc_gan_softmax_rows";
    DVC_REQUIRE(e && a, "%s: null argument", fn);
    if (gan_rows_check(fn, rows, P)) return 1;
    hipLaunchKernelGGL(gan_softmax_rows_kernel, dim3((unsigned)cdivl(rows, 4)), dim3(256), 0, (hipStream_t)stream, e, (long)rows, P, a);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_softmax_rows_bwd(const float* a, const float* dA, int64_t rows, int32_t P, float* dE, dvcStream stream) {
    const char* fn = "dvc_gan_softmax_rows_bwd";
    DVC_REQUIRE(a && dA && dE, "%s: null argument", fn);
    if (gan_rows_check(fn, rows, P)) return 1;
    hipLaunchKernelGGL(gan_softmax_rows_bwd_kernel, dim3((unsigned)cdivl(rows, 4)), dim3(256), 0, (hipStream_t)stream, a, dA, (long)rows,
                       P, dE);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_scale_add(const float* o, const float* x, const float* gamma, int64_t count, float* y, dvcStream stream) {
    const char* fn = "dvc_gan_scale_add";
    DVC_REQUIRE(o && gamma && y, "%s: null argument", fn);
    DVC_REQUIRE(count >= 1 && cdivl(count, 256) <= kGanMaxBlocks, "%s: bad count (%ld)", fn, (long)count);
    hipLaunchKernelGGL(gan_scale_add_kernel, dim3((unsigned)cdivl(count, 256)), dim3(256), 0, (hipStream_t)stream, o, x, gamma,
                       (long)count, y);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_lrelu_bwd(const float* d, const float* g, const float* act, float slope, int64_t count, float* out,
                                 dvcStream stream) {
    const char* fn = "dvc_gan_lrelu_bwd";
    DVC_REQUIRE((d || g) && act && out, "%s: null argument", fn);
    DVC_REQUIRE(count >= 1 && cdivl(count, 256) <= kGanMaxBlocks, "%s: bad count (%ld)", fn, (long)count);
    hipLaunchKernelGGL(gan_lrelu_bwd_kernel, dim3((unsigned)cdivl(count, 256)), dim3(256), 0, (hipStream_t)stream, d, g, act, slope,
                       (long)count, out);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}
