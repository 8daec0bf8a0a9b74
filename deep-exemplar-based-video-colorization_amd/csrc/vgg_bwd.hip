// Input gradient of the frozen VGG19 (train.py trains THROUGH it: the perceptual and contextual losses are taken on the
// features of the predicted frame) and of tensor_lab2rgb.  The 3x3 convolutions' input gradients run on the forward's engines
// (dvc_amd/nets.py: a stride-1 pad-1 3x3 convolution's input gradient is the same convolution with W^T flipped); what is here is
// what those engines do not do:
//   dvc_vgg_act_bwd       dZ = (dX [+ g]) * [R > 0]                                    between two convolutions
//   dvc_vgg_pool_act_bwd  dZ = (route(dP [+ gP]) [+ gR]) * [R > 0]                     where a 2x2 pool sits between them
//   dvc_vgg_conv1_bwd     conv1_1's input gradient (3 output channels; vgg_preprocess folded into the filters)
//   dvc_lab2rgb_bwd       tensor_lab2rgb's gradient, the forward's arithmetic recomputed (color.hip)
// The masks and routes are ATen's: threshold_backward(grad, relu_out, 0) passes where NOT out <= 0; max_pool2d's backward sends
// the window's gradient to the first element in scan order that satisfies v > max || isnan(v).  All deterministic.
#include "common.h"

namespace {

__device__ __forceinline__ float relu_mask(float g, float r) { return r <= 0.f ? 0.f : g; }

// ATen's max_pool2d scan (aten/src/ATen/native/cpu/MaxPoolKernel.cpp): start from (-inf, first element), take every element with
// v > max || isnan(v) — ties keep the first maximum, a NaN takes the window (the last NaN when there are several)
__device__ __forceinline__ int argmax4(const float v[4]) {
    int am = 0;
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k] > mx || isnan(v[k])) {
            mx = v[k];
            am = k;
        }
    return am;
}

// ------------------------------------------------------------------------------------------------ activation backward
// float4 pieces, four in flight per thread; dX / g may be null (not both).  dZ may be dX (in place: each lane reads its pieces
// before it writes them), hence no __restrict__ on those two.
constexpr int kActU = 4;
__global__ __launch_bounds__(256) void act_bwd_vec_kernel(const float* dX, const float* __restrict__ g,
                                                          const float* __restrict__ R, long n4, float* dZ) {
    const long nt = (long)gridDim.x * 256;
    const float4* x4 = reinterpret_cast<const float4*>(dX);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const float4* r4 = reinterpret_cast<const float4*>(R);
    float4* z4 = reinterpret_cast<float4*>(dZ);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += nt * kActU) {
        float4 a[kActU], b[kActU], r[kActU];
#pragma unroll
        for (int u = 0; u < kActU; ++u) {
            const long j = i + u * nt;
            const bool in = j < n4;
            a[u] = (in && x4) ? x4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            b[u] = (in && g4) ? g4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            r[u] = in ? r4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kActU; ++u) {
            const long j = i + u * nt;
            if (j < n4) {
                // (one of the two terms alone is passed unchanged: x + 0 would turn -0 into +0)
                float4 s = !x4 ? b[u] : !g4 ? a[u]
                                            : make_float4(a[u].x + b[u].x, a[u].y + b[u].y, a[u].z + b[u].z, a[u].w + b[u].w);
                z4[j] = make_float4(relu_mask(s.x, r[u].x), relu_mask(s.y, r[u].y), relu_mask(s.z, r[u].z), relu_mask(s.w, r[u].w));
            }
        }
    }
}

__global__ __launch_bounds__(256) void act_bwd_scalar_kernel(const float* dX, const float* __restrict__ g,
                                                             const float* __restrict__ R, long n, float* dZ) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float s = !dX ? g[i] : !g ? dX[i] : dX[i] + g[i];
        dZ[i] = relu_mask(s, R[i]);
    }
}

// ------------------------------------------------------------------------------------------------ pool + activation backward
// One thread per 2x2 cell of the full-resolution plane (ceil(H/2) x ceil(W/2) cells: with odd H or W the last row / column of
// cells is partial and lies outside every pooling window, floor mode — it gets gR * mask only).  VEC: W even and the plane
// rows 8-byte aligned, the cell's two rows move as float2.
template <bool VEC>
__global__ __launch_bounds__(256) void pool_act_bwd_kernel(const float* __restrict__ dP, const float* __restrict__ gP,
                                                           const float* __restrict__ gR, const float* __restrict__ R, int H,
                                                           int W, int avg, long cells_total, float* __restrict__ dZ) {
    const int OH = H >> 1, OW = W >> 1, CH = (H + 1) >> 1, CW = (W + 1) >> 1;
    const long per_plane = (long)CH * CW;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < cells_total; t += (long)gridDim.x * 256) {
        const long plane = t / per_plane;
        const int c = (int)(t - plane * per_plane);
        const int cy = c / CW, cx = c - cy * CW;
        const int y0 = 2 * cy, x0 = 2 * cx;
        const long base = plane * H * W + (long)y0 * W + x0;
        const bool full = cy < OH && cx < OW;
        if (VEC && full) {
            const float2 r0 = *reinterpret_cast<const float2*>(R + base), r1 = *reinterpret_cast<const float2*>(R + base + W);
            float2 e0 = make_float2(0.f, 0.f), e1 = make_float2(0.f, 0.f);
            if (gR) {
                e0 = *reinterpret_cast<const float2*>(gR + base);
                e1 = *reinterpret_cast<const float2*>(gR + base + W);
            }
            const long pi = plane * OH * OW + (long)cy * OW + cx;
            float p = 0.f;
            const bool routed = dP || gP;
            if (routed) p = !dP ? gP[pi] : !gP ? dP[pi] : dP[pi] + gP[pi];
            float q[4] = {0.f, 0.f, 0.f, 0.f};
            if (routed) {
                if (avg) {
                    const float v = p / 4.f;
                    q[0] = q[1] = q[2] = q[3] = v;
                } else {
                    const float v[4] = {r0.x, r0.y, r1.x, r1.y};
                    q[argmax4(v)] = p;
                }
            }
            // the pooled gradient and gR are both present: (routed + gR); one alone passes unchanged
            const float ev[4] = {e0.x, e0.y, e1.x, e1.y};
            const float rv[4] = {r0.x, r0.y, r1.x, r1.y};
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = !routed ? ev[k] : !gR ? q[k] : q[k] + ev[k];
                o[k] = relu_mask(s, rv[k]);
            }
            *reinterpret_cast<float2*>(dZ + base) = make_float2(o[0], o[1]);
            *reinterpret_cast<float2*>(dZ + base + W) = make_float2(o[2], o[3]);
            continue;
        }
        // scalar path: partial cells, and every cell when !VEC
        const long pi = plane * OH * OW + (long)cy * OW + cx;
        const bool routed = full && (dP || gP);
        float p = 0.f;
        if (routed) p = !dP ? gP[pi] : !gP ? dP[pi] : dP[pi] + gP[pi];
        int am = -1;
        if (routed && !avg) {
            const float v[4] = {R[base], R[base + 1], R[base + W], R[base + W + 1]};
            am = argmax4(v);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dy = k >> 1, dx = k & 1;
            if (y0 + dy >= H || x0 + dx >= W) continue;
            const long e = base + (long)dy * W + dx;
            float q = 0.f;
            if (routed) q = avg ? p / 4.f : (k == am ? p : 0.f);
            const float s = !routed ? (gR ? gR[e] : 0.f) : !gR ? q : q + gR[e];
            dZ[e] = relu_mask(s, R[e]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ conv1_1 input gradient
// dx[n][c][y][x] = sum_{ci, kh, kw} dZ[n][ci][y + kh - 1][x + kw - 1] * wt[c][ci][kh][kw]   (c < 3, zero padding)
// A 16 x 16 tile of output pixels per workgroup, one pixel (all three channels) per thread; 8 input channels at a time are
// staged as 18 x 18 halo tiles in LDS, the whole filter set [3][C][9] lives in LDS.  Fixed summation order (ci, kh, kw).
constexpr int kC1Tile = 16, kC1Halo = kC1Tile + 2, kC1Stage = 8, kC1MaxC = 256;
__global__ __launch_bounds__(256) void conv1_bwd_kernel(const float* __restrict__ dZ, const float* __restrict__ wt, int C, int H,
                                                        int W, int tiles_x, float* __restrict__ dx) {
    __shared__ float s_w[3 * kC1MaxC * 9];
    __shared__ float s_in[kC1Stage][kC1Halo][kC1Halo + 1];
    const int n = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * kC1Tile, tx0 = (blockIdx.x % tiles_x) * kC1Tile;
    const int tid = threadIdx.x, ly = tid / kC1Tile, lx = tid % kC1Tile;
    for (int i = tid; i < 3 * C * 9; i += 256) s_w[i] = wt[i];
    const long HW = (long)H * W;
    const float* zn = dZ + (long)n * C * HW;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    for (int c0 = 0; c0 < C; c0 += kC1Stage) {
        __syncthreads();
        for (int i = tid; i < kC1Stage * kC1Halo * kC1Halo; i += 256) {
            const int s = i / (kC1Halo * kC1Halo), r = i - s * kC1Halo * kC1Halo;
            const int hy = r / kC1Halo, hx = r - hy * kC1Halo;
            const int y = ty0 + hy - 1, x = tx0 + hx - 1;
            s_in[s][hy][hx] = (y >= 0 && y < H && x >= 0 && x < W) ? zn[(long)(c0 + s) * HW + (long)y * W + x] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kC1Stage; ++s) {
            const float* w0 = s_w + (0 * C + c0 + s) * 9;
            const float* w1 = s_w + (1 * C + c0 + s) * 9;
            const float* w2 = s_w + (2 * C + c0 + s) * 9;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float v = s_in[s][ly + kh][lx + kw];
                    acc0 = fmaf(v, w0[kh * 3 + kw], acc0);
                    acc1 = fmaf(v, w1[kh * 3 + kw], acc1);
                    acc2 = fmaf(v, w2[kh * 3 + kw], acc2);
                }
        }
    }
    const int y = ty0 + ly, x = tx0 + lx;
    if (y < H && x < W) {
        float* o = dx + (long)n * 3 * HW + (long)y * W + x;
        o[0] = acc0;
        o[HW] = acc1;
        o[2 * HW] = acc2;
    }
}

// ------------------------------------------------------------------------------------------------ tensor_lab2rgb backward
// The forward (color.hip lab2rgb_kernel) recomputed with the same float arithmetic, so that every branch test sees the value the
// forward saw; then ATen's derivatives of the reference's composition (oracle/dvc_oracle.py tensor_lab2rgb):
//   clamp(0, 1): passes where 0 <= v <= 1 (pre-clamp value, inclusive);  gamma: 1.055 / 2.4 * v^(1/2.4 - 1) or 12.92;
//   M^T and the white point;  cube: 3 v^2 or 1 / 7.787;  z clamp(min=0): passes where fz >= 0;
//   dL = (dfx + dfy + dfz) / 116, da = dfx / 500, db = -dfz / 200.
__global__ __launch_bounds__(256) void lab2rgb_bwd_kernel(const float* __restrict__ lab, long HW, float l_offset,
                                                          const float* __restrict__ grad_rgb, float* __restrict__ grad_lab) {
    const int n = blockIdx.y;
    const float* in = lab + (long)n * 3 * HW;
    const float* go = grad_rgb + (long)n * 3 * HW;
    float* gi = grad_lab + (long)n * 3 * HW;
    const float M[3][3] = {{3.24048134f, -0.96925495f, 0.05564664f},
                           {-1.53715152f, 1.87599f, -0.20404134f},
                           {-0.49853633f, 0.04155593f, 1.05731107f}};
    const float white[3] = {0.95047f, 1.0f, 1.08883f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
        float L = in[i] + l_offset, a = in[HW + i], b = in[2 * HW + i];
        float fy = (L + 16.0f) / 116.0f;
        float fx = (a / 500.0f) + fy;
        float fz_pre = fy - (b / 200.0f);
        float fz = fz_pre < 0.f ? 0.f : fz_pre;
        const float f[3] = {fx, fy, fz};
        float xyz[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = f[k];
            xyz[k] = v > 0.2068966f ? v * v * v : (v - 16.0f / 116.0f) / 7.787f;
        }
        xyz[0] *= 0.95047f;
        xyz[2] *= 1.08883f;
        float drgb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = xyz[0] * M[0][k] + xyz[1] * M[1][k] + xyz[2] * M[2][k];
            const bool gam = v > 0.0031308f;
            float o = gam ? 1.055f * powf(v, 1.0f / 2.4f) - 0.055f : v * 12.92f;
            const float g = go[k * HW + i];
            const float gc = (o >= 0.f && o <= 1.f) ? g : 0.f;
            drgb[k] = gam ? gc * (1.055f * ((1.0f / 2.4f) * powf(v, 1.0f / 2.4f - 1.0f))) : gc * 12.92f;
        }
        float df[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float dlin = (drgb[0] * M[j][0] + drgb[1] * M[j][1] + drgb[2] * M[j][2]) * white[j];
            const float v = f[j];
            df[j] = v > 0.2068966f ? dlin * (3.0f * v * v) : dlin / 7.787f;
        }
        const float dfz = fz_pre >= 0.f ? df[2] : 0.f;
        gi[i] = (df[0] + df[1] + dfz) / 116.0f;
        gi[HW + i] = df[0] / 500.0f;
        gi[2 * HW + i] = -dfz / 200.0f;
    }
}

int grid_for(long work, long per_block) {
    long g = (work + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

}  // namespace

extern "C" int dvc_vgg_act_bwd(const float* dX, const float* g, const float* R, int64_t n, float* dZ, dvcStream stream) {
    DVC_REQUIRE(R && dZ && n > 0, "dvc_vgg_act_bwd: bad argument (R, dZ and n > 0 are required)");
    DVC_REQUIRE(dX || g, "dvc_vgg_act_bwd: dX and g are both null");
    DVC_REQUIRE(dZ != R && (!g || dZ != g), "dvc_vgg_act_bwd: dZ may alias dX only");
    auto al = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (n % 4 == 0 && al(dX) && al(g) && al(R) && al(dZ)) {
        const long n4 = n / 4;
        hipLaunchKernelGGL(act_bwd_vec_kernel, dim3(grid_for(n4, 256L * kActU)), dim3(256), 0, (hipStream_t)stream, dX, g, R, n4,
                           dZ);
    } else {
        hipLaunchKernelGGL(act_bwd_scalar_kernel, dim3(grid_for(n, 1024)), dim3(256), 0, (hipStream_t)stream, dX, g, R, (long)n,
                           dZ);
    }
    DVC_CHECK_LAUNCH("dvc_vgg_act_bwd");
    return 0;
}

extern "C" int dvc_vgg_pool_act_bwd(const float* dP, const float* gP, const float* gR, const float* R, int32_t planes, int32_t H,
                                    int32_t W, int32_t pool_mode, float* dZ, dvcStream stream) {
    DVC_REQUIRE(R && dZ && planes > 0 && H >= 2 && W >= 2, "dvc_vgg_pool_act_bwd: bad argument (R, dZ, planes > 0, H, W >= 2)");
    DVC_REQUIRE(pool_mode == DVC_POOL_MAX || pool_mode == DVC_POOL_AVG, "dvc_vgg_pool_act_bwd: pool_mode must be 0 (max) or 1 (avg)");
    DVC_REQUIRE(dP || gP || gR, "dvc_vgg_pool_act_bwd: no incoming gradient (dP, gP and gR are all null)");
    DVC_REQUIRE(dZ != R && dZ != gR && dZ != dP && dZ != gP, "dvc_vgg_pool_act_bwd: dZ must not alias an input");
    const long cells = (long)planes * ((H + 1) / 2) * ((W + 1) / 2);
    auto al = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
    const bool vec = W % 2 == 0 && al(R) && al(gR) && al(dZ);
    if (vec)
        hipLaunchKernelGGL(pool_act_bwd_kernel<true>, dim3(grid_for(cells, 1024)), dim3(256), 0, (hipStream_t)stream, dP, gP, gR, R,
                           (int)H, (int)W, pool_mode == DVC_POOL_AVG ? 1 : 0, cells, dZ);
    else
        hipLaunchKernelGGL(pool_act_bwd_kernel<false>, dim3(grid_for(cells, 1024)), dim3(256), 0, (hipStream_t)stream, dP, gP, gR,
                           R, (int)H, (int)W, pool_mode == DVC_POOL_AVG ? 1 : 0, cells, dZ);
    DVC_CHECK_LAUNCH("dvc_vgg_pool_act_bwd");
    return 0;
}

extern "C" int dvc_vgg_conv1_bwd(const float* dZ, const float* w_t, int32_t N, int32_t C, int32_t H, int32_t W, float* dx,
                                 dvcStream stream) {
    DVC_REQUIRE(dZ && w_t && dx && N > 0 && H > 0 && W > 0, "dvc_vgg_conv1_bwd: bad argument");
    DVC_REQUIRE(C > 0 && C % kC1Stage == 0 && C <= kC1MaxC, "dvc_vgg_conv1_bwd: C must be a multiple of %d, at most %d (got %d)",
                kC1Stage, kC1MaxC, C);
    DVC_REQUIRE(N <= 65535, "dvc_vgg_conv1_bwd: N must be <= 65535");
    const int tx = cdiv(W, kC1Tile), ty = cdiv(H, kC1Tile);
    DVC_REQUIRE((long)tx * ty < (1L << 31), "dvc_vgg_conv1_bwd: image too large");
    hipLaunchKernelGGL(conv1_bwd_kernel, dim3(tx * ty, N), dim3(256), 0, (hipStream_t)stream, dZ, w_t, (int)C, (int)H, (int)W, tx,
                       dx);
    DVC_CHECK_LAUNCH("dvc_vgg_conv1_bwd");
    return 0;
}

extern "C" int dvc_lab2rgb_bwd(const float* lab, int32_t N, int32_t HW, float l_offset, const float* grad_rgb, float* grad_lab,
                               dvcStream stream) {
    DVC_REQUIRE(lab && grad_rgb && grad_lab && N > 0 && HW > 0, "dvc_lab2rgb_bwd: bad argument");
    DVC_REQUIRE(N <= 65535, "dvc_lab2rgb_bwd: N must be <= 65535");
    DVC_REQUIRE(grad_lab != lab && grad_lab != grad_rgb, "dvc_lab2rgb_bwd: grad_lab must not alias an input");
    hipLaunchKernelGGL(lab2rgb_bwd_kernel, dim3(cdiv(HW, 1024), N), dim3(256), 0, (hipStream_t)stream, lab, (long)HW, l_offset,
                       grad_rgb, grad_lab);
    DVC_CHECK_LAUNCH("dvc_lab2rgb_bwd");
    return 0;
}
