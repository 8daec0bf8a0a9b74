// Flow warp (WarpingLayer, utils/warping.py: get_grid + F.grid_sample, bilinear, zeros padding), forward and backward, for
// gfx950.  x [B][C][H][W], flow [B][2][H][W] (channel 0 = u, the x displacement; channel 1 = v, the y displacement; pixels).
// Per output pixel p = (y, x), with X = x + u(p), Y = y + v(p):
//
//   align_corners = 1:  px = X,                      py = Y                        (sx = sy = 1)
//   align_corners = 0:  px = X W / (W - 1) - 0.5,    py = Y H / (H - 1) - 0.5      (sx = W / (W - 1), sy = H / (H - 1))
//   x0 = floor(px), fx = px - x0 (same in y);   out_c(p) = sum over the four corners of w x_c(corner),
//   w = (1-fy)(1-fx), (1-fy) fx, fy (1-fx), fy fx;  a corner outside [0, W-1] x [0, H-1] contributes 0.
//
// Backward for an incoming G:
//   dx_c(q) = sum_{p : q is an in-range corner of p} w G_c(p)                                          (a scatter)
//   du(p)   = sx sum_c G_c(p) [(1-fy)(x_c01 - x_c00) + fy (x_c11 - x_c10)],  dv(p) likewise in y       (a gather)
//
// Coordinates, weights and the per-pixel sums are double: x + u is then exact for every flow that matters (an integer flow
// gives fx = 0 exactly, so with align_corners = 1 the output is the shifted input bit for bit) and the result is rounded to
// fp32 once.  A non-finite coordinate gives NaN in every channel of that pixel, adds nothing to dx and gives a NaN dflow.  A
// finite coordinate is range-checked as a double BEFORE it is converted to an integer: px outside [-1, W) or py outside
// [-1, H) has no in-range corner, the pixel is zero and no address is formed from it.
//
// dx is bitwise reproducible and independent of the batch around the image: the scatter adds INTEGERS.  Per image,
// amax = max |G| (an integer max on the bit pattern of |G|: order-independent, and a NaN or inf sorts above every finite
// value), q = 2^(e - 40) with 2^e the smallest power of two above amax; each contribution is llrint(w G / q), |.| < 2^40,
// added with a 64-bit integer atomic into an int64 workspace [B][C][H][W]; a destination receives at most one corner from
// each of the H W <= 2^22 output pixels, so |acc| < 2^62; the last launch writes (float)(acc q).  Integer addition is
// associative: the arrival order of the atomics cannot change a bit.  Every contribution is within q / 2 of exact, so the
// error before the final rounding is below H W 2^-41 amax.  amax == 0 gives dx = 0, a non-finite amax a NaN dx for that image.
// Launches: forward 1.  Backward with dx: workspace memset, amax, scatter (+ dflow gather in the same pass), finish.
// Backward with dflow alone: 1.  grid (x tiles, y tiles, image), a wave = one 64-pixel row segment: coalesced dwords.
#include "common.h"

#include <cmath>
#include <cstdint>

#include "reduce.h"

#define FW_TW 64
#define FW_TH 4
#define FW_MAX_HW (1L << 22)
#define FW_AMAX_BLOCKS 64   // per image

// sample position of one output pixel: the top-left corner, the fractions, and which corners are inside the image
struct FwSample {
    int x0, y0;
    double fx, fy;
    bool finite;   // false: NaN / inf coordinate
    bool any;      // some corner may be in range (false: all four are outside, nothing is read or written)
};

__device__ __forceinline__ FwSample fw_sample(float u, float v, int x, int y, int H, int W, int align) {
    double px = (double)x + (double)u, py = (double)y + (double)v;
    if (!align) {
        px = px * ((double)W / (double)(W - 1)) - 0.5;
        py = py * ((double)H / (double)(H - 1)) - 0.5;
    }
    FwSample s;
    s.finite = __builtin_isfinite(px) && __builtin_isfinite(py);
    // the range check on the doubles comes before any conversion: a NaN compares false
    s.any = s.finite && px >= -1.0 && px < (double)W && py >= -1.0 && py < (double)H;
    s.x0 = s.y0 = 0;
    s.fx = s.fy = 0.0;
    if (s.any) {
        const double flx = floor(px), fly = floor(py);   // in [-1, W - 1], [-1, H - 1]
        s.x0 = (int)flx;
        s.y0 = (int)fly;
        s.fx = px - flx;
        s.fy = py - fly;
    }
    return s;
}

__global__ __launch_bounds__(256) void fw_fwd_kernel(const float* __restrict__ xin, const float* __restrict__ flow,
                                                     float* __restrict__ out, int C, int H, int W, int align) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * FW_TW + (threadIdx.x & (FW_TW - 1)), y = blockIdx.y * FW_TH + threadIdx.x / FW_TW;
    if (x >= W || y >= H) return;
    const long HW = (long)H * W, pix = (long)y * W + x;
    const float* fb = flow + (long)b * 2 * HW + pix;
    const FwSample s = fw_sample(fb[0], fb[HW], x, y, H, W, align);
    float* op = out + (long)b * C * HW + pix;
    if (!s.any) {
        const float fill = s.finite ? 0.f : __builtin_nanf("");
        for (int c = 0; c < C; ++c) op[(long)c * HW] = fill;
        return;
    }
    const int x1 = s.x0 + 1, y1 = s.y0 + 1;
    const bool inx0 = s.x0 >= 0, inx1 = x1 < W, iny0 = s.y0 >= 0, iny1 = y1 < H;
    const double w00 = (1.0 - s.fy) * (1.0 - s.fx), w01 = (1.0 - s.fy) * s.fx, w10 = s.fy * (1.0 - s.fx), w11 = s.fy * s.fx;
    const float* xb = xin + (long)b * C * HW;
    const long r0 = (long)s.y0 * W, r1 = (long)y1 * W;
    for (int c = 0; c < C; ++c) {
        const float* xc = xb + (long)c * HW;
        const double v00 = (iny0 && inx0) ? (double)xc[r0 + s.x0] : 0.0, v01 = (iny0 && inx1) ? (double)xc[r0 + x1] : 0.0;
        const double v10 = (iny1 && inx0) ? (double)xc[r1 + s.x0] : 0.0, v11 = (iny1 && inx1) ? (double)xc[r1 + x1] : 0.0;
        op[(long)c * HW] = (float)(w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11);
    }
}

// per image: amax_bits[2 b] = max over the image of the bit pattern of |G| (the word was zeroed on the stream before)
__global__ __launch_bounds__(256) void fw_amax_kernel(const float* __restrict__ G, long n, unsigned* __restrict__ amax_bits) {
    __shared__ unsigned red[4];
    const int b = blockIdx.y;
    const unsigned* g = reinterpret_cast<const unsigned*>(G) + (long)b * n;
    unsigned m = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = max(m, g[i] & 0x7fffffffu);
    m = block_tree_max4(wave_max(m), red);
    if (threadIdx.x == 0) atomicMax(amax_bits + 2 * b, m);
}

// 2^k as a double, k within the normal range
__device__ __forceinline__ double fw_pow2(int k) { return __longlong_as_double((long long)(k + 1023) << 52); }
// e with 2^e the smallest power of two above a finite amax given by its bits: amax < 2^(E - 126) for a biased exponent E
// (E = 0, the subnormals, included)
__device__ __forceinline__ int fw_exp_above(unsigned amax_bits) { return (int)(amax_bits >> 23) - 126; }

// the backward's pass over the output pixels: scatters the quantised w G into acc (dx wanted), gathers dflow (wanted)
template <bool WANT_DX, bool WANT_DF>
__global__ __launch_bounds__(256) void fw_bwd_kernel(const float* __restrict__ xin, const float* __restrict__ flow,
                                                     const float* __restrict__ G, long long* __restrict__ acc,
                                                     const unsigned* __restrict__ amax_bits, float* __restrict__ dflow, int C,
                                                     int H, int W, int align) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * FW_TW + (threadIdx.x & (FW_TW - 1)), y = blockIdx.y * FW_TH + threadIdx.x / FW_TW;
    if (x >= W || y >= H) return;
    const long HW = (long)H * W, pix = (long)y * W + x;
    const float* fb = flow + (long)b * 2 * HW + pix;
    const FwSample s = fw_sample(fb[0], fb[HW], x, y, H, W, align);
    float* dfp = WANT_DF ? dflow + (long)b * 2 * HW + pix : nullptr;
    if (!s.any) {
        if (WANT_DF) dfp[0] = dfp[HW] = s.finite ? 0.f : __builtin_nanf("");
        return;
    }
    bool scatter = WANT_DX;
    double inv_q = 0.0;
    if (WANT_DX) {
        const unsigned ab = amax_bits[2 * b];
        scatter = ab < 0x7f800000u;                      // a non-finite amax: the image's dx is NaN, nothing is added
        inv_q = fw_pow2(40 - fw_exp_above(ab));
    }
    const int x1 = s.x0 + 1, y1 = s.y0 + 1;
    const bool in00 = s.y0 >= 0 && s.x0 >= 0, in01 = s.y0 >= 0 && x1 < W, in10 = y1 < H && s.x0 >= 0, in11 = y1 < H && x1 < W;
    const double w00 = (1.0 - s.fy) * (1.0 - s.fx), w01 = (1.0 - s.fy) * s.fx, w10 = s.fy * (1.0 - s.fx), w11 = s.fy * s.fx;
    const long o00 = (long)s.y0 * W + s.x0, o01 = o00 + 1, o10 = o00 + W, o11 = o10 + 1;
    const float* xb = xin + (long)b * C * HW;
    const float* gp = G + (long)b * C * HW + pix;
    long long* ab_ = WANT_DX ? acc + (long)b * C * HW : nullptr;
    double du = 0.0, dv = 0.0;
    for (int c = 0; c < C; ++c) {
        const double g = (double)gp[(long)c * HW];
        if (WANT_DF) {
            const float* xc = xb + (long)c * HW;
            const double v00 = in00 ? (double)xc[o00] : 0.0, v01 = in01 ? (double)xc[o01] : 0.0;
            const double v10 = in10 ? (double)xc[o10] : 0.0, v11 = in11 ? (double)xc[o11] : 0.0;
            du += g * ((1.0 - s.fy) * (v01 - v00) + s.fy * (v11 - v10));
            dv += g * ((1.0 - s.fx) * (v10 - v00) + s.fx * (v11 - v01));
        }
        if (WANT_DX && scatter) {
            long long* ac = ab_ + (long)c * HW;
            const double gq = g * inv_q;   // exact: a power of two, |gq| < 2^40
            const long long k00 = llrint(w00 * gq), k01 = llrint(w01 * gq), k10 = llrint(w10 * gq), k11 = llrint(w11 * gq);
            // zero adds nothing: skipping it is as deterministic as adding it
            if (in00 && k00) __hip_atomic_fetch_add(ac + o00, k00, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (in01 && k01) __hip_atomic_fetch_add(ac + o01, k01, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (in10 && k10) __hip_atomic_fetch_add(ac + o10, k10, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (in11 && k11) __hip_atomic_fetch_add(ac + o11, k11, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (WANT_DF) {
        const double sx = align ? 1.0 : (double)W / (double)(W - 1), sy = align ? 1.0 : (double)H / (double)(H - 1);
        dfp[0] = (float)(sx * du);
        dfp[HW] = (float)(sy * dv);
    }
}

// dx = (float)(acc q), per image; grid (blocks over C H W, image)
__global__ __launch_bounds__(256) void fw_finish_kernel(const long long* __restrict__ acc, const unsigned* __restrict__ amax_bits,
                                                        float* __restrict__ dx, long n) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned ab = amax_bits[2 * b];
    float r;
    if (ab >= 0x7f800000u) {
        r = __builtin_nanf("");
    } else {
        // the conversion of |acc| < 2^62 to double rounds at 2^-53 relative, far below the fp32 rounding that follows
        r = (float)((double)acc[(long)b * n + i] * fw_pow2(fw_exp_above(ab) - 40));
    }
    dx[(long)b * n + i] = r;
}

// ------------------------------------------------------------------------------------------------
static int fw_check(const char* fn, const float* x, const float* flow, int32_t B, int32_t C, int32_t H, int32_t W,
                    int32_t align_corners) {
    DVC_REQUIRE(x && flow, "%s: null argument", fn);
    DVC_REQUIRE(B >= 1 && C >= 1, "%s: bad shape (B %d, C %d)", fn, B, C);
    DVC_REQUIRE(H >= 2 && W >= 2, "%s: H and W must be at least 2 (got %d x %d): the grid divides by (W - 1) / 2", fn, H, W);
    DVC_REQUIRE((long)H * W <= FW_MAX_HW, "%s: H * W is above 2^22 (got %d x %d)", fn, H, W);
    DVC_REQUIRE(align_corners == 0 || align_corners == 1, "%s: align_corners must be 0 or 1 (got %d)", fn, align_corners);
    DVC_REQUIRE(B <= 65535 && cdiv(H, FW_TH) <= 65535 && (long)C * H * W <= (1L << 31), "%s: map or batch too large for one launch",
                fn);
    return 0;
}

static size_t fw_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    return ((size_t)B * (size_t)C * (size_t)H * (size_t)W + (size_t)B) * 8;   // acc [B][C][H][W] int64, then 8 bytes per image
}

extern "C" size_t dvc_flow_warp_bwd_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B < 1 || C < 1 || H < 2 || W < 2 || (long)H * W > FW_MAX_HW) return 0;
    return fw_workspace_bytes(B, C, H, W);
}

extern "C" int dvc_flow_warp_fwd(const float* x, const float* flow, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t align_corners, float* y, dvcStream stream) {
    if (fw_check("dvc_flow_warp_fwd", x, flow, B, C, H, W, align_corners)) return 1;
    DVC_REQUIRE(y, "dvc_flow_warp_fwd: null argument");
    hipLaunchKernelGGL(fw_fwd_kernel, dim3(cdiv(W, FW_TW), cdiv(H, FW_TH), B), dim3(256), 0, (hipStream_t)stream, x, flow, y, C, H,
                       W, align_corners);
    DVC_CHECK_LAUNCH("dvc_flow_warp_fwd");
    return 0;
}

extern "C" int dvc_flow_warp_bwd(const float* x, const float* flow, const float* G, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t align_corners, float* dx, float* dflow, void* workspace, size_t workspace_bytes,
                                 dvcStream stream) {
    if (fw_check("dvc_flow_warp_bwd", x, flow, B, C, H, W, align_corners)) return 1;
    DVC_REQUIRE(G, "dvc_flow_warp_bwd: null argument");
    DVC_REQUIRE(dx || dflow, "dvc_flow_warp_bwd: neither dx nor dflow is wanted");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(W, FW_TW), cdiv(H, FW_TH), B);
    if (!dx) {
        hipLaunchKernelGGL((fw_bwd_kernel<false, true>), grid, dim3(256), 0, s, x, flow, G, (long long*)nullptr,
                           (const unsigned*)nullptr, dflow, C, H, W, align_corners);
        DVC_CHECK_LAUNCH("dvc_flow_warp_bwd");
        return 0;
    }
    const size_t need = fw_workspace_bytes(B, C, H, W);
    DVC_REQUIRE(workspace, "dvc_flow_warp_bwd: dx needs a workspace of %zu bytes (got NULL)", need);
    DVC_REQUIRE(workspace_bytes >= need, "dvc_flow_warp_bwd: workspace too small (%zu bytes, dx needs %zu)", workspace_bytes, need);
    DVC_REQUIRE(((uintptr_t)workspace & 7) == 0, "dvc_flow_warp_bwd: workspace must be 8-byte aligned");
    const long n = (long)C * H * W;
    long long* acc = (long long*)workspace;
    unsigned* amax_bits = (unsigned*)(acc + (long)B * n);
    DVC_REQUIRE(hipMemsetAsync(workspace, 0, need, s) == hipSuccess, "dvc_flow_warp_bwd: zeroing the workspace failed");
    const int ablocks = (int)std::min<long>(FW_AMAX_BLOCKS, cdivl(n, 256));
    hipLaunchKernelGGL(fw_amax_kernel, dim3(ablocks, B), dim3(256), 0, s, G, n, amax_bits);
    if (dflow)
        hipLaunchKernelGGL((fw_bwd_kernel<true, true>), grid, dim3(256), 0, s, x, flow, G, acc, amax_bits, dflow, C, H, W,
                           align_corners);
    else
        hipLaunchKernelGGL((fw_bwd_kernel<true, false>), grid, dim3(256), 0, s, x, flow, G, acc, amax_bits, (float*)nullptr, C, H,
                           W, align_corners);
    hipLaunchKernelGGL(fw_finish_kernel, dim3((unsigned)cdivl(n, 256), B), dim3(256), 0, s, acc, amax_bits, dx, n);
    DVC_CHECK_LAUNCH("dvc_flow_warp_bwd");
    return 0;
}
