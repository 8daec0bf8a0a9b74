// Local weighted average (WeightedAverage_color, models/NonlocalNet.py; find_local_patch :12-17), forward and backward, for
// gfx950.  With r = k / 2, g = (L + l_offset, a, b) of the nearest-resized x_lab and v = (a', b') of the prediction, both ZERO
// outside the image (the offset is applied before the zero padding), per pixel p and offset d in [-r, r]^2 (dy major):
//
//   D_d(p) = |g(p + d) - g(p)|^2     s_d = exp(-D_d / alpha)     Z = sum_d s_d (all k*k offsets)     w_d = s_d / Z
//   y_c(p) = sum_d w_d(p) v_c(p + d)
//
// The centre offset has D = 0: the softmax's largest argument is exactly 0, so nothing is shifted and no alpha > 0 overflows.
// Backward for an incoming G, both gradients in gather form (no atomics, fixed order):
//
//   dv_c(q)  = sum_{d : q-d inside} w_d(q-d) G_c(q-d)
//   t_d(p)   = sum_c G_c(p) (v_c(p+d) - y_c(p))          e_d(p) = -(1/alpha) w_d(p) t_d(p)
//   dg_ch(q) = sum_{d : q-d inside} 2 (g_ch(q) - g_ch(q-d)) e_d(q-d)  -  sum_{all d} 2 (g_ch(q+d) - g_ch(q)) e_d(q)
//
// One launch each.  A workgroup of 256 threads owns an 8 x 32 pixel tile, one pixel per thread (a wave covers two rows of
// 32: 128-byte row segments in global memory, conflict-free rows in the LDS); the planes it needs are staged in the LDS with
// their halo, zero-filled outside the image, the nearest resize of x_lab folded into the tile load.  The backward needs
// 1 / Z on the tile + halo r: it is recomputed from a guide tile with halo 2r by the forward's own summation, then G, y and
// 1 / Z (all zero outside the image, which drops the "q-d outside" terms without a branch) on halo r give both gradients.
// Nothing k*k-times unfolded exists anywhere; there is no workspace.  grid (x tiles, y tiles, image): an image's result
// does not depend on the batch it came in.
#include "common.h"

#include <cfloat>
#include <cmath>

#define LW_TW 32
#define LW_TH 8
#define LW_MAX_K 7

// the weight numerator of neighbour n seen from centre g: exp(-|n - g|^2 / alpha) as exp2(-D c), c = log2(e) / alpha
__device__ __forceinline__ float lwa_s(float g0, float g1, float g2, float n0, float n1, float n2, float c) {
    const float d0 = n0 - g0, d1 = n1 - g1, d2 = n2 - g2;
    const float D = fmaf(d2, d2, fmaf(d1, d1, d0 * d0));
    return __builtin_amdgcn_exp2f(-(D * c));
}

// guide tile with halo HALO: s[3][LH][LWD], (L + l_offset, a, b) of the nearest-resized x_lab, zero outside the image
template <int HALO>
__device__ __forceinline__ void lwa_load_guide(float* __restrict__ s, const float* __restrict__ xb, int Hx, int Wx, float sxh,
                                               float sxw, int H, int W, int y0, int x0, float l_offset) {
    constexpr int LH = LW_TH + 2 * HALO, LWD = LW_TW + 2 * HALO;
    const long plane = (long)Hx * Wx;
    for (int e = threadIdx.x; e < LH * LWD; e += 256) {
        const int ly = e / LWD, lx = e - ly * LWD;
        const int y = y0 - HALO + ly, x = x0 - HALO + lx;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int sy = min((int)floorf((float)y * sxh), Hx - 1), sx = min((int)floorf((float)x * sxw), Wx - 1);
            const float* src = xb + (long)sy * Wx + sx;
            g0 = src[0] + l_offset;
            g1 = src[plane];
            g2 = src[2 * plane];
        }
        s[e] = g0;
        s[LH * LWD + e] = g1;
        s[2 * LH * LWD + e] = g2;
    }
}

// two consecutive [H][W] planes with halo HALO: s[2][LH][LWD], zero outside the image
template <int HALO>
__device__ __forceinline__ void lwa_load_pair(float* __restrict__ s, const float* __restrict__ src, int H, int W, int y0, int x0) {
    constexpr int LH = LW_TH + 2 * HALO, LWD = LW_TW + 2 * HALO;
    const long plane = (long)H * W;
    for (int e = threadIdx.x; e < LH * LWD; e += 256) {
        const int ly = e / LWD, lx = e - ly * LWD;
        const int y = y0 - HALO + ly, x = x0 - HALO + lx;
        float a = 0.f, b = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const float* p = src + (long)y * W + x;
            a = p[0];
            b = p[plane];
        }
        s[e] = a;
        s[LH * LWD + e] = b;
    }
}

struct LwaArgs {
    const float* x_lab;   // [B][Cx][Hx][Wx]
    const float* pred;    // [B][Cp][H][W], channels ab_ch, ab_ch + 1 are read
    const float* G;       // [B][2][H][W]   (backward)
    const float* y_in;    // [B][2][H][W]   (backward: the forward's output)
    float* y;             // [B][2][H][W]   (forward)
    float* dv;            // [B][2][H][W]   (backward)
    float* dg;            // [B][3][H][W] or NULL (backward)
    int Cx, Hx, Wx, Cp, ab_ch, H, W;
    float sxh, sxw, l_offset, c, inv_alpha;
};

template <int R>
__global__ __launch_bounds__(256) void lwa_fwd_kernel(LwaArgs a) {
    constexpr int LH = LW_TH + 2 * R, LWD = LW_TW + 2 * R, LP = LH * LWD;
    __shared__ float sg[3 * LP];
    __shared__ float sv[2 * LP];
    const int b = blockIdx.z, y0 = blockIdx.y * LW_TH, x0 = blockIdx.x * LW_TW;
    const int H = a.H, W = a.W;
    const long HW = (long)H * W;
    lwa_load_guide<R>(sg, a.x_lab + (long)b * a.Cx * a.Hx * a.Wx, a.Hx, a.Wx, a.sxh, a.sxw, H, W, y0, x0, a.l_offset);
    lwa_load_pair<R>(sv, a.pred + ((long)b * a.Cp + a.ab_ch) * HW, H, W, y0, x0);
    __syncthreads();
    const int tx = threadIdx.x & (LW_TW - 1), ty = threadIdx.x / LW_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    const int ctr = (ty + R) * LWD + tx + R;
    const float g0 = sg[ctr], g1 = sg[LP + ctr], g2 = sg[2 * LP + ctr];
    float Z = 0.f, acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int n = ctr + dy * LWD + dx;
            const float s = lwa_s(g0, g1, g2, sg[n], sg[LP + n], sg[2 * LP + n], a.c);
            Z += s;
            acc0 = fmaf(s, sv[n], acc0);
            acc1 = fmaf(s, sv[LP + n], acc1);
        }
    float* yp = a.y + (long)b * 2 * HW + (long)y * W + x;
    yp[0] = acc0 / Z;
    yp[HW] = acc1 / Z;
}

template <int R>
__global__ __launch_bounds__(256) void lwa_bwd_kernel(LwaArgs a) {
    constexpr int GH = LW_TH + 4 * R, GW = LW_TW + 4 * R, GP = GH * GW;   // guide: halo 2R
    constexpr int LH = LW_TH + 2 * R, LWD = LW_TW + 2 * R, LP = LH * LWD;  // everything else: halo R
    __shared__ float sg[3 * GP];
    __shared__ float sv[2 * LP];
    __shared__ float sG[2 * LP];
    __shared__ float sy[2 * LP];
    __shared__ float siz[LP];
    const int b = blockIdx.z, y0 = blockIdx.y * LW_TH, x0 = blockIdx.x * LW_TW;
    const int H = a.H, W = a.W;
    const long HW = (long)H * W;
    const bool want_dg = a.dg != nullptr;
    lwa_load_guide<2 * R>(sg, a.x_lab + (long)b * a.Cx * a.Hx * a.Wx, a.Hx, a.Wx, a.sxh, a.sxw, H, W, y0, x0, a.l_offset);
    lwa_load_pair<R>(sG, a.G + (long)b * 2 * HW, H, W, y0, x0);
    if (want_dg) {
        lwa_load_pair<R>(sv, a.pred + ((long)b * a.Cp + a.ab_ch) * HW, H, W, y0, x0);
        lwa_load_pair<R>(sy, a.y_in + (long)b * 2 * HW, H, W, y0, x0);
    }
    __syncthreads();
    // 1 / Z on the tile + halo R, the forward's summation; 0 outside the image
    for (int e = threadIdx.x; e < LP; e += 256) {
        const int ly = e / LWD, lx = e - ly * LWD;
        const int yy = y0 - R + ly, xx = x0 - R + lx;
        float iz = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const int ctr = (ly + R) * GW + lx + R;
            const float g0 = sg[ctr], g1 = sg[GP + ctr], g2 = sg[2 * GP + ctr];
            float Z = 0.f;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy)
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const int n = ctr + dy * GW + dx;
                    Z += lwa_s(g0, g1, g2, sg[n], sg[GP + n], sg[2 * GP + n], a.c);
                }
            iz = 1.f / Z;
        }
        siz[e] = iz;
    }
    __syncthreads();
    const int tx = threadIdx.x & (LW_TW - 1), ty = threadIdx.x / LW_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    const int gq = (ty + 2 * R) * GW + tx + 2 * R, lq = (ty + R) * LWD + tx + R;
    const float q0 = sg[gq], q1 = sg[GP + gq], q2 = sg[2 * GP + gq];
    float dv0 = 0.f, dv1 = 0.f;
    if (!want_dg) {
#pragma unroll
        for (int dy = -R; dy <= R; ++dy)
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int gp = gq - dy * GW - dx, lp = lq - dy * LWD - dx;   // p = q - d
                const float w = lwa_s(sg[gp], sg[GP + gp], sg[2 * GP + gp], q0, q1, q2, a.c) * siz[lp];
                dv0 = fmaf(w, sG[lp], dv0);
                dv1 = fmaf(w, sG[LP + lp], dv1);
            }
    } else {
        const float vq0 = sv[lq], vq1 = sv[LP + lq], yq0 = sy[lq], yq1 = sy[LP + lq];
        const float Gq0 = sG[lq], Gq1 = sG[LP + lq], izq = siz[lq];
        float dg0 = 0.f, dg1 = 0.f, dg2 = 0.f;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy)
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                // p = q - d: pixel p's weight for its neighbour q
                const int gp = gq - dy * GW - dx, lp = lq - dy * LWD - dx;
                const float p0 = sg[gp], p1 = sg[GP + gp], p2 = sg[2 * GP + gp];
                const float Gp0 = sG[lp], Gp1 = sG[LP + lp];
                const float w = lwa_s(p0, p1, p2, q0, q1, q2, a.c) * siz[lp];
                dv0 = fmaf(w, Gp0, dv0);
                dv1 = fmaf(w, Gp1, dv1);
                const float t = fmaf(Gp1, vq1 - sy[LP + lp], Gp0 * (vq0 - sy[lp]));
                const float e = -a.inv_alpha * w * t;
                // n = q + d: pixel q's own weight for its neighbour n
                const int gn = gq + dy * GW + dx, ln = lq + dy * LWD + dx;
                const float n0 = sg[gn], n1 = sg[GP + gn], n2 = sg[2 * GP + gn];
                const float wn = lwa_s(q0, q1, q2, n0, n1, n2, a.c) * izq;
                const float tn = fmaf(Gq1, sv[LP + ln] - yq1, Gq0 * (sv[ln] - yq0));
                const float en = -a.inv_alpha * wn * tn;
                dg0 += 2.f * (q0 - p0) * e - 2.f * (n0 - q0) * en;
                dg1 += 2.f * (q1 - p1) * e - 2.f * (n1 - q1) * en;
                dg2 += 2.f * (q2 - p2) * e - 2.f * (n2 - q2) * en;
            }
        float* gp_out = a.dg + (long)b * 3 * HW + (long)y * W + x;
        gp_out[0] = dg0;
        gp_out[HW] = dg1;
        gp_out[2 * HW] = dg2;
    }
    float* dvp = a.dv + (long)b * 2 * HW + (long)y * W + x;
    dvp[0] = dv0;
    dvp[HW] = dv1;
}

// ------------------------------------------------------------------------------------------------
static int lwa_check(const char* fn, const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* pred, int32_t Cp,
                     int32_t ab_ch, int32_t B, int32_t H, int32_t W, float scale_xh, float scale_xw, float l_offset,
                     int32_t patch_size, float alpha) {
    DVC_REQUIRE(x_lab && pred, "%s: null argument", fn);
    DVC_REQUIRE(B > 0 && Hx > 0 && Wx > 0 && H > 0 && W > 0, "%s: bad shape", fn);
    DVC_REQUIRE(Cx >= 3, "%s: x_lab needs at least 3 channels (L, a, b; got %d)", fn, Cx);
    DVC_REQUIRE(ab_ch >= 0 && Cp >= 2 && ab_ch <= Cp - 2, "%s: pred has no channels %d, %d (it has %d)", fn, ab_ch, ab_ch + 1, Cp);
    DVC_REQUIRE(patch_size >= 1 && patch_size <= LW_MAX_K && patch_size % 2 == 1,
                "%s: patch_size must be odd and within 1..%d (got %d)", fn, LW_MAX_K, patch_size);
    DVC_REQUIRE(alpha > 0.f && std::isfinite(alpha), "%s: alpha must be > 0 and finite (got %g)", fn, (double)alpha);
    DVC_REQUIRE(scale_xh > 0.f && scale_xw > 0.f && std::isfinite(scale_xh) && std::isfinite(scale_xw),
                "%s: resize scales must be > 0 and finite", fn);
    DVC_REQUIRE(std::isfinite(l_offset), "%s: l_offset must be finite", fn);
    DVC_REQUIRE(B <= 65535 && cdiv(H, LW_TH) <= 65535 && (long)H * W < (1L << 30) && (long)Hx * Wx < (1L << 30),
                "%s: map or batch too large", fn);
    return 0;
}

template <template <int> class Launch>
static void lwa_dispatch(int r, const LwaArgs& a, dim3 grid, hipStream_t s) {
    switch (r) {
        case 0: Launch<0>::go(a, grid, s); break;
        case 1: Launch<1>::go(a, grid, s); break;
        case 2: Launch<2>::go(a, grid, s); break;
        default: Launch<3>::go(a, grid, s); break;
    }
}
template <int R>
struct LwaFwd {
    static void go(const LwaArgs& a, dim3 grid, hipStream_t s) { hipLaunchKernelGGL(lwa_fwd_kernel<R>, grid, dim3(256), 0, s, a); }
};
template <int R>
struct LwaBwd {
    static void go(const LwaArgs& a, dim3 grid, hipStream_t s) { hipLaunchKernelGGL(lwa_bwd_kernel<R>, grid, dim3(256), 0, s, a); }
};

static LwaArgs lwa_args(const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* pred, int32_t Cp, int32_t ab_ch,
                        int32_t H, int32_t W, float scale_xh, float scale_xw, float l_offset, float alpha) {
    LwaArgs a = {};
    a.x_lab = x_lab;
    a.pred = pred;
    a.Cx = Cx;
    a.Hx = Hx;
    a.Wx = Wx;
    a.Cp = Cp;
    a.ab_ch = ab_ch;
    a.H = H;
    a.W = W;
    a.sxh = scale_xh;
    a.sxw = scale_xw;
    a.l_offset = l_offset;
    a.c = (float)std::min(1.4426950408889634 / (double)alpha, (double)FLT_MAX);
    a.inv_alpha = (float)std::min(1.0 / (double)alpha, (double)FLT_MAX);
    return a;
}

extern "C" int dvc_lwa_fwd(const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* pred, int32_t Cp, int32_t ab_ch,
                           int32_t B, int32_t H, int32_t W, float scale_xh, float scale_xw, float l_offset, int32_t patch_size,
                           float alpha, float* y, dvcStream stream) {
    if (lwa_check("dvc_lwa_fwd", x_lab, Cx, Hx, Wx, pred, Cp, ab_ch, B, H, W, scale_xh, scale_xw, l_offset, patch_size, alpha))
        return 1;
    DVC_REQUIRE(y, "dvc_lwa_fwd: null argument");
    LwaArgs a = lwa_args(x_lab, Cx, Hx, Wx, pred, Cp, ab_ch, H, W, scale_xh, scale_xw, l_offset, alpha);
    a.y = y;
    lwa_dispatch<LwaFwd>(patch_size / 2, a, dim3(cdiv(W, LW_TW), cdiv(H, LW_TH), B), (hipStream_t)stream);
    DVC_CHECK_LAUNCH("dvc_lwa_fwd");
    return 0;
}

extern "C" int dvc_lwa_bwd(const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* pred, int32_t Cp, int32_t ab_ch,
                           int32_t B, int32_t H, int32_t W, float scale_xh, float scale_xw, float l_offset, int32_t patch_size,
                           float alpha, const float* G, const float* y, float* d_pred_ab, float* d_guide, dvcStream stream) {
    if (lwa_check("dvc_lwa_bwd", x_lab, Cx, Hx, Wx, pred, Cp, ab_ch, B, H, W, scale_xh, scale_xw, l_offset, patch_size, alpha))
        return 1;
    DVC_REQUIRE(G && y && d_pred_ab, "dvc_lwa_bwd: null argument");
    DVC_REQUIRE(!d_guide || (Hx == H && Wx == W && scale_xh == 1.f && scale_xw == 1.f),
                "dvc_lwa_bwd: d_guide needs an unresized x_lab (scales 1, %d x %d; got %g, %g, %d x %d): resize it first", H, W,
                (double)scale_xh, (double)scale_xw, Hx, Wx);
    LwaArgs a = lwa_args(x_lab, Cx, Hx, Wx, pred, Cp, ab_ch, H, W, scale_xh, scale_xw, l_offset, alpha);
    a.G = G;
    a.y_in = y;
    a.dv = d_pred_ab;
    a.dg = d_guide;
    lwa_dispatch<LwaBwd>(patch_size / 2, a, dim3(cdiv(W, LW_TW), cdiv(H, LW_TH), B), (hipStream_t)stream);
    DVC_CHECK_LAUNCH("dvc_lwa_bwd");
    return 0;
}
