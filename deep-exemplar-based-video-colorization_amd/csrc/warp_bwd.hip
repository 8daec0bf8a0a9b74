// WarpNet's backward behind the trunk tensor (training mode, dvc_amd/nets.py): the residual blocks, the theta / phi projections,
// the centre-and-normalise step and the x4 nearest upsample.  The 3x3 input gradients run on the forward's engines (zero pad 1 on
// a zero-ringed map, W^T flipped), the 3x3 weight gradients on dvc_cvn_wgrad (zero-ringed dZ against a reflect-padded copy of
// the input), the correlation on dvc_amd/corr_autograd.py, the centre-and-normalise step's backward on dvc_warp_cn_bwd
// (feature_norm.hip); what is here is the steps between them:
//   dvc_warp_up4_bwd         4x4 block sums (backward of the x4 nearest upsample)
//   dvc_warp_prelu_fwd       y = prelu(n [+ skip]) — the forward's activation as a launch of its own, so that the norm's output
//                            exists as a tensor
//   dvc_warp_k1_wgrad        dW = sum_n dT[n] F[n]^T, db = sum dT of a 1x1 convolution on v_mfma_f32_32x32x2_f32
//   dvc_warp_norm_prelu_bwd  PReLU + InstanceNorm backward per plane into a zero-ringed map (+ the skip's gradient, the slope's
//                            partial sum)
//   dvc_warp_slope_sum       the slope's partial sums added in a fixed order, in double
//   dvc_warp_reflect_pad     reflect-padded copy (one pixel)
//   dvc_warp_fold            adjoint of that padding: the ring added back onto rows / columns 1 and H-2 / W-2 (+ a skip gradient)
// Every sum has a fixed order: the results are bit-deterministic and do not depend on timing.
#include <cstdint>

#include "bwd_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ x4 upsample backward
__global__ __launch_bounds__(256) void up4_bwd_kernel(const float* __restrict__ g, long total, int h, int w, int vec,
                                                      float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long plane = i / ((long)h * w);
    const int r = (int)(i - plane * h * w), y = r / w, x = r - y * w;
    const float* gp = g + plane * 16L * h * w + (long)(4 * y) * (4 * w) + 4 * x;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float4 v;
        if (vec)
            v = *reinterpret_cast<const float4*>(gp + (long)k * 4 * w);
        else
            v = make_float4(gp[(long)k * 4 * w], gp[(long)k * 4 * w + 1], gp[(long)k * 4 * w + 2], gp[(long)k * 4 * w + 3]);
        s += (v.x + v.y) + (v.z + v.w);
    }
    out[i] = s;
}

// ------------------------------------------------------------------------------------------------ PReLU forward
__global__ __launch_bounds__(256) void prelu_fwd_kernel(const float* __restrict__ n, const float* __restrict__ res,
                                                        const float* __restrict__ slope_ptr, long total, float* __restrict__ y) {
    const float slope = *slope_ptr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        float v = n[i];
        if (res) v += res[i];
        y[i] = v >= 0.f ? v : v * slope;       // (the expression of instnorm_apply_plane, csrc/norm_pool.hip)
    }
}

// ------------------------------------------------------------------------------------------------ 1x1 weight gradient
// A GEMM [Cout x K] . [K x Cin], K = N * P, both operands contiguous along K.  A workgroup owns a 64 (co) x 64 (ci) tile and a
// contiguous range of 32-position chunks (never across two images); per chunk it stages dT [64][32] and F [64][32] in LDS and
// each wave runs 16 MFMAs on its 32 x 32 quarter.  The K order inside a chunk is permuted (lane half h takes positions
// 16h..16h+15) so that both operands are float4 reads, as dvc_cvn_wgrad does.
constexpr int kK1T = kWgTile;       // co / ci tile
constexpr int kK1P = 32;            // positions per chunk
constexpr int kK1S = kK1P + 4;      // LDS row stride

struct K1Args {
    const float* dT;    // [N][Cout][P]
    const float* F;     // [N][Cin][P]
    float* part;        // [S][Cout*Cin + Cout]
    int N, Cin, Cout, P, ncp, nchunks, S, vec;
    long ld;
};

__device__ __forceinline__ float4 k1_load4(const float* row, bool row_ok, int p, int P, int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok || p >= P) return v;
    if (vec && p + 3 < P) return *reinterpret_cast<const float4*>(row + p);
    v.x = row[p];
    if (p + 1 < P) v.y = row[p + 1];
    if (p + 2 < P) v.z = row[p + 2];
    if (p + 3 < P) v.w = row[p + 3];
    return v;
}

__global__ __launch_bounds__(256) void k1_wgrad_kernel(K1Args a) {
    __shared__ __attribute__((aligned(16))) float sA[kK1T * kK1S];
    __shared__ __attribute__((aligned(16))) float sB[kK1T * kK1S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int ci0 = blockIdx.x * kK1T, co0 = blockIdx.y * kK1T, sp = blockIdx.z;
    const int wco = (wave & 1) * 32, wci = (wave >> 1) * 32;
    int c_beg, c_end;
    wgrad_chunk_range(sp, a.nchunks, a.S, c_beg, c_end);
    const bool do_bias = blockIdx.x == 0;

    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    double bacc = 0.0;

    for (int c = c_beg; c < c_end; ++c) {
        const int b = c / a.ncp, p0 = (c - b * a.ncp) * kK1P;
        const float* zb = a.dT + ((long)b * a.Cout + co0) * a.P;
        const float* xb = a.F + ((long)b * a.Cin + ci0) * a.P;
#pragma unroll
        for (int k = 0; k < kK1T * kK1P / (4 * 256); ++k) {
            const int e = tid + 256 * k, row = e >> 3, q = (e & 7) * 4;
            *reinterpret_cast<float4*>(sA + row * kK1S + q) = k1_load4(zb + (long)row * a.P, co0 + row < a.Cout, p0 + q, a.P, a.vec);
            *reinterpret_cast<float4*>(sB + row * kK1S + q) = k1_load4(xb + (long)row * a.P, ci0 + row < a.Cin, p0 + q, a.P, a.vec);
        }
        __syncthreads();
        if (do_bias && tid < kK1T) {
#pragma unroll
            for (int s = 0; s < kK1P; ++s) bacc += (double)sA[tid * kK1S + s];
        }
        const float4* za = reinterpret_cast<const float4*>(sA + (wco + l31) * kK1S + hi * 16);
        const float4* xa = reinterpret_cast<const float4*>(sB + (wci + l31) * kK1S + hi * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 z = za[j], x = xa[j];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.x, x.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.y, x.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.z, x.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.w, x.w, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    float* slot = a.part + (long)sp * a.ld;
    wgrad_store_tile<1>(slot, &acc, ci0 + wci + l31, co0 + wco, hi, a.Cin, a.Cout);
    wgrad_store_bias<1>(slot, do_bias, tid, co0, a.Cin, a.Cout, bacc);
}

// ------------------------------------------------------------------------------------------------ PReLU + InstanceNorm backward
// One workgroup per (image, channel) plane.  u = n (+ skip), du = g * (u > 0 ? 1 : a) and the slope's partial
// sum (u > 0 ? 0 : u g) — ATen's prelu backward, u == 0 on the slope's side —, then
// dz = rstd (du - mean(du) - n mean(du n)) into the interior of a zero-ringed (H+2) x (W+2) plane.  The three plane sums run in
// double (butterfly per wave, waves in order).
constexpr int kNpT = 512;

__global__ __launch_bounds__(kNpT) void norm_prelu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ n,
                                                              const float* __restrict__ res, const float* __restrict__ rstd,
                                                              const float* __restrict__ slope_ptr, int H, int W,
                                                              float* __restrict__ dzr, float* __restrict__ du_out,
                                                              double* __restrict__ slope_part) {
    __shared__ double red[kNpT / 64];
    const long plane = blockIdx.x;
    const int HW = H * W, PW = W + 2, PHW = (H + 2) * PW;
    const float a = *slope_ptr;
    const float* gp = g + plane * HW;
    const float* np = n + plane * HW;
    const float* rp = res ? res + plane * HW : nullptr;
    float* dup = du_out ? du_out + plane * HW : nullptr;
    float* zp = dzr + plane * PHW;
    double sd = 0.0, sdn = 0.0, ss = 0.0;
    for (int p = threadIdx.x; p < HW; p += kNpT) {
        const float nv = np[p], gv = gp[p];
        const float u = rp ? nv + rp[p] : nv;
        const bool pos = u > 0.f;
        const float du = pos ? gv : a * gv;
        if (!pos) ss += (double)u * (double)gv;
        sd += (double)du;
        sdn += (double)du * (double)nv;
    }
    const float md = (float)(block_sum<double, kNpT>(sd, red) / (double)HW);
    const float mdn = (float)(block_sum<double, kNpT>(sdn, red) / (double)HW);
    const double sl = block_sum<double, kNpT>(ss, red);
    if (threadIdx.x == 0) slope_part[plane] = sl;
    const float r = rstd[plane];
    for (int i = threadIdx.x; i < PHW; i += kNpT) {
        const int py = i / PW, px = i - py * PW;
        float v = 0.f;
        if (py >= 1 && py <= H && px >= 1 && px <= W) {
            const int p = (py - 1) * W + (px - 1);
            const float nv = np[p], gv = gp[p];
            const float u = rp ? nv + rp[p] : nv;
            const float du = u > 0.f ? gv : a * gv;
            v = r * (du - md - nv * mdn);
            if (dup) dup[p] = du;
        }
        zp[i] = v;
    }
}

// one workgroup: out = sum of n doubles, thread-strided partial sums then the fixed block order, rounded once
__global__ __launch_bounds__(256) void slope_sum_kernel(const double* __restrict__ part, long n, float* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) s += part[i];
    const double t = block_sum<double, 256>(s, red);
    if (threadIdx.x == 0) out[0] = (float)t;
}

// ------------------------------------------------------------------------------------------------ reflect pad and its adjoint
__global__ __launch_bounds__(256) void reflect_pad_kernel(const float* __restrict__ x, long total, int H, int W,
                                                          float* __restrict__ xp) {
    const int PW = W + 2, PHW = (H + 2) * PW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long plane = i / PHW;
        const int r = (int)(i - plane * PHW), py = r / PW, px = r - py * PW;
        const int y = py == 0 ? 1 : (py == H + 1 ? H - 2 : py - 1);
        const int xx = px == 0 ? 1 : (px == W + 1 ? W - 2 : px - 1);
        xp[i] = x[plane * H * W + (long)y * W + xx];
    }
}

// dx[y][x] = sum of gp over the padded positions that read x[y][x]: (y+1, x+1), plus padded row 0 for y == 1, row H+1 for
// y == H-2 (both when H == 3; for H == 2 row 0 lands on y = 1 and row 3 on y = 0), likewise the columns; rows outer, columns
// inner, the interior position first.  + skip when given.
__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ gp, const float* __restrict__ skip, long total, int H,
                                                   int W, float* __restrict__ dx) {
    const int PW = W + 2, PHW = (H + 2) * PW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long plane = i / ((long)H * W);
        const int r = (int)(i - plane * H * W), y = r / W, x = r - y * W;
        int rows[3], cols[3], nr = 0, nc = 0;
        rows[nr++] = y + 1;
        if (y == 1) rows[nr++] = 0;
        if (y == H - 2) rows[nr++] = H + 1;
        cols[nc++] = x + 1;
        if (x == 1) cols[nc++] = 0;
        if (x == W - 2) cols[nc++] = W + 1;
        const float* g = gp + plane * PHW;
        float s = 0.f;
        for (int j = 0; j < nr; ++j)
            for (int k = 0; k < nc; ++k) s += g[rows[j] * PW + cols[k]];
        if (skip) s += skip[i];
        dx[i] = s;
    }
}

static unsigned grid_for(long total) {
    const long blocks = cdivl(total, 256);
    return (unsigned)(blocks < 16384 ? blocks : 16384);
}

}  // namespace

// ================================================================================================ C entry points
extern "C" int dvc_warp_up4_bwd(const float* g, int32_t planes, int32_t h, int32_t w, float* out, dvcStream stream) {
    DVC_REQUIRE(g && out, "dvc_warp_up4_bwd: null pointer");
    DVC_REQUIRE(planes > 0 && h > 0 && w > 0, "dvc_warp_up4_bwd: bad size (planes %d h %d w %d)", planes, h, w);
    DVC_REQUIRE(g != out, "dvc_warp_up4_bwd: out must not alias g");
    const long total = (long)planes * h * w;
    DVC_REQUIRE(cdivl(total, 256) < (1L << 31), "dvc_warp_up4_bwd: tensor too large");
    const int vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;     // (rows of 4w floats: every 4-wide piece is then aligned)
    hipLaunchKernelGGL(up4_bwd_kernel, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, (hipStream_t)stream, g, total, (int)h,
                       (int)w, vec, out);
    DVC_CHECK_LAUNCH("dvc_warp_up4_bwd");
    return 0;
}

extern "C" int dvc_warp_prelu_fwd(const float* n, const float* skip, const float* slope, int64_t count, float* y,
                                  dvcStream stream) {
    DVC_REQUIRE(n && slope && y, "dvc_warp_prelu_fwd: null pointer");
    DVC_REQUIRE(count > 0, "dvc_warp_prelu_fwd: bad size (%ld)", (long)count);
    hipLaunchKernelGGL(prelu_fwd_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, n, skip, slope, (long)count, y);
    DVC_CHECK_LAUNCH("dvc_warp_prelu_fwd");
    return 0;
}

extern "C" int dvc_warp_k1_wgrad_splits(int32_t N, int32_t Cin, int32_t Cout, int32_t P) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || P <= 0) return 0;
    const long tiles = (long)cdiv(Cin, kK1T) * cdiv(Cout, kK1T);
    const long chunks = (long)N * cdiv(P, kK1P);
    return wgrad_default_splits(tiles, chunks);
}

extern "C" int dvc_warp_k1_wgrad(const float* dT, const float* F, int32_t N, int32_t Cin, int32_t Cout, int32_t P, int32_t S,
                                 float* part, size_t part_floats, float* out, dvcStream stream) {
    DVC_REQUIRE(dT && F && part && out, "dvc_warp_k1_wgrad: null pointer");
    DVC_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && P > 0, "dvc_warp_k1_wgrad: bad size (N %d Cin %d Cout %d P %d)", N, Cin, Cout, P);
    const int ncp = cdiv(P, kK1P);
    const long nchunks = (long)N * ncp;
    const long ld = (long)Cout * Cin + Cout;
    if (wgrad_check_frame("dvc_warp_k1_wgrad", S, Cin, Cout, nchunks, ld, dT, F, part, part_floats, out)) return 1;
    const int vec = P % 4 == 0 && ((reinterpret_cast<uintptr_t>(dT) | reinterpret_cast<uintptr_t>(F)) & 15) == 0;
    K1Args a{dT, F, part, N, Cin, Cout, P, ncp, (int)nchunks, S, vec, ld};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k1_wgrad_kernel, dim3(cdiv(Cin, kK1T), cdiv(Cout, kK1T), S), dim3(256), 0, st, a);
    DVC_CHECK_LAUNCH("dvc_warp_k1_wgrad");
    launch_sum_slots(part, S, ld, ld, out, st);
    DVC_CHECK_LAUNCH("dvc_warp_k1_wgrad (slot sum)");
    return 0;
}

extern "C" int dvc_warp_norm_prelu_bwd(const float* g, const float* n, const float* skip, const float* rstd, const float* slope,
                                       int32_t planes, int32_t H, int32_t W, float* dz_ringed, float* du, double* slope_part,
                                       dvcStream stream) {
    DVC_REQUIRE(g && n && rstd && slope && dz_ringed && slope_part, "dvc_warp_norm_prelu_bwd: null pointer");
    DVC_REQUIRE(planes > 0 && H > 0 && W > 0, "dvc_warp_norm_prelu_bwd: bad size (planes %d H %d W %d)", planes, H, W);
    DVC_REQUIRE(((long)H + 2) * ((long)W + 2) < (1L << 30), "dvc_warp_norm_prelu_bwd: plane too large");
    DVC_REQUIRE(dz_ringed != g && dz_ringed != n && dz_ringed != skip && (!du || (du != g && du != n && du != skip && du != dz_ringed)),
                "dvc_warp_norm_prelu_bwd: outputs must not alias inputs");
    hipLaunchKernelGGL(norm_prelu_bwd_kernel, dim3(planes), dim3(kNpT), 0, (hipStream_t)stream, g, n, skip, rstd, slope, (int)H,
                       (int)W, dz_ringed, du, slope_part);
    DVC_CHECK_LAUNCH("dvc_warp_norm_prelu_bwd");
    return 0;
}

extern "C" int dvc_warp_slope_sum(const double* part, int64_t count, float* out, dvcStream stream) {
    DVC_REQUIRE(part && out, "dvc_warp_slope_sum: null pointer");
    DVC_REQUIRE(count > 0, "dvc_warp_slope_sum: bad size (%ld)", (long)count);
    hipLaunchKernelGGL(slope_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (long)count, out);
    DVC_CHECK_LAUNCH("dvc_warp_slope_sum");
    return 0;
}

extern "C" int dvc_warp_reflect_pad(const float* x, int32_t planes, int32_t H, int32_t W, float* x_padded, dvcStream stream) {
    DVC_REQUIRE(x && x_padded, "dvc_warp_reflect_pad: null pointer");
    DVC_REQUIRE(planes > 0 && H >= 2 && W >= 2, "dvc_warp_reflect_pad: bad size (planes %d H %d W %d; H, W >= 2)", planes, H, W);
    DVC_REQUIRE(((long)H + 2) * ((long)W + 2) < (1L << 30), "dvc_warp_reflect_pad: plane too large");
    DVC_REQUIRE(x != x_padded, "dvc_warp_reflect_pad: x_padded must not alias x");
    const long total = (long)planes * (H + 2) * (W + 2);
    hipLaunchKernelGGL(reflect_pad_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, total, (int)H, (int)W,
                       x_padded);
    DVC_CHECK_LAUNCH("dvc_warp_reflect_pad");
    return 0;
}

extern "C" int dvc_warp_fold(const float* g_padded, const float* skip, int32_t planes, int32_t H, int32_t W, float* dx,
                             dvcStream stream) {
    DVC_REQUIRE(g_padded && dx, "dvc_warp_fold: null pointer");
    DVC_REQUIRE(planes > 0 && H >= 2 && W >= 2, "dvc_warp_fold: bad size (planes %d H %d W %d; H, W >= 2)", planes, H, W);
    DVC_REQUIRE(((long)H + 2) * ((long)W + 2) < (1L << 30), "dvc_warp_fold: plane too large");
    DVC_REQUIRE(dx != g_padded, "dvc_warp_fold: dx must not alias g_padded");
    const long total = (long)planes * H * W;
    hipLaunchKernelGGL(fold_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g_padded, skip, total, (int)H, (int)W,
                       dx);
    DVC_CHECK_LAUNCH("dvc_warp_fold");
    return 0;
}
