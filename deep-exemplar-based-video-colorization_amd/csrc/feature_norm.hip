// Centre a [B][C][P] feature map by its per-channel mean over positions, divide every position by its L2 norm over channels — the
// step in front of every cosine-affinity consumer (correlation: NonlocalNet.py:469-476, contextual loss: ContextualLoss.py:48-61,
// feature_normalize: FrameColor.py:16-23) — forward and backward, once:
//   dvc_corr_prepare          row mean, then the float4 normalise (P % 4 == 0, aligned) or the scalar one with 4 channel groups
//   dvc_cx_prepare            row mean (own, given or none), then the scalar normalise with 16 channel groups (+ the norms)
//   dvc_channel_l2norm(_multi) the same two normalise forms without a mean, several tensors in one launch
//   dvc_cx_normalize_bwd      backward of the normalise from the saved xn and norm, sums in float
//   dvc_warp_cn_bwd           backward of centre + normalise, recomputed from t and the mean, sums in double
// (dvc_corr_prepare_bf16, corr_bf16.hip, launches the row mean here and keeps its transposing normalise.)
// All are deterministic: per thread an fmaf chain over its channels in ascending order, the channel groups added in ascending
// order, the row sums in reduce.h's CHAIN order.
#include "feature_norm.h"

#include <cstdint>

#include "reduce.h"

namespace {

// ------------------------------------------------------------------------------------------------ row sums over positions
// Sum of a row of P floats over a 256-thread workgroup, in double: thread-strided partial sums, CHAIN order; every thread
// returns it.
__device__ __forceinline__ double row_sum(const float* row, int P, double* red /* [4] */) {
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += 256) s += (double)row[i];
    return block_chain_sum<4>(wave_sum(s), red);
}

__global__ __launch_bounds__(256) void rowmean_kernel(const float* __restrict__ t, int P, float* __restrict__ mean) {
    __shared__ double red[4];
    const double s = row_sum(t + (long)blockIdx.x * P, P, red);
    if (threadIdx.x == 0) mean[blockIdx.x] = (float)(s / (double)P);
}

// backward of the centring, per (image, channel) row: d t = d tc - mean_P(d tc), in place; the mean in double, rounded once
__global__ __launch_bounds__(256) void cn_bwd_center_kernel(float* __restrict__ d, int P) {
    __shared__ double red[4];
    float* row = d + (long)blockIdx.x * P;
    const float m = (float)(row_sum(row, P, red) / (double)P);
    for (int i = threadIdx.x; i < P; i += 256) row[i] -= m;
}

// ------------------------------------------------------------------------------------------------ normalise, scalar form
// The NG channel groups' partial results for position px, added in ascending order.  (Started from part[0], not from 0: the
// two differ only for part[0] == -0.0, which an fmaf chain that starts at +0.0 never produces — DESIGN.md.)
template <int NG>
__device__ __forceinline__ float groups_sum(const float (*part)[64], int px) {
    float s = part[0][px];
#pragma unroll
    for (int k = 1; k < NG; ++k) s += part[k][px];
    return s;
}

// Workgroup = 64 positions x NG channel groups; group g walks channels g, g + NG, ..., four channel rows in flight per thread,
// accumulated in the same order as one at a time (r06: with one load at a time a thread walked C / NG dependent round trips
// twice — 72 us for 16 maps of 512 x 13 x 24 with NG = 4).  MEAN: subtract mean[b][c] first.  NORM: also write the norms
// [B][P] (for the backward).  out = v / (sqrt(sum_c v^2) + eps).
template <int NG, bool MEAN, bool NORM>
__global__ __launch_bounds__(64 * NG) void normalize_kernel(const float* __restrict__ t, const float* __restrict__ mean, int C,
                                                            int P, float eps, float* __restrict__ out, float* __restrict__ norm) {
    __shared__ float part[NG][64];
    const int px = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long p = (long)blockIdx.x * 64 + px;
    const int b = blockIdx.y;
    const float* tb = t + (long)b * C * P + p;
    const float* mb = MEAN ? mean + (long)b * C : nullptr;
    float* ob = out + (long)b * C * P + p;
    const bool ok = p < P;
    auto centred = [&](int c) {
        const float v = tb[(long)c * P];
        return MEAN ? v - mb[c] : v;
    };
    float s = 0.f;
    if (ok) {
        int c = g;
        for (; c + 3 * NG < C; c += 4 * NG) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = centred(c + u * NG);
#pragma unroll
            for (int u = 0; u < 4; ++u) s = fmaf(v[u], v[u], s);
        }
        for (; c < C; c += NG) {
            const float v = centred(c);
            s = fmaf(v, v, s);
        }
    }
    part[g][px] = s;
    __syncthreads();
    const float n = sqrtf(groups_sum<NG>(part, px)), den = n + eps;
    if (ok) {
        if (NORM && g == 0) norm[(long)b * P + p] = n;
        int c = g;
        for (; c + 3 * NG < C; c += 4 * NG) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = centred(c + u * NG);
#pragma unroll
            for (int u = 0; u < 4; ++u) ob[(long)(c + u * NG) * P] = v[u] / den;
        }
        for (; c < C; c += NG) ob[(long)c * P] = centred(c) / den;
    }
}

template <int NG, bool MEAN, bool NORM>
void normalize_launch(const float* t, const float* mean, int B, int C, int P, float eps, float* out, float* norm, hipStream_t s) {
    hipLaunchKernelGGL((normalize_kernel<NG, MEAN, NORM>), dim3(cdiv(P, 64), B), dim3(64 * NG), 0, s, t, mean, C, P, eps, out, norm);
}

// ------------------------------------------------------------------------------------------------ normalise, float4 form
// P % 4 == 0 and 16-byte aligned maps.  Workgroup `wg` of a map = 32 positions (8 lanes x float4: one 128-byte line per channel
// row) x 32 channel groups, four channel rows in flight per thread, accumulated in the same order as one at a time — 162
// workgroups at P = 5184, where the scalar form with 4 groups runs 81 workgroups of 64-deep serial loops.  xb / mb / yb: the image.
// (Written out, not folded into helper lambdas: channel_l2norm_multi_kernel sits in every frame and must stay at 64 VGPRs, eight
// waves per SIMD; the lambda forms tried came to 65.)
template <bool MEAN>
__device__ __forceinline__ void normalize_v4_body(const float* xb, const float* mb, int C, long P, long wg,
                                                  float eps, float* yb) {
    __shared__ float4 part[32][8];
    const int px4 = threadIdx.x & 7, g = threadIdx.x >> 3;
    const long p = (wg * 8 + px4) * 4;
    const bool ok = p < P;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
        int c = g;
        for (; c + 96 < C; c += 128) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(xb + (long)(c + 32 * u) * P + p);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (MEAN) { const float mu = mb[c + 32 * u]; v[u].x -= mu; v[u].y -= mu; v[u].z -= mu; v[u].w -= mu; }
                s.x = fmaf(v[u].x, v[u].x, s.x);
                s.y = fmaf(v[u].y, v[u].y, s.y);
                s.z = fmaf(v[u].z, v[u].z, s.z);
                s.w = fmaf(v[u].w, v[u].w, s.w);
            }
        }
        for (; c < C; c += 32) {
            float4 v = *reinterpret_cast<const float4*>(xb + (long)c * P + p);
            if (MEAN) { const float mu = mb[c]; v.x -= mu; v.y -= mu; v.z -= mu; v.w -= mu; }
            s.x = fmaf(v.x, v.x, s.x);
            s.y = fmaf(v.y, v.y, s.y);
            s.z = fmaf(v.z, v.z, s.z);
            s.w = fmaf(v.w, v.w, s.w);
        }
    }
    part[g][px4] = s;
    __syncthreads();
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const float4 v = part[k][px4];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    const float4 den = make_float4(sqrtf(t.x) + eps, sqrtf(t.y) + eps, sqrtf(t.z) + eps, sqrtf(t.w) + eps);
    if (ok) {
        int c = g;
        for (; c + 96 < C; c += 128) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(xb + (long)(c + 32 * u) * P + p);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (MEAN) { const float mu = mb[c + 32 * u]; v[u].x -= mu; v[u].y -= mu; v[u].z -= mu; v[u].w -= mu; }
                v[u].x /= den.x; v[u].y /= den.y; v[u].z /= den.z; v[u].w /= den.w;
                *reinterpret_cast<float4*>(yb + (long)(c + 32 * u) * P + p) = v[u];
            }
        }
        for (; c < C; c += 32) {
            float4 v = *reinterpret_cast<const float4*>(xb + (long)c * P + p);
            if (MEAN) { const float mu = mb[c]; v.x -= mu; v.y -= mu; v.z -= mu; v.w -= mu; }
            v.x /= den.x; v.y /= den.y; v.z /= den.z; v.w /= den.w;
            *reinterpret_cast<float4*>(yb + (long)c * P + p) = v;
        }
    }
}

__global__ __launch_bounds__(256) void corr_normalize_v4_kernel(const float* __restrict__ t, const float* __restrict__ mean, int C,
                                                                int P, float eps, float* __restrict__ out) {
    const long b = blockIdx.y;
    normalize_v4_body<true>(t + b * C * P, mean + b * C, C, P, blockIdx.x, eps, out + b * C * P);
}

// The four feature_normalize calls of a frame (FrameColor.py:16-23: relu2_1 .. relu5_1, 10.6 / 5.3 / 2.7 / 0.6 MB) as ONE
// launch: separately they are 324 / 81 / 21 / 5 workgroups on 256 CUs — latency-bound, 62 us for 38 MB of traffic.  The tensors'
// workgroup ranges are concatenated (wg_start), so the small maps ride along with the large one.
struct L2MultiArgs {
    const float* x[DVC_L2NORM_MAX_TENSORS];
    float* y[DVC_L2NORM_MAX_TENSORS];
    int C[DVC_L2NORM_MAX_TENSORS], HW[DVC_L2NORM_MAX_TENSORS], wg_start[DVC_L2NORM_MAX_TENSORS + 1];
    int count;
    float eps;
};
__global__ __launch_bounds__(256) void channel_l2norm_multi_kernel(L2MultiArgs a) {
    int ti = 0;
#pragma unroll
    for (int k = 1; k < DVC_L2NORM_MAX_TENSORS; ++k) ti += (k < a.count && (int)blockIdx.x >= a.wg_start[k]) ? 1 : 0;
    const int C = a.C[ti];
    const long HW = a.HW[ti];
    const int n = blockIdx.y;
    normalize_v4_body<false>(a.x[ti] + (long)n * C * HW, nullptr, C, HW, blockIdx.x - a.wg_start[ti], a.eps, a.y[ti] + (long)n * C * HW);
}

// ------------------------------------------------------------------------------------------------ backward
// Two kernels with different arithmetic, both 64 positions x channel groups per workgroup.

// dvc_cx_normalize_bwd: backward of xn = xc / (||xc|| + eps) from the SAVED xn and norm, the channel sum in float:
//     d xc_k = d xn_k / (n + eps) - xn_k (xn . d xn) / n
constexpr int kCxNG = 16;
__global__ __launch_bounds__(64 * kCxNG) void cx_normalize_bwd_kernel(const float* __restrict__ xn, const float* __restrict__ norm,
                                                                      const float* __restrict__ dxn, int C, int P, float eps,
                                                                      float* __restrict__ dx) {
    __shared__ float part[kCxNG][64];
    const int px = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + px;
    const int b = blockIdx.y;
    const long base = (long)b * C * P + p;
    const bool ok = p < P;
    float s = 0.f;
    if (ok) {
        int c = g;
        for (; c + 3 * kCxNG < C; c += 4 * kCxNG) {
            float a[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = xn[base + (long)(c + u * kCxNG) * P];
                d[u] = dxn[base + (long)(c + u * kCxNG) * P];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s = fmaf(a[u], d[u], s);
        }
        for (; c < C; c += kCxNG) s = fmaf(xn[base + (long)c * P], dxn[base + (long)c * P], s);
    }
    part[g][px] = s;
    __syncthreads();
    const float dot = groups_sum<kCxNG>(part, px);
    if (ok) {
        const float n = norm[(long)b * P + p];
        const float inv = 1.f / (n + eps), k = n > 0.f ? dot / n : 0.f;
        int c = g;
        for (; c + 3 * kCxNG < C; c += 4 * kCxNG) {
            float a[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = xn[base + (long)(c + u * kCxNG) * P];
                d[u] = dxn[base + (long)(c + u * kCxNG) * P];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) dx[base + (long)(c + u * kCxNG) * P] = d[u] * inv - a[u] * k;
        }
        for (; c < C; c += kCxNG) {
            const long o = base + (long)c * P;
            dx[o] = dxn[o] * inv - xn[o] * k;
        }
    }
}

// dvc_warp_cn_bwd, step 1 (step 2 is cn_bwd_center_kernel above): RECOMPUTES tc = t - mean, r = ||tc||, s = r + eps,
//     d tc = g / s - tc (tc . g) / (r s^2)   (the second term is zero where r == 0)
// with 4 channel groups; the two channel sums run in double, the groups in TREE order.
__global__ __launch_bounds__(256) void cn_bwd_pos_kernel(const float* __restrict__ t, const float* __restrict__ mean,
                                                         const float* __restrict__ g, int C, int P, float eps,
                                                         float* __restrict__ dtc) {
    __shared__ double pss[4][64], pdot[4][64];
    const int px = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + px, b = blockIdx.y;
    const float* tb = t + (long)b * C * P;
    const float* gb = g + (long)b * C * P;
    const float* mb = mean + (long)b * C;
    float* ob = dtc + (long)b * C * P;
    const bool ok = p < P;
    double ss = 0.0, dot = 0.0;
    if (ok)
        for (int c = grp; c < C; c += 4) {
            const float v = tb[(long)c * P + p] - mb[c];
            ss += (double)v * (double)v;
            dot += (double)v * (double)gb[(long)c * P + p];
        }
    pss[grp][px] = ss;
    pdot[grp][px] = dot;
    __syncthreads();
    const double SS = (pss[0][px] + pss[1][px]) + (pss[2][px] + pss[3][px]);
    const double DOT = (pdot[0][px] + pdot[1][px]) + (pdot[2][px] + pdot[3][px]);
    const double r = sqrt(SS), s = r + (double)eps;
    const float inv_s = (float)(1.0 / s);
    const float k = r > 0.0 ? (float)(DOT / (r * s * s)) : 0.f;
    if (ok)
        for (int c = grp; c < C; c += 4) {
            const float v = tb[(long)c * P + p] - mb[c];
            ob[(long)c * P + p] = gb[(long)c * P + p] * inv_s - v * k;
        }
}

}  // namespace

// ================================================================================================ C entry points
void feature_rowmean_launch(const float* t, int rows, int P, float* mean, hipStream_t stream) {
    hipLaunchKernelGGL(rowmean_kernel, dim3(rows), dim3(256), 0, stream, t, P, mean);
}

extern "C" int dvc_corr_prepare(const float* t_raw, int32_t B, int32_t C, int32_t P, float eps,
                                float* mean_scratch, float* t_out, dvcStream stream) {
    DVC_REQUIRE(t_raw && mean_scratch && t_out && B > 0 && C > 0 && P > 0, "dvc_corr_prepare: bad argument");
    hipStream_t s = (hipStream_t)stream;
    feature_rowmean_launch(t_raw, B * C, P, mean_scratch, s);
    DVC_CHECK_LAUNCH("dvc_corr_prepare(mean)");
    if (P % 4 == 0 && (((reinterpret_cast<uintptr_t>(t_raw) | reinterpret_cast<uintptr_t>(t_out)) & 15) == 0))
        hipLaunchKernelGGL(corr_normalize_v4_kernel, dim3(cdiv(P, 32), B), dim3(256), 0, s, t_raw, mean_scratch, C, P, eps, t_out);
    else
        normalize_launch<4, true, false>(t_raw, mean_scratch, B, C, P, eps, t_out, nullptr, s);
    DVC_CHECK_LAUNCH("dvc_corr_prepare(normalise)");
    return 0;
}

extern "C" int dvc_cx_prepare(const float* x, const float* mean_in, int32_t centre, int32_t B, int32_t C, int32_t P, float eps,
                              float* mean_out, float* norm_out, float* out, dvcStream stream) {
    DVC_REQUIRE(x && out && B > 0 && C > 0 && P > 0, "dvc_cx_prepare: bad argument");
    DVC_REQUIRE(!centre || mean_in || mean_out, "dvc_cx_prepare: centring needs a mean to use or a place to put its own");
    hipStream_t s = (hipStream_t)stream;
    const float* mean = nullptr;
    if (centre) {
        mean = mean_in;
        if (!mean) {
            feature_rowmean_launch(x, B * C, P, mean_out, s);
            DVC_CHECK_LAUNCH("dvc_cx_prepare(mean)");
            mean = mean_out;
        }
    }
    auto* launch = mean ? (norm_out ? normalize_launch<kCxNG, true, true> : normalize_launch<kCxNG, true, false>)
                        : (norm_out ? normalize_launch<kCxNG, false, true> : normalize_launch<kCxNG, false, false>);
    launch(x, mean, B, C, P, eps, out, norm_out, s);
    DVC_CHECK_LAUNCH("dvc_cx_prepare(normalise)");
    return 0;
}

extern "C" int dvc_cx_normalize_bwd(const float* xn, const float* norm, const float* dxn, int32_t B, int32_t C, int32_t P, float eps,
                                    float* dx, dvcStream stream) {
    DVC_REQUIRE(xn && norm && dxn && dx && B > 0 && C > 0 && P > 0, "dvc_cx_normalize_bwd: bad argument");
    hipLaunchKernelGGL(cx_normalize_bwd_kernel, dim3(cdiv(P, 64), B), dim3(64 * kCxNG), 0, (hipStream_t)stream, xn, norm, dxn, C, P, eps, dx);
    DVC_CHECK_LAUNCH("dvc_cx_normalize_bwd");
    return 0;
}

extern "C" int dvc_channel_l2norm_multi(const float* const* x, float* const* y, const int32_t* C, const int32_t* HW,
                                        int32_t count, int32_t N, float eps, dvcStream stream) {
    DVC_REQUIRE(x && y && C && HW && count > 0 && count <= DVC_L2NORM_MAX_TENSORS && N > 0, "dvc_channel_l2norm_multi: bad argument");
    L2MultiArgs a;
    a.count = count;
    a.eps = eps;
    int wgs = 0;
    for (int i = 0; i < DVC_L2NORM_MAX_TENSORS; ++i) {
        const int k = i < count ? i : count - 1;
        a.x[i] = x[k]; a.y[i] = y[k]; a.C[i] = C[k]; a.HW[i] = HW[k];
        a.wg_start[i] = wgs;
        if (i < count) {
            DVC_REQUIRE(x[i] && y[i] && C[i] > 0 && HW[i] > 0, "dvc_channel_l2norm_multi: bad tensor %d", i);
            DVC_REQUIRE(HW[i] % 4 == 0 && (((reinterpret_cast<uintptr_t>(x[i]) | reinterpret_cast<uintptr_t>(y[i])) & 15) == 0),
                        "dvc_channel_l2norm_multi: tensor %d needs H*W %% 4 == 0 and 16-byte aligned pointers (use dvc_channel_l2norm)", i);
            wgs += cdiv(HW[i], 32);
        }
    }
    a.wg_start[DVC_L2NORM_MAX_TENSORS] = wgs;
    hipLaunchKernelGGL(channel_l2norm_multi_kernel, dim3(wgs, N), dim3(256), 0, (hipStream_t)stream, a);
    DVC_CHECK_LAUNCH("dvc_channel_l2norm_multi");
    return 0;
}

extern "C" int dvc_channel_l2norm(const float* x, int32_t N, int32_t C, int32_t HW, float eps, float* y,
                                  dvcStream stream) {
    DVC_REQUIRE(x && y && N > 0 && C > 0 && HW > 0, "dvc_channel_l2norm: bad argument");
    const bool v4 = (HW % 4 == 0) && (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0);
    // (the float4 case IS the multi-tensor kernel with one tensor: a map normalised alone and the same map normalised in a
    // group of four give the same bits)
    if (v4) return dvc_channel_l2norm_multi(&x, &y, &C, &HW, 1, N, eps, stream);
    normalize_launch<4, false, false>(x, nullptr, N, C, HW, eps, y, nullptr, (hipStream_t)stream);
    DVC_CHECK_LAUNCH("dvc_channel_l2norm");
    return 0;
}

extern "C" int dvc_warp_cn_bwd(const float* t_raw, const float* mean, const float* g, int32_t B, int32_t C, int32_t P, float eps,
                               float* dt, dvcStream stream) {
    DVC_REQUIRE(t_raw && mean && g && dt, "dvc_warp_cn_bwd: null pointer");
    DVC_REQUIRE(B > 0 && C > 0 && P > 0, "dvc_warp_cn_bwd: bad size (B %d C %d P %d)", B, C, P);
    DVC_REQUIRE(B <= 65535 && (long)B * C < (1L << 31), "dvc_warp_cn_bwd: batch too large");
    DVC_REQUIRE(dt != t_raw && dt != g && dt != mean, "dvc_warp_cn_bwd: dt must not alias an input");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cn_bwd_pos_kernel, dim3(cdiv(P, 64), B), dim3(256), 0, st, t_raw, mean, g, (int)C, (int)P, eps, dt);
    DVC_CHECK_LAUNCH("dvc_warp_cn_bwd (positions)");
    hipLaunchKernelGGL(cn_bwd_center_kernel, dim3(B * C), dim3(256), 0, st, dt, (int)P);
    DVC_CHECK_LAUNCH("dvc_warp_cn_bwd (centre)");
    return 0;
}
