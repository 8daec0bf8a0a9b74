// Discriminator_x64's own parameter gradients (models/GAN_models.py:104-157 with models/spectral_normalization.py), for gfx950:
// what dvc_amd/gan.py launches behind `set_parameter_training()`.  include/dvc_hip.h states every entry point.
//
//   dvc_gan_conv4s2_wgrad   the plain weight gradient G of a 4x4 stride-2 pad-1 layer and its bias gradient, on
//                           v_mfma_f32_32x32x2_f32 in the tile step of gan.hip (gan_common.h).  The gathered operand is the
//                           matrix the forward stages, B[k][pixel] with k = 16 ci + 4 ky + kx; here the PIXELS are the reduction
//                           axis (numbered over the whole batch, chunks of 16) and a workgroup owns 64 output channels x 128
//                           columns k (8 input channels x 16 taps): wave w the columns [32 w, 32 w + 32), two 32 x 32 tiles.
//                           Both operands are staged k-major (pixel-major) in LDS; the next chunk is fetched into registers
//                           before the MFMA loop of the current one.  Pixel chunks are split over S slots in the frame of
//                           bwd_common.h (a slot is [Cout][Cin][16] then [Cout]) and the slots are summed in slot order in
//                           double: no atomics, bit-deterministic for a given S.  Inside a slot the fma chain is closed into a
//                           block total every kGanFlush chunks, as in the forward.
//   dvc_gan_sn_wgrad        the gradient through sigma = u'^T W_bar v':  dW_bar = (G - c u' v'^T) / sigma, c = <G, W_bar> / sigma
//   dvc_gan_last_wgrad      G and db of `last` (the mean over the positions of a [3, 6] valid convolution)
//   dvc_gan_dot             sum a[i] b[i], for d loss / d gamma
// The inner products: per-thread partial sums in double over a grid-strided range, CHAIN over the waves (reduce.h), one double
// per workgroup; the second launch adds those in a fixed order.  The grid depends on the element count alone.
#include "bwd_common.h"
#include "common.h"
#include "gan_common.h"
#include "reduce.h"

#include <cstdint>

constexpr int kGwCi = kGanN / 16;    // input channels per workgroup tile

struct GanWgradArgs {
    const float* dz;         // [N][Cout][OH][OW], batch stride ybs
    const float* x;          // [N][Cin][H][W], batch stride xbs
    float* part;             // [S][Cout*Cin*16 + Cout]
    int N, Cin, H, W, Cout, OH, OW, nchunks, S;
    long xbs, ybs, P, ld;
};

// grid (Cin tiles, Cout tiles, S)
__global__ __launch_bounds__(256) void gan_conv4s2_wgrad_kernel(GanWgradArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[kGanK * kGanLdA];
    __shared__ __attribute__((aligned(16))) float sB[kGanK * kGanLdB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int ci0 = blockIdx.x * kGwCi, co0 = blockIdx.y * kGanM, sp = blockIdx.z;
    const long HW = (long)a.H * a.W, OHW = (long)a.OH * a.OW;
    int c_beg, c_end;
    wgrad_chunk_range(sp, a.nchunks, a.S, c_beg, c_end);
    const bool do_bias = blockIdx.x == 0;

    // staging: thread -> pixel pk of the chunk.  A: dz of the output channels co0 + ar + 16 j.  B: input channel ci0 + bci, filter
    // rows 2 bh and 2 bh + 1, all four kx — the columns 8 (tid >> 4) .. + 7 of the tile
    const int pk = tid & 15, ar = tid >> 4, bci = tid >> 5, bh = (tid >> 4) & 1;
    const bool b_ok = ci0 + bci < a.Cin;
    float ra[4], rb[8];
    auto load = [&](int c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ra[j] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) rb[j] = 0.f;
        const long p = (long)c * kGanK + pk;
        if (p >= a.P) return;
        const int n = (int)(p / OHW), rem = (int)(p - (long)n * OHW), oy = rem / a.OW, ox = rem - oy * a.OW;
        const float* zp = a.dz + (long)n * a.ybs + rem;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + ar + 16 * j;
            if (co < a.Cout) ra[j] = zp[(long)co * OHW];
        }
        if (!b_ok) return;
        // the eight bounds predicates of the pixel, once
        const int iy0 = 2 * oy - 1 + 2 * bh, ix0 = 2 * ox - 1;
        const float* xp = a.x + (long)n * a.xbs + (long)(ci0 + bci) * HW + (long)iy0 * a.W + ix0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kx = 0; kx < 4; ++kx)
                if (iy0 + j >= 0 && iy0 + j < a.H && ix0 + kx >= 0 && ix0 + kx < a.W) rb[j * 4 + kx] = xp[j * a.W + kx];
    };

    gan_f16v acc[2], tot[2];
    gan_zero(acc);
    gan_zero(tot);
    double bacc = 0.0;
    if (c_beg < c_end) load(c_beg);
    for (int c = c_beg; c < c_end; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sA[pk * kGanLdA + ar + 16 * j] = ra[j];
        {
            float4* d = reinterpret_cast<float4*>(sB + pk * kGanLdB + (tid >> 4) * 8);
            d[0] = make_float4(rb[0], rb[1], rb[2], rb[3]);
            d[1] = make_float4(rb[4], rb[5], rb[6], rb[7]);
        }
        __syncthreads();
        if (c + 1 < c_end) load(c + 1);
        if (do_bias && tid < kGanM) {
#pragma unroll
            for (int s = 0; s < kGanK; ++s) bacc += (double)sA[s * kGanLdA + tid];
        }
        gan_mma_step(sA, sB, wave, l31, hi, acc);
        if ((c - c_beg) % kGanFlush == kGanFlush - 1) gan_flush(acc, tot);
        __syncthreads();
    }
    gan_flush(acc, tot);

    // C/D layout: column (k) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* slot = a.part + (long)sp * a.ld;
    const int col = wave * 32 + l31, ci = ci0 + (col >> 4), tap = col & 15;
    if (ci < a.Cin) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (co < a.Cout) slot[((long)co * a.Cin + ci) * 16 + tap] = tot[i][r];
            }
    }
    if (do_bias && tid < kGanM && co0 + tid < a.Cout) slot[(long)a.Cout * a.Cin * 16 + co0 + tid] = (float)bacc;
}

// ---- inner products.  part[b] = sum over the elements e = 256 b + t, + 256 gridDim.x, ... of a[e] b[e]
constexpr int kGanDotMaxBlocks = 1024;

static int gan_dot_blocks(long count) {
    const long b = cdivl(count, 256 * 8);
    return (int)(b < kGanDotMaxBlocks ? b : kGanDotMaxBlocks);
}

__global__ __launch_bounds__(256) void gan_dot_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, long count,
                                                              double* __restrict__ part) {
    __shared__ double red[4];
    double s = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) s += (double)x[e] * (double)y[e];
    s = block_sum<double, 256>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the close: thread t adds part[t], part[t + 256], ...; then CHAIN.  The same value in every thread of every workgroup.
__device__ __forceinline__ double gan_dot_close(const double* __restrict__ part, int nb, double* red) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[b];
    return block_sum<double, 256>(s, red);
}

__global__ __launch_bounds__(256) void gan_dot_close_kernel(const double* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ double red[4];
    const double s = gan_dot_close(part, nb, red);
    if (threadIdx.x == 0) out[0] = (float)s;
}

// dW_bar[co][k] = (G[co][k] - c u[co] v[k]) * inv_sigma, c = <G, W_bar> * inv_sigma; the element in double, rounded once (with
// G near c u v^T the difference is small against both terms)
__global__ __launch_bounds__(256) void gan_sn_wgrad_kernel(const float* __restrict__ G, const float* __restrict__ u,
                                                           const float* __restrict__ v, const float* __restrict__ inv_sigma,
                                                           const double* __restrict__ part, int nb, int K, long count,
                                                           float* __restrict__ out) {
    __shared__ double red[4];
    const double inv = (double)inv_sigma[0];
    const double c = gan_dot_close(part, nb, red) * inv;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
        const int co = (int)(e / K), k = (int)(e - (long)co * K);
        out[e] = (float)(((double)G[e] - c * (double)u[co] * (double)v[k]) * inv);
    }
}

// ---- `last`: one workgroup per channel; wave w the taps w, w + 4, ...; the lanes stride over (image, position), partial sums
// in double, the butterfly closes them.  The workgroup of channel 0 also adds up g.
__global__ __launch_bounds__(256) void gan_last_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, int N, int Cin,
                                                             int H, int W, long xbs, float* __restrict__ out) {
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int OH = H - 2, OW = W - 5, cnt = OH * OW;
    const float* xc = x + (long)c * H * W;
    for (int t = wave; t < 18; t += 4) {
        const int ky = t / 6, kx = t - ky * 6;
        double s = 0.0;
        for (long e = lane; e < (long)N * cnt; e += 64) {
            const int n = (int)(e / cnt), r = (int)(e - (long)n * cnt), oy = r / OW, ox = r - oy * OW;
            s += (double)g[n] * (double)xc[(long)n * xbs + (oy + ky) * W + ox + kx];
        }
        s = wave_sum(s);
        if (lane == 0) out[c * 18 + t] = (float)(s / (double)cnt);
    }
    if (c == 0 && wave == 0) {
        double s = 0.0;
        for (int n = lane; n < N; n += 64) s += (double)g[n];
        s = wave_sum(s);
        if (lane == 0) out[(long)Cin * 18] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------
static long gan_wgrad_chunks(const GanConvArgs& a) { return cdivl(a.P, kGanK); }

extern "C" int dvc_gan_conv4s2_wgrad_splits(const DvcConvDesc* d) {
    GanConvArgs a;
    if (gan_check_desc("dvc_gan_conv4s2_wgrad_splits", d, a)) return 0;
    return wgrad_default_splits((long)cdiv(a.Cin, kGwCi) * cdiv(a.Cout, kGanM), gan_wgrad_chunks(a));
}

extern "C" int dvc_gan_conv4s2_wgrad(const DvcConvDesc* d, const float* dz, const float* x, int32_t S, float* part,
                                     size_t part_floats, float* out, dvcStream stream) {
    const char* fn = "dvc_gan_conv4s2_wgrad";
    GanConvArgs g;
    if (gan_check_desc(fn, d, g)) return 1;
    DVC_REQUIRE(dz && x && part && out, "%s: null argument", fn);
    DVC_REQUIRE((((uintptr_t)dz | (uintptr_t)x | (uintptr_t)part | (uintptr_t)out) & 3) == 0, "%s: pointers must be 4-byte aligned", fn);
    DVC_REQUIRE((long)g.H * g.W <= 0x7fffffffL, "%s: map too large", fn);
    const long nchunks = gan_wgrad_chunks(g);
    const long ld = (long)g.Cout * g.Cin * 16 + g.Cout;
    if (wgrad_check_frame(fn, S, g.Cin, g.Cout, nchunks, ld, dz, x, part, part_floats, out)) return 1;
    DVC_REQUIRE(cdiv(g.Cout, kGanM) <= 65535, "%s: too many tiles for one launch", fn);
    GanWgradArgs a{dz, x, part, g.N, g.Cin, g.H, g.W, g.Cout, g.OH, g.OW, (int)nchunks, S, g.xbs, g.ybs, g.P, ld};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gan_conv4s2_wgrad_kernel, dim3(cdiv(g.Cin, kGwCi), cdiv(g.Cout, kGanM), S), dim3(256), 0, st, a);
    DVC_CHECK_LAUNCH(fn);
    launch_sum_slots(part, S, ld, ld, out, st);
    DVC_CHECK_LAUNCH("dvc_gan_conv4s2_wgrad (slot sum)");
    return 0;
}

static int gan_dot_check(const char* fn, long count, const void* workspace, size_t workspace_bytes) {
    DVC_REQUIRE(count >= 1, "%s: bad count (%ld)", fn, count);
    const size_t need = (size_t)gan_dot_blocks(count) * sizeof(double);
    DVC_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", fn,
                workspace ? workspace_bytes : 0, need);
    DVC_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", fn);
    return 0;
}

extern "C" size_t dvc_gan_dot_workspace_bytes(int64_t count) {
    return count >= 1 ? (size_t)gan_dot_blocks(count) * sizeof(double) : 0;
}

extern "C" int dvc_gan_dot(const float* a, const float* b, int64_t count, float* out, void* workspace, size_t workspace_bytes,
                           dvcStream stream) {
    const char* fn = "dvc_gan_dot";
    DVC_REQUIRE(a && b && out, "%s: null argument", fn);
    if (gan_dot_check(fn, count, workspace, workspace_bytes)) return 1;
    DVC_REQUIRE(out != a && out != b, "%s: out must not alias an input", fn);
    const int nb = gan_dot_blocks(count);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gan_dot_partial_kernel, dim3(nb), dim3(256), 0, st, a, b, (long)count, (double*)workspace);
    hipLaunchKernelGGL(gan_dot_close_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nb, out);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_sn_wgrad(const float* G, const float* w_bar, const float* u, const float* v, const float* inv_sigma,
                                int32_t Cout, int32_t K, float* out, void* workspace, size_t workspace_bytes, dvcStream stream) {
    const char* fn = "dvc_gan_sn_wgrad";
    DVC_REQUIRE(G && w_bar && u && v && inv_sigma && out, "%s: null argument", fn);
    DVC_REQUIRE(Cout >= 1 && K >= 1 && (long)Cout * K <= 0x7fffffffL, "%s: bad shape (Cout %d, K %d)", fn, Cout, K);
    const long count = (long)Cout * K;
    if (gan_dot_check(fn, count, workspace, workspace_bytes)) return 1;
    DVC_REQUIRE(out != G && out != w_bar && out != u && out != v, "%s: out must not alias an input", fn);
    const int nb = gan_dot_blocks(count);
    const long blocks = cdivl(count, 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gan_dot_partial_kernel, dim3(nb), dim3(256), 0, st, G, w_bar, count, (double*)workspace);
    hipLaunchKernelGGL(gan_sn_wgrad_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, G, u, v, inv_sigma,
                       (const double*)workspace, nb, K, count, out);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_gan_last_wgrad(const float* g, const float* x, int32_t N, int32_t Cin, int32_t H, int32_t W,
                                  int64_t x_batch_stride, float* out, dvcStream stream) {
    const char* fn = "dvc_gan_last_wgrad";
    DVC_REQUIRE(g && x && out, "%s: null argument", fn);
    DVC_REQUIRE(N >= 1 && Cin >= 1 && (long)Cin * 18 <= 0x7fffffffL, "%s: bad shape (N %d, Cin %d)", fn, N, Cin);
    DVC_REQUIRE(H >= 3 && W >= 6, "%s: the map (%d x %d) is smaller than the 3 x 6 filter", fn, H, W);
    DVC_REQUIRE((long)H * W <= 0x7fffffffL, "%s: map too large", fn);
    const long dense = (long)Cin * H * W;
    DVC_REQUIRE(x_batch_stride == 0 || x_batch_stride >= dense, "%s: x_batch_stride (%ld) is below Cin*H*W (%ld)", fn,
                (long)x_batch_stride, dense);
    DVC_REQUIRE(out != g && out != x, "%s: out must not alias an input", fn);
    hipLaunchKernelGGL(gan_last_wgrad_kernel, dim3(Cin), dim3(256), 0, (hipStream_t)stream, g, x, N, Cin, H, W,
                       x_batch_stride ? (long)x_batch_stride : dense, out);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}
