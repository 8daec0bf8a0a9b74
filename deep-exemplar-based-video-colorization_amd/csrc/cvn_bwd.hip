// ColorVidNet's backward (training mode, dvc_amd/nets.py): the weight gradients of its convolutions, the head, and the
// InstanceNorm steps.  The 3x3 input gradients run on the forward's engines with transposed, flipped filters (as VGG19's do);
// what is here is what those engines do not do:
//   dvc_cvn_wgrad      dW[co][ci][ky][kx] = sum_{b,y,x} dZ[b,co,y,x] X[b,ci,y+(ky-1)d,x+(kx-1)d],  db[co] = sum dZ
//                      on v_mfma_f32_32x32x2_f32 (exact fp32), positions split over workgroups, partials summed in slot order
//                      (the slot sums and the bias sums run in double and are rounded once)
//   dvc_cvn_head_bwd   conv10_ab (1x1, 2 outputs) + tanh*128: d c10_2 through the leaky mask, dW_ab, db_ab
//   dvc_cvn_inorm_bwd  InstanceNorm backward with up to three consumers, the producing layer's ReLU mask, and the `_ss` weights'
//                      gradient
// Every sum has a fixed order: the results are bit-deterministic and do not depend on timing.
#include "bwd_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ 3x3 weight gradient
// Per tap this is a GEMM [Cout x P] . [P x Cin] whose operands are both contiguous along positions.  A workgroup owns a 64 (co) x
// 64 (ci) tile of all nine taps and a contiguous range of 16-position chunks (one image row segment each).  Per chunk it stages
// dZ [64][16] and, for every (ci, ky, kx), the 16-position window of X that tap reads (zero outside the map; for in_up = 2 the
// half-resolution map is read through nearest x2 indexing) into LDS, then each wave runs 9 taps x 8 MFMAs on its 32 x 32 quarter.
// The K order inside a chunk is permuted (lane half h takes positions 8h..8h+7) so that both operands are float4 reads.
constexpr int kWgT = kWgTile;    // co / ci tile
constexpr int kWgP = 16;         // positions per chunk
constexpr int kWgZs = kWgP + 4;  // LDS row stride of dZ
constexpr int kWgXs = 9 * kWgP + 4;  // LDS row stride (per ci) of the nine tap windows

struct WgradArgs {
    const float* dZ;   // [N][Cout][H][W]
    const float* X;    // [N][Cin][XH][XW]  (XH = H / in_up)
    float* part;       // [S][Cout*Cin*9 + Cout]
    int N, Cin, Cout, H, W, XH, XW, ncx, nchunks, S;
    long ld;
};

template <int DIL, int UP>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
    __shared__ __attribute__((aligned(16))) float sZ[kWgT * kWgZs];
    __shared__ __attribute__((aligned(16))) float sX[kWgT * kWgXs];
    constexpr int L = kWgP + 2 * DIL;          // columns of one X row a chunk needs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int ci0 = blockIdx.x * kWgT, co0 = blockIdx.y * kWgT, sp = blockIdx.z;
    const int wco = (wave & 1) * 32, wci = (wave >> 1) * 32;
    int c_beg, c_end;
    wgrad_chunk_range(sp, a.nchunks, a.S, c_beg, c_end);
    const bool do_bias = blockIdx.x == 0;

    f16v acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    double bacc = 0.0;      // (db is a plain sum over every position of the slot: a double chain, rounded once per slot)

    const long HW = (long)a.H * a.W, XHW = (long)a.XH * a.XW;
    for (int c = c_beg; c < c_end; ++c) {
        const int b = c / (a.H * a.ncx);
        const int rem = c - b * a.H * a.ncx;
        const int y = rem / a.ncx, x0 = (rem - (rem / a.ncx) * a.ncx) * kWgP;
        // dZ chunk
        const float* zb = a.dZ + ((long)b * a.Cout + co0) * HW + (long)y * a.W + x0;
#pragma unroll
        for (int k = 0; k < kWgT * kWgP / 256; ++k) {
            const int e = tid + 256 * k, co = e / kWgP, s = e % kWgP;
            float v = 0.f;
            if (co0 + co < a.Cout && x0 + s < a.W) v = zb[(long)co * HW + s];
            sZ[co * kWgZs + s] = v;
        }
        // X windows: each (ci, ky, column) is loaded once and written to the (up to three) kx windows that contain it
        const float* xb = a.X + ((long)b * a.Cin + ci0) * XHW;
        for (int e = tid; e < kWgT * 3 * L; e += 256) {
            const int ci = e / (3 * L), r = e - ci * (3 * L), ky = r / L, col = r - ky * L;
            const int yy = y + (ky - 1) * DIL, xx = x0 - DIL + col;
            float v = 0.f;
            if (ci0 + ci < a.Cin && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W)
                v = xb[(long)ci * XHW + (long)(yy / UP) * a.XW + xx / UP];
            float* row = sX + ci * kWgXs + ky * 3 * kWgP;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int s = col - kx * DIL;
                if (s >= 0 && s < kWgP) row[kx * kWgP + s] = v;
            }
        }
        __syncthreads();
        if (do_bias && tid < kWgT) {
#pragma unroll
            for (int s = 0; s < kWgP; ++s) bacc += (double)sZ[tid * kWgZs + s];
        }
        const float4* za = reinterpret_cast<const float4*>(sZ + (wco + l31) * kWgZs + hi * 8);
        const float4 z0 = za[0], z1 = za[1];
        const float av[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float4* xa = reinterpret_cast<const float4*>(sX + (wci + l31) * kWgXs + t * kWgP + hi * 8);
            const float4 x0v = xa[0], x1v = xa[1];
            const float bv[8] = {x0v.x, x0v.y, x0v.z, x0v.w, x1v.x, x1v.y, x1v.z, x1v.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    float* slot = a.part + (long)sp * a.ld;
    wgrad_store_tile<9>(slot, acc, ci0 + wci + l31, co0 + wco, hi, a.Cin, a.Cout);
    wgrad_store_bias<9>(slot, do_bias, tid, co0, a.Cin, a.Cout, bacc);
}

// ------------------------------------------------------------------------------------------------ head backward
// One workgroup per (image, 256 positions).  dpre_o = g_o * 128 * (1 - (ab_o / 128)^2) goes to LDS; then wave w takes channels
// w, w+4, ...: dZ = (W0c dpre0 + W1c dpre1) * (R > 0 ? 1 : slope) and the partial sums dpre_o * R for dW_ab (a fixed butterfly
// over the wave).  Slot layout [2][C] then [2] (the bias).
constexpr int kHdP = 256;
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ ab, const float* __restrict__ g,
                                                       const float* __restrict__ w, const float* __restrict__ R, int C, int HW,
                                                       float slope, int nbx, float* __restrict__ dZ, float* __restrict__ part) {
    __shared__ float sd[2][kHdP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, p0 = blockIdx.x * kHdP;
    {
        const int p = p0 + tid;
        float d0 = 0.f, d1 = 0.f;
        if (p < HW) {
            const float* abb = ab + (long)b * 2 * HW;
            const float* gb = g + (long)b * 2 * HW;
            const float a0 = abb[p] * (1.f / 128.f), a1 = abb[HW + p] * (1.f / 128.f);
            d0 = gb[p] * 128.f * (1.f - a0 * a0);
            d1 = gb[HW + p] * 128.f * (1.f - a1 * a1);
        }
        sd[0][tid] = d0;
        sd[1][tid] = d1;
    }
    __syncthreads();
    float* slot = part + ((long)b * nbx + blockIdx.x) * (2L * C + 2);
    for (int c = wave; c < C; c += 4) {
        const float w0 = w[c], w1 = w[C + c];
        const float* rc = R + ((long)b * C + c) * HW;
        float* zc = dZ + ((long)b * C + c) * HW;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < kHdP / 64; ++k) {
            const int q = lane + 64 * k, p = p0 + q;
            if (p < HW) {
                const float r = rc[p], d0 = sd[0][q], d1 = sd[1][q];
                zc[p] = (w0 * d0 + w1 * d1) * (r > 0.f ? 1.f : slope);
                s0 = fmaf(d0, r, s0);
                s1 = fmaf(d1, r, s1);
            }
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) {
            slot[c] = s0;
            slot[C + c] = s1;
        }
    }
    if (tid < 2) {
        double s = 0.0;
        for (int q = 0; q < kHdP; ++q) s += (double)sd[tid][q];
        slot[2 * C + tid] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------ InstanceNorm backward
// One workgroup per (image, channel) plane.  dn = g_full + [even y, x] ss_c g_ss(y/2, x/2) + (2x2 sum of g_up);
// dZ = rstd (dn - mean(dn) - n mean(dn n)) * [R > 0];  ss_part = sum_{even y, x} n g_ss.
constexpr int kNbT = 512;

__global__ __launch_bounds__(kNbT) void inorm_bwd_kernel(const float* __restrict__ n, const float* __restrict__ rstd,
                                                         const float* __restrict__ R, const float* __restrict__ gf,
                                                         const float* __restrict__ gs, const float* __restrict__ ssw,
                                                         const float* __restrict__ gu, int C, int H, int W,
                                                         float* __restrict__ dZ, float* __restrict__ ss_part) {
    __shared__ float red[kNbT / 64];
    const int plane = blockIdx.x, c = plane % C;
    const long HW = (long)H * W;
    const int Hs = (H + 1) / 2, Ws = (W + 1) / 2;
    const float* np = n + plane * HW;
    const float* gfp = gf ? gf + plane * HW : nullptr;
    const float* gsp = gs ? gs + (long)plane * Hs * Ws : nullptr;
    const float* gup = gu ? gu + plane * 4 * HW : nullptr;
    const float ss = gs ? ssw[c] : 0.f;
    auto dn_at = [&](long p, float& gsv) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        float d = gfp ? gfp[p] : 0.f;
        gsv = 0.f;
        if (gsp && !(y & 1) && !(x & 1)) {
            gsv = gsp[(long)(y >> 1) * Ws + (x >> 1)];
            d += ss * gsv;
        }
        if (gup) {
            const float* u = gup + (long)(2 * y) * (2 * W) + 2 * x;
            d += (u[0] + u[1]) + (u[2 * W] + u[2 * W + 1]);
        }
        return d;
    };
    float sd = 0.f, sdn = 0.f, sg = 0.f;
    for (long p = threadIdx.x; p < HW; p += kNbT) {
        float gsv;
        const float d = dn_at(p, gsv), nv = np[p];
        sd += d;
        sdn = fmaf(d, nv, sdn);
        sg = fmaf(nv, gsv, sg);
    }
    const float inv = 1.f / (float)HW;
    const float md = block_sum<float, kNbT>(sd, red) * inv;
    const float mdn = block_sum<float, kNbT>(sdn, red) * inv;
    if (gsp) {
        const float s = block_sum<float, kNbT>(sg, red);
        if (threadIdx.x == 0) ss_part[plane] = s;
    }
    const float r = rstd[plane];
    const float* Rp = R + plane * HW;
    float* zp = dZ + plane * HW;
    for (long p = threadIdx.x; p < HW; p += kNbT) {
        float gsv;
        const float d = dn_at(p, gsv);
        const float v = r * (d - md - np[p] * mdn);
        zp[p] = Rp[p] > 0.f ? v : 0.f;
    }
}

}  // namespace

// ================================================================================================ C entry points
extern "C" int dvc_cvn_wgrad_splits(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
    const long tiles = (long)cdiv(Cin, kWgT) * cdiv(Cout, kWgT);
    const long chunks = (long)N * H * cdiv(W, kWgP);
    return wgrad_default_splits(tiles, chunks);
}

extern "C" int dvc_cvn_wgrad(const float* dZ, const float* X, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W,
                             int32_t dil, int32_t in_up, int32_t S, float* part, size_t part_floats, float* out,
                             dvcStream stream) {
    DVC_REQUIRE(dZ && X && part && out, "dvc_cvn_wgrad: null pointer");
    DVC_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "dvc_cvn_wgrad: bad size (N %d Cin %d Cout %d H %d W %d)", N, Cin,
                Cout, H, W);
    DVC_REQUIRE(dil == 1 || dil == 2, "dvc_cvn_wgrad: dil must be 1 or 2 (got %d)", dil);
    DVC_REQUIRE(in_up == 1 || in_up == 2, "dvc_cvn_wgrad: in_up must be 1 or 2 (got %d)", in_up);
    DVC_REQUIRE(in_up == 1 || (H % 2 == 0 && W % 2 == 0), "dvc_cvn_wgrad: in_up = 2 needs even H and W");
    const int ncx = cdiv(W, kWgP);
    const long nchunks = (long)N * H * ncx;
    const long ld = (long)Cout * Cin * 9 + Cout;
    if (wgrad_check_frame("dvc_cvn_wgrad", S, Cin, Cout, nchunks, ld, dZ, X, part, part_floats, out)) return 1;
    WgradArgs a{dZ, X, part, N, Cin, Cout, H, W, H / in_up, W / in_up, ncx, (int)nchunks, S, ld};
    const dim3 grid(cdiv(Cin, kWgT), cdiv(Cout, kWgT), S);
    hipStream_t st = (hipStream_t)stream;
    if (dil == 1 && in_up == 1)
        hipLaunchKernelGGL((wgrad_kernel<1, 1>), grid, dim3(256), 0, st, a);
    else if (dil == 1)
        hipLaunchKernelGGL((wgrad_kernel<1, 2>), grid, dim3(256), 0, st, a);
    else if (in_up == 1)
        hipLaunchKernelGGL((wgrad_kernel<2, 1>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((wgrad_kernel<2, 2>), grid, dim3(256), 0, st, a);
    DVC_CHECK_LAUNCH("dvc_cvn_wgrad");
    launch_sum_slots(part, S, ld, ld, out, st);
    DVC_CHECK_LAUNCH("dvc_cvn_wgrad (slot sum)");
    return 0;
}

extern "C" size_t dvc_cvn_head_bwd_workspace_floats(int32_t N, int32_t C, int32_t HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    return (size_t)N * cdiv(HW, kHdP) * (2 * (size_t)C + 2);
}

extern "C" int dvc_cvn_head_bwd(const float* ab, const float* grad_ab, const float* w_ab, const float* R, int32_t N, int32_t C,
                                int32_t HW, float slope, float* dZ, float* part, size_t part_floats, float* out,
                                dvcStream stream) {
    DVC_REQUIRE(ab && grad_ab && w_ab && R && dZ && part && out, "dvc_cvn_head_bwd: null pointer");
    DVC_REQUIRE(N > 0 && C > 0 && HW > 0, "dvc_cvn_head_bwd: bad size (N %d C %d HW %d)", N, C, HW);
    DVC_REQUIRE(N <= 65535, "dvc_cvn_head_bwd: N must be <= 65535");
    DVC_REQUIRE(part_floats >= dvc_cvn_head_bwd_workspace_floats(N, C, HW), "dvc_cvn_head_bwd: workspace too small");
    DVC_REQUIRE(dZ != R && dZ != ab && dZ != grad_ab, "dvc_cvn_head_bwd: dZ must not alias an input");
    const int nbx = cdiv(HW, kHdP);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(head_bwd_kernel, dim3(nbx, N), dim3(256), 0, st, ab, grad_ab, w_ab, R, (int)C, (int)HW, slope, nbx, dZ,
                       part);
    DVC_CHECK_LAUNCH("dvc_cvn_head_bwd");
    launch_sum_slots(part, N * nbx, 2L * C + 2, 2L * C + 2, out, st);
    DVC_CHECK_LAUNCH("dvc_cvn_head_bwd (slot sum)");
    return 0;
}

extern "C" int dvc_cvn_inorm_bwd(const float* n, const float* rstd, const float* R, const float* g_full, const float* g_ss,
                                 const float* ss_w, const float* g_up, int32_t N, int32_t C, int32_t H, int32_t W, float* dZ,
                                 float* ss_part, float* ss_grad, dvcStream stream) {
    DVC_REQUIRE(n && rstd && R && dZ, "dvc_cvn_inorm_bwd: null pointer (n, rstd, R and dZ are required)");
    DVC_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "dvc_cvn_inorm_bwd: bad size (N %d C %d H %d W %d)", N, C, H, W);
    DVC_REQUIRE(g_full || g_ss || g_up, "dvc_cvn_inorm_bwd: no incoming gradient");
    DVC_REQUIRE(!g_ss || (ss_w && ss_part && ss_grad), "dvc_cvn_inorm_bwd: g_ss needs ss_w, ss_part and ss_grad");
    DVC_REQUIRE((long)N * C < (1L << 31) && (long)H * W * 4 < (1L << 31), "dvc_cvn_inorm_bwd: tensor too large");
    DVC_REQUIRE(dZ != n && dZ != R && dZ != g_full && dZ != g_ss && dZ != g_up, "dvc_cvn_inorm_bwd: dZ must not alias an input");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(inorm_bwd_kernel, dim3(N * C), dim3(kNbT), 0, st, n, rstd, R, g_full, g_ss, ss_w, g_up, (int)C, (int)H,
                       (int)W, dZ, ss_part);
    DVC_CHECK_LAUNCH("dvc_cvn_inorm_bwd");
    if (g_ss) {
        launch_sum_slots(ss_part, N, C, C, ss_grad, st);
        DVC_CHECK_LAUNCH("dvc_cvn_inorm_bwd (image sum)");
    }
    return 0;
}
