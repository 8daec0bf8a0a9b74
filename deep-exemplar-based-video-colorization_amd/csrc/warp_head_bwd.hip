// WarpNet's backward through its four heads (training mode with WarpNet.set_head_training, dvc_amd/nets.py).  The heads' norm +
// PReLU sites run on dvc_warp_norm_prelu_bwd, their 3x3 input gradients on the forward's engines (W^T flipped on a zero-ringed
// map, then dvc_warp_fold), as the residual trunk's do (warp_bwd.hip); what is here is what the heads add:
//   dvc_warp_head_wgrad      dW[co][ci][ky][kx] = sum_{b,oy,ox} dz[b,co,oy,ox] Xp[b,ci,s oy + ky,s ox + kx],  db[co] = sum dz
//                            of a 3x3 reflect-pad-1 convolution of stride s in {1, 2}, from the zero-ringed dz that
//                            dvc_warp_norm_prelu_bwd writes and the reflect-padded input Xp (dvc_warp_reflect_pad), on
//                            v_mfma_f32_32x32x2_f32 (exact fp32); positions split over slots, slots summed in order (in double)
//   dvc_warp_dilate_ring     dz of a stride-2 layer spread onto the odd rows / columns of a zero (H+2) x (W+2) map: the map the
//                            3x3 engines turn into the gradient at the reflect-padded input (zero pad 1, W^T flipped)
//   dvc_warp_up2_bwd         2x2 block sums (backward of a x2 nearest upsample)
//   dvc_warp_rpad_rows_bwd   backward of replicated rows top and bottom: they are added onto the first / last row
// Every sum has a fixed order: the results are bit-deterministic and do not depend on timing.
#include <cstdint>

#include "bwd_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ strided 3x3 weight gradient
// The frame of dvc_cvn_wgrad (bwd_common.h): a workgroup owns a 64 (co) x 64 (ci) tile of all nine taps and a contiguous range of
// 16-position chunks, a chunk being 16 consecutive output columns of one output row of one image.  Per chunk it stages dz [64][16]
// and, for every (ci, tap), the 16 input values that tap multiplies — Xp[s oy + ky][s (ox0 + j) + kx] — into LDS, then each wave
// runs 9 taps x 8 MFMAs on its 32 x 32 quarter.  Only the positions a stride-2 layer really has are multiplied: a quarter of
// the matrix work of the stride-1 gradient of a dilated dz.  Lane half h takes positions 8h..8h+7 of the chunk.
constexpr int kHwT = kWgTile;
constexpr int kHwP = 16;
constexpr int kHwZs = kHwP + 4;
constexpr int kHwXs = 9 * kHwP + 4;

struct HeadWgradArgs {
    const float* dzr;   // [N][Cout][Ho+2][Wo+2], zero ring
    const float* Xp;    // [N][Cin][H+2][W+2]
    float* part;        // [S][Cout*Cin*9 + Cout]
    int N, Cin, Cout, H, W, Ho, Wo, ncx, nchunks, S;
    long ld;
};

template <int STRIDE>
__global__ __launch_bounds__(256) void head_wgrad_kernel(HeadWgradArgs a) {
    __shared__ __attribute__((aligned(16))) float sZ[kHwT * kHwZs];
    __shared__ __attribute__((aligned(16))) float sX[kHwT * kHwXs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int ci0 = blockIdx.x * kHwT, co0 = blockIdx.y * kHwT, sp = blockIdx.z;
    const int wco = (wave & 1) * 32, wci = (wave >> 1) * 32;
    int c_beg, c_end;
    wgrad_chunk_range(sp, a.nchunks, a.S, c_beg, c_end);
    const bool do_bias = blockIdx.x == 0;

    f16v acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    double bacc = 0.0;

    const int ZW = a.Wo + 2, PW = a.W + 2;
    const long ZHW = (long)(a.Ho + 2) * ZW, PHW = (long)(a.H + 2) * PW;
    for (int c = c_beg; c < c_end; ++c) {
        const int b = c / (a.Ho * a.ncx);
        const int rem = c - b * a.Ho * a.ncx;
        const int oy = rem / a.ncx, ox0 = (rem - oy * a.ncx) * kHwP;
        // dz chunk (the interior of the ringed plane)
        const float* zb = a.dzr + ((long)b * a.Cout + co0) * ZHW + (long)(oy + 1) * ZW + ox0 + 1;
#pragma unroll
        for (int k = 0; k < kHwT * kHwP / 256; ++k) {
            const int e = tid + 256 * k, co = e / kHwP, j = e % kHwP;
            float v = 0.f;
            if (co0 + co < a.Cout && ox0 + j < a.Wo) v = zb[(long)co * ZHW + j];
            sZ[co * kHwZs + j] = v;
        }
        // the nine tap windows: every slot is written, with 0 behind the row's last output column and for absent channels
        // (an output column ox < Wo reads padded columns up to s (Wo - 1) + 2 <= W + 1, rows up to s (Ho - 1) + 2 <= H + 1)
        const float* xb = a.Xp + ((long)b * a.Cin + ci0) * PHW + (long)(STRIDE * oy) * PW;
        for (int e = tid; e < kHwT * 9 * kHwP; e += 256) {
            const int ci = e / (9 * kHwP), r = e - ci * (9 * kHwP), t = r / kHwP, j = r - t * kHwP;
            const int ky = t / 3, kx = t - ky * 3;
            float v = 0.f;
            if (ci0 + ci < a.Cin && ox0 + j < a.Wo) v = xb[(long)ci * PHW + (long)ky * PW + STRIDE * (ox0 + j) + kx];
            sX[ci * kHwXs + r] = v;
        }
        __syncthreads();
        if (do_bias && tid < kHwT) {
#pragma unroll
            for (int j = 0; j < kHwP; ++j) bacc += (double)sZ[tid * kHwZs + j];
        }
        const float4* za = reinterpret_cast<const float4*>(sZ + (wco + l31) * kHwZs + hi * 8);
        const float4 z0 = za[0], z1 = za[1];
        const float av[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float4* xa = reinterpret_cast<const float4*>(sX + (wci + l31) * kHwXs + t * kHwP + hi * 8);
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

// ------------------------------------------------------------------------------------------------ stride-2 dz onto a zero map
// out[1 + 2 oy][1 + 2 ox] = dz[oy][ox], 0 elsewhere (Ho = (H - 1) / 2 + 1: the last dz row lands on row H or H - 1 <= H + 1)
__global__ __launch_bounds__(256) void dilate_ring_kernel(const float* __restrict__ dzr, long total, int Ho, int Wo, int H, int W,
                                                          float* __restrict__ out) {
    const int PW = W + 2, PHW = (H + 2) * PW, ZW = Wo + 2, ZHW = (Ho + 2) * ZW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long plane = i / PHW;
        const int r = (int)(i - plane * PHW), py = r / PW, px = r - py * PW;
        float v = 0.f;
        if ((py & 1) && (px & 1)) {
            const int oy = py >> 1, ox = px >> 1;
            if (oy < Ho && ox < Wo) v = dzr[plane * ZHW + (long)(oy + 1) * ZW + ox + 1];
        }
        out[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------ x2 upsample backward
__global__ __launch_bounds__(256) void up2_bwd_kernel(const float* __restrict__ g, long total, int h, int w,
                                                      float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long plane = i / ((long)h * w);
        const int r = (int)(i - plane * h * w), y = r / w, x = r - y * w;
        const float* gp = g + plane * 4L * h * w + (long)(2 * y) * (2 * w) + 2 * x;
        out[i] = (gp[0] + gp[1]) + (gp[2 * w] + gp[2 * w + 1]);
    }
}

// ------------------------------------------------------------------------------------------------ replicated rows backward
// g [planes][h + 2 rpad][w] -> out [planes][h][w]: row y takes g row y + rpad; row 0 also the rpad rows above it (top down),
// row h - 1 the rpad rows below it
__global__ __launch_bounds__(256) void rpad_rows_bwd_kernel(const float* __restrict__ g, long total, int h, int w, int rpad,
                                                            float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long plane = i / ((long)h * w);
        const int r = (int)(i - plane * h * w), y = r / w, x = r - y * w;
        const float* gp = g + plane * (long)(h + 2 * rpad) * w + x;
        float s = gp[(long)(y + rpad) * w];
        if (y == 0)
            for (int k = 0; k < rpad; ++k) s += gp[(long)k * w];
        if (y == h - 1)
            for (int k = 0; k < rpad; ++k) s += gp[(long)(h + rpad + k) * w];
        out[i] = s;
    }
}

static unsigned grid_for(long total) {
    const long blocks = cdivl(total, 256);
    return (unsigned)(blocks < 16384 ? blocks : 16384);
}

static bool head_out_size_ok(int H, int Ho, int stride) { return Ho == (H - 1) / stride + 1; }

}  // namespace

// ================================================================================================ C entry points
extern "C" int dvc_warp_head_wgrad_splits(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t stride) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H < 2 || W < 2 || (stride != 1 && stride != 2)) return 0;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long tiles = (long)cdiv(Cin, kHwT) * cdiv(Cout, kHwT);
    const long chunks = (long)N * Ho * cdiv(Wo, kHwP);
    return wgrad_default_splits(tiles, chunks);
}

extern "C" int dvc_warp_head_wgrad(const float* dz_ringed, const float* x_padded, int32_t N, int32_t Cin, int32_t Cout, int32_t H,
                                   int32_t W, int32_t stride, int32_t S, float* part, size_t part_floats, float* out,
                                   dvcStream stream) {
    DVC_REQUIRE(dz_ringed && x_padded && part && out, "dvc_warp_head_wgrad: null pointer");
    DVC_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H >= 2 && W >= 2,
                "dvc_warp_head_wgrad: bad size (N %d Cin %d Cout %d H %d W %d; H, W >= 2)", N, Cin, Cout, H, W);
    DVC_REQUIRE(stride == 1 || stride == 2, "dvc_warp_head_wgrad: stride must be 1 or 2 (got %d)", stride);
    DVC_REQUIRE(((long)H + 2) * ((long)W + 2) < (1L << 30), "dvc_warp_head_wgrad: plane too large");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int ncx = cdiv(Wo, kHwP);
    const long nchunks = (long)N * Ho * ncx;
    const long ld = (long)Cout * Cin * 9 + Cout;
    if (wgrad_check_frame("dvc_warp_head_wgrad", S, Cin, Cout, nchunks, ld, dz_ringed, x_padded, part, part_floats, out)) return 1;
    HeadWgradArgs a{dz_ringed, x_padded, part, N, Cin, Cout, H, W, Ho, Wo, ncx, (int)nchunks, S, ld};
    const dim3 grid(cdiv(Cin, kHwT), cdiv(Cout, kHwT), S);
    hipStream_t st = (hipStream_t)stream;
    if (stride == 1)
        hipLaunchKernelGGL((head_wgrad_kernel<1>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((head_wgrad_kernel<2>), grid, dim3(256), 0, st, a);
    DVC_CHECK_LAUNCH("dvc_warp_head_wgrad");
    launch_sum_slots(part, S, ld, ld, out, st);
    DVC_CHECK_LAUNCH("dvc_warp_head_wgrad (slot sum)");
    return 0;
}

extern "C" int dvc_warp_dilate_ring(const float* dz_ringed, int32_t planes, int32_t Ho, int32_t Wo, int32_t H, int32_t W,
                                    float* out, dvcStream stream) {
    DVC_REQUIRE(dz_ringed && out, "dvc_warp_dilate_ring: null pointer");
    DVC_REQUIRE(planes > 0 && H >= 2 && W >= 2 && Ho > 0 && Wo > 0,
                "dvc_warp_dilate_ring: bad size (planes %d Ho %d Wo %d H %d W %d; H, W >= 2)", planes, Ho, Wo, H, W);
    DVC_REQUIRE(head_out_size_ok(H, Ho, 2) && head_out_size_ok(W, Wo, 2),
                "dvc_warp_dilate_ring: Ho x Wo = %d x %d is not the stride-2 output size of %d x %d", Ho, Wo, H, W);
    DVC_REQUIRE(((long)H + 2) * ((long)W + 2) < (1L << 30), "dvc_warp_dilate_ring: plane too large");
    DVC_REQUIRE(out != dz_ringed, "dvc_warp_dilate_ring: out must not alias dz_ringed");
    const long total = (long)planes * (H + 2) * (W + 2);
    hipLaunchKernelGGL(dilate_ring_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dz_ringed, total, (int)Ho,
                       (int)Wo, (int)H, (int)W, out);
    DVC_CHECK_LAUNCH("dvc_warp_dilate_ring");
    return 0;
}

extern "C" int dvc_warp_up2_bwd(const float* g, int32_t planes, int32_t h, int32_t w, float* out, dvcStream stream) {
    DVC_REQUIRE(g && out, "dvc_warp_up2_bwd: null pointer");
    DVC_REQUIRE(planes > 0 && h > 0 && w > 0, "dvc_warp_up2_bwd: bad size (planes %d h %d w %d)", planes, h, w);
    DVC_REQUIRE((long)h * w < (1L << 28), "dvc_warp_up2_bwd: plane too large");
    DVC_REQUIRE(g != out, "dvc_warp_up2_bwd: out must not alias g");
    const long total = (long)planes * h * w;
    hipLaunchKernelGGL(up2_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g, total, (int)h, (int)w, out);
    DVC_CHECK_LAUNCH("dvc_warp_up2_bwd");
    return 0;
}

extern "C" int dvc_warp_rpad_rows_bwd(const float* g, int32_t planes, int32_t h, int32_t w, int32_t rpad, float* out,
                                      dvcStream stream) {
    DVC_REQUIRE(g && out, "dvc_warp_rpad_rows_bwd: null pointer");
    DVC_REQUIRE(planes > 0 && h > 0 && w > 0 && rpad >= 1 && rpad <= 64,
                "dvc_warp_rpad_rows_bwd: bad size (planes %d h %d w %d rpad %d; 1 <= rpad <= 64)", planes, h, w, rpad);
    DVC_REQUIRE(((long)h + 2 * rpad) * w < (1L << 30), "dvc_warp_rpad_rows_bwd: plane too large");
    DVC_REQUIRE(g != out, "dvc_warp_rpad_rows_bwd: out must not alias g");
    const long total = (long)planes * h * w;
    hipLaunchKernelGGL(rpad_rows_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g, total, (int)h, (int)w,
                       (int)rpad, out);
    DVC_CHECK_LAUNCH("dvc_warp_rpad_rows_bwd");
    return 0;
}
