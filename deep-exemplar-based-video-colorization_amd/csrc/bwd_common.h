// What the backward files (cvn_bwd.hip, warp_bwd.hip) share: the fixed-order slot sum, the fixed-order block sum (reduce.h), and
// the frame of the two fp32-MFMA weight-gradient kernels (slot heuristic, chunk range, epilogue stores, host-side checks).  The
// library is built with -fno-gpu-rdc: everything here is in an anonymous namespace and each including file gets its own instance.
#pragma once
#include "common.h"
#include "reduce.h"

namespace {

// ------------------------------------------------------------------------------------------------ fixed-order slot sum
// out[i] = part[0][i] + part[1][i] + ... + part[S-1][i]   (slot stride `ld` floats)
// The running sum is a double, rounded once at the end: a layer at 216x384 has hundreds of slots, and an fp32 chain over them
// put the bias gradients of the full-resolution layers at 5x what a float32 pairwise sum makes (tests/test_gpu_bwd_audit.py).
__global__ __launch_bounds__(256) void sum_slots_kernel(const float* __restrict__ part, int S, long ld, long n,
                                                        float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        double s = part[i];
        for (int k = 1; k < S; ++k) s += (double)part[(long)k * ld + i];
        out[i] = (float)s;
    }
}

static int launch_sum_slots(const float* part, int S, long ld, long n, float* out, hipStream_t st) {
    const long blocks = cdivl(n, 256);
    hipLaunchKernelGGL(sum_slots_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, part, S, ld, n, out);
    return 0;
}

// ------------------------------------------------------------------------------------------------ weight-gradient frame
// Both weight-gradient kernels (wgrad_kernel: 3x3, 16-position chunks; k1_wgrad_kernel: 1x1, 32-position chunks) give a 256-thread
// workgroup a 64 (co) x 64 (ci) tile — wave w the 32 x 32 quarter at (wco, wci) = ((w & 1) * 32, (w >> 1) * 32) — and slot `sp` of S
// a contiguous range of position chunks; the workgroups with blockIdx.x == 0 also add up the bias gradient of their 64 output
// channels, a double chain rounded once per slot.  A slot is [Cout][Cin][TAPS] then [Cout]; sum_slots_kernel adds the slots.
// The main loops differ (chunk shape, staging, K order inside a chunk) and stay with their kernels.
constexpr int kWgTile = 64;

typedef float f16v __attribute__((ext_vector_type(16)));

// The default slot count: about two workgroups per CU (256 CUs) and at least four chunks per workgroup.
static int wgrad_default_splits(long tiles, long chunks) {
    long s = cdivl(512, tiles);
    const long cap = chunks / 4 > 1 ? chunks / 4 : 1;
    if (s > cap) s = cap;
    if (s > 65535) s = 65535;
    return (int)(s < 1 ? 1 : s);
}

// [c_beg, c_end): the chunks of slot sp
__device__ __forceinline__ void wgrad_chunk_range(int sp, int nchunks, int S, int& c_beg, int& c_end) {
    c_beg = (int)((long)sp * nchunks / S);
    c_end = (int)((long)(sp + 1) * nchunks / S);
}

// A wave's 32 x 32 accumulators (one f16v per tap) into the slot.  ci = ci0 + wci + (lane & 31), co_base = co0 + wco, hi = lane >> 5.
// C/D layout: column (ci) = lane & 31, row (co) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
template <int TAPS>
__device__ __forceinline__ void wgrad_store_tile(float* slot, const f16v* acc, int ci, int co_base, int hi, int Cin, int Cout) {
    if (ci < Cin) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co_base + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (co < Cout) {
                float* dst = slot + ((long)co * Cin + ci) * TAPS;
#pragma unroll
                for (int t = 0; t < TAPS; ++t) dst[t] = acc[t][r];
            }
        }
    }
}

// The bias sums of the tile's output channels (threads 0..63 of the blockIdx.x == 0 workgroups) behind the slot's weights.
template <int TAPS>
__device__ __forceinline__ void wgrad_store_bias(float* slot, bool do_bias, int tid, int co0, int Cin, int Cout, double bacc) {
    if (do_bias && tid < kWgTile && co0 + tid < Cout) slot[(long)Cout * Cin * TAPS + co0 + tid] = (float)bacc;
}

// The checks both entry points make on their slot count, grid and workspace; `fn` is the entry point's name in the message.
static int wgrad_check_frame(const char* fn, int S, int Cin, int Cout, long nchunks, long ld, const void* in0, const void* in1,
                             const float* part, size_t part_floats, const float* out) {
    DVC_REQUIRE(S >= 1 && S <= 65535, "%s: S must be in [1, 65535] (got %d)", fn, S);
    DVC_REQUIRE(Cout <= 65535 * kWgTile && Cin <= 65535 * kWgTile, "%s: too many channels", fn);
    DVC_REQUIRE(nchunks < (1L << 30), "%s: map too large", fn);
    DVC_REQUIRE(part_floats >= (size_t)S * ld, "%s: workspace too small (%zu floats, need %ld)", fn, part_floats, (long)S * ld);
    DVC_REQUIRE(out != in0 && out != in1 && part != in0 && part != in1 && part != out, "%s: outputs must not alias inputs", fn);
    return 0;
}

}  // namespace
