// train.py's pixel losses — every term scale * mean(w * |x - t|^p), p in {1, 2}, of a training step — on one fused reduction
// (dvc_loss_fwd, dvc_loss_bwd; the contract is in include/dvc_hip.h, the driver is dvc_amd/losses.py, the design, the error bound
// and the measured rates are in DESIGN.md §6d).
//
// Pure streaming, like csrc/optim.hip: a chunk walker around 16-byte loads.  256 threads x 4 floats = 1,024 elements per pass,
// DVC_LOSS_CHUNK = 4 passes; the grid is min(chunks, 256 CUs x 8 workgroups) and strides over the chunk table.  The descriptors of
// a chunk are wave-uniform and arrive by scalar loads.
//
// The ORDER is the point.  Thread j of a chunk owns the elements 4 (j + 256 r) + k, r = 0..3, k = 0..3, whichever path loads them,
// and adds their fp32 values w * |d|^p into a double in that order; block_sum<double, 256> (reduce.h, CHAIN order) combines the 256
// doubles and thread 0 stores the chunk's partial with an ordinary store.  A partial depends on the chunk's data alone — not on
// the grid, on the workgroup that ran it, on the alignment that chose the load path, or on what else is in the launch.  Stage 2
// (one workgroup) adds a term's partials j, j + 256, ... in thread j, block_sum again, and the terms' doubles in term order for
// the total.  No atomics, no counters, no inline assembly.
//
// Contraction is off: the roundings are the ones written here (tests/losses_reference.py counts them).
#include "common.h"
#include "reduce.h"

#include <cstdint>

#pragma clang fp contract(off)

#include "loss_chunk.h"     // the element and chunk code, shared with csrc/loss_plan.hip

static_assert(sizeof(DvcLossTerm) == 80 && sizeof(DvcLossChunk) == 16, "table layouts are part of the ABI (dvc_amd/_lib.py)");

namespace {

#define LOSS_DISPATCH(FN, ...)                                              \
    do {                                                                    \
        if (p == 2) {                                                       \
            if (wm == kWNone) FN<2, kWNone>(__VA_ARGS__);                   \
            else if (wm == kWFull) FN<2, kWFull>(__VA_ARGS__);              \
            else FN<2, kWBcast>(__VA_ARGS__);                               \
        } else {                                                            \
            if (wm == kWNone) FN<1, kWNone>(__VA_ARGS__);                   \
            else if (wm == kWFull) FN<1, kWFull>(__VA_ARGS__);              \
            else FN<1, kWBcast>(__VA_ARGS__);                               \
        }                                                                   \
    } while (0)

template <int P, int WM>
__device__ __forceinline__ void chunk_sum_into(const LossChunk& c, double& acc) { acc = chunk_sum<P, WM>(c); }

__global__ __launch_bounds__(kLossBlock) void loss_partial_kernel(const DvcLossTerm* __restrict__ terms, int n_terms,
                                                                  const DvcLossChunk* __restrict__ chunks, long n_chunks,
                                                                  double* __restrict__ partials) {
    __shared__ double red[kLossBlock / 64];
    for (long ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        LossChunk c;
        int p, wm, ti;
        double acc = 0.0;
        if (make_chunk(terms, n_terms, chunks, ci, false, c, p, wm, ti)) LOSS_DISPATCH(chunk_sum_into, c, acc);
        const double s = block_sum<double, kLossBlock>(acc, red);       // (block-uniform control flow up to here)
        if (threadIdx.x == 0) partials[ci] = s;
    }
}

// Stage 2, ONE workgroup: per term, thread j adds the term's partials j, j + 256, ... and block_sum combines them;
// values[k] = (float)(S_k * scale_k / n_k), and the same doubles, added in term order, give values[n_terms].  Term k's partials
// are the ceil(n_k / DVC_LOSS_CHUNK) that follow those of the terms before it (dvc_loss_fwd has checked that n_chunks is their sum).
__global__ __launch_bounds__(kLossBlock) void loss_finish_kernel(const DvcLossTerm* __restrict__ terms, int n_terms,
                                                                 const double* __restrict__ partials, long n_chunks,
                                                                 float* __restrict__ values) {
    __shared__ double red[kLossBlock / 64];
    double total = 0.0;
    long first = 0;
    for (int k = 0; k < n_terms; ++k) {
        const long n = terms[k].n;
        long count = (n + DVC_LOSS_CHUNK - 1) / DVC_LOSS_CHUNK;
        if (count > n_chunks - first) count = n_chunks - first;
        double acc = 0.0;
        for (long j = threadIdx.x; j < count; j += kLossBlock) acc += partials[first + j];
        const double S = block_sum<double, kLossBlock>(acc, red);
        const double v = S * (double)terms[k].scale / (double)n;
        total = k == 0 ? v : total + v;     // (not 0.0 + v: the total of a one-row table has the bits of values[0], a -0 included)
        if (threadIdx.x == 0) values[k] = (float)v;
        first += count;
    }
    if (threadIdx.x == 0) values[n_terms] = (float)total;
}

__global__ __launch_bounds__(kLossBlock) void loss_bwd_kernel(const DvcLossTerm* __restrict__ terms, int n_terms,
                                                              const DvcLossChunk* __restrict__ chunks, long n_chunks,
                                                              const float* __restrict__ grad_total, const float* __restrict__ grad_values) {
    for (long ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        LossChunk c;
        int p, wm, ti;
        if (!make_chunk(terms, n_terms, chunks, ci, true, c, p, wm, ti)) continue;
        if (!c.dx && !c.dt) continue;
        const double up = (double)grad_total[0] + (grad_values ? (double)grad_values[ti] : 0.0);
        const float coef = (float)(up * (double)terms[ti].scale / (double)terms[ti].n);
        LOSS_DISPATCH(chunk_grad, c, coef);
    }
}

// Everything that can be refused is refused here, from the HOST copy of the term table, before anything is launched.
int loss_validate(const char* fn, const DvcLossTerm* terms, const DvcLossTerm* terms_host, int32_t n_terms, const DvcLossChunk* chunks,
                  int64_t n_chunks) {
    DVC_REQUIRE(n_terms >= 0 && n_chunks >= 0, "%s: negative count (%d terms, %ld chunks)", fn, n_terms, (long)n_chunks);
    if (n_terms == 0) return 0;
    DVC_REQUIRE(terms && terms_host && chunks, "%s: null table", fn);
    DVC_REQUIRE(n_chunks >= 1, "%s: no chunks for %d terms", fn, n_terms);
    int64_t want = 0;
    for (int32_t k = 0; k < n_terms; ++k) {
        const DvcLossTerm& t = terms_host[k];
        DVC_REQUIRE(t.p == 1 || t.p == 2, "%s: term %d: p = %d is neither 1 nor 2", fn, k, t.p);
        DVC_REQUIRE(t.n > 0, "%s: term %d: n = %ld is not positive", fn, k, (long)t.n);
        DVC_REQUIRE(t.x, "%s: term %d: null x", fn, k);
        DVC_REQUIRE(t.plane > 0, "%s: term %d: plane = %ld is not positive", fn, k, (long)t.plane);
        DVC_REQUIRE(t.cpl >= 0 && t.cpl % t.plane == 0, "%s: term %d: cpl = %ld is not a multiple of plane = %ld", fn, k, (long)t.cpl,
                    (long)t.plane);
        DVC_REQUIRE(t.cpl == 0 || t.n % t.cpl == 0, "%s: term %d: n = %ld is not a multiple of cpl = %ld", fn, k, (long)t.n, (long)t.cpl);
        want += (t.n + DVC_LOSS_CHUNK - 1) / DVC_LOSS_CHUNK;
    }
    DVC_REQUIRE(n_chunks == want, "%s: %ld chunks for terms that cut into %ld", fn, (long)n_chunks, (long)want);
    return 0;
}

}  // namespace

extern "C" int dvc_loss_fwd(const DvcLossTerm* terms, const DvcLossTerm* terms_host, int32_t n_terms, const DvcLossChunk* chunks,
                            int64_t n_chunks, double* partials, float* values, dvcStream stream) {
    const char* fn = "dvc_loss_fwd";
    if (int rc = loss_validate(fn, terms, terms_host, n_terms, chunks, n_chunks)) return rc;
    if (n_terms == 0) return 0;
    DVC_REQUIRE(partials && values, "%s: null partials / values", fn);
    const unsigned grid = (unsigned)(n_chunks < kLossMaxBlocks ? n_chunks : kLossMaxBlocks);
    hipLaunchKernelGGL(loss_partial_kernel, dim3(grid), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms, chunks,
                       (long)n_chunks, partials);
    DVC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms,
                       (const double*)partials, (long)n_chunks, values);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_loss_bwd(const DvcLossTerm* terms, const DvcLossTerm* terms_host, int32_t n_terms, const DvcLossChunk* chunks,
                            int64_t n_chunks, const float* grad_total, const float* grad_values, dvcStream stream) {
    const char* fn = "dvc_loss_bwd";
    if (int rc = loss_validate(fn, terms, terms_host, n_terms, chunks, n_chunks)) return rc;
    if (n_terms == 0) return 0;
    DVC_REQUIRE(grad_total, "%s: null grad_total", fn);
    const unsigned grid = (unsigned)(n_chunks < kLossMaxBlocks ? n_chunks : kLossMaxBlocks);
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(grid), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms, chunks,
                       (long)n_chunks, grad_total, grad_values);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}
