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

static_assert(sizeof(DvcLossTerm) == 80 && sizeof(DvcLossChunk) == 16, "table layouts are part of the ABI (dvc_amd/_lib.py)");

namespace {

constexpr int kLossBlock = 256;
constexpr int kLossMaxBlocks = 256 * 8;
constexpr int kLossPasses = DVC_LOSS_CHUNK / (4 * kLossBlock);
static_assert(DVC_LOSS_CHUNK % (4 * kLossBlock) == 0, "a chunk is a whole number of 16-byte passes");

enum { kWNone = 0, kWFull = 1, kWBcast = 2 };

// The pointers come out of a table in memory; they are device memory by contract (see csrc/optim.hip).
#define AS1 __attribute__((address_space(1)))
typedef AS1 float gfloat;
typedef float vfloat4 __attribute__((ext_vector_type(4)));
typedef AS1 vfloat4 gfloat4;

// One chunk of one term: the pointers already advanced to the chunk's first element (w only when it has x's shape).
struct LossChunk {
    const gfloat* x;
    const gfloat* t;    // null: t_scalar
    const gfloat* w;    // kWFull: at the chunk; kWBcast: the mask's base
    gfloat* dx;         // backward only, either may be null
    gfloat* dt;
    float t_scalar;
    int len;            // elements of the chunk, 1 .. DVC_LOSS_CHUNK
    bool vec, wvec;     // 16-byte path for x / t / dx / dt, and for w
    long start, cpl, plane;     // kWBcast: the chunk's first element in the term, C * plane, plane
    bool narrow;        // every index of the term fits 32 bits
};

// index into a [B,1,H,W] mask of element i of x [B,C,H,W]: (i / cpl) * plane + i % plane  (plane divides cpl)
__device__ __forceinline__ long bcast_index(const LossChunk& c, int local) {
    if (c.narrow) {
        const unsigned i = (unsigned)c.start + (unsigned)local;
        return (long)(i / (unsigned)c.cpl) * c.plane + (long)(i % (unsigned)c.plane);
    }
    const long i = c.start + local;
    return (i / c.cpl) * c.plane + i % c.plane;
}

// Loads group g (elements 4 g .. 4 g + cnt - 1) of the chunk: d = x - t and, with a weight, w.  Lanes past cnt hold zeros.
template <int WM>
__device__ __forceinline__ void load_group(const LossChunk& c, int base, int cnt, vfloat4& D, vfloat4& W) {
    vfloat4 X = {0.f, 0.f, 0.f, 0.f}, T = {c.t_scalar, c.t_scalar, c.t_scalar, c.t_scalar};
    W = vfloat4{0.f, 0.f, 0.f, 0.f};
    if (c.vec && cnt == 4) {
        X = *(const gfloat4*)(c.x + base);
        if (c.t) T = *(const gfloat4*)(c.t + base);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) {
                X[k] = c.x[base + k];
                if (c.t) T[k] = c.t[base + k];
            }
    }
    if (WM == kWFull) {
        if (c.wvec && cnt == 4) {
            W = *(const gfloat4*)(c.w + base);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) W[k] = c.w[base + k];
        }
    } else if (WM == kWBcast) {
        if (c.wvec && cnt == 4) {       // plane % 4 == 0: the four elements share a plane row and the group is 16-byte aligned
            W = *(const gfloat4*)(c.w + bcast_index(c, base));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) W[k] = c.w[bcast_index(c, base + k)];
        }
    }
    D = X - T;
}

// ---- forward, stage 1
template <int P, int WM>
__device__ __forceinline__ double chunk_sum(const LossChunk& c) {
    double acc = 0.0;
#pragma unroll 1
    for (int r = 0; r < kLossPasses; ++r) {
        const int base = 4 * ((int)threadIdx.x + kLossBlock * r);
        if (base >= c.len) break;
        const int cnt = c.len - base < 4 ? c.len - base : 4;
        vfloat4 D, W;
        load_group<WM>(c, base, cnt, D, W);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) {
                const float d = D[k];
                const float e = P == 2 ? d * d : fabsf(d);
                const float v = WM == kWNone ? e : W[k] * e;       // (a NaN under a zero weight stays a NaN, as in torch)
                acc += (double)v;
            }
    }
    return acc;
}

// ---- backward
template <int P, int WM>
__device__ __forceinline__ void chunk_grad(const LossChunk& c, float coef) {
    const float c2 = P == 2 ? 2.f * coef : coef;        // exact
#pragma unroll 1
    for (int r = 0; r < kLossPasses; ++r) {
        const int base = 4 * ((int)threadIdx.x + kLossBlock * r);
        if (base >= c.len) break;
        const int cnt = c.len - base < 4 ? c.len - base : 4;
        vfloat4 D, W, G;
        load_group<WM>(c, base, cnt, D, W);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = D[k];
            const float cw = WM == kWNone ? c2 : c2 * W[k];
            const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : d);       // sgn(0) = 0, as torch.abs; a NaN stays
            G[k] = P == 2 ? cw * d : cw * s;
        }
        if (c.vec && cnt == 4) {
            if (c.dx) *(gfloat4*)(c.dx + base) = G;
            if (c.dt) *(gfloat4*)(c.dt + base) = -G;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) {
                    if (c.dx) c.dx[base + k] = G[k];
                    if (c.dt) c.dt[base + k] = -G[k];
                }
        }
    }
}

// The chunk's descriptor from the two tables; false for a chunk that names no element of any term (skipped).
__device__ __forceinline__ bool make_chunk(const DvcLossTerm* terms, int n_terms, const DvcLossChunk* chunks, long ci, bool backward,
                                           LossChunk& c, int& p, int& wm, int& ti) {
    ti = chunks[ci].term;
    const long start = chunks[ci].start;
    if (ti < 0 || ti >= n_terms) return false;
    const DvcLossTerm* t = terms + ti;
    const long n = t->n;
    if (start < 0 || start >= n) return false;
    const long rest = n - start;
    c.len = rest < DVC_LOSS_CHUNK ? (int)rest : DVC_LOSS_CHUNK;
    c.x = (const gfloat*)(t->x + start);
    c.t = t->t ? (const gfloat*)(t->t + start) : nullptr;
    c.t_scalar = t->t_scalar;
    c.dx = backward && t->dx ? (gfloat*)(t->dx + start) : nullptr;
    c.dt = backward && t->dt ? (gfloat*)(t->dt + start) : nullptr;
    c.start = start, c.cpl = t->cpl, c.plane = t->plane;
    c.narrow = n <= 0xffffffffL;
    uintptr_t bits = (uintptr_t)c.x | (uintptr_t)c.t | (uintptr_t)c.dx | (uintptr_t)c.dt;       // (a null pointer adds no bits)
    c.vec = (bits & 15) == 0;
    wm = !t->w ? kWNone : (t->cpl > 0 ? kWBcast : kWFull);
    c.w = wm == kWFull ? (const gfloat*)(t->w + start) : (const gfloat*)t->w;
    c.wvec = ((uintptr_t)c.w & 15) == 0 && (wm == kWFull || (t->plane & 3) == 0);
    p = t->p;
    return true;
}

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
