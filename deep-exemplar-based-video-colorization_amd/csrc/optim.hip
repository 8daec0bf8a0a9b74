// Adam over every parameter tensor of a step in one launch (dvc_adam_step; the contract is in include/dvc_hip.h, the driver is
// dvc_amd/optim.py, the design and the measured rates are in DESIGN.md §6d).
//
// Pure streaming: 28 B per element (36 with amsgrad) and ~12 fp32 operations, so the kernel is a chunk walker around 16-byte loads
// and stores.  256 threads x 4 floats = 1,024 elements per pass, DVC_ADAM_CHUNK = 4 passes; the grid is min(chunks, 256 CUs x 8
// workgroups) and strides over the chunk table, so the tensor sizes do not shape the load.  The two descriptors of a chunk are
// wave-uniform and arrive by scalar loads.  No LDS, no atomics, 62 VGPRs: 8 workgroups per CU are resident.
//
// The arithmetic is spelled with explicit fmaf and the file is compiled with contraction off, so the roundings are the ones
// written here whatever the compiler's default: tests/adam_reference.py counts them.
//
// dvc_adam_advance (below the step kernel) is the capturable variant's second launch: it keeps the step counts and the two
// bias-correction columns of the tensor table on the device, so that dvc_adam_step, unchanged, can be replayed from a graph.
//
// The gradient guard (bottom of the file: dvc_grad_norm, dvc_adam_advance_guarded, dvc_adam_step_guarded, dvc_grad_scale) lets a
// replayed step look at its gradients.  dvc_grad_norm reduces sum g^2 over the SAME two tables in the two stages and the fixed
// order of csrc/loss.hip (thread j of a chunk owns elements 4 (j + 256 r) + k whichever path loaded them, squares exact in double,
// block_sum<double, 256>, one partial per chunk that depends on the chunk's data alone; stage 2 is one workgroup) and leaves a
// 24-byte DvcGradGuard record on the device: the norm, clip_grad_norm_'s coefficient, a non-finite flag and a running count of
// skipped steps, written by thread 0 with ordinary stores.  The guarded advance and step are the kernels above with that record in
// front of them: flag set -> return before any load or store (the flag comes by a scalar load, so the branch is wave-uniform);
// otherwise g' = clip_coef * g, one fp32 multiply that is exact for 1.0f, takes g's place.  adam_element / adam_chunk carry a third
// template parameter for it; the instantiations without it are the ones the unguarded kernel always had.
// Finite gradients whose norm is past the fp32 range report total_norm = inf with found_inf = 0: the flag and the coefficient come
// from the double.
// Resources (hipcc --save-temps, gfx950): adam_step_kernel 62 VGPRs, adam_step_guarded_kernel 62, grad_norm_partial_kernel 28,
// grad_norm_finish_kernel 16, grad_scale_kernel 28, the two advance kernels 40; no scratch anywhere; LDS: 32 B in each of the
// two norm kernels (block_sum's four doubles), none elsewhere.
#include "common.h"
#include "reduce.h"

#include <cstdint>

#pragma clang fp contract(off)

static_assert(sizeof(DvcAdamTensor) == 80 && sizeof(DvcAdamChunk) == 16, "table layouts are part of the ABI (dvc_amd/_lib.py)");
static_assert(sizeof(DvcAdamAdvance) == 40, "table layouts are part of the ABI (dvc_amd/_lib.py)");
static_assert(sizeof(DvcGradGuard) == 24, "table layouts are part of the ABI (dvc_amd/_lib.py)");

namespace {

constexpr int kAdamBlock = 256;
constexpr int kAdamMaxBlocks = 256 * 8;
static_assert(DVC_ADAM_CHUNK % (4 * kAdamBlock) == 0, "a chunk is a whole number of 16-byte passes");

struct AdamScalars {
    float step_size, inv_sqrt_bc2, beta2, omb1, omb2, eps, wd;
};

// kClip (the guarded step): clip * g takes g's place, one rounding; without it `clip` is not read.
template <bool kWd, bool kAms, bool kClip>
__device__ __forceinline__ void adam_element(const AdamScalars& s, float clip, float& p, float g, float& m, float& v, float& vmax) {
    if (kClip) g = clip * g;
    if (kWd) g = fmaf(s.wd, p, g);
    m = fmaf(s.omb1, g - m, m);
    v = fmaf(s.omb2, g * g, s.beta2 * v);
    float vv = v;
    if (kAms) vv = vmax = (v > vmax || v != v) ? v : vmax;      // torch.maximum: a NaN on either side stays (fmaxf would drop it)
    const float denom = fmaf(sqrtf(vv), s.inv_sqrt_bc2, s.eps);
    p = fmaf(-s.step_size, m / denom, p);
}

// The pointers come out of a table in memory, so the compiler knows no address space for them and would emit flat_load / flat_store
// (which test every address against the LDS and scratch apertures); they are device memory by contract.
#define AS1 __attribute__((address_space(1)))
typedef AS1 float gfloat;
typedef float vfloat4 __attribute__((ext_vector_type(4)));
typedef AS1 vfloat4 gfloat4;

template <bool kWd, bool kAms, bool kClip>
__device__ __forceinline__ void adam_lane(const AdamScalars& s, float clip, vfloat4& P, const vfloat4& G, vfloat4& M, vfloat4& V, vfloat4& X,
                                          int k) {
    float p = P[k], m = M[k], v = V[k], x = X[k];
    adam_element<kWd, kAms, kClip>(s, clip, p, G[k], m, v, x);
    P[k] = p, M[k] = m, V[k] = v, X[k] = x;
}

template <bool kWd, bool kAms, bool kClip>
__device__ __forceinline__ void adam_chunk(const AdamScalars& s, float clip, float* p_, const float* g_, float* m_, float* v_, float* vmax_,
                                           int len) {
    gfloat* __restrict__ p = (gfloat*)p_;
    const gfloat* __restrict__ g = (const gfloat*)g_;
    gfloat* __restrict__ m = (gfloat*)m_;
    gfloat* __restrict__ v = (gfloat*)v_;
    gfloat* __restrict__ vmax = (gfloat*)vmax_;
    uintptr_t bits = (uintptr_t)p_ | (uintptr_t)g_ | (uintptr_t)m_ | (uintptr_t)v_;
    if (kAms) bits |= (uintptr_t)vmax_;
    const int nvec = (bits & 15) == 0 ? len >> 2 : 0;          // 16-byte groups that lie wholly inside [0, len)
    for (int i = threadIdx.x; i < nvec; i += kAdamBlock) {
        vfloat4 P = ((gfloat4*)p)[i];
        const vfloat4 G = ((const gfloat4*)g)[i];
        vfloat4 M = ((gfloat4*)m)[i];
        vfloat4 V = ((gfloat4*)v)[i];
        vfloat4 X = kAms ? (vfloat4)((gfloat4*)vmax)[i] : vfloat4{0.f, 0.f, 0.f, 0.f};
        adam_lane<kWd, kAms, kClip>(s, clip, P, G, M, V, X, 0);
        adam_lane<kWd, kAms, kClip>(s, clip, P, G, M, V, X, 1);
        adam_lane<kWd, kAms, kClip>(s, clip, P, G, M, V, X, 2);
        adam_lane<kWd, kAms, kClip>(s, clip, P, G, M, V, X, 3);
        ((gfloat4*)p)[i] = P;
        ((gfloat4*)m)[i] = M;
        ((gfloat4*)v)[i] = V;
        if (kAms) ((gfloat4*)vmax)[i] = X;
    }
#pragma unroll 1
    for (int i = nvec * 4 + threadIdx.x; i < len; i += kAdamBlock) {     // the tail, or all of a misaligned chunk
        float P = p[i], M = m[i], V = v[i], X = kAms ? (float)vmax[i] : 0.f;
        adam_element<kWd, kAms, kClip>(s, clip, P, g[i], M, V, X);
        p[i] = P;
        m[i] = M;
        v[i] = V;
        if (kAms) vmax[i] = X;
    }
}

// The chunk walk of both step kernels.
template <bool kClip>
__device__ __forceinline__ void adam_walk(const DvcAdamTensor* __restrict__ tensors, int n_tensors, const DvcAdamChunk* __restrict__ chunks,
                                          long n_chunks, float clip) {
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int ti = chunks[c].tensor;
        const long start = chunks[c].start;
        if (ti < 0 || ti >= n_tensors) continue;
        const DvcAdamTensor* t = tensors + ti;
        const long n = t->n;
        if (start < 0 || start >= n) continue;
        const long rest = n - start;
        const int len = rest < DVC_ADAM_CHUNK ? (int)rest : DVC_ADAM_CHUNK;
        const AdamScalars s = {t->step_size, t->inv_sqrt_bc2, t->beta2, t->one_minus_beta1, t->one_minus_beta2, t->eps, t->weight_decay};
        float* p = t->p + start;
        const float* g = t->g + start;
        float* m = t->m + start;
        float* v = t->v + start;
        float* vmax = t->vmax ? t->vmax + start : nullptr;
        if (vmax) {
            if (s.wd != 0.f) adam_chunk<true, true, kClip>(s, clip, p, g, m, v, vmax, len);
            else adam_chunk<false, true, kClip>(s, clip, p, g, m, v, vmax, len);
        } else {
            if (s.wd != 0.f) adam_chunk<true, false, kClip>(s, clip, p, g, m, v, vmax, len);
            else adam_chunk<false, false, kClip>(s, clip, p, g, m, v, vmax, len);
        }
    }
}

__global__ __launch_bounds__(kAdamBlock) void adam_step_kernel(const DvcAdamTensor* __restrict__ tensors, int n_tensors,
                                                               const DvcAdamChunk* __restrict__ chunks, long n_chunks) {
    adam_walk<false>(tensors, n_tensors, chunks, n_chunks, 1.f);
}

// The guarded step: nothing is loaded or stored when the guard's flag is set (a kernel-argument pointer read without a lane index:
// a scalar load, the same in every wave).  .grad is only read.
__global__ __launch_bounds__(kAdamBlock) void adam_step_guarded_kernel(const DvcAdamTensor* __restrict__ tensors, int n_tensors,
                                                                       const DvcAdamChunk* __restrict__ chunks, long n_chunks,
                                                                       const DvcGradGuard* __restrict__ guard) {
    if (guard->found_inf != 0) return;
    adam_walk<true>(tensors, n_tensors, chunks, n_chunks, guard->clip_coef);
}

// The device-side half of a capturable step: one thread per tensor advances that tensor's step count and rewrites the two
// columns of its record that depend on it, in double as optim.adam_scalars does on the host.  Everything else in the record is
// the caller's.  A few dozen threads of work; what it buys is that nothing per step comes from the host.
constexpr int kAdvanceBlock = 64;

__device__ __forceinline__ void adam_advance_one(const DvcAdamAdvance* __restrict__ advance, DvcAdamTensor* __restrict__ tensors, int i) {
    const DvcAdamAdvance a = advance[i];
    const float t = *a.step + 1.0f;
    *a.step = t;
    const double lr = a.lr_tensor ? (double)*a.lr_tensor : a.lr;
    const double bc1 = 1.0 - pow(a.beta1, (double)t);
    const double bc2 = 1.0 - pow(a.beta2, (double)t);
    tensors[i].step_size = (float)(lr / bc1);
    tensors[i].inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
}

__global__ __launch_bounds__(kAdvanceBlock) void adam_advance_kernel(const DvcAdamAdvance* __restrict__ advance,
                                                                     DvcAdamTensor* __restrict__ tensors, int n_tensors) {
    const int i = blockIdx.x * kAdvanceBlock + threadIdx.x;
    if (i >= n_tensors) return;
    adam_advance_one(advance, tensors, i);
}

// The guarded advance: a skipped step keeps its count, and the two columns keep the values of the last step that ran.
__global__ __launch_bounds__(kAdvanceBlock) void adam_advance_guarded_kernel(const DvcAdamAdvance* __restrict__ advance,
                                                                             DvcAdamTensor* __restrict__ tensors, int n_tensors,
                                                                             const DvcGradGuard* __restrict__ guard) {
    if (guard->found_inf != 0) return;
    const int i = blockIdx.x * kAdvanceBlock + threadIdx.x;
    if (i >= n_tensors) return;
    adam_advance_one(advance, tensors, i);
}

// ---- the gradient guard
constexpr int kNormPasses = DVC_ADAM_CHUNK / (4 * kAdamBlock);

// Stage 1: partials[chunk] = sum over the chunk of (double)g * (double)g.  Only g and n of a tensor record are read.  Thread j adds
// its elements 4 (j + 256 r) + k in the order r, k; a group of four moves as one 16-byte load when the chunk's first element is
// 16-byte aligned and the group lies wholly inside the chunk, element by element otherwise — the same values in the same order.
__global__ __launch_bounds__(kAdamBlock) void grad_norm_partial_kernel(const DvcAdamTensor* __restrict__ tensors, int n_tensors,
                                                                       const DvcAdamChunk* __restrict__ chunks, long n_chunks,
                                                                       double* __restrict__ partials) {
    __shared__ double red[kAdamBlock / 64];
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        double acc = 0.0;
        const int ti = chunks[c].tensor;
        const long start = chunks[c].start;
        if (ti >= 0 && ti < n_tensors) {
            const long n = tensors[ti].n;
            if (start >= 0 && start < n) {
                const long rest = n - start;
                const int len = rest < DVC_ADAM_CHUNK ? (int)rest : DVC_ADAM_CHUNK;
                const float* g_ = tensors[ti].g + start;
                const gfloat* __restrict__ g = (const gfloat*)g_;
                const bool vec = ((uintptr_t)g_ & 15) == 0;
#pragma unroll 1
                for (int r = 0; r < kNormPasses; ++r) {
                    const int base = 4 * ((int)threadIdx.x + kAdamBlock * r);
                    if (base >= len) break;
                    const int cnt = len - base < 4 ? len - base : 4;
                    vfloat4 G = {0.f, 0.f, 0.f, 0.f};
                    if (vec && cnt == 4) {
                        G = *(const gfloat4*)(g + base);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < cnt) G[k] = g[base + k];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < cnt) acc += (double)G[k] * (double)G[k];
                }
            }
        }
        const double s = block_sum<double, kAdamBlock>(acc, red);       // (block-uniform control flow up to here)
        if (threadIdx.x == 0) partials[c] = s;
    }
}

// Stage 2, ONE workgroup: thread j adds partials j, j + 256, ...; block_sum gives S; thread 0 writes the record.
__global__ __launch_bounds__(kAdamBlock) void grad_norm_finish_kernel(const double* __restrict__ partials, long n_chunks, double max_norm,
                                                                      unsigned flags, DvcGradGuard* __restrict__ guard) {
    __shared__ double red[kAdamBlock / 64];
    double acc = 0.0;
    for (long j = threadIdx.x; j < n_chunks; j += kAdamBlock) acc += partials[j];
    const double S = block_sum<double, kAdamBlock>(acc, red);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(S);
    const bool nonfinite = !(S - S == 0.0);         // S is NaN or +inf (a sum of squares is never -inf)
    const int found = nonfinite && !(flags & DVC_GRAD_NORM_KEEP_NONFINITE) ? 1 : 0;
    double coef = 1.0;
    if (!nonfinite) {
        coef = max_norm / (norm + 1e-6);
        if (!(coef < 1.0)) coef = 1.0;
    }
    guard->total_norm = (float)norm;
    guard->clip_coef = (float)coef;
    guard->found_inf = found;
    guard->skipped += found;
    guard->sumsq = S;
}

// g *= coef in place over the tables.  coef is the record's clip_coef; with the flag set it is the one
// torch.nn.utils.clip_grad_norm_ multiplies by on such gradients: NaN for a NaN norm, 0 for an infinite one.  1.0f writes nothing.
__global__ __launch_bounds__(kAdamBlock) void grad_scale_kernel(const DvcAdamTensor* __restrict__ tensors, int n_tensors,
                                                                const DvcAdamChunk* __restrict__ chunks, long n_chunks,
                                                                const DvcGradGuard* __restrict__ guard) {
    float coef = guard->clip_coef;
    if (guard->found_inf != 0) {
        const double S = guard->sumsq;
        coef = S != S ? __builtin_nanf("") : 0.f;
    }
    if (coef == 1.0f) return;
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int ti = chunks[c].tensor;
        const long start = chunks[c].start;
        if (ti < 0 || ti >= n_tensors) continue;
        const long n = tensors[ti].n;
        if (start < 0 || start >= n) continue;
        const long rest = n - start;
        const int len = rest < DVC_ADAM_CHUNK ? (int)rest : DVC_ADAM_CHUNK;
        float* g_ = const_cast<float*>(tensors[ti].g) + start;
        gfloat* __restrict__ g = (gfloat*)g_;
        const int nvec = ((uintptr_t)g_ & 15) == 0 ? len >> 2 : 0;      // 16-byte groups that lie wholly inside [0, len)
        for (int i = threadIdx.x; i < nvec; i += kAdamBlock) {
            vfloat4 G = ((gfloat4*)g)[i];
            G[0] = coef * G[0], G[1] = coef * G[1], G[2] = coef * G[2], G[3] = coef * G[3];
            ((gfloat4*)g)[i] = G;
        }
#pragma unroll 1
        for (int i = nvec * 4 + threadIdx.x; i < len; i += kAdamBlock) g[i] = coef * g[i];
    }
}

// What the four guard entry points refuse, from their arguments alone, before anything is launched.
int guard_validate(const char* fn, const void* tensors, int32_t n_tensors, const void* chunks, int64_t n_chunks, const void* guard) {
    DVC_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "%s: negative count (%d tensors, %ld chunks)", fn, n_tensors, (long)n_chunks);
    if (n_tensors == 0) return 0;
    DVC_REQUIRE(tensors && chunks, "%s: null table", fn);
    DVC_REQUIRE(guard, "%s: null guard", fn);
    DVC_REQUIRE(n_chunks >= 1, "%s: no chunks for %d tensors", fn, n_tensors);
    return 0;
}

}  // namespace

extern "C" int dvc_adam_advance(const DvcAdamAdvance* advance, DvcAdamTensor* tensors, int32_t n_tensors, dvcStream stream) {
    const char* fn = "dvc_adam_advance";
    DVC_REQUIRE(n_tensors >= 0, "%s: negative count (%d tensors)", fn, n_tensors);
    if (n_tensors == 0) return 0;
    DVC_REQUIRE(advance && tensors, "%s: null table", fn);
    hipLaunchKernelGGL(adam_advance_kernel, dim3((unsigned)cdiv(n_tensors, kAdvanceBlock)), dim3(kAdvanceBlock), 0,
                       (hipStream_t)stream, advance, tensors, (int)n_tensors);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_adam_step(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks,
                             dvcStream stream) {
    const char* fn = "dvc_adam_step";
    DVC_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "%s: negative count (%d tensors, %ld chunks)", fn, n_tensors, (long)n_chunks);
    if (n_tensors == 0) return 0;
    DVC_REQUIRE(tensors && chunks, "%s: null table", fn);
    DVC_REQUIRE(n_chunks >= 1, "%s: no chunks for %d tensors", fn, n_tensors);
    const unsigned grid = (unsigned)(n_chunks < kAdamMaxBlocks ? n_chunks : kAdamMaxBlocks);
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(kAdamBlock), 0, (hipStream_t)stream, tensors, (int)n_tensors, chunks,
                       (long)n_chunks);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_grad_norm(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks,
                             double* partials, double max_norm, uint32_t flags, DvcGradGuard* guard, dvcStream stream) {
    const char* fn = "dvc_grad_norm";
    DVC_REQUIRE(max_norm > 0.0, "%s: max_norm = %g is not a positive number (+inf: no clipping)", fn, max_norm);     // (a NaN fails it too)
    DVC_REQUIRE((flags & ~(uint32_t)DVC_GRAD_NORM_KEEP_NONFINITE) == 0, "%s: unknown flags 0x%x", fn, flags);
    if (int rc = guard_validate(fn, tensors, n_tensors, chunks, n_chunks, guard)) return rc;
    if (n_tensors == 0) return 0;
    DVC_REQUIRE(partials, "%s: null partials", fn);
    const unsigned grid = (unsigned)(n_chunks < kAdamMaxBlocks ? n_chunks : kAdamMaxBlocks);
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(grid), dim3(kAdamBlock), 0, (hipStream_t)stream, tensors, (int)n_tensors, chunks,
                       (long)n_chunks, partials);
    DVC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kAdamBlock), 0, (hipStream_t)stream, (const double*)partials, (long)n_chunks,
                       max_norm, (unsigned)flags, guard);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_adam_advance_guarded(const DvcAdamAdvance* advance, DvcAdamTensor* tensors, int32_t n_tensors, const DvcGradGuard* guard,
                                        dvcStream stream) {
    const char* fn = "dvc_adam_advance_guarded";
    DVC_REQUIRE(n_tensors >= 0, "%s: negative count (%d tensors)", fn, n_tensors);
    if (n_tensors == 0) return 0;
    DVC_REQUIRE(advance && tensors, "%s: null table", fn);
    DVC_REQUIRE(guard, "%s: null guard", fn);
    hipLaunchKernelGGL(adam_advance_guarded_kernel, dim3((unsigned)cdiv(n_tensors, kAdvanceBlock)), dim3(kAdvanceBlock), 0,
                       (hipStream_t)stream, advance, tensors, (int)n_tensors, guard);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_adam_step_guarded(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks,
                                     const DvcGradGuard* guard, dvcStream stream) {
    const char* fn = "dvc_adam_step_guarded";
    if (int rc = guard_validate(fn, tensors, n_tensors, chunks, n_chunks, guard)) return rc;
    if (n_tensors == 0) return 0;
    const unsigned grid = (unsigned)(n_chunks < kAdamMaxBlocks ? n_chunks : kAdamMaxBlocks);
    hipLaunchKernelGGL(adam_step_guarded_kernel, dim3(grid), dim3(kAdamBlock), 0, (hipStream_t)stream, tensors, (int)n_tensors, chunks,
                       (long)n_chunks, guard);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_grad_scale(const DvcAdamTensor* tensors, int32_t n_tensors, const DvcAdamChunk* chunks, int64_t n_chunks,
                              const DvcGradGuard* guard, dvcStream stream) {
    const char* fn = "dvc_grad_scale";
    if (int rc = guard_validate(fn, tensors, n_tensors, chunks, n_chunks, guard)) return rc;
    if (n_tensors == 0) return 0;
    const unsigned grid = (unsigned)(n_chunks < kAdamMaxBlocks ? n_chunks : kAdamMaxBlocks);
    hipLaunchKernelGGL(grad_scale_kernel, dim3(grid), dim3(kAdamBlock), 0, (hipStream_t)stream, tensors, (int)n_tensors, chunks,
                       (long)n_chunks, guard);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}
