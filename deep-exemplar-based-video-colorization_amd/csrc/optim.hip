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
#include "common.h"

#include <cstdint>

#pragma clang fp contract(off)

static_assert(sizeof(DvcAdamTensor) == 80 && sizeof(DvcAdamChunk) == 16, "table layouts are part of the ABI (dvc_amd/_lib.py)");
static_assert(sizeof(DvcAdamAdvance) == 40, "table layouts are part of the ABI (dvc_amd/_lib.py)");

namespace {

constexpr int kAdamBlock = 256;
constexpr int kAdamMaxBlocks = 256 * 8;
static_assert(DVC_ADAM_CHUNK % (4 * kAdamBlock) == 0, "a chunk is a whole number of 16-byte passes");

struct AdamScalars {
    float step_size, inv_sqrt_bc2, beta2, omb1, omb2, eps, wd;
};

template <bool kWd, bool kAms>
__device__ __forceinline__ void adam_element(const AdamScalars& s, float& p, float g, float& m, float& v, float& vmax) {
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

template <bool kWd, bool kAms>
__device__ __forceinline__ void adam_lane(const AdamScalars& s, vfloat4& P, const vfloat4& G, vfloat4& M, vfloat4& V, vfloat4& X, int k) {
    float p = P[k], m = M[k], v = V[k], x = X[k];
    adam_element<kWd, kAms>(s, p, G[k], m, v, x);
    P[k] = p, M[k] = m, V[k] = v, X[k] = x;
}

template <bool kWd, bool kAms>
__device__ __forceinline__ void adam_chunk(const AdamScalars& s, float* p_, const float* g_, float* m_, float* v_, float* vmax_, int len) {
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
        adam_lane<kWd, kAms>(s, P, G, M, V, X, 0);
        adam_lane<kWd, kAms>(s, P, G, M, V, X, 1);
        adam_lane<kWd, kAms>(s, P, G, M, V, X, 2);
        adam_lane<kWd, kAms>(s, P, G, M, V, X, 3);
        ((gfloat4*)p)[i] = P;
        ((gfloat4*)m)[i] = M;
        ((gfloat4*)v)[i] = V;
        if (kAms) ((gfloat4*)vmax)[i] = X;
    }
#pragma unroll 1
    for (int i = nvec * 4 + threadIdx.x; i < len; i += kAdamBlock) {     // the tail, or all of a misaligned chunk
        float P = p[i], M = m[i], V = v[i], X = kAms ? (float)vmax[i] : 0.f;
        adam_element<kWd, kAms>(s, P, g[i], M, V, X);
        p[i] = P;
        m[i] = M;
        v[i] = V;
        if (kAms) vmax[i] = X;
    }
}

__global__ __launch_bounds__(kAdamBlock) void adam_step_kernel(const DvcAdamTensor* __restrict__ tensors, int n_tensors,
                                                               const DvcAdamChunk* __restrict__ chunks, long n_chunks) {
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
            if (s.wd != 0.f) adam_chunk<true, true>(s, p, g, m, v, vmax, len);
            else adam_chunk<false, true>(s, p, g, m, v, vmax, len);
        } else {
            if (s.wd != 0.f) adam_chunk<true, false>(s, p, g, m, v, vmax, len);
            else adam_chunk<false, false>(s, p, g, m, v, vmax, len);
        }
    }
}

// The device-side half of a capturable step: one thread per tensor advances that tensor's step count and rewrites the two
// columns of its record that depend on it, in double as optim.adam_scalars does on the host.  Everything else in the record is
// the caller's.  A few dozen threads of work; what it buys is that nothing per step comes from the host.
constexpr int kAdvanceBlock = 64;

__global__ __launch_bounds__(kAdvanceBlock) void adam_advance_kernel(const DvcAdamAdvance* __restrict__ advance,
                                                                     DvcAdamTensor* __restrict__ tensors, int n_tensors) {
    const int i = blockIdx.x * kAdvanceBlock + threadIdx.x;
    if (i >= n_tensors) return;
    const DvcAdamAdvance a = advance[i];
    const float t = *a.step + 1.0f;
    *a.step = t;
    const double lr = a.lr_tensor ? (double)*a.lr_tensor : a.lr;
    const double bc1 = 1.0 - pow(a.beta1, (double)t);
    const double bc2 = 1.0 - pow(a.beta2, (double)t);
    tensors[i].step_size = (float)(lr / bc1);
    tensors[i].inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
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
