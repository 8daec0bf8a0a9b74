// Loss plans: the terms of csrc/loss.hip plus the signed mean and the relativistic GAN term, on tables that stay resident, so that a
// call whose tensors did not move is launches only and replays from a captured graph (dvc_loss_plan_check, dvc_loss_plan_fwd,
// dvc_loss_plan_bwd; the contract is in include/dvc_hip.h, the driver is dvc_amd.losses.Plan, the design, the error bounds and the
// measured rates are in DESIGN.md §6d).
//
// Kinds 1 and 2 run csrc/loss_chunk.h's chunk_sum / chunk_grad — the templates csrc/loss.hip instantiates — and stage 2 applies the
// same rule, so their bits are dvc_loss_fwd's.  Kind 3 is the same walk with e = d.  Kind 4, scale * mean(((x - mean(y)) - c)^2):
// stage 0 reduces y (thread ownership and CHAIN order as everywhere here) and leaves m = (float)(S_y / n_y) in the term's slot of
// the scratch; a chunk of x reads m back as a wave-uniform value, uses it as the scalar target of load_group, subtracts c and adds
// d*d and d into two doubles; stage 2 leaves sum d in the slot for the backward, which does not reduce again.
//
// Every launch is a straight line on the caller's stream.  No atomics, no counters, no inline assembly; contraction is off.
#include "common.h"
#include "reduce.h"

#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "loss_chunk.h"

static_assert(sizeof(DvcPlanTerm) == 112, "table layouts are part of the ABI (dvc_amd/_lib.py)");
static_assert(offsetof(DvcPlanTerm, n) == offsetof(DvcLossTerm, n) && offsetof(DvcPlanTerm, p) == offsetof(DvcLossTerm, p) &&
                  offsetof(DvcPlanTerm, kind) == offsetof(DvcLossTerm, reserved) &&
                  offsetof(DvcPlanTerm, scale) == offsetof(DvcLossTerm, scale) && offsetof(DvcPlanTerm, y) == sizeof(DvcLossTerm),
              "a DvcPlanTerm begins with a DvcLossTerm");

namespace {

// [partials | partials of sum d | partials of y | per slot {m, sum d}]
struct PlanScratch {
    double *part, *part_d, *part_y, *slots;
};
__host__ __device__ inline PlanScratch plan_scratch(double* s, long n_chunks, long n_ychunks) {
    return PlanScratch{s, s + n_chunks, s + 2 * n_chunks, s + 2 * n_chunks + n_ychunks};
}

// A chunk of a REL term's y; false for a chunk that names no element of any y (skipped).
__device__ __forceinline__ bool make_ychunk(const DvcPlanTerm* terms, int n_terms, const DvcLossChunk* ychunks, long ci, int& ti,
                                            long& start, int& len) {
    ti = ychunks[ci].term;
    start = ychunks[ci].start;
    if (ti < 0 || ti >= n_terms) return false;
    const DvcPlanTerm* t = terms + ti;
    if (t->kind != DVC_LOSS_KIND_REL || !t->y || t->slot < 0 || t->slot >= n_terms) return false;
    if (start < 0 || start >= t->n_y) return false;
    const long rest = t->n_y - start;
    len = rest < DVC_LOSS_CHUNK ? (int)rest : DVC_LOSS_CHUNK;
    return true;
}

// ---- stage 0a: the partial sums of y, one per y chunk
__global__ __launch_bounds__(kLossBlock) void plan_ysum_kernel(const DvcPlanTerm* __restrict__ terms, int n_terms,
                                                               const DvcLossChunk* __restrict__ ychunks, long n_ychunks,
                                                               double* __restrict__ part_y) {
    __shared__ double red[kLossBlock / 64];
    for (long ci = blockIdx.x; ci < n_ychunks; ci += gridDim.x) {
        int ti, len;
        long start;
        double acc = 0.0;
        if (make_ychunk(terms, n_terms, ychunks, ci, ti, start, len)) {
            const gfloat* y = (const gfloat*)(terms[ti].y + start);
            const bool vec = ((uintptr_t)y & 15) == 0;
#pragma unroll 1
            for (int r = 0; r < kLossPasses; ++r) {
                const int base = 4 * ((int)threadIdx.x + kLossBlock * r);
                if (base >= len) break;
                const int cnt = len - base < 4 ? len - base : 4;
                vfloat4 Y = {0.f, 0.f, 0.f, 0.f};
                if (vec && cnt == 4) {
                    Y = *(const gfloat4*)(y + base);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < cnt) Y[k] = y[base + k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) acc += (double)Y[k];
            }
        }
        const double s = block_sum<double, kLossBlock>(acc, red);       // (block-uniform control flow up to here)
        if (threadIdx.x == 0) part_y[ci] = s;
    }
}

// ---- stage 0b, ONE workgroup: per REL term, in term order, S_y from the term's y partials and m = (float)(S_y / n_y) into its slot
__global__ __launch_bounds__(kLossBlock) void plan_mean_kernel(const DvcPlanTerm* __restrict__ terms, int n_terms,
                                                               const double* __restrict__ part_y, long n_ychunks,
                                                               double* __restrict__ slots) {
    __shared__ double red[kLossBlock / 64];
    long first = 0;
    for (int k = 0; k < n_terms; ++k) {
        if (terms[k].kind != DVC_LOSS_KIND_REL) continue;
        const long n_y = terms[k].n_y;
        long count = (n_y + DVC_LOSS_CHUNK - 1) / DVC_LOSS_CHUNK;
        if (count > n_ychunks - first) count = n_ychunks - first;
        double acc = 0.0;
        for (long j = threadIdx.x; j < count; j += kLossBlock) acc += part_y[first + j];
        const double S = block_sum<double, kLossBlock>(acc, red);
        const int slot = terms[k].slot;
        if (threadIdx.x == 0 && slot >= 0 && slot < n_terms) slots[2 * slot] = (double)(float)(S / (double)n_y);
        first += count > 0 ? count : 0;
    }
}

// ---- the REL element code: d = (x - m) - c through load_group with m as the scalar target
__device__ __forceinline__ void rel_chunk_sum(const LossChunk& c, float cc, double& s2, double& s1) {
#pragma unroll 1
    for (int r = 0; r < kLossPasses; ++r) {
        const int base = 4 * ((int)threadIdx.x + kLossBlock * r);
        if (base >= c.len) break;
        const int cnt = c.len - base < 4 ? c.len - base : 4;
        vfloat4 D, W;
        load_group<kWNone>(c, base, cnt, D, W);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) {
                const float d = D[k] - cc;
                const float v = d * d;
                s2 += (double)v;
                s1 += (double)d;
            }
    }
}

__device__ __forceinline__ void rel_chunk_grad(const LossChunk& c, float cc, float coef) {
    const float c2 = 2.f * coef;        // exact
#pragma unroll 1
    for (int r = 0; r < kLossPasses; ++r) {
        const int base = 4 * ((int)threadIdx.x + kLossBlock * r);
        if (base >= c.len) break;
        const int cnt = c.len - base < 4 ? c.len - base : 4;
        vfloat4 D, W, G;
        load_group<kWNone>(c, base, cnt, D, W);
#pragma unroll
        for (int k = 0; k < 4; ++k) G[k] = c2 * (D[k] - cc);
        if (c.vec && cnt == 4) {
            *(gfloat4*)(c.dx + base) = G;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) c.dx[base + k] = G[k];
        }
    }
}

// m of a REL term as the scalar target of its chunk (t and w are null for REL: dvc_loss_plan_check)
__device__ __forceinline__ bool rel_target(const DvcPlanTerm& t, int n_terms, const double* slots, LossChunk& c) {
    if (t.slot < 0 || t.slot >= n_terms) return false;
    c.t = nullptr, c.dt = nullptr;
    c.t_scalar = (float)slots[2 * t.slot];      // (exact: stage 0b stored a float's value)
    return true;
}

#define PLAN_DISPATCH_WM(FN, P, ...)                                        \
    do {                                                                    \
        if (wm == kWNone) FN<P, kWNone>(__VA_ARGS__);                       \
        else if (wm == kWFull) FN<P, kWFull>(__VA_ARGS__);                  \
        else FN<P, kWBcast>(__VA_ARGS__);                                   \
    } while (0)

template <int P, int WM>
__device__ __forceinline__ void chunk_sum_into(const LossChunk& c, double& acc) { acc = chunk_sum<P, WM>(c); }

// ---- stage 1
__global__ __launch_bounds__(kLossBlock) void plan_partial_kernel(const DvcPlanTerm* __restrict__ terms, int n_terms,
                                                                  const DvcLossChunk* __restrict__ chunks, long n_chunks,
                                                                  double* __restrict__ part, double* __restrict__ part_d,
                                                                  const double* __restrict__ slots) {
    __shared__ double red[kLossBlock / 64];
    for (long ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        LossChunk c;
        int p, wm, ti, kind = 0;
        double acc = 0.0, acc_d = 0.0;
        if (make_chunk(terms, n_terms, chunks, ci, false, c, p, wm, ti)) {
            kind = terms[ti].kind;
            if (kind == DVC_LOSS_KIND_REL) {
                if (rel_target(terms[ti], n_terms, slots, c)) rel_chunk_sum(c, terms[ti].c, acc, acc_d);
            } else if (kind == DVC_LOSS_KIND_MEAN) {
                PLAN_DISPATCH_WM(chunk_sum_into, 0, c, acc);
            } else if (kind == DVC_LOSS_KIND_MSE) {
                PLAN_DISPATCH_WM(chunk_sum_into, 2, c, acc);
            } else if (kind == DVC_LOSS_KIND_L1) {
                PLAN_DISPATCH_WM(chunk_sum_into, 1, c, acc);
            }
        }
        const double s = block_sum<double, kLossBlock>(acc, red);       // (block-uniform control flow up to here: kind is the chunk's)
        if (threadIdx.x == 0) part[ci] = s;
        if (kind == DVC_LOSS_KIND_REL) {
            const double sd = block_sum<double, kLossBlock>(acc_d, red);
            if (threadIdx.x == 0) part_d[ci] = sd;
        }
    }
}

// ---- stage 2, ONE workgroup: csrc/loss.hip's loss_finish_kernel, and a REL term's sum d into its slot
__global__ __launch_bounds__(kLossBlock) void plan_finish_kernel(const DvcPlanTerm* __restrict__ terms, int n_terms,
                                                                 const double* __restrict__ part, const double* __restrict__ part_d,
                                                                 long n_chunks, double* __restrict__ slots, float* __restrict__ values) {
    __shared__ double red[kLossBlock / 64];
    double total = 0.0;
    long first = 0;
    for (int k = 0; k < n_terms; ++k) {
        const long n = terms[k].n;
        long count = (n + DVC_LOSS_CHUNK - 1) / DVC_LOSS_CHUNK;
        if (count > n_chunks - first) count = n_chunks - first;
        double acc = 0.0;
        for (long j = threadIdx.x; j < count; j += kLossBlock) acc += part[first + j];
        const double S = block_sum<double, kLossBlock>(acc, red);
        const double v = S * (double)terms[k].scale / (double)n;
        total = k == 0 ? v : total + v;     // (not 0.0 + v: the total of a one-row table has the bits of values[0], a -0 included)
        if (threadIdx.x == 0) values[k] = (float)v;
        if (terms[k].kind == DVC_LOSS_KIND_REL) {
            double acc_d = 0.0;
            for (long j = threadIdx.x; j < count; j += kLossBlock) acc_d += part_d[first + j];
            const double Sd = block_sum<double, kLossBlock>(acc_d, red);
            const int slot = terms[k].slot;
            if (threadIdx.x == 0 && slot >= 0 && slot < n_terms) slots[2 * slot + 1] = Sd;
        }
        first += count;
    }
    if (threadIdx.x == 0) values[n_terms] = (float)total;
}

// ---- backward: the x chunks, then the y chunks (dy is one value per term: a fill)
__global__ __launch_bounds__(kLossBlock) void plan_bwd_kernel(const DvcPlanTerm* __restrict__ terms, int n_terms,
                                                              const DvcLossChunk* __restrict__ chunks, long n_chunks, long n_ychunks,
                                                              const double* __restrict__ slots, const float* __restrict__ grad_total,
                                                              const float* __restrict__ grad_values) {
    for (long ci = blockIdx.x; ci < n_chunks + n_ychunks; ci += gridDim.x) {
        if (ci < n_chunks) {
            LossChunk c;
            int p, wm, ti;
            if (!make_chunk(terms, n_terms, chunks, ci, true, c, p, wm, ti)) continue;
            if (!c.dx && !c.dt) continue;
            const double up = (double)grad_total[0] + (grad_values ? (double)grad_values[ti] : 0.0);
            const float coef = (float)(up * (double)terms[ti].scale / (double)terms[ti].n);
            const int kind = terms[ti].kind;
            if (kind == DVC_LOSS_KIND_REL) {
                if (c.dx && rel_target(terms[ti], n_terms, slots, c)) rel_chunk_grad(c, terms[ti].c, coef);
            } else if (kind == DVC_LOSS_KIND_MEAN) {
                PLAN_DISPATCH_WM(chunk_grad, 0, c, coef);
            } else if (kind == DVC_LOSS_KIND_MSE) {
                PLAN_DISPATCH_WM(chunk_grad, 2, c, coef);
            } else if (kind == DVC_LOSS_KIND_L1) {
                PLAN_DISPATCH_WM(chunk_grad, 1, c, coef);
            }
        } else {
            int ti, len;
            long start;
            if (!make_ychunk(terms, n_terms, chunks, ci, ti, start, len)) continue;
            if (!terms[ti].dy) continue;
            const double up = (double)grad_total[0] + (grad_values ? (double)grad_values[ti] : 0.0);
            const float coef = (float)(up * (double)terms[ti].scale / (double)terms[ti].n);
            const float c2 = 2.f * coef;        // exact
            const float g = (float)(-(double)c2 * slots[2 * terms[ti].slot + 1] / (double)terms[ti].n_y);
            gfloat* dy = (gfloat*)(terms[ti].dy + start);
            const bool vec = ((uintptr_t)dy & 15) == 0;
            const vfloat4 G = {g, g, g, g};
#pragma unroll 1
            for (int r = 0; r < kLossPasses; ++r) {
                const int base = 4 * ((int)threadIdx.x + kLossBlock * r);
                if (base >= len) break;
                const int cnt = len - base < 4 ? len - base : 4;
                if (vec && cnt == 4) {
                    *(gfloat4*)(dy + base) = G;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < cnt) dy[base + k] = g;
                }
            }
        }
    }
}

// What the check and both launch entry points refuse alike: the counts and a null term table.
int plan_counts(const char* fn, const void* terms, int32_t n_terms, int64_t n_chunks, int64_t n_ychunks) {
    DVC_REQUIRE(n_terms >= 0 && n_chunks >= 0 && n_ychunks >= 0, "%s: negative count (%d terms, %ld chunks, %ld y chunks)", fn, n_terms,
                (long)n_chunks, (long)n_ychunks);
    if (n_terms == 0) return 0;
    DVC_REQUIRE(terms, "%s: null table", fn);
    DVC_REQUIRE(n_chunks >= 1, "%s: no chunks for %d terms", fn, n_terms);
    return 0;
}

}  // namespace

extern "C" int dvc_loss_plan_check(const DvcPlanTerm* terms_host, int32_t n_terms, int64_t n_chunks, int64_t n_ychunks) {
    const char* fn = "dvc_loss_plan_check";
    if (int rc = plan_counts(fn, terms_host, n_terms, n_chunks, n_ychunks)) return rc;
    if (n_terms == 0) return 0;
    int64_t want = 0, want_y = 0;
    for (int32_t k = 0; k < n_terms; ++k) {
        const DvcPlanTerm& t = terms_host[k];
        DVC_REQUIRE(t.kind >= DVC_LOSS_KIND_L1 && t.kind <= DVC_LOSS_KIND_REL, "%s: term %d: kind = %d is outside 1..4", fn, k, t.kind);
        const int want_p = t.kind == DVC_LOSS_KIND_L1 || t.kind == DVC_LOSS_KIND_MEAN ? 1 : 2;
        DVC_REQUIRE(t.p == want_p, "%s: term %d: p = %d does not belong to kind %d", fn, k, t.p, t.kind);
        DVC_REQUIRE(t.n > 0, "%s: term %d: n = %ld is not positive", fn, k, (long)t.n);
        DVC_REQUIRE(t.x, "%s: term %d: null x", fn, k);
        DVC_REQUIRE(t.plane > 0, "%s: term %d: plane = %ld is not positive", fn, k, (long)t.plane);
        DVC_REQUIRE(t.cpl >= 0 && t.cpl % t.plane == 0, "%s: term %d: cpl = %ld is not a multiple of plane = %ld", fn, k, (long)t.cpl,
                    (long)t.plane);
        DVC_REQUIRE(t.cpl == 0 || t.n % t.cpl == 0, "%s: term %d: n = %ld is not a multiple of cpl = %ld", fn, k, (long)t.n, (long)t.cpl);
        if (t.kind == DVC_LOSS_KIND_REL) {
            DVC_REQUIRE(t.y, "%s: term %d: a relativistic term with a null y", fn, k);
            DVC_REQUIRE(t.n_y > 0, "%s: term %d: n_y = %ld is not positive", fn, k, (long)t.n_y);
            DVC_REQUIRE(!t.t && !t.w && !t.dt, "%s: term %d: a relativistic term takes no target and no weights", fn, k);
            DVC_REQUIRE(t.slot >= 0 && t.slot < n_terms, "%s: term %d: slot = %d is outside [0, %d)", fn, k, t.slot, n_terms);
            for (int32_t j = 0; j < k; ++j)
                DVC_REQUIRE(terms_host[j].kind != DVC_LOSS_KIND_REL || terms_host[j].slot != t.slot,
                            "%s: term %d: slot = %d is term %d's", fn, k, t.slot, j);
            want_y += (t.n_y + DVC_LOSS_CHUNK - 1) / DVC_LOSS_CHUNK;
        } else {
            DVC_REQUIRE(!t.y && !t.dy && t.n_y == 0, "%s: term %d: y, dy and n_y belong to a relativistic term (kind 4), not to kind %d", fn,
                        k, t.kind);
        }
        want += (t.n + DVC_LOSS_CHUNK - 1) / DVC_LOSS_CHUNK;
    }
    DVC_REQUIRE(n_chunks == want, "%s: %ld chunks for terms that cut into %ld", fn, (long)n_chunks, (long)want);
    DVC_REQUIRE(n_ychunks == want_y, "%s: %ld y chunks for relativistic terms that cut into %ld", fn, (long)n_ychunks, (long)want_y);
    return 0;
}

extern "C" int dvc_loss_plan_fwd(const DvcPlanTerm* terms, int32_t n_terms, const DvcLossChunk* chunks, int64_t n_chunks,
                                 int64_t n_ychunks, double* scratch, float* values, dvcStream stream) {
    const char* fn = "dvc_loss_plan_fwd";
    if (int rc = plan_counts(fn, terms, n_terms, n_chunks, n_ychunks)) return rc;
    if (n_terms == 0) return 0;
    DVC_REQUIRE(chunks, "%s: null table", fn);
    DVC_REQUIRE(scratch && values, "%s: null scratch / values", fn);
    const PlanScratch s = plan_scratch(scratch, (long)n_chunks, (long)n_ychunks);
    if (n_ychunks > 0) {
        const unsigned ygrid = (unsigned)(n_ychunks < kLossMaxBlocks ? n_ychunks : kLossMaxBlocks);
        hipLaunchKernelGGL(plan_ysum_kernel, dim3(ygrid), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms,
                           chunks + n_chunks, (long)n_ychunks, s.part_y);
        DVC_CHECK_LAUNCH(fn);
        hipLaunchKernelGGL(plan_mean_kernel, dim3(1), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms,
                           (const double*)s.part_y, (long)n_ychunks, s.slots);
        DVC_CHECK_LAUNCH(fn);
    }
    const unsigned grid = (unsigned)(n_chunks < kLossMaxBlocks ? n_chunks : kLossMaxBlocks);
    hipLaunchKernelGGL(plan_partial_kernel, dim3(grid), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms, chunks,
                       (long)n_chunks, s.part, s.part_d, (const double*)s.slots);
    DVC_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(plan_finish_kernel, dim3(1), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms,
                       (const double*)s.part, (const double*)s.part_d, (long)n_chunks, s.slots, values);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int dvc_loss_plan_bwd(const DvcPlanTerm* terms, int32_t n_terms, const DvcLossChunk* chunks, int64_t n_chunks,
                                 int64_t n_ychunks, const double* scratch, const float* grad_total, const float* grad_values,
                                 dvcStream stream) {
    const char* fn = "dvc_loss_plan_bwd";
    if (int rc = plan_counts(fn, terms, n_terms, n_chunks, n_ychunks)) return rc;
    if (n_terms == 0) return 0;
    DVC_REQUIRE(chunks, "%s: null table", fn);
    DVC_REQUIRE(scratch && grad_total, "%s: null scratch / grad_total", fn);
    const PlanScratch s = plan_scratch(const_cast<double*>(scratch), (long)n_chunks, (long)n_ychunks);
    const int64_t all = n_chunks + n_ychunks;
    const unsigned grid = (unsigned)(all < kLossMaxBlocks ? all : kLossMaxBlocks);
    hipLaunchKernelGGL(plan_bwd_kernel, dim3(grid), dim3(kLossBlock), 0, (hipStream_t)stream, terms, (int)n_terms, chunks, (long)n_chunks,
                       (long)n_ychunks, (const double*)s.slots, grad_total, grad_values);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}
