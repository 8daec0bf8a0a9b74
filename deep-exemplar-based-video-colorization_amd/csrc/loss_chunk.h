// The element and chunk code of the pixel losses, shared by csrc/loss.hip (dvc_loss_fwd / dvc_loss_bwd) and csrc/loss_plan.hip
// (dvc_loss_plan_fwd / dvc_loss_plan_bwd): one chunk's descriptor, its loads, its forward sum and its gradient.  Both translation
// units instantiate the SAME templates, so a kind-1 or kind-2 term of a plan has dvc_loss_fwd's bits by construction (DESIGN.md
// §6d).  Thread j of a chunk owns the elements 4 (j + 256 r) + k, r = 0..3, k = 0..3, whichever path loads them, and adds their
// fp32 values into a double in that order.
// Device only; the library is built with -fno-gpu-rdc: everything here is in an anonymous namespace and each including file gets
// its own instance.  The including file sets `#pragma clang fp contract(off)` before the include.
#pragma once
#include "common.h"
#include "reduce.h"

#include <cstdint>

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

// ---- forward, stage 1.  P: 2 d*d, 1 |d|, 0 d itself (the signed mean of a plan, csrc/loss_plan.hip)
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
                const float e = P == 2 ? d * d : (P == 1 ? fabsf(d) : d);
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
            G[k] = P == 2 ? cw * d : (P == 1 ? cw * s : cw);
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

// The chunk's descriptor from the two tables (Term: DvcLossTerm, or DvcPlanTerm, whose first 80 bytes are the same fields);
// false for a chunk that names no element of any term (skipped).
template <typename Term>
__device__ __forceinline__ bool make_chunk(const Term* terms, int n_terms, const DvcLossChunk* chunks, long ci, bool backward,
                                           LossChunk& c, int& p, int& wm, int& ti) {
    ti = chunks[ci].term;
    const long start = chunks[ci].start;
    if (ti < 0 || ti >= n_terms) return false;
    const Term* t = terms + ti;
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

}  // namespace
