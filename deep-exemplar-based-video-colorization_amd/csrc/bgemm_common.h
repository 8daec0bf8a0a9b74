// What csrc/bgemm.hip (exact-fp32 MFMA) and csrc/bgemm_split3.hip (three bf16 terms per operand on the bf16 MFMA) share: the
// 128 x 128 x 16 tiling constants, the argument block, the split-K policy and its slice sum, and the argument checks.  One
// policy, so both engines cut a given (M, N, K) into the same slices.
#pragma once
#include "common.h"

#include <algorithm>
#include <cstdint>

constexpr int kBgT = 128;          // tile of C, both ways
constexpr int kBgK = 16;           // k per step
constexpr int kBgFill = 256;       // split until about this many workgroups per image
constexpr int kBgMinSteps = 16;    // ... but keep at least 16 steps (256 k) per slice
constexpr int kBgMaxSplits = 16;

struct BgArgs {
    const float* A;
    const float* B;
    float* C;          // the output, or the partial-sum workspace when S > 1
    int M, N, K, S, ksteps, a_vec, b_vec, accumulate;
    long a_sb, a_sm, a_sk, b_sb, b_sk, b_sn, c_sb, c_ss, ldc;
};

// C[b][m][n] = (C[b][m][n] +) part[0][b][m][n] + part[1][b][m][n] + ... in slice order; grid (blocks over M N, batch)
static __global__ __launch_bounds__(256) void bg_reduce_kernel(const float* __restrict__ part, float* __restrict__ C, int N, long MN,
                                                               int S, long slice_stride, long c_sb, long ldc, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    const int b = blockIdx.y;
    const float* p = part + (long)b * MN + i;
    float s = p[0];
    for (int k = 1; k < S; ++k) s += p[(long)k * slice_stride];
    const long m = i / N, n = i - m * N;
    float* dst = C + (long)b * c_sb + m * ldc + n;
    *dst = accumulate ? *dst + s : s;
}

static int bg_splits(int M, int N, int K) {
    const long tiles = (long)cdiv(M, kBgT) * cdiv(N, kBgT);
    long s = kBgFill / tiles;
    s = std::min<long>(s, cdiv(K, kBgK) / kBgMinSteps);
    s = std::min<long>(s, kBgMaxSplits);
    return (int)std::max<long>(s, 1);
}

static bool bg_sizes_ok(int batch, int M, int N, int K) { return batch >= 1 && M >= 1 && N >= 1 && K >= 1; }

static bool bg_vec_ok(const float* p, long sb, long s_other) { return ((uintptr_t)p & 15) == 0 && sb % 4 == 0 && s_other % 4 == 0; }

static size_t bg_workspace_bytes(int batch, int M, int N, int K) {
    if (!bg_sizes_ok(batch, M, N, K)) return 0;
    const int S = bg_splits(M, N, K);
    return S > 1 ? (size_t)S * (size_t)batch * (size_t)M * (size_t)N * sizeof(float) : 0;
}

// The slice count of a split-K call into S (1 for sizes bg_check will refuse), after the workspace checks.
static int bg_check_workspace(const char* fn, int batch, int M, int N, int K, const void* workspace, size_t workspace_bytes, int& S) {
    S = 1;
    if (!bg_sizes_ok(batch, M, N, K)) return 0;
    S = bg_splits(M, N, K);
    if (S > 1) {
        const size_t need = bg_workspace_bytes(batch, M, N, K);
        DVC_REQUIRE(workspace, "%s: these sizes need a workspace of %zu bytes (got NULL)", fn, need);
        DVC_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", fn, workspace_bytes, need);
        DVC_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", fn);
    }
    return 0;
}

// Every refusal, before any launch; then the argument block (C = the workspace, one slice after another, when S > 1).
static int bg_check(const char* fn, const float* A, const float* B, float* C, int batch, int M, int N, int K, long a_sb, long a_sm,
                    long a_sk, long b_sb, long b_sk, long b_sn, long c_sb, long ldc, int accumulate, int S, float* workspace,
                    BgArgs& a) {
    DVC_REQUIRE(A && B && C, "%s: null argument", fn);
    DVC_REQUIRE(bg_sizes_ok(batch, M, N, K), "%s: bad shape (batch %d, M %d, N %d, K %d)", fn, batch, M, N, K);
    DVC_REQUIRE(ldc >= N, "%s: ldc (%ld) is below N (%d)", fn, ldc, N);
    DVC_REQUIRE(a_sm == 1 || a_sk == 1, "%s: neither inner stride of A is 1 (a_sm %ld, a_sk %ld)", fn, a_sm, a_sk);
    DVC_REQUIRE(b_sk == 1 || b_sn == 1, "%s: neither inner stride of B is 1 (b_sk %ld, b_sn %ld)", fn, b_sk, b_sn);
    DVC_REQUIRE(a_sb >= 0 && a_sm >= 0 && a_sk >= 0 && b_sb >= 0 && b_sk >= 0 && b_sn >= 0 && c_sb >= 0,
                "%s: negative stride", fn);
    DVC_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1 (got %d)", fn, accumulate);
    DVC_REQUIRE(cdiv(M, kBgT) <= 65535 && (long)batch * S <= 65535, "%s: M or batch too large for one launch", fn);
    const long MN = (long)M * N;
    DVC_REQUIRE(S == 1 || (cdivl(MN, 256) <= 0x7fffffffL && batch <= 65535), "%s: M * N too large for the split-K reduce", fn);

    a.A = A, a.B = B;
    a.M = M, a.N = N, a.K = K, a.S = S, a.ksteps = cdiv(K, kBgK);
    a.a_sb = a_sb, a.a_sm = a_sm, a.a_sk = a_sk, a.b_sb = b_sb, a.b_sk = b_sk, a.b_sn = b_sn;
    a.a_vec = bg_vec_ok(A, a_sb, a_sm == 1 ? a_sk : a_sm);
    a.b_vec = bg_vec_ok(B, b_sb, b_sn == 1 ? b_sk : b_sn);
    if (S == 1) {
        a.C = C, a.c_sb = c_sb, a.c_ss = 0, a.ldc = ldc, a.accumulate = accumulate;
    } else {
        a.C = workspace, a.c_sb = MN, a.c_ss = (long)batch * MN, a.ldc = N, a.accumulate = 0;
    }
    return 0;
}

// The slices of workspace[s][b][M][N] into C, in slice order (the old C last, when accumulating).
static void bg_launch_reduce(const BgArgs& a, float* C, int batch, long c_sb, long ldc, int accumulate, hipStream_t stream) {
    const long MN = (long)a.M * a.N;
    hipLaunchKernelGGL(bg_reduce_kernel, dim3((unsigned)cdivl(MN, 256), batch), dim3(256), 0, stream, a.C, C, a.N, MN, a.S,
                       (long)batch * MN, c_sb, ldc, accumulate);
}
