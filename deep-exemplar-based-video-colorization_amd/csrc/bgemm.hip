// Batched fp32 GEMM on strided views for the training side's row-block products (dvc_amd/block_products.py), for gfx950:
//
//   C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n],   A by (a_sb, a_sm, a_sk), B by (b_sb, b_sk, b_sn), C by (c_sb, ldc, 1)
//
// with one of the two inner strides of A and of B equal to 1 — a transposed or column-sliced view of a contiguous tensor.
// Products and sums run on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fma chain per output element); nothing narrower
// than fp32 appears.
//
// Tiling.  A workgroup of 4 waves owns a 128 x 128 tile of C; wave w the 64 x 64 quarter (w & 1, w >> 1) as 2 x 2 MFMA tiles
// (64 accumulator registers).  K advances in steps of 16.  Both operands are "rows x k" matrices (rows = m for A, n for B) and
// are staged in LDS k-major, s[k][row] with a row stride of 132 floats: the MFMA loop reads one dword per lane per operand
// tile (lane l: row l & 31, k = 2 kk + (l >> 5)), each half wave from 32 consecutive banks, 4 reads for 4 MFMAs of 64 cycles
// each.  The intent is a loop paced by the MFMAs; no counter run has checked the LDS side, and as measured the kernel reaches
// 60-67 % of the fp32 matrix peak at 16 images.  Only the global read depends on the orientation (bg_load /
// bg_stage):
//   unit stride along the row index: lanes run along the rows, a float4 = 4 rows of one k, stored as a float4;
//   unit stride along k:             4 lanes cover the 16 k of one row (64 contiguous bytes), a float4 = 4 k of one row,
//                                    stored as 4 dwords (rows 132 floats apart: two k of a half wave share a bank, 8 dword
//                                    stores per thread and step beside 32 MFMAs per wave).
// Either way a wave reads whole 64-byte segments.  The next step's tiles are fetched into registers before the MFMA loop of
// the current one and stored after it (one LDS buffer, two barriers per step).  float4 reads are used where the base pointer,
// the batch stride and the non-unit stride are multiples of 16 bytes (decided per launch and per operand on the host); else
// dword reads.  Tails in M, N and K are predicated on the read (zero-filled in LDS) and on the store.
//
// Split-K.  With few output tiles (d L = M dS^T: 256 x R over K = 5184 positions is 32 tiles) the K range is cut into S slices of
// whole 16-steps, S = bg_splits(M, N, K) — a function of the sizes only, never of the batch, so an image's bits do not depend
// on the batch around it.  Slice s of image b writes its tile to workspace[s][b][M][N]; a second launch adds the slices in
// order s = 0 .. S-1 (and the old C last, when accumulating).  No atomics; every sum has a fixed order.  dvc_bgemm takes no
// workspace and never splits; dvc_bgemm_splitk does when dvc_bgemm_workspace_bytes(...) > 0.  The argument checks, bg_splits
// and the slice sum live in bgemm_common.h, shared with bgemm_split3.hip.
#include "bgemm_common.h"

typedef float bg_f16v __attribute__((ext_vector_type(16)));

constexpr int kBgLd = kBgT + 4;    // LDS row stride (floats): float4 stores stay 16-byte aligned

// One operand tile [16 k][128 rows] as 2 float4 per thread.  base: the image's operand; element (row, k) at row * s_row + k * s_k.
template <bool ROW_UNIT>
__device__ __forceinline__ void bg_load(const float* __restrict__ base, long s_row, long s_k, int row0, int rows, int k0, int kend,
                                        int vec, int tid, float4 (&r)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int e = tid + 256 * j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ROW_UNIT) {
            const int k = k0 + (e >> 5), row = row0 + (e & 31) * 4;
            if (k < kend && row < rows) {
                const float* p = base + (long)k * s_k + row;
                if (vec && row + 3 < rows) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    v.x = p[0];
                    if (row + 1 < rows) v.y = p[1];
                    if (row + 2 < rows) v.z = p[2];
                    if (row + 3 < rows) v.w = p[3];
                }
            }
        } else {
            const int row = row0 + (e >> 2), k = k0 + (e & 3) * 4;
            if (row < rows && k < kend) {
                const float* p = base + (long)row * s_row + k;
                if (vec && k + 3 < kend) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    v.x = p[0];
                    if (k + 1 < kend) v.y = p[1];
                    if (k + 2 < kend) v.z = p[2];
                    if (k + 3 < kend) v.w = p[3];
                }
            }
        }
        r[j] = v;
    }
}

template <bool ROW_UNIT>
__device__ __forceinline__ void bg_stage(float* s, const float4 (&r)[2], int tid) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int e = tid + 256 * j;
        if (ROW_UNIT) {
            *reinterpret_cast<float4*>(s + (e >> 5) * kBgLd + (e & 31) * 4) = r[j];
        } else {
            float* d = s + (e & 3) * 4 * kBgLd + (e >> 2);
            d[0] = r[j].x;
            d[kBgLd] = r[j].y;
            d[2 * kBgLd] = r[j].z;
            d[3 * kBgLd] = r[j].w;
        }
    }
}

// grid (N tiles, M tiles, batch * S)
template <bool A_M_UNIT, bool B_N_UNIT>
__global__ __launch_bounds__(256) void bg_kernel(BgArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[kBgK * kBgLd];
    __shared__ __attribute__((aligned(16))) float sB[kBgK * kBgLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int n0 = blockIdx.x * kBgT, m0 = blockIdx.y * kBgT;
    const int b = blockIdx.z / a.S, sp = blockIdx.z - b * a.S;
    const int st_beg = (int)((long)sp * a.ksteps / a.S), st_end = (int)((long)(sp + 1) * a.ksteps / a.S);
    const int kend = min(a.K, st_end * kBgK);
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const float* Ab = a.A + (long)b * a.a_sb;
    const float* Bb = a.B + (long)b * a.b_sb;

    bg_f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[2], rb[2];
    bg_load<A_M_UNIT>(Ab, a.a_sm, a.a_sk, m0, a.M, st_beg * kBgK, kend, a.a_vec, tid, ra);
    bg_load<B_N_UNIT>(Bb, a.b_sn, a.b_sk, n0, a.N, st_beg * kBgK, kend, a.b_vec, tid, rb);
    for (int st = st_beg; st < st_end; ++st) {
        bg_stage<A_M_UNIT>(sA, ra, tid);
        bg_stage<B_N_UNIT>(sB, rb, tid);
        __syncthreads();
        if (st + 1 < st_end) {
            bg_load<A_M_UNIT>(Ab, a.a_sm, a.a_sk, m0, a.M, (st + 1) * kBgK, kend, a.a_vec, tid, ra);
            bg_load<B_N_UNIT>(Bb, a.b_sn, a.b_sk, n0, a.N, (st + 1) * kBgK, kend, a.b_vec, tid, rb);
        }
        const float* pa = sA + hi * kBgLd + wm + l31;
        const float* pb = sB + hi * kBgLd + wn + l31;
#pragma unroll
        for (int kk = 0; kk < kBgK / 2; ++kk) {
            const float a0 = pa[2 * kk * kBgLd], a1 = pa[2 * kk * kBgLd + 32];
            const float b0 = pb[2 * kk * kBgLd], b1 = pb[2 * kk * kBgLd + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): a register is two 128-byte row segments
    float* Cb = a.C + (long)b * a.c_sb + (long)sp * a.c_ss;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + 32 * j + l31;
        if (n >= a.N) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m < a.M) {
                    float* dst = Cb + (long)m * a.ldc + n;
                    *dst = a.accumulate ? *dst + acc[i][j][r] : acc[i][j][r];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
static int bg_run(const char* fn, const float* A, const float* B, float* C, int batch, int M, int N, int K, long a_sb, long a_sm,
                  long a_sk, long b_sb, long b_sk, long b_sn, long c_sb, long ldc, int accumulate, int S, float* workspace,
                  hipStream_t stream) {
    BgArgs a;
    if (int rc = bg_check(fn, A, B, C, batch, M, N, K, a_sb, a_sm, a_sk, b_sb, b_sk, b_sn, c_sb, ldc, accumulate, S, workspace, a))
        return rc;
    const bool a_m_unit = a_sm == 1, b_n_unit = b_sn == 1;
    const dim3 grid(cdiv(N, kBgT), cdiv(M, kBgT), batch * S);
    if (a_m_unit && b_n_unit)
        hipLaunchKernelGGL((bg_kernel<true, true>), grid, dim3(256), 0, stream, a);
    else if (a_m_unit)
        hipLaunchKernelGGL((bg_kernel<true, false>), grid, dim3(256), 0, stream, a);
    else if (b_n_unit)
        hipLaunchKernelGGL((bg_kernel<false, true>), grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((bg_kernel<false, false>), grid, dim3(256), 0, stream, a);
    if (S > 1) bg_launch_reduce(a, C, batch, c_sb, ldc, accumulate, stream);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" size_t dvc_bgemm_workspace_bytes(int32_t batch, int32_t M, int32_t N, int32_t K) {
    return bg_workspace_bytes(batch, M, N, K);
}

extern "C" int dvc_bgemm(const float* A, const float* B, float* C, int32_t batch, int32_t M, int32_t N, int32_t K, int64_t a_sb,
                         int64_t a_sm, int64_t a_sk, int64_t b_sb, int64_t b_sk, int64_t b_sn, int64_t c_sb, int64_t ldc,
                         int32_t accumulate, dvcStream stream) {
    return bg_run("dvc_bgemm", A, B, C, batch, M, N, K, a_sb, a_sm, a_sk, b_sb, b_sk, b_sn, c_sb, ldc, accumulate, 1, nullptr,
                  (hipStream_t)stream);
}

extern "C" int dvc_bgemm_splitk(const float* A, const float* B, float* C, int32_t batch, int32_t M, int32_t N, int32_t K,
                                int64_t a_sb, int64_t a_sm, int64_t a_sk, int64_t b_sb, int64_t b_sk, int64_t b_sn, int64_t c_sb,
                                int64_t ldc, int32_t accumulate, void* workspace, size_t workspace_bytes, dvcStream stream) {
    const char* fn = "dvc_bgemm_splitk";
    int S;
    if (int rc = bg_check_workspace(fn, batch, M, N, K, workspace, workspace_bytes, S)) return rc;
    return bg_run(fn, A, B, C, batch, M, N, K, a_sb, a_sm, a_sk, b_sb, b_sk, b_sn, c_sb, ldc, accumulate, S, (float*)workspace,
                  (hipStream_t)stream);
}
