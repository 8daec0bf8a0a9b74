// dvc_bgemm_splitk's contract (include/dvc_hip.h; csrc/bgemm.hip) on the bf16 matrix pipes of gfx950, at fp32-grade accuracy:
//
//   C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n]        fp32 in, fp32 out, strided views, one inner stride of A and of B equal to 1
//
// The split.  Every fp32 operand element x is cut, on its way from registers into LDS, into three bf16 terms with
// x1 + x2 + x3 == x exactly, by rounding to nearest-even (v_cvt_pk_bf16_f32, two elements per instruction):
//   x1 = bf16(clamp(x, -M, M)), M = 0x1.FEp127 the largest finite bf16;   x2 = bf16(x - x1);   x3 = x - x1 - x2.
// The subtractions are exact; |x - x1| <= 2^-8 2^e for x in [2^e, 2^(e+1)), a multiple of ulp(x), so x2 keeps its upper 8
// bits and what is left, at most 8 bits, is x3 itself.  Rounding to nearest alone would take every |x| >= 0x1.FFp127 (FLT_MAX
// among them) to infinity; the clamp gives those x1 = +-M, which is their truncation, and their residual is below 2^120: no
// term of a finite x is ever infinite.  An infinite or NaN x passes through x - x1 into x2 (Inf - M = Inf).
//
// The products.  a b = sum over the nine a_i b_j.  Eight run on v_mfma_f32_32x32x16_bf16 with fp32 accumulators:
//   a1 b1                                              into the high accumulator   (one addition per k-step of 16)
//   a3 b2, a2 b3, a3 b1, a2 b2, a1 b3, a2 b1, a1 b2    into the low accumulator, in this order, every k-step
// and the low accumulator is added to the high one once, in the epilogue (hi + lo), so the large sum sees K / 16 additions and
// not 8 K / 16.  Only a3 b3 is dropped.  |x2| <= 2^-8 |x| and |x3| <= 2^-16 |x| (both reached just above a power of two; 2^-9
// and 2^-17 just below one), so a3 b3 is at most 2^-32 |a||b| = U / 256 |a||b| with U = 2^-24.  a2 b3 and a3 b2 cannot be
// dropped with it inside a budget of U / 4 per product: each reaches 2^-24 |a||b|, and on 10^6 random pairs the three together
// measured 0.85 U at the largest — U / 4 for six products would need 9 significant bits per term — so they are computed: two
// more MFMAs per tile and step, no more staging.  Restated in float64 by tests/bgemm_split3_reference.py, checked by
// tests/test_bgemm_split3_host.py.  Each of the eight products is exact in fp32 (8 x 8 bits); what rounds is the MFMA's 16-deep
// sum and the accumulator additions.  The bound the fp32 kernel is held to, (K + 2) U (|A||B| + |C0|), is asserted for this
// kernel too (tests/test_gpu_bgemm_split3.py; measured: DESIGN.md 6d).
//
// Special values.  Zeros stay exact (every term of +-0 is a zero).  A non-finite input gives a non-finite output in the
// elements the fp32 kernel makes non-finite, but the kind may differ: Inf splits into (M, Inf, NaN), so Inf * 2 arrives as
// NaN.  Inputs below 2^-100 in magnitude are outside the accuracy bound (their low terms may underflow in bf16); the result
// is finite.
//
// Tiling.  bgemm.hip's: a workgroup of 4 waves owns a 128 x 128 tile of C, wave w the 64 x 64 quarter (w & 1, w >> 1) as 2 x 2
// MFMA tiles, twice: 64 high and 64 low accumulator registers.  K advances in steps of 16 = one MFMA.  LDS holds, per operand,
// three planes of bf16 [k half (k >> 3)][128 rows][8 k]: a lane's fragment (row l & 31, k = 8 (l >> 5) .. + 7) is one
// ds_read_b128, 32 lanes read 512 contiguous bytes.  12 reads feed the 32 MFMAs of a step.  The halves are 64 elements more
// than 128 rows apart so that the 8-byte stores of the k-unit staging fall into different banks.  The global read:
//   unit stride along the row index: thread t takes row t & 127, k half t >> 7: 8 dword reads, each a wave's 256 contiguous
//                                    bytes; three 16-byte LDS stores;
//   unit stride along k:             bgemm.hip's read (4 lanes cover the 64 bytes of a row's 16 k; float4 where pointer and
//                                    strides allow, else dwords); six 8-byte LDS stores.
// The next step's elements are fetched before the MFMAs of the current one and split and stored after them (one LDS buffer,
// two barriers per step).  Tails in M, N and K are zero-filled on the read and predicated on the store.
//
// Split-K: bgemm_common.h's policy and slice sum, unchanged — the slice count is a function of M, N, K only.  No atomics.
#include "bgemm_common.h"

typedef float s3_f16v __attribute__((ext_vector_type(16)));
typedef __bf16 s3_bf8v __attribute__((ext_vector_type(8)));

constexpr int kS3Half = kBgT * 8 + 64;      // bf16 elements between the two k halves of a plane
constexpr int kS3Plane = 2 * kS3Half;
constexpr int kS3Operand = 3 * kS3Plane;

typedef float s3_f2v __attribute__((ext_vector_type(2)));
typedef __bf16 s3_bf2v __attribute__((ext_vector_type(2)));

// (lo, hi) rounded to nearest-even bf16, lo in the low half of the word
__device__ __forceinline__ unsigned s3_pack(float lo, float hi) {
    const s3_f2v v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, s3_bf2v));
}

// Two elements at once: x = the low halves of w[0], w[1], w[2] summed, y = the high halves, exactly.
__device__ __forceinline__ void s3_split(float x, float y, unsigned (&w)[3]) {
    constexpr float kMax = 0x1.fep127f;
    w[0] = s3_pack(__builtin_amdgcn_fmed3f(x, -kMax, kMax), __builtin_amdgcn_fmed3f(y, -kMax, kMax));
    x -= __uint_as_float(w[0] << 16), y -= __uint_as_float(w[0] & 0xffff0000u);
    w[1] = s3_pack(x, y);
    x -= __uint_as_float(w[1] << 16), y -= __uint_as_float(w[1] & 0xffff0000u);
    w[2] = s3_pack(x, y);
}

// The 8 elements a thread stages per step: ROW_UNIT: row tid & 127, k = k0 + 8 (tid >> 7) + i; else rows (tid >> 2) and
// (tid >> 2) + 64, k = k0 + 4 (tid & 3) + (i & 3).  base: the image's operand; element (row, k) at row * s_row + k * s_k.
template <bool ROW_UNIT>
__device__ __forceinline__ void s3_load(const float* __restrict__ base, long s_row, long s_k, int row0, int rows, int k0, int kend,
                                        int vec, int tid, float (&r)[8]) {
    if (ROW_UNIT) {
        const int row = row0 + (tid & 127), kb = k0 + 8 * (tid >> 7);
        const float* p = base + (long)kb * s_k + row;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (row < rows && kb + i < kend) ? p[(long)i * s_k] : 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = row0 + (tid >> 2) + 64 * j, k = k0 + (tid & 3) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
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
            r[4 * j] = v.x, r[4 * j + 1] = v.y, r[4 * j + 2] = v.z, r[4 * j + 3] = v.w;
        }
    }
}

template <bool ROW_UNIT>
__device__ __forceinline__ void s3_stage(unsigned short* s, const float (&r)[8], int tid) {
    unsigned w[3][4];                                   // plane p, bf16 pair q = elements 2 q (low half) and 2 q + 1
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned t[3];
        s3_split(r[2 * q], r[2 * q + 1], t);
#pragma unroll
        for (int p = 0; p < 3; ++p) w[p][q] = t[p];
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        if (ROW_UNIT) {
            *reinterpret_cast<uint4*>(s + p * kS3Plane + (tid >> 7) * kS3Half + (tid & 127) * 8) =
                make_uint4(w[p][0], w[p][1], w[p][2], w[p][3]);
        } else {
            unsigned short* d = s + p * kS3Plane + ((tid & 3) >> 1) * kS3Half + (tid >> 2) * 8 + (tid & 1) * 4;
            *reinterpret_cast<uint2*>(d) = make_uint2(w[p][0], w[p][1]);
            *reinterpret_cast<uint2*>(d + 64 * 8) = make_uint2(w[p][2], w[p][3]);
        }
    }
}

__device__ __forceinline__ s3_f16v s3_mfma(const uint4& a, const uint4& b, s3_f16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(s3_bf8v, a), __builtin_bit_cast(s3_bf8v, b), c, 0, 0, 0);
}

// grid (N tiles, M tiles, batch * S)
template <bool A_M_UNIT, bool B_N_UNIT>
__global__ __launch_bounds__(256) void s3_kernel(BgArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short sA[kS3Operand];
    __shared__ __attribute__((aligned(16))) unsigned short sB[kS3Operand];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int n0 = blockIdx.x * kBgT, m0 = blockIdx.y * kBgT;
    const int b = blockIdx.z / a.S, sp = blockIdx.z - b * a.S;
    const int st_beg = (int)((long)sp * a.ksteps / a.S), st_end = (int)((long)(sp + 1) * a.ksteps / a.S);
    const int kend = min(a.K, st_end * kBgK);
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const float* Ab = a.A + (long)b * a.a_sb;
    const float* Bb = a.B + (long)b * a.b_sb;

    s3_f16v acc[2][2], low[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f, low[i][j][r] = 0.f;

    float ra[8], rb[8];
    s3_load<A_M_UNIT>(Ab, a.a_sm, a.a_sk, m0, a.M, st_beg * kBgK, kend, a.a_vec, tid, ra);
    s3_load<B_N_UNIT>(Bb, a.b_sn, a.b_sk, n0, a.N, st_beg * kBgK, kend, a.b_vec, tid, rb);
    const unsigned short* pa = sA + hi * kS3Half + (wm + l31) * 8;
    const unsigned short* pb = sB + hi * kS3Half + (wn + l31) * 8;
    for (int st = st_beg; st < st_end; ++st) {
        s3_stage<A_M_UNIT>(sA, ra, tid);
        s3_stage<B_N_UNIT>(sB, rb, tid);
        __syncthreads();
        if (st + 1 < st_end) {
            s3_load<A_M_UNIT>(Ab, a.a_sm, a.a_sk, m0, a.M, (st + 1) * kBgK, kend, a.a_vec, tid, ra);
            s3_load<B_N_UNIT>(Bb, a.b_sn, a.b_sk, n0, a.N, (st + 1) * kBgK, kend, a.b_vec, tid, rb);
        }
        uint4 fa[2][3], fb[2][3];                       // [MFMA tile][plane]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                fa[i][p] = *reinterpret_cast<const uint4*>(pa + p * kS3Plane + i * 32 * 8);
                fb[i][p] = *reinterpret_cast<const uint4*>(pb + p * kS3Plane + i * 32 * 8);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] = s3_mfma(fa[i][0], fb[j][0], acc[i][j]);
                low[i][j] = s3_mfma(fa[i][2], fb[j][1], low[i][j]);
                low[i][j] = s3_mfma(fa[i][1], fb[j][2], low[i][j]);
                low[i][j] = s3_mfma(fa[i][2], fb[j][0], low[i][j]);
                low[i][j] = s3_mfma(fa[i][1], fb[j][1], low[i][j]);
                low[i][j] = s3_mfma(fa[i][0], fb[j][2], low[i][j]);
                low[i][j] = s3_mfma(fa[i][1], fb[j][0], low[i][j]);
                low[i][j] = s3_mfma(fa[i][0], fb[j][1], low[i][j]);
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
                    const float v = acc[i][j][r] + low[i][j][r];
                    *dst = a.accumulate ? *dst + v : v;
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
extern "C" size_t dvc_bgemm_split3_workspace_bytes(int32_t batch, int32_t M, int32_t N, int32_t K) {
    return bg_workspace_bytes(batch, M, N, K);
}

extern "C" int dvc_bgemm_split3(const float* A, const float* B, float* C, int32_t batch, int32_t M, int32_t N, int32_t K,
                                int64_t a_sb, int64_t a_sm, int64_t a_sk, int64_t b_sb, int64_t b_sk, int64_t b_sn, int64_t c_sb,
                                int64_t ldc, int32_t accumulate, void* workspace, size_t workspace_bytes, dvcStream stream_) {
    const char* fn = "dvc_bgemm_split3";
    hipStream_t stream = (hipStream_t)stream_;
    int S;
    if (int rc = bg_check_workspace(fn, batch, M, N, K, workspace, workspace_bytes, S)) return rc;
    BgArgs a;
    if (int rc = bg_check(fn, A, B, C, batch, M, N, K, a_sb, a_sm, a_sk, b_sb, b_sk, b_sn, c_sb, ldc, accumulate, S,
                          (float*)workspace, a))
        return rc;
    const bool a_m_unit = a_sm == 1, b_n_unit = b_sn == 1;
    const dim3 grid(cdiv(N, kBgT), cdiv(M, kBgT), batch * S);
    if (a_m_unit && b_n_unit)
        hipLaunchKernelGGL((s3_kernel<true, true>), grid, dim3(256), 0, stream, a);
    else if (a_m_unit)
        hipLaunchKernelGGL((s3_kernel<true, false>), grid, dim3(256), 0, stream, a);
    else if (b_n_unit)
        hipLaunchKernelGGL((s3_kernel<false, true>), grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((s3_kernel<false, false>), grid, dim3(256), 0, stream, a);
    if (S > 1) bg_launch_reduce(a, C, batch, c_sb, ldc, accumulate, stream);
    DVC_CHECK_LAUNCH(fn);
    return 0;
}
