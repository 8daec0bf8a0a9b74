// Non-local weighted average (NonlocalWeightedAverage, models/NonlocalNet.py:86-111, find_local_patch :12-17) for gfx950.
//
//   U[c*k*k + ky*k + kx][i] = F_pad[c][y_i + ky][x_i + kx]     k x k patches of the resized feature, zero border k/2
//   A[i][:] = softmax_j( <U[:,i], U[:,j]> / alpha )             N x N self-affinity, K = C*k*k deep
//   out[:, i] = sum_j A[i][j] ab[:, j]                           2-channel gather of the resized ab
//
// Two launches plus a merge; nothing N x N (107 MB per image at 54 x 96) and nothing k*k-times unfolded is written:
//   * prep: nearest-resizes feature into F_pad[B][Cp][H+2p][W+2p] (zero border p = k/2, zero planes up to Cp, a multiple
//     of NL_KC) and x_lab's channels 1..2 into ab[B][2][N], both with ATen's nearest rule src = min(floor(dst*scale), in-1);
//   * fused forward, flash-style on v_mfma_f32_32x32x2_f32 (exact fp32): a workgroup owns 128 query positions and sweeps
//     a contiguous range of 128-key tiles.  The K loop walks chunks = (shift (ky, kx), group of NL_KC channels); the
//     operand rows of a chunk are shifted windows of F_pad (row i of the query / key tile is F_pad[c][base_i + shift],
//     base_i = y_i (W+2p) + x_i), so both tiles are gathered straight from F_pad by LDS-DMA — double buffered, one
//     barrier per chunk.  Each wave computes a 64-query x 64-key block (2 x 2 accumulators, S^T = keys x queries as in
//     corr_fwd_kernel: a lane holds 32 keys of one query, the row softmax is lane-local).  After a tile's last chunk the
//     online softmax folds the block into per-lane (m, l, y0, y1);
//   * merge: the partial states of a query (2 waves x NL split workgroups) are combined in a fixed order.
// The key range is split into `nsplit` workgroups per query block, a function of N only (not of B), so an image's result
// does not depend on the batch it came in; no atomics.
//
// Softmax form: the running maximum m is kept in the AFFINITY domain and p = exp2((f - m) * c), c = log2(e) / alpha
// (clamped to FLT_MAX): the maximum gets exp2(0) = 1 exactly, equal affinities get equal weights, and no alpha > 0 can
// overflow or produce inf - inf, so every row is a convex combination.
#include "common.h"

#include <cfloat>
#include <cmath>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define NL_QB 128     // queries per workgroup (2 query halves x 64)
#define NL_KT 128     // keys per tile (2 key halves x 64)
#define NL_KC 32      // channels per K chunk
#define NL_NF 4       // fields per partial state: m, l, y0, y1
#define NL_WG_TARGET 512   // resident workgroups to aim for: 2 per CU x 256 CUs

#define AS1 __attribute__((address_space(1)))
#define AS3 __attribute__((address_space(3)))

// ------------------------------------------------------------------------------------------------
// prep: blockIdx.y = plane (0 .. Cp-1: F_pad, Cp / Cp+1: ab), blockIdx.z = image
__global__ __launch_bounds__(256) void nlwa_prep_kernel(const float* __restrict__ x_lab, int Cx, int Hx, int Wx, float sxh,
                                                        float sxw, const float* __restrict__ feat, int C, int Hf, int Wf,
                                                        float sfh, float sfw, int H, int W, int p, int Cp,
                                                        float* __restrict__ fpad, float* __restrict__ ab) {
    const int plane = blockIdx.y, b = blockIdx.z;
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (plane < Cp) {
        if (e >= Hp * Wp) return;
        const int y = e / Wp - p, x = e % Wp - p;
        float v = 0.f;
        if (plane < C && y >= 0 && y < H && x >= 0 && x < W) {
            const int sy = min((int)floorf((float)y * sfh), Hf - 1), sx = min((int)floorf((float)x * sfw), Wf - 1);
            v = feat[(((long)b * C + plane) * Hf + sy) * Wf + sx];
        }
        fpad[(((long)b * Cp + plane) * Hp) * Wp + e] = v;
    } else {
        if (e >= H * W) return;
        const int j = plane - Cp, y = e / W, x = e % W;
        const int sy = min((int)floorf((float)y * sxh), Hx - 1), sx = min((int)floorf((float)x * sxw), Wx - 1);
        ab[((long)b * 2 + j) * H * W + e] = x_lab[(((long)b * Cx + 1 + j) * Hx + sy) * Wx + sx];
    }
}

// ------------------------------------------------------------------------------------------------
struct NlwaArgs {
    const float* fpad;   // [B][Cp][Hp][Wp]
    const float* ab;     // [B][2][N]
    float* part;         // [B][2 * nsplit][NL_NF][N]
    float c;             // log2(e) / alpha, clamped to FLT_MAX
    int N, W, Wp, k, Cp;
    long plane;          // Hp * Wp
    int ntiles, nsplit;
};

// grid (query block, key split, image)
__global__ __launch_bounds__(256, 2) void nlwa_fwd_kernel(NlwaArgs a) {
    // [buf][Q | K][NL_KC][128]: 2 x 32 KB
    __shared__ __attribute__((aligned(16))) float smem[2 * 2 * NL_KC * 128];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int qb = blockIdx.x, sp = blockIdx.y, b = blockIdx.z;
    const int N = a.N, W = a.W, Wp = a.Wp, k = a.k;
    const int t0 = (int)((long)sp * a.ntiles / a.nsplit), t1 = (int)((long)(sp + 1) * a.ntiles / a.nsplit);
    const int ngroups = a.Cp / NL_KC, nch = k * k * ngroups;
    const int nit = (t1 - t0) * nch;
    const float* fb = a.fpad + (long)b * a.Cp * a.plane;
    const float* abb = a.ab + (long)b * 2 * N;

    // F_pad offset of a position (clamped into the image: rows past N are computed and discarded / masked)
    auto base_of = [&](int pos) {
        pos = min(pos, N - 1);
        const int y = pos / W;
        return (unsigned)(y * Wp + (pos - y * W));
    };
    const unsigned qbase0 = base_of(qb * NL_QB + lane), qbase1 = base_of(qb * NL_QB + 64 + lane);
    unsigned kbase0 = 0, kbase1 = 0;
    int ktile_staged = -1;

    // LDS-DMA of the next chunk of this workgroup's range into buffer `buf`: wave w moves channels 8w .. 8w+7 of the chunk,
    // each as 2 x 64 positions for the query tile and for the key tile (lane -> position, 4 bytes each)
    int is_t = t0, is_ch = 0;   // the next chunk to stage: key tile, chunk within the tile
    auto issue = [&](int buf) {
        const int t = is_t, ch = is_ch;
        if (++is_ch == nch) {
            is_ch = 0;
            ++is_t;
        }
        if (t != ktile_staged) {
            ktile_staged = t;
            kbase0 = base_of(t * NL_KT + lane);
            kbase1 = base_of(t * NL_KT + 64 + lane);
        }
        const int s = ch / ngroups, g = ch - s * ngroups;
        const int ky = s / k, kx = s - ky * k;
        const float* src = fb + (long)(g * NL_KC + wave * 8) * a.plane + (ky * Wp + kx);
        float* dq = smem + buf * (2 * NL_KC * 128) + (wave * 8) * 128;
        float* dk = dq + NL_KC * 128;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* row = src + i * a.plane;
            __builtin_amdgcn_global_load_lds((const AS1 void*)(row + qbase0), (AS3 void*)(dq + i * 128), 4, 0, 0);
            __builtin_amdgcn_global_load_lds((const AS1 void*)(row + qbase1), (AS3 void*)(dq + i * 128 + 64), 4, 0, 0);
            __builtin_amdgcn_global_load_lds((const AS1 void*)(row + kbase0), (AS3 void*)(dk + i * 128), 4, 0, 0);
            __builtin_amdgcn_global_load_lds((const AS1 void*)(row + kbase1), (AS3 void*)(dk + i * 128 + 64), 4, 0, 0);
        }
    };

    // wave w: queries (w >> 1) * 64 + [0, 64) of the block, keys (w & 1) * 64 + [0, 64) of each tile
    const int qoff = (wave >> 1) * 64 + l31, koff = (wave & 1) * 64 + l31;
    f32x16 acc[2][2];   // [key half][query half]: D[row = key][col = query]
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int qh = 0; qh < 2; ++qh)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kb][qh][r] = 0.f;
    float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f}, y0[2] = {0.f, 0.f}, y1[2] = {0.f, 0.f};
    const float c = a.c;

    // online softmax of one finished key tile
    auto process_tile = [&](int t) {
        const int kt0 = t * NL_KT + (wave & 1) * 64;
        float a0[2][16], a1[2][16];
        bool kv[2][16];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                kv[kb][r] = key < N;
                const int kc = kv[kb][r] ? key : 0;
                a0[kb][r] = abb[kc];
                a1[kb][r] = abb[N + kc];
            }
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
            float tmax = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float f = kv[kb][r] ? acc[kb][qh][r] : -INFINITY;
                    acc[kb][qh][r] = f;
                    tmax = fmaxf(tmax, f);
                }
            const float mn = fmaxf(m[qh], tmax);
            // (mn == -inf: every key of this half lies past N — nothing to add; m == -inf: nothing to rescale)
            const float sc = m[qh] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((m[qh] - mn) * c);
            const float base = mn == -INFINITY ? 0.f : mn;
            float ll = l[qh] * sc, s0 = y0[qh] * sc, s1 = y1[qh] * sc;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pe = __builtin_amdgcn_exp2f((acc[kb][qh][r] - base) * c);
                    ll += pe;
                    s0 = fmaf(pe, a0[kb][r], s0);
                    s1 = fmaf(pe, a1[kb][r], s1);
                }
            m[qh] = mn;
            l[qh] = ll;
            y0[qh] = s0;
            y1[qh] = s1;
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int qh = 0; qh < 2; ++qh)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[kb][qh][r] = 0.f;
    };

    issue(0);
    __syncthreads();
    int tc = t0, cc = 0;   // the chunk being computed
    for (int it = 0; it < nit; ++it) {
        const int cur = it & 1;
        if (it + 1 < nit) issue(cur ^ 1);
        const float* Qs = smem + cur * (2 * NL_KC * 128);
        const float* Ks = Qs + NL_KC * 128;
        // fragments: A[i = key l31][k = hi] and B[k = hi][j = query l31], channel row 2s + hi
        float fq[NL_KC / 2][2], fk[NL_KC / 2][2];
#pragma unroll
        for (int s = 0; s < NL_KC / 2; ++s) {
            const int row = (2 * s + hi) * 128;
            fk[s][0] = Ks[row + koff];
            fk[s][1] = Ks[row + koff + 32];
            fq[s][0] = Qs[row + qoff];
            fq[s][1] = Qs[row + qoff + 32];
        }
#pragma unroll
        for (int s = 0; s < NL_KC / 2; ++s)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qh = 0; qh < 2; ++qh)
                    acc[kb][qh] = __builtin_amdgcn_mfma_f32_32x32x2f32(fk[s][kb], fq[s][qh], acc[kb][qh], 0, 0, 0);
        if (++cc == nch) {
            process_tile(tc);
            cc = 0;
            ++tc;
        }
        __syncthreads();   // chunk it+1 landed (DMA drained); every wave is done reading buffer `cur`
    }

    // combine the two key quarters of a query held by lanes l and l ^ 32 (fixed order: lower lane's state first), then
    // store this wave's partial state in slot 2 * split + (wave & 1)
    const int slot = 2 * sp + (wave & 1), nslot = 2 * a.nsplit;
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
        const float mo = __shfl_xor(m[qh], 32), lo = __shfl_xor(l[qh], 32), y0o = __shfl_xor(y0[qh], 32),
                    y1o = __shfl_xor(y1[qh], 32);
        const float M = fmaxf(m[qh], mo);
        const float sa = m[qh] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((m[qh] - M) * c);
        const float sb = mo == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((mo - M) * c);
        const int query = qb * NL_QB + (wave >> 1) * 64 + qh * 32 + l31;
        if (hi == 0 && query < N) {
            float* pp = a.part + (((long)b * nslot + slot) * NL_NF) * N + query;
            pp[0] = M;
            pp[(long)N] = fmaf(lo, sb, l[qh] * sa);
            pp[2L * N] = fmaf(y0o, sb, y0[qh] * sa);
            pp[3L * N] = fmaf(y1o, sb, y1[qh] * sa);
        }
    }
}

// merge the partial states of each query in slot order; out[B][2][N]
__global__ __launch_bounds__(256) void nlwa_merge_kernel(const float* __restrict__ part, int nslot, int N, float c,
                                                         float* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (q >= N) return;
    const float* pb = part + (long)b * nslot * NL_NF * N + q;
    float M = -INFINITY;
    for (int s = 0; s < nslot; ++s) M = fmaxf(M, pb[(long)s * NL_NF * N]);
    float L = 0.f, Y0 = 0.f, Y1 = 0.f;
    for (int s = 0; s < nslot; ++s) {
        const float* ps = pb + (long)s * NL_NF * N;
        const float ms = ps[0];
        const float sc = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((ms - M) * c);
        L = fmaf(ps[(long)N], sc, L);
        Y0 = fmaf(ps[2L * N], sc, Y0);
        Y1 = fmaf(ps[3L * N], sc, Y1);
    }
    out[((long)b * 2) * N + q] = Y0 / L;
    out[((long)b * 2 + 1) * N + q] = Y1 / L;
}

// ------------------------------------------------------------------------------------------------
struct NlwaPlan {
    int Cp, p, Hp, Wp, ntiles, nqb, nsplit;
    size_t fpad_off, ab_off, part_off, bytes;
};
static size_t nl_align(size_t x) { return (x + 255) & ~(size_t)255; }
static NlwaPlan nlwa_plan(int B, int C, int k, int H, int W) {
    NlwaPlan pl;
    const long N = (long)H * W;
    pl.Cp = cdiv(C, NL_KC) * NL_KC;
    pl.p = k / 2;
    pl.Hp = H + 2 * pl.p;
    pl.Wp = W + 2 * pl.p;
    pl.ntiles = (int)cdivl(N, NL_KT);
    pl.nqb = (int)cdivl(N, NL_QB);
    // key splits per query block: one image's workgroups fill the resident slots but never exceed them (at 54 x 96:
    // 41 query blocks x 12 splits = 492; 13 splits = 533 would run 21 workgroups as a second round), never more than the tiles
    pl.nsplit = std::min(pl.ntiles, std::max(1, NL_WG_TARGET / pl.nqb));
    pl.fpad_off = 0;
    pl.ab_off = nl_align((size_t)B * pl.Cp * pl.Hp * pl.Wp * sizeof(float));
    pl.part_off = pl.ab_off + nl_align((size_t)B * 2 * N * sizeof(float));
    pl.bytes = pl.part_off + nl_align((size_t)B * 2 * pl.nsplit * NL_NF * N * sizeof(float));
    return pl;
}

extern "C" size_t dvc_nlwa_workspace_bytes(int32_t B, int32_t C, int32_t k, int32_t H, int32_t W) {
    if (B <= 0 || C <= 0 || k <= 0 || H <= 0 || W <= 0) return 0;
    return nlwa_plan(B, C, k, H, W).bytes;
}

extern "C" int dvc_nlwa_fwd(const float* x_lab, int32_t Cx, int32_t Hx, int32_t Wx, const float* feature, int32_t C,
                            int32_t Hf, int32_t Wf, int32_t B, int32_t H, int32_t W, float scale_xh, float scale_xw,
                            float scale_fh, float scale_fw, int32_t patch_size, float alpha, float* out, void* workspace,
                            size_t workspace_bytes, dvcStream stream) {
    DVC_REQUIRE(x_lab && feature && out && workspace, "dvc_nlwa_fwd: null argument");
    DVC_REQUIRE(B > 0 && C > 0 && Hx > 0 && Wx > 0 && Hf > 0 && Wf > 0 && H > 0 && W > 0, "dvc_nlwa_fwd: bad shape");
    DVC_REQUIRE(Cx >= 3, "dvc_nlwa_fwd: x_lab needs at least 3 channels (L, a, b; got %d)", Cx);
    DVC_REQUIRE(patch_size >= 1 && patch_size % 2 == 1, "dvc_nlwa_fwd: patch_size must be odd and >= 1 (got %d)", patch_size);
    DVC_REQUIRE(alpha > 0.f && std::isfinite(alpha), "dvc_nlwa_fwd: alpha must be > 0 and finite (got %g)", (double)alpha);
    DVC_REQUIRE(scale_xh > 0.f && scale_xw > 0.f && scale_fh > 0.f && scale_fw > 0.f && std::isfinite(scale_xh) &&
                    std::isfinite(scale_xw) && std::isfinite(scale_fh) && std::isfinite(scale_fw),
                "dvc_nlwa_fwd: resize scales must be > 0 and finite");
    DVC_REQUIRE(patch_size / 2 < 1024 && (long)(H + patch_size) * (W + patch_size) < (1L << 30),
                "dvc_nlwa_fwd: map too large");
    DVC_REQUIRE(workspace_bytes >= dvc_nlwa_workspace_bytes(B, C, patch_size, H, W), "dvc_nlwa_fwd: workspace too small");
    DVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "dvc_nlwa_fwd: workspace must be 256-byte aligned");
    const NlwaPlan pl = nlwa_plan(B, C, patch_size, H, W);
    const int N = H * W;
    char* ws = reinterpret_cast<char*>(workspace);
    NlwaArgs a;
    a.fpad = reinterpret_cast<const float*>(ws + pl.fpad_off);
    a.ab = reinterpret_cast<const float*>(ws + pl.ab_off);
    a.part = reinterpret_cast<float*>(ws + pl.part_off);
    a.c = (float)std::min(1.4426950408889634 / (double)alpha, (double)FLT_MAX);
    a.N = N;
    a.W = W;
    a.Wp = pl.Wp;
    a.k = patch_size;
    a.Cp = pl.Cp;
    a.plane = (long)pl.Hp * pl.Wp;
    a.ntiles = pl.ntiles;
    a.nsplit = pl.nsplit;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nlwa_prep_kernel, dim3(cdiv(pl.Hp * pl.Wp, 256), pl.Cp + 2, B), dim3(256), 0, s, x_lab, Cx, Hx, Wx,
                       scale_xh, scale_xw, feature, C, Hf, Wf, scale_fh, scale_fw, H, W, pl.p, pl.Cp,
                       reinterpret_cast<float*>(ws + pl.fpad_off), reinterpret_cast<float*>(ws + pl.ab_off));
    DVC_CHECK_LAUNCH("dvc_nlwa_fwd(prep)");
    hipLaunchKernelGGL(nlwa_fwd_kernel, dim3(pl.nqb, pl.nsplit, B), dim3(256), 0, s, a);
    DVC_CHECK_LAUNCH("dvc_nlwa_fwd");
    hipLaunchKernelGGL(nlwa_merge_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, s, (const float*)a.part, 2 * pl.nsplit, N, a.c,
                       out);
    DVC_CHECK_LAUNCH("dvc_nlwa_fwd(merge)");
    return 0;
}
