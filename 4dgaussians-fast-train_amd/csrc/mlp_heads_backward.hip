// mlp_heads_backward.hip -- the deformation heads' second layers, backward (scene/deformation.py:73-78): the
// tall-skinny weight gradients of single Linear layers (linear_dw_kernel, gs4d_linear_dw) and the heads block's
// da / db1 / dW2 / db2 in one pass over the first layers' output (gs4d_heads_backward[_bf16]): the narrow heads
// (n <= 16) on heads_bwd_kernel / heads_bwd2_kernel, the 48-wide head on the MFMA (heads_bwd_wide_mfma_kernel,
// heads_bwd_wide_bf16_kernel), the workgroups' partials summed by heads_bwd_reduce_kernel.  The entry points,
// with the launch grouping and the scratch sizes, are at the end of the file.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {

// ---- tall-skinny weight gradients -----------------------------------------------------------------
// dW = dy^T x and db = column sums of dy for Linear layers' backward, reduced over P ~ 1e5 rows with
// n <= 64 outputs and W in {64, 128, 256} inputs -- the deformation heads' second layers, which the
// GEMM library tiles only by their small output (~55 us per call whatever n, split-K included).  Up to
// kDwMaxProblems such products (same P and W) go in one launch, blockIdx.y picking the problem.  A
// workgroup takes a contiguous block of rows; inside it G = 512 / W thread groups take interleaved
// runs of kDwUnroll rows; a thread owns column c and accumulates all n outputs: x[p, c] is one
// coalesced vector load per row, the dy row is wave-uniform (scalar loads, the FMA's SGPR operand).
// db: lane l of each group's first wave adds dy[p, l].  Groups combine through LDS in group order and
// the per-workgroup partials are summed in a fixed order by a second launch: deterministic.
constexpr int kDwMaxProblems = 8;
constexpr int kDwThreads = 512;
constexpr int kDwMaxNW = 64 * 128;  // n * W bound (LDS combine buffer)

struct DwProblem {
    const float *dy;
    const float *x;
    float *dw;
    float *db;
    int n, ld_dy, ld_x, pad;
    int64_t part_off;  // floats into the partials buffer
};
struct DwBatch {
    DwProblem q[kDwMaxProblems];
};

template <int N, bool EXACT, int kDwUnroll>
__device__ __forceinline__ void dw_block(const DwProblem &q, int P, int W, int rows_per_wg, float *__restrict__ part,
                                         float *s_red, float *s_bs) {
    const int tid = threadIdx.x;
    const int G = kDwThreads / W;
    const int g = __builtin_amdgcn_readfirstlane(tid / W);  // W is a multiple of 64: wave-uniform
    const int c = tid - g * W;
    const bool lead = __builtin_amdgcn_readfirstlane(c) == 0;  // the group's first wave
    const int n = EXACT ? N : q.n;
    const float *__restrict__ dy = q.dy;
    const float *__restrict__ x = q.x;
    const int64_t p0 = (int64_t)blockIdx.x * rows_per_wg, p1 = min((int64_t)P, p0 + rows_per_wg);
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] = 0.f;
    float bs = 0.f;
    for (int64_t p = p0 + (int64_t)g * kDwUnroll; p < p1; p += (int64_t)G * kDwUnroll) {
        float xv[kDwUnroll];
#pragma unroll
        for (int u = 0; u < kDwUnroll; u++) xv[u] = p + u < p1 ? x[(p + u) * q.ld_x + c] : 0.f;
#pragma unroll
        for (int u = 0; u < kDwUnroll; u++) {
            if (p + u < p1) {
                const float *d = dy + (p + u) * q.ld_dy;
#pragma unroll
                for (int j = 0; j < N; j++)
                    if (EXACT || j < n) acc[j] = fmaf(d[j], xv[u], acc[j]);
                if (lead && c < n) bs += d[c];
            }
        }
    }
    for (int h = 0; h < G; h++) {
        if (g == h) {
#pragma unroll
            for (int j = 0; j < N; j++)
                if (EXACT || j < n) s_red[j * W + c] = (h == 0 ? 0.f : s_red[j * W + c]) + acc[j];
            if (lead && c < n) s_bs[c] = (h == 0 ? 0.f : s_bs[c]) + bs;
        }
        __syncthreads();
    }
    float *out = part + q.part_off + (int64_t)blockIdx.x * n * (W + 1);
    for (int e = tid; e < n * (W + 1); e += kDwThreads) {
        const int r = e / (W + 1), cc = e - r * (W + 1);
        out[e] = cc < W ? s_red[r * W + cc] : s_bs[r];
    }
}

// FAMILY 0: n <= 8 (16 rows in flight per thread); FAMILY 1: n = 48 or n <= 16 (4 rows)
template <int FAMILY>
__global__ __launch_bounds__(kDwThreads) void linear_dw_kernel(DwBatch b, int P, int W, int rows_per_wg,
                                                                float *__restrict__ part) {
    __shared__ float s_red[kDwMaxNW];
    __shared__ float s_bs[64];
    const DwProblem &q = b.q[blockIdx.y];
    if constexpr (FAMILY == 0) {
        switch (q.n) {
        case 1: dw_block<1, true, 16>(q, P, W, rows_per_wg, part, s_red, s_bs); break;
        case 2: dw_block<2, true, 16>(q, P, W, rows_per_wg, part, s_red, s_bs); break;
        case 3: dw_block<3, true, 16>(q, P, W, rows_per_wg, part, s_red, s_bs); break;
        case 4: dw_block<4, true, 16>(q, P, W, rows_per_wg, part, s_red, s_bs); break;
        default: dw_block<8, false, 8>(q, P, W, rows_per_wg, part, s_red, s_bs);
        }
    } else {
        if (q.n == 48) dw_block<48, true, 4>(q, P, W, rows_per_wg, part, s_red, s_bs);
        else if (q.n <= 8) dw_block<8, false, 8>(q, P, W, rows_per_wg, part, s_red, s_bs);
        else dw_block<16, false, 4>(q, P, W, rows_per_wg, part, s_red, s_bs);
    }
}

// sum of the per-workgroup partials: 32 outputs (r, c | bias) of problem blockIdx.y per workgroup,
// 8 interleaved eighths of the workgroups combined in a fixed order
__global__ __launch_bounds__(256) void linear_dw_reduce_kernel(DwBatch b, int W, int nwg, const float *__restrict__ part) {
    __shared__ float s_sum[8][32];
    const DwProblem &q = b.q[blockIdx.y];
    const int per = q.n * (W + 1);
    if ((int)blockIdx.x * 32 >= per) return;  // uniform over the workgroup
    const int o = threadIdx.x & 31, k = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    const float *src = part + q.part_off;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;  // four independent chains: loads in flight
    if (i < per) {
        int w = k;
        for (; w + 24 < nwg; w += 32) {
            v0 += src[(size_t)w * per + i];
            v1 += src[(size_t)(w + 8) * per + i];
            v2 += src[(size_t)(w + 16) * per + i];
            v3 += src[(size_t)(w + 24) * per + i];
        }
        for (; w < nwg; w += 8) v0 += src[(size_t)w * per + i];
    }
    s_sum[k][o] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    if (k == 0 && i < per) {
        float t = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) t += s_sum[e][o];
        const int r = i / (W + 1), cc = i - r * (W + 1);
        if (cc < W) q.dw[(size_t)r * W + cc] = t;
        else if (q.db) q.db[r] = t;
    }
}

// ---- the deformation heads' second layers, backward, in one pass over the first layers' output ------
// For k heads (scene/deformation.py:73-78: ReLU -> Linear(W, W) -> ReLU -> Linear(W, n_i)) evaluated as
// one block (gs4d_train/deformation.py _DeformHeads): a = relu(h W1^T + b1) is (P, kW), head i's output
// is a[:, iW:(i+1)W] W2_i^T + b2_i.  Given the output gradients g_i (P, n_i) this forms, reading `a` once:
//   da[:, iW + c] = (a > 0) * sum_r g_i[:, r] W2_i[r, c]   (mm + threshold_backward in autograd)
//   db1 = column sums of da,  dW2_i = g_i^T a_i,  db2_i = column sums of g_i.
// A workgroup takes a block of rows; thread c owns column c of a (kW <= 768 threads, head = c / W is
// wave-uniform): its W2_i column and dW2_i accumulators stay in registers, the g_i row is wave-uniform
// (scalar loads).  Per-workgroup partials are summed in a fixed order by a second launch.
// One launch serves the heads [h0, h0 + hk) (columns h0 W .. (h0 + hk) W of a): the narrow heads and
// the 48-wide one go in separate launches, each with its own row blocking, so no workgroup waits on a
// few compute-heavy waves.
struct HbArgs {
    int P, W, k, rows_per_wg, h0, hk;
    int n[kHbMaxHeads];
    const float *w2[kHbMaxHeads];
    int poff[kHbMaxHeads + 1];  // local head i's partials: n_{h0+i} (W + 1) floats from poff[i]; poff[0] = hk W
};

// One wave's columns of head h.  The head's output-gradient rows for U rows at a time are one or a few
// coalesced vector loads (the U x n block is contiguous in g); each value reaches the FMAs as an SGPR
// through v_readlane.  The next block's loads are issued before the current block is used.  db2: the
// lead wave adds the blocks elementwise (flattened index i holds output i mod n) and folds them at the
// end in a fixed order.
// TA: the element type of a and da -- float, or __bf16 on the bf16 path (hyper.mlp_dtype = "bf16"), where
// the products still run in f32 on the bf16 values and da is rounded once when stored.
template <int N, bool EXACT, int U, class TA>
__device__ __forceinline__ void heads_bwd_cols(const HbArgs &A, int h, const TA *__restrict__ a,
                                               TA *__restrict__ da, const float *__restrict__ g,
                                               float *__restrict__ part, float *s_fold) {
    constexpr int KG = (U * N + 63) / 64;
    static_assert(EXACT || KG == 1, "runtime widths keep the block in one register");
    const int W = A.W, ld = A.k * W, hl = h - A.h0;
    const int col = A.h0 * W + threadIdx.x, c = (int)threadIdx.x - hl * W;
    const int lane = threadIdx.x & 63;
    const bool lead = c < 64;  // the head's first wave: db2 partials
    const int n = EXACT ? N : A.n[h];
    const float *__restrict__ w2 = A.w2[h];
    float w[N], acc[N];
#pragma unroll
    for (int r = 0; r < N; r++) {
        w[r] = (EXACT || r < n) ? w2[r * W + c] : 0.f;
        acc[r] = 0.f;
    }
    float gacc[KG];
#pragma unroll
    for (int k = 0; k < KG; k++) gacc[k] = 0.f;
    float csum = 0.f;
    const int64_t p0 = (int64_t)blockIdx.x * A.rows_per_wg, p1 = min((int64_t)A.P, p0 + A.rows_per_wg);
    const int64_t gend = p1 * n;
    // xn holds the raw elements: a bf16 value widened right after its (conditional) load would make the
    // compiler wait for that load inside the branch
    TA xn[U];
    float gn[KG];
    auto fetch = [&](int64_t p) {
#pragma unroll
        for (int u = 0; u < U; u++) xn[u] = p + u < p1 ? a[(p + u) * ld + col] : (TA)0.f;
#pragma unroll
        for (int k = 0; k < KG; k++) {
            const int64_t i = p * n + lane + 64 * k;
            gn[k] = (lane + 64 * k < U * n && i < gend) ? g[i] : 0.f;  // this block's U x n values only
        }
    };
    if (p0 < p1) fetch(p0);
    for (int64_t p = p0; p < p1; p += U) {
        float x[U], gv[KG];
#pragma unroll
        for (int u = 0; u < U; u++) x[u] = (float)xn[u];
#pragma unroll
        for (int k = 0; k < KG; k++) gv[k] = gn[k], gacc[k] += gn[k];
        if (p + U < p1) fetch(p + U);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (p + u < p1) {
                float sdot = 0.f;
#pragma unroll
                for (int r = 0; r < N; r++)
                    if (EXACT || r < n) {
                        const int idx = EXACT ? u * N + r : u * n + r;
                        const float dv = __builtin_bit_cast(
                            float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, gv[EXACT ? idx / 64 : 0]),
                                                             EXACT ? idx % 64 : idx));
                        sdot = fmaf(dv, w[r], sdot);
                        acc[r] = fmaf(dv, x[u], acc[r]);
                    }
                const float gvv = x[u] > 0.f ? sdot : 0.f;
                da[(p + u) * ld + col] = (TA)gvv;
                csum += gvv;
            }
        }
    }
    float *pw = part + (size_t)blockIdx.x * A.poff[A.hk];
    pw[threadIdx.x] = csum;
    float *ph = pw + A.poff[hl];
#pragma unroll
    for (int r = 0; r < N; r++)
        if (EXACT || r < n) ph[r * (W + 1) + c] = acc[r];
    if (lead) {
        // fold the flattened block sums: output r = sum over flattened indices i with i mod n == r
        float *f = s_fold + (threadIdx.x >> 6) * 64 * KG;
#pragma unroll
        for (int k = 0; k < KG; k++) f[lane + 64 * k] = gacc[k];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane < n) {
            float t = 0.f;
            for (int i = lane; i < 64 * KG; i += n) t += f[i];
            ph[lane * (W + 1) + W] = t;
        }
    }
}

template <class TA>
__global__ __launch_bounds__(768) void heads_bwd_kernel(HbArgs A, const TA *__restrict__ a, TA *__restrict__ da,
                                                         const float *__restrict__ g0, const float *__restrict__ g1,
                                                         const float *__restrict__ g2, const float *__restrict__ g3,
                                                         const float *__restrict__ g4, const float *__restrict__ g5,
                                                         const float *__restrict__ g6, const float *__restrict__ g7,
                                                         float *__restrict__ part) {
    __shared__ float s_fold[16 * 64];  // per wave: the lead waves' flattened db2 block sums
    const int h = A.h0 + __builtin_amdgcn_readfirstlane((int)threadIdx.x / A.W);
    const float *__restrict__ g = h == 0 ? g0 : h == 1 ? g1 : h == 2 ? g2 : h == 3 ? g3 : h == 4 ? g4 : h == 5 ? g5
                                : h == 6 ? g6 : g7;
    switch (A.n[h]) {
    case 1: heads_bwd_cols<1, true, 8, TA>(A, h, a, da, g, part, s_fold); break;
    case 2: heads_bwd_cols<2, true, 8, TA>(A, h, a, da, g, part, s_fold); break;
    case 3: heads_bwd_cols<3, true, 8, TA>(A, h, a, da, g, part, s_fold); break;
    case 4: heads_bwd_cols<4, true, 8, TA>(A, h, a, da, g, part, s_fold); break;
    default:
        if (A.n[h] <= 8) heads_bwd_cols<8, false, 8, TA>(A, h, a, da, g, part, s_fold);
        else heads_bwd_cols<16, false, 4, TA>(A, h, a, da, g, part, s_fold);
    }
}

// The bf16 form with two columns per thread (W a multiple of 128: a head is whole waves of W / 2 threads):
// a and da move as bf16 pairs (4-byte loads and stores, half the memory instructions of one column per
// thread), the products and sums as in heads_bwd_cols, column by column.
typedef __attribute__((ext_vector_type(2))) __bf16 bf2v;
template <int N, bool EXACT, int U>
__device__ __forceinline__ void heads_bwd_cols2(const HbArgs &A, int h, const __bf16 *__restrict__ a,
                                                __bf16 *__restrict__ da, const float *__restrict__ g,
                                                float *__restrict__ part, float *s_fold) {
    constexpr int KG = (U * N + 63) / 64;
    static_assert(EXACT || KG == 1, "runtime widths keep the block in one register");
    const int W = A.W, ld = A.k * W, hl = h - A.h0;
    const int c = 2 * ((int)threadIdx.x - hl * (W / 2));  // this thread's first column in the head
    const int col = (A.h0 + hl) * W + c;
    const int lane = threadIdx.x & 63;
    const bool lead = c < 128;  // the head's first wave: db2 partials
    const int n = EXACT ? N : A.n[h];
    const float *__restrict__ w2 = A.w2[h];
    float w0[N], w1[N], acc0[N], acc1[N];
#pragma unroll
    for (int r = 0; r < N; r++) {
        const float2 wv = (EXACT || r < n) ? *reinterpret_cast<const float2 *>(w2 + r * W + c) : make_float2(0.f, 0.f);
        w0[r] = wv.x, w1[r] = wv.y;
        acc0[r] = acc1[r] = 0.f;
    }
    float gacc[KG];
#pragma unroll
    for (int k = 0; k < KG; k++) gacc[k] = 0.f;
    float csum0 = 0.f, csum1 = 0.f;
    const int64_t p0 = (int64_t)blockIdx.x * A.rows_per_wg, p1 = min((int64_t)A.P, p0 + A.rows_per_wg);
    const int64_t gend = p1 * n;
    bf2v xn[U];  // raw pairs until use (see heads_bwd_cols)
    float gn[KG];
    auto fetch = [&](int64_t p) {
#pragma unroll
        for (int u = 0; u < U; u++)
            xn[u] = p + u < p1 ? *reinterpret_cast<const bf2v *>(a + (p + u) * ld + col) : bf2v{(__bf16)0.f, (__bf16)0.f};
#pragma unroll
        for (int k = 0; k < KG; k++) {
            const int64_t i = p * n + lane + 64 * k;
            gn[k] = (lane + 64 * k < U * n && i < gend) ? g[i] : 0.f;
        }
    };
    if (p0 < p1) fetch(p0);
    for (int64_t p = p0; p < p1; p += U) {
        float x0[U], x1[U], gv[KG];
#pragma unroll
        for (int u = 0; u < U; u++) x0[u] = (float)xn[u][0], x1[u] = (float)xn[u][1];
#pragma unroll
        for (int k = 0; k < KG; k++) gv[k] = gn[k], gacc[k] += gn[k];
        if (p + U < p1) fetch(p + U);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (p + u < p1) {
                float sd0 = 0.f, sd1 = 0.f;
#pragma unroll
                for (int r = 0; r < N; r++)
                    if (EXACT || r < n) {
                        const int idx = EXACT ? u * N + r : u * n + r;
                        const float dv = __builtin_bit_cast(
                            float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, gv[EXACT ? idx / 64 : 0]),
                                                             EXACT ? idx % 64 : idx));
                        sd0 = fmaf(dv, w0[r], sd0);
                        sd1 = fmaf(dv, w1[r], sd1);
                        acc0[r] = fmaf(dv, x0[u], acc0[r]);
                        acc1[r] = fmaf(dv, x1[u], acc1[r]);
                    }
                const float g0 = x0[u] > 0.f ? sd0 : 0.f, g1 = x1[u] > 0.f ? sd1 : 0.f;
                *reinterpret_cast<bf2v *>(da + (p + u) * ld + col) = bf2v{(__bf16)g0, (__bf16)g1};
                csum0 += g0;
                csum1 += g1;
            }
        }
    }
    float *pw = part + (size_t)blockIdx.x * A.poff[A.hk];
    pw[hl * W + c] = csum0;
    pw[hl * W + c + 1] = csum1;
    float *ph = pw + A.poff[hl];
#pragma unroll
    for (int r = 0; r < N; r++)
        if (EXACT || r < n) ph[r * (W + 1) + c] = acc0[r], ph[r * (W + 1) + c + 1] = acc1[r];
    if (lead) {
        float *f = s_fold + (threadIdx.x >> 6) * 64 * KG;
#pragma unroll
        for (int k = 0; k < KG; k++) f[lane + 64 * k] = gacc[k];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane < n) {
            float t = 0.f;
            for (int i = lane; i < 64 * KG; i += n) t += f[i];
            ph[lane * (W + 1) + W] = t;
        }
    }
}

__global__ __launch_bounds__(512) void heads_bwd2_kernel(HbArgs A, const __bf16 *__restrict__ a, __bf16 *__restrict__ da,
                                                        const float *__restrict__ g0, const float *__restrict__ g1,
                                                        const float *__restrict__ g2, const float *__restrict__ g3,
                                                        const float *__restrict__ g4, const float *__restrict__ g5,
                                                        const float *__restrict__ g6, const float *__restrict__ g7,
                                                        float *__restrict__ part) {
    __shared__ float s_fold[8 * 64];
    const int h = A.h0 + __builtin_amdgcn_readfirstlane((int)threadIdx.x / (A.W / 2));
    const float *__restrict__ g = h == 0 ? g0 : h == 1 ? g1 : h == 2 ? g2 : h == 3 ? g3 : h == 4 ? g4 : h == 5 ? g5
                                : h == 6 ? g6 : g7;
    switch (A.n[h]) {
    case 1: heads_bwd_cols2<1, true, 8>(A, h, a, da, g, part, s_fold); break;
    case 2: heads_bwd_cols2<2, true, 8>(A, h, a, da, g, part, s_fold); break;
    case 3: heads_bwd_cols2<3, true, 8>(A, h, a, da, g, part, s_fold); break;
    case 4: heads_bwd_cols2<4, true, 8>(A, h, a, da, g, part, s_fold); break;
    default:
        if (A.n[h] <= 8) heads_bwd_cols2<8, false, 8>(A, h, a, da, g, part, s_fold);
        else heads_bwd_cols2<16, false, 4>(A, h, a, da, g, part, s_fold);
    }
}

// The wide head (n = 48: the SH-coefficient deformation) is compute-bound rather than streaming (96 FMAs per
// row and column), so it runs on the f32 MFMA (v_mfma_f32_16x16x4_f32), for W in {64, 128} and N a multiple
// of 16: a wave takes 16-row blocks and forms
//   da (16 x W) = (a > 0) * (g (16 x N) W2 (N x W)):  lane group q = l >> 4 reads columns 4q..4q+3 of its
//       g row l & 15 per 16-column K chunk as one float4 (k index of step s = column 4q + s); W2^T in LDS
//       (row stride N + 4) is the B operand;
//   dW2 (N x W) += g^T a:  K = the 16 rows, lane group q takes rows 4q..4q+3 (k index of step s = row
//       4q + s), so the a values it needs are exactly the ones the da mask reads at the C positions
//       (rows 4q + j, columns 16t + c): loaded once, used twice;
//   db1 (column sums of da) and db2 (column sums of g) on the way.
// The waves' partials are added in wave order in LDS, the workgroups' by heads_bwd_reduce_kernel.  A
// workgroup's partial is HbArgs::poff's layout for a launch of one head (hk = 1): db1 (W floats), then for
// each output r its row of dW2 (W floats) followed by db2[r] -- W + N (W + 1) floats in all.
template <int W, int N, class TA>
__global__ __launch_bounds__(256) void heads_bwd_wide_mfma_kernel(HbArgs A, const TA *__restrict__ a,
                                                                   TA *__restrict__ da,
                                                                   const float *__restrict__ g,
                                                                   float *__restrict__ part) {
    // each wave takes half of the head's W columns (CT tiles of 16) of a row block: waves 2i and 2i + 1
    // share block i's rows; only the first half accumulates db2 (g's column sums)
    constexpr int CT = W / 32, MT = N / 16, NKC = N / 16, WS = N + 4, NWV = 4;
    constexpr int PER = W + N * (W + 1);  // partial: db1 (W) then for each output r: dW2[r][0..W), db2[r]
    __shared__ float s_w2t[W * WS];
    __shared__ float s_red[PER];
    const int ld = A.k * W, h = A.h0;
    const float *__restrict__ w2 = A.w2[h];
    for (int e = threadIdx.x; e < N * W; e += 256) {  // W2 (N x W) -> W2^T rows
        const int r = e / W, col = e % W;
        s_w2t[col * WS + r] = w2[e];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4, c = lane & 15;
    const int half = wv & 1, cb = half * (W / 2);  // this wave's first column
    f4v accw[MT][CT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int t = 0; t < CT; t++) accw[m][t] = f4v{0.f, 0.f, 0.f, 0.f};
    float csum[CT], bsum[MT];
#pragma unroll
    for (int t = 0; t < CT; t++) csum[t] = 0.f;
#pragma unroll
    for (int m = 0; m < MT; m++) bsum[m] = 0.f;
    const int P = A.P, nblk = (P + 15) / 16;
    const TA *acol = a + h * W + cb;
    TA *dacol = da + h * W + cb;
    // a block's loads: g rows as the da A operand, g at (row 4q + s, output 16m + c) as the dW2 A operand,
    // a at the C positions (row 4q + j, column 16t + c); issued one block ahead of their use
    float4 gA[NKC];
    float gT[MT][4];
    TA av[CT][4];  // raw elements, widened when the block comes up (see heads_bwd_cols)
    // rows past P (and the prefetch past the last block) read row P - 1: the loads are unconditional, so
    // the compiler's waits count exactly the loads issued after a block's (a branch around them made it wait
    // for every load in flight, the next block's prefetch included); such rows are masked when the block
    // comes up
    auto load_block = [&](int blk) {
        const int r0 = blk * 16, rg = min(r0 + c, P - 1);
#pragma unroll
        for (int kc = 0; kc < NKC; kc++) gA[kc] = *reinterpret_cast<const float4 *>(g + (size_t)rg * N + 16 * kc + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = min(r0 + 4 * q + j, P - 1);
#pragma unroll
            for (int m = 0; m < MT; m++) gT[m][j] = g[(size_t)r * N + 16 * m + c];
#pragma unroll
            for (int t = 0; t < CT; t++) av[t][j] = acol[(size_t)r * ld + 16 * t + c];
        }
    };
    const int stride = gridDim.x * (NWV / 2);
    int blk = blockIdx.x * (NWV / 2) + (wv >> 1);
    load_block(blk);
    for (; blk < nblk; blk += stride) {
        const int r0 = blk * 16;
        float4 gAc[NKC];
        float gTc[MT][4], avc[CT][4];
#pragma unroll
        for (int kc = 0; kc < NKC; kc++) gAc[kc] = gA[kc];  // rows past P: da rows neither stored nor summed
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = r0 + 4 * q + j < P;
#pragma unroll
            for (int m = 0; m < MT; m++) gTc[m][j] = ok ? gT[m][j] : 0.f;
#pragma unroll
            for (int t = 0; t < CT; t++) avc[t][j] = ok ? (float)av[t][j] : 0.f;
        }
        load_block(blk + stride);
        // da
#pragma unroll
        for (int t = 0; t < CT; t++) {
            f4v acc = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < NKC; kc++) {
                const float4 bv = *reinterpret_cast<const float4 *>(s_w2t + (cb + 16 * t + c) * WS + 16 * kc + 4 * q);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(gAc[kc].x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(gAc[kc].y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(gAc[kc].z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(gAc[kc].w, bv.w, acc, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = r0 + 4 * q + j;
                const float v = avc[t][j] > 0.f ? acc[j] : 0.f;
                if (r < P) dacol[(size_t)r * ld + 16 * t + c] = (TA)v;
                csum[t] += v;
            }
        }
        // dW2 += g^T a, db2
#pragma unroll
        for (int m = 0; m < MT; m++) {
#pragma unroll
            for (int j = 0; j < 4; j++) bsum[m] += gTc[m][j];
#pragma unroll
            for (int t = 0; t < CT; t++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    accw[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(gTc[m][j], avc[t][j], accw[m][t], 0, 0, 0);
        }
    }
    // wave partials -> LDS: the two halves' column ranges are disjoint; waves of the same half are
    // added in wave order (accw C layout: row = output 16m + 4q + j, column cb + 16t + c); db1 / db2: the
    // 4 lane groups (q) of a column added in q order; db2 from the first half only
    for (int qw = 0; qw < NWV; qw++) {
        __syncthreads();
        if (wv == qw) {
            const bool first = qw < 2;  // the first wave of this half
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int t = 0; t < CT; t++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        float &d = s_red[W + (16 * m + 4 * q + j) * (W + 1) + cb + 16 * t + c];
                        d = first ? accw[m][t][j] : d + accw[m][t][j];
                    }
            for (int qq = 0; qq < 4; qq++) {
                if (q == qq) {
#pragma unroll
                    for (int t = 0; t < CT; t++) {
                        float &d = s_red[cb + 16 * t + c];
                        d = (first && qq == 0) ? csum[t] : d + csum[t];
                    }
                    if (half == 0) {
#pragma unroll
                        for (int m = 0; m < MT; m++) {
                            float &d = s_red[W + (16 * m + c) * (W + 1) + W];
                            d = (first && qq == 0) ? bsum[m] : d + bsum[m];
                        }
                    }
                }
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __syncthreads();
    float *pw = part + (size_t)blockIdx.x * PER;
    for (int i = threadIdx.x; i < PER; i += 256) pw[i] = s_red[i];
}

// ---- the wide head's second-layer backward on the bf16 path (n = 48, W = 128): heads_bwd_wide_mfma_kernel's
// products on v_mfma_f32_16x16x32_bf16 with g rounded to bf16 (the bf16 leg's operands), sums in fp32.  A
// workgroup takes 32-row steps (grid-stride): the a tile (32 x 128 bf16) and the g tile (32 x 48 -> bf16,
// columns 48..63 zero) are staged in LDS (the swizzled 256-byte rows of mlp_dw_bf16_kernel), W2^T (128 x 64
// bf16, zero-padded k) once per workgroup.
//   da^T = W2^T g^T: A = W2^T rows (LDS row reads), B = g rows (LDS row reads), D = 4 consecutive columns of one
//        row per lane: masked by a > 0 and stored as 8 bytes; db1 summed from the fp32 results;
//   dW2 += g^T a: both operands by ds_read_b64_tr_b16 (K = the 32 rows);
//   db2: the fp32 g values summed as staged.
// Partials in heads_bwd_reduce_kernel's layout (fixed-order sums: deterministic).
__global__ __launch_bounds__(256) void heads_bwd_wide_bf16_kernel(HbArgs A, const __bf16 *__restrict__ a,
                                                                  __bf16 *__restrict__ da, const float *__restrict__ g,
                                                                  float *__restrict__ part) {
    constexpr int W = 128, N = 48, KS = 72;  // W2^T row stride (bf16): 64 + 8 (144 B)
    __shared__ __attribute__((aligned(16))) __bf16 s_w2t[W * KS];
    __shared__ __attribute__((aligned(16))) unsigned char s_ta[32 * 256], s_tg[32 * 256];
    __shared__ float4 s_red[192];
    const int ld = A.k * W, h = A.h0;
    const float *__restrict__ w2 = A.w2[h];
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4, c = lane & 15;
    for (int e = threadIdx.x; e < W * 64; e += 256) {
        const int n = e / 64, k = e % 64;
        s_w2t[n * KS + k] = (__bf16)(k < N ? w2[k * W + n] : 0.f);
    }
    for (int e = threadIdx.x; e < 32 * 10; e += 256) {  // g tile chunks 6..15 stay zero
        const int row = e / 10, ch = 6 + e % 10;
        *reinterpret_cast<bf8v *>(&s_tg[dwb_off(row, ch)]) = bf8v{};
    }
    f4v accw[3][2];
#pragma unroll
    for (int m = 0; m < 3; m++) accw[m][0] = accw[m][1] = f4v{0.f, 0.f, 0.f, 0.f};
    float4 dsum[2][2];  // [n local][row block]: this lane's da column sums (4 columns)
#pragma unroll
    for (int i = 0; i < 2; i++) dsum[i][0] = dsum[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gsum = make_float4(0.f, 0.f, 0.f, 0.f);  // threads < 192: fp32 column sums of g, columns 4 (t % 12) ..
    const int P = A.P, nb32 = (P + 31) / 32;
    for (int blk = blockIdx.x; blk < nb32; blk += gridDim.x) {
        const int64_t r0 = (int64_t)blk * 32;
        // stage the a tile (512 16-byte chunks, two per thread) and the g tile (384 float4, two per thread < 192)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int e = threadIdx.x + 256 * i, row = e >> 4, ch = e & 15;
            const int64_t pr = r0 + row;
            bf8v v = bf8v{};
            if (pr < P) v = *reinterpret_cast<const bf8v *>(a + (size_t)pr * ld + h * W + 8 * ch);
            *reinterpret_cast<bf8v *>(&s_ta[dwb_off(row, ch)]) = v;
        }
        if (threadIdx.x < 192) {
            const int c4 = threadIdx.x % 12;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int row = threadIdx.x / 12 + 16 * i;
                const int64_t pr = r0 + row;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pr < P) v = *reinterpret_cast<const float4 *>(g + (size_t)pr * N + 4 * c4);
                gsum.x += v.x; gsum.y += v.y; gsum.z += v.z; gsum.w += v.w;
                *reinterpret_cast<bf4v *>(&s_tg[dwb_off(row, c4 >> 1) + 8 * (c4 & 1)]) =
                    bf4v{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
            }
        }
        __syncthreads();
        // da^T: wave wv takes columns tiles n = 2 wv, 2 wv + 1 for both 16-row blocks
#pragma unroll
        for (int nl = 0; nl < 2; nl++) {
            const int n = 2 * wv + nl;
#pragma unroll
            for (int rb = 0; rb < 2; rb++) {
                f4v d = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 2; st++) {
                    const bf8v wa = *reinterpret_cast<const bf8v *>(&s_w2t[(16 * n + c) * KS + 32 * st + 8 * q]);
                    const bf8v gb = *reinterpret_cast<const bf8v *>(&s_tg[dwb_off(16 * rb + c, 4 * st + q)]);
                    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, gb, d, 0, 0, 0);
                }
                // D[column 16 n + 4 q + r][row 16 rb + c]
                const int row = 16 * rb + c;
                const bf4v av = *reinterpret_cast<const bf4v *>(&s_ta[dwb_off(row, 2 * n + (q >> 1)) + 8 * (q & 1)]);
                const float v0 = (float)av[0] > 0.f ? d[0] : 0.f, v1 = (float)av[1] > 0.f ? d[1] : 0.f;
                const float v2 = (float)av[2] > 0.f ? d[2] : 0.f, v3 = (float)av[3] > 0.f ? d[3] : 0.f;
                if (r0 + row < P) {
                    *reinterpret_cast<bf4v *>(da + (size_t)(r0 + row) * ld + h * W + 16 * n + 4 * q) =
                        bf4v{(__bf16)v0, (__bf16)v1, (__bf16)v2, (__bf16)v3};
                    dsum[nl][rb].x += v0; dsum[nl][rb].y += v1; dsum[nl][rb].z += v2; dsum[nl][rb].w += v3;
                }
            }
        }
        // dW2 += g^T a: tiles (m = 0..2, n = 2 wv, 2 wv + 1), K = the 32 rows
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const bf8v ga = dwb_tr_frag(s_tg, 0, q, c, 2 * m);
#pragma unroll
            for (int nl = 0; nl < 2; nl++) {
                const bf8v ab = dwb_tr_frag(s_ta, 0, q, c, 2 * (2 * wv + nl));
                accw[m][nl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga, ab, accw[m][nl], 0, 0, 0);
            }
        }
        __syncthreads();  // the tiles are restaged by the next step
    }
    float *pw = part + (size_t)blockIdx.x * (W + N * (W + 1));
    // db1: the 16 lanes of a lane group (rows) summed by a fixed butterfly, both row blocks in order
#pragma unroll
    for (int nl = 0; nl < 2; nl++) {
        float4 t = make_float4(dsum[nl][0].x + dsum[nl][1].x, dsum[nl][0].y + dsum[nl][1].y,
                               dsum[nl][0].z + dsum[nl][1].z, dsum[nl][0].w + dsum[nl][1].w);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            t.x += __shfl_xor(t.x, off, 16); t.y += __shfl_xor(t.y, off, 16);
            t.z += __shfl_xor(t.z, off, 16); t.w += __shfl_xor(t.w, off, 16);
        }
        if (c == 0) {
            const int col = 16 * (2 * wv + nl) + 4 * q;
            pw[col] = t.x, pw[col + 1] = t.y, pw[col + 2] = t.z, pw[col + 3] = t.w;
        }
    }
    // dW2: D[output 16 m + 4 q + r][column 16 n + c]
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int nl = 0; nl < 2; nl++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                pw[W + (16 * m + 4 * q + r) * (W + 1) + 16 * (2 * wv + nl) + c] = accw[m][nl][r];
    // db2: the 16 threads of each column group summed in thread order
    if (threadIdx.x < 192) s_red[threadIdx.x] = gsum;
    __syncthreads();
    if (threadIdx.x < 12) {
        float4 t = s_red[threadIdx.x];
        for (int j = 1; j < 16; j++) {
            const float4 v = s_red[threadIdx.x + 12 * j];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        const int o = 4 * threadIdx.x;
        pw[W + (o + 0) * (W + 1) + W] = t.x;
        pw[W + (o + 1) * (W + 1) + W] = t.y;
        pw[W + (o + 2) * (W + 1) + W] = t.z;
        pw[W + (o + 3) * (W + 1) + W] = t.w;
    }
}

// the partials summed over the workgroups (32 record entries per workgroup, 8 eighths in a fixed
// order) and routed to db1 / dW2_i / db2_i
struct HbOut {
    float *db1;
    float *dw2[kHbMaxHeads];
    float *db2[kHbMaxHeads];
};
// 16 outputs per workgroup (16 interleaved sixteenths of the workgroups each, combined in a fixed order): the
// ~2k outputs of a launch then fill ~120 CUs instead of ~60
constexpr int kHbRedOut = 16, kHbRedSlices = 256 / kHbRedOut;
// One launch reduces the partials of up to kHbRedGroups launch groups (the narrow heads' and the wide head's):
// group g owns workgroups [blk0[g], blk0[g + 1]).
constexpr int kHbRedGroups = 2;
struct HbRed {
    HbArgs A[kHbRedGroups];
    const float *part[kHbRedGroups];
    int nwg[kHbRedGroups];
    int blk0[kHbRedGroups + 1];
    int count;
};
__global__ __launch_bounds__(256) void heads_bwd_reduce_kernel(HbRed R, HbOut O) {
    __shared__ float s_sum[kHbRedSlices][kHbRedOut];
    int gi = 0;
    while (gi + 1 < R.count && (int)blockIdx.x >= R.blk0[gi + 1]) gi++;
    const HbArgs &A = R.A[gi];
    const float *__restrict__ part = R.part[gi];
    const int nwg = R.nwg[gi];
    const int per = A.poff[A.hk];
    const int o = threadIdx.x % kHbRedOut, q = threadIdx.x / kHbRedOut;
    const int i = ((int)blockIdx.x - R.blk0[gi]) * kHbRedOut + o;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (i < per) {
        int w = q;
        constexpr int K = kHbRedSlices;
        for (; w + 7 * K < nwg; w += 8 * K) {  // eight loads in flight per thread (the kernel is latency-bound)
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = part[(size_t)(w + u * K) * per + i];
            v0 += x[0]; v1 += x[1]; v2 += x[2]; v3 += x[3];
            v0 += x[4]; v1 += x[5]; v2 += x[6]; v3 += x[7];
        }
        for (; w + 3 * K < nwg; w += 4 * K) {
            v0 += part[(size_t)w * per + i];
            v1 += part[(size_t)(w + K) * per + i];
            v2 += part[(size_t)(w + 2 * K) * per + i];
            v3 += part[(size_t)(w + 3 * K) * per + i];
        }
        for (; w < nwg; w += K) v0 += part[(size_t)w * per + i];
    }
    s_sum[q][o] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    if (q == 0 && i < per) {
        float t = 0.f;
#pragma unroll
        for (int e = 0; e < kHbRedSlices; e++) t += s_sum[e][o];
        if (i < A.poff[0]) {
            O.db1[A.h0 * A.W + i] = t;
        } else {
            int hl = 0;
            while (hl + 1 < A.hk && i >= A.poff[hl + 1]) hl++;
            const int e = i - A.poff[hl], r = e / (A.W + 1), c = e - r * (A.W + 1);
            if (c < A.W) O.dw2[A.h0 + hl][r * A.W + c] = t;
            else O.db2[A.h0 + hl][r] = t;
        }
    }
}

static int dw_rows_per_wg(int P, int nmax) {
    // enough workgroups to cover the chip, few enough that the partials stay small next to x
    (void)P;
    return nmax <= 8 ? 256 : 1024;
}

}  // namespace gs4d

using namespace gs4d;

extern "C" {

// the launches: maximal runs of heads of one class (narrow: n <= 16; wide: n = 48)
static bool hb_wide(int n) { return n > 16; }  // n = 48 (validated), one head per launch
static bool hb_mfma(int W, int n) { return (W == 64 || W == 128) && n == 48; }  // the wide head's MFMA kernels
static int hb_rows_per_wg(int P, bool wide, bool bf) {
    // narrow heads stream a: about two (fp32) or four (bf16: half the bytes per row) workgroups per CU; the wide
    // head's waves are compute-heavy and its per-workgroup partials large (9 KB per block of rows): 512-row
    // blocks on the fp32 MFMA kernel, 256 on the bf16 one (tools/ab_heads.sh at P = 100k: the fp32 heads
    // backward 160 -> 148 us, the bf16 one 106 -> 97 us against 128-row blocks and P / 512 narrow rows)
    if (wide) return bf ? 256 : 512;
    return bf ? std::max(64, (P + 1023) / 1024) : std::max(64, (P + 511) / 512);
}
extern "C++" {
template <class Fn>
static void hb_groups(int k, const int *n, Fn fn) {  // fn(h0, hk)
    for (int h0 = 0; h0 < k;) {
        int h1 = h0 + 1;
        while (h1 < k && !hb_wide(n[h0]) && !hb_wide(n[h1])) h1++;
        fn(h0, h1 - h0);
        h0 = h1;
    }
}
}

size_t gs4d_heads_backward_scratch_bytes(int P, int W, int k, const int *n) {
    if (P < 0 || W < 1 || k < 1 || k > kHbMaxHeads || !n) return 0;
    size_t total = 256;
    hb_groups(k, n, [&](int h0, int hk) {
        size_t per = (size_t)hk * W;
        for (int i = h0; i < h0 + hk; i++) per += (size_t)std::max(n[i], 0) * (W + 1);
        // one size for both element types: the smaller row block (more workgroups, more partials)
        const int rows = std::min(hb_rows_per_wg(P, hb_wide(n[h0]), false), hb_rows_per_wg(P, hb_wide(n[h0]), true));
        const size_t nwg = std::max<size_t>(1, ((size_t)P + rows - 1) / rows);
        total += align_up(4 * nwg * per, 256);
    });
    return total;
}

extern "C++" {
template <class TA, class Args>
static int heads_backward_t(const Args *args, void *scratch, void *stream) {
    if (!args || !scratch) return 1;
    const Args &b = *args;
    const TA *ba = reinterpret_cast<const TA *>(b.a);
    TA *bda = reinterpret_cast<TA *>(b.da);
    if (b.P < 0 || (b.W != 64 && b.W != 128 && b.W != 256) || b.k < 1 || b.k > kHbMaxHeads || b.k * b.W > 768 ||
        !b.db1)
        return 1;
    if (b.P > 0 && (!b.a || !b.da)) return 1;
    HbArgs A{};
    HbOut O{};
    A.P = b.P, A.W = b.W, A.k = b.k;
    const float *g[kHbMaxHeads] = {};
    for (int i = 0; i < b.k; i++) {
        if (b.n[i] < 1 || (b.n[i] > 16 && b.n[i] != 48) || !b.w2[i] || !b.dw2[i] || !b.db2[i] || (b.P > 0 && !b.g[i]))
            return 1;
        if (b.n[i] == 48 && (((size_t)b.g[i] & 15) || b.W > 128)) return 1;  // rows read as float4; W in {64, 128}
        A.n[i] = b.n[i], A.w2[i] = b.w2[i], g[i] = b.g[i];
        O.dw2[i] = b.dw2[i], O.db2[i] = b.db2[i];
    }
    O.db1 = b.db1;
    hipStream_t s = (hipStream_t)stream;
    char *q = (char *)align_up((size_t)scratch, 256);
    int err = 0;
    HbRed R{};
    auto flush = [&]() {  // the pending groups' reduction, one launch
        if (!R.count) return;
        hipLaunchKernelGGL(heads_bwd_reduce_kernel, dim3(R.blk0[R.count]), dim3(256), 0, s, R, O);
        R = HbRed{};
    };
    hb_groups(b.k, b.n, [&](int h0, int hk) {
        A.h0 = h0, A.hk = hk;
        A.rows_per_wg = hb_rows_per_wg(b.P, hb_wide(b.n[h0]), std::is_same<TA, __bf16>::value);
        A.poff[0] = hk * b.W;
        for (int i = 0; i < hk; i++) A.poff[i + 1] = A.poff[i] + b.n[h0 + i] * (b.W + 1);
        const int nwg = std::max(1, (int)(((int64_t)b.P + A.rows_per_wg - 1) / A.rows_per_wg));
        float *part = (float *)q;
        q += align_up(4 * (size_t)nwg * A.poff[hk], 256);
        if (b.P == 0) {  // empty sums: the partials of one empty workgroup
            if (hipMemsetAsync(part, 0, 4 * (size_t)A.poff[hk], s) != hipSuccess) err = 3;
        } else {
            if (hb_wide(b.n[h0]) && hb_mfma(b.W, b.n[h0])) {
                // bf16 at W = 128 has a kernel of its own (the f32-MFMA one is not instantiated for it)
                if (b.W == 64)
                    hipLaunchKernelGGL((heads_bwd_wide_mfma_kernel<64, 48, TA>), dim3(nwg), dim3(256), 0, s, A, ba, bda,
                                       g[h0], part);
                else if constexpr (std::is_same<TA, __bf16>::value)
                    hipLaunchKernelGGL(heads_bwd_wide_bf16_kernel, dim3(nwg), dim3(256), 0, s, A, ba, bda, g[h0], part);
                else
                    hipLaunchKernelGGL((heads_bwd_wide_mfma_kernel<128, 48, TA>), dim3(nwg), dim3(256), 0, s, A, ba,
                                       bda, g[h0], part);
            } else if (hb_wide(b.n[h0])) {
                err = 1;  // unreachable while the checks above hold: a wide head never falls to a narrow kernel
            } else if (std::is_same<TA, __bf16>::value && b.W % 128 == 0 && hk * b.W <= 1024)
                hipLaunchKernelGGL(heads_bwd2_kernel, dim3(nwg), dim3(hk * b.W / 2), 0, s, A, (const __bf16 *)ba,
                                   (__bf16 *)bda, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], part);
            else
                hipLaunchKernelGGL(heads_bwd_kernel<TA>, dim3(nwg), dim3(hk * b.W), 0, s, A, ba, bda, g[0], g[1], g[2],
                                   g[3], g[4], g[5], g[6], g[7], part);
        }
        if (R.count == kHbRedGroups) flush();
        R.A[R.count] = A, R.part[R.count] = part, R.nwg[R.count] = nwg;
        R.blk0[R.count + 1] = R.blk0[R.count] + (A.poff[hk] + kHbRedOut - 1) / kHbRedOut;
        R.count++;
    });
    flush();
    if (err) return err;
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
}

int gs4d_heads_backward(const gs4d_heads_bwd *args, void *scratch, void *stream) {
    return heads_backward_t<float>(args, scratch, stream);
}

int gs4d_heads_backward_bf16(const gs4d_heads_bwd_bf16 *args, void *scratch, void *stream) {
    if (args)
        for (int i = 0; i < args->k && i < kHbMaxHeads; i++)
            if (hb_wide(args->n[i]) && !hb_mfma(args->W, args->n[i])) return 1;
    return heads_backward_t<__bf16>(args, scratch, stream);
}

size_t gs4d_linear_dw_scratch_bytes(int P, int W, int count, const int *n) {
    if (P < 0 || W < 1 || count < 1 || count > kDwMaxProblems || !n) return 0;
    int nmax = 0, nsum = 0;
    for (int i = 0; i < count; i++) nmax = std::max(nmax, n[i]), nsum += std::max(n[i], 0);
    const size_t nwg = std::max<size_t>(1, ((size_t)P + dw_rows_per_wg(P, nmax) - 1) / dw_rows_per_wg(P, nmax));
    return 4 * nwg * (size_t)nsum * (W + 1) + 256;
}

int gs4d_linear_dw(int P, int W, int count, const gs4d_dw_problem *problems, void *scratch, void *stream) {
    if (P < 0 || (W != 64 && W != 128 && W != 256) || count < 1 || count > kDwMaxProblems || !problems || !scratch)
        return 1;
    DwBatch b{};
    int nmax = 0, nsum = 0;
    for (int i = 0; i < count; i++) {
        const gs4d_dw_problem &p = problems[i];
        if (p.n < 1 || (p.n > 16 && p.n != 48) || p.n * W > kDwMaxNW || (P > 0 && (!p.dy || !p.x)) || !p.dw || p.ld_dy < p.n || p.ld_x < W)
            return 1;
        nmax = std::max(nmax, p.n);
        b.q[i] = DwProblem{p.dy, p.x, p.dw, p.db, p.n, p.ld_dy, p.ld_x, 0, 0};
    }
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        for (int i = 0; i < count; i++) {
            if (hipMemsetAsync(b.q[i].dw, 0, 4 * (size_t)b.q[i].n * W, s) != hipSuccess) return 3;
            if (b.q[i].db && hipMemsetAsync(b.q[i].db, 0, 4 * (size_t)b.q[i].n, s) != hipSuccess) return 3;
        }
        return 0;
    }
    const int rows = dw_rows_per_wg(P, nmax);
    const int nwg = (int)(((int64_t)P + rows - 1) / rows);
    for (int i = 0; i < count; i++) b.q[i].part_off = (int64_t)nwg * nsum * (W + 1), nsum += b.q[i].n;
    float *part = (float *)align_up((size_t)scratch, 256);
    if (nmax <= 8) hipLaunchKernelGGL(linear_dw_kernel<0>, dim3(nwg, count), dim3(kDwThreads), 0, s, b, P, W, rows, part);
    else hipLaunchKernelGGL(linear_dw_kernel<1>, dim3(nwg, count), dim3(kDwThreads), 0, s, b, P, W, rows, part);
    hipLaunchKernelGGL(linear_dw_reduce_kernel, dim3((nmax * (W + 1) + 31) / 32, count), dim3(256), 0, s, b, W, nwg,
                       (const float *)part);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // extern "C"
