// mlp_gemm.hip -- the heads block's first layers, backward: the two GEMMs over the P rows that follow
// gs4d_heads_backward, hand-written so that their bits do not depend on a library's per-process kernel choice:
//   dh  (P x W)  = da W1     gs4d_mlp_dx_bf16 / gs4d_mlp_dx_f32   (input gradient)
//   dW1 (KW x W) = da^T h    gs4d_mlp_dw_bf16 / gs4d_mlp_dw_f32   (weight gradient, split over row chunks)
// Kernels first, their entry points at the end of the file.
#include <math.h>

#include <algorithm>

#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {

// ---- the bf16 heads block's input gradient: dh (P x W, fp32) = da (P x KW, bf16) W1 (KW x W, bf16), computed
// as dh^T = W1^T da^T on v_mfma_f32_16x16x32_bf16: the A operand is W1^T (W x KW, written by the block forward),
// the B operand da's rows as they lie in memory (lane (q, c): row c of a 16-row block, k = 32 s + 8 q .. + 7:
// one 16-byte load), and D[n = 16 m + 4 q + r][row c] leaves as one float4 per lane and tile.  A 512-thread
// workgroup takes 256 rows (32 per wave); W1^T is staged per 64-wide k chunk in LDS (16 KiB, double-buffered,
// row stride 144 B so the 16 rows of a fragment read fall on distinct banks) and shared by the 8 waves, so it
// is read from L2 once per workgroup instead of once per wave; da is prefetched one chunk ahead.  fp32
// accumulation over KW.
constexpr int kDxThreads = 512, kDxRowsPerWave = 32, kDxChunk = 64, kDxLdsStride = kDxChunk + 8;  // bf16 units
template <int W>
__global__ __launch_bounds__(kDxThreads) void mlp_dx_bf16_kernel(int P, int KW, const __bf16 *__restrict__ da,
                                                                 const __bf16 *__restrict__ w1t,
                                                                 float *__restrict__ dh) {
    constexpr int NT = W / 16, RB = kDxRowsPerWave / 16;
    constexpr int kPieces = W * kDxChunk / 8 / kDxThreads;  // 16-byte pieces of a chunk per thread (W = 128: 2)
    __shared__ __attribute__((aligned(16))) __bf16 s_a[2][W * kDxLdsStride];
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4, c = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * (kDxThreads / 64) * kDxRowsPerWave + (int64_t)wv * kDxRowsPerWave;
    const __bf16 *brow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; rb++)  // rows past P read row P - 1 (unconditional loads; not stored)
        brow[rb] = da + (size_t)min(row0 + 16 * rb + c, (int64_t)P - 1) * KW + 8 * q;
    f4v acc[NT][RB];
#pragma unroll
    for (int m = 0; m < NT; m++)
#pragma unroll
        for (int rb = 0; rb < RB; rb++) acc[m][rb] = f4v{0.f, 0.f, 0.f, 0.f};
    const int nch = KW / kDxChunk;
    bf8v ga[kPieces];
    auto load_a = [&](int ch) {  // piece e: W1^T row e / 8, 16-byte column piece e % 8 of the chunk
#pragma unroll
        for (int i = 0; i < kPieces; i++) {
            const int e = threadIdx.x + i * kDxThreads;
            ga[i] = *reinterpret_cast<const bf8v *>(w1t + (size_t)(e >> 3) * KW + ch * kDxChunk + 8 * (e & 7));
        }
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kPieces; i++) {
            const int e = threadIdx.x + i * kDxThreads;
            *reinterpret_cast<bf8v *>(&s_a[buf][(e >> 3) * kDxLdsStride + 8 * (e & 7)]) = ga[i];
        }
    };
    bf8v bn[2][RB];
    auto load_b = [&](int ch) {
#pragma unroll
        for (int st = 0; st < 2; st++)
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
                bn[st][rb] = *reinterpret_cast<const bf8v *>(brow[rb] + ch * kDxChunk + 32 * st);
    };
    load_a(0);
    load_b(0);
    store_a(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ch++) {
        bf8v b[2][RB];
#pragma unroll
        for (int st = 0; st < 2; st++)
#pragma unroll
            for (int rb = 0; rb < RB; rb++) b[st][rb] = bn[st][rb];
        const int nx = min(ch + 1, nch - 1);  // the last chunk re-loads itself: loads stay unconditional
        load_a(nx);
        load_b(nx);
        const __bf16 *sa = s_a[ch & 1];
#pragma unroll
        for (int st = 0; st < 2; st++)
#pragma unroll
            for (int m = 0; m < NT; m++) {
                const bf8v a = *reinterpret_cast<const bf8v *>(sa + (16 * m + c) * kDxLdsStride + 32 * st + 8 * q);
#pragma unroll
                for (int rb = 0; rb < RB; rb++)
                    acc[m][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[st][rb], acc[m][rb], 0, 0, 0);
            }
        if (ch + 1 < nch) store_a((ch + 1) & 1);  // the other buffer: read by nobody since the last barrier
        __syncthreads();
    }
#pragma unroll
    for (int rb = 0; rb < RB; rb++) {
        const int64_t row = row0 + 16 * rb + c;
        if (row < P)
#pragma unroll
            for (int m = 0; m < NT; m++)
                *reinterpret_cast<float4 *>(dh + (size_t)row * W + 16 * m + 4 * q) =
                    make_float4(acc[m][rb][0], acc[m][rb][1], acc[m][rb][2], acc[m][rb][3]);
    }
}

// ---- the bf16 heads block's first-layer weight gradient: dW1 (KW x W, fp32) = da^T hb, reduced over the P rows.
// Workgroup (row chunk s of 1024 rows, head i) forms the 128 x 128 block of head i's rows of dW1 over its chunk
// into parts[s] (summed over the chunks by gs4d_sum_slices, in its fixed order): D[da feature 16 m + 4 q + r][hb feature
// 16 n + c] on v_mfma_f32_16x16x32_bf16 with K = rows.  Both operands need 8 consecutive ROWS of one column, so
// each 64-row step stages the da and hb tiles (64 x 128 bf16 each, row-major as loaded) in LDS and reads them
// back with ds_read_b64_tr_b16 (a 16-lane group reads a 4 x 16 block and receives it column-major): two
// transposed reads give an operand's 8 rows.  The tiles use the XOR-swizzled 256-byte rows of the guide's
// dual-use image (conflict-free transposed reads; dwb_off / dwb_tr_frag in train_internal.h, shared with
// heads_bwd_wide_bf16_kernel); rows past P are staged as zeros.  Double-buffered: the next step's tiles are
// loaded while this step's MFMAs run.
constexpr int kDwbThreads = 256, kDwbChunkRows = 1024, kDwbStepRows = 64;  // two MFMA k-steps per staged tile
__global__ __launch_bounds__(kDwbThreads) void mlp_dw_bf16_kernel(int P, int KW, const __bf16 *__restrict__ da,
                                                                  const __bf16 *__restrict__ hb,
                                                                  float *__restrict__ parts) {
    constexpr int W = 128, NT = W / 16, MW = NT / (kDwbThreads / 64);  // m tiles per wave: 2
    constexpr int kPer = kDwbStepRows * 16 / kDwbThreads;  // 16-byte chunks per thread and tile
    __shared__ __attribute__((aligned(16))) unsigned char s_t[2][2][kDwbStepRows * 256];  // [buffer][da, hb][tile]
    const int head = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * kDwbChunkRows;
    const int nst = (int)((min((int64_t)P, r0 + kDwbChunkRows) - r0 + kDwbStepRows - 1) / kDwbStepRows);
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, li = lane & 15;
    f4v acc[MW][NT];
#pragma unroll
    for (int m = 0; m < MW; m++)
#pragma unroll
        for (int n = 0; n < NT; n++) acc[m][n] = f4v{0.f, 0.f, 0.f, 0.f};
    // staging: thread t moves chunks t, t + 256, ... of each tile: row e / 16, chunk e % 16
    bf8v ld[2][kPer];
    auto load = [&](int st) {
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const int e = threadIdx.x + i * kDwbThreads, row = e >> 4, ch = e & 15;
            const int64_t pr = r0 + kDwbStepRows * st + row;
            const bool ok = pr < P;
            const int64_t prc = ok ? pr : 0;
            const bf8v z = bf8v{};
            const bf8v va = *reinterpret_cast<const bf8v *>(da + (size_t)prc * KW + head * W + 8 * ch);
            const bf8v vh = *reinterpret_cast<const bf8v *>(hb + (size_t)prc * W + 8 * ch);
            ld[0][i] = ok ? va : z;
            ld[1][i] = ok ? vh : z;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const int e = threadIdx.x + i * kDwbThreads, row = e >> 4, ch = e & 15;
            *reinterpret_cast<bf8v *>(&s_t[buf][0][dwb_off(row, ch)]) = ld[0][i];
            *reinterpret_cast<bf8v *>(&s_t[buf][1][dwb_off(row, ch)]) = ld[1][i];
        }
    };
    if (nst > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int st = 0; st < nst; st++) {
        if (st + 1 < nst) load(st + 1);
        const unsigned char *ta = s_t[st & 1][0], *th = s_t[st & 1][1];
#pragma unroll
        for (int kk = 0; kk < kDwbStepRows / 32; kk++) {
            bf8v a[MW];
#pragma unroll
            for (int m = 0; m < MW; m++) a[m] = dwb_tr_frag(ta, 32 * kk, g, li, 2 * (wv * MW + m));
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const bf8v b = dwb_tr_frag(th, 32 * kk, g, li, 2 * n);
#pragma unroll
                for (int m = 0; m < MW; m++)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b, acc[m][n], 0, 0, 0);
            }
        }
        if (st + 1 < nst) store((st + 1) & 1);  // the other buffer: nobody reads it since the last barrier
        __syncthreads();
    }
    // D[da feature 16 m + 4 g + r][hb feature 16 n + li] of head `head` -> parts[s]
    float *o = parts + (size_t)blockIdx.x * KW * W + (size_t)head * W * W;
#pragma unroll
    for (int m = 0; m < MW; m++)
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                o[(size_t)(16 * (wv * MW + m) + 4 * g + r) * W + 16 * n + li] = acc[m][n][r];
}

// ---- the fp32 heads block's input gradient: dh (P x W) = da (P x KW) W1 (KW x W) on v_mfma_f32_16x16x4_f32
// (f32 products and sums in one fixed order per element: the same bits in every process, where the library
// GEMM this replaces was picked per process by timing).  Computed transposed as mlp_dx_bf16_kernel does:
// dh^T = W1^T da^T.  In the 16-wide k slice kk, lane (q = l >> 4, c = l & 15) supplies k = 16 kk + 4 q + s in
// MFMA step s, so one float4 load of da row c gives the lane's 4 steps of the B operand, and the A operand
// W1^T[16 m + c][16 kk + 4 q .. + 3] is one 16-byte LDS read.  The operand is W1^T (W x KW, written by the heads
// block forward): its k-runs are staged with coalesced 16-byte loads and 16-byte LDS stores, row stride KC + 8
// floats, which is conflict-free for both (ds_read_b128's four 16-lane groups; 8-lane store groups).  (Round 6
// first staged W1 itself, transposing with scalar stores at stride KC + 4: 2-way conflicts on every read, 38M
// conflict cycles per launch, 63 % MFMA busy.)
// A workgroup is 4 waves on ONE 64-feature group of dh (4 m tiles) and 64 rows (16 per wave): small units of
// work (3136 workgroups at P = 100k, W = 128) keep the per-CU share even.  The group's 64 x KC block of W1^T is
// staged per k chunk, double-buffered; da is prefetched a chunk ahead.  Workgroups b and b + 8 (same XCD) take the
// two feature groups of the same rows, so the second read of those da rows is an L2 hit.
// KC: the k chunk, a divisor of 64 with an even KW / KC (the loop runs chunks in pairs: an even count keeps both
// halves unconditional, so the compiler cannot sink the second half's loads into a branch).
constexpr int kDxfThreads = 256;
// RB: 16-row blocks per wave (2: each W1^T LDS read feeds twice the MFMAs).  gs4d_mlp_dx_f32 launches KC = 32,
// RB = 2 only.
template <int W, int KC, int RB>
__global__ __launch_bounds__(kDxfThreads) void mlp_dx_f32_kernel(int P, int KW, int nrg, const float *__restrict__ da,
                                                                 const float *__restrict__ w1t, float *__restrict__ dh) {
    constexpr int NG = W / 64;  // feature groups
    constexpr int S = KC + 8, KK = KC / 16, NP = KC / 16, Q = KC / 4;  // NP: staging float4 per thread; Q per row
    __shared__ __attribute__((aligned(16))) float s_a[2][64 * S];
    int rg = blockIdx.x, fg = 0;
    if (NG == 2) {
        const int i = blockIdx.x & 15;
        fg = i >> 3;
        rg = (int)(blockIdx.x >> 4) * 8 + (i & 7);
    }
    if (rg >= nrg) return;  // the grid is padded to whole groups of 8 row groups (uniform over the workgroup)
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4,
              c = lane & 15;
    int64_t row[RB];
    const float *brow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; rb++) {
        row[rb] = (int64_t)rg * 64 * RB + wv * 16 * RB + 16 * rb + c;
        // rows past P read row P - 1 (unconditional loads; not stored)
        brow[rb] = da + (size_t)min(row[rb], (int64_t)P - 1) * KW + 4 * q;
    }
    f4v acc[4][RB];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int rb = 0; rb < RB; rb++) acc[m][rb] = f4v{0.f, 0.f, 0.f, 0.f};
    const int nch = KW / KC;
    // staging: piece e = t + 256 i is W1^T row 64 fg + e / Q (a feature), k 4 (e % Q) .. + 3 of the chunk.
    // Chunks run in pairs, the pair's two halves unrolled with compile-time buffer and register-set indices (no
    // lambdas: captured register arrays were left in scratch memory), each half issuing the next chunk's loads
    // ahead of its own MFMAs.  nch is even (KC), so both halves are straight-line code.
    float4 bb[2][RB][KK];
    {
        float4 ga[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int e = (int)threadIdx.x + kDxfThreads * i;
            ga[i] = *reinterpret_cast<const float4 *>(w1t + (size_t)(64 * fg + e / Q) * KW + 4 * (e % Q));
        }
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int kk = 0; kk < KK; kk++) bb[0][rb][kk] = *reinterpret_cast<const float4 *>(brow[rb] + 16 * kk);
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int e = (int)threadIdx.x + kDxfThreads * i;
            *reinterpret_cast<float4 *>(&s_a[0][(e / Q) * S + 4 * (e % Q)]) = ga[i];
        }
    }
    __syncthreads();
    for (int ch = 0; ch < nch; ch += 2) {
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            const int nx = min(ch + hf + 1, nch - 1);  // the last chunk re-loads itself: loads stay unconditional
            float4 ga[NP];
#pragma unroll
            for (int i = 0; i < NP; i++) {
                const int e = (int)threadIdx.x + kDxfThreads * i;
                ga[i] = *reinterpret_cast<const float4 *>(w1t + (size_t)(64 * fg + e / Q) * KW + nx * KC + 4 * (e % Q));
            }
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
#pragma unroll
                for (int kk = 0; kk < KK; kk++)
                    bb[hf ^ 1][rb][kk] = *reinterpret_cast<const float4 *>(brow[rb] + nx * KC + 16 * kk);
            __builtin_amdgcn_sched_barrier(0);  // left to itself the scheduler sank the loads below the MFMAs
            const float *sa = s_a[hf];
#pragma unroll
            for (int kk = 0; kk < KK; kk++)
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const float4 av = *reinterpret_cast<const float4 *>(sa + (16 * m + c) * S + 16 * kk + 4 * q);
#pragma unroll
                    for (int rb = 0; rb < RB; rb++) {
                        const float4 bv = bb[hf][rb][kk];
                        acc[m][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[m][rb], 0, 0, 0);
                        acc[m][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[m][rb], 0, 0, 0);
                        acc[m][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[m][rb], 0, 0, 0);
                        acc[m][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[m][rb], 0, 0, 0);
                    }
                }
            // the other buffer: read by nobody since the last barrier (after the last chunk, by nobody at all)
#pragma unroll
            for (int i = 0; i < NP; i++) {
                const int e = (int)threadIdx.x + kDxfThreads * i;
                *reinterpret_cast<float4 *>(&s_a[hf ^ 1][(e / Q) * S + 4 * (e % Q)]) = ga[i];
            }
            __syncthreads();
        }
    }
    // D[feature 16 m + 4 q + r][row c]
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
        if (row[rb] < P)
#pragma unroll
            for (int m = 0; m < 4; m++)
                *reinterpret_cast<float4 *>(dh + (size_t)row[rb] * W + 64 * fg + 16 * m + 4 * q) =
                    make_float4(acc[m][rb][0], acc[m][rb][1], acc[m][rb][2], acc[m][rb][3]);
}

// ---- the fp32 heads block's first-layer weight gradient: dW1 (KW x W) = da^T h reduced over the P rows, on
// v_mfma_f32_16x16x4_f32 with K = rows.  Workgroup (row chunk s, 64-row block mb of dW1): 4 waves, wave w owning
// the 64 x (W / 4) block of columns w W/4 ..; the chunk's rows pass through LDS in 16-row stages (da's 64 columns
// and h's W columns of each row, coalesced 16-byte loads and stores, double-buffered, the next stage's loads
// issued ahead of this stage's MFMAs).  In the MFMA k-step over stage rows r .. r + 3, lane (q, c) reads
// A[feature c][row q] = da[r + q][64 mb + 16 mt + c] and B[row q][feature c] = h[r + q][16 nt + c] as single
// dwords (row strides of 80 and W + 16 floats: the two rows a 32-lane half reads fall on opposite bank halves,
// conflict-free).  Rows past P are staged as zeros.  Each wave writes its block of parts[s]; gs4d_sum_slices adds
// the chunks in its fixed order.  Deterministic by construction.  The m blocks of one chunk sit on one XCD (they share its
// h rows).  (Round 6 first read both operands straight from HBM as dwords at 2 waves/SIMD: 50 % MFMA busy.)
constexpr int kDwfThreads = 256, kDwfStage = 16;
// v, or zeros: component selects (a select between two float4 values became a select of scratch addresses)
__device__ __forceinline__ float4 keep4(bool ok, float4 v) {
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}
// MB: dW1 rows per workgroup, 64 (waves side by side over the W columns) or 128 (waves 2 x 2, each a 64 x W/2
// block: twice the MFMAs per stage and per LDS read)
template <int W, int MB>
__global__ __launch_bounds__(kDwfThreads) void mlp_dw_f32_kernel(int P, int KW, int S, int chunk_rows,
                                                                 const float *__restrict__ da,
                                                                 const float *__restrict__ h,
                                                                 float *__restrict__ parts) {
    constexpr int MT = 4, NTW = MB == 64 ? W / 64 : W / 32;  // m tiles and n tiles per wave
    constexpr int SD = MB + 16, SH = W + 16, QD = MB / 4;    // QD: float4 per staged da row
    constexpr int PD = kDwfStage * QD / kDwfThreads, PH = kDwfStage * (W / 4) / kDwfThreads;  // float4 per thread
    __shared__ __attribute__((aligned(16))) float s_d[2][kDwfStage * SD];
    __shared__ __attribute__((aligned(16))) float s_h[2][kDwfStage * SH];
    const int nmb = KW / MB;
    // b = 8 (nmb j + mb) + x: chunk s = 8 j + x, so the nmb blocks of a chunk share b % 8 (the XCD)
    const int b = blockIdx.x, x = b & 7, jm = b >> 3, mb = jm % nmb, s = 8 * (jm / nmb) + x;
    if (s >= S) return;  // padding of the grid to whole groups of 8 chunks (uniform over the workgroup)
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4,
              c = lane & 15;
    const int wm = MB == 64 ? 0 : wv >> 1, wn = MB == 64 ? wv : wv & 1;  // the wave's m and n block
    const int64_t r0 = (int64_t)s * chunk_rows, r1 = min((int64_t)P, r0 + chunk_rows);
    f4v acc[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NTW; nt++) acc[mt][nt] = f4v{0.f, 0.f, 0.f, 0.f};
    // staging: da piece e: stage row e / QD, float4 e % QD; h piece e: stage row e / (W / 4), float4 e % (W / 4).
    // Stages run in pairs, each half unrolled with compile-time buffer indices (see mlp_dx_f32_kernel): the next
    // stage's loads, this stage's MFMAs from LDS, then the next stage into the other buffer (rows past r1 read row
    // r1 - 1 and are stored as zeros; past the last stage a padding stage, zeros, read by nobody).
    const int nst = (int)((r1 - r0 + 2 * kDwfStage - 1) / (2 * kDwfStage)) * 2;
#pragma unroll
    for (int pre = 0; pre < 1; pre++) {  // stage 0 into buffer 0
        float4 gd[PD], gh[PH];
#pragma unroll
        for (int i = 0; i < PD; i++) {
            const int e = (int)threadIdx.x + kDwfThreads * i;
            const int64_t r = r0 + e / QD;
            gd[i] = *reinterpret_cast<const float4 *>(da + (size_t)min(r, r1 - 1) * KW + MB * mb + 4 * (e % QD));
            *reinterpret_cast<float4 *>(&s_d[0][(e / QD) * SD + 4 * (e % QD)]) = keep4(r < r1, gd[i]);
        }
#pragma unroll
        for (int i = 0; i < PH; i++) {
            const int e = (int)threadIdx.x + kDwfThreads * i;
            const int64_t r = r0 + e / (W / 4);
            gh[i] = *reinterpret_cast<const float4 *>(h + (size_t)min(r, r1 - 1) * W + 4 * (e % (W / 4)));
            *reinterpret_cast<float4 *>(&s_h[0][(e / (W / 4)) * SH + 4 * (e % (W / 4))]) = keep4(r < r1, gh[i]);
        }
    }
    __syncthreads();
    for (int st = 0; st < nst; st += 2) {
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            const int64_t rn = r0 + (int64_t)kDwfStage * (st + hf + 1);  // the next stage's first row
            float4 gd[PD], gh[PH];
#pragma unroll
            for (int i = 0; i < PD; i++) {
                const int e = (int)threadIdx.x + kDwfThreads * i;
                gd[i] = *reinterpret_cast<const float4 *>(da + (size_t)min(rn + e / QD, r1 - 1) * KW + MB * mb +
                                                          4 * (e % QD));
            }
#pragma unroll
            for (int i = 0; i < PH; i++) {
                const int e = (int)threadIdx.x + kDwfThreads * i;
                gh[i] = *reinterpret_cast<const float4 *>(h + (size_t)min(rn + e / (W / 4), r1 - 1) * W +
                                                          4 * (e % (W / 4)));
            }
            __builtin_amdgcn_sched_barrier(0);
            const float *sd = s_d[hf], *sh = s_h[hf];
#pragma unroll
            for (int u = 0; u < kDwfStage / 4; u++) {
                float av[MT], hv[NTW];
#pragma unroll
                for (int mt = 0; mt < MT; mt++) av[mt] = sd[(4 * u + q) * SD + 64 * wm + 16 * mt + c];
#pragma unroll
                for (int nt = 0; nt < NTW; nt++) hv[nt] = sh[(4 * u + q) * SH + 16 * (NTW * wn + nt) + c];
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int nt = 0; nt < NTW; nt++)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], hv[nt], acc[mt][nt], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < PD; i++) {
                const int e = (int)threadIdx.x + kDwfThreads * i;
                *reinterpret_cast<float4 *>(&s_d[hf ^ 1][(e / QD) * SD + 4 * (e % QD)]) = keep4(rn + e / QD < r1, gd[i]);
            }
#pragma unroll
            for (int i = 0; i < PH; i++) {
                const int e = (int)threadIdx.x + kDwfThreads * i;
                *reinterpret_cast<float4 *>(&s_h[hf ^ 1][(e / (W / 4)) * SH + 4 * (e % (W / 4))]) =
                    keep4(rn + e / (W / 4) < r1, gh[i]);
            }
            __syncthreads();
        }
    }
    // D[feature 64 wm + 16 mt + 4 q + r][column 16 (NTW wn + nt) + c] of rows MB mb .. of dW1
    float *o = parts + (size_t)s * KW * W + (size_t)(MB * mb + 64 * wm) * W;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NTW; nt++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                o[(size_t)(16 * mt + 4 * q + r) * W + 16 * (NTW * wn + nt) + c] = acc[mt][nt][r];
}

}  // namespace gs4d

using namespace gs4d;

extern "C" {

int gs4d_mlp_dx_bf16(int P, int KW, int W, const uint16_t *da, const uint16_t *w1t, float *dh, void *stream) {
    if (P < 0 || KW < kDxChunk || KW % kDxChunk != 0 || (W != 64 && W != 128)) return 1;
    if (P == 0) return 0;
    if (!da || !w1t || !dh || (((size_t)da | (size_t)w1t | (size_t)dh) & 15) != 0) return 1;
    const int64_t rows_per_wg = (kDxThreads / 64) * kDxRowsPerWave;
    const dim3 grid((unsigned)(((int64_t)P + rows_per_wg - 1) / rows_per_wg));
    if (W == 128)
        hipLaunchKernelGGL(mlp_dx_bf16_kernel<128>, grid, dim3(kDxThreads), 0, (hipStream_t)stream, P, KW,
                           (const __bf16 *)da, (const __bf16 *)w1t, dh);
    else
        hipLaunchKernelGGL(mlp_dx_bf16_kernel<64>, grid, dim3(kDxThreads), 0, (hipStream_t)stream, P, KW,
                           (const __bf16 *)da, (const __bf16 *)w1t, dh);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

size_t gs4d_mlp_dw_bf16_scratch_bytes(int P, int KW, int W) {
    if (P <= 0 || KW <= 0 || W <= 0) return 256;
    const size_t S = ((size_t)P + kDwbChunkRows - 1) / kDwbChunkRows;
    return 4 * S * (size_t)KW * W + 256;
}

int gs4d_mlp_dw_bf16(int P, int KW, int W, const uint16_t *da, const uint16_t *hb, float *dw, void *scratch,
                     void *stream) {
    if (P < 0 || W != 128 || KW < W || KW % W != 0 || !dw) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) return hipMemsetAsync(dw, 0, 4 * (size_t)KW * W, s) == hipSuccess ? 0 : 3;
    if (!da || !hb || !scratch || (((size_t)da | (size_t)hb) & 15) != 0) return 1;
    const int S = (int)(((int64_t)P + kDwbChunkRows - 1) / kDwbChunkRows);
    float *parts = (float *)align_up((size_t)scratch, 256);
    hipLaunchKernelGGL(mlp_dw_bf16_kernel, dim3(S, KW / W), dim3(kDwbThreads), 0, s, P, KW, (const __bf16 *)da,
                       (const __bf16 *)hb, parts);
    if (hipGetLastError() != hipSuccess) return 3;
    return gs4d_sum_slices(parts, S, (int64_t)KW * W, dw, stream);
}

int gs4d_mlp_dx_f32(int P, int KW, int W, const float *da, const float *w1t, float *dh, void *stream) {
    if (P < 0 || KW < 64 || KW % 64 != 0 || (W != 64 && W != 128)) return 1;
    if (P == 0) return 0;
    if (!da || !w1t || !dh || (((size_t)da | (size_t)w1t | (size_t)dh) & 15) != 0) return 1;
    hipStream_t s = (hipStream_t)stream;
    // the one kept shape of the kernel: two 16-row blocks per wave (RB = 2) on 32-wide k chunks -- two register
    // sets of B for two row blocks fit 4 waves/SIMD
    constexpr int RB = 2;
    const int nrg = (int)(((int64_t)P + 64 * RB - 1) / (64 * RB));
    // W = 128: two feature groups per row group, the grid padded to whole groups of 8 row groups
    const dim3 grid((unsigned)(W == 128 ? (nrg + 7) / 8 * 16 : nrg));
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(kDxfThreads), 0, s, P, KW, nrg, da, w1t, dh); };
    if (W == 128) go(mlp_dx_f32_kernel<128, 32, RB>);
    else go(mlp_dx_f32_kernel<64, 32, RB>);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// the m-block rows of gs4d_mlp_dw_f32's workgroups
static int dwf_mb(int KW, int W) { return (KW % 128 == 0 && W == 128) ? 128 : 64; }
// the row chunks of gs4d_mlp_dw_f32: one resident round of workgroups over (chunk, m block) -- four per CU (a
// wave per SIMD each, <= 128 registers) -- so that every workgroup runs once and all finish together; chunks a
// multiple of 32 rows, at least 256.  The chunk count S therefore follows the device's CU count, and with it the
// grouping of gs4d_sum_slices' fixed-order sum: dW1 is the same bits on every run on one device model, but a
// device with another CU count may round it differently.
static void dwf_chunks(int P, int KW, int W, int *S, int *rows) {
    const int nmb = std::max(1, KW / dwf_mb(KW, W));
    const int64_t target = std::max<int64_t>(1, (4 * (int64_t)cu_count()) / nmb);
    int64_t c = ((int64_t)P + target - 1) / target;
    c = std::max<int64_t>(256, (c + 31) / 32 * 32);
    *rows = (int)c;
    *S = (int)std::max<int64_t>(1, ((int64_t)P + c - 1) / c);
}

size_t gs4d_mlp_dw_f32_scratch_bytes(int P, int KW, int W) {
    if (P <= 0 || KW <= 0 || W <= 0) return 256;
    int S = 1, rows = 0;
    dwf_chunks(P, KW, W, &S, &rows);
    return 4 * (size_t)S * KW * W + 256;
}

int gs4d_mlp_dw_f32(int P, int KW, int W, const float *da, const float *h, float *dw, void *scratch, void *stream) {
    if (P < 0 || (W != 64 && W != 128) || KW < 64 || KW % 64 != 0 || !dw) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) return hipMemsetAsync(dw, 0, 4 * (size_t)KW * W, s) == hipSuccess ? 0 : 3;
    if (!da || !h || !scratch) return 1;
    int S = 1, rows = 0;
    dwf_chunks(P, KW, W, &S, &rows);
    float *parts = (float *)align_up((size_t)scratch, 256);
    const int MB = dwf_mb(KW, W);
    const unsigned grid = (unsigned)(8 * (KW / MB) * ((S + 7) / 8));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kDwfThreads), 0, s, P, KW, S, rows, da, h, parts);
    };
    if (W == 128) MB == 128 ? go(mlp_dw_f32_kernel<128, 128>) : go(mlp_dw_f32_kernel<128, 64>);
    else go(mlp_dw_f32_kernel<64, 64>);
    if (hipGetLastError() != hipSuccess) return 3;
    return gs4d_sum_slices(parts, S, (int64_t)KW * W, dw, stream);
}

}  // extern "C"
