// mlp_heads_forward.hip -- the deformation heads (scene/deformation.py:73-78: ReLU -> Linear(W, W) -> ReLU ->
// Linear(W, n_i) per head), forward: the second layers alone over a given first-layer output (heads_fwd_kernel),
// and the whole block, both layers in one pass, on fp32 and on bf16 operands (heads_block_fwd[_bf16]_kernel).
// Their entry points gs4d_heads_forward and gs4d_heads_block_forward[_bf16] are at the end of the file.
#include <math.h>

#include <algorithm>

#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {

// ---- the deformation heads' second layers, forward (scene/deformation.py:73-78 as one block: head i =
// a[:, iW:(i+1)W] W2_i^T + b2_i on a = relu(h W1^T + b1), (P, kW)) in ONE pass over a on the f32 MFMA
// (v_mfma_f32_16x16x4_f32), where torch runs k small GEMMs on column slices.  A wave takes 16-row
// blocks; for each head and 16-column K chunk the wave reads a as float4 straight from HBM (lane group
// q = l >> 4 holds columns 4q..4q+3 of its row l & 15: the MFMA's k index in step s is column 4q + s,
// so each lane's 4 steps come from one 16-byte load), the matching W2 rows (staged in LDS, row stride
// W + 4: conflict-free 16-byte reads) are the B operand, one accumulator per 16 outputs of the head.
struct HfArgs {
    int P, W, k, kW;  // kW: the row stride of a (floats)
    int n[kHbMaxHeads];
    int roff[kHbMaxHeads];  // head i's first row in the LDS copy of the W2s
    const float *w2[kHbMaxHeads];
    const float *b2[kHbMaxHeads];
    float *out[kHbMaxHeads];
};
constexpr int kHfThreads = 256, kHfMaxTiles = 4;  // up to 64 outputs per head

// NT...: tiles of 16 outputs per head, compile-time, so that every head's accumulators are registers
// and ALL heads advance together through each 16-column K chunk (sum NT independent MFMA chains; the
// next chunk's loads are issued before this chunk's MFMAs).
template <int W, int... NT>
__global__ __launch_bounds__(kHfThreads) void heads_fwd_kernel(HfArgs A, const float *__restrict__ a) {
    constexpr int K = sizeof...(NT);
    constexpr int nt[K] = {NT...};
    extern __shared__ float4 s_w2v[];
    float *s_w2 = reinterpret_cast<float *>(s_w2v);
    constexpr int WS = W + 4;
    for (int i = 0; i < K; i++)
        for (int e = threadIdx.x; e < A.n[i] * (W / 4); e += kHfThreads) {
            const int row = e / (W / 4), c4 = e % (W / 4);
            reinterpret_cast<float4 *>(s_w2 + (size_t)(A.roff[i] + row) * WS)[c4] =
                reinterpret_cast<const float4 *>(A.w2[i] + (size_t)row * W)[c4];
        }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4, c = lane & 15;
    const int nblk = (A.P + 15) / 16;
    for (int blk = blockIdx.x * (kHfThreads / 64) + wv; blk < nblk; blk += gridDim.x * (kHfThreads / 64)) {
        const int r0 = blk * 16, ra = r0 + c;
        const bool live = ra < A.P;
        const float *arow = a + (size_t)min(ra, A.P - 1) * A.kW + 4 * q;
        f4v acc[K][4];
#pragma unroll
        for (int i = 0; i < K; i++)
#pragma unroll
            for (int t = 0; t < 4; t++) acc[i][t] = f4v{0.f, 0.f, 0.f, 0.f};
        float4 av[K], an[K];
#pragma unroll
        for (int i = 0; i < K; i++) an[i] = *reinterpret_cast<const float4 *>(arow + i * W);
#pragma unroll 2
        for (int kc = 0; kc < W / 16; kc++) {
#pragma unroll
            for (int i = 0; i < K; i++) av[i] = live ? an[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (kc + 1 < W / 16) {
#pragma unroll
                for (int i = 0; i < K; i++) an[i] = *reinterpret_cast<const float4 *>(arow + i * W + 16 * (kc + 1));
            }
#pragma unroll
            for (int i = 0; i < K; i++) {
#pragma unroll
                for (int t = 0; t < nt[i]; t++) {
                    const int nn = 16 * t + c;
                    const float4 bv = nn < A.n[i] ? *reinterpret_cast<const float4 *>(
                                                        s_w2 + (size_t)(A.roff[i] + nn) * WS + 16 * kc + 4 * q)
                                                  : make_float4(0.f, 0.f, 0.f, 0.f);
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].x, bv.x, acc[i][t], 0, 0, 0);
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].y, bv.y, acc[i][t], 0, 0, 0);
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].z, bv.z, acc[i][t], 0, 0, 0);
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].w, bv.w, acc[i][t], 0, 0, 0);
                }
            }
        }
        // C[row 4q + j][col 16 t + c]
#pragma unroll
        for (int i = 0; i < K; i++) {
#pragma unroll
            for (int t = 0; t < nt[i]; t++) {
                const int col = 16 * t + c, n = A.n[i];
                if (col < n) {
                    const float bias = A.b2[i][col];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int r = r0 + 4 * q + j;
                        if (r < A.P) A.out[i][(size_t)r * n + col] = acc[i][t][j] + bias;
                    }
                }
            }
        }
    }
}
// ---- the whole heads block, forward (scene/deformation.py:73-78: head i = relu(h W1_i^T + b1_i) W2_i^T + b2_i
// on the shared h = relu(hidden)), first AND second layers in one pass on the f32 MFMA
// (v_mfma_f32_16x16x4_f32), where torch runs one (P x W) @ (W x kW) GEMM for the first layers and this
// library's heads_fwd pass read its (P, kW) result back.  Workgroup (x, head i): w1_i (W x W) and w2_i
// (n_i x W) staged in LDS, its waves each taking 16-point blocks.  Both layers are computed TRANSPOSED
// (features along the MFMA rows, the 16 points along its columns), so the first layer's accumulators are
// already the second layer's B operand: in k-step (t, v) lane l supplies feature 16 t + 4 (l >> 4) + v of
// point l & 15 -- the v-th register of its t-th accumulator (D[4 (l >> 4) + v][l & 15]) -- and the A operand
// (w1 / w2 rows from LDS, one 16-byte read per 4 MFMAs; row stride W + 8 floats, conflict-free for ds_read_b128's
// four 16-lane groups -- round 5's W + 4 put two lanes of a group on one bank slot: 9.4M conflict cycles per
// launch) uses the same feature order; 16 waves per workgroup, one workgroup per CU.  h is read as that
// B operand directly (one float4 per lane per 16 features); a = relu(z + b1) is written once, for the
// backward, and never read back.
constexpr int kHbfThreads = 512;
template <int W>
__global__ __launch_bounds__(kHbfThreads) void heads_block_fwd_kernel(HfArgs A, const float *__restrict__ h,
                                                                      const float *__restrict__ w1,
                                                                      const float *__restrict__ b1,
                                                                      float *__restrict__ a,
                                                                      float *__restrict__ w1t) {
    constexpr int NT = W / 16, WS = W + 8, NW = kHbfThreads / 64;
    extern __shared__ float4 s_v[];
    float *s_w1 = reinterpret_cast<float *>(s_v);  // W rows x WS
    float *s_b1 = s_w1 + W * WS;                   // W
    float *s_w2 = s_b1 + W;                        // n_pad rows x WS (rows >= n zero)
    const int head = blockIdx.y;
    const int n = A.n[head], npad = (n + 15) & ~15;
    float *s_b2 = s_w2 + npad * WS;  // n_pad (in LDS: a global load in the store loop would wait for every
                                     // load and store in flight, the next block's h prefetch included)
    const float *w1i = w1 + (size_t)head * W * W;
    for (int e = threadIdx.x; e < W * W / 4; e += kHbfThreads) {
        const int row = e / (W / 4), c4 = e % (W / 4);
        reinterpret_cast<float4 *>(s_w1 + row * WS)[c4] = reinterpret_cast<const float4 *>(w1i + (size_t)row * W)[c4];
    }
    for (int e = threadIdx.x; e < W; e += kHbfThreads) s_b1[e] = b1[head * W + e];
    for (int e = threadIdx.x; e < npad * (W / 4); e += kHbfThreads) {
        const int row = e / (W / 4), c4 = e % (W / 4);
        reinterpret_cast<float4 *>(s_w2 + row * WS)[c4] =
            row < n ? reinterpret_cast<const float4 *>(A.w2[head] + (size_t)row * W)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int e = threadIdx.x; e < npad; e += kHbfThreads) s_b2[e] = e < n ? A.b2[head][e] : 0.f;
    __syncthreads();
    if (w1t && blockIdx.x == 0) {
        // workgroup 0 of each head also writes W1_i^T for the backward's input gradient (gs4d_mlp_dx_f32): 4 rows
        // of one column of the LDS image per 16-byte store
        for (int e = threadIdx.x; e < W * W / 4; e += kHbfThreads) {
            const int col = e / (W / 4), r4 = e % (W / 4);
            *reinterpret_cast<float4 *>(w1t + (size_t)col * A.kW + head * W + 4 * r4) =
                make_float4(s_w1[(4 * r4) * WS + col], s_w1[(4 * r4 + 1) * WS + col], s_w1[(4 * r4 + 2) * WS + col],
                            s_w1[(4 * r4 + 3) * WS + col]);
        }
    }
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4, c = lane & 15;
    const int nblk = (A.P + 15) / 16;
    const int stride = gridDim.x * NW;
    float *out = A.out[head];
    const bool v4out = (n & 3) == 0 && ((size_t)out & 15) == 0;
    float4 hn[NT];
    // rows past P (the last block's, and the prefetch past the last block) read row P - 1: every load is
    // unconditional, so the compiler's wait before a block's MFMAs counts exactly the loads issued after its
    // h (a branch around them made it wait for ALL loads, the next block's prefetch included); those rows'
    // results go to a's padding rows or are not stored
    auto load_h = [&](int blk) {
        const int pt = min(blk * 16 + c, A.P - 1);
#pragma unroll
        for (int t = 0; t < NT; t++) hn[t] = *reinterpret_cast<const float4 *>(h + (size_t)pt * W + 16 * t + 4 * q);
    };
    int blk = blockIdx.x * NW + wv;
    load_h(blk);
    for (; blk < nblk; blk += stride) {
        float4 hv[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) hv[t] = hn[t];
        load_h(blk + stride);  // the next block's h loads fly while this one runs on the MFMA
        // z^T (W x 16) = W1_i h^T (a compiler barrier per 16-feature chunk keeps the LDS reads of one chunk,
        // 8 float4, in registers at a time)
        f4v acc[NT];
#pragma unroll
        for (int m = 0; m < NT; m++) acc[m] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; t++) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int m = 0; m < NT; m++) {
                const float4 av = *reinterpret_cast<const float4 *>(s_w1 + (16 * m + c) * WS + 16 * t + 4 * q);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, hv[t].x, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, hv[t].y, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, hv[t].z, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, hv[t].w, acc[m], 0, 0, 0);
            }
        }
        // a = relu(z + b1): lane holds features 16 m + 4 q + j of point c; written as float4 per m
        const int pt = blk * 16 + c;
#pragma unroll
        for (int m = 0; m < NT; m++) {
            const float4 bb = *reinterpret_cast<const float4 *>(s_b1 + 16 * m + 4 * q);
            acc[m][0] = fmaxf(acc[m][0] + bb.x, 0.f);
            acc[m][1] = fmaxf(acc[m][1] + bb.y, 0.f);
            acc[m][2] = fmaxf(acc[m][2] + bb.z, 0.f);
            acc[m][3] = fmaxf(acc[m][3] + bb.w, 0.f);
            // a has ceil(P / 16) * 16 rows (gs4d_heads_block_forward): no condition on the store
            *reinterpret_cast<float4 *>(a + (size_t)pt * A.kW + head * W + 16 * m + 4 * q) =
                make_float4(acc[m][0], acc[m][1], acc[m][2], acc[m][3]);
        }
        // out^T (n_pad x 16) = W2_i a^T, B operand = the accumulators above
        for (int j = 0; j < npad; j += 16) {
            f4v o = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < NT; m++) {
                const float4 wv4 = *reinterpret_cast<const float4 *>(s_w2 + (j + c) * WS + 16 * m + 4 * q);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.x, acc[m][0], o, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.y, acc[m][1], o, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.z, acc[m][2], o, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.w, acc[m][3], o, 0, 0, 0);
            }
            // D[output j + 4 q + r][point c]: one float4 per lane when the rows are 16-byte aligned
            if (pt < A.P) {
                const int o0 = j + 4 * q;
                if (v4out && o0 + 3 < n) {
                    const float4 bb = *reinterpret_cast<const float4 *>(s_b2 + o0);
                    *reinterpret_cast<float4 *>(out + (size_t)pt * n + o0) =
                        make_float4(o[0] + bb.x, o[1] + bb.y, o[2] + bb.z, o[3] + bb.w);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (o0 + r < n) out[(size_t)pt * n + o0 + r] = o[r] + s_b2[o0 + r];
                }
            }
        }
    }
}

// ---- the heads block forward on bf16 operands (hyper.mlp_dtype = "bf16", BASELINE C3's bf16 leg): the
// structure of heads_block_fwd_kernel on v_mfma_f32_16x16x32_bf16 (16x the f32 MFMA's rate), fp32
// accumulation, fp32 outputs.  Workgroup (x, head i): W1_i and W2_i converted to bf16 into LDS (row stride
// W + 8 elements); per 16-point block the first layer z^T (W x 16) = W1_i h^T is TRANSPOSED as in the f32
// kernel: in k-step t lane (q = l >> 4, c = l & 15) supplies h[point c][32 t + 8 q .. + 7] (converted to bf16
// on load) and W1_i[16 m + c][32 t + 8 q .. + 7] (one 16-byte LDS read); accumulator m then holds
// z[16 m + 4 q + v][point c], v = 0..3.  a = relu(z + b1) is rounded to bf16 once: stored (8 bytes per tile,
// for the backward) and used as the second layer's B operand straight from the registers -- k-step s of
// out^T = W2_i a^T takes the lane's values of accumulators 2s and 2s + 1, i.e. MFMA k index 8 q + j <->
// feature 16 (2 s + (j >> 2)) + 4 q + (j & 3), and the A operand (W2_i rows, two 8-byte LDS reads) uses
// that same feature order.
// HBIN: h arrives already rounded to bf16 in hb ((ceil(P / 16) * 16, W), gs4d_feature_relu_forward_hb), read as
// 16-byte loads (half the fp32 bytes per head) and not written
template <int W, bool HBIN>
__global__ __launch_bounds__(kHbfThreads) void heads_block_fwd_bf16_kernel(HfArgs A, const float *__restrict__ h,
                                                                           const float *__restrict__ w1,
                                                                           const float *__restrict__ b1,
                                                                           __bf16 *__restrict__ a,
                                                                           __bf16 *__restrict__ hb,
                                                                           __bf16 *__restrict__ w1t) {
    constexpr int NT = W / 16, NK = W / 32, WS = W + 8, NW = kHbfThreads / 64;
    extern __shared__ float4 s_v[];
    __bf16 *s_w1 = reinterpret_cast<__bf16 *>(s_v);       // W rows x WS
    const int head = blockIdx.y;
    const int n = A.n[head], npad = (n + 15) & ~15;
    __bf16 *s_w2 = s_w1 + W * WS;                            // npad rows x WS (rows >= n zero)
    float *s_b1 = reinterpret_cast<float *>(s_w2 + npad * WS);  // W
    float *s_b2 = s_b1 + W;                                  // npad
    const float *w1i = w1 + (size_t)head * W * W;
    for (int e = threadIdx.x; e < W * W / 4; e += kHbfThreads) {
        const int row = e / (W / 4), c4 = e % (W / 4);
        const float4 v = reinterpret_cast<const float4 *>(w1i + (size_t)row * W)[c4];
        const bf4v vb = bf4v{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
        *reinterpret_cast<bf4v *>(s_w1 + row * WS + 4 * c4) = vb;
    }
    for (int e = threadIdx.x; e < npad * (W / 4); e += kHbfThreads) {
        const int row = e / (W / 4), c4 = e % (W / 4);
        const float4 v = row < n ? reinterpret_cast<const float4 *>(A.w2[head] + (size_t)row * W)[c4]
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<bf4v *>(s_w2 + row * WS + 4 * c4) = bf4v{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
    }
    for (int e = threadIdx.x; e < W; e += kHbfThreads) s_b1[e] = b1[head * W + e];
    for (int e = threadIdx.x; e < npad; e += kHbfThreads) s_b2[e] = e < n ? A.b2[head][e] : 0.f;
    __syncthreads();
    if (w1t && blockIdx.x == 0) {
        // workgroup 0 of each head also writes W1_i^T in bf16 for the backward's input gradient
        // (gs4d_mlp_dx_bf16): 8 rows of one column of the LDS image per 16-byte store
        for (int e = threadIdx.x; e < W * W / 8; e += kHbfThreads) {
            const int col = e / (W / 8), r8 = e % (W / 8);
            bf8v v;
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = s_w1[(8 * r8 + j) * WS + col];
            *reinterpret_cast<bf8v *>(w1t + (size_t)col * A.kW + head * W + 8 * r8) = v;
        }
    }
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4, c = lane & 15;
    const int nblk = (A.P + 15) / 16;
    const int stride = gridDim.x * NW;
    float *out = A.out[head];
    const bool v4out = (n & 3) == 0 && ((size_t)out & 15) == 0;
    float4 hn[2 * NK];
    bf8v hbn[NK];
    // unconditional loads (rows past P read row P - 1), as in heads_block_fwd_kernel
    auto load_h = [&](int blk) {
        const int pt = min(blk * 16 + c, A.P - 1);
        if (HBIN) {
            const bf8v *src = reinterpret_cast<const bf8v *>(hb + (size_t)pt * W + 8 * q);
#pragma unroll
            for (int t = 0; t < NK; t++) hbn[t] = src[4 * t];
        } else {
            const float4 *src = reinterpret_cast<const float4 *>(h + (size_t)pt * W + 8 * q);
#pragma unroll
            for (int t = 0; t < NK; t++) {
                hn[2 * t] = src[8 * t];
                hn[2 * t + 1] = src[8 * t + 1];
            }
        }
    };
    int blk = blockIdx.x * NW + wv;
    load_h(blk);
    for (; blk < nblk; blk += stride) {
        bf8v hv[NK];
#pragma unroll
        for (int t = 0; t < NK; t++) {
            if (HBIN) {
                hv[t] = hbn[t];
            } else {
                const float4 x = hn[2 * t], y = hn[2 * t + 1];
                hv[t] = bf8v{(__bf16)x.x, (__bf16)x.y, (__bf16)x.z, (__bf16)x.w, (__bf16)y.x, (__bf16)y.y,
                             (__bf16)y.z, (__bf16)y.w};
            }
        }
        load_h(blk + stride);  // the next block's h loads fly while this one runs on the MFMA
        if (!HBIN && hb && head == 0) {  // bf16 h for the backward's weight-gradient GEMM (ceil(P / 16) * 16 rows)
            __bf16 *dst = hb + (size_t)(blk * 16 + c) * W + 8 * q;
#pragma unroll
            for (int t = 0; t < NK; t++) *reinterpret_cast<bf8v *>(dst + 32 * t) = hv[t];
        }
        f4v acc[NT];
#pragma unroll
        for (int m = 0; m < NT; m++) acc[m] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NK; t++) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int m = 0; m < NT; m++) {
                const bf8v av = *reinterpret_cast<const bf8v *>(s_w1 + (16 * m + c) * WS + 32 * t + 8 * q);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, hv[t], acc[m], 0, 0, 0);
            }
        }
        // a = relu(z + b1) in bf16: lane holds features 16 m + 4 q + v of point c
        const int pt = blk * 16 + c;
        bf4v ab[NT];
#pragma unroll
        for (int m = 0; m < NT; m++) {
            const float4 bb = *reinterpret_cast<const float4 *>(s_b1 + 16 * m + 4 * q);
            ab[m] = bf4v{(__bf16)fmaxf(acc[m][0] + bb.x, 0.f), (__bf16)fmaxf(acc[m][1] + bb.y, 0.f),
                         (__bf16)fmaxf(acc[m][2] + bb.z, 0.f), (__bf16)fmaxf(acc[m][3] + bb.w, 0.f)};
            // a has ceil(P / 16) * 16 rows: no condition on the store
            *reinterpret_cast<bf4v *>(a + (size_t)pt * A.kW + head * W + 16 * m + 4 * q) = ab[m];
        }
        // out^T (n_pad x 16) = W2_i a^T, B operand = the lane's bf16 a values (k-step s: tiles 2s, 2s + 1)
        for (int j = 0; j < npad; j += 16) {
            f4v o = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < NT / 2; s2++) {
                const __bf16 *wr = s_w2 + (j + c) * WS + 32 * s2 + 4 * q;
                const bf4v lo = *reinterpret_cast<const bf4v *>(wr), hi = *reinterpret_cast<const bf4v *>(wr + 16);
                const bf8v wa = bf8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const bf4v x0 = ab[2 * s2], x1 = ab[2 * s2 + 1];
                const bf8v xb = bf8v{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
                o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, xb, o, 0, 0, 0);
            }
            // D[output j + 4 q + r][point c]: one float4 per lane when the rows are 16-byte aligned
            if (pt < A.P) {
                const int o0 = j + 4 * q;
                if (v4out && o0 + 3 < n) {
                    const float4 bb = *reinterpret_cast<const float4 *>(s_b2 + o0);
                    *reinterpret_cast<float4 *>(out + (size_t)pt * n + o0) =
                        make_float4(o[0] + bb.x, o[1] + bb.y, o[2] + bb.z, o[3] + bb.w);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (o0 + r < n) out[(size_t)pt * n + o0 + r] = o[r] + s_b2[o0 + r];
                }
            }
        }
    }
}

}  // namespace gs4d

using namespace gs4d;

extern "C" {

int gs4d_heads_forward(const gs4d_heads_fwd *args, void *stream) {
    if (!args) return 1;
    const gs4d_heads_fwd &b = *args;
    if (b.P < 0 || (b.W != 64 && b.W != 128 && b.W != 256) || b.k < 1 || b.k > kHbMaxHeads) return 1;
    HfArgs A{};
    A.P = b.P, A.W = b.W, A.k = b.k, A.kW = b.k * b.W;
    int rows = 0;
    for (int i = 0; i < b.k; i++) {
        if (b.n[i] < 1 || b.n[i] > 16 * kHfMaxTiles || !b.w2[i] || !b.b2[i] || (b.P > 0 && !b.out[i])) return 1;
        if (((size_t)b.w2[i] & 15) != 0) return 1;
        A.n[i] = b.n[i], A.w2[i] = b.w2[i], A.b2[i] = b.b2[i], A.out[i] = b.out[i], A.roff[i] = rows;
        rows += b.n[i];
    }
    const size_t lds = 4 * (size_t)rows * (b.W + 4);
    if (lds > 64 * 1024) return 1;
    if (b.P == 0) return 0;
    if (!b.a || ((size_t)b.a & 15) != 0) return 1;
    const int nblk = (b.P + 15) / 16;
    const int nwg = std::max(1, std::min(1024, (nblk + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    int tiles[kHbMaxHeads];
    for (int i = 0; i < b.k; i++) tiles[i] = (b.n[i] + 15) / 16;
    auto is = [&](std::initializer_list<int> cfg) {
        if ((int)cfg.size() != b.k) return false;
        int i = 0;
        for (int t : cfg) if (tiles[i++] != t) return false;
        return true;
    };
    auto launch = [&](auto kernel, const HfArgs &args, const float *ap) {
        hipLaunchKernelGGL(kernel, dim3(nwg), dim3(kHfThreads), lds, s, args, ap);
    };
    // the reference's head sets: arguments/dynerf (pos, scales, rotations, opacity, shs: 3,3,4,1,48 outputs)
    // and the defaults (pos, scales, rotations); any other set runs head by head
    if (b.W == 128 && is({1, 1, 1, 1, 3})) launch(heads_fwd_kernel<128, 1, 1, 1, 1, 3>, A, b.a);
    else if (b.W == 64 && is({1, 1, 1, 1, 3})) launch(heads_fwd_kernel<64, 1, 1, 1, 1, 3>, A, b.a);
    else if (b.W == 64 && is({1, 1, 1})) launch(heads_fwd_kernel<64, 1, 1, 1>, A, b.a);
    else if (b.W == 128 && is({1, 1, 1})) launch(heads_fwd_kernel<128, 1, 1, 1>, A, b.a);
    else {
        for (int i = 0; i < b.k; i++) {  // one head per launch: a's row stride stays k W
            HfArgs H{};
            H.P = b.P, H.W = b.W, H.k = 1, H.n[0] = b.n[i], H.roff[0] = 0, H.w2[0] = b.w2[i], H.b2[0] = b.b2[i];
            H.out[0] = b.out[i];
            const float *ap = b.a + (size_t)i * b.W;
            const int t = tiles[i];
            H.kW = b.k * b.W;
            auto one = [&](auto k64, auto k128, auto k256) {
                if (b.W == 64) launch(k64, H, ap);
                else if (b.W == 128) launch(k128, H, ap);
                else launch(k256, H, ap);
            };
            if (t == 1) one(heads_fwd_kernel<64, 1>, heads_fwd_kernel<128, 1>, heads_fwd_kernel<256, 1>);
            else if (t == 2) one(heads_fwd_kernel<64, 2>, heads_fwd_kernel<128, 2>, heads_fwd_kernel<256, 2>);
            else if (t == 3) one(heads_fwd_kernel<64, 3>, heads_fwd_kernel<128, 3>, heads_fwd_kernel<256, 3>);
            else one(heads_fwd_kernel<64, 4>, heads_fwd_kernel<128, 4>, heads_fwd_kernel<256, 4>);
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: done once per (device, kernel set), and
// false when the device's per-workgroup LDS cannot hold `need` bytes
constexpr int kErrLds = 4;
static bool raise_lds_limit(const void *k0, const void *k1, int set, size_t need) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    static int state[3][64] = {};  // [set][device]: 0 unknown, 1 raised, 2 unavailable
    int &st = state[set][dev];
    if (st == 0) {
        int maxlds = 0;
        (void)hipDeviceGetAttribute(&maxlds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        const bool ok = hipFuncSetAttribute(k0, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
                        hipFuncSetAttribute(k1, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        (void)hipGetLastError();
        st = ok ? 1 : 2;
        if (ok && maxlds > 0 && (size_t)maxlds < 96 * 1024) st = 2;  // not a gfx950-class LDS
    }
    return st == 1 && need <= 160 * 1024;
}

// What gs4d_heads_block_forward and its bf16 form check and fill alike (their argument structs differ in the
// element type of a / hb / w1t only, so the common fields are passed in): 0 with A filled and *npad_max = the
// widest head's outputs rounded up to 16, or 1 for an invalid argument.
static int hbf_args(int P, int W, int k, const float *w1, const float *b1, const int *n, const float *const *w2,
                    const float *const *b2, float *const *out, HfArgs *A, int *npad_max) {
    if (P < 0 || (W != 64 && W != 128) || k < 1 || k > kHbMaxHeads || !w1 || !b1) return 1;
    A->P = P, A->W = W, A->k = k, A->kW = k * W;
    *npad_max = 0;
    for (int i = 0; i < k; i++) {
        if (n[i] < 1 || n[i] > 64 || !w2[i] || !b2[i] || (P > 0 && !out[i])) return 1;
        if (((size_t)w2[i] & 15) != 0) return 1;
        A->n[i] = n[i], A->w2[i] = w2[i], A->b2[i] = b2[i], A->out[i] = out[i];
        *npad_max = std::max(*npad_max, (n[i] + 15) & ~15);
    }
    if (((size_t)w1 & 15) != 0 || ((size_t)b1 & 15) != 0) return 1;
    return 0;
}

int gs4d_heads_block_forward(const gs4d_heads_block_fwd *args, void *stream) {
    if (!args) return 1;
    const gs4d_heads_block_fwd &b = *args;
    HfArgs A{};
    int npad_max = 0;
    if (hbf_args(b.P, b.W, b.k, b.w1, b.b1, b.n, b.w2, b.b2, b.out, &A, &npad_max)) return 1;
    if (b.P == 0) return 0;
    if (!b.h || !b.a || (((size_t)b.h | (size_t)b.a | (size_t)b.w1t) & 15) != 0) return 1;
    const size_t lds = 4 * ((size_t)(b.W + npad_max) * (b.W + 8) + b.W + npad_max);
    const int nblk = (b.P + 15) / 16;
    // ~1024 workgroups over the heads, one resident per CU (LDS): each stages its head's weights once and
    // takes a few blocks per wave (measured at P = 100k, k = 5: 237 / 218 / 207 us for 256 / 512 / 1024)
    // (16-wave workgroups measured no faster: 185-196 us for 256-1024 of them)
    const int per_head = std::max(1, std::min((nblk + 7) / 8, std::max(1, 1024 / b.k)));
    hipStream_t s = (hipStream_t)stream;
    // dynamic LDS above 64 KiB (gfx950: 160 KiB per CU), set once per device; a device that cannot give it
    // returns GS4D_TRAIN_ERR_LDS (the caller falls back to the GEMM formulation)
    if (!raise_lds_limit((const void *)heads_block_fwd_kernel<128>, (const void *)heads_block_fwd_kernel<64>, 0, lds))
        return kErrLds;
    if (b.W == 128)
        hipLaunchKernelGGL(heads_block_fwd_kernel<128>, dim3(per_head, b.k), dim3(kHbfThreads), lds, s, A, b.h, b.w1,
                           b.b1, b.a, b.w1t);
    else
        hipLaunchKernelGGL(heads_block_fwd_kernel<64>, dim3(per_head, b.k), dim3(kHbfThreads), lds, s, A, b.h, b.w1,
                           b.b1, b.a, b.w1t);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_heads_block_forward_bf16(const gs4d_heads_block_fwd_bf16 *args, void *stream) {
    if (!args) return 1;
    const gs4d_heads_block_fwd_bf16 &b = *args;
    HfArgs A{};
    int npad_max = 0;
    if (hbf_args(b.P, b.W, b.k, b.w1, b.b1, b.n, b.w2, b.b2, b.out, &A, &npad_max)) return 1;
    if (b.P == 0) return 0;
    // h NULL: hb is the input (h already rounded to bf16, gs4d_feature_relu_forward_hb)
    const bool hbin = !b.h;
    if ((hbin && !b.hb) || !b.a || (((size_t)b.h | (size_t)b.a | (size_t)b.hb | (size_t)b.w1t) & 15) != 0) return 1;
    const size_t lds = 2 * (size_t)(b.W + npad_max) * (b.W + 8) + 4 * (size_t)(b.W + npad_max);
    const int nblk = (b.P + 15) / 16;
    // two workgroups per CU (the bf16 kernel's VGPRs allow two 512-thread workgroups): one round of
    // workgroups, each loading and converting its head's weights once (measured 85 -> 80 us at P = 100k, five
    // heads, against the fp32 kernel's 1024 / k)
    const int per_head = std::max(1, std::min((nblk + 7) / 8, std::max(1, 2 * cu_count() / b.k)));
    hipStream_t s = (hipStream_t)stream;
    if (!raise_lds_limit((const void *)heads_block_fwd_bf16_kernel<128, false>,
                         (const void *)heads_block_fwd_bf16_kernel<64, false>, 1, lds) ||
        !raise_lds_limit((const void *)heads_block_fwd_bf16_kernel<128, true>,
                         (const void *)heads_block_fwd_bf16_kernel<64, true>, 2, lds))
        return kErrLds;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(per_head, b.k), dim3(kHbfThreads), lds, s, A, b.h, b.w1, b.b1, (__bf16 *)b.a,
                           (__bf16 *)b.hb, (__bf16 *)b.w1t);
    };
    if (b.W == 128) hbin ? go(heads_block_fwd_bf16_kernel<128, true>) : go(heads_block_fwd_bf16_kernel<128, false>);
    else hbin ? go(heads_block_fwd_bf16_kernel<64, true>) : go(heads_block_fwd_bf16_kernel<64, false>);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // extern "C"
