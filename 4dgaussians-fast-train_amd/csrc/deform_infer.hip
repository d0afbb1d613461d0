// deform_infer.hip -- the deformation network at inference (scene/deformation.py:51-55 feature_out, :73-78 the
// heads, :97-146 forward_dynamic's residual adds; gaussian_renderer/__init__.py:94-99 the activations): one launch
// from the field features of P points to the five tensors the rasterizer (or a PLY writer) consumes.  No
// intermediate is written: no h, no a, no deltas.  Entry point gs4d_deform_infer at the end of the file.
#include <math.h>

#include <algorithm>
#include <string>

#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {

constexpr int kDiRoles = 5;  // GS4D_ROLE_*: pos, scales, rot, opacity, shs
struct DiArgs {
    int P, K, k, activate;
    int role[kDiRoles], n[kDiRoles];  // per head
    const float *w2[kDiRoles];
    const float *b2[kDiRoles];
    const float *base[kDiRoles];  // per ROLE: xyz, s, r, o, f_dc
    const float *f_rest;
    float *out[kDiRoles];  // per ROLE: means, scales, rot, opac, shs
    int off;               // bit r: role r has no head, its base passes through
};

__device__ __forceinline__ float di_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// F.normalize: x / max(||x||_2, eps), the operations of deform_tail_fwd_kernel
__device__ __forceinline__ void di_normalize(float *q) {
    const float nrm = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
#pragma unroll
    for (int c = 0; c < 4; c++) q[c] = q[c] / nrm;
}

// The roles without a head: base -> output, activated when asked (the workgroups of grid row k).
__device__ void di_passthrough(const DiArgs &A, int threads) {
    const int nth = gridDim.x * threads, tid = blockIdx.x * threads + threadIdx.x;
    const bool act = A.activate != 0;
    for (int i = tid; i < A.P; i += nth) {
        if (A.off & (1 << GS4D_ROLE_POS)) {
#pragma unroll
            for (int c = 0; c < 3; c++) A.out[GS4D_ROLE_POS][3 * (size_t)i + c] = A.base[GS4D_ROLE_POS][3 * (size_t)i + c];
        }
        if (A.off & (1 << GS4D_ROLE_SCALES)) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float v = A.base[GS4D_ROLE_SCALES][3 * (size_t)i + c];
                A.out[GS4D_ROLE_SCALES][3 * (size_t)i + c] = act ? expf(v) : v;
            }
        }
        if (A.off & (1 << GS4D_ROLE_ROT)) {
            float q[4];
#pragma unroll
            for (int c = 0; c < 4; c++) q[c] = A.base[GS4D_ROLE_ROT][4 * (size_t)i + c];
            if (act) di_normalize(q);
#pragma unroll
            for (int c = 0; c < 4; c++) A.out[GS4D_ROLE_ROT][4 * (size_t)i + c] = q[c];
        }
        if (A.off & (1 << GS4D_ROLE_OPACITY)) {
            const float v = A.base[GS4D_ROLE_OPACITY][i];
            A.out[GS4D_ROLE_OPACITY][i] = act ? di_sigmoid(v) : v;
        }
    }
    if (A.off & (1 << GS4D_ROLE_SHS)) {
        // shs = cat(f_dc, f_rest): the (P, 3K) values as one flat, coalesced range (P * 3K < 2^31: host check)
        const int row = 3 * A.K, n = A.P * row;
        for (int e = tid; e < n; e += nth) {
            const int g = e / row, k = e - g * row;
            A.out[GS4D_ROLE_SHS][e] =
                k < 3 ? A.base[GS4D_ROLE_SHS][3 * (size_t)g + k] : A.f_rest[(size_t)g * (row - 3) + (k - 3)];
        }
    }
}

// ---- one head of the network over the 16-point blocks of a workgroup, on the f32 MFMA (v_mfma_f32_16x16x4_f32,
// exact f32 products), in the TRANSPOSED layout of heads_block_fwd_kernel (mlp_heads_forward.hip): features along the
// MFMA rows, the 16 points along its columns, so each layer's accumulators are the next layer's B operand as
// they stand -- in k-step (t, v) lane l = (q = l >> 4, c = l & 15) supplies feature 16 t + 4 q + v of point c, the
// v-th register of its t-th accumulator.  Three layers: h^T = relu(Wf feat^T + bf) (recomputed per head: F W MACs
// against the W W of the next layer, and no h in memory), a^T = relu(W1 h^T + b1), d^T = W2 a^T + b2; then the
// residual add and the activation on the lane's own registers: lane (q, c) holds outputs 16 j + 4 q + 0..3 of point
// c, so a rotation's four values sit in one lane (the normalise needs no shuffle) and the 48 SH values of a point
// are twelve aligned float4.  NJ: 16-output tiles of the head (1: pos / scales / rot / opacity, 3: shs).
// The next block's feat and base values are loaded (unconditionally, rows past P read row P - 1) before this
// block's MFMAs, as heads_block_fwd_kernel loads its h.
constexpr int kDiThreads = 512;
template <int F, int W, int NJ>
__device__ __forceinline__ void di_head(const DiArgs &A, int head, const float *__restrict__ feat, const float *s_wf,
                                        const float *s_bf, const float *s_w1, const float *s_b1, const float *s_w2,
                                        const float *s_b2) {
    constexpr int NT = W / 16, FT = F / 16, WS = W + 8, FS = F + 8, NW = kDiThreads / 64;
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4,
              c = lane & 15;
    const int role = A.role[head], n = A.n[head];
    const bool act = A.activate != 0;
    const float *bp = A.base[role];
    const float *f_rest = A.f_rest;
    float *out = A.out[role];
    const int nblk = (A.P + 15) / 16;
    const int stride = gridDim.x * NW;
    float4 fn[FT];
    float bn[NJ][4];
    auto load_next = [&](int blk) {
        const int pt = min(blk * 16 + c, A.P - 1);
#pragma unroll
        for (int t = 0; t < FT; t++) fn[t] = *reinterpret_cast<const float4 *>(feat + (size_t)pt * F + 16 * t + 4 * q);
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                // output e of the head (clamped to a valid one: the load is unconditional, the value unused)
                const int e = min(16 * j + 4 * q + r, n - 1);
                if (NJ == 3)  // shs: cat(f_dc (P, 1, 3), f_rest (P, 15, 3))
                    bn[j][r] = e < 3 ? bp[3 * (size_t)pt + e] : f_rest[(size_t)pt * 45 + (e - 3)];
                else
                    bn[j][r] = bp[(size_t)pt * n + e];
            }
    };
    int blk = blockIdx.x * NW + wv;
    load_next(blk);
    for (; blk < nblk; blk += stride) {
        float4 fv[FT];
        float bv[NJ][4];
#pragma unroll
        for (int t = 0; t < FT; t++) fv[t] = fn[t];
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) bv[j][r] = bn[j][r];
        load_next(blk + stride);
        // h^T (W x 16) = relu(Wf feat^T + bf)
        f4v hh[NT];
#pragma unroll
        for (int m = 0; m < NT; m++) hh[m] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < FT; t++) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int m = 0; m < NT; m++) {
                const float4 av = *reinterpret_cast<const float4 *>(s_wf + (16 * m + c) * FS + 16 * t + 4 * q);
                hh[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, fv[t].x, hh[m], 0, 0, 0);
                hh[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, fv[t].y, hh[m], 0, 0, 0);
                hh[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, fv[t].z, hh[m], 0, 0, 0);
                hh[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, fv[t].w, hh[m], 0, 0, 0);
            }
        }
#pragma unroll
        for (int m = 0; m < NT; m++) {
            const float4 bb = *reinterpret_cast<const float4 *>(s_bf + 16 * m + 4 * q);
            hh[m][0] = fmaxf(hh[m][0] + bb.x, 0.f);
            hh[m][1] = fmaxf(hh[m][1] + bb.y, 0.f);
            hh[m][2] = fmaxf(hh[m][2] + bb.z, 0.f);
            hh[m][3] = fmaxf(hh[m][3] + bb.w, 0.f);
        }
        // a^T (W x 16) = relu(W1 h^T + b1), B operand = hh
        f4v acc[NT];
#pragma unroll
        for (int m = 0; m < NT; m++) acc[m] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; t++) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int m = 0; m < NT; m++) {
                const float4 av = *reinterpret_cast<const float4 *>(s_w1 + (16 * m + c) * WS + 16 * t + 4 * q);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, hh[t][0], acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, hh[t][1], acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, hh[t][2], acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, hh[t][3], acc[m], 0, 0, 0);
            }
        }
#pragma unroll
        for (int m = 0; m < NT; m++) {
            const float4 bb = *reinterpret_cast<const float4 *>(s_b1 + 16 * m + 4 * q);
            acc[m][0] = fmaxf(acc[m][0] + bb.x, 0.f);
            acc[m][1] = fmaxf(acc[m][1] + bb.y, 0.f);
            acc[m][2] = fmaxf(acc[m][2] + bb.z, 0.f);
            acc[m][3] = fmaxf(acc[m][3] + bb.w, 0.f);
        }
        // d^T (16 NJ x 16) = W2 a^T + b2, then base + d and the activation
        const int pt = blk * 16 + c;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            f4v o = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < NT; m++) {
                const float4 wv4 = *reinterpret_cast<const float4 *>(s_w2 + (16 * j + c) * WS + 16 * m + 4 * q);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.x, acc[m][0], o, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.y, acc[m][1], o, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.z, acc[m][2], o, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.w, acc[m][3], o, 0, 0, 0);
            }
            const float4 bb = *reinterpret_cast<const float4 *>(s_b2 + 16 * j + 4 * q);
            float v[4] = {bv[j][0] + (o[0] + bb.x), bv[j][1] + (o[1] + bb.y), bv[j][2] + (o[2] + bb.z),
                          bv[j][3] + (o[3] + bb.w)};
            if (NJ == 3) {  // shs (P, 16, 3): values 16 j + 4 q .. + 3 of the point's 48, one aligned float4
                if (pt < A.P)
                    *reinterpret_cast<float4 *>(out + (size_t)pt * 48 + 16 * j + 4 * q) =
                        make_float4(v[0], v[1], v[2], v[3]);
            } else if (q == 0 && pt < A.P) {  // n <= 4: the head's outputs are lane (0, c)'s registers
                if (role == GS4D_ROLE_ROT) {
                    if (act) di_normalize(v);
                    *reinterpret_cast<float4 *>(out + 4 * (size_t)pt) = make_float4(v[0], v[1], v[2], v[3]);
                } else if (role == GS4D_ROLE_OPACITY) {
                    out[pt] = act ? di_sigmoid(v[0]) : v[0];
                } else {
                    const bool ex = act && role == GS4D_ROLE_SCALES;
#pragma unroll
                    for (int r = 0; r < 3; r++) out[3 * (size_t)pt + r] = ex ? expf(v[r]) : v[r];
                }
            }
        }
    }
}

// Workgroup (x, head i) for i < k: Wf, W1_i and W2_i staged in LDS (row stride + 8 floats, as
// heads_block_fwd_kernel), its 8 waves each taking 16-point blocks; one workgroup per CU (LDS).  Grid row k, when
// present, passes the roles without a head through.
template <int F, int W>
__global__ __launch_bounds__(kDiThreads) void deform_infer_kernel(DiArgs A, const float *__restrict__ feat,
                                                                  const float *__restrict__ wf,
                                                                  const float *__restrict__ bf,
                                                                  const float *__restrict__ w1,
                                                                  const float *__restrict__ b1) {
    const int head = blockIdx.y;
    if (head >= A.k) {
        di_passthrough(A, kDiThreads);
        return;
    }
    constexpr int WS = W + 8, FS = F + 8;
    extern __shared__ float4 s_v[];
    const int n = A.n[head], npad = (n + 15) & ~15;
    float *s_wf = reinterpret_cast<float *>(s_v);  // W rows x FS
    float *s_w1 = s_wf + W * FS;                   // W rows x WS
    float *s_bf = s_w1 + W * WS;                   // W
    float *s_b1 = s_bf + W;                        // W
    float *s_w2 = s_b1 + W;                        // npad rows x WS (rows >= n zero)
    float *s_b2 = s_w2 + npad * WS;                // npad
    const float *w1i = w1 + (size_t)head * W * W;
    for (int e = threadIdx.x; e < W * F / 4; e += kDiThreads) {
        const int row = e / (F / 4), c4 = e % (F / 4);
        reinterpret_cast<float4 *>(s_wf + row * FS)[c4] = reinterpret_cast<const float4 *>(wf + (size_t)row * F)[c4];
    }
    for (int e = threadIdx.x; e < W * W / 4; e += kDiThreads) {
        const int row = e / (W / 4), c4 = e % (W / 4);
        reinterpret_cast<float4 *>(s_w1 + row * WS)[c4] = reinterpret_cast<const float4 *>(w1i + (size_t)row * W)[c4];
    }
    for (int e = threadIdx.x; e < W; e += kDiThreads) {
        s_bf[e] = bf[e];
        s_b1[e] = b1[head * W + e];
    }
    for (int e = threadIdx.x; e < npad * (W / 4); e += kDiThreads) {
        const int row = e / (W / 4), c4 = e % (W / 4);
        reinterpret_cast<float4 *>(s_w2 + row * WS)[c4] =
            row < n ? reinterpret_cast<const float4 *>(A.w2[head] + (size_t)row * W)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int e = threadIdx.x; e < npad; e += kDiThreads) s_b2[e] = e < n ? A.b2[head][e] : 0.f;
    __syncthreads();
    if (npad == 48)
        di_head<F, W, 3>(A, head, feat, s_wf, s_bf, s_w1, s_b1, s_w2, s_b2);
    else
        di_head<F, W, 1>(A, head, feat, s_wf, s_bf, s_w1, s_b1, s_w2, s_b2);
}

// bytes of LDS for the widest head (outputs rounded up to 16): the strides of deform_infer_kernel
static size_t di_lds_bytes(int F, int W, int npad) {
    return 4 * ((size_t)W * (F + 8) + (size_t)W * (W + 8) + 2 * (size_t)W + (size_t)npad * (W + 8) + npad);
}

// dynamic LDS above 64 KiB (gfx950: 160 KiB per workgroup): raised once per (device, kernel); false when the device
// cannot give it.  slot: the kernel's index among the kDiKernels instantiations gs4d_deform_infer launches
constexpr int kDiKernels = 4;
static bool di_raise_lds(const void *kern, int slot, size_t need) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    static int state[kDiKernels][64] = {};  // 0 unknown, 1 raised, 2 unavailable
    if (slot < 0 || slot >= kDiKernels) return false;
    int &st = state[slot][dev];
    if (st == 0) {
        int maxlds = 0;
        (void)hipDeviceGetAttribute(&maxlds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        const bool ok = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        (void)hipGetLastError();
        st = ok && (maxlds <= 0 || (size_t)maxlds >= 96 * 1024) ? 1 : 2;
    }
    return st == 1 && need <= 160 * 1024;
}

}  // namespace gs4d

using namespace gs4d;

extern "C" {

int gs4d_deform_infer(const gs4d_deform_infer_args *args, void *stream) {
    auto bad = [](const std::string &what) { return train_fail(1, "deform_infer: " + what); };
    if (!args) return bad("null arguments");
    const gs4d_deform_infer_args &b = *args;
    if (b.P < 0) return bad("P < 0");
    const bool shape_ok = (b.F == 32 && b.W == 128) || (b.F == 48 && b.W == 128) || (b.F == 64 && b.W == 64) ||
                          (b.F == 32 && b.W == 64);
    if (!shape_ok)
        return bad("(F, W) = (" + std::to_string(b.F) + ", " + std::to_string(b.W) +
                   ") is not one of (32, 128), (48, 128), (64, 64), (32, 64)");
    if (b.k < 1 || b.k > kDiRoles) return bad("k = " + std::to_string(b.k) + " heads (1..5)");
    if (b.K < 1) return bad("K < 1");
    static const int role_n[kDiRoles] = {3, 3, 4, 1, 48};
    DiArgs A{};
    A.P = b.P, A.K = b.K, A.k = b.k, A.activate = b.activate != 0;
    int seen = 0, npad_max = 0;
    for (int i = 0; i < b.k; i++) {
        const int r = b.role[i];
        if (r < 0 || r >= kDiRoles) return bad("role " + std::to_string(r) + " of head " + std::to_string(i));
        if (seen & (1 << r)) return bad("role " + std::to_string(r) + " given twice");
        seen |= 1 << r;
        if (b.n[i] != role_n[r])
            return bad("head " + std::to_string(i) + " has n = " + std::to_string(b.n[i]) + ", its role " +
                       std::to_string(r) + " has " + std::to_string(role_n[r]));
        if (r == GS4D_ROLE_SHS && b.K != 16) return bad("the shs head needs K = 16, got " + std::to_string(b.K));
        if (!b.w2[i] || !b.b2[i]) return bad("null second-layer weight or bias of head " + std::to_string(i));
        if (((size_t)b.w2[i] & 15) != 0) return bad("W2 must be 16-byte aligned");
        A.role[i] = r, A.n[i] = b.n[i], A.w2[i] = b.w2[i], A.b2[i] = b.b2[i];
        npad_max = std::max(npad_max, (b.n[i] + 15) & ~15);
    }
    A.off = ~seen & ((1 << kDiRoles) - 1);
    if (!b.wf || !b.bf || !b.w1 || !b.b1) return bad("null weight or bias");
    if ((((size_t)b.wf | (size_t)b.w1) & 15) != 0) return bad("Wf and W1 must be 16-byte aligned");
    if ((int64_t)b.P * 3 * b.K > INT32_MAX) return bad("P * 3K exceeds 2^31 - 1");
    if (b.P > 0) {
        if (!b.feat) return bad("null feat");
        if (!b.xyz || !b.s || !b.r || !b.o || !b.f_dc || (b.K > 1 && !b.f_rest)) return bad("null base tensor");
        if (!b.means || !b.scales || !b.rot || !b.opac || !b.shs) return bad("null output");
        if ((((size_t)b.feat | (size_t)b.rot | (size_t)b.shs) & 15) != 0)
            return bad("feat, rot and shs must be 16-byte aligned");
    }
    if (b.P == 0) return 0;
    A.base[GS4D_ROLE_POS] = b.xyz, A.base[GS4D_ROLE_SCALES] = b.s, A.base[GS4D_ROLE_ROT] = b.r;
    A.base[GS4D_ROLE_OPACITY] = b.o, A.base[GS4D_ROLE_SHS] = b.f_dc, A.f_rest = b.f_rest;
    A.out[GS4D_ROLE_POS] = b.means, A.out[GS4D_ROLE_SCALES] = b.scales, A.out[GS4D_ROLE_ROT] = b.rot;
    A.out[GS4D_ROLE_OPACITY] = b.opac, A.out[GS4D_ROLE_SHS] = b.shs;
    const size_t lds = di_lds_bytes(b.F, b.W, npad_max);
    const int nblk = (b.P + 15) / 16;
    // ~1024 workgroups over the heads, each staging its weights once (gs4d_heads_block_forward's measured choice)
    const int per_head = std::max(1, std::min((nblk + 7) / 8, std::max(1, 1024 / b.k)));
    const dim3 grid(per_head, b.k + (A.off ? 1 : 0));
    hipStream_t s = (hipStream_t)stream;
    auto go = [&](auto kern, int slot) {
        if (lds > 64 * 1024 && !di_raise_lds((const void *)kern, slot, lds))
            return train_fail(GS4D_TRAIN_ERR_LDS, "deform_infer: the device cannot give the kernel " +
                                                      std::to_string(lds) + " bytes of LDS");
        hipLaunchKernelGGL(kern, grid, dim3(kDiThreads), lds, s, A, b.feat, b.wf, b.bf, b.w1, b.b1);
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : train_fail(3, std::string("deform_infer: ") + hipGetErrorString(e));
    };
    if (b.F == 32 && b.W == 128) return go(deform_infer_kernel<32, 128>, 0);
    if (b.F == 64 && b.W == 64) return go(deform_infer_kernel<64, 64>, 1);
    if (b.F == 32 && b.W == 64) return go(deform_infer_kernel<32, 64>, 2);
    return go(deform_infer_kernel<48, 128>, 3);
}

}  // extern "C"
