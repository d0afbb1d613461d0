// mlp_feature.hip -- the deformation MLP's first layer (scene/deformation.py:51-55, feature_out with
// defor_depth <= 1): h = relu(x W^T + b) forward and its backward, both on the f32 MFMA, with their
// gs4d_feature_relu_* entry points at the end of the file.
#include <math.h>

#include <algorithm>

#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {

// ---- the deformation field's first layer, backward (scene/deformation.py:51-55 with defor_depth <= 1:
// hidden = feature_out(x) = x W^T + b; every head starts with ReLU, so the heads read h = relu(hidden)).
// Given g = dL/dh, ONE pass over the rows forms dz = g * (h > 0) and both GEMMs on the f32 MFMA
// (v_mfma_f32_16x16x4_f32: exact f32, a k-ordered fma chain):
//   dx = dz W   (rows x Fin)   and   dW += dz^T x,  db += column sums of dz  (per-wave partials).
// A wave takes 16-row blocks: g and h rows are read coalesced (lanes along the outputs), dz is staged
// in an LDS tile, W lives in LDS.  At the end the
// workgroup's waves add their dW / db partials in wave order and a second launch sums the workgroups'
// partials in workgroup order (deterministic).
constexpr int kFbThreads = 256, kFbRows = 16;

// LATEX (the (48, 128) instantiation): the next block's x loads are issued after this block's dW MFMAs instead of
// before its dx MFMAs, so x needs one register set (xb) and no copy (xc), and the kernel is held to two waves per
// SIMD (252 registers where the plain body takes 168 + 108 and one wave).  The MFMA chains, and so every bit of the
// results, are the same; measured 50.6 us against the plain body's 63.1 at P = 100k.
// -DGS4D_FB48_LATE_X=0 builds the plain body for that shape, to measure the two against each other again.
#ifndef GS4D_FB48_LATE_X
#define GS4D_FB48_LATE_X 1
#endif
constexpr bool kFb48LateX = GS4D_FB48_LATE_X != 0;
template <int FIN, int FOUT, bool LATEX = false>
__global__ __launch_bounds__(kFbThreads, LATEX ? 2 : 1) void feature_bwd_kernel(int P, const float *__restrict__ g,
                                                                 const float *__restrict__ h,
                                                                 const float *__restrict__ x,
                                                                 const float *__restrict__ w, float *__restrict__ dx,
                                                                 float *__restrict__ part) {
    constexpr int NB = FIN / 16, MB = FOUT / 16, NW = kFbThreads / 64;
    // tile row stride = 17 (mod 64) words: the 16-row column reads of dx and the 4-row x 16-column reads
    // of dW both spread over the LDS banks
    constexpr int TS = FOUT + 17;
    constexpr int PER = FOUT * FIN + FOUT;  // one partial: dW (row-major) then db
    __shared__ float s_w[FOUT * FIN + FOUT];
    __shared__ float s_t[NW][kFbRows * TS];
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < FOUT * FIN / 4; i += kFbThreads)
        reinterpret_cast<float4 *>(s_w)[i] = reinterpret_cast<const float4 *>(w)[i];
    __syncthreads();
    float *t = s_t[wv];
    f4v accw[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; m++)
#pragma unroll
        for (int n = 0; n < NB; n++) accw[m][n] = f4v{0.f, 0.f, 0.f, 0.f};
    float db0 = 0.f, db1 = 0.f;                  // this lane's output pair (o, o + 1)
    const int o = (2 * lane) % FOUT, rofs = (2 * lane) / FOUT;
    constexpr int RPI = 128 / FOUT;              // rows per coalesced load instruction
    const int nblk = (P + kFbRows - 1) / kFbRows;
    // block loads (g, h rows: lanes along the outputs; x rows as the B operand of dW:
    // B[k = row 4s + (l >> 4)][n = 16 nb + (l & 15)]), issued one block ahead of their use
    constexpr int NIT = kFbRows / RPI;
    float2 gv[NIT], hv[NIT];
    float xb[4][NB];
    // rows past P (and the prefetch past the last block) read row P - 1, masked when the block comes up:
    // unconditional loads let the compiler's waits count exactly the loads issued after a block's (with a
    // branch around them it waited for every load in flight, the next block's prefetch included)
    auto load_x = [&](int blk) {
        const int r0 = blk * kFbRows;
#pragma unroll
        for (int st = 0; st < 4; st++) {
            const int r = min(r0 + 4 * st + (lane >> 4), P - 1);
#pragma unroll
            for (int n = 0; n < NB; n++) xb[st][n] = x[(size_t)r * FIN + 16 * n + (lane & 15)];
        }
    };
    auto load_block = [&](int blk) {
        const int r0 = blk * kFbRows;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int r = min(r0 + it * RPI + rofs, P - 1);
            gv[it] = *reinterpret_cast<const float2 *>(g + (size_t)r * FOUT + o);
            hv[it] = *reinterpret_cast<const float2 *>(h + (size_t)r * FOUT + o);
        }
        if constexpr (!LATEX) load_x(blk);
    };
    const int stride = gridDim.x * NW;
    int blk = blockIdx.x * NW + wv;
    load_block(blk);
    if constexpr (LATEX) load_x(blk);
    for (; blk < nblk; blk += stride) {
        const int r0 = blk * kFbRows;
        // dz = g * (h > 0) into the tile, column sums into db
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int row = it * RPI + rofs;
            const bool ok = r0 + row < P;
            const float d0 = ok && hv[it].x > 0.f ? gv[it].x : 0.f, d1 = ok && hv[it].y > 0.f ? gv[it].y : 0.f;
            db0 += d0;
            db1 += d1;
            t[row * TS + o] = d0;
            t[row * TS + o + 1] = d1;
        }
        float xc[LATEX ? 1 : 4][NB];
        if constexpr (!LATEX) {
#pragma unroll
            for (int st = 0; st < 4; st++) {
                const bool ok = r0 + 4 * st + (lane >> 4) < P;
#pragma unroll
                for (int n = 0; n < NB; n++) xc[st][n] = ok ? xb[st][n] : 0.f;
            }
        }
        load_block(blk + stride);  // the next block's loads fly while this one runs on the MFMA
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the tile is written (LDS is in order per wave)
        __builtin_amdgcn_wave_barrier();
        // dx = dz W: A[row l & 15][k = o 4s + (l >> 4)], B[k = o][n = 16 nb + (l & 15)]
        f4v accx[NB];
#pragma unroll
        for (int n = 0; n < NB; n++) accx[n] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int st = 0; st < FOUT / 4; st++) {
            const int ok = 4 * st + (lane >> 4);
            const float av = t[(lane & 15) * TS + ok];
#pragma unroll
            for (int n = 0; n < NB; n++)
                accx[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_w[ok * FIN + 16 * n + (lane & 15)], accx[n], 0, 0, 0);
        }
        // C[row (l >> 4) * 4 + i][col 16 nb + (l & 15)]
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = r0 + (lane >> 4) * 4 + i;
            if (r < P) {
#pragma unroll
                for (int n = 0; n < NB; n++) dx[(size_t)r * FIN + 16 * n + (lane & 15)] = accx[n][i];
            }
        }
        // dW += dz^T x: A[m = o 16 mb + (l & 15)][k = row 4s + (l >> 4)], B = xb
#pragma unroll
        for (int st = 0; st < 4; st++) {
            if constexpr (LATEX) {  // the rows past P masked as they are used
                const bool ok = r0 + 4 * st + (lane >> 4) < P;
#pragma unroll
                for (int n = 0; n < NB; n++) xc[0][n] = ok ? xb[st][n] : 0.f;
            }
#pragma unroll
            for (int m = 0; m < MB; m++) {
                const float av = t[(4 * st + (lane >> 4)) * TS + 16 * m + (lane & 15)];
#pragma unroll
                for (int n = 0; n < NB; n++)
                    accw[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc[LATEX ? 0 : st][n], accw[m][n], 0, 0, 0);
            }
        }
        if constexpr (LATEX) load_x(blk + stride);
        __builtin_amdgcn_wave_barrier();  // the tile's reads are done before the next block overwrites it
    }
    // the waves' partials added in wave order in LDS (W is no longer needed there)
    for (int q = 0; q < NW; q++) {
        __syncthreads();
        if (wv == q) {
#pragma unroll
            for (int m = 0; m < MB; m++)
#pragma unroll
                for (int n = 0; n < NB; n++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        float &dst = s_w[(16 * m + (lane >> 4) * 4 + i) * FIN + 16 * n + (lane & 15)];
                        dst = q == 0 ? accw[m][n][i] : dst + accw[m][n][i];
                    }
            // db: lanes with the same outputs (RPI > 1) add in lane order
#pragma unroll
            for (int rr = 0; rr < RPI; rr++) {
                if (rofs == rr) {
                    float &d0 = s_w[FOUT * FIN + o], &d1 = s_w[FOUT * FIN + o + 1];
                    d0 = (q == 0 && rr == 0) ? db0 : d0 + db0;
                    d1 = (q == 0 && rr == 0) ? db1 : d1 + db1;
                }
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __syncthreads();
    float *dst = part + (size_t)blockIdx.x * PER;
    for (int i = threadIdx.x; i < PER; i += kFbThreads) dst[i] = s_w[i];
}

// dW / db = the workgroups' partials summed in workgroup order: 16 outputs per workgroup, 16 threads per
// output each summing a strided slice of the partials (all loads independent), then the 16 slices
// added in slice order
__global__ __launch_bounds__(256) void feature_bwd_reduce_kernel(int nwg, int per, int nwb, const float *__restrict__ part,
                                                                 float *__restrict__ dw, float *__restrict__ db) {
    __shared__ float s_sum[16][17];
    const int oi = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + oi;
    float acc = 0.f;
    if (i < per) {
        int k = sl;
        for (; k + 112 < nwg; k += 128) {  // eight loads in flight per thread (the kernel is latency-bound)
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = part[(size_t)(k + 16 * u) * per + i];
#pragma unroll
            for (int u = 0; u < 8; u++) acc += x[u];
        }
        for (; k + 48 < nwg; k += 64) {
            const float a0 = part[(size_t)k * per + i], a1 = part[(size_t)(k + 16) * per + i];
            const float a2 = part[(size_t)(k + 32) * per + i], a3 = part[(size_t)(k + 48) * per + i];
            acc += a0;
            acc += a1;
            acc += a2;
            acc += a3;
        }
        for (; k < nwg; k += 16) acc += part[(size_t)k * per + i];
    }
    s_sum[sl][oi] = acc;
    __syncthreads();
    if (sl == 0 && i < per) {
        float t = 0.f;
        for (int q = 0; q < 16; q++) t += s_sum[q][oi];
        if (i < nwb) dw[i] = t;
        else db[i - nwb] = t;
    }
}

// ---- the deformation field's first layer, forward: h = relu(x W^T + b) (P, FOUT) from x (P, FIN) on the
// f32 MFMA.  Per 16-row block: lane group q = l >> 4 reads columns 4q..4q+3 of its row l & 15 of a 16-column
// K chunk as one float4 (the MFMA's k index in step s is column 4q + s), the matching W rows (LDS, row stride
// FIN + 4) are the B operand, FOUT / 16 accumulators; bias and ReLU on the way out.
// hb (nullable): h rounded to bf16 as well, (ceil(P / 16) * 16, FOUT): the bf16 heads block reads it instead of
// converting h once per head; its padding rows hold row P - 1's values (every x load reads row min(r, P - 1)).
template <int FIN, int FOUT>
__global__ __launch_bounds__(kFbThreads) void feature_fwd_kernel(int P, const float *__restrict__ x,
                                                                 const float *__restrict__ w,
                                                                 const float *__restrict__ b, float *__restrict__ h,
                                                                 __bf16 *__restrict__ hb) {
    constexpr int WS = FIN + 4, NT = FOUT / 16, NW = kFbThreads / 64;
    __shared__ float s_w[FOUT * WS];
    for (int e = threadIdx.x; e < FOUT * FIN / 4; e += kFbThreads) {
        const int row = e / (FIN / 4), c4 = e % (FIN / 4);
        reinterpret_cast<float4 *>(s_w + row * WS)[c4] = reinterpret_cast<const float4 *>(w + (size_t)row * FIN)[c4];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), q = lane >> 4, c = lane & 15;
    float bias[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) bias[t] = b[16 * t + c];
    const int nblk = (P + 15) / 16;
    for (int blk = blockIdx.x * NW + wv; blk < nblk; blk += gridDim.x * NW) {
        const int r0 = blk * 16, ra = r0 + c;
        float4 xv[FIN / 16];
#pragma unroll
        for (int kc = 0; kc < FIN / 16; kc++)
            xv[kc] = *reinterpret_cast<const float4 *>(x + (size_t)min(ra, P - 1) * FIN + 16 * kc + 4 * q);
        f4v acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) acc[t] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < FIN / 16; kc++) {
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const float4 bv = *reinterpret_cast<const float4 *>(s_w + (16 * t + c) * WS + 16 * kc + 4 * q);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[kc].x, bv.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[kc].y, bv.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[kc].z, bv.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[kc].w, bv.w, acc[t], 0, 0, 0);
            }
        }
        // C[row 4q + j][col 16 t + c]
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = r0 + 4 * q + j;
            if (r < P) {
#pragma unroll
                for (int t = 0; t < NT; t++) h[(size_t)r * FOUT + 16 * t + c] = fmaxf(acc[t][j] + bias[t], 0.f);
            }
            if (hb) {
#pragma unroll
                for (int t = 0; t < NT; t++) hb[(size_t)r * FOUT + 16 * t + c] = (__bf16)fmaxf(acc[t][j] + bias[t], 0.f);
            }
        }
    }
}

}  // namespace gs4d

using namespace gs4d;

extern "C" {

// the (Fin, Fout) the two kernels are instantiated for: DyNeRF / multipleview, HyperNeRF / DyCheck, D-NeRF, small
static bool fb_shape_ok(int Fin, int Fout) {
    return (Fin == 32 && Fout == 128) || (Fin == 48 && Fout == 128) || (Fin == 64 && Fout == 64) ||
           (Fin == 32 && Fout == 64);
}
static int fb_grid(int P) {
    const int nblk = (P + kFbRows - 1) / kFbRows;
    return std::max(1, std::min(512, (nblk + 3) / 4));
}
size_t gs4d_feature_relu_backward_scratch_bytes(int P, int Fin, int Fout) {
    return 4 * (size_t)fb_grid(std::max(P, 0)) * ((size_t)Fout * Fin + Fout) + 256;
}

int gs4d_feature_relu_backward(int P, int Fin, int Fout, const float *g, const float *h, const float *x,
                               const float *w, float *dx, float *dw, float *db, void *scratch, void *stream) {
    if (P < 0 || !w || !dw || !db || !scratch) return 1;
    if (!fb_shape_ok(Fin, Fout)) return 1;
    if (P > 0 && (!g || !h || !x || !dx)) return 1;
    if ((((size_t)g | (size_t)h | (size_t)w) & 15) != 0) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int nwg = fb_grid(P), per = Fout * Fin + Fout;
    float *part = (float *)align_up((size_t)scratch, 256);
    if (P == 0) {
        if (hipMemsetAsync(part, 0, 4 * (size_t)per, s) != hipSuccess) return 3;
    } else if (Fin == 32 && Fout == 128) {
        hipLaunchKernelGGL((feature_bwd_kernel<32, 128>), dim3(nwg), dim3(kFbThreads), 0, s, P, g, h, x, w, dx, part);
    } else if (Fin == 48) {
        hipLaunchKernelGGL((feature_bwd_kernel<48, 128, kFb48LateX>), dim3(nwg), dim3(kFbThreads), 0, s, P, g, h, x, w, dx,
                           part);
    } else if (Fin == 64) {
        hipLaunchKernelGGL((feature_bwd_kernel<64, 64>), dim3(nwg), dim3(kFbThreads), 0, s, P, g, h, x, w, dx, part);
    } else {
        hipLaunchKernelGGL((feature_bwd_kernel<32, 64>), dim3(nwg), dim3(kFbThreads), 0, s, P, g, h, x, w, dx, part);
    }
    hipLaunchKernelGGL(feature_bwd_reduce_kernel, dim3((per + 15) / 16), dim3(256), 0, s, P == 0 ? 1 : nwg, per,
                       Fout * Fin, (const float *)part, dw, db);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_feature_relu_forward_hb(int P, int Fin, int Fout, const float *x, const float *w, const float *b, float *h,
                                 uint16_t *hb, void *stream) {
    if (P < 0 || !w || !b) return 1;
    if (!fb_shape_ok(Fin, Fout)) return 1;
    if (P == 0) return 0;
    if (!x || !h || (((size_t)x | (size_t)w) & 15) != 0) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int nwg = std::max(1, std::min(1024, ((P + 15) / 16 + 3) / 4));
    __bf16 *hbb = reinterpret_cast<__bf16 *>(hb);
    if (Fin == 32 && Fout == 128)
        hipLaunchKernelGGL((feature_fwd_kernel<32, 128>), dim3(nwg), dim3(kFbThreads), 0, s, P, x, w, b, h, hbb);
    else if (Fin == 48)
        hipLaunchKernelGGL((feature_fwd_kernel<48, 128>), dim3(nwg), dim3(kFbThreads), 0, s, P, x, w, b, h, hbb);
    else if (Fin == 64)
        hipLaunchKernelGGL((feature_fwd_kernel<64, 64>), dim3(nwg), dim3(kFbThreads), 0, s, P, x, w, b, h, hbb);
    else
        hipLaunchKernelGGL((feature_fwd_kernel<32, 64>), dim3(nwg), dim3(kFbThreads), 0, s, P, x, w, b, h, hbb);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
int gs4d_feature_relu_forward(int P, int Fin, int Fout, const float *x, const float *w, const float *b, float *h,
                              void *stream) {
    return gs4d_feature_relu_forward_hb(P, Fin, Fout, x, w, b, h, nullptr, stream);
}

}  // extern "C"
