// train_tail.hip -- the train step after the rasterizer: fused L1 loss, the
// densification statistics, a multi-tensor Adam and the HexPlane regularisers, and the small streaming passes
// around them: the deformation tail with the activations, the HexPlane field's input points, the row surgery
// of densification / pruning and the slice sum of the split-K weight gradients.  Kernels first, their gs4d_*
// entry points (argument checks, launch geometry) at the end of the file.  The deformation MLP lives in
// mlp_feature.hip, mlp_heads_forward.hip, mlp_heads_backward.hip and mlp_gemm.hip.
//
// Reference: utils/loss_utils.py:20-21 (l1_loss) with the L1 gradient torch's autograd derives
// (sign(x - y) / N), train.py:346-349 + scene/gaussian_model.py:521-523 (densification statistics),
// and torch.optim.Adam as configured by scene/gaussian_model.py:184 (betas (0.9, 0.999), eps 1e-15,
// no weight decay, no amsgrad), in the element-wise form of torch's multi-tensor ("foreach") path.
//
// All of them are HBM-bound streams; each is ONE pass over its data where torch runs several:
//   l1:     reads x, y once, writes a 1-byte sign per element and one partial sum per workgroup;
//           the last workgroup sums the partials in a fixed order (deterministic loss, "last-workgroup
//           totals" in train_internal.h); the backward expands sign * (dL/dloss / N) (1 byte in, 4 bytes out per element);
//   adam:   per element reads p, g, m, v and writes p, m, v (28 bytes) for EVERY parameter tensor of
//           the model in one launch (tensor descriptors passed by value, chunk -> tensor lookup);
//   stats:  per Gaussian reads the viewspace gradient, visibility and radius and updates the three
//           accumulators in place;
//   reg:    the 12 planes' smoothness + L1 terms (scene/gaussian_model.py:538-577), which torch runs as
//           ~100 slice / sub / square / mean kernels forward and their slice-backward zero-fills
//           backward: one launch per direction over every plane, the value totalled as the L1 loss is.
#include <math.h>

#include <algorithm>

#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {

constexpr int kL1PerThread = 8;
constexpr int kL1Chunk = kTailThreads * kL1PerThread;

__global__ __launch_bounds__(kTailThreads) void l1_partial_kernel(int64_t n, const float *__restrict__ x,
                                                                  const float *__restrict__ y,
                                                                  int8_t *__restrict__ sign, TicketScratch ts,
                                                                  float *__restrict__ loss) {
    const int64_t base = (int64_t)blockIdx.x * kL1Chunk;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kL1PerThread; k++) {
        const int64_t i = base + (int64_t)k * kTailThreads + threadIdx.x;
        if (i < n) {
            const float d = x[i] - y[i];
            acc += fabsf(d);
            sign[i] = (int8_t)((d > 0.f) - (d < 0.f));  // torch.sign; |x| has subgradient 0 at 0
        }
    }
    double s = acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    __shared__ double s_w[kTailThreads / 64];
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTailThreads / 64; w++) t += s_w[w];
    double total;
    if (publish_and_total(t, ts, (int)gridDim.x, &total) && threadIdx.x == 0) *loss = (float)(total / (double)n);
}

// The same pass over 16-byte words (n % 4 == 0, 16-byte aligned x / y and 4-byte aligned sign): each
// thread takes two float4 of x and y and stores two char4 of signs -- a quarter of the memory
// instructions of the scalar form, the same partial layout (kL1Chunk elements per workgroup).
// GRAD: the loss's gradient for the upstream gradient `scale` = dloss * (1 / n) is stored instead of the signs
// (gs4d_l1_loss_grad: value and gradient in one pass, where l1_backward would read the signs back)
template <bool GRAD>
__global__ __launch_bounds__(kTailThreads) void l1_partial_v4_kernel(int64_t n4, const float4 *__restrict__ x,
                                                                     const float4 *__restrict__ y,
                                                                     char4 *__restrict__ sign, TicketScratch ts,
                                                                     float *__restrict__ loss, float4 *__restrict__ grad,
                                                                     float scale) {
    const int64_t base = (int64_t)blockIdx.x * (kL1Chunk / 4);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kL1PerThread / 4; k++) {
        const int64_t i = base + (int64_t)k * kTailThreads + threadIdx.x;
        if (i < n4) {
            const float4 a = x[i], b = y[i];
            const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
            acc += fabsf(d0);
            acc += fabsf(d1);
            acc += fabsf(d2);
            acc += fabsf(d3);
            auto sg = [](float d) { return (signed char)((d > 0.f) - (d < 0.f)); };  // torch.sign
            const char4 c = make_char4(sg(d0), sg(d1), sg(d2), sg(d3));
            if (GRAD)  // as l1_backward_v4_kernel: sign * (dloss * (1 / n))
                grad[i] = make_float4((float)c.x * scale, (float)c.y * scale, (float)c.z * scale, (float)c.w * scale);
            else
                sign[i] = c;
        }
    }
    double s = acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    __shared__ double s_w[kTailThreads / 64];
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTailThreads / 64; w++) t += s_w[w];
    double total;
    if (publish_and_total(t, ts, (int)gridDim.x, &total) && threadIdx.x == 0) *loss = (float)(total / (double)(4 * n4));
}

__global__ __launch_bounds__(kTailThreads) void l1_backward_kernel(int64_t n, const int8_t *__restrict__ sign,
                                                                   const float *__restrict__ dloss,
                                                                   float *__restrict__ grad) {
    // d mean / dx = sign / N, times the upstream gradient, rounded as torch's MeanBackward does it
    // (grad / numel with a scalar divisor: grad * (1 / numel))
    const float scale = *dloss * (1.0f / (float)n);
    for (int64_t i = (int64_t)blockIdx.x * kTailThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTailThreads)
        grad[i] = (float)sign[i] * scale;
}

__global__ __launch_bounds__(kTailThreads) void l1_backward_v4_kernel(int64_t n4, const char4 *__restrict__ sign,
                                                                      const float *__restrict__ dloss,
                                                                      float4 *__restrict__ grad, int64_t n) {
    const float scale = *dloss * (1.0f / (float)n);  // as l1_backward_kernel
    for (int64_t i = (int64_t)blockIdx.x * kTailThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kTailThreads) {
        const char4 c = sign[i];
        grad[i] = make_float4((float)c.x * scale, (float)c.y * scale, (float)c.z * scale, (float)c.w * scale);
    }
}

// ---- depth + mask supervision (gs4d_aux_loss_grad) ----------------------------------------------
// w_depth * mean over the valid pixels (gt_depth > 0) of |depth - gt_depth| + w_mask * mean |alpha - gt_mask|,
// with both gradient images, in two launches and without a host readback of the valid count:
//   1. every workgroup stores its three partials (S |depth - gt|, the valid count, S |alpha - mask|) at its own
//      slot of the scratch (no atomics, nothing to zero);
//   2. every workgroup totals all the slots in the same fixed order (a few KB from L2: one slot per 2048
//      pixels), so each holds the same n_valid bit for bit, then writes its chunk of the gradient images;
//      workgroup 0 also writes the value.
// A NULL gt_depth or gt_mask drops that term: its inputs are not read and its gradient image is not written.
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
        c += __shfl_xor(c, off);
    }
    __shared__ double s_w[kTailThreads / 64][3];
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6][0] = a;
        s_w[threadIdx.x >> 6][1] = b;
        s_w[threadIdx.x >> 6][2] = c;
    }
    __syncthreads();
    a = b = c = 0.0;
#pragma unroll
    for (int w = 0; w < kTailThreads / 64; w++) {
        a += s_w[w][0];
        b += s_w[w][1];
        c += s_w[w][2];
    }
}

__global__ __launch_bounds__(kTailThreads) void aux_partial_kernel(int64_t n, const float *__restrict__ depth,
                                                                   const float *__restrict__ alpha,
                                                                   const float *__restrict__ gt_depth,
                                                                   const float *__restrict__ gt_mask,
                                                                   double *__restrict__ part) {
    const int64_t base = (int64_t)blockIdx.x * kL1Chunk;
    float sd = 0.f, sm = 0.f;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kL1PerThread; k++) {
        const int64_t i = base + (int64_t)k * kTailThreads + threadIdx.x;
        if (i < n) {
            if (gt_depth) {
                const float g = gt_depth[i];
                if (g > 0.f) {
                    sd += fabsf(depth[i] - g);
                    cnt++;
                }
            }
            if (gt_mask) sm += fabsf(alpha[i] - gt_mask[i]);
        }
    }
    double a = sd, b = (double)cnt, c = sm;
    block_sum3(a, b, c);
    if (threadIdx.x == 0) {
        part[3 * (size_t)blockIdx.x + 0] = a;
        part[3 * (size_t)blockIdx.x + 1] = b;
        part[3 * (size_t)blockIdx.x + 2] = c;
    }
}

__global__ __launch_bounds__(kTailThreads) void aux_grad_kernel(int64_t n, const float *__restrict__ depth,
                                                                const float *__restrict__ alpha,
                                                                const float *__restrict__ gt_depth,
                                                                const float *__restrict__ gt_mask, float w_depth,
                                                                float w_mask, const double *__restrict__ part,
                                                                float *__restrict__ loss, float *__restrict__ dL_ddepth,
                                                                float *__restrict__ dL_dalpha) {
    // the totals, by every workgroup alike: thread t takes the slots t, t + 256, ... in ascending order
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = (int)threadIdx.x; i < (int)gridDim.x; i += kTailThreads) {
        a += part[3 * (size_t)i + 0];
        b += part[3 * (size_t)i + 1];
        c += part[3 * (size_t)i + 2];
    }
    block_sum3(a, b, c);
    const double n_valid = b < 1.0 ? 1.0 : b;  // max(1, count)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *loss = (float)((double)w_depth * a / n_valid + (double)w_mask * c / (double)n);
    const float scale_d = (float)((double)w_depth / n_valid);
    const float scale_m = (float)((double)w_mask / (double)n);
    const int64_t base = (int64_t)blockIdx.x * kL1Chunk;
#pragma unroll
    for (int k = 0; k < kL1PerThread; k++) {
        const int64_t i = base + (int64_t)k * kTailThreads + threadIdx.x;
        if (i < n) {
            if (gt_depth) {
                const float g = gt_depth[i];
                const float d = depth[i] - g;
                const float sg = (float)((d > 0.f) - (d < 0.f));  // torch.sign: 0 at 0
                dL_ddepth[i] = g > 0.f ? sg * scale_d : 0.f;
            }
            if (gt_mask) {
                const float d = alpha[i] - gt_mask[i];
                dL_dalpha[i] = (float)((d > 0.f) - (d < 0.f)) * scale_m;
            }
        }
    }
}

// ---- densification statistics ------------------------------------------------------------------
__global__ __launch_bounds__(kTailThreads) void densify_stats_kernel(int P, const float *__restrict__ vs_grad,
                                                                     const uint8_t *__restrict__ visible,
                                                                     const int *__restrict__ radii,
                                                                     float *__restrict__ grad_accum,
                                                                     float *__restrict__ denom,
                                                                     float *__restrict__ max_radii) {
    const int i = blockIdx.x * kTailThreads + threadIdx.x;
    if (i >= P) return;
    // without a visibility mask the filter is train.py's own definition of it, radii > 0 (:229-232; for a batch,
    // max over views of radii > 0 is any over views of visibility)
    if (visible ? !visible[i] : !(radii[i] > 0)) return;
    if (radii) max_radii[i] = fmaxf(max_radii[i], (float)radii[i]);  // train.py:348
    const float gx = vs_grad[3 * (size_t)i], gy = vs_grad[3 * (size_t)i + 1];
    grad_accum[i] += sqrtf(gx * gx + gy * gy);  // gaussian_model.py:522 torch.norm(grad[:, :2])
    denom[i] += 1.f;                            // gaussian_model.py:523
}

// ---- multi-tensor Adam --------------------------------------------------------------------------
constexpr int kAdamChunk = 4096;  // elements per workgroup

__global__ __launch_bounds__(kTailThreads) void adam_kernel(gs4d_adam_batch batch) {
    // chunk -> tensor: the descriptors carry their first chunk index (few dozen tensors: linear scan)
    const int64_t c = blockIdx.x;
    int t = 0;
    while (t + 1 < batch.count && batch.t[t + 1].first_chunk <= c) t++;
    const gs4d_adam_tensor d = batch.t[t];
    const int64_t base = (c - d.first_chunk) * kAdamChunk;
    const float b1 = batch.beta1, omb1 = batch.one_minus_beta1, b2 = batch.beta2, omb2 = batch.one_minus_beta2;
    const float eps = batch.eps, step_size = d.neg_step_size, bc2 = d.bias_correction2_sqrt;
    (void)b1;
    // one element: exactly the scalar sequence below, whichever width the loop loads at
    auto upd = [&](float g, float &p, float &m, float &v) {
        // exp_avg.lerp_(grad, 1 - beta1): weight < 0.5 -> self + weight * (end - self)
        m = fmaf(omb1, g - m, m);
        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        v = v * b2;
        v = fmaf(omb2, g * g, v);
        // denom = exp_avg_sq.sqrt() / bias_correction2_sqrt + eps; param.addcdiv_(exp_avg, denom, -step_size)
        const float den = sqrtf(v) / bc2 + eps;
        p = fmaf(step_size, m / den, p);
    };
    const bool vec = (((uintptr_t)d.param | (uintptr_t)d.grad | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq) & 15) == 0;
    if (vec) {
        // 16-byte loads and stores (the chunk base is a multiple of 4); the tensor's last n % 4 elements by the
        // chunk that holds them
        const int64_t n4 = d.n >> 2;
        for (int k = threadIdx.x; k < kAdamChunk / 4; k += kTailThreads) {
            const int64_t i4 = (base >> 2) + k;
            if (i4 >= n4) break;
            const float4 g = reinterpret_cast<const float4 *>(d.grad)[i4];
            float4 p = reinterpret_cast<float4 *>(d.param)[i4];
            float4 m = reinterpret_cast<float4 *>(d.exp_avg)[i4];
            float4 v = reinterpret_cast<float4 *>(d.exp_avg_sq)[i4];
            upd(g.x, p.x, m.x, v.x);
            upd(g.y, p.y, m.y, v.y);
            upd(g.z, p.z, m.z, v.z);
            upd(g.w, p.w, m.w, v.w);
            reinterpret_cast<float4 *>(d.param)[i4] = p;
            reinterpret_cast<float4 *>(d.exp_avg)[i4] = m;
            reinterpret_cast<float4 *>(d.exp_avg_sq)[i4] = v;
        }
        const int64_t i = 4 * n4 + threadIdx.x;
        if (i < d.n && i >= base && i < base + kAdamChunk) {
            float p = d.param[i], m = d.exp_avg[i], v = d.exp_avg_sq[i];
            upd(d.grad[i], p, m, v);
            d.param[i] = p;
            d.exp_avg[i] = m;
            d.exp_avg_sq[i] = v;
        }
        return;
    }
    for (int k = threadIdx.x; k < kAdamChunk; k += kTailThreads) {
        const int64_t i = base + k;
        if (i >= d.n) break;
        float p = d.param[i], m = d.exp_avg[i], v = d.exp_avg_sq[i];
        upd(d.grad[i], p, m, v);
        d.param[i] = p;
        d.exp_avg[i] = m;
        d.exp_avg_sq[i] = v;
    }
}


// ---- deformation tail + activations (scene/deformation.py:140-146, gaussian_renderer/__init__.py:97-99)
// Blocks [0, nb_g) take one Gaussian per thread (means, scales, rotation, opacity); blocks [nb_g, ..)
// take the 3K SH values of the Gaussians as one flat, coalesced range.
__global__ __launch_bounds__(kTailThreads) void deform_tail_fwd_kernel(
    int P, int K, int nb_g, const float *__restrict__ xyz, const float *__restrict__ s, const float *__restrict__ r,
    const float *__restrict__ o, const float *__restrict__ f_dc, const float *__restrict__ f_rest,
    const float *__restrict__ dx, const float *__restrict__ ds, const float *__restrict__ dr,
    const float *__restrict__ d_o, const float *__restrict__ dshs, float *__restrict__ means,
    float *__restrict__ scales, float *__restrict__ rot, float *__restrict__ opac, float *__restrict__ shs, int v4) {
    if ((int)blockIdx.x < nb_g) {
        const int i = blockIdx.x * kTailThreads + threadIdx.x;
        if (i >= P) return;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const size_t k = 3 * (size_t)i + c;
            means[k] = dx ? xyz[k] + dx[k] : xyz[k];
            scales[k] = expf(ds ? s[k] + ds[k] : s[k]);
        }
        float q[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const size_t k = 4 * (size_t)i + c;
            q[c] = dr ? r[k] + dr[k] : r[k];
        }
        // F.normalize: x / max(||x||_2, eps)
        const float nrm = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
#pragma unroll
        for (int c = 0; c < 4; c++) rot[4 * (size_t)i + c] = q[c] / nrm;
        const float x = d_o ? o[i] + d_o[i] : o[i];
        opac[i] = 1.f / (1.f + expf(-x));
        return;
    }
    const int64_t n = (int64_t)P * 3 * K;
    if (v4) {
        // four consecutive values per thread (3K % 4 == 0: they share a Gaussian), dshs / shs as 16-byte accesses
        const int64_t e0 = 4 * ((int64_t)(blockIdx.x - nb_g) * kTailThreads + threadIdx.x);
        if (e0 >= n) return;
        const int64_t g = (int64_t)((uint32_t)e0 / (uint32_t)(3 * K)), k0 = e0 - g * 3 * K;
        const float4 d = dshs ? reinterpret_cast<const float4 *>(dshs)[e0 / 4] : make_float4(0.f, 0.f, 0.f, 0.f);
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t k = k0 + j;
            b[j] = k < 3 ? f_dc[3 * g + k] : f_rest[g * 3 * (K - 1) + (k - 3)];
        }
        reinterpret_cast<float4 *>(shs)[e0 / 4] =
            dshs ? make_float4(b[0] + d.x, b[1] + d.y, b[2] + d.z, b[3] + d.w) : make_float4(b[0], b[1], b[2], b[3]);
        return;
    }
    const int64_t e = (int64_t)(blockIdx.x - nb_g) * kTailThreads + threadIdx.x;
    if (e >= n) return;
    // 32-bit quotient (a 64-bit division is a long software sequence): e < P * 3K < 2^32 by the host check
    const int64_t g = (int64_t)((uint32_t)e / (uint32_t)(3 * K)), k = e - g * 3 * K;
    const float base = k < 3 ? f_dc[3 * g + k] : f_rest[g * 3 * (K - 1) + (k - 3)];
    shs[e] = dshs ? base + dshs[e] : base;
}

__global__ __launch_bounds__(kTailThreads) void deform_tail_bwd_kernel(
    int P, int K, int nb_g, const float *__restrict__ scales, const float *__restrict__ r,
    const float *__restrict__ dr, const float *__restrict__ opac, const float *__restrict__ g_means,
    const float *__restrict__ g_scales, const float *__restrict__ g_rot, const float *__restrict__ g_opac,
    const float *__restrict__ g_shs, float *__restrict__ d_xyz, float *__restrict__ d_s, float *__restrict__ d_r,
    float *__restrict__ d_o, float *__restrict__ d_fdc, float *__restrict__ d_frest, float *__restrict__ g_dx,
    float *__restrict__ g_ds, float *__restrict__ g_dr, float *__restrict__ g_do, int v4) {
    if ((int)blockIdx.x < nb_g) {
        const int i = blockIdx.x * kTailThreads + threadIdx.x;
        if (i >= P) return;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const size_t k = 3 * (size_t)i + c;
            const float gm = g_means ? g_means[k] : 0.f;
            const float gs = g_scales ? g_scales[k] * scales[k] : 0.f;  // d exp(x) = exp(x) dx
            d_xyz[k] = gm;
            d_s[k] = gs;
            if (g_dx) g_dx[k] = gm;
            if (g_ds) g_ds[k] = gs;
        }
        float q[4], g[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const size_t k = 4 * (size_t)i + c;
            q[c] = dr ? r[k] + dr[k] : r[k];
            g[c] = g_rot ? g_rot[k] : 0.f;
        }
        // autograd of x / clamp_min(||x||, eps): g / n - x (x . g) / n^3 (the second term only when ||x|| > eps)
        const float n0 = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const float nrm = fmaxf(n0, 1e-12f);
        const float xg = q[0] * g[0] + q[1] * g[1] + q[2] * g[2] + q[3] * g[3];
        // at or below eps (n0 may be 0: a zero quaternion, or squares that underflow) the gradient is g / eps alone,
        // with no division by n0
        const bool above = n0 > 1e-12f;
        const float gn = above ? -xg / (nrm * nrm) : 0.f;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float v = above ? g[c] / nrm + gn * (q[c] / n0) : g[c] / nrm;
            d_r[4 * (size_t)i + c] = v;
            if (g_dr) g_dr[4 * (size_t)i + c] = v;
        }
        const float y = opac[i];
        const float go = g_opac ? (g_opac[i] * (1.f - y)) * y : 0.f;  // sigmoid backward, torch's order
        d_o[i] = go;
        if (g_do) g_do[i] = go;
        return;
    }
    const int64_t n = (int64_t)P * 3 * K;
    if (v4) {  // as in deform_tail_fwd_kernel: g_shs as 16-byte loads
        const int64_t e0 = 4 * ((int64_t)(blockIdx.x - nb_g) * kTailThreads + threadIdx.x);
        if (e0 >= n) return;
        const int64_t gi = (int64_t)((uint32_t)e0 / (uint32_t)(3 * K)), k0 = e0 - gi * 3 * K;
        const float4 v4v = g_shs ? reinterpret_cast<const float4 *>(g_shs)[e0 / 4] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float v[4] = {v4v.x, v4v.y, v4v.z, v4v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t k = k0 + j;
            if (k < 3) d_fdc[3 * gi + k] = v[j];
            else d_frest[gi * 3 * (K - 1) + (k - 3)] = v[j];
        }
        return;
    }
    const int64_t e = (int64_t)(blockIdx.x - nb_g) * kTailThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t gi = (int64_t)((uint32_t)e / (uint32_t)(3 * K)), k = e - gi * 3 * K;  // e < 2^32: host check
    const float v = g_shs ? g_shs[e] : 0.f;
    if (k < 3) d_fdc[3 * gi + k] = v;
    else d_frest[gi * 3 * (K - 1) + (k - 3)] = v;
}

// ---- HexPlane regularisers ------------------------------------------------------------------------
constexpr int kRegPerThread = 8;
constexpr int kRegBlock = kTailThreads * kRegPerThread;  // plane elements per workgroup

__device__ __forceinline__ int reg_plane_of(const gs4d_reg_batch &b, int64_t blk) {
    int t = 0;
    while (t + 1 < b.count && b.p[t + 1].first_block <= blk) t++;
    return t;
}

// second difference along H at row y (0 <= y <= H-3), in the reference's operation order
// (regulation.py:25-26): first[j] = t[j+1] - t[j], second[y] = first[y+1] - first[y]
__device__ __forceinline__ float second_diff(const float *__restrict__ col, int y, int W) {
    const float t0 = col[(size_t)y * W], t1 = col[(size_t)(y + 1) * W], t2 = col[(size_t)(y + 2) * W];
    return (t2 - t1) - (t1 - t0);
}

__global__ __launch_bounds__(kTailThreads) void reg_forward_kernel(gs4d_reg_batch b, TicketScratch ts, float *__restrict__ loss) {
    const int64_t blk = blockIdx.x;
    const gs4d_reg_plane d = b.p[reg_plane_of(b, blk)];
    const int64_t n = (int64_t)d.C * d.H * d.W, hw = (int64_t)d.H * d.W;
    const double cs = (double)d.w_smooth / ((double)d.C * (d.H - 2) * d.W), cl = (double)d.w_l1 / (double)n;
    double acc = 0.0;
    // rows y .. y + 2 of every element first (indices clamped into the plane: all loads in flight at once, none
    // behind the loop's exit), then the terms in element order
    float r[kRegPerThread][3];
    const int64_t i0 = (blk - d.first_block) * kRegBlock + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kRegPerThread; k++) {
        const int64_t i = std::min<int64_t>(i0 + (int64_t)k * kTailThreads, n - 1);
        const int y = (int)(((uint32_t)i % (uint32_t)hw) / (uint32_t)d.W);  // 32-bit: a plane < 2^31 elements
        const float *col = d.data + (i - (int64_t)y * d.W);
#pragma unroll
        for (int q = 0; q < 3; q++) r[k][q] = col[(size_t)std::min(y + q, d.H - 1) * d.W];
    }
#pragma unroll
    for (int k = 0; k < kRegPerThread; k++) {
        const int64_t i = i0 + (int64_t)k * kTailThreads;
        if (i >= n) break;
        const float t = r[k][0];
        const int y = (int)(((uint32_t)i % (uint32_t)hw) / (uint32_t)d.W);
        if (y <= d.H - 3) {
            const float s2 = (r[k][2] - r[k][1]) - (r[k][1] - r[k][0]);  // second_diff at row y
            acc += cs * (double)(s2 * s2);
        }
        acc += cl * (double)fabsf(1.f - t);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    __shared__ double s_w[kTailThreads / 64];
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    double total;
    if (publish_and_total(s_w[0] + s_w[1] + s_w[2] + s_w[3], ts, (int)gridDim.x, &total) && threadIdx.x == 0)
        *loss = (float)total;
}

// d/dt of the batch loss, as autograd derives it from the reference's graph: mean -> g / N, square
// -> 2 s g, second[y] = first[y+1] - first[y] -> dfirst[j] = ds[j-1] - ds[j], first[j] = t[j+1] - t[j]
// -> dt[y] = dfirst[y-1] - dfirst[y] (out-of-range terms are 0); abs(1 - t) -> -sign(1 - t) g / N.
// loss (nullable): also the value, its per-workgroup partials exactly as reg_forward_kernel forms them (same
// workgroups, same per-thread order and terms: its second difference at row y is the ds[2] term below) and
// totalled by the last workgroup -- the value and the gradient from one read of the planes.  base (nullable):
// *loss = *base + value instead, the fp32 add of a loss term the value joins.
__global__ __launch_bounds__(kTailThreads) void reg_backward_kernel(gs4d_reg_batch b, const float *__restrict__ dloss,
                                                                    TicketScratch ts, float *__restrict__ loss,
                                                                    const float *__restrict__ base) {
    const bool part = loss != nullptr;
    const int64_t blk = blockIdx.x;
    const gs4d_reg_plane d = b.p[reg_plane_of(b, blk)];
    const int64_t n = (int64_t)d.C * d.H * d.W, hw = (int64_t)d.H * d.W;
    const float g = *dloss;
    const float gs = (g * d.w_smooth) / (float)((int64_t)d.C * (d.H - 2) * d.W);
    const float gl = (g * d.w_l1) / (float)n;
    const double cs = (double)d.w_smooth / ((double)d.C * (d.H - 2) * d.W), cl = (double)d.w_l1 / (double)n;
    double acc = 0.0;
    // rows y - 2 .. y + 2 of every element (and its gradient, when accumulating) first, indices clamped into the
    // plane: all loads in flight at once, none behind the loop's exit; out-of-range rows only feed masked terms
    float r[kRegPerThread][5], gv[kRegPerThread];
    const int64_t i0 = (blk - d.first_block) * kRegBlock + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kRegPerThread; k++) {
        const int64_t i = std::min<int64_t>(i0 + (int64_t)k * kTailThreads, n - 1);
        const int y = (int)(((uint32_t)i % (uint32_t)hw) / (uint32_t)d.W);  // 32-bit: a plane < 2^31 elements
        const float *col = d.data + (i - (int64_t)y * d.W);
#pragma unroll
        for (int q = 0; q < 5; q++) r[k][q] = col[(size_t)std::min(std::max(y - 2 + q, 0), d.H - 1) * d.W];
        gv[k] = b.accumulate ? d.grad[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kRegPerThread; k++) {
        const int64_t i = i0 + (int64_t)k * kTailThreads;
        if (i >= n) break;
        const int y = (int)(((uint32_t)i % (uint32_t)hw) / (uint32_t)d.W);
        float ds[3], s2y = 0.f;  // ds[y-2], ds[y-1], ds[y]; s2y: the second difference at row y itself
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int yy = y - 2 + q;
            const bool in = yy >= 0 && yy <= d.H - 3;
            const float s2 = in ? (r[k][q + 2] - r[k][q + 1]) - (r[k][q + 1] - r[k][q]) : 0.f;  // second_diff at yy
            ds[q] = in ? 2.f * s2 * gs : 0.f;
            if (q == 2) s2y = s2;
        }
        const float df_prev = (y >= 1) ? ds[0] - ds[1] : 0.f;      // dfirst[y-1] = ds[y-2] - ds[y-1]
        const float df_cur = (y <= d.H - 2) ? ds[1] - ds[2] : 0.f;  // dfirst[y] = ds[y-1] - ds[y]
        const float t = r[k][2];
        const float one_m = 1.f - t;
        const float sg = (float)((one_m > 0.f) - (one_m < 0.f));
        const float v = (df_prev - df_cur) + (-sg) * gl;
        d.grad[i] = b.accumulate ? gv[k] + v : v;
        if (part) {  // reg_forward_kernel's terms, in its order
            if (y <= d.H - 3) acc += cs * (double)(s2y * s2y);
            acc += cl * (double)fabsf(1.f - t);
        }
    }
    if (part) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        __shared__ double s_w[kTailThreads / 64];
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
        __syncthreads();
        double total;
        if (publish_and_total(s_w[0] + s_w[1] + s_w[2] + s_w[3], ts, (int)gridDim.x, &total) && threadIdx.x == 0)
            *loss = base ? *base + (float)total : (float)total;
    }
}

// ---- the HexPlane field's input points: scene/hexplane.py:20-21 normalize_aabb + :166 torch.cat((pts, t)) in
// one pass, pts4[n] = ((xyz[n] - aabb[0]) * s - 1, t[n]) with s = (1 / (aabb[1] - aabb[0])) * 2 (torch's
// 2.0 / tensor is reciprocal-then-multiply), the same float operations as the reference's graph; backward:
// dxyz = dpts[:, 0:3] * s (the mul's gradient; the time column takes none).
__device__ __forceinline__ float3 hex_scale(const float *aabb) {
    return make_float3((1.0f / (aabb[3] - aabb[0])) * 2.0f, (1.0f / (aabb[4] - aabb[1])) * 2.0f,
                       (1.0f / (aabb[5] - aabb[2])) * 2.0f);
}
__global__ __launch_bounds__(256) void hex_points_kernel(int N, const float *__restrict__ xyz, int64_t ld_xyz,
                                                         const float *__restrict__ t, int64_t ld_t,
                                                         const float *__restrict__ aabb, float4 *__restrict__ pts) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float3 sc = hex_scale(aabb);
    const float *x = xyz + (size_t)n * ld_xyz;
    pts[n] = make_float4((x[0] - aabb[0]) * sc.x - 1.0f, (x[1] - aabb[1]) * sc.y - 1.0f, (x[2] - aabb[2]) * sc.z - 1.0f,
                         t[(size_t)n * ld_t]);
}
// add (nullable): another gradient of xyz, summed in (the add autograd would launch for xyz's two uses)
__global__ __launch_bounds__(256) void hex_points_bwd_kernel(int N, const float4 *__restrict__ dpts,
                                                             const float *__restrict__ aabb,
                                                             const float *__restrict__ add, float *__restrict__ dxyz) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float3 sc = hex_scale(aabb);
    const float4 d = dpts[n];
    float g0 = d.x * sc.x, g1 = d.y * sc.y, g2 = d.z * sc.z;
    if (add) {
        g0 = add[3 * (size_t)n] + g0;
        g1 = add[3 * (size_t)n + 1] + g1;
        g2 = add[3 * (size_t)n + 2] + g2;
    }
    dxyz[3 * (size_t)n] = g0;
    dxyz[3 * (size_t)n + 1] = g1;
    dxyz[3 * (size_t)n + 2] = g2;
}

}  // namespace gs4d

using namespace gs4d;

// ---- row surgery of densification / pruning (gs4d_rows_assemble, scene/gaussian_model.py:316-506): tensor
// blockIdx.y, its output elements grid-strided over blockIdx.x.  Element c of output row r: r < K takes old
// row keep[r]; r = K + j takes, by the tensor's mode, old row append[j] or (the last given_rows) given rows,
// or zero.  Pure copies
// (4-byte words or bytes): bitwise the reference's cat / boolean-index results.  The batch is passed by value.
constexpr int64_t kRowsPerBlock = (int64_t)kTailThreads * 8;
template <class T>
__device__ __forceinline__ void rows_copy(const gs4d_rows_batch &b, const gs4d_rows_tensor &t) {
    const int64_t w = t.width, n = (b.K + b.A) * w;
    const T *__restrict__ src = (const T *)t.src;
    const T *__restrict__ given = (const T *)t.given;
    T *__restrict__ dst = (T *)t.dst;
    for (int64_t e = (int64_t)blockIdx.x * kTailThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kTailThreads) {
        const int64_t r = e / w, c = e - r * w;
        T v = T(0);
        if (t.mode != GS4D_ROWS_ZERO) {
            if (r < b.K) {
                v = src[(int64_t)b.keep[r] * w + c];
            } else if (t.mode == GS4D_ROWS_GATHER) {
                const int64_t j = r - b.K, jg = j - (b.A - t.given_rows);
                v = jg < 0 ? src[(int64_t)b.append[j] * w + c] : given[jg * w + c];
            }
        }
        dst[e] = v;
    }
}
__global__ __launch_bounds__(kTailThreads) void rows_assemble_kernel(gs4d_rows_batch b) {
    const gs4d_rows_tensor &t = b.t[blockIdx.y];
    if (t.esize == 4) rows_copy<uint32_t>(b, t);
    else rows_copy<uint8_t>(b, t);
}

// ---- sum of S slices of n floats in slice order (gs4d_sum_slices): eight slices in flight per thread, float4
// columns when n and the pointers allow
// 64-thread workgroups: a column per thread, so the (P / 1024)-slice sums of the MLP's 128 x 640 weight
// gradient (20480 float4 columns) spread over 320 workgroups, every CU, where 256-thread ones filled 80 CUs
constexpr int kSumThreads = 64;
template <bool V4>
__global__ __launch_bounds__(kSumThreads) void sum_slices_kernel(const float *__restrict__ parts, int S, int64_t n,
                                                                 float *__restrict__ out) {
    const int64_t m = V4 ? n / 4 : n;
    for (int64_t i = (int64_t)blockIdx.x * kSumThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kSumThreads) {
        if (V4) {
            const float4 *p = reinterpret_cast<const float4 *>(parts) + i;
            float4 acc = p[0];
            int s = 1;
            for (; s + 7 < S; s += 8) {  // the loads of eight slices issued together, added in order
                float4 v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = p[(size_t)(s + k) * m];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    acc.x += v[k].x; acc.y += v[k].y; acc.z += v[k].z; acc.w += v[k].w;
                }
            }
            for (; s < S; s++) {
                const float4 a = p[(size_t)s * m];
                acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
            }
            reinterpret_cast<float4 *>(out)[i] = acc;
        } else {
            float acc = parts[i];
            for (int s = 1; s < S; s++) acc += parts[(size_t)s * n + i];
            out[i] = acc;
        }
    }
}

// Many slices (S >= 16) over few outputs (the split-K weight gradients: 200 slices of 82k floats): a wave per
// 16 float4 outputs, its four 16-lane groups summing a quarter of the slices each in slice order, then the
// quarters as (q0 + q1) + (q2 + q3) through two lane swaps -- a fixed tree, so every run gives the same bits, and
// four times the loads in flight of one thread per output (which left most CUs idle: 80 workgroups).
__global__ __launch_bounds__(kSumThreads) void sum_slices_quarters_kernel(const float *__restrict__ parts, int S,
                                                                          int64_t m, float4 *__restrict__ out) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int64_t i = (((int64_t)blockIdx.x * kSumThreads + threadIdx.x) >> 6) * 16 + (lane & 15);
    const int s0 = g * S / 4, s1 = (g + 1) * S / 4;
    const float4 *p = reinterpret_cast<const float4 *>(parts) + (i < m ? i : 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = s0;
    for (; s + 7 < s1; s += 8) {  // eight slices' loads issued together, added in order
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = p[(size_t)(s + k) * m];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            acc.x += v[k].x; acc.y += v[k].y; acc.z += v[k].z; acc.w += v[k].w;
        }
    }
    for (; s < s1; s++) {
        const float4 a = p[(size_t)s * m];
        acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
    // (q0 + q1) + (q2 + q3): float addition commutes exactly, so both lanes of a swap hold the same bits
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        acc.x += __shfl_xor(acc.x, off);
        acc.y += __shfl_xor(acc.y, off);
        acc.z += __shfl_xor(acc.z, off);
        acc.w += __shfl_xor(acc.w, off);
    }
    if (g == 0 && i < m) out[i] = acc;
}

// ---- entry points (include/gs4d_train.h): argument checks and launch geometry of the kernels above ----
extern "C" {

int64_t gs4d_reg_blocks(int C, int H, int W) { return ((int64_t)C * H * W + kRegBlock - 1) / kRegBlock; }

static int reg_check(const gs4d_reg_batch *b, int64_t *nblk) {
    if (!b || b->count < 1 || b->count > GS4D_REG_MAX_PLANES) return 1;
    int64_t blocks = 0;
    for (int i = 0; i < b->count; i++) {
        const gs4d_reg_plane &p = b->p[i];
        if (!p.data || p.C < 1 || p.H < 3 || p.W < 1 || p.first_block != blocks) return 1;
        if ((int64_t)p.C * p.H * p.W > INT32_MAX) return 1;  // the kernels index a plane in 32 bits
        blocks += gs4d_reg_blocks(p.C, p.H, p.W);
    }
    *nblk = blocks;
    return 0;
}

size_t gs4d_reg_scratch_bytes(const gs4d_reg_batch *batch) {
    int64_t nblk = 0;
    if (reg_check(batch, &nblk)) return 0;
    return 8 * (size_t)nblk + 4 * kTicketWords + 256;
}

int gs4d_hexplane_reg_forward(const gs4d_reg_batch *batch, float *loss, void *scratch, void *stream) {
    int64_t nblk = 0;
    if (reg_check(batch, &nblk) || !loss || !scratch) return 1;
    hipLaunchKernelGGL(reg_forward_kernel, dim3((unsigned)nblk), dim3(kTailThreads), 0, (hipStream_t)stream, *batch,
                       ticket_scratch(scratch), loss);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_hexplane_reg_backward(const gs4d_reg_batch *batch, const float *dloss, void *stream) {
    int64_t nblk = 0;
    if (reg_check(batch, &nblk) || !dloss) return 1;
    for (int i = 0; i < batch->count; i++)
        if (!batch->p[i].grad) return 1;
    hipLaunchKernelGGL(reg_backward_kernel, dim3((unsigned)nblk), dim3(kTailThreads), 0, (hipStream_t)stream, *batch,
                       dloss, TicketScratch{nullptr, nullptr}, (float *)nullptr, (const float *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_hexplane_reg_backward_value(const gs4d_reg_batch *batch, const float *dloss, float *loss, const float *base,
                                     void *scratch, void *stream) {
    int64_t nblk = 0;
    if (reg_check(batch, &nblk) || !dloss || !loss || !scratch) return 1;
    for (int i = 0; i < batch->count; i++)
        if (!batch->p[i].grad) return 1;
    hipLaunchKernelGGL(reg_backward_kernel, dim3((unsigned)nblk), dim3(kTailThreads), 0, (hipStream_t)stream, *batch,
                       dloss, ticket_scratch(scratch), loss, base);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}


size_t gs4d_l1_scratch_bytes(int64_t n) { return 8 * (size_t)((n + kL1Chunk - 1) / kL1Chunk) + 4 * kTicketWords + 256; }

int gs4d_l1_loss_forward(int64_t n, const float *x, const float *y, int8_t *sign, float *loss, void *scratch,
                         void *stream) {
    if (n < 0 || (n > 0 && (!x || !y || !sign || !scratch)) || !loss) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return hipMemsetAsync(loss, 0, 4, s) == hipSuccess ? 0 : 3;
    const int64_t nblk = (n + kL1Chunk - 1) / kL1Chunk;
    if (nblk > INT32_MAX) return 1;
    if (n % 4 == 0 && (((size_t)x | (size_t)y) & 15) == 0 && ((size_t)sign & 3) == 0)
        hipLaunchKernelGGL(l1_partial_v4_kernel<false>, dim3((unsigned)nblk), dim3(kTailThreads), 0, s, n / 4,
                           (const float4 *)x, (const float4 *)y, (char4 *)sign, ticket_scratch(scratch), loss,
                           (float4 *)nullptr, 0.f);
    else
        hipLaunchKernelGGL(l1_partial_kernel, dim3((unsigned)nblk), dim3(kTailThreads), 0, s, n, x, y, sign,
                           ticket_scratch(scratch), loss);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_l1_loss_grad(int64_t n, const float *x, const float *y, float dloss, float *loss, float *grad, void *scratch,
                      void *stream) {
    if (n < 0 || (n > 0 && (!x || !y || !grad || !scratch)) || !loss) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return hipMemsetAsync(loss, 0, 4, s) == hipSuccess ? 0 : 3;
    if (n % 4 != 0 || (((size_t)x | (size_t)y | (size_t)grad) & 15) != 0) return 1;  // the float4 form only
    const int64_t nblk = (n + kL1Chunk - 1) / kL1Chunk;
    if (nblk > INT32_MAX) return 1;
    const float scale = dloss * (1.0f / (float)n);  // torch's MeanBackward rounding, as l1_backward
    hipLaunchKernelGGL(l1_partial_v4_kernel<true>, dim3((unsigned)nblk), dim3(kTailThreads), 0, s, n / 4,
                       (const float4 *)x, (const float4 *)y, (char4 *)nullptr, ticket_scratch(scratch), loss,
                       (float4 *)grad, scale);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

size_t gs4d_aux_loss_scratch_bytes(int64_t n) {
    return n > 0 ? 24 * (size_t)((n + kL1Chunk - 1) / kL1Chunk) + 256 : 256;
}

int gs4d_aux_loss_grad(int64_t n, const float *depth, const float *alpha, const float *gt_depth, const float *gt_mask,
                       float w_depth, float w_mask, float *loss, float *dL_ddepth, float *dL_dalpha, void *scratch,
                       void *stream) {
    if (n < 1 || !loss || !scratch) return 1;
    if (gt_depth && (!depth || !dL_ddepth)) return 1;
    if (gt_mask && (!alpha || !dL_dalpha)) return 1;
    const int64_t nblk = (n + kL1Chunk - 1) / kL1Chunk;
    if (nblk > INT32_MAX) return 1;
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)(((size_t)scratch + 7) & ~(size_t)7);
    hipLaunchKernelGGL(aux_partial_kernel, dim3((unsigned)nblk), dim3(kTailThreads), 0, s, n, depth, alpha, gt_depth,
                       gt_mask, part);
    if (hipGetLastError() != hipSuccess) return 3;
    hipLaunchKernelGGL(aux_grad_kernel, dim3((unsigned)nblk), dim3(kTailThreads), 0, s, n, depth, alpha, gt_depth,
                       gt_mask, w_depth, w_mask, (const double *)part, loss, dL_ddepth, dL_dalpha);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_l1_loss_backward(int64_t n, const int8_t *sign, const float *dloss, float *grad, void *stream) {
    if (n < 0 || (n > 0 && (!sign || !dloss || !grad))) return 1;
    if (n == 0) return 0;
    if (n % 4 == 0 && ((size_t)sign & 3) == 0 && ((size_t)grad & 15) == 0) {
        const int nblk = (int)std::min<int64_t>((n / 4 + kTailThreads - 1) / kTailThreads, 8192);
        hipLaunchKernelGGL(l1_backward_v4_kernel, dim3(nblk), dim3(kTailThreads), 0, (hipStream_t)stream, n / 4,
                           (const char4 *)sign, dloss, (float4 *)grad, n);
        return hipGetLastError() == hipSuccess ? 0 : 3;
    }
    const int nblk = (int)std::min<int64_t>((n + kTailThreads - 1) / kTailThreads, 8192);
    hipLaunchKernelGGL(l1_backward_kernel, dim3(nblk), dim3(kTailThreads), 0, (hipStream_t)stream, n, sign, dloss, grad);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_deform_tail_forward(int P, int K, const float *xyz, const float *s, const float *r, const float *o,
                             const float *f_dc, const float *f_rest, const float *dx, const float *ds, const float *dr,
                             const float *d_o, const float *dshs, float *means, float *scales, float *rot,
                             float *opac, float *shs, void *stream) {
    if (P < 0 || K < 1 || (P > 0 && (!xyz || !s || !r || !o || !f_dc || (K > 1 && !f_rest) || !means || !scales ||
                                     !rot || !opac || !shs)))
        return 1;
    if (P == 0) return 0;
    if ((int64_t)P * 3 * K > UINT32_MAX) return 1;  // the SH range is indexed in 32 bits
    const int nb_g = (P + kTailThreads - 1) / kTailThreads;
    const int v4 = (3 * K) % 4 == 0 && (((size_t)dshs | (size_t)shs) & 15) == 0;
    const int64_t nb_s = ((int64_t)P * 3 * K / (v4 ? 4 : 1) + kTailThreads - 1) / kTailThreads;
    hipLaunchKernelGGL(deform_tail_fwd_kernel, dim3((unsigned)(nb_g + nb_s)), dim3(kTailThreads), 0, (hipStream_t)stream,
                       P, K, nb_g, xyz, s, r, o, f_dc, f_rest, dx, ds, dr, d_o, dshs, means, scales, rot, opac, shs, v4);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_deform_tail_backward(int P, int K, const float *scales, const float *r, const float *dr, const float *opac,
                              const float *g_means, const float *g_scales, const float *g_rot, const float *g_opac,
                              const float *g_shs, float *d_xyz, float *d_s, float *d_r, float *d_o, float *d_fdc,
                              float *d_frest, float *g_dx, float *g_ds, float *g_dr, float *g_do, void *stream) {
    if (P < 0 || K < 1 || (P > 0 && (!scales || !r || !opac || !d_xyz || !d_s || !d_r || !d_o || !d_fdc ||
                                     (K > 1 && !d_frest))))
        return 1;
    if (P == 0) return 0;
    if ((int64_t)P * 3 * K > UINT32_MAX) return 1;  // the SH range is indexed in 32 bits
    const int nb_g = (P + kTailThreads - 1) / kTailThreads;
    const int v4 = (3 * K) % 4 == 0 && ((size_t)g_shs & 15) == 0;
    const int64_t nb_s = ((int64_t)P * 3 * K / (v4 ? 4 : 1) + kTailThreads - 1) / kTailThreads;
    hipLaunchKernelGGL(deform_tail_bwd_kernel, dim3((unsigned)(nb_g + nb_s)), dim3(kTailThreads), 0, (hipStream_t)stream,
                       P, K, nb_g, scales, r, dr, opac, g_means, g_scales, g_rot, g_opac, g_shs, d_xyz, d_s, d_r, d_o,
                       d_fdc, d_frest, g_dx, g_ds, g_dr, g_do, v4);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_rows_assemble(const gs4d_rows_batch *batch, void *stream) {
    if (!batch || batch->count < 0 || batch->count > GS4D_ROWS_MAX_TENSORS || batch->K < 0 || batch->A < 0) return 1;
    const gs4d_rows_batch &b = *batch;
    const int64_t rows = b.K + b.A;
    if (rows > INT32_MAX || (b.K > 0 && !b.keep)) return 1;
    int64_t most = 0;
    for (int i = 0; i < b.count; i++) {
        const gs4d_rows_tensor &t = b.t[i];
        if (t.width < 1 || (t.esize != 1 && t.esize != 4) || t.mode < GS4D_ROWS_GATHER || t.mode > GS4D_ROWS_ZERO) return 1;
        if (rows > 0 && !t.dst) return 1;
        if (t.mode != GS4D_ROWS_ZERO && b.K > 0 && !t.src) return 1;
        if (t.mode == GS4D_ROWS_GATHER) {
            if (t.given_rows < 0 || t.given_rows > b.A || (t.given_rows > 0 && !t.given)) return 1;
            if (t.given_rows < b.A && (!b.append || !t.src)) return 1;
        }
        most = std::max(most, rows * t.width);
    }
    if (b.count == 0 || most == 0) return 0;
    const unsigned gx = (unsigned)std::min<int64_t>((most + kRowsPerBlock - 1) / kRowsPerBlock, 4096);
    hipLaunchKernelGGL(rows_assemble_kernel, dim3(gx, b.count), dim3(kTailThreads), 0, (hipStream_t)stream, b);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_sum_slices(const float *parts, int S, int64_t n, float *out, void *stream) {
    if (S < 1 || n < 0 || (n > 0 && (!parts || !out))) return 1;
    if (n == 0) return 0;
    const bool v4 = n % 4 == 0 && ((uintptr_t)parts % 16) == 0 && ((uintptr_t)out % 16) == 0;
    const int64_t m = v4 ? n / 4 : n;
    if (v4 && S >= 16 && m <= ((int64_t)1 << 24)) {
        const unsigned g4 = (unsigned)((m + 15) / 16 * 64 + kSumThreads - 1) / kSumThreads;
        hipLaunchKernelGGL(sum_slices_quarters_kernel, dim3(g4), dim3(kSumThreads), 0, (hipStream_t)stream, parts, S,
                           m, reinterpret_cast<float4 *>(out));
        return hipGetLastError() == hipSuccess ? 0 : 3;
    }
    const unsigned grid = (unsigned)std::min<int64_t>((m + kSumThreads - 1) / kSumThreads, 16384);
    if (v4)
        hipLaunchKernelGGL(sum_slices_kernel<true>, dim3(grid), dim3(kSumThreads), 0, (hipStream_t)stream, parts, S, n, out);
    else
        hipLaunchKernelGGL(sum_slices_kernel<false>, dim3(grid), dim3(kSumThreads), 0, (hipStream_t)stream, parts, S, n,
                           out);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_densify_stats(int P, const float *viewspace_grad, const uint8_t *visible, const int *radii, float *grad_accum,
                       float *denom, float *max_radii, void *stream) {
    if (P < 0 || (P > 0 && (!viewspace_grad || (!visible && !radii) || !grad_accum || !denom || (radii && !max_radii))))
        return 1;
    if (P == 0) return 0;
    hipLaunchKernelGGL(densify_stats_kernel, dim3((P + kTailThreads - 1) / kTailThreads), dim3(kTailThreads), 0,
                       (hipStream_t)stream, P, viewspace_grad, visible, radii, grad_accum, denom, max_radii);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int64_t gs4d_adam_chunks(int64_t n) { return (n + kAdamChunk - 1) / kAdamChunk; }

int gs4d_adam_step(const gs4d_adam_batch *batch, void *stream) {
    if (!batch || batch->count < 0 || batch->count > GS4D_ADAM_MAX_TENSORS) return 1;
    int64_t chunks = 0;
    for (int i = 0; i < batch->count; i++) {
        if (batch->t[i].first_chunk != chunks || batch->t[i].n < 0) return 1;
        chunks += gs4d_adam_chunks(batch->t[i].n);
    }
    if (chunks == 0) return 0;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)chunks), dim3(kTailThreads), 0, (hipStream_t)stream, *batch);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_hexplane_points(int N, const float *xyz, int64_t ld_xyz, const float *t, int64_t ld_t, const float *aabb,
                         float *pts, void *stream) {
    if (N < 0 || !aabb) return 1;
    if (N == 0) return 0;
    if (!xyz || !t || !pts || ((size_t)pts & 15) != 0 || ld_xyz < 3 || ld_t < 0) return 1;
    hipLaunchKernelGGL(hex_points_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, xyz, ld_xyz, t,
                       ld_t, aabb, (float4 *)pts);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_hexplane_points_backward_add(int N, const float *dpts, const float *aabb, const float *add, float *dxyz,
                                      void *stream) {
    if (N < 0 || !aabb) return 1;
    if (N == 0) return 0;
    if (!dpts || !dxyz || ((size_t)dpts & 15) != 0) return 1;
    hipLaunchKernelGGL(hex_points_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N,
                       (const float4 *)dpts, aabb, add, dxyz);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_hexplane_points_backward(int N, const float *dpts, const float *aabb, float *dxyz, void *stream) {
    return gs4d_hexplane_points_backward_add(N, dpts, aabb, nullptr, dxyz, stream);
}

}  // extern "C"
