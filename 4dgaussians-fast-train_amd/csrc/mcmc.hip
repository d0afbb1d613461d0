// mcmc.hip -- the opt-in MCMC densification strategy's kernels (3DGS-MCMC, Kheradmand et al. 2024; gsplat's
// MCMCStrategy is the model; no counterpart in the reference): a counter-based generator, the opacity-proportional
// sampler of relocation and growth, the opacity / scale correction of the sampled sources, the per-step position
// noise, the opacity / scale regulariser's value and gradient, and the zeroing of the Adam moments' rows.
//
//   generator  Philox4x32-10, key (seed lo, seed hi), counter (j, purpose, iteration, 0): every draw is a function
//              of (seed, iteration, purpose, j) alone, so data-parallel replicas make the same draws with no
//              collective and a call repeats its bits.  Plain 32-bit integer VALU code.
//   sample     w_i = (u64)(o_i 2^32) where o_i > min_opacity, else 0 (exact: a power-of-two scaling); inclusive
//              64-bit prefix sums S in three launches (tile sums of 256, one workgroup scanning the tile sums, the
//              tiles' own scans), integer and therefore the same whatever the order; draw d takes u = w0 | w1 << 32 of
//              block d, t = mulhi64(u, S[P-1]) and picks by binary search the first row with S[i] > t; counts by
//              integer atomics.
//   relocate   one lane per row with counts > 0: n = min(counts + 1, 51), o' = -expm1(log1p(-o) / n), the
//              denominator D = sum_{i=1..n} sum_{k<i} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1) in fp64 over a constant
//              table of binomials, s' = s o / D; stores logit(o') and log(s').
//   noise      one lane per row, one launch: x += R diag(s^2) R^T (z g step_scale), z three Box-Muller normals of
//              the row's block (or the caller's), g the opacity gate.
//   reg_grad   value = w_o mean(sigmoid(o)) + w_s mean(exp(s)), its gradient ADDED to the given buffers; the value
//              by a per-workgroup tree and a second small launch in fp64 in a fixed order (no float atomics).
//   zero_rows  the listed rows of up to GS4D_ROWS_MAX_TENSORS float tensors set to zero in one launch.
#include <cfloat>

#include "../../include/gs4d.h"
#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {
namespace {

constexpr int kMcThreads = 256;
constexpr int kMcMaxN = 51;  // the correction's largest n (gsplat's N_MAX)

// ---- Philox4x32-10 --------------------------------------------------------------------------------------------------
struct Philox4 {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ Philox4 mcmc_block(uint32_t j, uint32_t purpose, uint32_t iteration, uint64_t seed) {
    return philox4x32_10(j, purpose, iteration, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__global__ __launch_bounds__(kMcThreads) void mcmc_bits_kernel(int n, uint64_t seed, uint32_t iteration, uint32_t purpose,
                                                               uint32_t *__restrict__ out) {
    const int j = blockIdx.x * kMcThreads + threadIdx.x;
    if (j >= n) return;
    const Philox4 b = mcmc_block((uint32_t)j, purpose, iteration, seed);
#pragma unroll
    for (int k = 0; k < 4; k++) out[4 * (size_t)j + k] = b.w[k];
}

// ---- the sampler ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mcmc_weight(float o, float min_opacity) {
    // o 2^32 is exact; a NaN compares false (weight 0); an opacity above 1 (never a sigmoid's) counts as 1
    return o > min_opacity ? (uint64_t)(fminf(o, 1.f) * 4294967296.f) : 0ull;
}

// the workgroup's inclusive scan of one value per thread (Hillis-Steele over LDS; integers: any order, same sums)
__device__ __forceinline__ uint64_t mcmc_block_scan(uint64_t v, uint64_t *s) {
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kMcThreads; off <<= 1) {
        const uint64_t add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    return s[threadIdx.x];
}

__global__ __launch_bounds__(kMcThreads) void mcmc_tile_sum_kernel(int P, const float *__restrict__ opacity,
                                                                   float min_opacity, uint64_t *__restrict__ tile_sum) {
    __shared__ uint64_t s[kMcThreads];
    const int i = blockIdx.x * kMcThreads + threadIdx.x;
    const uint64_t incl = mcmc_block_scan(i < P ? mcmc_weight(opacity[i], min_opacity) : 0ull, s);
    if (threadIdx.x == kMcThreads - 1) tile_sum[blockIdx.x] = incl;
}

// one workgroup: tile_sum[b] becomes the sum of the tiles before b (exclusive), chunk after chunk with a carry
__global__ __launch_bounds__(kMcThreads) void mcmc_tile_scan_kernel(int nblk, uint64_t *__restrict__ tile_sum) {
    __shared__ uint64_t s[kMcThreads];
    uint64_t carry = 0ull;
    for (int b0 = 0; b0 < nblk; b0 += kMcThreads) {
        const int b = b0 + threadIdx.x;
        const uint64_t v = b < nblk ? tile_sum[b] : 0ull;
        const uint64_t incl = mcmc_block_scan(v, s);
        if (b < nblk) tile_sum[b] = carry + incl - v;
        const uint64_t chunk = s[kMcThreads - 1];
        __syncthreads();  // s is reused by the next chunk's scan
        carry += chunk;
    }
}

__global__ __launch_bounds__(kMcThreads) void mcmc_prefix_kernel(int P, const float *__restrict__ opacity, float min_opacity,
                                                                 const uint64_t *__restrict__ tile_sum,
                                                                 uint64_t *__restrict__ S, int32_t *__restrict__ counts) {
    __shared__ uint64_t s[kMcThreads];
    const int i = blockIdx.x * kMcThreads + threadIdx.x;
    const uint64_t incl = mcmc_block_scan(i < P ? mcmc_weight(opacity[i], min_opacity) : 0ull, s);
    if (i < P) {
        S[i] = tile_sum[blockIdx.x] + incl;
        counts[i] = 0;
    }
}

__global__ __launch_bounds__(kMcThreads) void mcmc_draw_kernel(int P, int n, const uint64_t *__restrict__ S, uint64_t seed,
                                                               uint32_t iteration, uint32_t purpose,
                                                               int32_t *__restrict__ draws, int32_t *__restrict__ counts,
                                                               int32_t *__restrict__ n_drawn) {
    const int d = blockIdx.x * kMcThreads + threadIdx.x;
    const uint64_t total = S[P - 1];
    if (d == 0 && n_drawn) *n_drawn = total ? n : 0;
    if (d >= n || total == 0ull) return;
    const Philox4 b = mcmc_block((uint32_t)d, purpose, iteration, seed);
    const uint64_t u = (uint64_t)b.w[0] | ((uint64_t)b.w[1] << 32);
    const uint64_t t = __umul64hi(u, total);  // < total = S[P - 1]: the search ends inside [0, P - 1]
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (S[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    draws[d] = lo;
    atomicAdd(counts + lo, 1);
}

// ---- the correction of relocation's sources ---------------------------------------------------------------------------
struct McmcTables {
    double binom[kMcMaxN][kMcMaxN];  // C(i, k), exact in fp64 (C(50, 25) < 2^47)
};

constexpr McmcTables mcmc_make_tables() {
    McmcTables t{};
    for (int i = 0; i < kMcMaxN; i++)
        for (int k = 0; k <= i; k++) t.binom[i][k] = (k == 0 || k == i) ? 1.0 : t.binom[i - 1][k - 1] + t.binom[i - 1][k];
    return t;
}

// built once, by the host compiler's constant evaluation; part of the code object of every device
__constant__ McmcTables c_mcmc = mcmc_make_tables();

__global__ __launch_bounds__(kMcThreads) void mcmc_relocate_kernel(int P, const int32_t *__restrict__ counts,
                                                                   float min_opacity, float *__restrict__ opacity_raw,
                                                                   float *__restrict__ scaling_raw) {
    const int r = blockIdx.x * kMcThreads + threadIdx.x;
    if (r >= P) return;
    const int c = counts[r];
    if (c <= 0) return;
    const int n = min(c, kMcMaxN - 1) + 1;
    const float o = 1.f / (1.f + expf(-opacity_raw[r]));
    float o_new = -expm1f(log1pf(-o) / (float)n);
    const double q = (double)o_new;
    double D = 0.0;
    for (int i = 1; i <= n; i++) {
        double pw = q, sgn = 1.0;  // o'^(k+1), (-1)^k
        for (int k = 0; k < i; k++) {
            D += c_mcmc.binom[i - 1][k] * sgn * pw / sqrt((double)(k + 1));
            pw *= q;
            sgn = -sgn;
        }
    }
    const float ratio = (float)((double)o / D);
    o_new = fminf(fmaxf(o_new, min_opacity), 1.f - FLT_EPSILON);
    opacity_raw[r] = logf(o_new / (1.f - o_new));
#pragma unroll
    for (int a = 0; a < 3; a++) scaling_raw[3 * (size_t)r + a] = logf(expf(scaling_raw[3 * (size_t)r + a]) * ratio);
}

// ---- the per-step position noise --------------------------------------------------------------------------------------
__device__ __forceinline__ float mcmc_unit(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 0x1p-24f; }

__global__ __launch_bounds__(kMcThreads) void mcmc_noise_kernel(int P, const float *__restrict__ scaling_raw,
                                                                const float *__restrict__ rotation_raw,
                                                                const float *__restrict__ opacity_raw, float step_scale,
                                                                uint64_t seed, uint32_t iteration,
                                                                const float *__restrict__ normals, float *__restrict__ xyz) {
    const int r = blockIdx.x * kMcThreads + threadIdx.x;
    if (r >= P) return;
    float z[3];
    if (normals) {
#pragma unroll
        for (int a = 0; a < 3; a++) z[a] = normals[3 * (size_t)r + a];
    } else {
        const Philox4 b = mcmc_block((uint32_t)r, 0u, iteration, seed);
        const float u0 = mcmc_unit(b.w[0]), u1 = mcmc_unit(b.w[1]), u2 = mcmc_unit(b.w[2]), u3 = mcmc_unit(b.w[3]);
        const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
        const float two_pi = 6.283185307179586f;
        z[0] = r0 * cosf(two_pi * u1);
        z[1] = r0 * sinf(two_pi * u1);
        z[2] = r1 * cosf(two_pi * u3);
    }
    const float o = 1.f / (1.f + expf(-opacity_raw[r]));
    const float g = 1.f / (1.f + expf(-100.f * ((1.f - o) - 0.995f)));
    const float gs = g * step_scale;
    float v[3], s2[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        v[a] = z[a] * gs;
        const float s = expf(scaling_raw[3 * (size_t)r + a]);
        s2[a] = s * s;
    }
    float qw = rotation_raw[4 * (size_t)r], qx = rotation_raw[4 * (size_t)r + 1], qy = rotation_raw[4 * (size_t)r + 2],
          qz = rotation_raw[4 * (size_t)r + 3];
    const float nq = fmaxf(sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz), 1e-12f);
    qw /= nq, qx /= nq, qy /= nq, qz /= nq;
    const float R[3][3] = {{1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qw * qz), 2.f * (qx * qz + qw * qy)},
                           {2.f * (qx * qy + qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qw * qx)},
                           {2.f * (qx * qz - qw * qy), 2.f * (qy * qz + qw * qx), 1.f - 2.f * (qx * qx + qy * qy)}};
    float t[3];  // diag(s^2) R^T v
#pragma unroll
    for (int a = 0; a < 3; a++) t[a] = s2[a] * ((R[0][a] * v[0] + R[1][a] * v[1]) + R[2][a] * v[2]);
#pragma unroll
    for (int a = 0; a < 3; a++) xyz[3 * (size_t)r + a] += (R[a][0] * t[0] + R[a][1] * t[1]) + R[a][2] * t[2];
}

// ---- the regulariser ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMcThreads) void mcmc_reg_kernel(int P, const float *__restrict__ opacity_raw,
                                                              const float *__restrict__ scaling_raw, float go, float gsc,
                                                              double co, double cs, float *__restrict__ grad_o,
                                                              float *__restrict__ grad_s, double *__restrict__ part) {
    const int r = blockIdx.x * kMcThreads + threadIdx.x;
    double val = 0.0;
    if (r < P) {
        const float o = 1.f / (1.f + expf(-opacity_raw[r]));
        if (grad_o) grad_o[r] += go * (o * (1.f - o));
        double ssum = 0.0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float s = expf(scaling_raw[3 * (size_t)r + a]);
            if (grad_s) grad_s[3 * (size_t)r + a] += gsc * s;
            ssum += (double)s;
        }
        val = co * (double)o + cs * ssum;
    }
    __shared__ double s_w[kMcThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) val += __shfl_xor(val, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = val;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kMcThreads / 64; w++) s += s_w[w];
        part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kMcThreads) void mcmc_reg_total_kernel(int nblk, const double *__restrict__ part,
                                                                    float *__restrict__ value) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kMcThreads) s += part[b];
    __shared__ double s_w[kMcThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kMcThreads / 64; w++) t += s_w[w];
        *value = (float)t;
    }
}

// ---- zeroing rows -------------------------------------------------------------------------------------------------------
// blockIdx.y: the tensor; the grid's x threads stride over (listed row, column) pairs
__global__ __launch_bounds__(kMcThreads) void mcmc_zero_rows_kernel(gs4d_zero_rows_batch b) {
    const gs4d_zero_rows_tensor t = b.t[blockIdx.y];
    const int64_t total = b.n * t.width;
    for (int64_t e = (int64_t)blockIdx.x * kMcThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kMcThreads) {
        const int64_t j = e / t.width, c = e - j * t.width;
        const int64_t row = b.rows[j];
        if (row >= 0 && row < b.P) t.data[row * t.width + c] = 0.f;  // a foreign index is skipped, never written through
    }
}

int mcmc_fail(int code, const std::string &what) { return train_fail(code, "mcmc: " + what); }

int mcmc_launched() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mcmc_fail(GS4D_ERR_HIP, hipGetErrorString(e));
    return GS4D_OK;
}

inline int mcmc_blocks(int64_t n) { return (int)((n + kMcThreads - 1) / kMcThreads); }

}  // namespace
}  // namespace gs4d

using namespace gs4d;

extern "C" int gs4d_mcmc_random_bits(int n_blocks, uint64_t seed, uint32_t iteration, uint32_t purpose, uint32_t *out,
                                     void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_blocks < 0) return mcmc_fail(GS4D_ERR_ARG, "n_blocks must be >= 0");
    if (n_blocks == 0) return GS4D_OK;
    if (!out) return mcmc_fail(GS4D_ERR_ARG, "missing the output buffer");
    hipLaunchKernelGGL(mcmc_bits_kernel, dim3(mcmc_blocks(n_blocks)), dim3(kMcThreads), 0, stream, n_blocks, seed,
                       iteration, purpose, out);
    return mcmc_launched();
}

extern "C" int gs4d_mcmc_sample(int P, const float *opacity, float min_opacity, int n, uint64_t seed, uint32_t iteration,
                                uint32_t purpose, int32_t *draws, int32_t *counts, int32_t *n_drawn,
                                gs4d_alloc_fn scratch_alloc, void *scratch_ctx, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || n < 0) return mcmc_fail(GS4D_ERR_ARG, "P and n must be >= 0");
    if (!(min_opacity >= 0.f)) return mcmc_fail(GS4D_ERR_ARG, "min_opacity must be >= 0");
    if (P == 0 || n == 0) return GS4D_OK;
    if (!opacity || !draws || !counts) return mcmc_fail(GS4D_ERR_ARG, "missing buffers");
    if (!scratch_alloc) return mcmc_fail(GS4D_ERR_ARG, "missing the scratch allocator");
    const int nblk = mcmc_blocks(P);
    char *scratch = scratch_alloc(scratch_ctx, sizeof(uint64_t) * ((size_t)P + (size_t)nblk) + 256);
    if (!scratch) return mcmc_fail(GS4D_ERR_ALLOC, "scratch allocation failed");
    uint64_t *S = (uint64_t *)align_up((size_t)scratch, 256);
    uint64_t *tile_sum = S + P;
    hipLaunchKernelGGL(mcmc_tile_sum_kernel, dim3(nblk), dim3(kMcThreads), 0, stream, P, opacity, min_opacity, tile_sum);
    hipLaunchKernelGGL(mcmc_tile_scan_kernel, dim3(1), dim3(kMcThreads), 0, stream, nblk, tile_sum);
    hipLaunchKernelGGL(mcmc_prefix_kernel, dim3(nblk), dim3(kMcThreads), 0, stream, P, opacity, min_opacity, tile_sum, S,
                       counts);
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3(mcmc_blocks(n)), dim3(kMcThreads), 0, stream, P, n, S, seed, iteration,
                       purpose, draws, counts, n_drawn);
    return mcmc_launched();
}

extern "C" int gs4d_mcmc_relocate(int P, const int32_t *counts, float min_opacity, float *opacity_raw, float *scaling_raw,
                                  void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return mcmc_fail(GS4D_ERR_ARG, "P must be >= 0");
    if (!(min_opacity > 0.f && min_opacity < 1.f)) return mcmc_fail(GS4D_ERR_ARG, "min_opacity must be in (0, 1)");
    if (P == 0) return GS4D_OK;
    if (!counts || !opacity_raw || !scaling_raw) return mcmc_fail(GS4D_ERR_ARG, "missing buffers");
    hipLaunchKernelGGL(mcmc_relocate_kernel, dim3(mcmc_blocks(P)), dim3(kMcThreads), 0, stream, P, counts, min_opacity,
                       opacity_raw, scaling_raw);
    return mcmc_launched();
}

extern "C" int gs4d_mcmc_noise(int P, float *xyz, const float *scaling_raw, const float *rotation_raw,
                               const float *opacity_raw, float step_scale, uint64_t seed, uint32_t iteration,
                               const float *normals, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return mcmc_fail(GS4D_ERR_ARG, "P must be >= 0");
    if (P == 0) return GS4D_OK;
    if (!xyz || !scaling_raw || !rotation_raw || !opacity_raw) return mcmc_fail(GS4D_ERR_ARG, "missing buffers");
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(mcmc_blocks(P)), dim3(kMcThreads), 0, stream, P, scaling_raw, rotation_raw,
                       opacity_raw, step_scale, seed, iteration, normals, xyz);
    return mcmc_launched();
}

extern "C" int gs4d_mcmc_reg_grad(int P, const float *opacity_raw, const float *scaling_raw, float w_opacity, float w_scale,
                                  float *value, float *grad_opacity, float *grad_scaling, gs4d_alloc_fn scratch_alloc,
                                  void *scratch_ctx, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return mcmc_fail(GS4D_ERR_ARG, "P must be >= 0");
    if (P == 0) return GS4D_OK;
    if (!opacity_raw || !scaling_raw || !value) return mcmc_fail(GS4D_ERR_ARG, "missing buffers");
    if (!scratch_alloc) return mcmc_fail(GS4D_ERR_ARG, "missing the scratch allocator");
    const int nblk = mcmc_blocks(P);
    char *scratch = scratch_alloc(scratch_ctx, sizeof(double) * (size_t)nblk + 256);
    if (!scratch) return mcmc_fail(GS4D_ERR_ALLOC, "scratch allocation failed");
    double *part = (double *)align_up((size_t)scratch, 256);
    const double co = (double)w_opacity / (double)P, cs = (double)w_scale / (3.0 * (double)P);
    hipLaunchKernelGGL(mcmc_reg_kernel, dim3(nblk), dim3(kMcThreads), 0, stream, P, opacity_raw, scaling_raw, (float)co,
                       (float)cs, co, cs, grad_opacity, grad_scaling, part);
    hipLaunchKernelGGL(mcmc_reg_total_kernel, dim3(1), dim3(kMcThreads), 0, stream, nblk, part, value);
    return mcmc_launched();
}

extern "C" int gs4d_mcmc_zero_rows(const gs4d_zero_rows_batch *b, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!b) return mcmc_fail(GS4D_ERR_ARG, "zero_rows: missing the batch");
    if (b->count < 0 || b->count > GS4D_ROWS_MAX_TENSORS) return mcmc_fail(GS4D_ERR_ARG, "zero_rows: 0..32 tensors");
    if (b->P < 0 || b->n < 0 || b->n > ((int64_t)1 << 31) - 1) return mcmc_fail(GS4D_ERR_ARG, "zero_rows: P and n must be >= 0");
    if (b->count == 0 || b->n == 0 || b->P == 0) return GS4D_OK;
    if (!b->rows) return mcmc_fail(GS4D_ERR_ARG, "zero_rows: missing the row list");
    int64_t wmax = 0;
    for (int i = 0; i < b->count; i++) {
        if (!b->t[i].data || b->t[i].width < 1 || b->t[i].width > ((int64_t)1 << 20))
            return mcmc_fail(GS4D_ERR_ARG, "zero_rows: a tensor needs its data and a width in 1..2^20");
        wmax = b->t[i].width > wmax ? b->t[i].width : wmax;
    }
    int64_t nblk = (b->n * wmax + kMcThreads - 1) / kMcThreads;
    nblk = nblk < 1 ? 1 : (nblk > 4096 ? 4096 : nblk);
    hipLaunchKernelGGL(mcmc_zero_rows_kernel, dim3((unsigned)nblk, (unsigned)b->count), dim3(kMcThreads), 0, stream, *b);
    return mcmc_launched();
}
