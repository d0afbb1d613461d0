// ssim.hip -- the D-SSIM image loss of the train step and the SSIM metric: value, gradient and the fused
// L1 + D-SSIM form.  Kernels first, their gs4d_* entry points at the end of the file.
//
// Reference: utils/loss_utils.py:36-66 (ssim / _ssim): an 11x11 Gaussian window (sigma 1.5, normalised), zero
// padding of 5, one filter per channel, C1 = 0.01^2, C2 = 0.03^2, and the map
//   m = A B / (D E),  A = 2 mu1 mu2 + C1,  B = 2 s12 + C2,  D = mu1^2 + mu2^2 + C1,  E = s1 + s2 + C2,
// with s1 = w*x^2 - mu1^2, s2 = w*y^2 - mu2^2, s12 = w*xy - mu1 mu2.  Torch runs it as five grouped conv2d, a
// dozen element-wise kernels and their autograd backward (five transposed convolutions); here it is two
// launches.  The window is an outer product, so it is applied separably: 11 taps along the rows, then 11 along
// the columns.
//
// Pass 1 (ssim_forward_kernel): one workgroup owns a 32x32 tile of one (image, channel) plane.  It stages the
// tile and a 5-pixel halo of x and y in LDS (zeros outside the image: the padding), filters the five moments
// x, y, x^2, y^2, xy along the rows into LDS, then along the columns from LDS, forms m per pixel and adds it up
// over the tile.  For a gradient it also writes, per pixel, the derivatives of m by the filtered moments:
//   Ms = dm/d(w*x^2) = -m / E,   M12 = dm/d(w*xy) = 2 A / (D E),
//   Mm = dm/d(w*x)   = 2 mu2 B / (D E) - 2 mu1 m / D - 2 mu1 Ms - mu2 M12.
// Pass 2 (ssim_backward_kernel): the window is symmetric, so the adjoint of the zero-padded filter is the same
// zero-padded filter; the same tiling filters the three maps and gathers
//   grad_x(p) = u [ (w*Mm)(p) + 2 x(p) (w*Ms)(p) + y(p) (w*M12)(p) ]
// -- no atomics, every gradient element written once.  The fused form adds the L1 loss to both passes: pass 1
// also sums |x - y| (while it stages the tile), pass 2 adds sign(x - y) * (dloss / N) into the same store.
//
// Totals: the tiles of one image are the x dimension of the grid, so publish_and_total (train_internal.h) sums
// an image's tile sums in its fixed order, each image with its own ticket scratch; the last workgroups of the
// images then add the image totals in image order (image_totals below).  Value and gradient are bitwise
// repeatable.
//
// LDS: the staged rows have a pitch of 43 words (odd: the row pass reads 14 consecutive words per thread, the
// threads of a wave four apart in a row and a row apart: conflict-free); the row-filtered moments have a pitch
// of 32 words, written and read as 16-byte words (the column pass's 16-lane groups hold 8 words of two or three
// rows 32 words apart: conflict-free).  36 KB forward (the fifth moment reuses the staged images' space: four
// workgroups per CU), 38 KB backward (three per CU by its registers).
#include <math.h>

#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {

constexpr int kSsimTile = 32;                        // output tile edge
constexpr int kSsimR = 5;                            // window radius (window_size 11)
constexpr int kSsimIn = kSsimTile + 2 * kSsimR;      // staged edge: 42
constexpr int kSsimInPitch = kSsimIn + 1;            // 43
constexpr int kSsimRowTasks = kSsimIn * (kSsimTile / 4);  // row pass: 42 rows x 8 groups of 4 outputs
// utils/loss_utils.py:26-28 in fp32: exp(-(i - 5)^2 / 4.5) / sum
#define GS4D_SSIM_TAPS                                                                                             \
    {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005528f, 0.266011715f, 0.213005528f,      \
     0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f}
constexpr float kSsimC1 = (float)(0.01 * 0.01), kSsimC2 = (float)(0.03 * 0.03);

// where the totals of one call live (device pointers into the caller's scratch; see gs4d_ssim_scratch_bytes)
struct SsimTotals {
    unsigned char *per_image;  // image b, value v (0 SSIM, 1 L1): a ticket scratch at per_image + (2 b + v) * stride
    size_t stride;
    uint32_t *counter;         // [v]: images done
    unsigned long long *slot;  // [v * B + b]: image totals (bits + 1, 0 = not there yet)
};

// Thread 0 of an image's last workgroup holds that image's total `t` of value v.  Returns true in the thread
// that comes last over the images, with the sum of the image totals in image order; the slots and the counter
// are zero again then.  The protocol of publish_and_total: relaxed agent-scope stores, a bounded wait on a slot
// still reading 0, NaN if one never arrives.
__device__ inline bool image_totals(double t, const SsimTotals &st, int v, int B, double *total) {
    if (B == 1) {
        *total = t;
        return true;
    }
    unsigned long long *slot = st.slot + (size_t)v * B;
    __hip_atomic_store(slot + blockIdx.y, (unsigned long long)__double_as_longlong(t) + 1ull, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_fetch_add(st.counter + v, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (uint32_t)B - 1u)
        return false;
    double s = 0.0;
    bool lost = false;
    for (int b = 0; b < B; b++) {
        unsigned long long w = __hip_atomic_load(slot + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t spins = 0; w == 0ull && spins < (1u << 22); spins++)
            w = __hip_atomic_load(slot + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lost |= w == 0ull;
        __hip_atomic_store(slot + b, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w != 0ull) s += __longlong_as_double((long long)(w - 1ull));
    }
    __hip_atomic_store(st.counter + v, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *total = lost ? __builtin_nan("") : s;
    return true;
}

// the workgroup's sum of one float per thread, in thread 0 (wave tree, then the waves in order)
__device__ __forceinline__ double tile_sum(float acc, double *s_w) {
    double s = acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTailThreads / 64; w++) t += s_w[w];
    return t;
}

struct SsimTile {
    int64_t plane;  // offset of the (image, channel) plane
    int x0, y0;     // the tile's first pixel
};
__device__ __forceinline__ SsimTile ssim_tile(int C, int H, int W, int tiles_x, int tiles_y) {
    int t = (int)blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, c = t / tiles_y;
    return {((int64_t)blockIdx.y * C + c) * ((int64_t)H * W), tx * kSsimTile, ty * kSsimTile};
}

// The tile and its halo of N planes (p[k] at `plane`) into LDS (s + k * kSsimIn * kSsimInPitch), zeros outside the
// image: every load of the thread is issued before the first LDS store.  L1 (N == 2): returns the thread's share of
// the tile's sum |p0 - p1| (each pixel of the tile proper is staged by exactly one thread).
constexpr int kSsimStageIters = (kSsimIn * kSsimIn + kTailThreads - 1) / kTailThreads;  // 7
template <int N, bool L1>
__device__ __forceinline__ float ssim_stage(const float *const (&p)[N], int64_t plane, int H, int W, int x0, int y0,
                                            float *s) {
    float v[kSsimStageIters][N];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kSsimStageIters; k++) {
        const int i = (int)threadIdx.x + k * kTailThreads;
        const int r = i / kSsimIn, c = i - r * kSsimIn;
        const int gy = y0 - kSsimR + r, gx = x0 - kSsimR + c;
        const bool in = i < kSsimIn * kSsimIn && gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
        for (int m = 0; m < N; m++) v[k][m] = in ? p[m][plane + (int64_t)gy * W + gx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kSsimStageIters; k++) {
        const int i = (int)threadIdx.x + k * kTailThreads;
        const int r = i / kSsimIn, c = i - r * kSsimIn;
        if (i < kSsimIn * kSsimIn) {
#pragma unroll
            for (int m = 0; m < N; m++) s[m * (kSsimIn * kSsimInPitch) + r * kSsimInPitch + c] = v[k][m];
            // outside the image both are 0; the halo belongs to the neighbours' sums
            if (L1 && r >= kSsimR && r < kSsimR + kSsimTile && c >= kSsimR && c < kSsimR + kSsimTile)
                acc += fabsf(v[k][0] - v[k][N - 1]);
        }
    }
    return acc;
}

// MAPS: also write the three derivative maps (maps, maps + n, maps + 2 n; n = the element count of x);
// L1: also total |x - y|.  The means are written by the workgroup that finishes last (per_image may be NULL).
template <bool MAPS, bool L1>
__global__ __launch_bounds__(kTailThreads) void ssim_forward_kernel(int C, int H, int W, int tiles_x, int tiles_y,
                                                                    const float *__restrict__ x,
                                                                    const float *__restrict__ y,
                                                                    float *__restrict__ maps, int64_t n, int vec,
                                                                    SsimTotals st, float *__restrict__ mean,
                                                                    float *__restrict__ per_image,
                                                                    float *__restrict__ l1_mean) {
    constexpr float w[11] = GS4D_SSIM_TAPS;
    // the fifth row-filtered moment takes the staged images' place once every row task has read them: 36 KB
    // instead of 42, four workgroups per CU instead of three
    __shared__ __attribute__((aligned(16))) float s_in[2][kSsimIn * kSsimInPitch];
    __shared__ __attribute__((aligned(16))) float s_h[4][kSsimIn * kSsimTile];
    __shared__ double s_w[kTailThreads / 64];
    const SsimTile tile = ssim_tile(C, H, W, tiles_x, tiles_y);
    const float *const in2[2] = {x, y};
    const float acc_l1 = ssim_stage<2, L1>(in2, tile.plane, H, W, tile.x0, tile.y0, s_in[0]);
    __syncthreads();
    // along the rows: 4 adjacent outputs of one staged row per task, the five moments
    constexpr int kRounds = (kSsimRowTasks + kTailThreads - 1) / kTailThreads;  // 2
    float4 keep[kRounds];
#pragma unroll
    for (int round = 0; round < kRounds; round++) {
        const int task = (int)threadIdx.x + round * kTailThreads;
        if (task < kSsimRowTasks) {
            const int r = task >> 3, c0 = (task & 7) * 4;
            float a[14], b[14];
#pragma unroll
            for (int j = 0; j < 14; j++) {
                a[j] = s_in[0][r * kSsimInPitch + c0 + j];
                b[j] = s_in[1][r * kSsimInPitch + c0 + j];
            }
            float h[5][4];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                float sa = 0.f, sb = 0.f, saa = 0.f, sbb = 0.f, sab = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) {
                    const float av = a[o + k], bv = b[o + k];
                    sa = fmaf(w[k], av, sa);
                    sb = fmaf(w[k], bv, sb);
                    saa = fmaf(w[k], av * av, saa);
                    sbb = fmaf(w[k], bv * bv, sbb);
                    sab = fmaf(w[k], av * bv, sab);
                }
                h[0][o] = sa, h[1][o] = sb, h[2][o] = saa, h[3][o] = sbb, h[4][o] = sab;
            }
#pragma unroll
            for (int m = 0; m < 4; m++)
                *(float4 *)&s_h[m][r * kSsimTile + c0] = make_float4(h[m][0], h[m][1], h[m][2], h[m][3]);
            keep[round] = make_float4(h[4][0], h[4][1], h[4][2], h[4][3]);
        }
    }
    __syncthreads();  // the staged images are read
    float *s_h4 = s_in[0];
#pragma unroll
    for (int round = 0; round < kRounds; round++) {
        const int task = (int)threadIdx.x + round * kTailThreads;
        if (task < kSsimRowTasks) *(float4 *)&s_h4[(task >> 3) * kSsimTile + (task & 7) * 4] = keep[round];
    }
    __syncthreads();
    // along the columns: 4 adjacent pixels of one row per thread
    const int r = (int)threadIdx.x >> 3, c0 = ((int)threadIdx.x & 7) * 4;
    float f[5][4];
#pragma unroll
    for (int m = 0; m < 5; m++)
#pragma unroll
        for (int e = 0; e < 4; e++) f[m][e] = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
#pragma unroll
        for (int m = 0; m < 5; m++) {
            const float4 v = *(const float4 *)&(m < 4 ? s_h[m] : s_h4)[(r + k) * kSsimTile + c0];
            f[m][0] = fmaf(w[k], v.x, f[m][0]);
            f[m][1] = fmaf(w[k], v.y, f[m][1]);
            f[m][2] = fmaf(w[k], v.z, f[m][2]);
            f[m][3] = fmaf(w[k], v.w, f[m][3]);
        }
    }
    const int gy = tile.y0 + r, gx0 = tile.x0 + c0;
    float acc = 0.f;
    float ms[4], m12[4], mm[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float mu1 = f[0][e], mu2 = f[1][e];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float s1 = f[2][e] - mu1_sq, s2 = f[3][e] - mu2_sq, s12 = f[4][e] - mu1_mu2;
        const float A = 2.f * mu1_mu2 + kSsimC1, Bv = 2.f * s12 + kSsimC2;
        const float D = mu1_sq + mu2_sq + kSsimC1, E = s1 + s2 + kSsimC2;
        const float DE = D * E;
        const float m = (A * Bv) / DE;  // a true division: x == y gives exactly 1
        const bool in = gy < H && gx0 + e < W;
        if (in) acc += m;
        if (MAPS) {
            const float inv_de = 1.f / DE;
            const float inv_d = E * inv_de, inv_e = D * inv_de;
            ms[e] = -m * inv_e;
            m12[e] = 2.f * A * inv_de;
            // associated so that x == y (A == D, B == E, m == 1) cancels exactly: Mm == 0, M12 == -2 Ms
            mm[e] = 2.f * mu2 * (Bv * inv_de) - 2.f * mu1 * m * inv_d - 2.f * mu1 * ms[e] - mu2 * m12[e];
        }
    }
    if (MAPS && gy < H && gx0 < W) {
        const int64_t o = tile.plane + (int64_t)gy * W + gx0;
        if (vec) {  // W % 4 == 0: the four pixels are inside together
            *(float4 *)(maps + o) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *(float4 *)(maps + n + o) = make_float4(ms[0], ms[1], ms[2], ms[3]);
            *(float4 *)(maps + 2 * n + o) = make_float4(m12[0], m12[1], m12[2], m12[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (gx0 + e < W) {
                    maps[o + e] = mm[e];
                    maps[n + o + e] = ms[e];
                    maps[2 * n + o + e] = m12[e];
                }
        }
    }
    const int B = (int)gridDim.y;
    const double chw = (double)C * (double)H * (double)W;
    double t = tile_sum(acc, s_w), total;
    if (publish_and_total(t, ticket_scratch(st.per_image + (2 * (size_t)blockIdx.y) * st.stride), (int)gridDim.x,
                          &total) &&
        threadIdx.x == 0) {
        if (per_image) per_image[blockIdx.y] = (float)(total / chw);
        double all;
        if (image_totals(total, st, 0, B, &all)) *mean = (float)(all / (chw * (double)B));
    }
    if (L1) {
        __syncthreads();  // publish_and_total's shared words and s_w are used again
        t = tile_sum(acc_l1, s_w);
        if (publish_and_total(t, ticket_scratch(st.per_image + (2 * (size_t)blockIdx.y + 1) * st.stride),
                              (int)gridDim.x, &total) &&
            threadIdx.x == 0) {
            double all;
            if (image_totals(total, st, 1, B, &all)) *l1_mean = (float)(all / (chw * (double)B));
        }
    }
}

// grad = u (w*Mm + 2 x w*Ms + y w*M12) [+ sign(x - y) * l1_scale], u = up[b * up_stride] * scale (up NULL: scale)
template <bool L1>
__global__ __launch_bounds__(kTailThreads) void ssim_backward_kernel(int C, int H, int W, int tiles_x, int tiles_y,
                                                                     const float *__restrict__ x,
                                                                     const float *__restrict__ y,
                                                                     const float *__restrict__ maps, int64_t n, int vec,
                                                                     const float *__restrict__ up, int up_stride,
                                                                     float scale, float l1_scale,
                                                                     float *__restrict__ grad) {
    constexpr float w[11] = GS4D_SSIM_TAPS;
    __shared__ float s_in[3][kSsimIn * kSsimInPitch];
    __shared__ __attribute__((aligned(16))) float s_h[3][kSsimIn * kSsimTile];
    const SsimTile tile = ssim_tile(C, H, W, tiles_x, tiles_y);
    const float *const in3[3] = {maps, maps + n, maps + 2 * n};
    ssim_stage<3, false>(in3, tile.plane, H, W, tile.x0, tile.y0, s_in[0]);
    __syncthreads();
    for (int task = (int)threadIdx.x; task < kSsimRowTasks; task += kTailThreads) {
        const int r = task >> 3, c0 = (task & 7) * 4;
#pragma unroll
        for (int m = 0; m < 3; m++) {
            float a[14];
#pragma unroll
            for (int j = 0; j < 14; j++) a[j] = s_in[m][r * kSsimInPitch + c0 + j];
            float h[4];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) s = fmaf(w[k], a[o + k], s);
                h[o] = s;
            }
            *(float4 *)&s_h[m][r * kSsimTile + c0] = make_float4(h[0], h[1], h[2], h[3]);
        }
    }
    __syncthreads();
    const int r = (int)threadIdx.x >> 3, c0 = ((int)threadIdx.x & 7) * 4;
    const int gy = tile.y0 + r, gx0 = tile.x0 + c0;
    if (gy >= H || gx0 >= W) return;  // no barrier below
    float f[3][4];
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int e = 0; e < 4; e++) f[m][e] = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const float4 v = *(const float4 *)&s_h[m][(r + k) * kSsimTile + c0];
            f[m][0] = fmaf(w[k], v.x, f[m][0]);
            f[m][1] = fmaf(w[k], v.y, f[m][1]);
            f[m][2] = fmaf(w[k], v.z, f[m][2]);
            f[m][3] = fmaf(w[k], v.w, f[m][3]);
        }
    }
    const float u = (up ? up[(int64_t)blockIdx.y * up_stride] : 1.f) * scale;
    const int64_t o = tile.plane + (int64_t)gy * W + gx0;
    float xv[4], yv[4], g[4];
    if (vec) {
        const float4 a = *(const float4 *)(x + o), b = *(const float4 *)(y + o);
        xv[0] = a.x, xv[1] = a.y, xv[2] = a.z, xv[3] = a.w;
        yv[0] = b.x, yv[1] = b.y, yv[2] = b.z, yv[3] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool in = gx0 + e < W;
            xv[e] = in ? x[o + e] : 0.f;
            yv[e] = in ? y[o + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        g[e] = u * (f[0][e] + 2.f * xv[e] * f[1][e] + yv[e] * f[2][e]);
        if (L1) {
            const float d = xv[e] - yv[e];
            g[e] += (float)((d > 0.f) - (d < 0.f)) * l1_scale;  // torch.sign
        }
    }
    if (vec) {
        *(float4 *)(grad + o) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (gx0 + e < W) grad[o + e] = g[e];
    }
}

namespace {
struct SsimGeom {
    int tiles_x, tiles_y;
    int64_t tpi;  // tiles per image = the grid's x
    int64_t n;
};
// 0: launch, 1: bad argument, 2: nothing to do (an empty batch)
int ssim_geom(int B, int C, int H, int W, SsimGeom *g) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return 1;
    if (B == 0 || C == 0 || H == 0 || W == 0) return 2;
    if ((int64_t)H * W > INT32_MAX || B > 65535) return 1;
    g->tiles_x = (W + kSsimTile - 1) / kSsimTile;
    g->tiles_y = (H + kSsimTile - 1) / kSsimTile;
    g->tpi = (int64_t)C * g->tiles_x * g->tiles_y;
    if (g->tpi > INT32_MAX) return 1;
    g->n = (int64_t)B * C * H * W;
    return 0;
}
size_t ssim_stride(int64_t tpi) { return (4 * (size_t)kTicketWords + 8 * (size_t)tpi + 15) & ~(size_t)15; }
SsimTotals ssim_totals(void *scratch, int B, int64_t tpi) {
    unsigned char *p = (unsigned char *)(((size_t)scratch + 15) & ~(size_t)15);
    const size_t stride = ssim_stride(tpi);
    unsigned char *tail = p + 2 * (size_t)B * stride;
    return {p, stride, (uint32_t *)tail, (unsigned long long *)(tail + 16)};
}
bool aligned16(const void *p) { return ((size_t)p & 15) == 0; }
}  // namespace

}  // namespace gs4d

using namespace gs4d;

extern "C" {

size_t gs4d_ssim_scratch_bytes(int B, int C, int H, int W) {
    SsimGeom g;
    if (ssim_geom(B, C, H, W, &g) != 0) return 0;
    // the per-image tickets and slots, then the image counters and slots
    return 2 * (size_t)B * ssim_stride(g.tpi) + 16 + 16 * (size_t)B + 256;
}

int gs4d_ssim_forward(int B, int C, int H, int W, const float *x, const float *y, float *maps, float *mean,
                      float *per_image, void *scratch, void *stream) {
    SsimGeom g;
    const int st = ssim_geom(B, C, H, W, &g);
    if (st == 1 || !mean || (B > 0 && !per_image)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (st == 2) {
        if (hipMemsetAsync(mean, 0, 4, s) != hipSuccess) return 3;
        if (B > 0 && hipMemsetAsync(per_image, 0, 4 * (size_t)B, s) != hipSuccess) return 3;
        return 0;
    }
    if (!x || !y || !scratch) return 1;
    const int vec = W % 4 == 0 && aligned16(maps);
    const dim3 grid((unsigned)g.tpi, (unsigned)B);
    const SsimTotals tot = ssim_totals(scratch, B, g.tpi);
    if (maps)
        hipLaunchKernelGGL((ssim_forward_kernel<true, false>), grid, dim3(kTailThreads), 0, s, C, H, W, g.tiles_x,
                           g.tiles_y, x, y, maps, g.n, vec, tot, mean, per_image, (float *)nullptr);
    else
        hipLaunchKernelGGL((ssim_forward_kernel<false, false>), grid, dim3(kTailThreads), 0, s, C, H, W, g.tiles_x,
                           g.tiles_y, x, y, (float *)nullptr, g.n, 0, tot, mean, per_image, (float *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_ssim_backward(int B, int C, int H, int W, const float *x, const float *y, const float *maps,
                       const float *dvalue, int per_image, float *grad_x, void *stream) {
    SsimGeom g;
    const int st = ssim_geom(B, C, H, W, &g);
    if (st == 1) return 1;
    if (st == 2) return 0;
    if (!x || !y || !maps || !dvalue || !grad_x) return 1;
    const int vec = W % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(grad_x);
    // d mean / d map element: 1 / count, rounded as torch's MeanBackward (grad * (1 / numel))
    const float scale = 1.0f / (float)(per_image ? g.n / B : g.n);
    hipLaunchKernelGGL((ssim_backward_kernel<false>), dim3((unsigned)g.tpi, (unsigned)B), dim3(kTailThreads), 0,
                       (hipStream_t)stream, C, H, W, g.tiles_x, g.tiles_y, x, y, maps, g.n, vec, dvalue,
                       per_image ? 1 : 0, scale, 0.f, grad_x);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int gs4d_l1_dssim_loss_grad(int B, int C, int H, int W, const float *x, const float *y, float lambda, float dloss,
                            float *maps, float *l1, float *ssim, float *grad_x, void *scratch, void *stream) {
    SsimGeom g;
    const int st = ssim_geom(B, C, H, W, &g);
    if (st == 1 || !l1 || !ssim) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (st == 2) {
        if (hipMemsetAsync(l1, 0, 4, s) != hipSuccess || hipMemsetAsync(ssim, 0, 4, s) != hipSuccess) return 3;
        return 0;
    }
    if (!x || !y || !maps || !grad_x || !scratch) return 1;
    const dim3 grid((unsigned)g.tpi, (unsigned)B);
    const SsimTotals tot = ssim_totals(scratch, B, g.tpi);
    hipLaunchKernelGGL((ssim_forward_kernel<true, true>), grid, dim3(kTailThreads), 0, s, C, H, W, g.tiles_x, g.tiles_y,
                       x, y, maps, g.n, (int)(W % 4 == 0 && aligned16(maps)), tot, ssim, (float *)nullptr, l1);
    if (hipGetLastError() != hipSuccess) return 3;
    // loss = dloss * (L1 + lambda * (1 - ssim)): the means' gradients, rounded as MeanBackward does
    const float inv_n = 1.0f / (float)g.n;
    const int vec = W % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(grad_x);
    hipLaunchKernelGGL((ssim_backward_kernel<true>), grid, dim3(kTailThreads), 0, s, C, H, W, g.tiles_x, g.tiles_y, x, y,
                       maps, g.n, vec, (const float *)nullptr, 0, -(dloss * lambda) * inv_n, dloss * inv_n, grad_x);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // extern "C"
