// voxel.hip -- Instant4D grid pruning: voxel downsample of the initial point cloud (gs4d_voxel_downsample).
//
// Replaces the Open3D call of utils/grid_pruning.py:16-41 (PointCloud::VoxelDownSample), which
// scene/__init__.py:106-119 runs on the host before create_from_pcd.  The result is defined by these
// semantics (include/gs4d.h states them for callers):
//   origin = per-axis min of the points (as fp64) - voxel_size / 2;
//   voxel index per axis = floor((double(p) - origin) / voxel_size), fp64, true division, no contraction;
//   one output row per occupied voxel: the mean of its points (and colours), summed in fp64 in a fixed
//   order and rounded once to fp32, rows ascending in the linear index (iz ny + iy) nx + ix.
// MI355X mapping, one pass per stage:
//   bounds    fp32 min/max by wave shuffles and at most one order-preserving integer atomic per workgroup
//             and axis (knn.hip's reduction without its origin seed; a NaN coordinate counts as an infinite
//             bound on both sides, so the host sees it);     -> host readback 1 (six words)
//   keys      the 64-bit linear index per point, low and high word in arrays of their own, and the low
//             word's sharded digit histograms;
//   sort      radix_sort.h's stable onesweep LSD sort of (key, point index): one sort over
//             ceil(log2(nx ny nz)) bits when they fit a word, else the low word and then, stably, the high
//             word gathered through the permutation -- only the 8-bit passes that hold live bits;
//   heads     a key that differs from its predecessor starts a voxel; voxel number = exclusive scan of the
//             head flags (chunk prefixes by block_prefix / sum_published), first[v] = the voxel's first
//             sorted position, so its count is first[v + 1] - first[v]: an exact integer, no sum;
//   segments  a lane per sorted point, a wave per 64: segmented inclusive scan of the fp64 values by a
//             fixed DPP tree (the pattern of contrib_segments_kernel in preprocess_backward.hip); a voxel
//             inside one wave is divided by its count, rounded and written, a piece that crosses a wave
//             boundary goes to part[w][0] (continues from the wave before) or part[w][1] (starts here);
//   finish    a wave per voxel that crosses waves: lane l adds pieces w0 + 1 + l, + 64, ... in that order,
//             lane 0 starts from the head piece, then one fixed xor tree; divided, rounded, written.
//             The work per voxel is spread over 64 lanes whatever the run length (all N points in one
//             voxel included), and the order of every addition is a function of N and the sorted order
//             only: no floating-point atomics, bitwise-repeatable results.
//   -> host readback 2 (M and the chunk-prefix error word).
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/gs4d.h"
#include "radix_sort.h"

namespace gs4d {

int train_fail(int code, const std::string &msg);  // capi.hip: sets gs4d_last_error()

namespace {

constexpr int kVoxThreads = 256;
constexpr int kVoxSortThreads = 1024, kVoxSortItems = 4;  // keys per sort workgroup: 4096, as the kNN's Morton sort
constexpr int kVoxMaxChunks = 1024;                        // head-scan chunks: each sums at most this many prefixes
constexpr int kVoxAxisLimit = 1 << 21;                     // voxels per axis: three indices fit 63 bits
// header words of the scratch: [0..5] bounds, [8] chunk-prefix error flag, [9] M
constexpr int kVoxErr = 8, kVoxM = 9, kVoxHeader = 64;

// order-preserving float <-> u32 map for integer atomic min/max (knn.hip's, on bit patterns: the host decodes too)
__host__ __device__ inline uint32_t vox_f2ord(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline uint32_t vox_ord2f(uint32_t u) { return (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u; }

// bounds[0..2] = ord(min), pre-set to 0xFFFFFFFF; bounds[3..5] = ord(max), pre-set to 0
__global__ __launch_bounds__(kVoxThreads) void voxel_bounds_kernel(int N, const float *__restrict__ pts,
                                                                   uint32_t *__restrict__ bounds) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto take = [&](int c, float v) {
        if (v != v) {  // fminf / fmaxf drop a NaN: make it an infinite bound on both sides
            mn[c] = -INFINITY;
            v = INFINITY;
        }
        mn[c] = fminf(mn[c], v);
        mx[c] = fmaxf(mx[c], v);
    };
    // four points = three 16-byte loads per lane while the array is 16-byte aligned, the rest one by one
    const int tid = blockIdx.x * kVoxThreads + threadIdx.x, stride = gridDim.x * kVoxThreads;
    const int quads = (((size_t)pts & 15) == 0) ? N / 4 : 0;
    const float4 *p4 = reinterpret_cast<const float4 *>(pts);
    for (int q = tid; q < quads; q += stride) {
        const float4 a = p4[3 * (size_t)q], b = p4[3 * (size_t)q + 1], c = p4[3 * (size_t)q + 2];
        take(0, a.x), take(1, a.y), take(2, a.z);
        take(0, a.w), take(1, b.x), take(2, b.y);
        take(0, b.z), take(1, b.w), take(2, c.x);
        take(0, c.y), take(1, c.z), take(2, c.w);
    }
    for (int i = 4 * quads + tid; i < N; i += stride) {
#pragma unroll
        for (int c = 0; c < 3; c++) take(c, pts[3 * (size_t)i + c]);
    }
    __shared__ float s[6][kVoxThreads / 64];
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], off));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off));
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s[c][w] = mn[c];
            s[3 + c][w] = mx[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = s[c][0];
        for (int q = 1; q < kVoxThreads / 64; q++) v = c < 3 ? fminf(v, s[c][q]) : fmaxf(v, s[c][q]);
        // Same-address atomics serialise (with one per workgroup and axis, 977 workgroups took 26 us where 98 took
        // 5: DESIGN 10.6), so a workgroup issues one only when it would move the bound.  The bound moves one way:
        // a stale read costs an atomic that changes nothing, never a missed one.
        const uint32_t o = vox_f2ord(__float_as_uint(v)), cur = load_word(&bounds[c]);
        if (c < 3 ? o < cur : o > cur) {
            if (c < 3) atomicMin(&bounds[c], o);
            else atomicMax(&bounds[c], o);
        }
    }
}

struct VoxGrid {
    double origin[3];
    double voxel;
    uint64_t nx, ny;
};

// flush a workgroup's four 256-bin digit histograms into its shard of the sort's histograms
__device__ __forceinline__ void flush_hist(uint32_t (*s_hist)[256], uint32_t *__restrict__ hist) {
    uint32_t *h = hist + (blockIdx.x % kHistShards) * (kMaxPasses * 256);
#pragma unroll
    for (int p = 0; p < 4; p++)
        if (s_hist[p][threadIdx.x]) atomicAdd(&h[p * 256 + threadIdx.x], s_hist[p][threadIdx.x]);
}

// lo[i] | hi[i] << 32 = (iz ny + iy) nx + ix; lo_sort = the copy the sort consumes
__global__ __launch_bounds__(kVoxThreads) void voxel_keys_kernel(int N, const float *__restrict__ pts, VoxGrid g,
                                                                 uint32_t *__restrict__ lo_sort,
                                                                 uint32_t *__restrict__ lo, uint32_t *__restrict__ hi,
                                                                 uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_hist[4][256];
    for (int p = 0; p < 4; p++) s_hist[p][threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * kVoxThreads + threadIdx.x;
    if (i < N) {
        uint64_t ix[3];
#pragma unroll
        for (int c = 0; c < 3; c++)
            ix[c] = (uint64_t)(int64_t)floor(((double)pts[3 * (size_t)i + c] - g.origin[c]) / g.voxel);
        const uint64_t key = (ix[2] * g.ny + ix[1]) * g.nx + ix[0];
        const uint32_t l = (uint32_t)key;
        lo_sort[i] = l;
        lo[i] = l;
        hi[i] = (uint32_t)(key >> 32);
#pragma unroll
        for (int p = 0; p < 4; p++) atomicAdd(&s_hist[p][(l >> (8 * p)) & 0xFFu], 1u);
    }
    __syncthreads();
    flush_hist(s_hist, hist);
}

// the high words in the order the low-word sort left, with their digit histograms
__global__ __launch_bounds__(kVoxThreads) void voxel_gather_hi_kernel(int N, const uint32_t *__restrict__ order,
                                                                      const uint32_t *__restrict__ hi,
                                                                      uint32_t *__restrict__ hi_sorted,
                                                                      uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_hist[4][256];
    for (int p = 0; p < 4; p++) s_hist[p][threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * kVoxThreads + threadIdx.x;
    if (i < N) {
        const uint32_t h = hi[order[i]];
        hi_sorted[i] = h;
#pragma unroll
        for (int p = 0; p < 4; p++) atomicAdd(&s_hist[p][(h >> (8 * p)) & 0xFFu], 1u);
    }
    __syncthreads();
    flush_hist(s_hist, hist);
}

// The key at sorted position i.  One-word sort: keys = the sorted low words, lo = hi_sorted = nullptr.
// Two-word sort: keys = the sorted high words, lo = the low words by point, read through the permutation.
struct VoxSorted {
    const uint32_t *keys, *perm, *lo;
    __device__ __forceinline__ uint64_t at(int i) const {
        return lo ? ((uint64_t)keys[i] << 32) | lo[perm[i]] : (uint64_t)keys[i];
    }
};

// Chunk b = sorted positions [b span, (b + 1) span).  vid[i] = voxel of position i, first[v] = first position
// of voxel v, first[M] = N, hdr[kVoxM] = M.
__global__ __launch_bounds__(kVoxThreads) void voxel_heads_kernel(int N, int span, VoxSorted srt,
                                                                  uint32_t *__restrict__ vid,
                                                                  uint32_t *__restrict__ first,
                                                                  uint32_t *__restrict__ look,
                                                                  uint32_t *__restrict__ hdr) {
    __shared__ uint32_t s_w[kVoxThreads / 64], s_tmp[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int start = (int)min((size_t)N, (size_t)blockIdx.x * span), end = (int)min((size_t)N, (size_t)start + span);
    uint32_t cnt = 0;
    for (int i = start + tid; i < end; i += kVoxThreads) cnt += (i == 0 || srt.at(i) != srt.at(i - 1)) ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) s_w[w] = cnt;
    __syncthreads();
    const uint32_t c = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    uint32_t running = block_prefix(look, blockIdx.x, c, hdr + kVoxErr, s_tmp);  // syncs: s_w is free again
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int t0 = start; t0 < end; t0 += kVoxThreads) {
        const int i = t0 + tid;
        const bool h = i < end && (i == 0 || srt.at(i) != srt.at(i - 1));
        const uint64_t m = __builtin_amdgcn_ballot_w64(h);
        if (lane == 0) s_w[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = running + (uint32_t)__popcll(m & lt_mask);
        for (int q = 0; q < w; q++) before += s_w[q];
        if (i < end) {
            const uint32_t v = before + (h ? 1u : 0u) - 1u;  // position 0 is a head: never underflows
            vid[i] = v;
            if (h) first[v] = (uint32_t)i;
            if (i == N - 1) {
                first[v + 1] = (uint32_t)N;
                hdr[kVoxM] = v + 1;
            }
        }
        running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

template <int CTRL, int RM>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, RM, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, RM, 0xF, false);
    return __hiloint2double(hi, lo);
}
// one step of the wave's segmented inclusive scan (seg_scan_step of preprocess_backward.hip, in fp64)
template <int NV, int CTRL, int RM>
__device__ __forceinline__ void vox_scan_step(double acc[NV], bool &f) {
    const bool fu = __builtin_amdgcn_update_dpp(0, (int)f, CTRL, RM, 0xF, false) != 0;
    double up[NV];
#pragma unroll
    for (int q = 0; q < NV; q++) up[q] = dpp_f64<CTRL, RM>(acc[q]);
    if (!f) {
#pragma unroll
        for (int q = 0; q < NV; q++) acc[q] += up[q];
    }
    f = f || fu;
}

struct VoxOut {
    float *points, *colors;
    int32_t *counts;
    const uint32_t *first;
};
// the epilogue: divide the voxel's sums by its count, round once to fp32
template <int NV>
__device__ __forceinline__ void write_voxel(const VoxOut &o, uint32_t v, const double *acc) {
    const uint32_t n = o.first[v + 1] - o.first[v];
    const double d = (double)n;
#pragma unroll
    for (int q = 0; q < 3; q++) o.points[3 * (size_t)v + q] = (float)(acc[q] / d);
    if (NV == 6) {
#pragma unroll
        for (int q = 0; q < 3; q++) o.colors[3 * (size_t)v + q] = (float)(acc[3 + q] / d);
    }
    if (o.counts) o.counts[v] = (int32_t)n;
}

// part[(2 w + k) NV ..]: k = 0 the piece of wave w that continues a voxel from the wave before, k = 1 the piece
// that starts a voxel and runs on into the next wave; cross[w] = that voxel + 1, or 0 when there is none.
template <int NV>
__global__ __launch_bounds__(kVoxThreads) void voxel_segments_kernel(int N, const uint32_t *__restrict__ perm,
                                                                     const uint32_t *__restrict__ vid,
                                                                     const float *__restrict__ pts,
                                                                     const float *__restrict__ cols, VoxOut o,
                                                                     double *__restrict__ part,
                                                                     uint32_t *__restrict__ cross) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (kVoxThreads / 64) + (threadIdx.x >> 6);
    if ((size_t)w * 64 >= (size_t)N) return;
    const int e = w * 64 + lane;
    const bool valid = e < N;
    const uint32_t v = valid ? vid[e] : 0xFFFFFFFFu;
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; q++) acc[q] = 0.0;
    if (valid) {
        const size_t id = perm[e];
#pragma unroll
        for (int q = 0; q < 3; q++) acc[q] = (double)pts[3 * id + q];
        if (NV == 6) {
#pragma unroll
            for (int q = 0; q < 3; q++) acc[3 + q] = (double)cols[3 * id + q];
        }
    }
    uint32_t vp = __shfl_up(v, 1), vn = __shfl_down(v, 1);
    if (lane == 0) vp = e > 0 ? vid[e - 1] : 0xFFFFFFFFu;
    if (lane == 63) vn = e + 1 < N ? vid[e + 1] : 0xFFFFFFFFu;
    const bool head = valid && v != vp, tail = valid && v != vn;
    bool f = head || lane == 0;
    vox_scan_step<NV, 0x111, 0xF>(acc, f);  // row_shr:1
    vox_scan_step<NV, 0x112, 0xF>(acc, f);  // row_shr:2
    vox_scan_step<NV, 0x114, 0xF>(acc, f);  // row_shr:4
    vox_scan_step<NV, 0x118, 0xF>(acc, f);  // row_shr:8
    vox_scan_step<NV, 0x142, 0xA>(acc, f);  // row_bcast:15 -> rows 1, 3
    vox_scan_step<NV, 0x143, 0xC>(acc, f);  // row_bcast:31 -> rows 2, 3
    const bool ends = valid && (tail || lane == 63);
    const uint64_t endm = __ballot(ends);
    const int fe = __ffsll((unsigned long long)endm) - 1;  // end lane of the first piece
    const bool head0 = __ballot(head) & 1ull;
    const bool starts = lane != fe || head0;  // the piece starts at its voxel's first point
    if (ends) {
        if (starts && tail) write_voxel<NV>(o, v, acc);
        else {
            double *p = part + ((size_t)w * 2 + (starts ? 1 : 0)) * NV;
#pragma unroll
            for (int q = 0; q < NV; q++) p[q] = acc[q];
        }
    }
    const uint32_t cv = __shfl((ends && starts && !tail) ? v + 1u : 0u, 63);
    if (lane == 0) cross[w] = cv;
}

// One wave per wave w of the segments pass; it works when a voxel starts in w and runs on past it.
template <int NV>
__global__ __launch_bounds__(kVoxThreads) void voxel_finish_kernel(int N, const uint32_t *__restrict__ cross,
                                                                   const double *__restrict__ part, VoxOut o) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (kVoxThreads / 64) + (threadIdx.x >> 6);
    if ((size_t)w * 64 >= (size_t)N) return;
    const uint32_t cv = cross[w];
    if (cv == 0) return;
    const uint32_t v = cv - 1;
    const int w1 = (int)((o.first[v + 1] - 1u) >> 6);  // the wave holding the voxel's last point
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; q++) acc[q] = lane == 0 ? part[((size_t)w * 2 + 1) * NV + q] : 0.0;
    for (int k = w + 1 + lane; k <= w1; k += 64) {
#pragma unroll
        for (int q = 0; q < NV; q++) acc[q] += part[((size_t)k * 2) * NV + q];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < NV; q++) acc[q] += __shfl_xor(acc[q], off);
    }
    if (lane == 0) write_voxel<NV>(o, v, acc);
}

int vox_fail(int code, const std::string &what) { return train_fail(code, "voxel_downsample: " + what); }

#define VOX_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return vox_fail(GS4D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int head_span(int N) {  // sorted positions per head-scan chunk: a multiple of the workgroup, at most kVoxMaxChunks chunks
    const size_t per = ((size_t)N + kVoxMaxChunks - 1) / kVoxMaxChunks;
    return (int)align_up(per < 1 ? 1 : per, kVoxThreads);
}

}  // namespace
}  // namespace gs4d

using namespace gs4d;

extern "C" int gs4d_voxel_downsample(int N, const float *points, const float *colors, double voxel_size,
                                     float *out_points, float *out_colors, int32_t *out_counts, int *num_voxels,
                                     gs4d_alloc_fn scratch_alloc, void *scratch_ctx, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!num_voxels) return vox_fail(GS4D_ERR_ARG, "num_voxels is NULL");
    *num_voxels = 0;
    if (N < 0 || N >= (1 << 30)) return vox_fail(GS4D_ERR_ARG, "N must be in [0, 2^30)");
    if (!std::isfinite(voxel_size) || voxel_size <= 0.0)
        return vox_fail(GS4D_ERR_ARG, "voxel_size must be finite and positive");
    if ((colors == nullptr) != (out_colors == nullptr))
        return vox_fail(GS4D_ERR_ARG, "colors and out_colors must both be set or both be NULL");
    if (N == 0) return GS4D_OK;
    if (!points || !out_points || !scratch_alloc) return vox_fail(GS4D_ERR_ARG, "missing buffers");

    // scratch: header | histograms (low word, high word) | head-scan chain | look-back words of up to 8 passes,
    // then the per-point and per-wave arrays
    const size_t n = (size_t)N, nblk = (size_t)sort_nblk(N, kVoxSortThreads * kVoxSortItems), nw = (n + 63) / 64;
    const int span = head_span(N);
    const size_t nchunk = (n + span - 1) / span;
    const size_t chain_words = align_up(nchunk, 64), look_words = 256 * nblk;
    const size_t zero_words = kVoxHeader + 2 * (size_t)kHistWords + chain_words + 8 * look_words;
    const size_t bytes = align_up(4 * zero_words, 256) + 7 * align_up(4 * n, 256) + align_up(4 * (n + 1), 256) +
                         align_up(4 * nw, 256) + align_up(8 * 2 * 6 * nw, 256) + 256;
    char *scratch = scratch_alloc(scratch_ctx, bytes);
    if (!scratch) return vox_fail(GS4D_ERR_ALLOC, "scratch allocation failed");
    char *q = (char *)align_up((size_t)scratch, 256);
    auto take = [&](size_t b) {
        char *r = q;
        q += align_up(b, 256);
        return r;
    };
    uint32_t *hdr = (uint32_t *)take(4 * zero_words);
    uint32_t *hist_lo = hdr + kVoxHeader, *hist_hi = hist_lo + kHistWords, *chain = hist_hi + kHistWords;
    uint32_t *look = chain + chain_words;
    uint32_t *keys[2] = {(uint32_t *)take(4 * n), (uint32_t *)take(4 * n)};
    uint32_t *vals[2] = {(uint32_t *)take(4 * n), (uint32_t *)take(4 * n)};
    uint32_t *lo = (uint32_t *)take(4 * n), *hi = (uint32_t *)take(4 * n), *vid = (uint32_t *)take(4 * n);
    uint32_t *first = (uint32_t *)take(4 * (n + 1));
    uint32_t *cross = (uint32_t *)take(4 * nw);
    double *part = (double *)take(8 * 2 * 6 * nw);

    // ---- bounds, readback 1
    const int nb = (N + kVoxThreads - 1) / kVoxThreads;
    VOX_HIP(hipMemsetAsync(hdr, 0, 4 * kVoxHeader, stream));
    VOX_HIP(hipMemsetD32Async((hipDeviceptr_t)hdr, 0xFFFFFFFFu, 3, stream));
    const int nb4 = (nb + 3) / 4;  // four points per lane
    hipLaunchKernelGGL(voxel_bounds_kernel, dim3(nb4 < 1024 ? nb4 : 1024), dim3(kVoxThreads), 0, stream, N, points, hdr);
    VOX_HIP(hipGetLastError());
    uint32_t hb[6];
    VOX_HIP(hipMemcpyAsync(hb, hdr, sizeof(hb), hipMemcpyDeviceToHost, stream));
    VOX_HIP(hipStreamSynchronize(stream));
    VoxGrid g;
    g.voxel = voxel_size;
    uint64_t dim[3];
    for (int c = 0; c < 3; c++) {
        float mn, mx;
        const uint32_t umn = vox_ord2f(hb[c]), umx = vox_ord2f(hb[3 + c]);
        memcpy(&mn, &umn, 4);
        memcpy(&mx, &umx, 4);
        if (!std::isfinite(mn) || !std::isfinite(mx)) return vox_fail(GS4D_ERR_ARG, "a point coordinate is NaN or infinite");
        g.origin[c] = (double)mn - voxel_size * 0.5;
        const double top = floor(((double)mx - g.origin[c]) / voxel_size);
        if (!(top + 1.0 < (double)kVoxAxisLimit))
            return vox_fail(GS4D_ERR_ARG, "an axis spans 2^21 voxels or more; use a larger voxel_size");
        dim[c] = (uint64_t)top + 1;
    }
    g.nx = dim[0];
    g.ny = dim[1];
    const uint64_t total = dim[0] * dim[1] * dim[2];  // < 2^63
    int nbits = 1;
    while (nbits < 63 && (total - 1) >> nbits) nbits++;
    const bool two_words = nbits > 32;
    const int pass_lo = two_words ? 4 : (nbits + 7) / 8, pass_hi = two_words ? (nbits - 32 + 7) / 8 : 0;

    // ---- keys, sort
    VOX_HIP(hipMemsetAsync(hist_lo, 0, 4 * (2 * (size_t)kHistWords + chain_words + (size_t)(pass_lo + pass_hi) * look_words),
                           stream));
    hipLaunchKernelGGL(voxel_keys_kernel, dim3(nb), dim3(kVoxThreads), 0, stream, N, points, g, keys[0], lo, hi, hist_lo);
    int cur = onesweep_sort<kVoxSortThreads, kVoxSortItems>(keys, vals, N, nullptr, 8 * pass_lo, hist_lo, look,
                                                            hdr + kVoxErr, stream);
    VoxSorted srt{keys[cur], vals[cur], nullptr};
    if (two_words) {
        uint32_t *k2[2] = {keys[cur ^ 1], keys[cur]}, *v2[2] = {vals[cur], vals[cur ^ 1]};
        hipLaunchKernelGGL(voxel_gather_hi_kernel, dim3(nb), dim3(kVoxThreads), 0, stream, N, v2[0], hi, k2[0], hist_hi);
        int c2 = 0;
        for (int p = 0; p < pass_hi; p++) {  // the permutation rides along from pass 0 on, so not onesweep_sort
            hipLaunchKernelGGL((onesweep_kernel<kVoxSortThreads, kVoxSortItems>), dim3((unsigned)nblk), dim3(kVoxSortThreads),
                               0, stream, k2[c2], v2[c2], k2[c2 ^ 1], v2[c2 ^ 1], N, nullptr, 8 * p, hist_hi + 256 * p,
                               look + (size_t)(pass_lo + p) * look_words, hdr + kVoxErr);
            c2 ^= 1;
        }
        srt = VoxSorted{k2[c2], v2[c2], lo};
    }
    VOX_HIP(hipGetLastError());

    // ---- heads, segments, finish, readback 2
    hipLaunchKernelGGL(voxel_heads_kernel, dim3((unsigned)nchunk), dim3(kVoxThreads), 0, stream, N, span, srt, vid, first,
                       chain, hdr);
    const VoxOut o{out_points, out_colors, out_counts, first};
    const dim3 wgrid((unsigned)((nw + 3) / 4));
    if (colors) {
        hipLaunchKernelGGL(voxel_segments_kernel<6>, wgrid, dim3(kVoxThreads), 0, stream, N, srt.perm, vid, points, colors, o,
                           part, cross);
        hipLaunchKernelGGL(voxel_finish_kernel<6>, wgrid, dim3(kVoxThreads), 0, stream, N, cross, part, o);
    } else {
        hipLaunchKernelGGL(voxel_segments_kernel<3>, wgrid, dim3(kVoxThreads), 0, stream, N, srt.perm, vid, points, colors, o,
                           part, cross);
        hipLaunchKernelGGL(voxel_finish_kernel<3>, wgrid, dim3(kVoxThreads), 0, stream, N, cross, part, o);
    }
    VOX_HIP(hipGetLastError());
    uint32_t tail[2];  // error flag, M
    VOX_HIP(hipMemcpyAsync(tail, hdr + kVoxErr, sizeof(tail), hipMemcpyDeviceToHost, stream));
    VOX_HIP(hipStreamSynchronize(stream));
    if (tail[0] != 0) return vox_fail(GS4D_ERR_HIP, "a chunk-prefix wait ran out (device error flag set)");
    *num_voxels = (int)tail[1];
    return GS4D_OK;
}
