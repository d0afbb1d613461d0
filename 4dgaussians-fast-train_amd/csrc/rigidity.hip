// rigidity.hip -- the local-isometry regulariser over a K-NN graph (gs4d_isometry_loss_grad): neighbouring
// Gaussians keep their mutual distances between two position sets xa (canonical) and xb (deformed).
//
//   r(v) = sqrt(v.v + 1e-12),  Delta_e = r(xb_i - xb_j) - r(xa_i - xa_j) for the edge e = (i, k), j = nbr_idx[e]
//   value = scale / E * sum over the valid edges of w_e Delta_e^2,   E = P min(K, P - 1)
//
// No reference counterpart (Dynamic 3D Gaussians' rigidity / isometry terms and SC-GS's ARAP term are the model).
// One lane per node, two launches:
//   node   the node's K out-edges in ascending k, then its in-edges in in_edge order (gs4d_knn_graph's transpose:
//          ascending edge id), each edge's term RECOMPUTED from the four positions rather than read from a
//          per-edge record: a record would cost an edge pass writing 4 floats per edge and the node pass reading
//          them back, against two 12-byte gathers that the record pass makes anyway -- the gathers dominate either
//          way and the recomputation needs no scratch for E records.  An edge's arithmetic is fp32 (differences,
//          correctly rounded sqrt and division, as torch's fp32 formulation); a node's three sums per side and its
//          share of the value are accumulated in fp64 in that fixed order and rounded once.  A node of in-degree n
//          is one lane looping n times, four edges' loads at a time (the wave waits for its longest lane).  The
//          value: lanes by the wave's xor tree, the waves in order, one fp64 partial per workgroup.
//   total  one workgroup adds the partials in fp64: thread t the partials t, t + 256, ... in ascending order, the
//          xor tree, the waves in order; times scale / E, rounded once.
// No atomics: the order of every sum is a function of the graph alone, so two calls give the same bits.
#include <cfloat>

#include "../../include/gs4d.h"
#include "../../include/gs4d_train.h"
#include "train_internal.h"

namespace gs4d {
namespace {

constexpr int kIsoThreads = 256;
constexpr int kIsoBatch = 4;  // in-edges whose loads are in flight together

struct IsoEdge {
    float g;         // w Delta
    float ub[3], ua[3];  // (xb_i - xb_j) / r_b, (xa_i - xa_j) / r_a
};

__device__ __forceinline__ void iso_load3(const float *__restrict__ x, int i, float v[3]) {
    v[0] = x[3 * (size_t)i];
    v[1] = x[3 * (size_t)i + 1];
    v[2] = x[3 * (size_t)i + 2];
}

// the term of the edge from `i` to `j` (positions given): Delta, and the unit directions at the edge's source
__device__ __forceinline__ float iso_edge(const float ai[3], const float aj[3], const float bi[3], const float bj[3],
                                          float w, IsoEdge &e) {
    const float da[3] = {ai[0] - aj[0], ai[1] - aj[1], ai[2] - aj[2]};
    const float db[3] = {bi[0] - bj[0], bi[1] - bj[1], bi[2] - bj[2]};
    const float ra = sqrtf(((da[0] * da[0] + da[1] * da[1]) + da[2] * da[2]) + 1e-12f);
    const float rb = sqrtf(((db[0] * db[0] + db[1] * db[1]) + db[2] * db[2]) + 1e-12f);
    const float delta = rb - ra;
    e.g = w * delta;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        e.ub[c] = db[c] / rb;
        e.ua[c] = da[c] / ra;
    }
    return e.g * delta;  // w Delta^2
}

__global__ __launch_bounds__(kIsoThreads) void isometry_node_kernel(int P, int K, const int32_t *__restrict__ nbr_idx,
                                                                    const int32_t *__restrict__ in_start,
                                                                    const int32_t *__restrict__ in_edge,
                                                                    const float *__restrict__ weights,
                                                                    const float *__restrict__ xa,
                                                                    const float *__restrict__ xb, double coef,
                                                                    float *__restrict__ dxa, float *__restrict__ dxb,
                                                                    double *__restrict__ part) {
    const int i = blockIdx.x * kIsoThreads + threadIdx.x;
    double val = 0.0, ga[3] = {0.0, 0.0, 0.0}, gb[3] = {0.0, 0.0, 0.0};
    if (i < P) {
        const int slots = P * K;
        float ai[3], bi[3];
        iso_load3(xa, i, ai);
        iso_load3(xb, i, bi);
        for (int k = 0; k < K; k++) {
            const int e = i * K + k, j = nbr_idx[e];
            if (j < 0 || j >= P) continue;  // an empty slot (or a foreign graph's index: never read out of bounds)
            float aj[3], bj[3];
            iso_load3(xa, j, aj);
            iso_load3(xb, j, bj);
            IsoEdge t;
            val += (double)iso_edge(ai, aj, bi, bj, weights ? weights[e] : 1.f, t);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                gb[c] += (double)(t.g * t.ub[c]);
                ga[c] -= (double)(t.g * t.ua[c]);
            }
        }
        const int q0 = min(max(in_start[i], 0), slots), q1 = min(max(in_start[i + 1], q0), slots);
        // The in-edges in batches of kIsoBatch: the batch's edge ids, then its gathers, are issued together; the
        // terms are then added one by one in in_edge order, so the sums do not depend on the batching (measured at
        // an in-degree of 3000: 1.59 -> 1.41 ms).
        for (int qb = q0; qb < q1; qb += kIsoBatch) {
            int e[kIsoBatch];
            float am[kIsoBatch][3], bm[kIsoBatch][3], w[kIsoBatch];
#pragma unroll
            for (int b = 0; b < kIsoBatch; b++) e[b] = qb + b < q1 ? in_edge[qb + b] : -1;
#pragma unroll
            for (int b = 0; b < kIsoBatch; b++) {
                if (e[b] < 0 || e[b] >= slots) e[b] = -1;
                const int es = max(e[b], 0), m = es / K;  // the edge's source; this node is its target
                iso_load3(xa, m, am[b]);
                iso_load3(xb, m, bm[b]);
                w[b] = weights ? weights[es] : 1.f;
            }
#pragma unroll
            for (int b = 0; b < kIsoBatch; b++) {
                if (e[b] < 0) continue;
                IsoEdge t;
                (void)iso_edge(am[b], ai, bm[b], bi, w[b], t);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    gb[c] -= (double)(t.g * t.ub[c]);
                    ga[c] += (double)(t.g * t.ua[c]);
                }
            }
        }
        const double c2 = 2.0 * coef;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (dxa) dxa[3 * (size_t)i + c] = (float)(c2 * ga[c]);
            if (dxb) dxb[3 * (size_t)i + c] = (float)(c2 * gb[c]);
        }
    }
    __shared__ double s_w[kIsoThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) val += __shfl_xor(val, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = val;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kIsoThreads / 64; w++) s += s_w[w];
        part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kIsoThreads) void isometry_total_kernel(int nblk, const double *__restrict__ part, double coef,
                                                                     float *__restrict__ value) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kIsoThreads) s += part[b];
    __shared__ double s_w[kIsoThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kIsoThreads / 64; w++) t += s_w[w];
        *value = (float)(coef * t);
    }
}

int iso_fail(int code, const std::string &what) { return train_fail(code, "isometry: " + what); }

}  // namespace
}  // namespace gs4d

using namespace gs4d;

extern "C" int gs4d_isometry_loss_grad(int P, int K, const int32_t *nbr_idx, const int32_t *in_start,
                                       const int32_t *in_edge, const float *weights, const float *xa, const float *xb,
                                       float scale, float *value, float *dL_dxa, float *dL_dxb,
                                       gs4d_alloc_fn scratch_alloc, void *scratch_ctx, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 1 || K > 16) return iso_fail(GS4D_ERR_ARG, "K must be in 1..16");
    if (P < 0 || (size_t)P * K >= ((size_t)1 << 30)) return iso_fail(GS4D_ERR_ARG, "P must be >= 0 and P K below 2^30");
    if (P == 0) return GS4D_OK;
    if (!nbr_idx || !in_start || !in_edge || !xa || !xb || !value) return iso_fail(GS4D_ERR_ARG, "missing buffers");
    if (!scratch_alloc) return iso_fail(GS4D_ERR_ARG, "missing the scratch allocator");
    const int nblk = (P + kIsoThreads - 1) / kIsoThreads;
    char *scratch = scratch_alloc(scratch_ctx, sizeof(double) * (size_t)nblk + 256);
    if (!scratch) return iso_fail(GS4D_ERR_ALLOC, "scratch allocation failed");
    double *part = (double *)align_up((size_t)scratch, 256);
    const int E = P * (K < P - 1 ? K : P - 1);
    const double coef = E > 0 ? (double)scale / (double)E : 0.0;
    hipLaunchKernelGGL(isometry_node_kernel, dim3(nblk), dim3(kIsoThreads), 0, stream, P, K, nbr_idx, in_start, in_edge,
                       weights, xa, xb, coef, dL_dxa, dL_dxb, part);
    hipLaunchKernelGGL(isometry_total_kernel, dim3(1), dim3(kIsoThreads), 0, stream, nblk, part, coef, value);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return iso_fail(GS4D_ERR_HIP, hipGetErrorString(e));
    return GS4D_OK;
}
