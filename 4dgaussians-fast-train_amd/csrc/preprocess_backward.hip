// preprocess_backward.hip -- per-Gaussian backward: instance-gradient reduction, then
// computeCov2DCUDA (K8) + preprocessCUDA backward (K9) fused into one pass.
//
// Reference: cuda_rasterizer/backward.cu:144-274 (computeCov2DCUDA), :346-396 (preprocessCUDA),
// :20-139 (SH backward), :278-341 (cov3D backward); rasterize_points.cu:153-161 (zeroed outputs).
//
// 1. contrib_reduce: each Gaussian sums the per-(tile, Gaussian) records the render backward stored
//    at its emission slots -- consecutive, in tile-rect order -- with a fixed-order segmented
//    reduction, which replaces the reference's float atomics (backward.cu:523,545-554): bitwise
//    deterministic, and balanced (one lane per record, whatever the splat sizes).
// 2. gaussian_backward: the sums of the Gaussians whose records span waves, then K8 + K9 per
//    Gaussian except K9's SH part, which sh_backward runs after it with the block's coefficient
//    rows staged through LDS (coalesced loads and stores).  Every output element is written (zeros for culled Gaussians and for
//    SH coefficients >= (D+1)^2), so no zero-fill pass is needed.
#include <algorithm>

#include "gs4d_internal.h"

namespace gs4d {

// Render-level gradients of Gaussian g from its summed moments R (render.hip): backward.cu:545-554
// with dL/dG = opacity dL/dalpha, ddelx_dx = W/2, ddely_dy = H/2.  Returned as dL_dmeans2D (.z stays
// 0), dL_dcolors, dL_dopacity; the conic gradient uses the reference's float4 slots .x .y .w
// (backward.cu:549-551, read at :165).
struct GradOut {
    float *mean2D;
    float4 *conic;
    float *opacity;
    float *color;
    const float4 *conic_opacity;
    float hw, hh;
    float *abs_mean2D;  // (P, 3), the absgrad backward only (NULL otherwise)
};
// NV = 10 (the depth-gradient backward): R[9] = W3, the sum of w dL/ddepth, parked in the conic gradient's
// unused .z slot until gaussian_grads turns it into dL/dmean3D and clears the slot.
// ABS (the absgrad backward): R[NV], R[NV + 1] = the records' floats 10 and 11, the sums over the Gaussian's pixels
// of |u| |d power2 / d mean| (render.hip, base-2 exponent: ln 2 brings them to the reference's power), which
// become abs_mean2D in dL_dmeans2D's units.  NA = the number of values carried: NV + 2 with ABS.
constexpr float kLn2 = 0.6931471805599453f;
template <int NV, bool ABS>
constexpr int n_acc() { return NV + (ABS ? 2 : 0); }
template <int NV, bool ABS>
__device__ __forceinline__ void write_grads(const GradOut &o, uint32_t g, const float *R) {
    const float4 co = o.conic_opacity[g];
    const float op = co.w;
    o.mean2D[3 * g + 0] = o.hw * op * (-co.x * R[1] - co.y * R[2]);
    o.mean2D[3 * g + 1] = o.hh * op * (-co.z * R[2] - co.y * R[1]);
    o.mean2D[3 * g + 2] = 0.f;
    o.conic[g] = make_float4(-0.5f * op * R[3], -0.5f * op * R[4], NV == 10 ? R[9] : 0.f, -0.5f * op * R[5]);
    o.opacity[g] = R[0];
    o.color[3 * g + 0] = R[6];
    o.color[3 * g + 1] = R[7];
    o.color[3 * g + 2] = R[8];
    if (ABS) {
        o.abs_mean2D[3 * g + 0] = o.hw * op * (kLn2 * R[NV]);
        o.abs_mean2D[3 * g + 1] = o.hh * op * (kLn2 * R[NV + 1]);
        o.abs_mean2D[3 * g + 2] = 0.f;
    }
}
__device__ __forceinline__ void write_zero_abs(const GradOut &o, uint32_t g) {
    o.abs_mean2D[3 * g + 0] = 0.f;
    o.abs_mean2D[3 * g + 1] = 0.f;
    o.abs_mean2D[3 * g + 2] = 0.f;
}
__device__ __forceinline__ void write_zero_grads(const GradOut &o, uint32_t g) {
    o.mean2D[3 * g + 0] = 0.f;
    o.mean2D[3 * g + 1] = 0.f;
    o.mean2D[3 * g + 2] = 0.f;
    o.conic[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    o.opacity[g] = 0.f;
    o.color[3 * g + 0] = 0.f;
    o.color[3 * g + 1] = 0.f;
    o.color[3 * g + 2] = 0.f;
}
template <int NV, bool ABS>
__device__ __forceinline__ void store9(float4 *p, const float *acc) {
    p[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    p[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    p[2] = make_float4(acc[8], NV == 10 ? acc[9] : 0.f, ABS ? acc[NV] : 0.f, ABS ? acc[NV + 1] : 0.f);
}
template <int NV, bool ABS>
__device__ __forceinline__ void add9(float *acc, const float4 *p) {
    const float4 a = p[0], b = p[1], c = p[2];
    acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
    acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    acc[8] += c.x;
    if (NV == 10) acc[9] += c.y;
    if (ABS) {
        acc[NV] += c.z;
        acc[NV + 1] += c.w;
    }
}

// One step of the wave's segmented inclusive scan by DPP moves (no LDS): lane l takes the (sums, flag) of
// the lane CTRL names (row_shr:n inside rows of 16, row_bcast:15 / :31 across rows, only the rows RM
// enables; lanes without a source read zeros, the identity) and adds its sums unless a segment head
// lies between them.
template <int CTRL, int RM, int NV>
__device__ __forceinline__ void seg_scan_step(float (&acc)[NV], bool &f) {
    const bool fu = __builtin_amdgcn_update_dpp(0, (int)f, CTRL, RM, 0xF, false) != 0;
    float up[NV];
#pragma unroll
    for (int q = 0; q < NV; q++)
        up[q] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[q]), CTRL, RM, 0xF, false));
    if (!f) {
#pragma unroll
        for (int q = 0; q < NV; q++) acc[q] += up[q];
    }
    f = f || fu;
}

// Pass 1: one lane per emission slot, one wave per 64 slots.  A Gaussian's records occupy consecutive
// slots, so a segmented inclusive scan (fixed shuffle tree) sums each Gaussian's piece of the wave.
// Pieces that are a whole Gaussian are written out; a piece continuing from the previous wave goes
// to part[w][0], a piece that starts a Gaussian and continues into the next wave to part[w][1];
// e_first[g] = the Gaussian's first slot.  NV = 10 also sums the records' float 9 (W3), ABS their floats 10 and 11
// (the absolute sums), in the same order: 9, 10, 11 or 12 values ride the scan.
template <int NV, bool ABS>
__global__ __launch_bounds__(256) void contrib_segments_kernel(const uint32_t *__restrict__ n_dev,
                                                               const uint32_t *__restrict__ gid_by_e,
                                                               const float4 *__restrict__ rec, GradOut o,
                                                               float4 *__restrict__ part,
                                                               uint32_t *__restrict__ e_first) {
    const int n = (int)__builtin_amdgcn_readfirstlane(*n_dev);
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w * 64 >= n) return;
    const int e = w * 64 + lane;
    const bool valid = e < n;
    const uint32_t key = valid ? gid_by_e[e] & kGidMask : 0xFFFFFFFFu;
    constexpr int NA = n_acc<NV, ABS>();
    float acc[NA];
    {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
        if (valid) {
            a = rec[3 * (size_t)e];
            b = rec[3 * (size_t)e + 1];
            c = rec[3 * (size_t)e + 2];
        }
        acc[0] = a.x; acc[1] = a.y; acc[2] = a.z; acc[3] = a.w;
        acc[4] = b.x; acc[5] = b.y; acc[6] = b.z; acc[7] = b.w;
        acc[8] = c.x;
        if (NV == 10) acc[9] = c.y;
        if (ABS) {
            acc[NV] = c.z;
            acc[NV + 1] = c.w;
        }
    }
    uint32_t kp = __shfl_up(key, 1), kn = __shfl_down(key, 1);
    if (lane == 0) kp = e > 0 ? gid_by_e[e - 1] & kGidMask : 0xFFFFFFFFu;
    if (lane == 63) kn = e + 1 < n ? gid_by_e[e + 1] & kGidMask : 0xFFFFFFFFu;
    const bool head = valid && key != kp;  // first slot of its Gaussian
    const bool tail = valid && key != kn;  // last slot of its Gaussian
    if (head) e_first[key] = (uint32_t)e;  // locates the pieces of a Gaussian spanning waves
    bool f = head || lane == 0;
    seg_scan_step<0x111, 0xF>(acc, f);  // row_shr:1
    seg_scan_step<0x112, 0xF>(acc, f);  // row_shr:2
    seg_scan_step<0x114, 0xF>(acc, f);  // row_shr:4
    seg_scan_step<0x118, 0xF>(acc, f);  // row_shr:8
    seg_scan_step<0x142, 0xA>(acc, f);  // row_bcast:15 -> rows 1, 3
    seg_scan_step<0x143, 0xC>(acc, f);  // row_bcast:31 -> rows 2, 3
    const uint64_t endm = __ballot(valid && (tail || lane == 63));
    const int fe = __ffsll((unsigned long long)endm) - 1;  // end lane of the first piece
    const bool head0 = __ballot(head) & 1ull;
    if (valid && (tail || lane == 63)) {
        const bool starts = lane != fe || head0;  // the piece starts at its Gaussian's first slot
        if (starts && tail) write_grads<NV, ABS>(o, key, acc);
        else if (!starts) store9<NV, ABS>(part + ((size_t)w * 2) * 3, acc);
        else store9<NV, ABS>(part + ((size_t)w * 2 + 1) * 3, acc);
    }
}

// Pass 2 (at the start of gaussian_backward, one thread per Gaussian): a Gaussian whose slots span
// several waves sums its pieces in wave order -- part[w0][1] (its head piece) then part[w][0] of each
// following wave up to the one holding its last slot -- and a Gaussian without instances gets zeros.
// Then K8 + K9 without the SH part: dL/dcov3D, dL/dscale, dL/drot stored; dL/dmean3D's covariance +
// projection terms returned (the caller adds the SH term, backward.cu:390, and stores it).
// NV = 10: dL/dmean3D also takes W3 d(p_view.z)/dmean, the view matrix's depth row (forward.cu:250's
// p_view.z = m[2] x + m[6] y + m[10] z + m[14]); culled Gaussians (radii 0) get nothing.
// ABS: abs_mean2D of a Gaussian spanning waves comes from the same sum; zeros without instances or with radii 0.
// AA (the antialiased backward; `opacities` = the raw o): the dL_dopacity the reduction left is g = dL/do_eff
// (conic_opacity.w holds o_eff).  cov2D_backward takes dL/ds = g o into the covariance and returns s, and the
// stored dL_dopacity becomes dL/do = g s; a Gaussian with radii 0 has no instances and keeps its zero.
// CAM (the camera-gradient backward): cam[0..23] receive this Gaussian's terms of dL/dviewmatrix (columns 0..2:
// cam[3 i + j] = p_h[i] dL/dt[j], plus the rotation's share of T = J Rv in rows 0..2) and of dL/dprojmatrix
// (columns 0, 1, 3: cam[12 + 3 i + jj] = p_h[i] dL/dp_hom[j]), p_h = (mean, 1); zeros for a Gaussian with radii 0
// or without instances.  dL/dt carries the clamp's zeros, W3 (NV = 10) and, with AA, the factor's share.
constexpr int kCamValues = 27;  // 12 + 12 + the 3 of dL/dcampos (the SH kernel's)
template <int NV, bool ABS, bool AA, bool CAM = false>
__device__ __forceinline__ V3 gaussian_grads(
    int idx, const Args &a, const GeomState &g, const int *__restrict__ radii, const float *__restrict__ means3D,
    const float *__restrict__ scales, const float *__restrict__ rotations, const float *__restrict__ cov3Ds,
    const float *dL_dmean2D, const float4 *dL_dconic, float *__restrict__ dL_dcov3D, float *__restrict__ dL_dscale,
    float *__restrict__ dL_drot, const uint32_t *__restrict__ e_first, const float4 *__restrict__ part,
    const GradOut &o, const float *__restrict__ opacities, float *cam = nullptr) {
    {
        const uint32_t ni = g.n_inst[idx];
        if (ni == 0) {
            write_zero_grads(o, (uint32_t)idx);
            if (ABS) write_zero_abs(o, (uint32_t)idx);
        } else {
            const uint32_t e0 = e_first[idx], w0 = e0 >> 6, w1 = (e0 + ni - 1) >> 6;
            if (w0 != w1) {
                float acc[n_acc<NV, ABS>()] = {};
                add9<NV, ABS>(acc, part + ((size_t)w0 * 2 + 1) * 3);
                for (uint32_t w = w0 + 1; w <= w1; w++) add9<NV, ABS>(acc, part + ((size_t)w * 2) * 3);
                write_grads<NV, ABS>(o, (uint32_t)idx, acc);
            }
            if (ABS && radii[idx] <= 0) write_zero_abs(o, (uint32_t)idx);  // this thread wrote it, or pass 1 did
        }
    }
    float dcov[6] = {0, 0, 0, 0, 0, 0};
    V3 dmean = v3(0, 0, 0);
    V3 dscale = v3(0, 0, 0);
    float4 drot = make_float4(0, 0, 0, 0);
    if (radii[idx] > 0) {
        const Mat4 view = load_mat4(a.viewmatrix, a.view_transposed), projm = load_mat4(a.projmatrix);
        const V3 m = v3(means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]);
        float cov3D[6];
#pragma unroll
        for (int i = 0; i < 6; i++) cov3D[i] = cov3Ds[6 * (size_t)idx + i];
        const float4 dc = dL_dconic[idx];
        // K8 (backward.cu:144-274): the covariance part of dL/dmean (assigned, :273)
        float cb[CAM ? kCov2DCamValues : 1];
        if (AA) {
            const float gop = o.opacity[idx];  // pass 1 or this thread wrote it
            float s;
            dmean = cov2D_backward<true, CAM>(m, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, cov3D, view,
                                              make_float3(dc.x, dc.y, dc.w), dcov, gop * opacities[idx], &s, cb);
            o.opacity[idx] = gop * s;
        } else {
            dmean = cov2D_backward<false, CAM>(m, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, cov3D, view,
                                               make_float3(dc.x, dc.y, dc.w), dcov, 0.f, nullptr, cb);
        }
        // K9 (backward.cu:370-387): projection part
        const float *proj = projm.m;
        const float g2x = dL_dmean2D[3 * idx], g2y = dL_dmean2D[3 * idx + 1];
        float4 m_hom = transformPoint4x4(m, projm);
        float m_w = 1.0f / (m_hom.w + 0.0000001f);
        float mul1 = (proj[0] * m.x + proj[4] * m.y + proj[8] * m.z + proj[12]) * m_w * m_w;
        float mul2 = (proj[1] * m.x + proj[5] * m.y + proj[9] * m.z + proj[13]) * m_w * m_w;
        V3 dm2;
        dm2.x = (proj[0] * m_w - proj[3] * mul1) * g2x + (proj[1] * m_w - proj[3] * mul2) * g2y;
        dm2.y = (proj[4] * m_w - proj[7] * mul1) * g2x + (proj[5] * m_w - proj[7] * mul2) * g2y;
        dm2.z = (proj[8] * m_w - proj[11] * mul1) * g2x + (proj[9] * m_w - proj[11] * mul2) * g2y;
        dmean = dmean + dm2;
        if (NV == 10) {  // depth part: W3 times the depth row of the view matrix
            const float w3 = dc.z;
            dmean = dmean + v3(view.m[2] * w3, view.m[6] * w3, view.m[10] * w3);
        }
        if (CAM && g.n_inst[idx] != 0) {
            const float ph[4] = {m.x, m.y, m.z, 1.f};
            const float dt[3] = {cb[0], cb[1], NV == 10 ? cb[2] + dc.z : cb[2]};
            // dL/dp_hom of mean2D = p_hom.xy * m_w (column 2, the unused NDC depth, gets nothing)
            const float dp[3] = {m_w * g2x, m_w * g2y, -(m_hom.x * g2x + m_hom.y * g2y) * m_w * m_w};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    cam[3 * i + j] = ph[i] * dt[j];
                    cam[12 + 3 * i + j] = ph[i] * dp[j];
                }
            // T = J Rv, Rv[b][k] = V[k][b]: dL/dV[k][b] += sum_a dL/dT[a][k] J[a][b]
#pragma unroll
            for (int k = 0; k < 3; k++) {
                cam[3 * k + 0] += cb[3 + k] * cb[9];
                cam[3 * k + 1] += cb[6 + k] * cb[10];
                cam[3 * k + 2] += cb[3 + k] * cb[11] + cb[6 + k] * cb[12];
            }
        }
        // SH part (backward.cu:390-391): added by the caller
        // cov3D part (backward.cu:394-395)
        if (scales) {
            V3 sc = v3(scales[3 * idx], scales[3 * idx + 1], scales[3 * idx + 2]);
            float4 rot = reinterpret_cast<const float4 *>(rotations)[idx];
            cov3D_backward(sc, a.scale_modifier, rot, dcov, dscale, drot);
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) dL_dcov3D[6 * (size_t)idx + i] = dcov[i];
    dL_dscale[3 * idx + 0] = dscale.x;
    dL_dscale[3 * idx + 1] = dscale.y;
    dL_dscale[3 * idx + 2] = dscale.z;
    reinterpret_cast<float4 *>(dL_drot)[idx] = drot;
    if (NV == 10) reinterpret_cast<float *>(const_cast<float4 *>(dL_dconic) + idx)[2] = 0.f;  // W3's slot: back to 0
    return dmean;
}

// The antialiased instantiations of the two kernels below take one more argument, the raw opacities, as a
// trailing pack of one; the empty pack leaves the other instantiations' argument lists, and so their code
// objects, what they were.
__device__ __forceinline__ const float *raw_opacities() { return nullptr; }
__device__ __forceinline__ const float *raw_opacities(const float *p) { return p; }
// The camera-gradient instantiations take, last in the same pack, the partial rows they write: one row of
// kCamRow floats per workgroup (camera_grad.hip sums them).  The pack is then (CamRows) or (raw opacities, CamRows).
__device__ __forceinline__ const float *raw_opacities(CamRows) { return nullptr; }
__device__ __forceinline__ const float *raw_opacities(const float *p, CamRows) { return p; }
__device__ __forceinline__ float *cam_rows() { return nullptr; }
__device__ __forceinline__ float *cam_rows(const float *) { return nullptr; }
__device__ __forceinline__ float *cam_rows(CamRows c) { return c.rows; }
__device__ __forceinline__ float *cam_rows(const float *, CamRows c) { return c.rows; }
template <class... Raw>
constexpr bool kPackAA = (std::is_same<Raw, const float *>::value || ...);
template <class... Raw>
constexpr bool kPackCam = (std::is_same<Raw, CamRows>::value || ...);

// The workgroup's sum of each of the kCamValues per-thread values, in a fixed order: inside a wave the scan's DPP
// moves without the segment flags (row_shr 1, 2, 4, 8, then row_bcast 15 and 31: lane 63 ends with the wave's
// sum), then the waves' sums in wave order through LDS (consecutive floats: no bank conflict).  Thread q <
// kCamValues stores value q of the workgroup's row.  Every thread of the workgroup must call it.
template <int CTRL, int RM>
__device__ __forceinline__ void cam_sum_step(float (&v)[kCamValues]) {
#pragma unroll
    for (int q = 0; q < kCamValues; q++)
        v[q] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[q]), CTRL, RM, 0xF, false));
}
template <int WAVES>
__device__ __forceinline__ void cam_block_sum(float (&v)[kCamValues], float *__restrict__ row) {
    __shared__ float sums[WAVES * kCamValues];
    cam_sum_step<0x111, 0xF>(v);  // row_shr:1
    cam_sum_step<0x112, 0xF>(v);  // row_shr:2
    cam_sum_step<0x114, 0xF>(v);  // row_shr:4
    cam_sum_step<0x118, 0xF>(v);  // row_shr:8
    cam_sum_step<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
    cam_sum_step<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int q = 0; q < kCamValues; q++) sums[(threadIdx.x >> 6) * kCamValues + q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < kCamValues) {
        float s = sums[threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; w++) s += sums[w * kCamValues + threadIdx.x];
        row[threadIdx.x] = s;
    }
}

// Without SH coefficients (colours precomputed): one thread per Gaussian, dL/dmean3D = the two terms.
template <int NV, bool ABS, class... Raw>
__global__ __launch_bounds__(256) void gaussian_backward_kernel(
    Args a, GeomState g, const int *__restrict__ radii, const float *__restrict__ means3D,
    const float *__restrict__ scales, const float *__restrict__ rotations, const float *__restrict__ cov3Ds,
    const float *dL_dmean2D, const float4 *dL_dconic, float *__restrict__ dL_dmean3D,
    float *__restrict__ dL_dcov3D, float *__restrict__ dL_dscale, float *__restrict__ dL_drot,
    const uint32_t *__restrict__ e_first, const float4 *__restrict__ part, GradOut o,
    Raw... raw) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (kPackCam<Raw...>) {  // no early exit: the whole workgroup sums (threads past P add zeros)
        float cam[kCamValues] = {};
        if (idx < a.P) {
            const V3 dmean = gaussian_grads<NV, ABS, kPackAA<Raw...>, true>(
                idx, a, g, radii, means3D, scales, rotations, cov3Ds, dL_dmean2D, dL_dconic, dL_dcov3D, dL_dscale,
                dL_drot, e_first, part, o, raw_opacities(raw...), cam);
            dL_dmean3D[3 * idx + 0] = dmean.x;
            dL_dmean3D[3 * idx + 1] = dmean.y;
            dL_dmean3D[3 * idx + 2] = dmean.z;
        }
        cam_block_sum<4>(cam, cam_rows(raw...) + (size_t)blockIdx.x * kCamRow);
    } else {
        if (idx >= a.P) return;
        const V3 dmean = gaussian_grads<NV, ABS, kPackAA<Raw...>>(idx, a, g, radii, means3D, scales, rotations, cov3Ds, dL_dmean2D, dL_dconic,
                                        dL_dcov3D, dL_dscale, dL_drot, e_first, part, o, raw_opacities(raw...));
        dL_dmean3D[3 * idx + 0] = dmean.x;
        dL_dmean3D[3 * idx + 1] = dmean.y;
        dL_dmean3D[3 * idx + 2] = dmean.z;
    }
}

// With SH coefficients: the same per-Gaussian work and K9's SH part (backward.cu:390-391 -> computeColorFromSH
// backward, :20-139) in one launch, one thread per Gaussian.  The block's coefficient rows are staged through
// LDS: the block reads its 128 rows of 3M floats (one contiguous span, float4 when M = 16 and aligned) into a
// 49-float-stride tile (odd stride: a wave's rows hit distinct banks), each thread takes its row into
// registers, writes its gradients back into the same row (zeros past (D + 1)^2 and for culled Gaussians), and
// the block stores the tile as one contiguous span.  dL/dmean3D = (covariance + projection terms) + the
// view-direction term, the reference's order (:390).  A thread per Gaussian straight from global memory
// (192-byte strided rows) took 12.6 us of the old gaussian_backward's 26 at P = 100k; two launches (this
// work split at the SH part) cost one launch more.
constexpr int kShThreads = 128, kShRow = 49;

template <bool kVec4, int NV, bool ABS, class... Raw>
__global__ __launch_bounds__(kShThreads) void gaussian_sh_backward_kernel(
    Args a, GeomState g, const int *__restrict__ radii, const float *__restrict__ means3D,
    const float *__restrict__ scales, const float *__restrict__ rotations, const float *__restrict__ cov3Ds,
    const float *dL_dmean2D, const float4 *dL_dconic, float *__restrict__ dL_dmean3D,
    float *__restrict__ dL_dcov3D, float *__restrict__ dL_dscale, float *__restrict__ dL_drot,
    const uint32_t *__restrict__ e_first, const float4 *__restrict__ part, GradOut o, const float *__restrict__ shs,
    const uint8_t *__restrict__ clamped, const float *dL_dcolor, float *__restrict__ dL_dsh,
    Raw... raw) {
    __shared__ float tile[kShThreads * kShRow];
    const int g0 = blockIdx.x * kShThreads;
    // rows of M > 16 coefficients: only the first 16 can be used (D <= 3); the rest get zeros
    const int n = min(kShThreads, a.P - g0), row = 3 * a.M, rowl = min(row, 48);
    const size_t base = (size_t)g0 * row;
    const int total = n * row;
    if (kVec4) {  // row = 48 = 12 float4
        const float4 *s4 = reinterpret_cast<const float4 *>(shs + base);
        for (int i = threadIdx.x; i < total / 4; i += kShThreads) {
            const int r = i / 12, c = (i - r * 12) * 4;
            const float4 v = s4[i];
            float *t = tile + r * kShRow + c;
            t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
        }
    } else {
        for (int i = threadIdx.x; i < total; i += kShThreads) {
            const int r = i / row, c = i - r * row;
            if (c < 48) tile[r * kShRow + c] = shs[base + i];
        }
    }
    V3 dmean = v3(0, 0, 0);
    const int idx = g0 + threadIdx.x;
    constexpr bool CAM = kPackCam<Raw...>;
    float cam[CAM ? kCamValues : 1] = {};
    if ((int)threadIdx.x < n)  // pass 2 writes this Gaussian's dL/dcolor (when it spans waves) before it is read
        dmean = gaussian_grads<NV, ABS, kPackAA<Raw...>, CAM>(idx, a, g, radii, means3D, scales, rotations, cov3Ds, dL_dmean2D,
                                                              dL_dconic, dL_dcov3D, dL_dscale, dL_drot, e_first, part, o,
                                                              raw_opacities(raw...), cam);
    __syncthreads();
    if ((int)threadIdx.x < n) {
        float *trow = tile + threadIdx.x * kShRow;
        float shl[48];
#pragma unroll
        for (int k = 0; k < 48; k++) {
            shl[k] = k < rowl ? trow[k] : 0.f;
            if (k < rowl) trow[k] = 0.f;
        }
        if (radii[idx] > 0) {
            const uint8_t cl = clamped[idx];
            const V3 dRGB = v3(dL_dcolor[3 * idx] * ((cl & 1) ? 0.f : 1.f),
                               dL_dcolor[3 * idx + 1] * ((cl & 2) ? 0.f : 1.f),
                               dL_dcolor[3 * idx + 2] * ((cl & 4) ? 0.f : 1.f));
            const V3 m = v3(means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]);
            const V3 dm = sh_backward(a.D, shl, m - load_v3(a.campos), dRGB, trow);
            dmean = dmean + dm;
            if constexpr (CAM) {  // dir = mean - campos: the centre gets the opposite of the direction's gradient
                cam[24] = -dm.x;
                cam[25] = -dm.y;
                cam[26] = -dm.z;
            }
        }
        dL_dmean3D[3 * idx + 0] = dmean.x;
        dL_dmean3D[3 * idx + 1] = dmean.y;
        dL_dmean3D[3 * idx + 2] = dmean.z;
    }
    if constexpr (CAM) cam_block_sum<kShThreads / 64>(cam, cam_rows(raw...) + (size_t)blockIdx.x * kCamRow);
    __syncthreads();
    if (kVec4) {
        float4 *d4 = reinterpret_cast<float4 *>(dL_dsh + base);
        for (int i = threadIdx.x; i < total / 4; i += kShThreads) {
            const int r = i / 12, c = (i - r * 12) * 4;
            const float *t = tile + r * kShRow + c;
            d4[i] = make_float4(t[0], t[1], t[2], t[3]);
        }
    } else {
        for (int i = threadIdx.x; i < total; i += kShThreads) {
            const int r = i / row, c = i - r * row;
            dL_dsh[base + i] = c < 48 ? tile[r * kShRow + c] : 0.f;
        }
    }
}

// camera: room for the camera-gradient backward's partial rows, one per workgroup of the per-Gaussian kernel with
// the smaller workgroup, after e_first
static size_t cam_rows_max(int P) { return ((size_t)P + kShThreads - 1) / kShThreads; }
size_t contrib_scratch_bytes(int R, int P, bool camera) {
    const size_t nw = ((size_t)R + 63) / 64;
    return align_up(nw * 2 * 3 * sizeof(float4), 256) + align_up(4 * (size_t)P, 256) + 256 +
           (camera ? align_up(cam_rows_max(P) * kCamRow * sizeof(float), 256) : 0);
}

static GradOut grad_out(const Args &a, GeomState g, float *dL_dmean2D, float4 *dL_dconic, float *dL_dopacity,
                        float *dL_dcolor, float *abs_dmean2D) {
    return GradOut{dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, g.conic_opacity, 0.5f * a.W, 0.5f * a.H, abs_dmean2D};
}
static float4 *scratch_part(char *scratch) { return (float4 *)scratch; }
static uint32_t *scratch_e_first(char *scratch, int R) {
    const size_t nw = ((size_t)R + 63) / 64;
    return (uint32_t *)(scratch + align_up(nw * 2 * 3 * sizeof(float4), 256));
}
static float *scratch_cam_rows(char *scratch, int R, int P) {
    return (float *)((char *)scratch_e_first(scratch, R) + align_up(4 * (size_t)P, 256));
}

template <int NV, bool ABS>
static hipError_t contrib_reduce(const Args &a, GeomState g, BinningState b, int R, const float *contrib,
                                 char *scratch, float *dL_dmean2D, float4 *dL_dconic, float *dL_dopacity,
                                 float *dL_dcolor, float *abs_dmean2D, hipStream_t s) {
    if (R == 0) return hipSuccess;  // every Gaussian has n_inst = 0: gaussian_backward writes the zeros
    const size_t nw = ((size_t)R + 63) / 64;
    const uint32_t *n_dev = b.scratch;  // L' (binning.hip)
    hipLaunchKernelGGL((contrib_segments_kernel<NV, ABS>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, n_dev,
                       b.gid_by_e, reinterpret_cast<const float4 *>(contrib),
                       grad_out(a, g, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, abs_dmean2D),
                       scratch_part(scratch), scratch_e_first(scratch, R));
    return hipGetLastError();
}

template <int NV, bool ABS, class... Raw>
static hipError_t gaussian_backward(const Args &a, GeomState g, int R, char *scratch, const int *radii,
                                    const float *means3D, const float *shs, const float *scales, const float *rotations,
                                    const float *cov3D, float *dL_dmean2D, float4 *dL_dconic, float *dL_dopacity,
                                    float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh,
                                    float *dL_dscale, float *dL_drot, float *abs_dmean2D, hipStream_t s, Raw... raw) {
    const GradOut o = grad_out(a, g, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, abs_dmean2D);
    if (shs) {
        const bool vec4 = a.M == 16 && (((size_t)shs | (size_t)dL_dsh) & 15) == 0;
        const auto kernel = vec4 ? gaussian_sh_backward_kernel<true, NV, ABS, Raw...>
                                 : gaussian_sh_backward_kernel<false, NV, ABS, Raw...>;
        hipLaunchKernelGGL(kernel,
                           dim3((a.P + kShThreads - 1) / kShThreads), dim3(kShThreads), 0, s, a, g, radii, means3D,
                           scales, rotations, cov3D, dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot,
                           scratch_e_first(scratch, R), scratch_part(scratch), o, shs, g.clamped, dL_dcolor, dL_dsh,
                           raw...);
    } else {
        hipLaunchKernelGGL((gaussian_backward_kernel<NV, ABS, Raw...>), dim3((a.P + 255) / 256), dim3(256), 0, s, a, g, radii, means3D,
                           scales, rotations, cov3D, dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D,
                           dL_dscale, dL_drot, scratch_e_first(scratch, R), scratch_part(scratch), o, raw...);
    }
    return hipGetLastError();
}

// `depth`: the records carry W3 (NV = 10 floats are reduced instead of 9); abs_dmean2D (P x 3, or NULL for none):
// the absgrad variants, which carry the records' floats 10 and 11 into it
hipError_t launch_contrib_reduce(const Args &a, GeomState g, BinningState b, int R, const float *contrib,
                                 char *scratch, bool depth, float *dL_dmean2D, float4 *dL_dconic,
                                 float *dL_dopacity, float *dL_dcolor, float *abs_dmean2D, hipStream_t s) {
    return with_backward_variant(depth, abs_dmean2D != nullptr, [&](auto depth_c, auto abs_c) {
        return contrib_reduce<depth_c.value ? 10 : 9, abs_c.value>(a, g, b, R, contrib, scratch, dL_dmean2D, dL_dconic,
                                                                   dL_dopacity, dL_dcolor, abs_dmean2D, s);
    });
}
hipError_t launch_gaussian_backward(const Args &a, GeomState g, int R, char *scratch, bool depth, const int *radii,
                                    const float *means3D, const float *shs, const float *scales,
                                    const float *rotations, const float *cov3D, float *dL_dmean2D,
                                    float4 *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D,
                                    float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot,
                                    float *abs_dmean2D, const float *opacities, float *dL_dcamera, hipStream_t s) {
    // opacities (the raw ones; NULL for none): the antialiased backward's instantiations; dL_dcamera (35 floats;
    // NULL for none): the camera-gradient ones, whose workgroups' rows camera_grad.hip then sums
    const hipError_t e = with_backward_variant(depth, abs_dmean2D != nullptr, [&](auto depth_c, auto abs_c) {
        constexpr int NV = depth_c.value ? 10 : 9;
        constexpr bool ABS = abs_c.value;
        const auto run = [&](auto... pack) {
            return gaussian_backward<NV, ABS>(a, g, R, scratch, radii, means3D, shs, scales, rotations, cov3D, dL_dmean2D,
                                              dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale,
                                              dL_drot, abs_dmean2D, s, pack...);
        };
        const CamRows rows{dL_dcamera ? scratch_cam_rows(scratch, R, a.P) : nullptr};
        if (opacities) return dL_dcamera ? run(opacities, rows) : run(opacities);
        return dL_dcamera ? run(rows) : run();
    });
    if (e != hipSuccess || !dL_dcamera) return e;
    const int block = shs ? kShThreads : 256;
    return launch_camera_grad_sum(scratch_cam_rows(scratch, R, a.P), (a.P + block - 1) / block, dL_dcamera, s);
}

}  // namespace gs4d
