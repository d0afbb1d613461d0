// render.hip -- per-tile front-to-back alpha blending (K6) and its reverse walk (K7).
//
// Reference: cuda_rasterizer/forward.cu:261-379 (renderCUDA forward) and backward.cu:399-557
// (renderCUDA backward).
//
// MI355X mapping (not the reference's): ONE wave64 per 16x16 tile; each lane owns a column of 4
// pixels (rows r, r+4, r+8, r+12 with r = lane/16), processed as two pairs with packed-f32 VALU
// (v_pk_fma/mul/add_f32: two pixels per instruction).  A tile's sorted splats are fetched 64 at a
// time, one per lane (the next batch is prefetched while the current one is blended), converted to
// blend-ready constants and staged in LDS; the blend loop reads each splat with wave-uniform
// (broadcast) ds_read_b128.  The Gaussian falloff is evaluated in base 2 (log2(e) folded into the
// conic once per splat) so each pixel costs one v_exp_f32.  Which pixels a splat touches is kept in
// 64-bit lane masks (scalar unit); pixels are retired by a mask, and termination (T < 1e-4, rare)
// takes a wave-uniform side path, so the common path is branch- and select-light.
//
// Backward: per pixel the reference keeps accum_rec[3] and last_color[3] only to form
// dL/dalpha = sum_c (c_c - accum_rec_c) * dL/dpix_c; since dL/dpix is constant per pixel this is
// carried as one scalar A = accum_rec . dL/dpix, updated eagerly after each contributing splat
// (A = alpha CD + (1 - alpha) A, the same recurrence as backward.cu:515-517).  The 9 gradient terms of
// a splat (backward.cu:523,545-554) are linear in 6 per-pixel moments (sum u, sum u dx, sum u dy,
// sum u dx^2, sum u dx dy, sum u dy^2 with u = G dL/dalpha) and 3 colour sums; these 9 values are
// reduced over the wave with column sums through LDS and a 16-lane DPP tree (reduce-scatter), staged in
// LDS, and stored once per (tile, splat) instance at its emission slot (coalesced 48-byte records,
// no float atomics).  The per-Gaussian pass (preprocess_backward.hip) sums a Gaussian's records in
// a fixed order and applies the moment -> gradient map once (bitwise reproducible).
#include <type_traits>

#include "gs4d_internal.h"

namespace gs4d {

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 bc2(float x) { return f2{x, x}; }
// x + y of a pixel pair as one v_add_f32 (the backend would form a v_pk_add_f32 with op_sel, 4 issue
// cycles against ~2.5 for the plain add when other waves share the SIMD: tools/bench/valu_rates.hip)
__device__ __forceinline__ float hsum(f2 v) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(v.x), "v"(v.y));
    return r;
}


// Blend-ready splat constants.  geo = (x, y - yc, -a/2 log2e, -b log2e), opc = (-c/2 log2e, lo, 1/o, m),
// col = (r, g, b, depth): o G = m 2^(power2 + lo) with m = 1, lo = log2 o for a positive-definite conic (the
// opacity folded into the exponent: the common path has no o * G multiply) and m = o, lo = 0 otherwise.  power2 = log2(e) * power (forward.cu:340-342) at offset d = mean - pixel.
// Rows are measured from the tile's centre row yc = 16 ty + 7.5 (pixel row py = yc + yl, yl a
// half-integer in [-7.5, 7.5]): dy = (my - yc) - yl, the same two roundings in both kernels.
struct SplatLDS {
    float4 geo, opc, col;
};
struct SplatRegs {
    float4 geo, opc, col;
    uint32_t reach;  // bit h: the splat reaches some pixel centre of half tile h (rows 8h..8h+7)
};

// The alpha test of forward.cu:346-348 / backward.cu:486-490 is taken exactly as the reference states
// it: alpha = min(0.99, o G) >= 1/255, i.e. the rounded product o G >= 1/255 (the cap is above the
// threshold).  The splat record's 1/o (0 for o = 0) lets the backward accumulate its moments on
// o G dL/dalpha and divide by o once per splat record.
constexpr float kAlphaMin = 1.0f / 255.0f;

// A batch of 64 splats, each the Gaussian's packed 48-byte blend record (GeomState::splat, written by
// preprocess: s0 = (x, y, -a/2 log2e, -b log2e), s1 = (-c/2 log2e, o, 1/o, depth), s2 = (r, g, b, 0)),
// gathered straight into LDS by LDS-DMA loads (global_load_lds: per-lane global address, destination
// base + lane * 16): three 16-byte pieces of ONE contiguous record per splat, so the prefetch of the
// next batch spans the current batch's walk without holding registers.
struct RawLDS {
    float4 s0[64], s1[64], s2[64];
};
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;
__device__ __forceinline__ void issue_raw_lds(RawLDS &r, bool valid, uint32_t gid, const float4 *__restrict__ splat) {
    if (valid) {
        const float4 *rec = splat + 3 * (size_t)gid;
        __builtin_amdgcn_global_load_lds((gbl_void_t *)rec, (lds_void_t *)r.s0, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void_t *)(rec + 1), (lds_void_t *)r.s1, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void_t *)(rec + 2), (lds_void_t *)r.s2, 16, 0, 0);
    }
}
// waits for this wave's LDS-DMA loads, then lane l reads its splat of the staged batch: blend constants
// with rows measured from the tile's centre row (geo.y = my - yc), zeros for lanes past the batch
// (opacity 0: the zero splat passes no pixel)
__device__ __forceinline__ void read_raw_lds(SplatRegs &s, const RawLDS &r, int lane, bool valid, float yc,
                                             bool block_barrier) {
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the LDS-DMA writes have landed (lgkm/exp counters not waited)
    if (block_barrier) __builtin_amdgcn_s_barrier();
    else __builtin_amdgcn_wave_barrier();
    if (valid) {
        const float4 s0 = r.s0[lane], s1 = r.s1[lane], s2 = r.s2[lane];
        s.geo = make_float4(s0.x, s0.y - yc, s0.z, s0.w);
        s.opc = make_float4(s1.x, s2.w, s1.z, s1.y);  // -c/2 log2e, exponent offset lo, 1/o, multiplier m
        // (the walks read c and lo as one 8-byte LDS load)
        s.col = make_float4(s2.x, s2.y, s2.z, s1.w);  // rgb, view depth
    } else {
        s.geo = s.opc = s.col = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Falloff of one splat at a pixel pair: exponent (base 2) and G = 2^power2.  Forward and backward use
// this one sequence, so they take identical blend decisions.
// alpha = min(0.99, o G) caps nothing for opacities at or below kCapFree: G = 2^power <= 1 wherever the
// power test passes (up to an ulp), so o G <= 0.98 (1 + ulp) < 0.99.
constexpr float kCapFree = 0.98f;
constexpr float kInvCapFree = 1.f / kCapFree;  // the record holds 1/o: o > kCapFree <=> 1/o < kInvCapFree
struct Falloff {
    f2 dy, pw, G, alpha;
};
// pa = geo.z dx^2 + lo (lane constant per splat: fmaf(geo.z dx, dx, lo)); FOLD: every splat of the walk has a
// positive-definite conic, so m = 1 and o G is the exponential itself
template <bool CAP = true, bool FOLD = false>
__device__ __forceinline__ Falloff falloff(const float4 &geo, const float4 &opc, float pa, float pb, f2 yl) {
    Falloff f;
    f.dy = bc2(geo.y) - yl;
    f.pw = fma2(f.dy, fma2(bc2(opc.x), f.dy, bc2(pb)), bc2(pa));
    f.G = f2{__builtin_amdgcn_exp2f(f.pw.x), __builtin_amdgcn_exp2f(f.pw.y)};
    const f2 al = FOLD ? f.G : bc2(opc.w) * f.G;
    // without CAP every splat of the batch has opacity <= kCapFree: min(0.99, o G) = o G
    f.alpha = CAP ? f2{fminf(0.99f, al.x), fminf(0.99f, al.y)} : al;
    return f;
}
__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// a wave-uniform 64-bit mask kept in scalar registers (the compiler's divergence analysis may otherwise move a
// loop-carried mask to VGPRs and turn its bit scans into vector code)
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((uint32_t)v);
}
// this lane's bit of a wave mask, used directly as the select condition (no VALU shift)
__device__ __forceinline__ bool lane_bit(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// ---------------------------------------------------------------------------------------------
// A splat whose conic is positive definite has power <= 0 at every pixel (up to rounding at its
// centre), so the power test of forward.cu:341 is only evaluated in batches holding another splat.
// The same float operations, uncontracted, as preprocess.hip's choice of the record's opacity form.
__device__ __forceinline__ bool conic_pd(const float4 &geo, const float4 &opc) {
    // geo.z = -a/2 k, geo.w = -b k, opc.x = -c/2 k (k = log2 e > 0): a > 0 and ac - b^2 > 0
    return geo.z < 0.f && __fsub_rn(__fmul_rn(__fmul_rn(4.f, geo.z), opc.x), __fmul_rn(geo.w, geo.w)) > 0.f;
}

// ---------------------------------------------------------------------------------------------
// K4 for short tiles, fused into the forward: a run of up to 64*R instances is sorted by the key
// (depth bits << 32 | emission slot) by one wave in registers, lane l holding positions l, 64 + l, ..
// Inside a tile the emission slot increases with the Gaussian id (emission follows the visible
// Gaussians in id order), so this is the reference's (depth, id) order (rasterizer_impl.cu:94-105,
// 304-309) and the key carries its own value.  Bitonic network in its all-ascending ("flip") form,
// unrolled: every partner is a compile-time (register, lane-xor) pair, so cross-lane steps are
// shuffles and cross-register steps plain selects; a length that is not a power of two is padded
// with +inf keys.  The sorted slots are written back for the backward and returned in ev[].
template <int R>
__device__ __forceinline__ void sort_keys(uint64_t key[R], int lane) {
#pragma unroll
    for (int k = 2; k <= 64 * R; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            const int mask = j == (k >> 1) ? k - 1 : j;  // flip, then half-cleaners
            const int lx = mask & 63, rx = mask >> 6;
            uint64_t pk[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int rq = r ^ rx;
                if (lx == 0) {
                    pk[r] = key[rq];
                } else {
                    const uint32_t hi = xor_lane((uint32_t)(key[rq] >> 32), lx);
                    const uint32_t lo = xor_lane((uint32_t)key[rq], lx);
                    pk[r] = ((uint64_t)hi << 32) | lo;
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const bool lower = ((r * 64 + lane) & j) == 0;
                const uint64_t kr = key[r];
                key[r] = lower ? (pk[r] < kr ? pk[r] : kr) : (pk[r] > kr ? pk[r] : kr);
            }
        }
    }
}
// the sort keys of run positions base + r * 64 + lane (+inf past n)
template <int R>
__device__ __forceinline__ void load_keys(uint64_t key[R], const uint32_t *__restrict__ seg, int base, int n,
                                          const uint32_t *__restrict__ gid_by_e, const float *__restrict__ depths,
                                          int lane) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int i = base + r * 64 + lane;
        const uint32_t e = i < n ? seg[i] : 0u;
        const uint32_t gid = i < n ? gid_by_e[e] & kGidMask : 0u;
        key[r] = i < n ? ((uint64_t)__float_as_uint(depths[gid]) << 32) | e : ~0ull;  // depths > 0.2
    }
}
template <int R>
__device__ __forceinline__ void sort_run(uint32_t *__restrict__ seg, int n, const uint32_t *__restrict__ gid_by_e,
                                         const float *__restrict__ depths, int lane, uint32_t ev[4]) {
    uint64_t key[R];
    load_keys<R>(key, seg, 0, n, gid_by_e, depths, lane);
    sort_keys<R>(key, lane);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = r * 64 + lane;
        ev[r] = r < R ? (uint32_t)key[r < R ? r : 0] : 0u;
        if (r < R && i < n) seg[i] = ev[r];
    }
}

// TWO waves per tile: wave h blends half tile h (rows 8h .. 8h + 7; lane l holds the pixel pair at rows
// 8h + l/16 and 8h + l/16 + 4 of column l % 16), so a long tile's serial blend walk is split over two
// waves.  With one wave per tile every tile of the metric scene was resident at once and the kernel's end
// was set by the longest tiles walking alone on their SIMDs (a launch repeating every tile took only
// 0.67 of the first pass's time per extra pass).  The short run's sort is done once, by wave 0, and
// handed to wave 1 through LDS (the only cross-wave step, one barrier); each wave then stages and walks
// the splats that reach its half on its own (LDS-DMA gathers, no barriers), and retires when its half's
// pixels are all done.
__global__ __launch_bounds__(128) void render_forward_kernel(Args a, const uint2 *__restrict__ ranges,
                                                             const uint32_t *__restrict__ order,
                                                             uint32_t *__restrict__ upos,
                                                             const float *__restrict__ depths,
                                                             const uint32_t *__restrict__ gid_by_e,
                                                             const float4 *__restrict__ splat,
                                                             float *__restrict__ final_T,
                                                             uint32_t *__restrict__ n_contrib,
                                                             float *__restrict__ out_color,
                                                             float *__restrict__ out_depth) {
    __shared__ SplatLDS s_sp_all[2][64];
    __shared__ RawLDS s_raw_all[2];
    __shared__ uint32_t s_ev[kWaveSortMax];
    const int tile = (int)__builtin_amdgcn_readfirstlane(order[blockIdx.x]);  // longest runs first
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int lane = threadIdx.x & 63;
    const int h = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // this wave's half tile
    SplatLDS *s_sp = s_sp_all[h];
    RawLDS &s_raw = s_raw_all[h];
    const int px = tx * kBlockX + (lane & 15);
    const int py0 = ty * kBlockY + 8 * h + (lane >> 4);
    const float pfx = (float)px;
    const float yc = (float)(ty * kBlockY) + 7.5f;
    const float ylane = (float)(8 * h + (lane >> 4)) - 7.5f;
    const f2 yl = f2{ylane, ylane + 4.f};
    // live pixels (forward.cu:287-289: pixels outside the image never blend) as a per-lane alpha
    // threshold: 1/255 while the pixel blends, 2 (above any alpha) once it is outside or retired, so the
    // alpha test is one compare per pixel and needs no scalar mask
    f2 thr;
    thr.x = (px < a.W && py0 < a.H) ? kAlphaMin : 2.f;
    thr.y = (px < a.W && py0 + 4 < a.H) ? kAlphaMin : 2.f;
    f2 T = bc2(1.f), C0 = bc2(0.f), C1 = bc2(0.f), C2 = bc2(0.f), Dp = bc2(0.f);
    uint32_t stop[2] = {0, 0};  // list position of the terminating splat (retired pixels)
    uint2 range = ranges[tile];
    range.x = __builtin_amdgcn_readfirstlane(range.x);
    range.y = __builtin_amdgcn_readfirstlane(range.y);
    // short runs: sorted here (wave 0), their emission slots kept in registers (batch b in ev[0] after
    // b shifts)
    const int n_run = (int)(range.y - range.x);
    const bool in_regs = n_run <= kWaveSortMax;
    uint32_t ev[4] = {0u, 0u, 0u, 0u};
    if (in_regs && n_run > 128) {
        // 129..256: each wave sorts 128 keys in registers, then one merge-path step over the two sorted
        // halves (thread t emits positions 2t, 2t + 1, its start found by a binary search on its
        // diagonal) -- half the network depth of one wave sorting all 256 (the sort is the walk's
        // start-up latency).  The keys go through the splat staging area, unused until the walk.
        uint32_t *seg = upos + range.x;
        uint64_t *s_key = reinterpret_cast<uint64_t *>(&s_sp_all[0][0]);
        uint64_t key[2];
        load_keys<2>(key, seg, 128 * h, n_run, gid_by_e, depths, lane);
        sort_keys<2>(key, lane);
        s_key[128 * h + lane] = key[0];
        s_key[128 * h + 64 + lane] = key[1];
        __syncthreads();
        const int t = threadIdx.x, d = 2 * t;
        int lo = max(0, d - 128), hi = min(d, 128);
        while (lo < hi) {  // ties (the +inf padding only) go to the first half, as below
            const int mid = (lo + hi) >> 1;
            if (s_key[mid] > s_key[128 + d - 1 - mid]) hi = mid;
            else lo = mid + 1;
        }
        int i = lo, j = d - lo;
        uint64_t xk = i < 128 ? s_key[i] : ~0ull, yk = j < 128 ? s_key[128 + j] : ~0ull;
        uint32_t outv[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const bool first = xk <= yk;
            outv[k] = (uint32_t)(first ? xk : yk);
            if (first) {
                i++;
                xk = i < 128 ? s_key[i] : ~0ull;
            } else {
                j++;
                yk = j < 128 ? s_key[128 + j] : ~0ull;
            }
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            s_ev[d + k] = outv[k];
            if (d + k < n_run) seg[d + k] = outv[k];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) ev[r] = s_ev[r * 64 + lane];
    } else if (in_regs) {
        if (h == 0) {
            if (n_run > 1) {
                uint32_t *seg = upos + range.x;
                if (n_run <= 64) sort_run<1>(seg, n_run, gid_by_e, depths, lane, ev);
                else sort_run<2>(seg, n_run, gid_by_e, depths, lane, ev);
            } else if (n_run == 1 && lane == 0) {
                ev[0] = upos[range.x];
            }
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (r * 64 < n_run) s_ev[r * 64 + lane] = ev[r];
        }
        __syncthreads();
        if (h == 1) {
#pragma unroll
            for (int r = 0; r < 4; r++) ev[r] = r * 64 + lane < n_run ? s_ev[r * 64 + lane] : 0u;
        }
    }
    // gid_by_e of each batch's instances, 4 batches at a time (the short run's are all loaded here);
    // the next batch's attributes are issued before the current one is blended and only turned into
    // blend constants when it comes up, so their loads overlap the blend loop
    uint32_t ug[4];
    int ids_left = 0;
    auto refill = [&](uint32_t first) {  // list positions first + r*64 + lane
        if (!in_regs) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t i = first + r * 64 + lane;
                ev[r] = i < range.y ? upos[i] : 0u;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t i = first + r * 64 + lane;
            ug[r] = i < range.y ? gid_by_e[ev[r]] : 0u;
        }
        ids_left = 4;
    };
    // the next batch's attributes are gathered into this wave's LDS by LDS-DMA loads (as the backward
    // does), only its lanes' reach bits stay in a register
    uint32_t rnxt = 0;
    auto fetch = [&](uint32_t first) {
        if (ids_left == 0) refill(first);
        const uint32_t rge = ug[0];
        ev[0] = ev[1]; ev[1] = ev[2]; ev[2] = ev[3];
        ug[0] = ug[1]; ug[1] = ug[2]; ug[2] = ug[3];
        ids_left--;
        rnxt = rge >> kReachShift;
        issue_raw_lds(s_raw, first + lane < range.y, rge & kGidMask, splat);
    };
    if (range.x < range.y) fetch(range.x);
    for (uint32_t base = range.x; base < range.y; base += 64) {
        if (ballot(thr.x < 1.f || thr.y < 1.f) == 0) break;  // forward.cu:312-314 (this half)
        SplatRegs nxt;
        const bool valid = base + lane < range.y;
        read_raw_lds(nxt, s_raw, lane, valid, yc, false);  // this wave's own staging: no block barrier
        nxt.reach = valid ? rnxt : 0u;
        const uint64_t reach = ballot((nxt.reach >> h) & 1u);
        // per-splat wave masks (the staged zero splats past a partial batch are neither)
        const uint64_t nonpd = ballot(valid && !conic_pd(nxt.geo, nxt.opc));
        const bool cap = ballot(valid && nxt.opc.z < kInvCapFree) != 0;  // wave-uniform: a splat the 0.99 cap can bind
        // one wave writes and reads its own staging area: LDS operations of a wave complete in order
        __builtin_amdgcn_wave_barrier();
        s_sp[lane].geo = nxt.geo;
        s_sp[lane].opc = nxt.opc;
        s_sp[lane].col = nxt.col;
        __builtin_amdgcn_wave_barrier();
        if (base + 64 < range.y) fetch(base + 64);
        const uint32_t pos0 = base - range.x;
        // the batch's splats that reach this half, two at a time: both falloffs are independent, only
        // the blend updates chain (a lone last splat runs alone)
        auto blend = [&](const Falloff &f, const float4 &col, uint32_t j, auto pwc) {
            bool k0 = f.alpha.x >= thr.x, k1 = f.alpha.y >= thr.y;  // forward.cu:346-348 (live pixels)
            if (decltype(pwc)::value && ((nonpd >> j) & 1)) {  // forward.cu:341-342
                k0 = k0 && f.pw.x <= 0.0f;
                k1 = k1 && f.pw.y <= 0.0f;
            }
            f2 ae = f2{k0 ? f.alpha.x : 0.f, k1 ? f.alpha.y : 0.f};
            f2 tT = T * (bc2(1.f) - ae);  // forward.cu:349
            if (ballot(fminf(tT.x, tT.y) < 0.0001f) != 0) {
                // forward.cu:350-354: the splat that would drop T below 1e-4 is not blended; the pixel retires
                const bool t0 = tT.x < 0.0001f, t1 = tT.y < 0.0001f;
                ae = f2{t0 ? 0.f : ae.x, t1 ? 0.f : ae.y};
                tT = f2{t0 ? T.x : tT.x, t1 ? T.y : tT.y};
                stop[0] = t0 ? pos0 + j : stop[0];
                stop[1] = t1 ? pos0 + j : stop[1];
                thr = f2{t0 ? 2.f : thr.x, t1 ? 2.f : thr.y};
            }
            // every live pixel takes the update; pixels the splat does not touch have ae = 0
            const f2 w = ae * T;  // forward.cu:357-358
            C0 = fma2(bc2(col.x), w, C0);
            C1 = fma2(bc2(col.y), w, C1);
            C2 = fma2(bc2(col.z), w, C2);
            Dp = fma2(bc2(col.w), w, Dp);
            T = tT;
        };
        auto walk = [&](auto capc, auto pwc) {
            constexpr bool CAP = decltype(capc)::value, FOLD = !decltype(pwc)::value;
            for (uint64_t todo = reach; todo != 0;) {
                const uint32_t j0 = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                const bool two = todo != 0;
                const uint32_t j1 = two ? (uint32_t)__builtin_ctzll(todo) : j0;
                todo &= todo - (two ? 1 : 0);
                const float4 geo0 = s_sp[j0].geo, opc0 = s_sp[j0].opc, col0 = s_sp[j0].col;
                const float4 geo1 = s_sp[j1].geo, opc1 = s_sp[j1].opc, col1 = s_sp[j1].col;
                const float dx0 = geo0.x - pfx, dx1 = geo1.x - pfx;
                const Falloff f0 = falloff<CAP, FOLD>(geo0, opc0, fmaf(geo0.z * dx0, dx0, opc0.y), geo0.w * dx0, yl);
                const Falloff f1 = falloff<CAP, FOLD>(geo1, opc1, fmaf(geo1.z * dx1, dx1, opc1.y), geo1.w * dx1, yl);
                blend(f0, col0, j0, pwc);
                if (two) blend(f1, col1, j1, pwc);
            }
        };
        // the batch's walk without the 0.99 cap unless one of its splats has opacity > kCapFree, and
        // without the power test unless one has a conic that is not positive definite (cov3D_precomp)
        if (nonpd != 0) walk(std::true_type{}, std::true_type{});
        else if (cap) walk(std::true_type{}, std::false_type{});
        else walk(std::false_type{}, std::false_type{});
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);  // an early exit may leave the next batch's LDS-DMA loads in flight
    const size_t HW = (size_t)a.W * a.H;
    const V3 bg = load_v3(a.bg);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int py = py0 + 4 * k;
        if (px < a.W && py < a.H) {
            const float t = k ? T.y : T.x;
            const size_t pix = (size_t)py * a.W + px;
            final_T[pix] = t;
            // splats at positions >= n_contrib never blended into this pixel (the backward's bound):
            // the terminating splat's position, or the list length for pixels that never terminated
            n_contrib[pix] = (k ? thr.y : thr.x) < 1.f ? range.y - range.x : stop[k];
            out_color[pix] = (k ? C0.y : C0.x) + t * bg.x;
            out_color[HW + pix] = (k ? C1.y : C1.x) + t * bg.y;
            out_color[2 * HW + pix] = (k ? C2.y : C2.x) + t * bg.z;
            out_depth[pix] = k ? Dp.y : Dp.x;
        }
    }
}

hipError_t launch_render_forward(const Args &a, GeomState g, BinningState b, ImageState img, float *out_color,
                                 float *out_depth, hipStream_t s) {
    const int T = a.gx * a.gy;
    hipLaunchKernelGGL(render_forward_kernel, dim3(T), dim3(128), 0, s, a, img.ranges, img.order, b.upos, g.depths,
                       b.gid_by_e, g.splat, img.final_T, img.n_contrib, out_color, out_depth);
    return hipGetLastError();
}

// Diagnostic (test infrastructure's view of the blend arithmetic): o G and the base-2 exponent of given
// (Gaussian, pixel) pairs, by the exact sequence both blend kernels evaluate (read_raw_lds's row shift,
// falloff()), so the parity tests can measure how far the blend's alpha lies from the oracle's near the
// 1/255 threshold and size the near-threshold band from that measurement.
__global__ void pair_alpha_kernel(const float4 *__restrict__ splat, int n, const int *__restrict__ gid,
                                  const int *__restrict__ px, const int *__restrict__ py, float *__restrict__ og,
                                  float *__restrict__ pw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 *rec = splat + 3 * (size_t)gid[i];
    const float4 s0 = rec[0], s1 = rec[1];
    const int ty = py[i] / kBlockY;
    const float yc = (float)(ty * kBlockY) + 7.5f;
    const float yl = (float)(py[i] - ty * kBlockY) - 7.5f;
    const float4 geo = make_float4(s0.x, s0.y - yc, s0.z, s0.w);
    const float4 opc = make_float4(s1.x, rec[2].w, s1.z, s1.y);
    const float dx = geo.x - (float)px[i];
    const Falloff f = falloff<false>(geo, opc, fmaf(geo.z * dx, dx, opc.y), geo.w * dx, f2{yl, yl});
    og[i] = f.alpha.x;
    pw[i] = f.pw.x;
}
hipError_t launch_pair_alpha(GeomState g, int n, const int *gid, const int *px, const int *py, float *og, float *pw,
                             hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(pair_alpha_kernel, dim3((n + 255) / 256), dim3(256), 0, s, g.splat, n, gid, px, py, og, pw);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// lanes 0-31 of the result hold a's half-wave sums, lanes 32-63 b's (v_permlane32_swap)
__device__ __forceinline__ float swap32_add(float a, float b) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// rows (0,1,2,3) of the result hold (a rows 0+1, b rows 0+1, a rows 2+3, b rows 2+3) (v_permlane16_swap)
__device__ __forceinline__ float swap16_add(float a, float b) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Per-lane partial sums of one splat of the reverse walk, its pixel pair already added: the moments
// of u = G dL/dalpha in the tile-centred row coordinate yl (sum u, sum u yl, sum u yl^2) and the
// colour sums (sum w dL/dpix_c, w = alpha T).
struct SplatPart {
    float u0, u1, u2, w0, w1, w2;
};

// Column sums of one register quadruple through the wave's 1 KiB transpose buffer `col` (one round): every lane
// stores its four values, lane (g = lane / 16, c = lane % 16) reads value g of the four lanes (r, c) of its column
// and adds them as (row 0 + row 2) + (row 1 + row 3) -- the association v_permlane32_swap then v_permlane16_swap
// and their adds give, so the result is theirs to the bit.  LDS instructions take no VALU issue cycles: a round
// costs the VALU its 3 adds, against 3 swaps (8.25 issue cycles each, tools/bench/valu_rates.hip) and 3 adds.
// Layout: (v0, v1) as one float2 at word 2 lane, (v2, v3) at word 128 + 2 lane, so value g of lane (r, c) lies
// at word 128 (g / 2) + 32 r + 2 c + g % 2.  A 4-byte read banks on (word mod 32) within each 32-lane group
// (MI355X: ds_read_b32): the group's lanes have g / 2 and r in common and 2 c + g % 2 covers 0..31 once -- no
// conflict (one float4 per lane at word 4 lane would put columns c and c + 8 on one bank); the 8-byte stores
// are lane-contiguous.  One wave is the workgroup and a wave's LDS operations complete in order, so rounds
// reuse the buffer with no s_barrier and no wait: the wave barriers only keep the compiler from reordering
// the stores and loads, and each read is waited for (counted lgkmcnt) where its add consumes it.
constexpr int kColSumWords = 256;
__device__ __forceinline__ float lds_col_sum(float *col, int lane, float v0, float v1, float v2, float v3) {
    float2 *st = reinterpret_cast<float2 *>(col) + lane;
    st[0] = make_float2(v0, v1);
    st[64] = make_float2(v2, v3);
    __builtin_amdgcn_wave_barrier();
    const float *rd = col + ((lane >> 5) << 7) + ((lane & 15) << 1) + ((lane >> 4) & 1);
    const float p0 = rd[0], p1 = rd[32], p2 = rd[64], p3 = rd[96];
    __builtin_amdgcn_wave_barrier();
    return (p0 + p2) + (p1 + p3);
}

// Wave64 totals of two splats' partial sums, left in LDS as their 9 record values:
//   0 sum u, 1 sum dx u, 2 sum u yl, 3 sum dx^2 u, 4 sum dx u yl, 5 sum u yl^2, 6-8 colour sums
// (dx = mean.x - pixel x, per lane column).  Each value is first summed over the 4 lanes of a column
// (reduce-scatter: row r of x1 ends with (a.u0, a.u1, b.u0, b.u1)[r], of x2 (a.u2, a.w0, b.u2, b.w0)[r], of
// x3 (a.w1, a.w2, b.w1, b.w2)[r]) by three rounds of lds_col_sum() (COLS_LDS, the blend's form; the DEPTH value
// and the ABS pair take a round each), or by v_permlane32_swap then v_permlane16_swap (the earlier form, kept
// as the reference of gs4d_debug_wave_sum only: same bits); the dx-weighted moments x4, x5 are
// formed on those column sums.  The 16 columns of each row are then reduce-scattered too, with DPP:
// pairs of registers halve at each of the four stages (column c with c ^ 8, the half-row mirror, c ^ 2,
// c ^ 1), so every lane ends with one finished total (15 DPP-stage instructions for the 5 registers
// instead of 20 for 5 butterflies) and writes it with ONE ds_write at a lane-constant offset `roff`
// (red_offset(); -1: nothing to write).
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// record float offset (from record j's start; record j + 1 follows at +12) of this lane's total.
// DEPTH: the odd rows of x5, which hold nothing otherwise, carry the depth sum W3 = sum w dL/ddepth to
// record float 9 (the first of the three free floats after W2).
// ABS: a sixth register x7 = (a.AX, a.AY, b.AX, b.AY) shares x5's tree from stage B on and ends in column 6:
// the absolute sums of the absgrad walk, record floats 10 and 11 (the record is full).
template <bool DEPTH, bool ABS>
__device__ __forceinline__ int red_offset(int lane) {
    const int r = lane >> 4, c = lane & 15, splat = (r >> 1) * 12, odd = r & 1;
    switch (c) {
    case 0: return splat + (odd ? 2 : 0);   // x1: S u, S u yl
    case 4: return splat + (odd ? 8 : 7);   // x3: W1, W2
    case 8: return splat + (odd ? 6 : 5);   // x2: S u yl^2, W0
    case 12: return splat + (odd ? 4 : 1);  // x4: S dx u yl, S dx u
    case 2: return odd ? (DEPTH ? splat + 9 : -1) : splat + 3;  // x5: S dx^2 u (odd rows: W3 or nothing)
    case 6: return ABS ? splat + (odd ? 11 : 10) : -1;          // x7: S |u fx|, S |u fy|
    default: return -1;
    }
}
template <bool DEPTH, bool ABS, bool COLS_LDS = true>
__device__ __forceinline__ void wave_sum_pair_to_lds(const SplatPart &a, const SplatPart &b, float dxa, float dxb,
                                                     float w3a, float w3b, float axa, float aya, float axb, float ayb,
                                                     float *col, float *rec_pair, int lane, int roff) {
    // x6 (DEPTH): rows 1 and 3 hold the column sums of a's and b's W3; x7 (ABS) = (a.AX, a.AY, b.AX, b.AY)
    float x1, x2, x3, x6 = 0.f, x7 = 0.f;
    if (COLS_LDS) {
        x1 = lds_col_sum(col, lane, a.u0, a.u1, b.u0, b.u1);
        x2 = lds_col_sum(col, lane, a.u2, a.w0, b.u2, b.w0);
        x3 = lds_col_sum(col, lane, a.w1, a.w2, b.w1, b.w2);
        if (DEPTH) x6 = lds_col_sum(col, lane, 0.f, w3a, 0.f, w3b);
        if (ABS) x7 = lds_col_sum(col, lane, axa, aya, axb, ayb);
    } else {
        const float h0 = swap32_add(a.u0, b.u0);  // lanes 0-31: a, 32-63: b
        const float h1 = swap32_add(a.u1, b.u1);
        const float h2 = swap32_add(a.u2, b.u2);
        const float h3 = swap32_add(a.w0, b.w0);
        const float h4 = swap32_add(a.w1, b.w1);
        const float h5 = swap32_add(a.w2, b.w2);
        x1 = swap16_add(h0, h1);
        x2 = swap16_add(h2, h3);
        x3 = swap16_add(h4, h5);
        if (DEPTH) x6 = swap16_add(0.f, swap32_add(w3a, w3b));
        if (ABS) x7 = swap16_add(swap32_add(axa, axb), swap32_add(aya, ayb));
    }
    const float dxs = lane < 32 ? dxa : dxb;  // rows 0-1 hold splat a, rows 2-3 splat b
    const float x4 = x1 * dxs;                 // (dx a.u0, dx a.u1, dx b.u0, dx b.u1)
    const float x5 = x4 * dxs;                 // (dx^2 a.u0, -, dx^2 b.u0, -)
    const bool c8 = (lane & 8) == 0, c4 = (lane & 4) == 0, c2 = (lane & 2) == 0;
    // stage A (c, c ^ 8): x1 | x2 -> z12, x3 | x4 -> z34, x5 -> z5
    const float z12 = (c8 ? x1 : x2) + dpp<0x128>(c8 ? x2 : x1);  // row_ror:8
    const float z34 = (c8 ? x3 : x4) + dpp<0x128>(c8 ? x4 : x3);
    float z5 = x5 + dpp<0x128>(x5);
    if (DEPTH) {
        // x6's odd rows take z5's unused odd rows from here on (one DPP move more).  They join after x5's own
        // stage A so that the even rows' arithmetic is the colour-only kernel's to the bit (x5's product and add
        // contract into one fma there).
        const float z6 = x6 + dpp<0x128>(x6);
        z5 = (lane & 16) ? z6 : z5;
    }
    // stage B (half-row mirror): z12 | z34 -> w
    const float w = (c4 ? z12 : z34) + dpp<0x141>(c4 ? z34 : z12);
    float w5;
    if (ABS) {
        // x7 takes its own stage A (sums only, no product) and the half of z5's stage B that carried copies: the
        // columns with bit 2 clear keep x5's sums in x5's order (the bits of S dx^2 u and W3 stay), the others x7's
        const float z7 = x7 + dpp<0x128>(x7);
        w5 = (c4 ? z5 : z7) + dpp<0x141>(c4 ? z7 : z5);
    } else {
        w5 = z5 + dpp<0x141>(z5);
    }
    // stage C (c ^ 2): w | w5 -> v; stage D (c ^ 1)
    const float v = (c2 ? w : w5) + dpp<0x4E>(c2 ? w5 : w);  // quad_perm [2, 3, 0, 1]
    const float u = v + dpp<0xB1>(v);                         // quad_perm [1, 0, 3, 2]
    if (roff >= 0) rec_pair[roff] = u;
}

// Diagnostic (gs4d_debug_wave_sum): one wave per pair of splats runs wave_sum_pair_to_lds on given per-lane
// inputs, `in` = n x kWaveSumInputs x 64 floats (value k of lane l of pair p at (p kWaveSumInputs + k) 64 + l):
// k = 0-5 a's (u0, u1, u2, w0, w1, w2), 6-11 b's, 12-13 W3 of a and b, 14-17 (a.AX, a.AY, b.AX, b.AY), 18-19 the
// lanes' dx of a and b.  out = n x 24: the two records as the blend's s_rec holds them (floats no lane writes: 0).
constexpr int kWaveSumInputs = 20;
template <bool DEPTH, bool ABS, bool COLS_LDS>
__global__ __launch_bounds__(64) void wave_sum_debug_kernel(const float *__restrict__ in, float *__restrict__ out) {
    __shared__ float s_col[kColSumWords];
    __shared__ float s_rec[24];
    const int lane = threadIdx.x;
    const float *p = in + ((size_t)blockIdx.x * kWaveSumInputs) * 64 + lane;
    if (lane < 24) s_rec[lane] = 0.f;
    __syncthreads();
    const SplatPart a{p[0], p[64], p[128], p[192], p[256], p[320]};
    const SplatPart b{p[384], p[448], p[512], p[576], p[640], p[704]};
    wave_sum_pair_to_lds<DEPTH, ABS, COLS_LDS>(a, b, p[18 * 64], p[19 * 64], p[12 * 64], p[13 * 64], p[14 * 64],
                                               p[15 * 64], p[16 * 64], p[17 * 64], s_col, s_rec, lane,
                                               red_offset<DEPTH, ABS>(lane));
    __syncthreads();
    if (lane < 24) out[(size_t)blockIdx.x * 24 + lane] = s_rec[lane];
}
hipError_t launch_wave_sum_debug(int n, const float *in, bool depth, bool abs, float *out_lds, float *out_permlane,
                                 hipStream_t s) {
    if (n <= 0) return hipSuccess;
    return with_backward_variant(depth, abs, [&](auto depth_c, auto abs_c) {
        hipLaunchKernelGGL((wave_sum_debug_kernel<depth_c.value, abs_c.value, true>), dim3(n), dim3(64), 0, s, in,
                           out_lds);
        hipLaunchKernelGGL((wave_sum_debug_kernel<depth_c.value, abs_c.value, false>), dim3(n), dim3(64), 0, s, in,
                           out_permlane);
        return hipGetLastError();
    });
}

// Per-pixel state of the reverse walk (pairs): T (recovered backwards), A = accum_rec . dL/dpix and
// dL/dpix.  The background term of backward.cu:534, -T_final / (1 - alpha) (bg . dL/dpix), is the
// background taken as one more layer behind the last contributor (colour bg, alpha 1): A starts at
// bg . dL/dpix instead of 0, and T_final / (1 - alpha_i) = T_i prod_{i<j} (1 - alpha_j) follows from
// the walk's own T -- the same value up to rounding, without a per-pixel constant.
// dd = dL/ddepth (the depth-gradient instantiation only): the depth image is one more blended channel
// whose "colour" is the splat's view depth and whose background is 0, so A needs no second accumulator.
struct BwdPixels {
    f2 T[2], A[2], dp0[2], dp1[2], dp2[2], dd[2];
};

// The per-splat half of a step (half_step below, which explains ALL and GEN): falloff, the reference's skip
// decisions and alpha.
struct HalfAlpha {
    f2 ale, ae, om;  // o G with the skips applied, alpha, 1 - alpha
    f2 dy;           // mean row - pixel row (read by the absgrad walk only)
};
template <bool ALL, bool GEN>
__device__ __forceinline__ HalfAlpha half_alpha(const f2 Y2, const f2 C2, const f2 O2, const f2 pa2, const f2 pb2,
                                                f2 yl, bool chk, uint32_t contributor, uint32_t last0,
                                                uint32_t last1) {
    const f2 dy = Y2 - yl;  // Y2 = my - yc
    const f2 pw = fma2(dy, fma2(C2, dy, pb2), pa2);
    const f2 G = f2{__builtin_amdgcn_exp2f(pw.x), __builtin_amdgcn_exp2f(pw.y)};
    // o G: min(0.99, o G) >= 1/255 iff o G >= 1/255.  Without GEN every splat of the pair has a positive-
    // definite conic, whose record folds o into the exponent (O2 = m = 1)
    const f2 al = GEN ? O2 * G : G;
    // backward.cu:486-497: contributor test, alpha < 1/255 and power > 0 skip -- the forward's decisions
    bool k0 = al.x >= kAlphaMin, k1 = al.y >= kAlphaMin;
    if (!ALL) {
        k0 = k0 && contributor < last0;
        k1 = k1 && contributor < last1;
    }
    if (GEN) {
        k0 = k0 && (!chk || pw.x <= 0.0f);
        k1 = k1 && (!chk || pw.y <= 0.0f);
    }
    // the skip applied to o G: a skipped pixel has alpha 0 exactly
    HalfAlpha h;
    h.dy = dy;
    h.ale = f2{k0 ? al.x : 0.f, k1 ? al.y : 0.f};
    h.ae = GEN ? f2{fminf(0.99f, h.ale.x), fminf(0.99f, h.ale.y)} : h.ale;
    h.om = bc2(1.f) - h.ae;
    return h;
}
// The rest of a step once the splat's T (the transmittance in front of it, Tn) is known.
// DEPTH: diff gains d_g dL/ddepth as its last term (dL/ddepth = 0 leaves every value as it was) and
// U[6] = W3 accumulates w dL/ddepth.
// ABS (absgrad): the pixel's pull on the 2-D mean is u' times the exponent's slope, d power2 / d mean =
// (fx, fy) = (2 geo.z dx + geo.w dy, geo.w dx + 2 opc.x dy) = -log2e (a dx + b dy, b dx + c dy) (backward.cu:
// 541-546); the last two sums take |u'| |fx| and |u'| |fy| -- plain v_fma_f32 with |src| modifiers, packed f32
// has none.  A skipped pixel has u' = 0 and adds an exact 0.  Nothing else reads fx, fy.
struct AbsOps {
    f2 QX2, BW2, CC2;  // 2 geo.z dx (per lane), geo.w, 2 opc.x; pb2 = geo.w dx is the falloff's own
};
template <bool GEN, bool DEPTH, bool ABS, int NU>
__device__ __forceinline__ void half_accum(const HalfAlpha &h, const f2 Tn, f2 &A, const f2 dp0, const f2 dp1,
                                           const f2 dp2, const f2 dd, const f2 R2, const f2 G2, const f2 B2,
                                           const f2 D2, const f2 pb2, const AbsOps &ao, f2 yl, f2 yl2, f2 (&U)[NU]) {
    static_assert(NU == 6 + (DEPTH ? 1 : 0) + (ABS ? 2 : 0), "sums: 6, W3 with DEPTH, then the two absolute sums");
    f2 &U0 = U[0], &U1 = U[1], &U2 = U[2], &W0 = U[3], &W1 = U[4], &W2 = U[5];
    f2 diff = fma2(B2, dp2, fma2(G2, dp1, fma2(R2, dp0, -A)));  // c . dL/dpix - accum_rec . dL/dpix
    if (DEPTH) diff = fma2(D2, dd, diff);                        // + d_g dL/ddepth
    A = fma2(h.ae, diff, A);                    // accum_rec for the next splat in front
    const f2 w = h.ae * Tn;                     // dchannel_dcolor (backward.cu:521)
    // u' = o G dL/dalpha = o G T diff (backward.cu:519-534, bg term in A's start value); without the
    // cap o G T = w
    const f2 u = (GEN ? h.ale * Tn : w) * diff;
    U0 += u;
    U1 = fma2(u, yl, U1);
    U2 = fma2(u, yl2, U2);
    W0 = fma2(w, dp0, W0);
    W1 = fma2(w, dp1, W1);
    W2 = fma2(w, dp2, W2);
    if (DEPTH) U[6] = fma2(w, dd, U[6]);
    if (ABS) {
        const f2 fx = fma2(ao.BW2, h.dy, ao.QX2), fy = fma2(ao.CC2, h.dy, pb2);
        f2 &AX = U[NU - 2], &AY = U[NU - 1];
        AX.x = fmaf(fabsf(u.x), fabsf(fx.x), AX.x);
        AX.y = fmaf(fabsf(u.y), fabsf(fx.y), AX.y);
        AY.x = fmaf(fabsf(u.x), fabsf(fy.x), AY.x);
        AY.y = fmaf(fabsf(u.y), fabsf(fy.y), AY.y);
    }
}
// One half tile of one splat of the reverse walk: updates the half's pixel state and adds its
// per-lane partial sums (moments of u' = o G dL/dalpha in the tile-centred row coordinate yl -- the
// record divides them by o once -- and the colour sums) to U0..U2 / W0..W2.  The falloff is the
// forward's sequence (falloff()) on operand pairs: identical blend decisions.  Branch-free, so that the
// pair walk below is one basic block.
//   ALL: the splat lies below every pixel's n_contrib (the contributor test passes; pixels outside
//        the image have T = dL/dpix = 0 and contribute exact zeros).
//   GEN: the general splat: `chk` = its conic is not positive definite (power > 0 skips, forward.cu:341),
//        and the 0.99 cap applies; without GEN the opacity is <= kCapFree, so o * G never reaches the cap.
// Two splats walking the same half share one reciprocal (half_pair_step): T in front of the back splat
// a is T / (1 - alpha_a), in front of b T / ((1 - alpha_a)(1 - alpha_b)) -- one v_rcp_f32 of the
// product per pixel (8 issue cycles each) and two multiplies instead of two reciprocals.
struct SplatOps {
    f2 Y2, C2, O2, R2, G2, B2, D2, pa2, pb2;  // D2 = the view depth (read by the depth-gradient walk only)
    bool chk;
    uint32_t contributor;
    AbsOps ao;  // read by the absgrad walk only
};
template <bool ALL, bool GEN, bool DEPTH, bool ABS, int NU>
__device__ __forceinline__ void half_step(f2 &T, f2 &A, const f2 dp0, const f2 dp1, const f2 dp2, const f2 dd,
                                          const SplatOps &s, f2 yl, f2 yl2, uint32_t last0, uint32_t last1,
                                          f2 (&U)[NU]) {
    const HalfAlpha h = half_alpha<ALL, GEN>(s.Y2, s.C2, s.O2, s.pa2, s.pb2, yl, s.chk, s.contributor, last0, last1);
    const f2 inv = f2{__builtin_amdgcn_rcpf(h.om.x), __builtin_amdgcn_rcpf(h.om.y)};
    const f2 Tn = T * inv;  // backward.cu:503
    T = Tn;
    half_accum<GEN, DEPTH, ABS>(h, Tn, A, dp0, dp1, dp2, dd, s.R2, s.G2, s.B2, s.D2, s.pb2, s.ao, yl, yl2, U);
}
template <bool ALL, bool GEN, bool DEPTH, bool ABS, int NU>
__device__ __forceinline__ void half_pair_step(f2 &T, f2 &A, const f2 dp0, const f2 dp1, const f2 dp2, const f2 dd,
                                               const SplatOps &sa, const SplatOps &sb, f2 yl, f2 yl2, uint32_t last0,
                                               uint32_t last1, f2 (&Ua)[NU], f2 (&Ub)[NU]) {
    const HalfAlpha ha = half_alpha<ALL, GEN>(sa.Y2, sa.C2, sa.O2, sa.pa2, sa.pb2, yl, sa.chk, sa.contributor,
                                              last0, last1);
    const HalfAlpha hb = half_alpha<ALL, GEN>(sb.Y2, sb.C2, sb.O2, sb.pa2, sb.pb2, yl, sb.chk, sb.contributor,
                                              last0, last1);
    const f2 prod = ha.om * hb.om;
    const f2 r = f2{__builtin_amdgcn_rcpf(prod.x), __builtin_amdgcn_rcpf(prod.y)};
    const f2 Tb = T * r;         // backward.cu:503 twice: T / (1 - alpha_a) / (1 - alpha_b)
    const f2 Ta = Tb * hb.om;    // T / (1 - alpha_a)
    half_accum<GEN, DEPTH, ABS>(ha, Ta, A, dp0, dp1, dp2, dd, sa.R2, sa.G2, sa.B2, sa.D2, sa.pb2, sa.ao, yl, yl2, Ua);
    half_accum<GEN, DEPTH, ABS>(hb, Tb, A, dp0, dp1, dp2, dd, sb.R2, sb.G2, sb.B2, sb.D2, sb.pb2, sb.ao, yl, yl2, Ub);
    T = Tb;
}

constexpr int kBwdDepthWaves = 4;  // waves per SIMD of the depth-gradient instantiation (<= 128 VGPRs)
// 4 waves per SIMD (<= 128 VGPRs, no spills): the reach-combo blocks hold at most the four falloff chains
// of one pair.  DEPTH (gs4d_backward_depth): dL/ddepth joins the walk as a fourth channel; its extra
// per-pixel state, operands and sums are kBwdDepthWaves's business.  ABS (gs4d_backward_absgrad):
// two more sums per splat and their three operands, with or without DEPTH.
constexpr int kBwdAbsWaves = 3;  // waves per SIMD of the two absgrad instantiations (<= 168 VGPRs)
constexpr int bwd_waves(bool depth, bool abs) { return abs ? kBwdAbsWaves : depth ? kBwdDepthWaves : 4; }
template <bool DEPTH, bool ABS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(bwd_waves(DEPTH, ABS), bwd_waves(DEPTH, ABS)))) void render_backward_kernel(Args a, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ order,
                            const uint32_t *__restrict__ gid_by_e,
                            const uint32_t *__restrict__ upos, const float4 *__restrict__ splat,
                            const float *__restrict__ final_Ts,
                            const uint32_t *__restrict__ n_contrib, const float *__restrict__ dL_dpixels,
                            const float *__restrict__ dL_ddepths, const float *__restrict__ dL_dalphas,
                            float *__restrict__ contrib) {
    constexpr int NU = 6 + (DEPTH ? 1 : 0) + (ABS ? 2 : 0);
    __shared__ SplatLDS s_sp[64];
    __shared__ float4 s_rec[64][3];  // reduced sums of the batch's splats
    // the reduction's transpose buffer: 10,240 B of LDS per workgroup with it, 16 workgroups on a CU's 160 KiB
    __shared__ float s_col[kColSumWords];
    const int tile = (int)__builtin_amdgcn_readfirstlane(order[blockIdx.x]);  // longest runs first
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int lane = threadIdx.x;
    const int px = tx * kBlockX + (lane & 15);
    const int py0 = ty * kBlockY + (lane >> 4);
    const float pfx = (float)px;
    const size_t HW = (size_t)a.W * a.H;
    uint2 range = ranges[tile];
    range.x = __builtin_amdgcn_readfirstlane(range.x);
    range.y = __builtin_amdgcn_readfirstlane(range.y);
    if (range.y <= range.x) return;
    const V3 bg = load_v3(a.bg);
    // rows relative to the tile's centre row (ty*16 + 7.5): the y moments are accumulated in them
    const float ylane = (float)(lane >> 4) - 7.5f;
    const f2 yl[2] = {f2{ylane, ylane + 4.f}, f2{ylane + 8.f, ylane + 12.f}};
    const f2 yl2[2] = {yl[0] * yl[0], yl[1] * yl[1]};
    const float yc = (float)(ty * kBlockY) + 7.5f;
    const int roff = red_offset<DEPTH, ABS>(lane);

    BwdPixels st;
    uint32_t lastc[4];
    uint64_t inside_m[4];
    uint32_t max_last = 0, min_last = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int py = py0 + 4 * k;
        const bool inside = px < a.W && py < a.H;
        const size_t pix = (size_t)py * a.W + px;
        const float tf = inside ? final_Ts[pix] : 0.f;
        const float d0 = inside ? dL_dpixels[pix] : 0.f;
        const float d1 = inside ? dL_dpixels[HW + pix] : 0.f;
        const float d2 = inside ? dL_dpixels[2 * HW + pix] : 0.f;
        const float d3 = (DEPTH && inside) ? dL_ddepths[pix] : 0.f;
        lastc[k] = inside ? n_contrib[pix] : 0u;
        inside_m[k] = ballot(inside);
        // dL/dalpha of the alpha image 1 - T_final (gs4d_backward_aux; NULL, a wave-uniform test, for none):
        // d(1 - T_final)/dalpha_i = T_final / (1 - alpha_i) is the background layer's factor with colour -1
        const float dA = (dL_dalphas && inside) ? dL_dalphas[pix] : 0.f;
        const float a0 = (bg.x * d0 + bg.y * d1 + bg.z * d2) - dA;  // the background layer behind the last splat
        const int h = k >> 1;
        if (k & 1) {
            st.T[h].y = tf; st.dp0[h].y = d0; st.dp1[h].y = d1; st.dp2[h].y = d2; st.A[h].y = a0;
            st.dd[h].y = d3;
        } else {
            st.T[h].x = tf; st.dp0[h].x = d0; st.dp1[h].x = d1; st.dp2[h].x = d2; st.A[h].x = a0;
            st.dd[h].x = d3;
        }
        max_last = max(max_last, lastc[k]);
        if (inside) min_last = min(min_last, lastc[k]);
    }
    // splats at list position >= every pixel's n_contrib never contribute: the walk starts there;
    // below every inside pixel's n_contrib the contributor test (backward.cu:486-488) always passes
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        max_last = max(max_last, (uint32_t)__shfl_xor((int)max_last, off));
        min_last = min(min_last, (uint32_t)__shfl_xor((int)min_last, off));
    }
    max_last = __builtin_amdgcn_readfirstlane(max_last);
    min_last = __builtin_amdgcn_readfirstlane(min_last);

    const uint32_t len = range.y - range.x;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t p = max_last + lane; p < len; p += 64) {
        float4 *rec = reinterpret_cast<float4 *>(contrib + (size_t)upos[range.x + p] * kContribStride);
        rec[0] = z4;
        rec[1] = z4;
        rec[2] = z4;
    }
    // The walk's instances: emission slot e (where the gradient record goes) and gid_by_e[e] of list
    // position end-1-lane of each batch, loaded 2 batches at a time (independent loads, one wait per
    // refill).  The next batch's attributes are issued before the current batch is blended and only
    // turned into blend constants after it, so their loads are the only ones in flight across the
    // blend loop.
    constexpr int kRing = 2;
    uint32_t ue[kRing], ug[kRing];
    int ids_left = 0;
    auto refill = [&](int end) {
#pragma unroll
        for (int r = 0; r < kRing; r++) {
            const int pos = end - 1 - (r * 64 + lane);
            ue[r] = pos >= 0 ? upos[range.x + pos] : 0u;
        }
#pragma unroll
        for (int r = 0; r < kRing; r++) {
            const int pos = end - 1 - (r * 64 + lane);
            ug[r] = pos >= 0 ? gid_by_e[ue[r]] : 0u;
        }
        ids_left = kRing;
    };
    __shared__ RawLDS s_raw;
    uint32_t unxt = 0;  // where this lane's splat record goes (the instance's emission slot)
    uint32_t rnxt = 0;  // its half-reach bits
    auto fetch = [&](int end) {  // ids of the batch ending at `end`, then its attribute loads
        if (ids_left == 0) refill(end);
        unxt = ue[0];
        const uint32_t ge = ug[0];
        rnxt = ge >> kReachShift;
#pragma unroll
        for (int r = 0; r + 1 < kRing; r++) {
            ue[r] = ue[r + 1];
            ug[r] = ug[r + 1];
        }
        ids_left--;
        issue_raw_lds(s_raw, lane < min(64, end), ge & kGidMask, splat);
    };
    if (max_last > 0) fetch((int)max_last);
    for (int end = (int)max_last; end > 0; end -= 64) {
        const int n = min(64, end);
        const uint32_t ucur = unxt;
        const uint64_t reach[2] = {ballot(lane < n && (rnxt & 1u)), ballot(lane < n && (rnxt & 2u))};
        SplatRegs nxt;
        read_raw_lds(nxt, s_raw, lane, lane < n, yc, true);  // my - yc, as the forward stages it
        // per-splat wave masks (the staged zero splats past n are neither)
        const uint64_t nonpd = ballot(lane < n && !conic_pd(nxt.geo, nxt.opc));
        const uint64_t hiop = ballot(lane < n && nxt.opc.z < kInvCapFree);
        __syncthreads();
        s_sp[lane].geo = nxt.geo;
        s_sp[lane].opc = nxt.opc;
        s_sp[lane].col = nxt.col;
        __syncthreads();
        if (end - 64 > 0) fetch(end - 64);
        // Splats in pairs, each pair one branch-free block over the (splat, half) steps it needs: the
        // falloffs are independent and only the short T / A updates chain, which gives the scheduler up
        // to four chains to interleave.  M0 / M1 = the splats (bit 0: j, bit 1: j + 1) walked on half 0 /
        // half 1: the halves each splat reaches in the common case, all four otherwise (a half a splat
        // does not reach has alpha < 1/255 at every pixel, so walking it changes nothing).  An odd
        // batch's last splat pairs with the zero splat staged past it (opacity 0: an exact no-op).  The
        // two splats' sums share one reduce-scatter.
        auto walk_pair = [&](int j, auto all, auto gen, auto m0, auto m1) {
            constexpr bool ALL = decltype(all)::value, GEN = decltype(gen)::value;
            constexpr int M[2] = {decltype(m0)::value, decltype(m1)::value};
            SplatPart part[2];
            float dxs[2], pa[2], pb[2];
            float4 geo[2], opc[2], col[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                geo[i] = s_sp[j + i].geo; opc[i] = s_sp[j + i].opc; col[i] = s_sp[j + i].col;
                dxs[i] = geo[i].x - pfx;
                pa[i] = fmaf(geo[i].z * dxs[i], dxs[i], opc[i].y);  // forward: fmaf(geo.z dx, dx, lo), geo.w dx
                pb[i] = geo[i].w * dxs[i];
            }
            f2 U[2][NU];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int k = 0; k < NU; k++) U[i][k] = bc2(0.f);
            SplatOps so[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                so[i] = SplatOps{bc2(geo[i].y), bc2(opc[i].x), bc2(opc[i].w), bc2(col[i].x), bc2(col[i].y),
                                 bc2(col[i].z), bc2(col[i].w), bc2(pa[i]), bc2(pb[i]), ((nonpd >> (j + i)) & 1) != 0,
                                 (uint32_t)(end - 1 - (j + i)),
                                 AbsOps{bc2(2.f * geo[i].z * dxs[i]), bc2(geo[i].w), bc2(2.f * opc[i].x)}};
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (M[h] == 3)
                    half_pair_step<ALL, GEN, DEPTH, ABS>(st.T[h], st.A[h], st.dp0[h], st.dp1[h], st.dp2[h], st.dd[h],
                                                         so[0], so[1], yl[h], yl2[h], lastc[2 * h], lastc[2 * h + 1],
                                                         U[0], U[1]);
                else if (M[h] != 0)
                    half_step<ALL, GEN, DEPTH, ABS>(st.T[h], st.A[h], st.dp0[h], st.dp1[h], st.dp2[h], st.dd[h],
                                                    so[M[h] >> 1], yl[h], yl2[h], lastc[2 * h], lastc[2 * h + 1],
                                                    U[M[h] >> 1]);
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
                part[i] = SplatPart{hsum(U[i][0]), hsum(U[i][1]), hsum(U[i][2]), hsum(U[i][3]), hsum(U[i][4]),
                                    hsum(U[i][5])};
            wave_sum_pair_to_lds<DEPTH, ABS>(part[0], part[1], dxs[0], dxs[1], DEPTH ? hsum(U[0][6]) : 0.f,
                                             DEPTH ? hsum(U[1][6]) : 0.f, ABS ? hsum(U[0][NU - 2]) : 0.f,
                                             ABS ? hsum(U[0][NU - 1]) : 0.f, ABS ? hsum(U[1][NU - 2]) : 0.f,
                                             ABS ? hsum(U[1][NU - 1]) : 0.f, s_col,
                                             reinterpret_cast<float *>(s_rec[j]), lane, roff);
        };
        using I3 = std::integral_constant<int, 3>;
        auto walk_batch = [&](auto all) {
            for (int j = 0; j < n; j += 2) {
                if (((nonpd | hiop) >> j) & 3) {
                    walk_pair(j, all, std::true_type{}, I3{}, I3{});
                } else {
                    const uint32_t combo = (uint32_t)((reach[0] >> j) & 3u) | (uint32_t)(((reach[1] >> j) & 3u) << 2);
                    auto go = [&](auto c) {
                        constexpr int C = decltype(c)::value;
                        walk_pair(j, all, std::false_type{}, std::integral_constant<int, C & 3>{},
                                  std::integral_constant<int, (C >> 2)>{});
                    };
                    switch (combo) {
                    case 1: go(std::integral_constant<int, 1>{}); break;
                    case 2: go(std::integral_constant<int, 2>{}); break;
                    case 3: go(std::integral_constant<int, 3>{}); break;
                    case 4: go(std::integral_constant<int, 4>{}); break;
                    case 5: go(std::integral_constant<int, 5>{}); break;
                    case 6: go(std::integral_constant<int, 6>{}); break;
                    case 7: go(std::integral_constant<int, 7>{}); break;
                    case 8: go(std::integral_constant<int, 8>{}); break;
                    case 9: go(std::integral_constant<int, 9>{}); break;
                    case 10: go(std::integral_constant<int, 10>{}); break;
                    case 11: go(std::integral_constant<int, 11>{}); break;
                    case 12: go(std::integral_constant<int, 12>{}); break;
                    case 13: go(std::integral_constant<int, 13>{}); break;
                    case 14: go(std::integral_constant<int, 14>{}); break;
                    default: go(std::integral_constant<int, 15>{}); break;
                    }
                }
            }
        };
        // batches wholly below every inside pixel's n_contrib: the contributor test passes everywhere
        if ((uint32_t)(end - 1) < min_last) walk_batch(std::true_type{});
        else walk_batch(std::false_type{});
        __syncthreads();
        if (lane < n) {
            // lane j writes splat j's record, its y moments moved from the tile centre to the splat's
            // centre row: dy = my_l - yl (backward.cu:545-551 moments of dy)
            const float4 r0 = s_rec[lane][0], r1 = s_rec[lane][1], r2 = s_rec[lane][2];
            const float my_l = s_sp[lane].geo.y;  // this lane's splat, my - yc
            const float io = s_sp[lane].opc.z;    // 1 / o: the moments were taken on u' = o u
            // r0 = (S u, S dx u, S u yl, S dx^2 u), r1 = (S dx u yl, S u yl^2, W0, W1),
            // r2 = (W2, W3 or -, S |u fx| or -, S |u fy| or -)
            const float s_u = r0.x, s_uyl = r0.z;
            const float v2 = my_l * s_u - s_uyl;                 // S u dy
            const float v4 = my_l * r0.y - r1.x;                 // S dx u dy
            const float v5 = my_l * v2 - (my_l * s_uyl - r1.y);  // S u dy^2
            float4 *rec = reinterpret_cast<float4 *>(contrib + (size_t)ucur * kContribStride);
            rec[0] = make_float4(s_u * io, r0.y * io, v2 * io, r0.w * io);
            rec[1] = make_float4(v4 * io, v5 * io, r1.z, r1.w);
            rec[2] = ABS ? make_float4(r2.x, r2.y, r2.z * io, r2.w * io) : r2;  // the absolute sums are u' sums too
        }
    }
}

// dL_ddepth (H x W, or NULL for none) selects the walk with dL/ddepth, whose records also carry W3 in float 9; abs
// the absgrad walk, whose records also carry the absolute sums in floats 10 and 11; dL_dalpha (H x W, or NULL for
// none): the alpha image's gradient.  The splat records hold the colours the forward blended (colors_precomp or SH).
hipError_t launch_render_backward(const Args &a, GeomState g, const uint32_t *gid_by_e, const uint32_t *upos,
                                  ImageState img, const float *dL_dpix, const float *dL_ddepth,
                                  const float *dL_dalpha, bool abs, float *contrib, hipStream_t s) {
    const int T = a.gx * a.gy;
    return with_backward_variant(dL_ddepth != nullptr, abs, [&](auto depth_c, auto abs_c) {
        hipLaunchKernelGGL((render_backward_kernel<depth_c.value, abs_c.value>), dim3(T), dim3(64), 0, s, a, img.ranges,
                           img.order, gid_by_e, upos, g.splat, img.final_T, img.n_contrib, dL_dpix, dL_ddepth, dL_dalpha,
                           contrib);
        return hipGetLastError();
    });
}

// how many of an instantiation's single-wave workgroups the runtime keeps resident on one CU (registers and LDS):
// 4 waves per SIMD are 16, the absgrad instantiations' 3 are 12
hipError_t render_backward_occupancy(bool depth, bool abs, int *workgroups_per_cu) {
    return with_backward_variant(depth, abs, [&](auto depth_c, auto abs_c) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(
            workgroups_per_cu, render_backward_kernel<depth_c.value, abs_c.value>, 64, 0);
    });
}

// gs4d_alpha_image: the accumulated alpha A = sum alpha_i T_i = 1 - T_final of every pixel, from the final_T the
// forward stored (forward.cu:373; tiles with an empty list included, T = 1).  One streaming pass: n = W * H.
__global__ __launch_bounds__(256) void alpha_image_kernel(size_t n, const float *__restrict__ final_T,
                                                          float *__restrict__ out_alpha) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out_alpha[i] = 1.f - final_T[i];
}
hipError_t launch_alpha_image(ImageState img, size_t n, float *out_alpha, hipStream_t s) {
    hipLaunchKernelGGL(alpha_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, img.final_T,
                       out_alpha);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// gs4d_importance: the blend weight w = alpha T every (pixel, splat) pair of a finished forward deposited
// (forward.cu:357-358), reduced per Gaussian to its sum, its maximum and the number of pixels it reached.
//
// The walk replays render_forward_kernel's over the lists the forward left sorted (upos holds the sorted
// emission slots, so nothing is sorted here): the same batches of 64 from the run's start, the same per-batch
// choice of the falloff<CAP, FOLD> instantiation, the same rule sequence and the same recurrence of T, so every
// w is the forward's to the bit.  No colour is read.  ONE wave per tile, as the backward has it: a lane holds its
// column's pixel pair of half tile 0 and of half tile 1, each half skipped for a splat that does not reach it
// (the forward's wave of that half never saw it) and carrying w = 0 once its pixels are retired (the forward's
// wave had stopped).  Per splat the lane adds its four pixels as (w00 + w01) + (w10 + w11), the wave reduces the 64
// lane values with a fixed DPP tree (quad, quad, half row, row, then row_bcast:15 and :31 -- lane 63 ends with
// ((r3 + r2) + (r0 + r1)) of the row sums), the maximum takes the same tree and the count is four ballot
// popcounts.  Lane 63 leaves (sum, max, count, 0) in the batch's LDS record array and the batch's lanes store
// their splats' records at their emission slots: 16 bytes per slot, zeros for a splat not walked (its half bits
// and the early exit), so every slot below L' is written and nothing is cleared beforehand.
template <int CTRL, int RM = 0xF>
__device__ __forceinline__ float dpp_rows(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, RM, 0xF, false));
}
// lane 63 of the result holds the wave's total in the fixed order stated above (other lanes: partial values)
__device__ __forceinline__ float wave_sum_lane63(float v) {
    v = __fadd_rn(v, dpp_rows<0xB1>(v));        // quad_perm [1, 0, 3, 2]
    v = __fadd_rn(v, dpp_rows<0x4E>(v));        // quad_perm [2, 3, 0, 1]
    v = __fadd_rn(v, dpp_rows<0x141>(v));       // row_half_mirror
    v = __fadd_rn(v, dpp_rows<0x140>(v));       // row_mirror: every lane holds its row's sum
    v = __fadd_rn(v, dpp_rows<0x142, 0xA>(v));  // row_bcast:15 -> rows 1, 3 (other rows add 0)
    v = __fadd_rn(v, dpp_rows<0x143, 0xC>(v));  // row_bcast:31 -> rows 2, 3
    return v;
}
// the same tree with max; the values are weights (>= 0), so the 0 a disabled row reads is the identity
__device__ __forceinline__ float wave_max_lane63(float v) {
    v = fmaxf(v, dpp_rows<0xB1>(v));
    v = fmaxf(v, dpp_rows<0x4E>(v));
    v = fmaxf(v, dpp_rows<0x141>(v));
    v = fmaxf(v, dpp_rows<0x140>(v));
    v = fmaxf(v, dpp_rows<0x142, 0xA>(v));
    v = fmaxf(v, dpp_rows<0x143, 0xC>(v));
    return v;
}

__global__ __launch_bounds__(64) void importance_walk_kernel(Args a, const uint2 *__restrict__ ranges,
                                                             const uint32_t *__restrict__ order,
                                                             const uint32_t *__restrict__ upos,
                                                             const uint32_t *__restrict__ gid_by_e,
                                                             const float4 *__restrict__ splat,
                                                             float4 *__restrict__ rec) {
    __shared__ SplatLDS s_sp[64];
    __shared__ RawLDS s_raw;
    __shared__ float4 s_rec[64];
    const int tile = (int)__builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int lane = threadIdx.x;
    const int px = tx * kBlockX + (lane & 15);
    const int py0 = ty * kBlockY + (lane >> 4);  // rows py0, py0 + 4 (half 0), py0 + 8, py0 + 12 (half 1)
    const float pfx = (float)px;
    const float yc = (float)(ty * kBlockY) + 7.5f;
    const float ylane = (float)(lane >> 4) - 7.5f;
    const f2 yl0 = f2{ylane, ylane + 4.f}, yl1 = f2{ylane + 8.f, ylane + 12.f};
    // the forward's per-lane alpha threshold: 1/255 while the pixel blends, 2 once it is outside or retired
    const bool xin = px < a.W;
    f2 thr0 = f2{(xin && py0 < a.H) ? kAlphaMin : 2.f, (xin && py0 + 4 < a.H) ? kAlphaMin : 2.f};
    f2 thr1 = f2{(xin && py0 + 8 < a.H) ? kAlphaMin : 2.f, (xin && py0 + 12 < a.H) ? kAlphaMin : 2.f};
    f2 T0 = bc2(1.f), T1 = bc2(1.f);
    uint2 range = ranges[tile];
    range.x = __builtin_amdgcn_readfirstlane(range.x);
    range.y = __builtin_amdgcn_readfirstlane(range.y);
    // list position first + lane: its emission slot, and that slot's Gaussian id | reach bits.  The slots are
    // loaded three batches ahead and the ids two, so that no load of an iteration waits for another of the same
    // iteration; the splat records of the next batch are gathered (LDS-DMA) under the current batch's walk.
    auto load_slot = [&](uint32_t first) { return first + lane < range.y ? upos[first + lane] : 0u; };
    auto load_gid = [&](uint32_t first, uint32_t e) { return first + lane < range.y ? gid_by_e[e] : 0u; };
    uint32_t e0 = 0, e1 = 0, e2 = 0, g0 = 0, g1 = 0;
    if (range.x < range.y) {
        e0 = load_slot(range.x);
        g0 = load_gid(range.x, e0);
        issue_raw_lds(s_raw, range.x + lane < range.y, g0 & kGidMask, splat);
        e1 = load_slot(range.x + 64);
        g1 = load_gid(range.x + 64, e1);
        e2 = load_slot(range.x + 128);
    }
    uint32_t base = range.x;
    for (; base < range.y; base += 64) {
        // forward.cu:312-314, both halves (a half that is done alone carries w = 0 from here on)
        if (ballot(thr0.x < 1.f || thr0.y < 1.f || thr1.x < 1.f || thr1.y < 1.f) == 0) break;
        SplatRegs nxt;
        const bool valid = base + lane < range.y;
        read_raw_lds(nxt, s_raw, lane, valid, yc, false);
        const uint64_t reach0 = ballot(valid && ((g0 >> kReachShift) & 1u));
        const uint64_t reach1 = ballot(valid && ((g0 >> (kReachShift + 1)) & 1u));
        // the forward's per-batch masks, over the whole batch whatever half a splat reaches
        const uint64_t nonpd = ballot(valid && !conic_pd(nxt.geo, nxt.opc));
        const bool cap = ballot(valid && nxt.opc.z < kInvCapFree) != 0;
        __builtin_amdgcn_wave_barrier();
        s_sp[lane].geo = nxt.geo;
        s_sp[lane].opc = nxt.opc;
        s_rec[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
        __builtin_amdgcn_wave_barrier();
        if (base + 64 < range.y) issue_raw_lds(s_raw, base + 64 + lane < range.y, g1 & kGidMask, splat);
        const uint32_t g2 = load_gid(base + 128, e2);
        const uint32_t e3 = load_slot(base + 192);
        // one half of one splat: the forward's blend() without the colour, returning w
        auto blend = [&](f2 &T, f2 &thr, const Falloff &f, uint32_t j, auto pwc) {
            bool k0 = f.alpha.x >= thr.x, k1 = f.alpha.y >= thr.y;  // forward.cu:346-348 (live pixels)
            if (decltype(pwc)::value && ((nonpd >> j) & 1)) {      // forward.cu:341-342
                k0 = k0 && f.pw.x <= 0.0f;
                k1 = k1 && f.pw.y <= 0.0f;
            }
            f2 ae = f2{k0 ? f.alpha.x : 0.f, k1 ? f.alpha.y : 0.f};
            f2 tT = T * (bc2(1.f) - ae);  // forward.cu:349
            if (ballot(fminf(tT.x, tT.y) < 0.0001f) != 0) {
                // forward.cu:350-354: not blended, the pixel retires
                const bool t0 = tT.x < 0.0001f, t1 = tT.y < 0.0001f;
                ae = f2{t0 ? 0.f : ae.x, t1 ? 0.f : ae.y};
                tT = f2{t0 ? T.x : tT.x, t1 ? T.y : tT.y};
                thr = f2{t0 ? 2.f : thr.x, t1 ? 2.f : thr.y};
            }
            const f2 w = ae * T;  // forward.cu:357-358
            T = tT;
            return w;
        };
        auto walk = [&](auto capc, auto pwc) {
            constexpr bool CAP = decltype(capc)::value, FOLD = !decltype(pwc)::value;
            for (uint64_t todo = reach0 | reach1; todo != 0; todo &= todo - 1) {
                const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                const float4 geo = s_sp[j].geo, opc = s_sp[j].opc;
                const float dx = geo.x - pfx;
                const float pa = fmaf(geo.z * dx, dx, opc.y), pb = geo.w * dx;
                f2 w0 = bc2(0.f), w1 = bc2(0.f);
                if ((reach0 >> j) & 1) w0 = blend(T0, thr0, falloff<CAP, FOLD>(geo, opc, pa, pb, yl0), j, pwc);
                if ((reach1 >> j) & 1) w1 = blend(T1, thr1, falloff<CAP, FOLD>(geo, opc, pa, pb, yl1), j, pwc);
                const float ls = __fadd_rn(__fadd_rn(w0.x, w0.y), __fadd_rn(w1.x, w1.y));
                const float lm = fmaxf(fmaxf(w0.x, w0.y), fmaxf(w1.x, w1.y));
                const uint32_t cnt = (uint32_t)(__builtin_popcountll(ballot(w0.x > 0.f)) +
                                                __builtin_popcountll(ballot(w0.y > 0.f)) +
                                                __builtin_popcountll(ballot(w1.x > 0.f)) +
                                                __builtin_popcountll(ballot(w1.y > 0.f)));
                const float ws = wave_sum_lane63(ls), wm = wave_max_lane63(lm);
                if (lane == 63) s_rec[j] = make_float4(ws, wm, __uint_as_float(cnt), 0.f);
            }
        };
        if (nonpd != 0) walk(std::true_type{}, std::true_type{});
        else if (cap) walk(std::true_type{}, std::false_type{});
        else walk(std::false_type{}, std::false_type{});
        __builtin_amdgcn_wave_barrier();
        if (valid) rec[e0] = s_rec[lane];
        e0 = e1; e1 = e2; e2 = e3;
        g0 = g1; g1 = g2;
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);  // an early exit may leave the next batch's LDS-DMA loads in flight
    // the splats behind the exit blended nowhere
    for (uint32_t i = base + lane; i < range.y; i += 64) rec[upos[i]] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The per-Gaussian pass, as contrib_segments_kernel (preprocess_backward.hip) has it with (add, max, add) for the
// operators: one lane per emission slot, a segmented inclusive scan over the wave's 64 slots by DPP moves, a
// Gaussian's consecutive slots being one segment.  A segment that is a whole Gaussian is written out; a piece
// continuing from the previous wave goes to part[w][0], one that starts a Gaussian and continues into the next
// wave to part[w][1]; e_first[g] = the Gaussian's first slot.
struct ImpAcc {
    float sum, mx;
    uint32_t cnt;
};
template <int CTRL, int RM>
__device__ __forceinline__ void imp_scan_step(ImpAcc &v, bool &f) {
    const bool fu = __builtin_amdgcn_update_dpp(0, (int)f, CTRL, RM, 0xF, false) != 0;
    const float us = dpp_rows<CTRL, RM>(v.sum), um = dpp_rows<CTRL, RM>(v.mx);
    const uint32_t uc = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.cnt, CTRL, RM, 0xF, false);
    if (!f) {
        v.sum = __fadd_rn(v.sum, us);
        v.mx = fmaxf(v.mx, um);
        v.cnt += uc;
    }
    f = f || fu;
}
__global__ __launch_bounds__(256) void importance_segments_kernel(const uint32_t *__restrict__ n_dev,
                                                                  const uint32_t *__restrict__ gid_by_e,
                                                                  const float4 *__restrict__ rec,
                                                                  float *__restrict__ weight_sum,
                                                                  float *__restrict__ weight_max,
                                                                  int32_t *__restrict__ pixel_count,
                                                                  float4 *__restrict__ part,
                                                                  uint32_t *__restrict__ e_first) {
    const int n = (int)__builtin_amdgcn_readfirstlane(*n_dev);
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w * 64 >= n) return;
    const int e = w * 64 + lane;
    const bool valid = e < n;
    const uint32_t key = valid ? gid_by_e[e] & kGidMask : 0xFFFFFFFFu;
    const float4 r = valid ? rec[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    ImpAcc v{r.x, r.y, __float_as_uint(r.z)};
    uint32_t kp = __shfl_up(key, 1), kn = __shfl_down(key, 1);
    if (lane == 0) kp = e > 0 ? gid_by_e[e - 1] & kGidMask : 0xFFFFFFFFu;
    if (lane == 63) kn = e + 1 < n ? gid_by_e[e + 1] & kGidMask : 0xFFFFFFFFu;
    const bool head = valid && key != kp;
    const bool tail = valid && key != kn;
    if (head) e_first[key] = (uint32_t)e;
    bool f = head || lane == 0;
    imp_scan_step<0x111, 0xF>(v, f);  // row_shr:1
    imp_scan_step<0x112, 0xF>(v, f);  // row_shr:2
    imp_scan_step<0x114, 0xF>(v, f);  // row_shr:4
    imp_scan_step<0x118, 0xF>(v, f);  // row_shr:8
    imp_scan_step<0x142, 0xA>(v, f);  // row_bcast:15 -> rows 1, 3
    imp_scan_step<0x143, 0xC>(v, f);  // row_bcast:31 -> rows 2, 3
    const uint64_t endm = __ballot(valid && (tail || lane == 63));
    const int fe = __ffsll((unsigned long long)endm) - 1;  // end lane of the first piece
    const bool head0 = __ballot(head) & 1ull;
    if (valid && (tail || lane == 63)) {
        const bool starts = lane != fe || head0;  // the piece starts at its Gaussian's first slot
        if (starts && tail) {
            weight_sum[key] = v.sum;
            weight_max[key] = v.mx;
            pixel_count[key] = (int32_t)v.cnt;
        } else {
            part[(size_t)w * 2 + (starts ? 1 : 0)] = make_float4(v.sum, v.mx, __uint_as_float(v.cnt), 0.f);
        }
    }
}
// One thread per Gaussian: zeros without slots; the pieces of a Gaussian whose slots span waves in wave order,
// part[w0][1] then part[w][0] of each following wave up to the one holding its last slot.
__global__ __launch_bounds__(256) void importance_finish_kernel(int P, const uint32_t *__restrict__ n_inst,
                                                                const uint32_t *__restrict__ e_first,
                                                                const float4 *__restrict__ part,
                                                                float *__restrict__ weight_sum,
                                                                float *__restrict__ weight_max,
                                                                int32_t *__restrict__ pixel_count) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const uint32_t ni = n_inst[idx];
    if (ni == 0) {
        weight_sum[idx] = 0.f;
        weight_max[idx] = 0.f;
        pixel_count[idx] = 0;
        return;
    }
    const uint32_t e0 = e_first[idx], w0 = e0 >> 6, w1 = (e0 + ni - 1) >> 6;
    if (w0 == w1) return;  // the segments kernel wrote it
    float4 p = part[(size_t)w0 * 2 + 1];
    float sum = p.x, mx = p.y;
    uint32_t cnt = __float_as_uint(p.z);
    for (uint32_t w = w0 + 1; w <= w1; w++) {
        p = part[(size_t)w * 2];
        sum = __fadd_rn(sum, p.x);
        mx = fmaxf(mx, p.y);
        cnt += __float_as_uint(p.z);
    }
    weight_sum[idx] = sum;
    weight_max[idx] = mx;
    pixel_count[idx] = (int32_t)cnt;
}

// scratch: R records | 2 partial records per wave of 64 slots | e_first (P)
size_t importance_scratch_bytes(int R, int P) {
    const size_t nw = ((size_t)R + 63) / 64;
    return align_up((size_t)R * sizeof(float4), 256) + align_up(nw * 2 * sizeof(float4), 256) +
           align_up(4 * (size_t)P, 256) + 256;
}
hipError_t launch_importance(const Args &a, GeomState g, BinningState b, ImageState img, int R, char *scratch,
                             float *weight_sum, float *weight_max, int32_t *pixel_count, hipStream_t s) {
    const size_t nw = ((size_t)R + 63) / 64;
    float4 *rec = (float4 *)align_up((size_t)scratch, 256);
    float4 *part = (float4 *)((char *)rec + align_up((size_t)R * sizeof(float4), 256));
    uint32_t *e_first = (uint32_t *)((char *)part + align_up(nw * 2 * sizeof(float4), 256));
    hipLaunchKernelGGL(importance_walk_kernel, dim3(a.gx * a.gy), dim3(64), 0, s, a, img.ranges, img.order, b.upos,
                       b.gid_by_e, g.splat, rec);
    hipLaunchKernelGGL(importance_segments_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, b.scratch,
                       b.gid_by_e, rec, weight_sum, weight_max, pixel_count, part, e_first);
    hipLaunchKernelGGL(importance_finish_kernel, dim3((a.P + 255) / 256), dim3(256), 0, s, a.P, g.n_inst, e_first,
                       part, weight_sum, weight_max, pixel_count);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// gs4d_features_forward / gs4d_features_backward: a caller's per-Gaussian feature rows f (P x C) blended with the
// weights w = alpha T of a finished forward, F_c(p) = sum_i w_ip f_ic, and that image's gradient.
//
// Forward: importance_walk_kernel's replay (same batches, falloff<CAP, FOLD> choice, rule sequence and recurrence
// of T, so every w is the forward's to the bit) with kFeatureChunk accumulators per pixel, each updated as the
// forward updates a colour channel, acc = fma(f, w, acc) in list order: a channel is bit for bit what the forward
// blends for that colour over a zero background.  Chunks of kFeatureChunk channels are the grid's y dimension;
// the rows are read in place (channels past C read as 0 and are not stored), so the pass takes no scratch.  A
// batch's feature rows sit in LDS beside its splat records (lane l stages its splat's chunk, loaded one batch
// ahead); the walk reads them wave-uniformly.
constexpr int kFeatureChunk = 8;
struct FeatRow {
    float4 lo, hi;  // channels 0..3 and 4..7 of the chunk
};
static_assert(kFeatureChunk == 8, "FeatRow holds two float4");
__device__ __forceinline__ void load_feat_row(float (&f)[kFeatureChunk], bool valid, uint32_t gid, int C, int c0,
                                              const float *__restrict__ features) {
#pragma unroll
    for (int k = 0; k < kFeatureChunk; k++)
        f[k] = (valid && c0 + k < C) ? features[(size_t)gid * C + c0 + k] : 0.f;
}

__global__ __launch_bounds__(64) void feature_walk_kernel(Args a, int C, const uint2 *__restrict__ ranges,
                                                          const uint32_t *__restrict__ order,
                                                          const uint32_t *__restrict__ upos,
                                                          const uint32_t *__restrict__ gid_by_e,
                                                          const float4 *__restrict__ splat,
                                                          const float *__restrict__ features,
                                                          float *__restrict__ out) {
    constexpr int K = kFeatureChunk;
    __shared__ SplatLDS s_sp[64];
    __shared__ RawLDS s_raw;
    __shared__ FeatRow s_feat[64];
    const int c0 = (int)blockIdx.y * K;
    const int tile = (int)__builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int lane = threadIdx.x;
    const int px = tx * kBlockX + (lane & 15);
    const int py0 = ty * kBlockY + (lane >> 4);  // rows py0, py0 + 4 (half 0), py0 + 8, py0 + 12 (half 1)
    const float pfx = (float)px;
    const float yc = (float)(ty * kBlockY) + 7.5f;
    const float ylane = (float)(lane >> 4) - 7.5f;
    const f2 yl0 = f2{ylane, ylane + 4.f}, yl1 = f2{ylane + 8.f, ylane + 12.f};
    const bool xin = px < a.W;
    f2 thr0 = f2{(xin && py0 < a.H) ? kAlphaMin : 2.f, (xin && py0 + 4 < a.H) ? kAlphaMin : 2.f};
    f2 thr1 = f2{(xin && py0 + 8 < a.H) ? kAlphaMin : 2.f, (xin && py0 + 12 < a.H) ? kAlphaMin : 2.f};
    f2 T0 = bc2(1.f), T1 = bc2(1.f);
    f2 acc0[K], acc1[K];
#pragma unroll
    for (int k = 0; k < K; k++) acc0[k] = acc1[k] = bc2(0.f);
    uint2 range = ranges[tile];
    range.x = __builtin_amdgcn_readfirstlane(range.x);
    range.y = __builtin_amdgcn_readfirstlane(range.y);
    auto load_slot = [&](uint32_t first) { return first + lane < range.y ? upos[first + lane] : 0u; };
    auto load_gid = [&](uint32_t first, uint32_t e) { return first + lane < range.y ? gid_by_e[e] : 0u; };
    uint32_t e1 = 0, e2 = 0, g0 = 0, g1 = 0;
    float fcur[K], fnxt[K];
#pragma unroll
    for (int k = 0; k < K; k++) fcur[k] = fnxt[k] = 0.f;
    if (range.x < range.y) {
        const uint32_t e0 = load_slot(range.x);
        g0 = load_gid(range.x, e0);
        issue_raw_lds(s_raw, range.x + lane < range.y, g0 & kGidMask, splat);
        load_feat_row(fcur, range.x + lane < range.y, g0 & kGidMask, C, c0, features);
        e1 = load_slot(range.x + 64);
        g1 = load_gid(range.x + 64, e1);
        e2 = load_slot(range.x + 128);
    }
    for (uint32_t base = range.x; base < range.y; base += 64) {
        // forward.cu:312-314, both halves (a half that is done alone carries w = 0 from here on)
        if (ballot(thr0.x < 1.f || thr0.y < 1.f || thr1.x < 1.f || thr1.y < 1.f) == 0) break;
        SplatRegs nxt;
        const bool valid = base + lane < range.y;
        read_raw_lds(nxt, s_raw, lane, valid, yc, false);
        const uint64_t reach0 = ballot(valid && ((g0 >> kReachShift) & 1u));
        const uint64_t reach1 = ballot(valid && ((g0 >> (kReachShift + 1)) & 1u));
        // the forward's per-batch masks, over the whole batch whatever half a splat reaches
        const uint64_t nonpd = ballot(valid && !conic_pd(nxt.geo, nxt.opc));
        const bool cap = ballot(valid && nxt.opc.z < kInvCapFree) != 0;
        __builtin_amdgcn_wave_barrier();
        s_sp[lane].geo = nxt.geo;
        s_sp[lane].opc = nxt.opc;
        s_feat[lane].lo = make_float4(fcur[0], fcur[1], fcur[2], fcur[3]);
        s_feat[lane].hi = make_float4(fcur[4], fcur[5], fcur[6], fcur[7]);
        __builtin_amdgcn_wave_barrier();
        if (base + 64 < range.y) {
            issue_raw_lds(s_raw, base + 64 + lane < range.y, g1 & kGidMask, splat);
            load_feat_row(fnxt, base + 64 + lane < range.y, g1 & kGidMask, C, c0, features);
        }
        const uint32_t g2 = load_gid(base + 128, e2);
        const uint32_t e3 = load_slot(base + 192);
        // one half of one splat: the forward's blend() without the colour, returning w
        auto blend = [&](f2 &T, f2 &thr, const Falloff &f, uint32_t j, auto pwc) {
            bool k0 = f.alpha.x >= thr.x, k1 = f.alpha.y >= thr.y;  // forward.cu:346-348 (live pixels)
            if (decltype(pwc)::value && ((nonpd >> j) & 1)) {      // forward.cu:341-342
                k0 = k0 && f.pw.x <= 0.0f;
                k1 = k1 && f.pw.y <= 0.0f;
            }
            f2 ae = f2{k0 ? f.alpha.x : 0.f, k1 ? f.alpha.y : 0.f};
            f2 tT = T * (bc2(1.f) - ae);  // forward.cu:349
            if (ballot(fminf(tT.x, tT.y) < 0.0001f) != 0) {
                // forward.cu:350-354: not blended, the pixel retires
                const bool t0 = tT.x < 0.0001f, t1 = tT.y < 0.0001f;
                ae = f2{t0 ? 0.f : ae.x, t1 ? 0.f : ae.y};
                tT = f2{t0 ? T.x : tT.x, t1 ? T.y : tT.y};
                thr = f2{t0 ? 2.f : thr.x, t1 ? 2.f : thr.y};
            }
            const f2 w = ae * T;  // forward.cu:357-358
            T = tT;
            return w;
        };
        auto walk = [&](auto capc, auto pwc) {
            constexpr bool CAP = decltype(capc)::value, FOLD = !decltype(pwc)::value;
            for (uint64_t todo = reach0 | reach1; todo != 0; todo &= todo - 1) {
                const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                const float4 geo = s_sp[j].geo, opc = s_sp[j].opc;
                const float4 flo = s_feat[j].lo, fhi = s_feat[j].hi;
                const float fj[K] = {flo.x, flo.y, flo.z, flo.w, fhi.x, fhi.y, fhi.z, fhi.w};
                const float dx = geo.x - pfx;
                const float pa = fmaf(geo.z * dx, dx, opc.y), pb = geo.w * dx;
                if ((reach0 >> j) & 1) {
                    const f2 w = blend(T0, thr0, falloff<CAP, FOLD>(geo, opc, pa, pb, yl0), j, pwc);
#pragma unroll
                    for (int k = 0; k < K; k++) acc0[k] = fma2(bc2(fj[k]), w, acc0[k]);
                }
                if ((reach1 >> j) & 1) {
                    const f2 w = blend(T1, thr1, falloff<CAP, FOLD>(geo, opc, pa, pb, yl1), j, pwc);
#pragma unroll
                    for (int k = 0; k < K; k++) acc1[k] = fma2(bc2(fj[k]), w, acc1[k]);
                }
            }
        };
        if (nonpd != 0) walk(std::true_type{}, std::true_type{});
        else if (cap) walk(std::true_type{}, std::false_type{});
        else walk(std::false_type{}, std::false_type{});
        e1 = e2; e2 = e3;
        g0 = g1; g1 = g2;
#pragma unroll
        for (int k = 0; k < K; k++) fcur[k] = fnxt[k];
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);  // an early exit may leave the next batch's LDS-DMA loads in flight
    const size_t HW = (size_t)a.W * a.H;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int py = py0 + 4 * r;
        if (xin && py < a.H) {
            const size_t pix = (size_t)py * a.W + px;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const f2 v = r < 2 ? acc0[k] : acc1[k];
                if (c0 + k < C) out[(size_t)(c0 + k) * HW + pix] = (r & 1) ? v.y : v.x;
            }
        }
    }
}

hipError_t launch_features_forward(const Args &a, int C, GeomState g, BinningState b, ImageState img,
                                   const float *features, float *out_image, hipStream_t s) {
    const unsigned chunks = (unsigned)((C + kFeatureChunk - 1) / kFeatureChunk);
    hipLaunchKernelGGL(feature_walk_kernel, dim3(a.gx * a.gy, chunks), dim3(64), 0, s, a, C, img.ranges, img.order,
                       b.upos, b.gid_by_e, g.splat, features, out_image);
    return hipGetLastError();
}

// Backward of one chunk: render_backward_kernel's reverse walk with the chunk's K channels in the place of the three
// colours and no background layer -- T recovered backwards from final_T (backward.cu:503), the contributor test
// against n_contrib, the forward's alpha and power rules, A = accum_rec . dL/dF carried as one scalar per pixel
// (A = alpha CD + (1 - alpha) A with CD = f_i . dL/dF), dL/dalpha = T (CD - A), and the moments of u' = o G dL/dalpha
// (uncapped o G, as backward.cu:519-551 has it) that make the geometry record of the kContribStride layout, colour
// and depth fields zero.  One splat at a time over both halves; every splat takes the general path (0.99 cap, power
// test where its conic is not positive definite).  Per splat the 6 moments and the K sums W_k = sum_p w dL/dF_k(p)
// are reduced over the wave four at a time: lds_col_sum() over a column's four lanes, then the row's 16 columns by
// four DPP steps (fixed order, no atomics); lane j of the batch then writes splat j's two records at its emission
// slot.  GEOM = false (no geometry input requires grad): only the W_k are formed.  `accumulate` (chunks after the
// first): the geometry record is added to the one the earlier chunks left at the slot, so the chunks' terms are
// summed per instance in ascending chunk order; the K-float dL/df record is the chunk's alone.
template <bool GEOM>
__global__ __launch_bounds__(64) void feature_backward_kernel(Args a, int C, int c0, int accumulate,
                                                              const uint2 *__restrict__ ranges,
                                                              const uint32_t *__restrict__ order,
                                                              const uint32_t *__restrict__ gid_by_e,
                                                              const uint32_t *__restrict__ upos,
                                                              const float4 *__restrict__ splat,
                                                              const float *__restrict__ final_Ts,
                                                              const uint32_t *__restrict__ n_contrib,
                                                              const float *__restrict__ features,
                                                              const float *__restrict__ dL_dF,
                                                              float *__restrict__ contrib, float4 *__restrict__ frec) {
    constexpr int K = kFeatureChunk;
    constexpr int NV = (GEOM ? 6 : 0) + K, NR = (NV + 3) / 4;  // values reduced per splat, rounds of four
    __shared__ SplatLDS s_sp[64];
    __shared__ RawLDS s_raw;
    __shared__ FeatRow s_feat[64];
    __shared__ float s_red[64][4 * NR];
    __shared__ float s_col[kColSumWords];
    const int tile = (int)__builtin_amdgcn_readfirstlane(order[blockIdx.x]);
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int lane = threadIdx.x;
    const int px = tx * kBlockX + (lane & 15);
    const int py0 = ty * kBlockY + (lane >> 4);
    const float pfx = (float)px;
    const size_t HW = (size_t)a.W * a.H;
    uint2 range = ranges[tile];
    range.x = __builtin_amdgcn_readfirstlane(range.x);
    range.y = __builtin_amdgcn_readfirstlane(range.y);
    if (range.y <= range.x) return;
    const float ylane = (float)(lane >> 4) - 7.5f;
    const f2 yl[2] = {f2{ylane, ylane + 4.f}, f2{ylane + 8.f, ylane + 12.f}};
    const f2 yl2[2] = {yl[0] * yl[0], yl[1] * yl[1]};
    const float yc = (float)(ty * kBlockY) + 7.5f;

    f2 T[2], A[2] = {bc2(0.f), bc2(0.f)}, dF[2][K];
    uint32_t lastc[4];
    uint32_t max_last = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int py = py0 + 4 * r;
        const bool inside = px < a.W && py < a.H;
        const size_t pix = (size_t)py * a.W + px;
        const float tf = inside ? final_Ts[pix] : 0.f;
        lastc[r] = inside ? n_contrib[pix] : 0u;
        max_last = max(max_last, lastc[r]);
        if (r & 1) T[r >> 1].y = tf;
        else T[r >> 1].x = tf;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const float d = (inside && c0 + k < C) ? dL_dF[(size_t)(c0 + k) * HW + pix] : 0.f;
            if (r & 1) dF[r >> 1][k].y = d;
            else dF[r >> 1][k].x = d;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) max_last = max(max_last, (uint32_t)__shfl_xor((int)max_last, off));
    max_last = __builtin_amdgcn_readfirstlane(max_last);

    // splats at list position >= every pixel's n_contrib never contributed: zero records
    const uint32_t len = range.y - range.x;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t p = max_last + lane; p < len; p += 64) {
        const uint32_t e = upos[range.x + p];
        if (GEOM && !accumulate) {
            float4 *rec = reinterpret_cast<float4 *>(contrib + (size_t)e * kContribStride);
            rec[0] = z4;
            rec[1] = z4;
            rec[2] = z4;
        }
        frec[2 * (size_t)e] = z4;
        frec[2 * (size_t)e + 1] = z4;
    }
    for (int end = (int)max_last; end > 0; end -= 64) {
        const int n = min(64, end);
        // lane l holds list position end - 1 - l: the walk goes back to front
        const bool valid = lane < n;
        const uint32_t ecur = valid ? upos[range.x + (uint32_t)(end - 1 - lane)] : 0u;
        const uint32_t ge = valid ? gid_by_e[ecur] : 0u;
        issue_raw_lds(s_raw, valid, ge & kGidMask, splat);
        float fl[K];
        load_feat_row(fl, valid, ge & kGidMask, C, c0, features);
        const uint64_t reach[2] = {ballot(valid && ((ge >> kReachShift) & 1u)),
                                   ballot(valid && ((ge >> (kReachShift + 1)) & 1u))};
        SplatRegs nxt;
        read_raw_lds(nxt, s_raw, lane, valid, yc, false);  // my - yc, as the forward stages it
        const uint64_t nonpd = ballot(valid && !conic_pd(nxt.geo, nxt.opc));
        __builtin_amdgcn_wave_barrier();
        s_sp[lane].geo = nxt.geo;
        s_sp[lane].opc = nxt.opc;
        s_feat[lane].lo = make_float4(fl[0], fl[1], fl[2], fl[3]);
        s_feat[lane].hi = make_float4(fl[4], fl[5], fl[6], fl[7]);
#pragma unroll
        for (int q = 0; q < 4 * NR; q++) s_red[lane][q] = 0.f;  // a splat reaching neither half is not walked
        __builtin_amdgcn_wave_barrier();
        for (uint64_t todo = reach[0] | reach[1]; todo != 0; todo &= todo - 1) {
            const int j = __builtin_ctzll(todo);
            const float4 geo = s_sp[j].geo, opc = s_sp[j].opc;
            const float4 flo = s_feat[j].lo, fhi = s_feat[j].hi;
            const float fj[K] = {flo.x, flo.y, flo.z, flo.w, fhi.x, fhi.y, fhi.z, fhi.w};
            const float dx = geo.x - pfx;
            const float pa = fmaf(geo.z * dx, dx, opc.y), pb = geo.w * dx;  // the forward's operands
            const bool chk = (nonpd >> j) & 1;
            const uint32_t contributor = (uint32_t)(end - 1 - j);
            float lu0 = 0.f, lu1 = 0.f, lu2 = 0.f, Wk[K];
#pragma unroll
            for (int k = 0; k < K; k++) Wk[k] = 0.f;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (!((reach[h] >> j) & 1)) continue;  // alpha < 1/255 at every pixel of the half
                const Falloff f = falloff<true, false>(geo, opc, pa, pb, yl[h]);
                const f2 al = bc2(opc.w) * f.G;  // o G, the forward's product
                // backward.cu:486-497: the contributor test, alpha < 1/255 and power > 0 skip
                bool k0 = al.x >= kAlphaMin && contributor < lastc[2 * h];
                bool k1 = al.y >= kAlphaMin && contributor < lastc[2 * h + 1];
                if (chk) {
                    k0 = k0 && f.pw.x <= 0.0f;
                    k1 = k1 && f.pw.y <= 0.0f;
                }
                const f2 ale = f2{k0 ? al.x : 0.f, k1 ? al.y : 0.f};
                const f2 ae = f2{fminf(0.99f, ale.x), fminf(0.99f, ale.y)};
                const f2 om = bc2(1.f) - ae;
                const f2 Tn = T[h] * f2{__builtin_amdgcn_rcpf(om.x), __builtin_amdgcn_rcpf(om.y)};  // backward.cu:503
                T[h] = Tn;
                const f2 w = ae * Tn;
#pragma unroll
                for (int k = 0; k < K; k++) Wk[k] += hsum(w * dF[h][k]);
                if (GEOM) {
                    f2 diff = -A[h];
#pragma unroll
                    for (int k = 0; k < K; k++) diff = fma2(bc2(fj[k]), dF[h][k], diff);  // f . dL/dF - accum_rec . dL/dF
                    A[h] = fma2(ae, diff, A[h]);
                    const f2 u = (ale * Tn) * diff;  // o G dL/dalpha
                    lu0 += hsum(u);
                    lu1 += hsum(u * yl[h]);
                    lu2 += hsum(u * yl2[h]);
                }
            }
            float v[4 * NR];
#pragma unroll
            for (int q = 0; q < 4 * NR; q++) v[q] = 0.f;
            if (GEOM) {
                v[0] = lu0; v[1] = dx * lu0; v[2] = lu1; v[3] = dx * dx * lu0; v[4] = dx * lu1; v[5] = lu2;
            }
#pragma unroll
            for (int k = 0; k < K; k++) v[(GEOM ? 6 : 0) + k] = Wk[k];
#pragma unroll
            for (int r = 0; r < NR; r++) {
                // value 4 r + g summed over the wave, on every lane of row g
                float x = lds_col_sum(s_col, lane, v[4 * r], v[4 * r + 1], v[4 * r + 2], v[4 * r + 3]);
                x += dpp<0xB1>(x);   // quad_perm [1, 0, 3, 2]
                x += dpp<0x4E>(x);   // quad_perm [2, 3, 0, 1]
                x += dpp<0x141>(x);  // row_half_mirror
                x += dpp<0x140>(x);  // row_mirror
                if ((lane & 15) == 0) s_red[j][4 * r + (lane >> 4)] = x;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            float r[4 * NR];
#pragma unroll
            for (int q = 0; q < 4 * NR; q++) r[q] = s_red[lane][q];
            if (GEOM) {
                // the y moments moved from the tile's centre row to the splat's: dy = my_l - yl, and the division
                // by o (the moments were taken on u' = o u), as render_backward_kernel writes its record
                const float my_l = s_sp[lane].geo.y, io = s_sp[lane].opc.z;
                const float s_u = r[0], s_dxu = r[1], s_uyl = r[2], s_dx2u = r[3], s_dxuyl = r[4], s_uyl2 = r[5];
                const float v2 = my_l * s_u - s_uyl;                   // S u dy
                const float v4 = my_l * s_dxu - s_dxuyl;               // S dx u dy
                const float v5 = my_l * v2 - (my_l * s_uyl - s_uyl2);  // S u dy^2
                float4 r0 = make_float4(s_u * io, s_dxu * io, v2 * io, s_dx2u * io);
                float4 r1 = make_float4(v4 * io, v5 * io, 0.f, 0.f);
                float4 *rec = reinterpret_cast<float4 *>(contrib + (size_t)ecur * kContribStride);
                if (accumulate) {
                    const float4 p0 = rec[0], p1 = rec[1];
                    r0 = make_float4(p0.x + r0.x, p0.y + r0.y, p0.z + r0.z, p0.w + r0.w);
                    r1 = make_float4(p1.x + r1.x, p1.y + r1.y, 0.f, 0.f);
                }
                rec[0] = r0;
                rec[1] = r1;
                rec[2] = z4;
            }
            constexpr int o = GEOM ? 6 : 0;
            frec[2 * (size_t)ecur] = make_float4(r[o], r[o + 1], r[o + 2], r[o + 3]);
            frec[2 * (size_t)ecur + 1] = make_float4(r[o + 4], r[o + 5], r[o + 6], r[o + 7]);
        }
        __builtin_amdgcn_wave_barrier();  // the next batch restages s_sp / s_red
    }
}

// dL/df of one chunk per Gaussian: importance_segments_kernel / importance_finish_kernel with K adds for the
// operators.  One lane per emission slot, a segmented inclusive scan over the wave's 64 slots by DPP moves, a
// Gaussian's consecutive slots being one segment.  A segment that is a whole Gaussian is written out; a piece
// continuing from the previous wave goes to part[w][0], one that starts a Gaussian and continues into the next wave
// to part[w][1] (two float4 each); e_first[g] = the Gaussian's first slot.
template <int CTRL, int RM>
__device__ __forceinline__ void feat_scan_step(float (&v)[kFeatureChunk], bool &f) {
    const bool fu = __builtin_amdgcn_update_dpp(0, (int)f, CTRL, RM, 0xF, false) != 0;
    float up[kFeatureChunk];
#pragma unroll
    for (int k = 0; k < kFeatureChunk; k++) up[k] = dpp_rows<CTRL, RM>(v[k]);
    if (!f) {
#pragma unroll
        for (int k = 0; k < kFeatureChunk; k++) v[k] = __fadd_rn(v[k], up[k]);
    }
    f = f || fu;
}
__device__ __forceinline__ void store_feat_row(float *__restrict__ dL_df, uint32_t gid, int C, int c0,
                                               const float (&v)[kFeatureChunk]) {
#pragma unroll
    for (int k = 0; k < kFeatureChunk; k++)
        if (c0 + k < C) dL_df[(size_t)gid * C + c0 + k] = v[k];
}
__global__ __launch_bounds__(256) void feature_segments_kernel(const uint32_t *__restrict__ n_dev,
                                                               const uint32_t *__restrict__ gid_by_e,
                                                               const float4 *__restrict__ frec, int C, int c0,
                                                               float *__restrict__ dL_df, float4 *__restrict__ part,
                                                               uint32_t *__restrict__ e_first) {
    constexpr int K = kFeatureChunk;
    const int n = (int)__builtin_amdgcn_readfirstlane(*n_dev);
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w * 64 >= n) return;
    const int e = w * 64 + lane;
    const bool valid = e < n;
    const uint32_t key = valid ? gid_by_e[e] & kGidMask : 0xFFFFFFFFu;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 lo = valid ? frec[2 * (size_t)e] : z4, hi = valid ? frec[2 * (size_t)e + 1] : z4;
    float v[K] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t kp = __shfl_up(key, 1), kn = __shfl_down(key, 1);
    if (lane == 0) kp = e > 0 ? gid_by_e[e - 1] & kGidMask : 0xFFFFFFFFu;
    if (lane == 63) kn = e + 1 < n ? gid_by_e[e + 1] & kGidMask : 0xFFFFFFFFu;
    const bool head = valid && key != kp;
    const bool tail = valid && key != kn;
    if (head) e_first[key] = (uint32_t)e;
    bool f = head || lane == 0;
    feat_scan_step<0x111, 0xF>(v, f);  // row_shr:1
    feat_scan_step<0x112, 0xF>(v, f);  // row_shr:2
    feat_scan_step<0x114, 0xF>(v, f);  // row_shr:4
    feat_scan_step<0x118, 0xF>(v, f);  // row_shr:8
    feat_scan_step<0x142, 0xA>(v, f);  // row_bcast:15 -> rows 1, 3
    feat_scan_step<0x143, 0xC>(v, f);  // row_bcast:31 -> rows 2, 3
    const uint64_t endm = __ballot(valid && (tail || lane == 63));
    const int fe = __ffsll((unsigned long long)endm) - 1;  // end lane of the first piece
    const bool head0 = __ballot(head) & 1ull;
    if (valid && (tail || lane == 63)) {
        const bool starts = lane != fe || head0;  // the piece starts at its Gaussian's first slot
        if (starts && tail) {
            store_feat_row(dL_df, key, C, c0, v);
        } else {
            float4 *p = part + ((size_t)w * 2 + (starts ? 1 : 0)) * 2;
            p[0] = make_float4(v[0], v[1], v[2], v[3]);
            p[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
}
// One thread per Gaussian: zeros without slots; the pieces of a Gaussian whose slots span waves in wave order,
// part[w0][1] then part[w][0] of each following wave up to the one holding its last slot.
__global__ __launch_bounds__(256) void feature_finish_kernel(int P, const uint32_t *__restrict__ n_inst,
                                                             const uint32_t *__restrict__ e_first,
                                                             const float4 *__restrict__ part, int C, int c0,
                                                             float *__restrict__ dL_df) {
    constexpr int K = kFeatureChunk;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const uint32_t ni = n_inst[idx];
    float v[K] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ni != 0) {
        const uint32_t e0 = e_first[idx], w0 = e0 >> 6, w1 = (e0 + ni - 1) >> 6;
        if (w0 == w1) return;  // the segments kernel wrote it
        for (uint32_t w = w0; w <= w1; w++) {
            const float4 *p = part + ((size_t)w * 2 + (w == w0 ? 1 : 0)) * 2;
            const float4 l = p[0], h = p[1];
            const float a[K] = {l.x, l.y, l.z, l.w, h.x, h.y, h.z, h.w};
#pragma unroll
            for (int k = 0; k < K; k++) v[k] = w == w0 ? a[k] : __fadd_rn(v[k], a[k]);
        }
    }
    store_feat_row(dL_df, (uint32_t)idx, C, c0, v);
}

int feature_chunk() { return kFeatureChunk; }
// scratch of the dL/df reduce: R records | 2 partial records per wave of 64 slots | e_first (P)
static size_t feat_rec_bytes(int R) { return align_up((size_t)R * kFeatureChunk * sizeof(float), 256); }
static size_t feat_part_bytes(int R) {
    return align_up(((size_t)R + 63) / 64 * 2 * kFeatureChunk * sizeof(float), 256);
}
size_t features_scratch_bytes(int R, int P) {
    return feat_rec_bytes(R) + feat_part_bytes(R) + align_up(4 * (size_t)P, 256);
}
// contrib (R x kContribStride floats; NULL: no geometry gradient) and fscratch (features_scratch_bytes(R, P), 256-byte
// aligned) are the caller's scratch; every element of dL_df (P x C) is written.  R > 0.
hipError_t launch_features_backward(const Args &a, int C, int R, GeomState g, BinningState b, ImageState img,
                                    const float *features, const float *dL_dF, float *contrib, char *fscratch,
                                    float *dL_df, hipStream_t s) {
    const size_t nw = ((size_t)R + 63) / 64;
    float4 *frec = (float4 *)fscratch;
    float4 *part = (float4 *)(fscratch + feat_rec_bytes(R));
    uint32_t *e_first = (uint32_t *)((char *)part + feat_part_bytes(R));
    for (int c0 = 0; c0 < C; c0 += kFeatureChunk) {
        const auto kernel = contrib ? feature_backward_kernel<true> : feature_backward_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(a.gx * a.gy), dim3(64), 0, s, a, C, c0, c0 > 0 ? 1 : 0, img.ranges, img.order,
                           b.gid_by_e, b.upos, g.splat, img.final_T, img.n_contrib, features, dL_dF, contrib, frec);
        hipLaunchKernelGGL(feature_segments_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, b.scratch,
                           b.gid_by_e, (const float4 *)frec, C, c0, dL_df, part, e_first);
        hipLaunchKernelGGL(feature_finish_kernel, dim3((a.P + 255) / 256), dim3(256), 0, s, a.P, g.n_inst, e_first,
                           (const float4 *)part, C, c0, dL_df);
    }
    return hipGetLastError();
}

}  // namespace gs4d
