// train_internal.h -- the few things two or more of the train-step translation units share (train_tail.hip,
// ssim.hip, mlp_feature.hip, mlp_heads_forward.hip, mlp_heads_backward.hip, mlp_gemm.hip, deform_infer.hip): the MFMA fragment
// types and LDS tile addressing of the bf16 weight-gradient kernels, the CU count, and the last-workgroup totals
// of the loss kernels (train_tail.hip's L1 and regularisers, ssim.hip).  Whatever one file alone uses stays in
// that file.
#pragma once
#include <string>

#include "gs4d_internal.h"

namespace gs4d {

// sets gs4d_last_error()'s text for the calling thread and returns `code` (capi.hip)
int train_fail(int code, const std::string &msg);

constexpr int kHbMaxHeads = 8;  // heads of one deformation block (argument structs of the forward and the backward)

typedef float f4v __attribute__((ext_vector_type(4)));  // an MFMA 16x16 accumulator (4 per lane)
typedef __attribute__((ext_vector_type(8))) __bf16 bf8v;  // a bf16 MFMA operand fragment (8 k values per lane)
typedef __attribute__((ext_vector_type(4))) __bf16 bf4v;
typedef short s4v __attribute__((ext_vector_type(4)));

// The XOR-swizzled 256-byte LDS tile rows of the bf16 weight-gradient kernels (mlp_dw_bf16_kernel in mlp_gemm.hip,
// heads_bwd_wide_bf16_kernel in mlp_heads_backward.hip): conflict-free transposed reads.
__device__ __forceinline__ int dwb_off(int row, int ch) {  // byte offset of 16-byte chunk ch of tile row `row`
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}
__device__ __forceinline__ bf8v dwb_tr_frag(const unsigned char *tile, int rb, int g, int li, int c0) {
    // rows rb + 8 g .. + 7 of the 16 columns starting at chunk c0, as an MFMA operand fragment (lane li gets
    // column li): lane 4 q + p of the group addresses row (base + q), columns 4 p .. 4 p + 3
    const int q = li >> 2, p = li & 3;
    const unsigned char *a0 = tile + dwb_off(rb + 8 * g + q, c0 + (p >> 1)) + 8 * (p & 1);
    const unsigned char *a1 = tile + dwb_off(rb + 8 * g + 4 + q, c0 + (p >> 1)) + 8 * (p & 1);
    typedef __attribute__((address_space(3))) s4v lds_s4v;
    const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v *)a0);
    const s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v *)a1);
    const s4v v[2] = {lo, hi};
    return __builtin_bit_cast(bf8v, v);
}

// compute units of the current device (cached per device; inline: one cache for the whole library)
inline int cu_count() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

constexpr int kTailThreads = 256;  // workgroup size of the streaming kernels that total this way

// ---- last-workgroup totals ------------------------------------------------------------------------
// A sum over a grid's per-workgroup partials without a second launch.  Each workgroup publishes its partial
// in its slot (agent-scope relaxed atomic store: coherent across the XCDs' L2s) and draws a ticket; the
// workgroup that draws the last ticket reads every slot and sums them in a fixed order -- thread-strided, then
// the wave tree, then the waves in order: the order of the separate one-workgroup final kernels these replace,
// so totals are unchanged bit for bit -- then puts every slot and ticket back to 0 for the next call.
// Tickets in two levels: workgroup b draws from sub-counter b % kTicketFan (each on its own 128-byte line),
// the last drawer of a sub-counter from the top counter -- one counter drawn by ~2000 workgroups serialised
// its atomics (~10 ns each, ~20 us per launch here).  No fences: an acquire/release pair at agent scope
// writes back the whole L2 in every workgroup (buffer_wbl2; ~70 us per launch here).  Instead a slot holds
// bits + 1 (never 0 for a partial: a double whose bits are all ones is not produced), and the last workgroup
// waits on any slot still reading 0 (a store issued before its workgroup's ticket, not yet visible); the wait
// is bounded.  Scratch layout: the counters at the 8-aligned start (kTicketWords words), the slots after them;
// all zero on entry and again on return (the callers keep the scratch).
constexpr int kTicketFan = 16, kTicketLine = 32;  // sub-counters; u32 words per counter (128 bytes)
constexpr int kTicketWords = (kTicketFan + 1) * kTicketLine;
struct TicketScratch {
    uint32_t *ticket;  // [0] top, [(j + 1) * kTicketLine] sub-counter j
    double *part;
};
__host__ __device__ inline TicketScratch ticket_scratch(void *scratch) {
    uint32_t *t = (uint32_t *)(((size_t)scratch + 7) & ~(size_t)7);
    return {t, (double *)(t + kTicketWords)};
}

// Thread 0 holds `t`, this workgroup's partial.  Returns true in every thread of the last workgroup, with
// the total in *total (all threads); false elsewhere.
__device__ __forceinline__ bool publish_and_total(double t, TicketScratch ts, int nblk, double *total) {
    __shared__ uint32_t s_last;
    __shared__ double s_w[kTailThreads / 64];
    unsigned long long *slot = (unsigned long long *)ts.part;
    if (threadIdx.x == 0) {
        __hip_atomic_store(slot + blockIdx.x, (unsigned long long)__double_as_longlong(t) + 1ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t j = blockIdx.x % kTicketFan, nj = ((uint32_t)nblk - j + kTicketFan - 1) / kTicketFan;
        uint32_t *sub = ts.ticket + (j + 1) * kTicketLine;
        bool last = false;
        if (__hip_atomic_fetch_add(sub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nj - 1u) {
            __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every draw on it is done
            const uint32_t nsub = nblk < kTicketFan ? (uint32_t)nblk : (uint32_t)kTicketFan;
            last = __hip_atomic_fetch_add(ts.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsub - 1u;
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return false;
    // the slots in rounds of kRound per thread, all loads of a round in flight at once (then the rare waits)
    constexpr int kRound = 8;
    double s = 0.0;
    bool lost = false;  // a slot still 0 after the bounded wait
    for (int i0 = 0; i0 < nblk; i0 += kRound * kTailThreads) {
        unsigned long long v[kRound];
#pragma unroll
        for (int k = 0; k < kRound; k++) {
            const int i = i0 + k * kTailThreads + (int)threadIdx.x;
            v[k] = i < nblk ? __hip_atomic_load(slot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 1ull;  // 1: +0.0
        }
#pragma unroll
        for (int k = 0; k < kRound; k++) {
            const int i = i0 + k * kTailThreads + (int)threadIdx.x;
            for (uint32_t spins = 0; v[k] == 0ull && spins < (1u << 22); spins++)
                v[k] = __hip_atomic_load(slot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lost |= v[k] == 0ull;
            if (i < nblk) __hip_atomic_store(slot + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (i < nblk && v[k] != 0ull) s += __longlong_as_double((long long)(v[k] - 1ull));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    // A slot that never arrived (the wait gave up: never seen, but possible in principle) leaves its late store
    // behind in the kept scratch, which would corrupt a later call's total silently.  Instead the scratch is
    // poisoned (word 1 of the top counter's line, sticky): this total and every later one with this scratch
    // are NaN, until the caller zeroes the scratch again.
    const bool any_lost = __syncthreads_or(lost);
    if (any_lost && threadIdx.x == 0) __hip_atomic_store(ts.ticket + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool poisoned = any_lost || __hip_atomic_load(ts.ticket + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < kTailThreads / 64; w++) sum += s_w[w];
    *total = poisoned ? __builtin_nan("") : sum;
    if (threadIdx.x == 0) __hip_atomic_store(ts.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

}  // namespace gs4d
