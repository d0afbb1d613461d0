// train_internal.h -- the few things two or more of the train-step translation units share (train_tail.hip,
// mlp_feature.hip, mlp_heads_forward.hip, mlp_heads_backward.hip, mlp_gemm.hip).  Whatever one file alone
// uses stays in that file.
#pragma once
#include "gs4d_internal.h"

namespace gs4d {

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

}  // namespace gs4d
