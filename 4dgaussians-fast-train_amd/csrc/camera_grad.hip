// camera_grad.hip -- the last step of the camera gradient (gs4d_backward_camera): the sum over the workgroups of the
// per-Gaussian backward (preprocess_backward.hip) of the rows they left, into dL/dviewmatrix, dL/dprojmatrix and
// dL/dcampos.
//
// No float atomics and no completion counter: one workgroup of kSumSlices x 32 threads.  Thread (slice, k) adds value
// k of the rows of its slice -- a contiguous run of ceil(n_rows / kSumSlices) rows -- in ascending row order, in
// fp64; thread k then adds the slices' sums in ascending slice order and rounds once to fp32.  The order is a
// function of n_rows alone (of P and of which per-Gaussian kernel ran), so the 35 floats are bitwise repeatable.
// At P = 100k the rows are 782 x 128 B: one small launch.
#include "gs4d_internal.h"

namespace gs4d {

constexpr int kSumSlices = 32;

// the row's value that output element e of dL_dcamera takes, or -1 for an element that is identically zero:
// viewmatrix column 3 (t reads three columns) and projmatrix column 2 (the NDC depth is not used)
__device__ __forceinline__ int cam_value_of(int e) {
    if (e < 16) return (e & 3) < 3 ? 3 * (e >> 2) + (e & 3) : -1;
    if (e < 32) {
        const int j = e & 3, i = (e - 16) >> 2;
        return j == 2 ? -1 : 12 + 3 * i + (j == 3 ? 2 : j);
    }
    return 24 + (e - 32);
}

__global__ __launch_bounds__(kSumSlices * 32) void camera_grad_sum_kernel(const float *__restrict__ rows, int n_rows,
                                                                         float *__restrict__ dL_dcamera) {
    __shared__ double sums[kSumSlices][33];
    const int k = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const int per = (n_rows + kSumSlices - 1) / kSumSlices;
    const int r0 = min(n_rows, slice * per), r1 = min(n_rows, r0 + per);
    double acc = 0.0;
    if (k < 27)
        for (int r = r0; r < r1; r++) acc += (double)rows[(size_t)r * kCamRow + k];
    sums[slice][k] = acc;
    __syncthreads();
    if (threadIdx.x < 35) {
        const int q = cam_value_of(threadIdx.x);
        double t = 0.0;
        if (q >= 0)
            for (int s = 0; s < kSumSlices; s++) t += sums[s][q];
        dL_dcamera[threadIdx.x] = (float)t;
    }
}

hipError_t launch_camera_grad_sum(const float *rows, int n_rows, float *dL_dcamera, hipStream_t s) {
    hipLaunchKernelGGL(camera_grad_sum_kernel, dim3(1), dim3(kSumSlices * 32), 0, s, rows, n_rows, dL_dcamera);
    return hipGetLastError();
}

}  // namespace gs4d
