/* The slice of the CUDA programming model that the reference's rasterizer and simple-knn sources use, for a
 * host compiler: qualifiers, vector types, the built-in index variables, barriers, cooperative-groups ranks,
 * and the few cub / thrust / runtime calls, all single-threaded (cuda_on_cpu.cpp runs one block at a time, its
 * threads as fibers in rank order).  Test infrastructure only; build_ref.py puts this directory first on the
 * include path so that <cuda.h>, <cub/cub.cuh>, ... resolve to the one-line headers that forward here.
 *
 * Arithmetic is left to the host compiler: <math.h> makes exp(float), sqrt(float), abs(float) resolve to the
 * float overloads as they do under nvcc, and nothing here contracts or reorders an expression. */
#pragma once
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <numeric>
#include <type_traits>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
/* one block runs at a time, so a block's shared array is a function-local static */
#define __shared__ static
#ifndef CUDA_VERSION
#define CUDA_VERSION 12000
#endif

static_assert(std::is_same<decltype(exp(1.0f)), float>::value && std::is_same<decltype(sqrt(1.0f)), float>::value &&
                  std::is_same<decltype(abs(1.0f)), float>::value,
              "exp / sqrt / abs of a float must stay in float, as under nvcc");

/* ---- vector types ---------------------------------------------------------------------------------------- */
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct uint2 { unsigned x, y; };
struct uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static inline float2 make_float2(float a, float b) { return {a, b}; }
static inline float3 make_float3(float a, float b, float c) { return {a, b, c}; }
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
static inline int2 make_int2(int a, int b) { return {a, b}; }
static inline int3 make_int3(int a, int b, int c) { return {a, b, c}; }
static inline uint2 make_uint2(unsigned a, unsigned b) { return {a, b}; }
static inline uint3 make_uint3(unsigned a, unsigned b, unsigned c) { return {a, b, c}; }

/* ---- min / max, with CUDA's mixed-sign overloads (the signed operand converts to unsigned) --------------- */
#define GS4D_MINMAX(T, A, B)                                                 \
    static inline T min(A a, B b) { return (T)a < (T)b ? (T)a : (T)b; } \
    static inline T max(A a, B b) { return (T)a > (T)b ? (T)a : (T)b; }
GS4D_MINMAX(int, int, int)
GS4D_MINMAX(unsigned, unsigned, unsigned)
GS4D_MINMAX(unsigned, unsigned, int)
GS4D_MINMAX(unsigned, int, unsigned)
GS4D_MINMAX(long long, long long, long long)
GS4D_MINMAX(unsigned long long, unsigned long long, unsigned long long)
GS4D_MINMAX(float, float, float)
GS4D_MINMAX(double, double, double)
#undef GS4D_MINMAX

/* ---- runtime calls: host memory is device memory --------------------------------------------------------- */
typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
static inline cudaError_t cudaMemcpy(void *d, const void *s, size_t n, cudaMemcpyKind) { memcpy(d, s, n); return cudaSuccess; }
static inline cudaError_t cudaMemset(void *d, int v, size_t n) { memset(d, v, n); return cudaSuccess; }
template <class T> static inline cudaError_t cudaMalloc(T **p, size_t n) { *p = (T *)calloc(n ? n : 1, 1); return cudaSuccess; }
static inline cudaError_t cudaFree(void *p) { free(p); return cudaSuccess; }
static inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
static inline const char *cudaGetErrorString(cudaError_t) { return "no error (host run)"; }
/* threads run one after another, so an atomic sum is a plain one, accumulated in thread-rank order */
static inline float atomicAdd(float *p, float v) { float old = *p; *p = old + v; return old; }
static inline int atomicAdd(int *p, int v) { int old = *p; *p = old + v; return old; }
static inline unsigned atomicAdd(unsigned *p, unsigned v) { unsigned old = *p; *p = old + v; return old; }
[[noreturn]] static inline void __trap() { fprintf(stderr, "\n__trap() reached in a host run of a CUDA kernel\n"); abort(); }

/* ---- the block runtime (cuda_on_cpu.cpp) ----------------------------------------------------------------- */
namespace cuda_on_cpu {
struct Indices { dim3 thread, block, block_dim, grid_dim; };
extern Indices current;                   /* of the fiber that is running */
void barrier();                           /* __syncthreads */
int barrier_count(int predicate);         /* __syncthreads_count */
void launch(const std::function<void()> &thread_body, dim3 grid, dim3 block);
}
#define threadIdx (cuda_on_cpu::current.thread)
#define blockIdx (cuda_on_cpu::current.block)
#define blockDim (cuda_on_cpu::current.block_dim)
#define gridDim (cuda_on_cpu::current.grid_dim)
static inline void __syncthreads() { cuda_on_cpu::barrier(); }
static inline int __syncthreads_count(int predicate) { return cuda_on_cpu::barrier_count(predicate); }
/* kernel<<<grid, block>>>(args...), as build_ref.py rewrites a launch site; the arguments are evaluated again by
 * every thread, which is harmless for the plain values and pointers the reference passes */
#define CUDA_ON_CPU_LAUNCH(kernel, grid, block, ...) \
    cuda_on_cpu::launch([&]() { kernel(__VA_ARGS__); }, dim3(grid), dim3(block))

namespace cooperative_groups {
struct thread_block {
    void sync() const { __syncthreads(); }
    dim3 group_index() const { return blockIdx; }
    dim3 thread_index() const { return threadIdx; }
    unsigned thread_rank() const { return (threadIdx.z * blockDim.y + threadIdx.y) * blockDim.x + threadIdx.x; }
    unsigned size() const { return blockDim.x * blockDim.y * blockDim.z; }
};
struct grid_group {
    unsigned long long thread_rank() const {
        unsigned long long b = ((unsigned long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        return b * (blockDim.x * blockDim.y * blockDim.z) + thread_block().thread_rank();
    }
};
static inline thread_block this_thread_block() { return {}; }
static inline grid_group this_grid() { return {}; }
}

/* ---- cub: the two-call convention (a null temporary buffer only reports a size) -------------------------- */
namespace cub {
struct DeviceScan {
    template <class In, class Out>
    static cudaError_t InclusiveSum(void *tmp, size_t &tmp_bytes, In in, Out out, int n) {
        if (!tmp) { tmp_bytes = 1; return cudaSuccess; }
        std::partial_sum(in, in + n, out);
        return cudaSuccess;
    }
};
struct DeviceRadixSort {
    /* stable, ascending on bits [begin_bit, end_bit) of the key, like cub's */
    template <class K, class V>
    static cudaError_t SortPairs(void *tmp, size_t &tmp_bytes, const K *keys_in, K *keys_out, const V *vals_in,
                                 V *vals_out, int n, int begin_bit = 0, int end_bit = sizeof(K) * 8) {
        if (!tmp) { tmp_bytes = 1; return cudaSuccess; }
        const int bits = end_bit - begin_bit;
        const K mask = bits >= (int)sizeof(K) * 8 ? ~K(0) : (K(1) << bits) - 1;
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return ((keys_in[a] >> begin_bit) & mask) < ((keys_in[b] >> begin_bit) & mask);
        });
        for (int i = 0; i < n; i++) { keys_out[i] = keys_in[order[i]]; vals_out[i] = vals_in[order[i]]; }
        return cudaSuccess;
    }
};
struct DeviceReduce {
    template <class In, class Out, class Op, class T>
    static cudaError_t Reduce(void *tmp, size_t &tmp_bytes, In in, Out out, int n, Op op, T init) {
        if (!tmp) { tmp_bytes = 1; return cudaSuccess; }
        T acc = init;
        for (int i = 0; i < n; i++) acc = op(acc, in[i]);
        *out = acc;
        return cudaSuccess;
    }
};
}

/* ---- thrust: device_vector and sequence ------------------------------------------------------------------ */
namespace thrust {
template <class T> struct device_ptr {
    T *p;
    T *get() const { return p; }
};
template <class T> class device_vector {
    std::vector<T> v;
public:
    device_vector() {}
    explicit device_vector(size_t n) : v(n) {}
    void resize(size_t n) { v.resize(n); }
    size_t size() const { return v.size(); }
    device_ptr<T> data() { return {v.data()}; }
    T *begin() { return v.data(); }
    T *end() { return v.data() + v.size(); }
};
template <class It> static inline void sequence(It first, It last) { std::iota(first, last, 0); }
}
