// Shared device/host helpers for the habitat_amd gfx950 kernel library.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#define HAB_OK 0
#define HAB_ERR_ARG -1
#define HAB_ERR_UNSUPPORTED -2
// Internal: "this kernel form does not apply to the problem, try the next one".  Returned by the launch functions of the kernel
// headers to their callers inside the library; it never crosses the C ABI (the entry points map it to HAB_ERR_UNSUPPORTED).
#define HAB_NOT_APPLICABLE 1

#define HAB_LAUNCH_CHECK()                                  \
    do {                                                    \
        hipError_t e__ = hipGetLastError();                 \
        if (e__ != hipSuccess) return (int)e__;             \
    } while (0)

#define HAB_TRY(expr)                                       \
    do {                                                    \
        int r__ = (int)(expr);                              \
        if (r__ != 0) return r__;                           \
    } while (0)

// Try one kernel form: return its result unless the form does not apply to this problem.
#define HAB_TRY_FORM(expr)                                  \
    do {                                                    \
        int r__ = (int)(expr);                              \
        if (r__ != HAB_NOT_APPLICABLE) return r__;          \
    } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace hab {

constexpr int WAVE = 64;

// Development switches (HAB_GN_STREAM, HAB_BF3_NOSIGN, ...) select the older variant of a kernel for A/B measurements.  They are read
// once per process: `static const bool off = hab_env_flag("HAB_...");` at the point of use.
inline bool hab_env_flag(const char* name) { return getenv(name) != nullptr; }
inline int hab_env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline long long cdivl(long long a, long long b) { return (a + b - 1) / b; }

// Launch prologue of a kernel with dynamic LDS: raise Kern's MaxDynamicSharedMemorySize to `bytes` (the same value at every call of
// an instantiation), once per process and instantiation; `needed` = false (launchers whose LDS may fit the default 64 KB) skips it.
// Thread-safe static initialisation: engines of several inference-worker threads launch concurrently.
template <auto Kern>
inline hipError_t lds_opt_in(int bytes, bool needed = true) {
    static const hipError_t err =
        needed ? hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) : hipSuccess;
    return err;
}

// Workgroups of a persistent kernel: max_grid, less 8 (one per XCD) while there are fewer items than workgroups, at least 8.
inline int persistent_grid(int items, int max_grid = 256) {
    int grid = max_grid;
    while (grid > 8 && grid > items) grid -= 8;
    return grid;
}

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-wide sum for blockDim.x == 256 (4 waves); result valid in every thread.
__device__ inline float block_sum_256(float v, float* smem4) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smem4[w] = v;
    __syncthreads();
    return (smem4[0] + smem4[1]) + (smem4[2] + smem4[3]);
}

__device__ inline float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

}  // namespace hab

namespace hab {
// Division by a runtime-invariant divisor d (1 <= d < 2^31) of 0 <= n < 2^31 via multiply-high, branch-free:
// d >= 2: l = ceil(log2 d), M = ceil(2^(31+l)/d) < 2^32, q = mulhi(n, M) >> (l-1)  (exact for n < 2^31);
// d == 1: M = 0, add = 1, shift = 0 -> q = n.
struct FastDiv {
    uint32_t mul, shift, d, add;
    FastDiv() : mul(0), shift(0), d(1), add(1) {}
    explicit FastDiv(int dd) {
        d = (uint32_t)dd;
        mul = 0;
        shift = 0;
        add = 1;
        if (dd <= 1) return;
        uint32_t l = 0;
        while ((1ull << l) < (uint64_t)d) ++l;
        mul = (uint32_t)((((uint64_t)1 << (31 + l)) + d - 1) / d);
        shift = l - 1;
        add = 0;
    }
    __host__ __device__ inline int div(int n) const {
#ifdef __HIP_DEVICE_COMPILE__
        const uint32_t hi = __umulhi((uint32_t)n, mul);
#else
        const uint32_t hi = (uint32_t)(((uint64_t)(uint32_t)n * mul) >> 32);
#endif
        return (int)((hi + (uint32_t)n * add) >> shift);
    }
    __host__ __device__ inline void divmod(int n, int& q, int& r) const {
        q = div(n);
        r = n - q * (int)d;
    }
};
}  // namespace hab
