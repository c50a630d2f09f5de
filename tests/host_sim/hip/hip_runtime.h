// A host stand-in for <hip/hip_runtime.h>: enough to compile csrc/optim_step.h with a host compiler and run apply_kernel one
// thread after the other (it has no barrier and no cross-lane traffic).  The kernels that do are compiled, not run.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(n)

struct dim3 {
    unsigned x, y, z;
};
struct alignas(16) float4 {
    float x, y, z, w;
};
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

inline dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1}, gridDim{1, 1, 1};

inline void __syncthreads() {}
template <class T>
inline T __shfl_down(T v, int, int) { return v; }
using std::isinf;
using std::isnan;
