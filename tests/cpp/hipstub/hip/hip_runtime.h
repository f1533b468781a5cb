// Stand-in for <hip/hip_runtime.h> in CPU checks of device headers (tests/cpp/slots_kernel_check.cpp): the qualifiers vanish, a workgroup is ONE thread
// (threadIdx 0, blockDim 1), so every loop of a phase runs to its end before the next phase starts and a barrier has nothing to wait for.
#pragma once
#include <cstddef>
#include <cstdint>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
struct ulonglong2 { unsigned long long x, y; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
extern dim3 threadIdx, blockIdx, blockDim, gridDim;
inline void __syncthreads() {}
inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
