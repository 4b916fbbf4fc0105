// Test hooks (include/hop_testhooks.h): put a known bit pattern into the LDS of every
// compute unit, and witness that it is what a following launch finds.  LDS keeps its
// contents from one kernel to the next, so a kernel that reads a word it has not written
// computes with whatever the kernel before it left there; the suite runs the kernels
// under test after these fills (tests/test_gpu_lds_poison.py).  Not a product path.
#include "hop_kernels.hpp"
#include "../../include/hop_testhooks.h"

namespace hop {
namespace probe {

constexpr int kFillThreads = 1024;
constexpr int kLdsWords = HOP_TEST_LDS_BYTES / 8;
// a group keeps its compute unit for kIdleIters sleeps of 127 x 64 clocks after its
// writes (about 0.2 ms): far longer than the dispatcher needs to place one group on each
// of the other compute units, so the first groups_per_cu-th of the grid covers them all
constexpr int kIdleIters = 64;

// one workgroup = the whole LDS of a compute unit
__global__ __launch_bounds__(kFillThreads) void lds_fill_kernel(unsigned long long pattern) {
  __shared__ unsigned long long lds[kLdsWords];
  for (int i = threadIdx.x; i < kLdsWords; i += kFillThreads) lds[i] = pattern;
  // nothing here reads the words: the empty statement takes the array's address and may
  // read memory, so the stores stay (as plain LDS stores; volatile would make them flat)
  asm volatile("" : : "v"((unsigned)(unsigned long long)&lds[0]) : "memory");
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < kIdleIters; ++i) __builtin_amdgcn_s_sleep(127);
}

// the first wave of each group reads the group's whole dynamic allocation; nothing
// writes LDS here
__global__ void lds_scan_kernel(unsigned long long pattern, int words, int* all_pattern) {
  extern __shared__ unsigned long long dyn[];
  if (threadIdx.x >= 64) return;  // wave-uniform
  // the words are whatever the kernel before left: the empty statement may have written
  // memory, so the loads below are real ones
  asm volatile("" : : "v"((unsigned)(unsigned long long)&dyn[0]) : "memory");
  bool same = true;
  for (int i = threadIdx.x; i < words; i += 64) same = same && (dyn[i] == pattern);
  const int all = __all(same) != 0;
  if (threadIdx.x == 0) all_pattern[blockIdx.x] = all;
}

}  // namespace probe
}  // namespace hop

extern "C" {

int hop_test_lds_fill(uint64_t pattern, int32_t groups_per_cu, void* stream) {
  using hop::set_error;
  if (groups_per_cu < 1 || groups_per_cu > 16)
    return set_error(HOP_E_ARG, "groups_per_cu must be in [1, 16]");
  int dev = -1, cus = 0;
  if (hipStreamGetDevice((hipStream_t)stream, &dev) != hipSuccess) {
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hop::set_hip_status(e);
  }
  const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return hop::set_hip_status(e);
  if (cus < 1) return set_error(HOP_E_HIP, "the device reports no compute units");
  const unsigned grid = (unsigned)groups_per_cu * (unsigned)cus;
  hipLaunchKernelGGL(hop::probe::lds_fill_kernel, dim3(grid), dim3(hop::probe::kFillThreads), 0,
                     (hipStream_t)stream, (unsigned long long)pattern);
  return hop::set_hip_status(hipGetLastError());
}

int hop_test_lds_scan(uint64_t pattern, int32_t lds_bytes, int32_t threads, int64_t groups,
                      int32_t* all_pattern, void* stream) {
  using hop::set_error;
  if (lds_bytes < 8 || lds_bytes > HOP_TEST_LDS_BYTES || lds_bytes % 8 != 0)
    return set_error(HOP_E_ARG, "lds_bytes must be a multiple of 8 in [8, 163840]");
  if (threads < 64 || threads > 1024) return set_error(HOP_E_ARG, "threads must be in [64, 1024]");
  if (groups < 1 || groups > 0x7fffffffLL)
    return set_error(HOP_E_ARG, "groups must be in [1, 2^31 - 1]");
  if (!all_pattern) return set_error(HOP_E_ARG, "null pointer");
  if (lds_bytes > 65536) {  // past the default limit of a dynamic allocation
    const hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void*>(hop::probe::lds_scan_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return hop::set_hip_status(e);
  }
  hipLaunchKernelGGL(hop::probe::lds_scan_kernel, dim3((unsigned)groups), dim3((unsigned)threads),
                     (size_t)lds_bytes, (hipStream_t)stream, (unsigned long long)pattern,
                     lds_bytes / 8, all_pattern);
  return hop::set_hip_status(hipGetLastError());
}

}  // extern "C"
