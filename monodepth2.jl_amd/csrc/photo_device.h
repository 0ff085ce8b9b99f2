// Device helpers shared by the two photometric kernels (photo.hip, photo_sources.hip): the wave
// tile width, the DPP lane shifts and the 3-lane window sum, reflect indexing, and the row-step
// tags.  photo.hip's header describes how they are used.
#pragma once
#include <type_traits>

#include "loss_kernels.h"

namespace md2 {
namespace {

constexpr int PW = 60;            // output columns per wave

__device__ __forceinline__ float from_left(float v) {    // lane i <- lane i-1 (lane 0 <- 0)
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_right(float v) {   // lane i <- lane i+1 (lane 63 <- 0)
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}
// 3-lane window sums in the fixed order (v + left) + right, for NV values in two passes
// (photo.hip's header): every DPP read stays NV instructions away from the write of its operand
template <int NV>
__device__ __forceinline__ void hsum3_n(float (&v)[NV]) {
  float t[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) t[i] = v[i] + from_left(v[i]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = t[i] + from_right(v[i]);
}
__device__ __forceinline__ int reflect_clamp(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
// a wave-uniform value pinned in a VGPR (photo.hip's header: the kernels are short of SGPRs)
__device__ __forceinline__ float vreg(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

template <int N_>
using Slot = std::integral_constant<int, N_>;

// which phases a row step runs (P1 always)
constexpr int PH_P2 = 1, PH_P3 = 2, PH_ALL = 3;

}  // namespace
}  // namespace md2
