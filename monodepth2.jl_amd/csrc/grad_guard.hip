// md2_grad_norm: the global L2 norm of a flat fp32 gradient, the clip coefficient and the
// non-finite count, as one device state block (md2_guard_state) that the guarded ADAM kernels
// (optim.hip) read. include/md2.h states the summation order and every operation of the finish.
//
// Built with -ffp-contract=off and correctly rounded division / square root: the finish is a handful
// of scalar operations that the NumPy restatement of the tests repeats bit for bit.  (The sum itself
// is insensitive to contraction: the product of two fp32 values is exact in fp64.)
//
// Passes:
//   grad_sumsq         B = min(ceil(n / 4096), 1024) blocks; one fp64 partial and one count per block
//   grad_guard_finish  one block: the partials in a fixed order, then the state
// No atomics and no counters: the result is bitwise reproducible, and it does not depend on the
// pointer's alignment (the 4-byte path reads the same elements in the same threads).
#include "nn.h"

#include <cmath>

namespace md2 {
namespace {

constexpr int GG_MAX_BLOCKS = 1024;

__device__ __forceinline__ void gg_add(float x, double& s, double& c) {
  if (fabsf(x) <= 3.402823466e38f) {   // false for NaN and the infinities
    const double d = (double)x;
    s = s + d * d;
  }
  else
    c = c + 1.0;
}

// VEC: g is 16-byte aligned, so element 4 q is too
template <bool VEC>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n,
                                                          double* __restrict__ part, double* __restrict__ cnt) {
  __shared__ double red[4 * 2];
  const long long stride = (long long)gridDim.x * 1024;
  long long i = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
  double v[2] = {0.0, 0.0};   // sum of squares, non-finite count (exact in fp64: at most 2^31)
#pragma unroll 4
  for (; i + 3 < n; i += stride) {
    float4 x;
    if (VEC)
      x = *reinterpret_cast<const float4*>(g + i);
    else
      x = make_float4(g[i], g[i + 1], g[i + 2], g[i + 3]);
    gg_add(x.x, v[0], v[1]);
    gg_add(x.y, v[0], v[1]);
    gg_add(x.z, v[0], v[1]);
    gg_add(x.w, v[0], v[1]);
  }
  // the one group that n cuts (i + 3 >= n): every later group of this thread lies past n
  for (int e = 0; e < 3; ++e)
    if (i + e < n) gg_add(g[i + e], v[0], v[1]);
  block_sum256_d<2>(v, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = v[0];
    cnt[blockIdx.x] = v[1];
  }
}

__global__ __launch_bounds__(256) void grad_guard_finish_kernel(const double* __restrict__ part,
                                                                 const double* __restrict__ cnt, int B,
                                                                 float grad_scale, float max_norm,
                                                                 md2_guard_state* __restrict__ state) {
  __shared__ double red[4 * 2];
  double v[2] = {0.0, 0.0};
  for (int k = threadIdx.x; k < B; k += 256) {
    v[0] = v[0] + part[k];
    v[1] = v[1] + cnt[k];
  }
  block_sum256_d<2>(v, red);
  if (threadIdx.x != 0) return;
  const double S = v[0];
  const long long c = (long long)v[1];
  const int ok = c == 0;
  const float norm = (float)(sqrt(S) * (double)grad_scale);
  const bool clip = ok && fabsf(max_norm) <= 3.402823466e38f && norm > max_norm;
  const float coef = clip ? __fdiv_rn(max_norm, norm) : 1.0f;
  state->sumsq = S;
  state->nonfinite = c;
  state->skipped = state->skipped + (ok ? 0 : 1);
  state->norm = norm;
  state->coef = coef;
  state->gscale = grad_scale * coef;
  state->ok = ok;
}

}  // namespace

static int grad_norm_blocks(long long n) {
  const long long b = (n + 4095) / 4096;
  return (int)(b < GG_MAX_BLOCKS ? b : GG_MAX_BLOCKS);
}

size_t grad_norm_workspace_bytes(long long n) {
  if (n < 1 || n > (1LL << 31)) return 0;
  return 2 * sizeof(double) * (size_t)grad_norm_blocks(n);   // partials, then counts
}

int grad_norm(const float* g, long long n, float grad_scale, float max_norm, md2_guard_state* state,
              void* workspace, hipStream_t st) {
  const int B = grad_norm_blocks(n);
  double* part = (double*)workspace;
  double* cnt = part + B;
  if (((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(B), dim3(256), 0, st, g, n, part, cnt);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(B), dim3(256), 0, st, g, n, part, cnt);
  hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part,
                     (const double*)cnt, B, grad_scale, max_norm, state);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
