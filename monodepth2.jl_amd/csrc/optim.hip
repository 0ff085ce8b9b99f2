// Flux ADAM over the flat parameter vector (nn.h), eager and graph-replayed, plain and guarded.
#include "nn.h"

namespace md2 {

// Flux ADAM (Flux.Optimise.apply!): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= lr * (m / bc1) / (sqrt(v / bc2) + eps), with bc = 1 - beta^t.
// The one copy of the update.  The guarded step must give the plain step's bytes and the captured
// step the eager step's (tests/test_gpu_grad_guard.py, tests/test_gpu_graph.py): the four kernels
// below only differ in where bc1 / bc2 / gscale come from, and they share this translation unit,
// so that they are compiled alike.
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g,
                                            float* __restrict__ m, float* __restrict__ v, long i,
                                            float lr, float b1, float b2, float eps, float bc1,
                                            float bc2, float gscale) {
  const float gi = g[i] * gscale;
  const float mi = b1 * m[i] + (1.f - b1) * gi;
  const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long n,
                                                   float lr, float b1, float b2, float eps, float bc1,
                                                   float bc2, float gscale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  adam_update(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2, gscale);
}

// Graph-replayed ADAM: the step counter lives on the device (adam_prep increments it and forms
// the bias corrections), so one captured step replays for every t.
__global__ void adam_prep_kernel(int* __restrict__ step, float* __restrict__ bc, float b1, float b2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int t = step[0] + 1;
  step[0] = t;
  bc[0] = (float)(1.0 - pow((double)b1, (double)t));
  bc[1] = (float)(1.0 - pow((double)b2, (double)t));
}

__global__ void set_int_kernel(int* __restrict__ p, int v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) p[0] = v;
}

__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, long n,
                                                       float lr, float b1, float b2, float eps,
                                                       const float* __restrict__ bc, float gscale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  adam_update(p, g, m, v, i, lr, b1, b2, eps, bc[0], bc[1], gscale);
}

// The guarded forms (md2_adam_guarded, md2_model_set_grad_guard): the gradient scale and the verdict
// come from the device state grad_guard_finish wrote (grad_guard.hip).  A step that is not ok
// returns before it touches p, m or v.
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long n,
                                                           float lr, float b1, float b2, float eps, float bc1,
                                                           float bc2, const md2_guard_state* __restrict__ gs) {
  if (!gs->ok) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  adam_update(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2, gs->gscale);
}

__global__ __launch_bounds__(256) void adam_dev_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               long n, float lr, float b1, float b2, float eps,
                                                               const float* __restrict__ bc,
                                                               const md2_guard_state* __restrict__ gs) {
  if (!gs->ok) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  adam_update(p, g, m, v, i, lr, b1, b2, eps, bc[0], bc[1], gs->gscale);
}

int adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
              float eps, float bc1, float bc2, float gscale, hipStream_t st) {
  hipLaunchKernelGGL(adam_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, p, g, m, v, n, lr, b1, b2,
                     eps, bc1, bc2, gscale);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int adam_step_dev(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                  float eps, const float* bc, float gscale, hipStream_t st) {
  hipLaunchKernelGGL(adam_dev_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, p, g, m, v, n, lr, b1, b2,
                     eps, bc, gscale);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int adam_step_guarded(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                      float eps, float bc1, float bc2, const md2_guard_state* gs, hipStream_t st) {
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, p, g, m, v, n, lr, b1, b2,
                     eps, bc1, bc2, gs);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int adam_step_dev_guarded(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                          float eps, const float* bc, const md2_guard_state* gs, hipStream_t st) {
  hipLaunchKernelGGL(adam_dev_guarded_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, p, g, m, v, n, lr, b1,
                     b2, eps, bc, gs);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int adam_prep(int* step, float* bc, float b1, float b2, hipStream_t st) {
  hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(64), 0, st, step, bc, b1, b2);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int set_device_int(int* p, int v, hipStream_t st) {
  hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, st, p, v);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
