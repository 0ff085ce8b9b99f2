// Pose head and the pose-pair gather / gradient scatter (nn.h).
#include "nn_util.h"

namespace md2 {

// ---------------------------------------------------------------------------------------------
// Pose head: Conv((1,1), 256=>6) + mean over (w,h) + 1e-2 scale (src/pose_decoder.jl:19,29-30).
// mean(W x + b) = W mean(x) + b, so the 1x1 conv runs on the spatial means.
// ---------------------------------------------------------------------------------------------
// one wave per (pair, channel): lanes stride the plane, then a fixed-order wave sum (one thread
// per channel walking its plane serially was latency-bound: 28 us for 24 x 256 planes of 52)
__global__ __launch_bounds__(256) void pose_means_kernel(const float* __restrict__ x, int C, long HW,
                                                         float* __restrict__ means) {
  const int q = blockIdx.x, c = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const float* p = x + ((long)q * C + c) * HW;
  float s = 0.f;
  for (long i = lane; i < HW; i += 64) s += p[i];
  s = wave_sum(s);
  if (lane == 0) means[(long)q * C + c] = s / (float)HW;
}

__global__ __launch_bounds__(64) void pose_fc_kernel(const float* __restrict__ means, int C,
                                                     const float* __restrict__ w,
                                                     const float* __restrict__ b,
                                                     float* __restrict__ pose) {
  const int q = blockIdx.x, k = blockIdx.y;
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 64) s += w[(long)k * C + c] * means[(long)q * C + c];
  s = wave_sum(s);
  if (threadIdx.x == 0) pose[q * 6 + k] = 1e-2f * (s + b[k]);
}

int pose_head_fwd(const float* x, int Q, int C, long HW, const float* w, const float* b,
                  float* means, float* pose, hipStream_t st) {
  hipLaunchKernelGGL(pose_means_kernel, dim3(Q, cdiv(C, 4)), dim3(256), 0, st, x, C, HW, means);
  MD2_LAUNCH_CHECK();
  hipLaunchKernelGGL(pose_fc_kernel, dim3(Q, 6), dim3(64), 0, st, means, C, w, b, pose);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

__global__ __launch_bounds__(256) void pose_head_dx_kernel(const float* __restrict__ dpose, int C,
                                                           long HW, const float* __restrict__ w,
                                                           FastDiv fdHW, FastDiv fdC,
                                                           float* __restrict__ dx, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t qc = fdiv(i, fdHW), q = fdiv(qc, fdC);
  const int c = (int)(qc - q * fdC.d);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) s += dpose[q * 6 + k] * w[(long)k * C + c];
  dx[i] = s * (1e-2f / (float)HW);
}

__global__ __launch_bounds__(256) void pose_head_dw_kernel(const float* __restrict__ dpose, int Q,
                                                           int C, const float* __restrict__ means,
                                                           float* __restrict__ dw,
                                                           float* __restrict__ db) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < 6 * C) {
    const int k = idx / C, c = idx % C;
    float s = 0.f;
    for (int q = 0; q < Q; ++q) s += dpose[q * 6 + k] * means[(long)q * C + c];
    dw[idx] = 1e-2f * s;
  }
  if (idx < 6) {
    float s = 0.f;
    for (int q = 0; q < Q; ++q) s += dpose[q * 6 + idx];
    db[idx] = 1e-2f * s;
  }
}

int pose_head_bwd(const float* dpose, int Q, int C, long HW, const float* w, const float* means,
                  float* dx, float* dw, float* db, hipStream_t st) {
  const long n = (long)Q * C * HW;
  MD2_TRY(check_u31(n));
  hipLaunchKernelGGL(pose_head_dx_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dpose, C, HW, w,
                     fd(HW), fd(C), dx, (uint32_t)n);
  MD2_LAUNCH_CHECK();
  hipLaunchKernelGGL(pose_head_dw_kernel, dim3(cdiv(6 * C, 256)), dim3(256), 0, st, dpose, Q, C,
                     means, dw, db);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// Pose pairs (src/model.jl:57-70 _get_pose_features): pair j of sample q = (frame a_j, frame b_j)
// with a_j = min(source_j, target), b_j = max(source_j, target); squeezer outputs are frame-major
// images f*N + q.  pair_gather builds the PoseDecoder input [2N][2C][HW] (only when the pairs are
// not the (q, q+N) zero-copy layout of target 2 / sources 1, 3); pair_grad scatters its gradient
// back: d sq[f*N + q] = sum_j [a_j == f] d pin[jN + q][:C] + [b_j == f] d pin[jN + q][C:].
__global__ __launch_bounds__(256) void pair_gather_kernel(const float* __restrict__ sq, int N,
                                                          FastDiv fdper, int a0, int a1, int b0,
                                                          int b1, float* __restrict__ pin,
                                                          uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;   // over [2N][2][per]
  if (i >= n) return;
  const long per = fdper.d;
  const uint32_t row = fdiv(i, fdper);                // (jN + q)*2 + half
  const long r = i - (long)row * per;
  const int half = row & 1, img = row >> 1, j = img >= N ? 1 : 0, q = img - j * N;
  const int f = half ? (j ? b1 : b0) : (j ? a1 : a0);
  pin[i] = sq[((long)f * N + q) * per + r];
}

__global__ __launch_bounds__(256) void pair_grad_kernel(const float* __restrict__ dpin, int N,
                                                        FastDiv fdper, int a0, int a1, int b0,
                                                        int b1, float* __restrict__ dsq,
                                                        uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;   // over [3N][per]
  if (i >= n) return;
  const long per = fdper.d;
  const uint32_t b = fdiv(i, fdper);
  const long r = i - (long)b * per;
  const int f = (int)b / N, q = (int)b - f * N;
  float s = 0.f;
  if (a0 == f) s += dpin[((long)q * 2) * per + r];
  if (b0 == f) s += dpin[((long)q * 2 + 1) * per + r];
  if (a1 == f) s += dpin[((long)(N + q) * 2) * per + r];
  if (b1 == f) s += dpin[((long)(N + q) * 2 + 1) * per + r];
  dsq[i] = s;
}

int pair_gather(const float* sq, int N, int C, long HW, const int a[2], const int b[2], float* pin,
                hipStream_t st) {
  const long n = 4L * N * C * HW;
  MD2_TRY(check_u31(n));
  hipLaunchKernelGGL(pair_gather_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, sq, N, fd((long)C * HW),
                     a[0], a[1], b[0], b[1], pin, (uint32_t)n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int pair_grad_gather(const float* dpin, int N, int C, long HW, const int a[2], const int b[2],
                     float* dsq, hipStream_t st) {
  const long n = 3L * N * C * HW;
  MD2_TRY(check_u31(2 * n));
  hipLaunchKernelGGL(pair_grad_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dpin, N, fd((long)C * HW),
                     a[0], a[1], b[0], b[1], dsq, (uint32_t)n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
