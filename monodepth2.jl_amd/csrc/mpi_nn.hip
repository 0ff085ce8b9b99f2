// MPI-mode helpers of the executor (nn.h): the plane embedding of the decoder input, the _repeat
// pullback over the plane axis and the row repeat with its adjoint.
#include "nn_util.h"

namespace md2 {

// MPI-mode decoder input: repeat(target features, planes) ++ repeat(embed(bins), h, w) along
// channels, planes merged into the batch (src/model.jl:39-50, embed :4-15).  One thread per
// output element; the embedding channel is recomputed per element (2 transcendental ops at most).
__global__ __launch_bounds__(256) void mpi_embed_kernel(const float* __restrict__ feat, long sstride,
                                                        int C, int hw, const float* __restrict__ bins,
                                                        int P, int E, int Ctot, float* __restrict__ out,
                                                        long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int px = (int)(i % hw);
  const long t = i / hw;
  const int c = (int)(t % Ctot);
  const long img = t / Ctot;            // b * P + p
  const int b = (int)(img / P), p = (int)(img - (long)b * P);
  float v;
  if (c < C) {
    v = feat[(long)b * sstride + (long)c * hw + px];
  } else if (c >= C + E) {
    v = 0.f;                            // zero padding channels (Ctot > C + E)
  } else {
    const int e = c - C;
    const float x = bins[(long)b * P + p];
    if (e == 0) {
      v = x;
    } else {
      const float a = ldexpf(x, (e - 1) >> 1);  // 2^i x, exact in fp32 like the reference's 2^i .* x
      v = (e & 1) ? sinf(a) : cosf(a);
    }
  }
  out[i] = v;
}

int mpi_embed_features(const float* feat, long sample_stride, int N, int C, int h, int w,
                       const float* bins, int P, int L, float* out, hipStream_t st, int Ctot) {
  const int E = 2 * L + 1;
  if (Ctot <= 0) Ctot = C + E;
  if (Ctot < C + E) {
    set_error("mpi_embed_features: output channels < C + 2L + 1");
    return MD2_EINVAL;
  }
  const long n = (long)N * P * Ctot * h * w;
  MD2_TRY(check_u31(n));
  hipLaunchKernelGGL(mpi_embed_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, feat, sample_stride, C,
                     h * w, bins, P, E, Ctot, out, n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// The _repeat pullback over the plane axis (src/repeat.jl:44-53, block sum): for the first C of
// the Cin channels of every decoder input image, out[b][c][q] (+)= sum_p in[b*P + p][c][q], in the
// fixed order p = 0..P-1 (the embedding channels c >= C get no gradient: embed is
// @non_differentiable, src/model.jl:15).  4 pixels per thread.
__global__ __launch_bounds__(256) void plane_sum_kernel(const float* __restrict__ in, int P, int Cin,
                                                        int C, int hw4, float* __restrict__ out,
                                                        int acc, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int q = (int)(i % hw4);
  const long t = i / hw4;
  const int c = (int)(t % C);
  const long b = t / C;
  const long pstride = (long)Cin * hw4;
  const float4* src = reinterpret_cast<const float4*>(in) + ((b * P) * Cin + c) * (long)hw4 + q;
  float4 s = src[0];
  for (int p = 1; p < P; ++p) {
    const float4 v = src[(long)p * pstride];
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  float4* dst = reinterpret_cast<float4*>(out) + i;
  if (acc) {
    const float4 o = *dst;
    s.x += o.x;
    s.y += o.y;
    s.z += o.z;
    s.w += o.w;
  }
  *dst = s;
}

// the same block sum one pixel per thread, for maps whose h*w is not a multiple of 4 (e.g. the
// 3x10 level-4 map of a 96x320 input)
__global__ __launch_bounds__(256) void plane_sum1_kernel(const float* __restrict__ in, int P, int Cin,
                                                         int C, int hw, float* __restrict__ out,
                                                         int acc, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int q = (int)(i % hw);
  const long t = i / hw;
  const int c = (int)(t % C);
  const long b = t / C;
  const float* src = in + ((b * P) * Cin + c) * (long)hw + q;
  float s = src[0];
  for (int p = 1; p < P; ++p) s += src[(long)p * Cin * hw];
  if (acc) s += out[i];
  out[i] = s;
}

int plane_sum(const float* in, int N, int P, int Cin, int C, long hw, float* out, int accumulate,
              hipStream_t st) {
  if (hw % 4 != 0) {
    const long n = (long)N * C * hw;
    MD2_TRY(check_u31(n));
    hipLaunchKernelGGL(plane_sum1_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, in, P, Cin, C, (int)hw,
                       out, accumulate, n);
    MD2_LAUNCH_CHECK();
    return MD2_OK;
  }
  const long n4 = (long)N * C * (hw / 4);
  MD2_TRY(check_u31(4 * n4));
  hipLaunchKernelGGL(plane_sum_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, st, in, P, Cin, C,
                     (int)(hw / 4), out, accumulate, n4);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// rows of a [R][cols] matrix repeated P times (row r -> rows r*P .. r*P+P-1) and the adjoint sum
__global__ __launch_bounds__(256) void repeat_rows_kernel(const float* __restrict__ src, int cols,
                                                          int P, float* __restrict__ dst, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long row = i / cols;
  dst[i] = src[(row / P) * cols + (i - row * cols)];
}
__global__ __launch_bounds__(256) void repeat_rows_adj_kernel(const float* __restrict__ src, int cols,
                                                              int P, float* __restrict__ dst, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long row = i / cols, col = i - row * cols;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += src[(row * P + p) * cols + col];
  dst[i] = s;
}

int repeat_rows(const float* src, long rows, int cols, int P, float* dst, hipStream_t st) {
  const long n = rows * P * cols;
  MD2_TRY(check_u31(n));
  if (n == 0) return MD2_OK;
  hipLaunchKernelGGL(repeat_rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, src, cols, P, dst, n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}
int repeat_rows_adjoint(const float* src, long rows, int cols, int P, float* dst, hipStream_t st) {
  const long n = rows * cols;
  MD2_TRY(check_u31(n * P));
  if (n == 0) return MD2_OK;
  hipLaunchKernelGGL(repeat_rows_adj_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, src, cols, P, dst, n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
