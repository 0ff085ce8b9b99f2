// md2_color_jitter: torchvision's float-tensor ColorJitter (brightness, contrast, saturation, hue in
// a per-sample order) on a batch of frame tuples.  include/md2.h states the semantics.
//
// Built with -ffp-contract=off and correctly rounded divisions: every product, sum and quotient
// below is rounded on its own, in the order the header gives, so the float32 NumPy restatement of
// the tests gets the same bits.
//
// Two launches, each over all samples and frames (grid = blocks of a frame, frame, sample):
//   reduce   the operations that precede contrast in the sample's order, then gray; summed in fp64
//            per thread, by shuffles over the wave, through LDS over the block's four waves: one
//            partial per block in the workspace
//   apply    thread 0 of each block adds the frame's partials in index order (the frame mean), then
//            every thread recomputes the whole chain from x and writes out
// No floating-point atomics, and a grid that depends on the sizes alone: the result is bitwise
// reproducible.  A pixel is read and written by the same thread of the apply pass and the reduce
// pass only reads x, so out == x is safe.  The per-sample parameters travel by value in the kernels'
// arguments (1.3 KB at MD2_JITTER_MAX_SAMPLES): no copy and no host synchronisation.
#include "common.h"

#include <cmath>

namespace md2 {
namespace jitter {

constexpr int MAX_BLOCKS = 64;   // blocks per frame: the partials thread 0 of the apply pass adds
constexpr int PX_PER_BLOCK = 1024;   // four pixels per thread before the grid stride starts

struct Args {
  float fac[MD2_JITTER_MAX_SAMPLES][4];   // brightness, contrast, saturation, hue
  uint32_t oa[MD2_JITTER_MAX_SAMPLES];    // order[j] in bits 2j..2j+1, apply in bit 8
};

inline int blocks_per_frame(int h, int w) {
  const int b = cdiv((long)h * w, PX_PER_BLOCK);
  return b > MAX_BLOCKS ? MAX_BLOCKS : b;
}

namespace {

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float blend(float a, float b, float t) { return clamp01(t * a + (1.f - t) * b); }
__device__ __forceinline__ float gray3(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

// rgb -> hsv, the hue shifted by `hue` turns, hsv -> rgb (md2.h, steps 1-9)
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float hue) {
  const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
  const bool eq = mx == mn;
  const float cr = mx - mn;
  const float s = __fdiv_rn(cr, eq ? 1.f : mx);
  const float d = eq ? 1.f : cr;
  const float rc = __fdiv_rn(mx - r, d), gc = __fdiv_rn(mx - g, d), bc = __fdiv_rn(mx - b, d);
  float hh = mx == r ? bc - gc : mx == g ? (2.f + rc) - bc : (4.f + gc) - rc;
  float t = __fdiv_rn(hh, 6.f) + 1.f;
  hh = t - floorf(t);
  t = hh + hue;
  hh = t - floorf(t);
  const float h6 = hh * 6.f;
  const float fi = floorf(h6);
  const float f = h6 - fi;
  const int i = (int)fi % 6;
  const float p = clamp01(mx * (1.f - s));
  const float q = clamp01(mx * (1.f - s * f));
  const float tt = clamp01(mx * (1.f - s * (1.f - f)));
  switch (i) {
    case 0: r = mx, g = tt, b = p; break;
    case 1: r = q, g = mx, b = p; break;
    case 2: r = p, g = mx, b = tt; break;
    case 3: r = p, g = q, b = mx; break;
    case 4: r = tt, g = p, b = mx; break;
    default: r = mx, g = p, b = q; break;
  }
}

template <int C>
__device__ __forceinline__ void apply_op(int op, float (&v)[C], const float* fac, float mean) {
  switch (op) {
    case 0:
#pragma unroll
      for (int k = 0; k < C; ++k) v[k] = clamp01(fac[0] * v[k]);
      break;
    case 1:
#pragma unroll
      for (int k = 0; k < C; ++k) v[k] = blend(v[k], mean, fac[1]);
      break;
    case 2:
      if (C == 3) {
        const float gr = gray3(v[0], v[C / 2], v[C - 1]);
#pragma unroll
        for (int k = 0; k < C; ++k) v[k] = blend(v[k], gr, fac[2]);
      }
      break;
    default:
      if (C == 3) hue_shift(v[0], v[C / 2], v[C - 1], fac[3]);
      break;
  }
}

template <int C>
__global__ __launch_bounds__(256) void reduce_kernel(const Args A, const float* __restrict__ x, int frames, int hw,
                                                     double* __restrict__ partials) {
  __shared__ double red[4];
  const int sample = blockIdx.z, frame = blockIdx.y;
  const uint32_t oa = A.oa[sample];
  if (!(oa >> 8)) return;   // the whole block: the apply pass reads no partial of this sample
  const float fac[4] = {A.fac[sample][0], A.fac[sample][1], A.fac[sample][2], A.fac[sample][3]};
  const size_t img = (size_t)sample * frames + frame;
  const float* src = x + img * C * hw;
  double acc[1] = {0.0};
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
    float v[C];
#pragma unroll
    for (int k = 0; k < C; ++k) v[k] = src[(size_t)k * hw + p];
    for (int j = 0; j < 4; ++j) {
      const int op = (oa >> (2 * j)) & 3;
      if (op == 1) break;
      apply_op<C>(op, v, fac, 0.f);
    }
    acc[0] += (double)(C == 3 ? gray3(v[0], v[C / 2], v[C - 1]) : v[0]);
  }
  block_sum256_d<1>(acc, red);
  if (threadIdx.x == 0) partials[img * gridDim.x + blockIdx.x] = acc[0];
}

template <int C>
__global__ __launch_bounds__(256) void apply_kernel(const Args A, const float* x, float* out, int frames, int hw,
                                                    const double* __restrict__ partials, float* __restrict__ means) {
  __shared__ float smean;
  const int sample = blockIdx.z, frame = blockIdx.y;
  const uint32_t oa = A.oa[sample];
  const size_t img = (size_t)sample * frames + frame;
  const float* src = x + img * C * hw;
  float* dst = out + img * C * hw;
  if (!(oa >> 8)) {
    if (means && blockIdx.x == 0 && threadIdx.x == 0) means[img] = 0.f;
    if (src == dst) return;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
#pragma unroll
      for (int k = 0; k < C; ++k) dst[(size_t)k * hw + p] = src[(size_t)k * hw + p];
    }
    return;
  }
  if (threadIdx.x == 0) {
    const double* part = partials + img * gridDim.x;
    double S = 0.0;
    for (unsigned k = 0; k < gridDim.x; ++k) S += part[k];
    const float m = (float)(S / (double)hw);
    smean = m;
    if (means && blockIdx.x == 0) means[img] = m;
  }
  __syncthreads();
  const float mean = smean;
  const float fac[4] = {A.fac[sample][0], A.fac[sample][1], A.fac[sample][2], A.fac[sample][3]};
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
    float v[C];
#pragma unroll
    for (int k = 0; k < C; ++k) v[k] = src[(size_t)k * hw + p];
    for (int j = 0; j < 4; ++j) apply_op<C>((oa >> (2 * j)) & 3, v, fac, mean);
#pragma unroll
    for (int k = 0; k < C; ++k) dst[(size_t)k * hw + p] = v[k];
  }
}

bool valid_sizes(int n, int frames, int h, int w) {
  return n >= 1 && n <= MD2_JITTER_MAX_SAMPLES && frames >= 1 && frames <= 65535 && h >= 1 && w >= 1 &&
         (long long)h * w <= (1LL << 24);
}

}  // namespace
}  // namespace jitter
}  // namespace md2

using namespace md2;
using namespace md2::jitter;

extern "C" {

size_t md2_color_jitter_workspace_size(int n, int frames, int h, int w) {
  if (!valid_sizes(n, frames, h, w)) return 0;
  return sizeof(double) * (size_t)n * frames * blocks_per_frame(h, w);
}

int md2_color_jitter(const float* x, int n, int frames, int c, int h, int w, const md2_jitter* params, float* out,
                     float* means, void* workspace, void* stream) {
  // validation first, without a HIP call
  MD2_CHECK_ARG(x && out && params && workspace, "color_jitter: null pointer");
  MD2_CHECK_ARG(n >= 1 && frames >= 1 && h >= 1 && w >= 1, "color_jitter: sizes must be at least 1");
  MD2_CHECK_ARG(n <= MD2_JITTER_MAX_SAMPLES, "color_jitter: n exceeds MD2_JITTER_MAX_SAMPLES");
  MD2_CHECK_ARG(frames <= 65535, "color_jitter: frames exceeds 65535");
  MD2_CHECK_ARG(c == 1 || c == 3, "color_jitter: c must be 1 or 3");
  MD2_CHECK_ARG((long long)h * w <= (1LL << 24), "color_jitter: h * w exceeds 2^24");
  MD2_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "color_jitter: workspace must be 8-byte aligned");
  Args A;
  for (int i = 0; i < n; ++i) {
    const md2_jitter& p = params[i];
    MD2_CHECK_ARG(std::isfinite(p.brightness) && std::isfinite(p.contrast) && std::isfinite(p.saturation) &&
                      std::isfinite(p.hue),
                  "color_jitter: a factor is not finite");
    MD2_CHECK_ARG(p.brightness >= 0.f && p.contrast >= 0.f && p.saturation >= 0.f,
                  "color_jitter: brightness, contrast and saturation must not be negative");
    MD2_CHECK_ARG(p.hue >= -0.5f && p.hue <= 0.5f, "color_jitter: |hue| exceeds 0.5");
    MD2_CHECK_ARG(p.apply == 0 || p.apply == 1, "color_jitter: apply must be 0 or 1");
    unsigned seen = 0, packed = 0;
    for (int j = 0; j < 4; ++j) {
      MD2_CHECK_ARG(p.order[j] < 4, "color_jitter: order is not a permutation of 0..3");
      seen |= 1u << p.order[j];
      packed |= (unsigned)p.order[j] << (2 * j);
    }
    MD2_CHECK_ARG(seen == 0xFu, "color_jitter: order is not a permutation of 0..3");
    A.fac[i][0] = p.brightness, A.fac[i][1] = p.contrast, A.fac[i][2] = p.saturation, A.fac[i][3] = p.hue;
    A.oa[i] = packed | ((unsigned)p.apply << 8);
  }
  const int hw = h * w;
  const size_t bytes = sizeof(float) * (size_t)n * frames * c * hw;
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  MD2_CHECK_ARG(xa == oa || xa + bytes <= oa || oa + bytes <= xa, "color_jitter: out overlaps x without being x");

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks_per_frame(h, w), frames, n);
  if (c == 3) {
    hipLaunchKernelGGL(reduce_kernel<3>, grid, dim3(256), 0, st, A, x, frames, hw, (double*)workspace);
    hipLaunchKernelGGL(apply_kernel<3>, grid, dim3(256), 0, st, A, x, out, frames, hw, (const double*)workspace,
                       means);
  } else {
    hipLaunchKernelGGL(reduce_kernel<1>, grid, dim3(256), 0, st, A, x, frames, hw, (double*)workspace);
    hipLaunchKernelGGL(apply_kernel<1>, grid, dim3(256), 0, st, A, x, out, frames, hw, (const double*)workspace,
                       means);
  }
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // extern "C"
