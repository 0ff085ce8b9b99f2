// md2_lidar_depth: a batch of Velodyne scans rasterised into ground-truth depth maps (project,
// round, "minus one", nearest point wins), and md2_disp_post_process: the flip blend of Monodepth's
// "+pp" evaluation.  include/md2.h states the semantics of both.
//
// Built with -ffp-contract=off: every product and sum below is rounded on its own, in the order the
// header gives, so the float32 NumPy restatement of the tests gets the same bits.
//
// Passes of md2_lidar_depth, each over all scans (scan index on a grid axis):
//   memset    depth := all-ones words, the largest unsigned key (a NaN pattern no point can store)
//   scatter   one thread per point, grid stride over the scan: one 16-byte load, the projection, and
//             atomicMin on the pixel's unsigned bit pattern -- positive finite floats order as
//             their bit patterns do.  Stored points are counted per wave, one integer atomic each.
//   finish    all-ones -> 0.0f; hit pixels counted per block, one integer atomic each
// Integer atomics only and no floating-point sum: the result does not depend on arrival order and
// is bitwise reproducible.  offsets and P travel by value in the scatter kernel's arguments
// (3.3 KB at MD2_LIDAR_MAX_SCANS), so there is no workspace, no copy and no host synchronisation.
#include "common.h"

#include <cmath>

namespace md2 {
namespace lidar {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr int MAX_GRID = 4096;   // blocks of one launch, all scans together

struct Scans {
  int off[MD2_LIDAR_MAX_SCANS + 1];    // offsets <= 2^27 fit
  float P[MD2_LIDAR_MAX_SCANS][12];
};

namespace {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void scatter_kernel(const Scans S, const float4* __restrict__ points,
                                                      uint32_t* __restrict__ depth, int* __restrict__ counts,
                                                      int h, int w, int forward_only, int vel_depth) {
  const int img = blockIdx.y;
  const int begin = S.off[img], end = S.off[img + 1];
  const float* p = S.P[img];
  const float p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5], p6 = p[6], p7 = p[7],
              p8 = p[8], p9 = p[9], p10 = p[10], p11 = p[11];
  const float fw = (float)w, fh = (float)h;   // exact: h * w <= 2^24
  uint32_t* out = depth + (size_t)img * h * w;
  int stored = 0;
  // every lane of a wave runs the same number of rounds, so the shuffle below sees all 64
  for (int base = begin + blockIdx.x * 256; base < end; base += gridDim.x * 256) {
    const int i = base + threadIdx.x;
    if (i >= end) continue;
    const float4 q = points[i];
    const float X = q.x, Y = q.y, Z = q.z;
    const float x = ((p0 * X + p1 * Y) + p2 * Z) + p3;
    const float y = ((p4 * X + p5 * Y) + p6 * Z) + p7;
    const float zc = ((p8 * X + p9 * Y) + p10 * Z) + p11;
    const float u = __fdiv_rn(x, zc), v = __fdiv_rn(y, zc);
    const float ru = rintf(u), rv = rintf(v);   // ties to even
    const float s = vel_depth ? X : zc;
    // every comparison is false for a NaN; the pixel test is on the floats, so a huge u cannot wrap
    const bool keep = !(forward_only && X < 0.f) && s > 0.f && s <= 3.402823466e38f && zc > 0.f &&
                      zc <= 3.402823466e38f && ru >= 1.f && ru <= fw && rv >= 1.f && rv <= fh;
    if (keep) {
      const int ix = (int)ru - 1, iy = (int)rv - 1;
      atomicMin(&out[iy * w + ix], __float_as_uint(s));
      ++stored;
    }
  }
  if (counts) {
    stored = wave_sum_i(stored);
    if ((threadIdx.x & 63) == 0 && stored) atomicAdd(&counts[2 * img], stored);
  }
}

__global__ __launch_bounds__(256) void finish_kernel(uint32_t* __restrict__ depth, int* __restrict__ counts,
                                                     int npix) {
  __shared__ int red[4];
  const int img = blockIdx.y;
  uint32_t* d = depth + (size_t)img * npix;
  int hit = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    if (d[i] == EMPTY)
      d[i] = 0u;   // 0.0f
    else
      ++hit;
  }
  if (!counts) return;
  hit = wave_sum_i(hit);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = hit;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = red[0] + red[1] + red[2] + red[3];
    if (t) atomicAdd(&counts[2 * img + 1], t);
  }
}

// the left ramp of the flip blend at column x: 1 on the left 5 %, down to 0 at 10 %
__device__ __forceinline__ float ramp(int x, int w) {
  const float t = w > 1 ? __fdiv_rn((float)x, (float)(w - 1)) : 0.f;
  return 1.f - fminf(fmaxf(20.f * (t - 0.05f), 0.f), 1.f);
}

__global__ __launch_bounds__(256) void post_process_kernel(const float* disp, const float* __restrict__ flipped,
                                                           float* out, int w, long rows) {
  // one thread per pixel of a row chunk: blockIdx.y strides the rows, x the columns
  for (long row = blockIdx.y; row < rows; row += gridDim.y) {
    for (int x = blockIdx.x * 256 + threadIdx.x; x < w; x += gridDim.x * 256) {
      const float l = disp[row * w + x], r = flipped[row * w + (w - 1 - x)];
      const float ml = ramp(x, w), mr = ramp(w - 1 - x, w);
      out[row * w + x] = (mr * l + ml * r) + ((1.f - ml) - mr) * (0.5f * (l + r));
    }
  }
}

}  // namespace
}  // namespace lidar
}  // namespace md2

using namespace md2;
using namespace md2::lidar;

extern "C" {

int md2_lidar_depth(const md2_lidar_cfg* cfg, const float* points, const long long* offsets, const float* P,
                    float* depth, int* counts, void* stream) {
  // validation first, without a HIP call
  MD2_CHECK_ARG(cfg, "lidar_depth: null cfg");
  MD2_CHECK_ARG(offsets && P && depth, "lidar_depth: null pointer");
  const md2_lidar_cfg& c = *cfg;
  MD2_CHECK_ARG(c.n >= 1 && c.n <= MD2_LIDAR_MAX_SCANS, "lidar_depth: n must be in 1..64");
  MD2_CHECK_ARG(c.h >= 1 && c.w >= 1, "lidar_depth: sizes must be at least 1");
  MD2_CHECK_ARG((long long)c.h * c.w <= (1LL << 24), "lidar_depth: h * w exceeds 2^24");
  MD2_CHECK_ARG((c.forward_only == 0 || c.forward_only == 1) && (c.vel_depth == 0 || c.vel_depth == 1),
                "lidar_depth: forward_only and vel_depth must be 0 or 1");
  MD2_CHECK_ARG(offsets[0] >= 0, "lidar_depth: offsets[0] is negative");
  for (int i = 0; i < c.n; ++i)
    MD2_CHECK_ARG(offsets[i + 1] >= offsets[i], "lidar_depth: offsets must not decrease");
  MD2_CHECK_ARG(offsets[c.n] <= (1LL << 27), "lidar_depth: offsets[n] exceeds 2^27");
  MD2_CHECK_ARG(points || offsets[c.n] == 0, "lidar_depth: null points");
  MD2_CHECK_ARG(((uintptr_t)points & 15) == 0, "lidar_depth: points must be 16-byte aligned");
  for (int i = 0; i < c.n * 12; ++i) MD2_CHECK_ARG(std::isfinite(P[i]), "lidar_depth: P has a non-finite entry");

  hipStream_t st = (hipStream_t)stream;
  const int npix = c.h * c.w;
  const int cap = MAX_GRID / c.n;   // >= 64
  Scans S;
  long long longest = 0;
  for (int i = 0; i <= c.n; ++i) S.off[i] = (int)offsets[i];
  for (int i = 0; i < c.n; ++i) {
    if (offsets[i + 1] - offsets[i] > longest) longest = offsets[i + 1] - offsets[i];
    for (int k = 0; k < 12; ++k) S.P[i][k] = P[i * 12 + k];
  }

  MD2_HIP(hipMemsetAsync(depth, 0xFF, sizeof(float) * (size_t)c.n * npix, st));
  if (counts) MD2_HIP(hipMemsetAsync(counts, 0, sizeof(int) * 2 * (size_t)c.n, st));
  if (longest > 0) {
    const long gx = (longest + 255) / 256;
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)(gx > cap ? cap : gx), c.n), dim3(256), 0, st, S,
                       (const float4*)points, (uint32_t*)depth, counts, c.h, c.w, c.forward_only, c.vel_depth);
  }
  const int gp = cdiv(npix, 1024);   // 4 pixels per thread before the grid stride starts
  hipLaunchKernelGGL(finish_kernel, dim3(gp > cap ? cap : gp, c.n), dim3(256), 0, st, (uint32_t*)depth, counts,
                     npix);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int md2_disp_post_process(const float* disp, const float* disp_flipped, int n, int h, int w, float* out,
                          void* stream) {
  MD2_CHECK_ARG(disp && disp_flipped && out, "disp_post_process: null pointer");
  MD2_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "disp_post_process: sizes must be at least 1");
  MD2_CHECK_ARG((long long)n * h * w <= (1LL << 40), "disp_post_process: n * h * w exceeds 2^40");
  MD2_CHECK_ARG(out != disp_flipped, "disp_post_process: out must not alias disp_flipped");
  const long rows = (long)n * h;
  const int gx = cdiv(w, 256);
  const long gy = rows < 65535 / gx ? rows : 65535 / gx;
  hipLaunchKernelGGL(post_process_kernel, dim3(gx > 65535 ? 65535 : gx, (unsigned)(gy < 1 ? 1 : gy)), dim3(256), 0,
                     (hipStream_t)stream, disp, disp_flipped, out, w, rows);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // extern "C"
