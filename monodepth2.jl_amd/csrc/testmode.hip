// BatchNorm test mode kernels (testmode.h): the statistics check of md2_model_set_bn_stats, the
// batched BatchNorm-into-conv fold, the stem tail (affine + ReLU + max pool) and the block tail
// (residual add + ReLU).  All four are memory-bound streaming passes: 16-byte accesses, >= 4
// independent loads per thread, 64-bit element offsets.
#include "testmode.h"

#include <algorithm>
#include <cmath>

namespace md2 {

namespace {

__global__ __launch_bounds__(256) void bn_stats_validate_kernel(const float* __restrict__ stats,
                                                                BNStatLayout L, int* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L.off[L.n]) return;
  int lo = 0, hi = L.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (L.off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int C = (L.off[lo + 1] - L.off[lo]) / 2;
  const bool is_var = i - L.off[lo] >= C;
  const float v = stats[i];
  // !(v >= 0) also catches a NaN variance
  if (!isfinite(v) || (is_var && !(v >= 0.f))) *flag = 1;   // same value from every writer
}

// s and t of one channel, formed in fp64 and rounded once (like the warp maps of the loss tail)
__device__ __forceinline__ double fold_scale(const FoldJob& j, int c, double eps) {
  return (double)j.gamma[c] / sqrt((double)j.var[c] + eps);
}

constexpr int FOLD_UPT = 4;   // float4 units per thread

__global__ __launch_bounds__(256) void bn_fold_kernel(const FoldJob* __restrict__ jobs, int njobs,
                                                      double eps) {
  __shared__ int s_job;
  if (threadIdx.x == 0) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (jobs[mid].block_begin <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_job = lo;
  }
  __syncthreads();
  const FoldJob& j = jobs[__builtin_amdgcn_readfirstlane(s_job)];
  const long blk = (long)blockIdx.x - j.block_begin;
  if (blk == 0) {   // the job's first block also writes its (s, t) vectors
    for (int c = threadIdx.x; c < j.Cout; c += 256) {
      const double s = fold_scale(j, c, eps);
      j.s[c] = (float)s;
      j.t[c] = (float)((double)j.beta[c] - (double)j.mean[c] * s);
    }
  }
  if (!j.w) return;
  const long nu = (long)j.Cout * j.per4;
  const long u0 = blk * (256L * FOLD_UPT) + threadIdx.x;
  float4 v[FOLD_UPT];
  float s[FOLD_UPT];
#pragma unroll
  for (int k = 0; k < FOLD_UPT; ++k) {
    const long u = u0 + 256L * k;
    const long uc = u < nu ? u : 0;
    v[k] = *reinterpret_cast<const float4*>(j.w + 4 * uc);
    s[k] = (float)fold_scale(j, (int)(uc / j.per4), eps);
  }
#pragma unroll
  for (int k = 0; k < FOLD_UPT; ++k) {
    const long u = u0 + 256L * k;
    if (u >= nu) break;
    *reinterpret_cast<float4*>(j.wf + 4 * u) =
        make_float4(v[k].x * s[k], v[k].y * s[k], v[k].z * s[k], v[k].w * s[k]);
  }
}

// One thread owns input columns [4q, 4q+4) of rows 2oh-1 .. 2oh+1 (one float4 and the left
// neighbour per row: six loads in flight): it stores the activation of rows 2oh and 2oh+1 as two
// float4 (every activation exactly once, even H) and the two pooled outputs (oh, 2q), (oh, 2q+1)
// as one float2 -- the tiling of bn_relu_maxpool_kernel, twice as wide.
__global__ __launch_bounds__(256) void affine_relu_maxpool_kernel(
    const float* __restrict__ y, const float* __restrict__ sc, const float* __restrict__ sh,
    float* __restrict__ act, float* __restrict__ pool, int C, int H, int W, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int Wq = W >> 2, Ho = H >> 1, Wo = W >> 1;
  const long r = i / Wq;
  const int q = (int)(i - r * Wq);
  const long plane = r / Ho;
  const int oh = (int)(r - plane * Ho);
  const int c = (int)(plane % C);
  const float s = sc[c], t = sh[c];
  const long base = plane * ((long)H * W);
  const int iw = 4 * q;
  float4 v[3];
  float l[3];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = 2 * oh - 1 + kh;             // ih <= 2*oh + 1 < H (even H)
    const float* row = y + base + (long)max(ih, 0) * W + iw;
    v[kh] = *reinterpret_cast<const float4*>(row);
    l[kh] = iw > 0 ? row[-1] : 0.f;
  }
  float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = 2 * oh - 1 + kh;
    if (ih < 0) continue;                       // the padding row
    const float a0 = fmaxf(__fmaf_rn(v[kh].x, s, t), 0.f), a1 = fmaxf(__fmaf_rn(v[kh].y, s, t), 0.f);
    const float a2 = fmaxf(__fmaf_rn(v[kh].z, s, t), 0.f), a3 = fmaxf(__fmaf_rn(v[kh].w, s, t), 0.f);
    if (kh > 0) *reinterpret_cast<float4*>(act + base + (long)ih * W + iw) = make_float4(a0, a1, a2, a3);
    if (iw > 0) m0 = fmaxf(m0, fmaxf(__fmaf_rn(l[kh], s, t), 0.f));
    m0 = fmaxf(m0, fmaxf(a0, a1));
    m1 = fmaxf(m1, fmaxf(a1, fmaxf(a2, a3)));
  }
  *reinterpret_cast<float2*>(pool + plane * ((long)Ho * Wo) + (long)oh * Wo + 2 * q) = make_float2(m0, m1);
}

constexpr int ADD_UPT = 4;   // float4 units per thread and operand: 8 loads in flight

__global__ __launch_bounds__(256) void add_relu_kernel(const float* __restrict__ a,
                                                       const float* __restrict__ b,
                                                       float* __restrict__ out, long nu) {
  const long u0 = (long)blockIdx.x * (256L * ADD_UPT) + threadIdx.x;
  float4 va[ADD_UPT], vb[ADD_UPT];
#pragma unroll
  for (int k = 0; k < ADD_UPT; ++k) {
    const long u = u0 + 256L * k;
    const long uc = u < nu ? u : 0;
    va[k] = *reinterpret_cast<const float4*>(a + 4 * uc);
    vb[k] = *reinterpret_cast<const float4*>(b + 4 * uc);
  }
#pragma unroll
  for (int k = 0; k < ADD_UPT; ++k) {
    const long u = u0 + 256L * k;
    if (u >= nu) break;
    *reinterpret_cast<float4*>(out + 4 * u) =
        make_float4(fmaxf(va[k].x + vb[k].x, 0.f), fmaxf(va[k].y + vb[k].y, 0.f),
                    fmaxf(va[k].z + vb[k].z, 0.f), fmaxf(va[k].w + vb[k].w, 0.f));
  }
}

}  // namespace

int bn_stats_validate(const float* stats, const BNStatLayout& L, int* flag, hipStream_t st) {
  MD2_CHECK_ARG(stats && flag && L.n >= 1 && L.n <= MAX_BN, "bn_stats_validate args");
  hipLaunchKernelGGL(bn_stats_validate_kernel, dim3(cdiv(L.off[L.n], 256)), dim3(256), 0, st, stats, L,
                     flag);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

long bn_fold_job_blocks(const FoldJob& j) {
  return j.w ? std::max<long>(1, cdiv((long)j.Cout * j.per4, 256L * FOLD_UPT)) : 1;
}

int bn_fold_batch(const FoldJob* dev_jobs, int njobs, long total_blocks, double eps, hipStream_t st) {
  if (njobs == 0) return MD2_OK;
  MD2_CHECK_ARG(dev_jobs && total_blocks >= njobs && total_blocks < (1L << 31), "bn_fold_batch args");
  hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, dev_jobs, njobs, eps);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int affine_relu_maxpool(const float* y, const float* s, const float* t, int N, int C, int H, int W,
                        float* act, float* pool, hipStream_t st) {
  MD2_CHECK_ARG(y && s && t && act && pool && N >= 1 && C >= 1, "affine_relu_maxpool pointers");
  MD2_CHECK_ARG(H >= 2 && H % 2 == 0 && W >= 4 && W % 4 == 0, "affine_relu_maxpool: even H, W % 4 == 0");
  const long n = (long)N * C * (H / 2) * (W / 4);
  const long blocks = (n + 255) / 256;
  MD2_CHECK_ARG(blocks < (1L << 31), "affine_relu_maxpool: tensor too large");
  hipLaunchKernelGGL(affine_relu_maxpool_kernel, dim3((unsigned)blocks), dim3(256), 0, st, y, s, t, act,
                     pool, C, H, W, n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int add_relu(const float* a, const float* b, float* out, long n, hipStream_t st) {
  MD2_CHECK_ARG(a && b && out && n >= 4 && n % 4 == 0, "add_relu: n % 4 == 0");
  const long nu = n / 4;
  const long blocks = (nu + 256L * ADD_UPT - 1) / (256L * ADD_UPT);
  MD2_CHECK_ARG(blocks < (1L << 31), "add_relu: tensor too large");
  hipLaunchKernelGGL(add_relu_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, nu);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
