// What the BatchNorm forward (bn_fwd.hip) and backward (bn_bwd.hip) kernels share: the launch
// constants, the statistics finalise and the ReLU-mask / skip-addend helpers of the backward.
// Every reduction here and in the two files is deterministic: fp64 sums in one fixed order.
#pragma once
#include "nn_util.h"

namespace md2 {

// units in flight per thread and trip in the BN reduction passes (all loads issued before the
// first is summed; the sums take the units in the one-unit-per-trip order: bit-identical)
constexpr int BN_INFLIGHT = 4;

// Units per thread of the fused apply passes: a block covers 256 * UPT consecutive units, so the
// per-block finalise (one wave per plane) is paid once per 256 * UPT units and a thread has UPT
// independent loads in flight.  UPT only regroups the same per-element arithmetic (bit-identical
// for every UPT).  The host picks the largest UPT that keeps >= BN_MIN_BLOCKS blocks and the
// block's plane count within the 256-entry LDS tables.
constexpr int BN_MIN_BLOCKS = 1024;
static inline int bn_upt(long units, long U) {
  int upt = 8;
  while (upt > 1 && (units / (256L * upt) < BN_MIN_BLOCKS || 256L * upt / U + 2 > 256)) upt /= 2;
  return upt;
}

// The one-kernel passes (bn_fwd_channel, bn_bwd_channel): one 1024-thread block per channel holds
// the channel in registers, BN_CH_UNITS float4 units per thread.  16 waves x 2 units: 8192 values
// per channel.  (4 waves x 8 units left the split-K slab form of the backward at 21-23 us per
// launch on layers 3-4, against 17.5: a round trip per split with 4 waves per CU to hide it; the
// step measured 6.255 against 6.266 ms, profiles/bn_bwd_channel_ab.txt.)
constexpr int BN_CH_THREADS = 1024;
constexpr int BN_CH_UNITS = 2;

// From a channel's fp64 sums (a = sum y, aa = sum y^2 over `total` values) to the scale / shift of
// the apply; the thread with `store` set writes mean, invstd and the running statistics.  The one
// copy of these roundings: bn_finalise_plane and bn_fwd_channel_kernel both end here, and the
// backward re-derives the ReLU mask from y with the same operations.
__device__ __forceinline__ void bn_finalise_sums(const BNStatsIn& s, int c, double a, double aa,
                                                 double total, bool store, float& sc, float& sh) {
  const double mu = a / total;
  const double var = fmax(aa / total - mu * mu, 0.0);
  const float meanf = (float)mu;
  const float isf = (float)(1.0 / sqrt(var + (double)s.eps));
  // explicit roundings: bn_bwd_* re-derive relu(y*sc + sh) > 0 from y with the same operations
  sc = __fmul_rn(s.gamma[c], isf);
  sh = __fmaf_rn(-meanf, sc, s.beta[c]);
  if (store) {
    s.mean[c] = meanf;
    s.invstd[c] = isf;
    if (s.run_mean) {
      const float m = s.momentum;
      s.run_mean[c] = (1.f - m) * s.run_mean[c] + m * meanf;
      s.run_var[c] = (1.f - m) * s.run_var[c] + m * (float)(var * total / fmax(total - 1.0, 1.0));
    }
  }
}

// called by a whole wave: lane l sums partials l, l+64, ... (fixed order), then a wave reduction
// -- one partial-load latency per plane instead of `parts` dependent ones
__device__ __forceinline__ void bn_finalise_plane(const BNStatsIn& s, int c, double total,
                                                  bool owner, float& sc, float& sh) {
  double a = 0.0, aa = 0.0;
  const double* q = s.part + (long)c * s.parts * 2;
  for (int p = threadIdx.x & 63; p < s.parts; p += 64) {
    a += q[2 * p];
    aa += q[2 * p + 1];
  }
  a = wave_sum_d(a);
  aa = wave_sum_d(aa);
  bn_finalise_sums(s, c, a, aa, total, owner && (threadIdx.x & 63) == 0, sc, sh);
}

// ReLU mask of a BN+ReLU output without a residual, re-derived from the pre-BN y: the forward's
// relu(fma(y, sc, sh)) with sc = gamma*invstd, sh = beta - mean*sc in the same explicit roundings
// (bn_finalise_sums), so the mask is bit-identical and the activation is not read back
struct YMask {
  float sc, sh;
  bool on;
};
__device__ __forceinline__ YMask ymask(const float* mgamma, const float* mbeta, int c, float mu, float is) {
  YMask m{0.f, 0.f, mbeta != nullptr};
  if (m.on) {
    m.sc = __fmul_rn(mgamma[c], is);
    m.sh = __fmaf_rn(-mu, m.sc, mbeta[c]);
  }
  return m;
}
__device__ __forceinline__ float ymasked(float g, float y, const YMask& m) {
  return (m.on && !(__fmaf_rn(y, m.sc, m.sh) > 0.f)) ? 0.f : g;
}

__device__ __forceinline__ float4 add_skip4(const SkipSrc& q, uint32_t i, float4 g) {
  if (i >= q.skip_lo && i < q.skip_hi) {
    const float4 k = *reinterpret_cast<const float4*>(q.skip + (i - q.skip_lo));
    g.x += k.x; g.y += k.y; g.z += k.z; g.w += k.w;
  }
  return g;
}

}  // namespace md2
