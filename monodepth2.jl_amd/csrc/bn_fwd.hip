// BatchNorm forward (nn.h; Flux BatchNorm in trainmode!: batch statistics, biased variance,
// eps = 1e-5).  HBM-bound streaming kernels; the channel statistics are deterministic two-stage
// sums (per-block fp64 partials, finalised inside the apply pass), or one block per channel.
#include "bn_device.h"

namespace md2 {

int bn_parts(int C, long N, long HW) {
  long total = N * HW;
  int parts = (int)std::max(1L, std::min(1024L / std::max(1, C) + 1, total / 2048 + 1));
  return (int)std::min<long>(std::min(parts, 256), std::max(1L, N));   // parts split images
}

bool bn_channel_fits(int N, long HW) {
  return HW % 4 == 0 && (long)N * (HW / 4) <= (long)BN_CH_THREADS * BN_CH_UNITS;
}

// One block per (channel c, image group p): the group's images x HW elements of channel c,
// walked as a flat range (float4 units when HW % 4 == 0); fp64 accumulation.
// SLAB: y is not read but formed here from the split-K slabs of the conv that produced it
// (sum in split order = the conv's own reduction, bit-identical) and written to yout -- the
// conv's separate reduction launch and one read of y disappear
template <bool VEC, bool SLAB = false>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ y, int C,
                                                               int HW, int N, int parts,
                                                               FastDiv fdu, double* __restrict__ part,
                                                               SlabIn sl = SlabIn{},
                                                               float* __restrict__ yout = nullptr) {
  __shared__ double red[8];
  const int c = blockIdx.x, p = blockIdx.y;
  const int i0 = (int)((long)N * p / parts), i1 = (int)((long)N * (p + 1) / parts);
  const int U = VEC ? HW / 4 : HW;                 // units per image
  const uint32_t nu = (uint32_t)(i1 - i0) * U;
  const long sstride = (long)C * N * HW;           // one slab [C][N*HW]
  double s = 0.0, ss = 0.0;
  // BN_INFLIGHT units per thread and trip (all loads in flight first), summed in the one-unit order
  for (uint32_t e0 = threadIdx.x; e0 < nu; e0 += 256u * BN_INFLIGHT) {
    float4 vv[BN_INFLIGHT];
    bool live[BN_INFLIGHT];
#pragma unroll
    for (int h = 0; h < BN_INFLIGHT; ++h) {
      const uint32_t e = e0 + 256u * h;
      live[h] = e < nu;
      vv[h] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!live[h]) continue;
      const uint32_t im = fdiv(e, fdu), k = e - im * U;
      const long base = ((long)(i0 + im) * C + c) * HW;
      if (SLAB) {
        const long si = (long)c * N * HW + (long)(i0 + im) * HW + (VEC ? 4 * k : k);
        if (VEC) {
#pragma unroll 4
          for (int q = 0; q < sl.splits; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(sl.slab + q * sstride + si);
            vv[h].x += t.x; vv[h].y += t.y; vv[h].z += t.z; vv[h].w += t.w;
          }
          *reinterpret_cast<float4*>(yout + base + 4 * k) = vv[h];
        } else {
          for (int q = 0; q < sl.splits; ++q) vv[h].x += sl.slab[q * sstride + si];
          yout[base + k] = vv[h].x;
        }
      } else if (VEC) {
        vv[h] = *reinterpret_cast<const float4*>(y + base + 4 * k);
      } else {
        vv[h].x = y[base + k];
      }
    }
#pragma unroll
    for (int h = 0; h < BN_INFLIGHT; ++h) {
      if (!live[h]) continue;
      const float4 v = vv[h];
      if (VEC) {
        s += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
        ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
      } else {
        const double d = v.x;
        s += d;
        ss += d * d;
      }
    }
  }
  s = wave_sum_d(s);
  ss = wave_sum_d(ss);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[wid] = s;
    red[4 + wid] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[((long)c * parts + p) * 2 + 0] = red[0] + red[1] + red[2] + red[3];
    part[((long)c * parts + p) * 2 + 1] = red[4] + red[5] + red[6] + red[7];
  }
}

// one wave per channel, bn_finalise_plane's order: lane l sums partials l, l+64, ..., then the
// wave reduction
__global__ __launch_bounds__(64) void bn_partials_collapse_kernel(const double* __restrict__ part, int parts,
                                                                  double* __restrict__ out) {
  const int c = blockIdx.x;
  double a = 0.0, aa = 0.0;
  const double* q = part + (long)c * parts * 2;
  for (int p = threadIdx.x; p < parts; p += 64) {
    a += q[2 * p];
    aa += q[2 * p + 1];
  }
  a = wave_sum_d(a);
  aa = wave_sum_d(aa);
  if (threadIdx.x == 0) {
    out[2 * c] = a;
    out[2 * c + 1] = aa;
  }
}

int bn_partials_collapse(const double* part, int C, int parts, double* out, hipStream_t st) {
  MD2_CHECK_ARG(part && out && C >= 1 && parts >= 1, "bn_partials_collapse: arguments");
  hipLaunchKernelGGL(bn_partials_collapse_kernel, dim3(C), dim3(64), 0, st, part, parts, out);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int bn_stats_partial(const float* y, int N, int C, long HW, BNStatsWs ws, hipStream_t st) {
  MD2_TRY(check_u31((long)N * C * HW));
  MD2_CHECK_ARG(ws.parts >= 1 && ws.parts <= N, "bn_stats: parts must split the images");
  const int vec = HW % 4 == 0;
  const FastDiv fdu = fd(vec ? HW / 4 : HW);
  if (vec)
    hipLaunchKernelGGL(bn_stats_partial_kernel<true>, dim3(C, ws.parts), dim3(256), 0, st, y, C,
                       (int)HW, N, ws.parts, fdu, ws.partials);
  else
    hipLaunchKernelGGL(bn_stats_partial_kernel<false>, dim3(C, ws.parts), dim3(256), 0, st, y, C,
                       (int)HW, N, ws.parts, fdu, ws.partials);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int bn_stats_partial_slabs(SlabIn sl, float* y, int N, int C, long HW, BNStatsWs ws, hipStream_t st) {
  MD2_TRY(check_u31((long)N * C * HW));
  MD2_CHECK_ARG(ws.parts >= 1 && ws.parts <= N, "bn_stats: parts must split the images");
  MD2_CHECK_ARG(sl.slab && sl.splits >= 1 && y, "bn_stats_partial_slabs: slabs / output");
  const int vec = HW % 4 == 0;
  const FastDiv fdu = fd(vec ? HW / 4 : HW);
  if (vec)
    hipLaunchKernelGGL((bn_stats_partial_kernel<true, true>), dim3(C, ws.parts), dim3(256), 0, st,
                       (const float*)nullptr, C, (int)HW, N, ws.parts, fdu, ws.partials, sl, y);
  else
    hipLaunchKernelGGL((bn_stats_partial_kernel<false, true>), dim3(C, ws.parts), dim3(256), 0, st,
                       (const float*)nullptr, C, (int)HW, N, ws.parts, fdu, ws.partials, sl, y);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// ---- fused finalise + apply.  A block covers 256 * UPT consecutive units (float4 or scalar),
// i.e. the planes pl0..pl1 (plane = image*C + channel, <= 256 of them); wave w finalises the
// channels of planes pl0+w, pl0+w+4, ... from the partials (bn_finalise_plane: lane-parallel
// fixed-order sum + wave reduction, same result in every block), the scale/shift go through LDS.
// The block holding the first unit of image 0's plane of channel c writes mean[c], invstd[c] and
// the running statistics.
template <bool VEC, int UPT = 1>
__global__ __launch_bounds__(256) void bn_apply_fused_kernel(BNApplyFused p, float* __restrict__ out,
                                                             uint32_t nu, FastDiv fdU, FastDiv fdC,
                                                             double total) {
  __shared__ float s_sc[256], s_sh[256], s_sc2[256], s_sh2[256];
  const uint32_t u0 = blockIdx.x * (256u * UPT);
  const uint32_t pl0 = fdiv(u0, fdU);
  const uint32_t npl = fdiv(min(u0 + 256u * UPT - 1u, nu - 1u), fdU) - pl0 + 1u;
  // the block's loads are issued before the per-plane finalise (independent of it): its partial
  // sums -- up to one per 256-pixel tile when the conv epilogue took the statistics -- are read
  // while the tensor's bytes are in flight
  float4 v[UPT], q2[UPT], qr[UPT];
  if (VEC) {
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      const uint32_t u = u0 + threadIdx.x + 256u * j;
      const long i = 4L * (u < nu ? u : 0u);
      v[j] = *reinterpret_cast<const float4*>(p.y + i);
      if (p.y2) q2[j] = *reinterpret_cast<const float4*>(p.y2 + i);
      if (p.res) qr[j] = *reinterpret_cast<const float4*>(p.res + i);
    }
  }
  for (uint32_t t = threadIdx.x >> 6; t < npl; t += 4) {   // wave-uniform plane loop
    const uint32_t pl = pl0 + t;
    const int c = (int)(pl - fdiv(pl, fdC) * fdC.d);
    const bool owner = pl < fdC.d && pl * fdU.d >= u0;
    float sc, sh;
    bn_finalise_plane(p.s1, c, total, owner, sc, sh);
    float sc2 = 0.f, sh2 = 0.f;
    if (p.y2) bn_finalise_plane(p.s2, c, total, owner, sc2, sh2);
    if ((threadIdx.x & 63) == 0) {
      s_sc[t] = sc;
      s_sh[t] = sh;
      s_sc2[t] = sc2;
      s_sh2[t] = sh2;
    }
  }
  __syncthreads();
  if (VEC) {
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      const uint32_t u = u0 + threadIdx.x + 256u * j;
      if (u >= nu) break;
      const uint32_t li = fdiv(u, fdU) - pl0;
      const float sc = s_sc[li], sh = s_sh[li];
      float r[4] = {__fmaf_rn(v[j].x, sc, sh), __fmaf_rn(v[j].y, sc, sh), __fmaf_rn(v[j].z, sc, sh),
                    __fmaf_rn(v[j].w, sc, sh)};
      if (p.y2) {
        const float sc2 = s_sc2[li], sh2 = s_sh2[li];
        const float4 q = q2[j];
        r[0] += q.x * sc2 + sh2; r[1] += q.y * sc2 + sh2; r[2] += q.z * sc2 + sh2; r[3] += q.w * sc2 + sh2;
      }
      if (p.res) {
        const float4 q = qr[j];
        r[0] += q.x; r[1] += q.y; r[2] += q.z; r[3] += q.w;
      }
      if (p.relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = fmaxf(r[k], 0.f);
      }
      *reinterpret_cast<float4*>(out + 4L * u) = make_float4(r[0], r[1], r[2], r[3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      const uint32_t u = u0 + threadIdx.x + 256u * j;
      if (u >= nu) break;
      const uint32_t li = fdiv(u, fdU) - pl0;
      const float sc = s_sc[li], sh = s_sh[li];
      float r = __fmaf_rn(p.y[u], sc, sh);
      if (p.y2) r += p.y2[u] * s_sc2[li] + s_sh2[li];
      if (p.res) r += p.res[u];
      if (p.relu) r = fmaxf(r, 0.f);
      out[u] = r;
    }
  }
}

int bn_apply_fused(const BNApplyFused& p, float* out, int N, int C, long HW, hipStream_t st) {
  const long n = (long)N * C * HW;
  MD2_TRY(check_u31(n));
  MD2_CHECK_ARG(p.s1.part && p.s1.parts >= 1 && (!p.y2 || (p.s2.part && p.s2.parts >= 1)),
                "bn_apply_fused: missing statistics partials");
  const double total = (double)((long)N * HW);
  if (HW % 4 == 0) {
    const long nu = n / 4;
    const int upt = bn_upt(nu, HW / 4);
    const dim3 grid(cdiv(nu, 256L * upt));
    if (upt == 8)
      hipLaunchKernelGGL((bn_apply_fused_kernel<true, 8>), grid, dim3(256), 0, st, p, out, (uint32_t)nu,
                         fd(HW / 4), fd(C), total);
    else if (upt == 4)
      hipLaunchKernelGGL((bn_apply_fused_kernel<true, 4>), grid, dim3(256), 0, st, p, out, (uint32_t)nu,
                         fd(HW / 4), fd(C), total);
    else if (upt == 2)
      hipLaunchKernelGGL((bn_apply_fused_kernel<true, 2>), grid, dim3(256), 0, st, p, out, (uint32_t)nu,
                         fd(HW / 4), fd(C), total);
    else
      hipLaunchKernelGGL((bn_apply_fused_kernel<true, 1>), grid, dim3(256), 0, st, p, out, (uint32_t)nu,
                         fd(HW / 4), fd(C), total);
  } else {
    hipLaunchKernelGGL(bn_apply_fused_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, st, p, out,
                       (uint32_t)n, fd(HW), fd(C), total);
  }
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// ---- statistics and apply of a BN whose channel fits in a block (bn_channel_fits), in one
// kernel.  The block takes the channel's y into registers (SLAB: formed from the conv's split-K
// slabs in split order, as bn_stats_partial_kernel<.., SLAB> forms it, and stored -- the backward
// reads it), sums y and y^2 in fp64 (a thread's units in order, wave reduction, the 16 waves in
// order: one barrier), finalises through bn_finalise_sums like every other BN forward and applies
// with bn_apply_fused_kernel's expressions: y is read once and the partials never leave the block.
// The downsample branch's BN (p.y2) keeps its own statistics pass; its partials are finalised here
// by the last wave, behind the loads, and reach the others through the same barrier.  Thread 0
// and that wave's lane 0 are the owners of the channel's mean / invstd / running statistics.
template <bool SLAB>
__global__ __launch_bounds__(BN_CH_THREADS) void bn_fwd_channel_kernel(
    BNApplyFused p, float* yout, float* __restrict__ out, int C, int N, FastDiv fdu, double total,
    SlabIn sl) {
  constexpr int NW = BN_CH_THREADS / 64;
  __shared__ double red[2 * NW];
  __shared__ float s_two[2];
  const int c = blockIdx.x;
  const uint32_t U = fdu.d, HW = 4u * U, nu = (uint32_t)N * U;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float4 v[BN_CH_UNITS], q2[BN_CH_UNITS], qr[BN_CH_UNITS];
  uint32_t off[BN_CH_UNITS];
  // every load of the channel in flight before the first is used
#pragma unroll
  for (int h = 0; h < BN_CH_UNITS; ++h) {
    const uint32_t e = threadIdx.x + (uint32_t)BN_CH_THREADS * h;
    v[h] = q2[h] = qr[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    off[h] = 0;
    if (e >= nu) continue;
    const uint32_t im = fdiv(e, fdu), k = e - im * U;
    const uint32_t i = (im * (uint32_t)C + (uint32_t)c) * HW + 4u * k;
    off[h] = i;
    if (!SLAB) v[h] = *reinterpret_cast<const float4*>(p.y + i);
    if (p.y2) q2[h] = *reinterpret_cast<const float4*>(p.y2 + i);
    if (p.res) qr[h] = *reinterpret_cast<const float4*>(p.res + i);
  }
  if (SLAB) {
    // split by split, a split's units all in flight; each element adds its slabs to 0 in split order
    const long sstride = (long)C * N * HW;
    const float* sq = sl.slab + (long)c * N * HW;
    for (int q = 0; q < sl.splits; ++q, sq += sstride) {
      float4 t[BN_CH_UNITS];
#pragma unroll
      for (int h = 0; h < BN_CH_UNITS; ++h) {
        const uint32_t e = threadIdx.x + (uint32_t)BN_CH_THREADS * h;   // slab plane [N][HW]: 4 * e
        if (e < nu) t[h] = *reinterpret_cast<const float4*>(sq + 4u * e);
      }
#pragma unroll
      for (int h = 0; h < BN_CH_UNITS; ++h) {
        if (threadIdx.x + (uint32_t)BN_CH_THREADS * h >= nu) continue;
        v[h].x += t[h].x; v[h].y += t[h].y; v[h].z += t[h].z; v[h].w += t[h].w;
      }
    }
#pragma unroll
    for (int h = 0; h < BN_CH_UNITS; ++h) {
      if (threadIdx.x + (uint32_t)BN_CH_THREADS * h >= nu) continue;
      *reinterpret_cast<float4*>(yout + off[h]) = v[h];
    }
  }
  if (p.y2 && wid == NW - 1) {   // wave-uniform
    float a2, b2;
    bn_finalise_plane(p.s2, c, total, true, a2, b2);
    if (lane == 0) {
      s_two[0] = a2;
      s_two[1] = b2;
    }
  }
  double s = 0.0, ss = 0.0;
#pragma unroll
  for (int h = 0; h < BN_CH_UNITS; ++h) {
    if (threadIdx.x + (uint32_t)BN_CH_THREADS * h >= nu) continue;
    const float4 w = v[h];
    s += (double)w.x + (double)w.y + (double)w.z + (double)w.w;
    ss += (double)w.x * w.x + (double)w.y * w.y + (double)w.z * w.z + (double)w.w * w.w;
  }
  s = wave_sum_d(s);
  ss = wave_sum_d(ss);
  if (lane == 0) {
    red[wid] = s;
    red[NW + wid] = ss;
  }
  __syncthreads();
  double ts = red[0], tss = red[NW];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    ts += red[w];
    tss += red[NW + w];
  }
  float sc, sh;
  bn_finalise_sums(p.s1, c, ts, tss, total, threadIdx.x == 0, sc, sh);
  float sc2 = 0.f, sh2 = 0.f;
  if (p.y2) {
    sc2 = s_two[0];
    sh2 = s_two[1];
  }
#pragma unroll
  for (int h = 0; h < BN_CH_UNITS; ++h) {
    if (threadIdx.x + (uint32_t)BN_CH_THREADS * h >= nu) continue;
    float r[4] = {__fmaf_rn(v[h].x, sc, sh), __fmaf_rn(v[h].y, sc, sh), __fmaf_rn(v[h].z, sc, sh),
                  __fmaf_rn(v[h].w, sc, sh)};
    if (p.y2) {
      const float4 q = q2[h];
      r[0] += q.x * sc2 + sh2; r[1] += q.y * sc2 + sh2; r[2] += q.z * sc2 + sh2; r[3] += q.w * sc2 + sh2;
    }
    if (p.res) {
      const float4 q = qr[h];
      r[0] += q.x; r[1] += q.y; r[2] += q.z; r[3] += q.w;
    }
    if (p.relu) {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = fmaxf(r[k], 0.f);
    }
    *reinterpret_cast<float4*>(out + off[h]) = make_float4(r[0], r[1], r[2], r[3]);
  }
}

int bn_fwd_channel(SlabIn sl, float* y, const BNApplyFused& p, float* out, int N, int C, long HW,
                   hipStream_t st) {
  MD2_TRY(check_u31((long)N * C * HW));
  MD2_CHECK_ARG(bn_channel_fits(N, HW), "bn_fwd_channel: a channel must fit in a block");
  MD2_CHECK_ARG(out && (sl.slab ? sl.splits >= 1 && y != nullptr : p.y != nullptr),
                "bn_fwd_channel: y, or slabs and the y they are summed into");
  MD2_CHECK_ARG(p.s1.gamma && p.s1.beta && p.s1.mean && p.s1.invstd, "bn_fwd_channel: BN operands");
  MD2_CHECK_ARG(!p.y2 || (p.s2.part && p.s2.parts >= 1), "bn_fwd_channel: missing statistics partials");
  const double total = (double)((long)N * HW);
  if (sl.slab)
    hipLaunchKernelGGL(bn_fwd_channel_kernel<true>, dim3(C), dim3(BN_CH_THREADS), 0, st, p, y, out, C,
                       N, fd(HW / 4), total, sl);
  else
    hipLaunchKernelGGL(bn_fwd_channel_kernel<false>, dim3(C), dim3(BN_CH_THREADS), 0, st, p, y, out,
                       C, N, fd(HW / 4), total, sl);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// ResNet stem tail in one pass: BN (batch statistics finalised per block, bn_apply_fused's
// explicit roundings) + ReLU + MaxPool 3x3/2/pad 1.  One pooled output per thread: it evaluates
// relu(fma(y, sc, sh)) over its window (bit-identical to bn_apply_fused then maxpool_fwd), stores
// the window's own 2x2 block of the activation (rows 2oh..2oh+1, columns 2ow..2ow+1: every
// activation exactly once, even H and W) and the max / argmax -- the activation is written but
// never read back (the pool used to re-read it: one full read of the stem output less).
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(BNApplyFused p, float* __restrict__ act,
                                                              int H, int W, float* __restrict__ y,
                                                              unsigned char* __restrict__ arg,
                                                              FastDiv fdWo, FastDiv fdHo, FastDiv fdU,
                                                              FastDiv fdC, uint32_t n, double total) {
  __shared__ float s_sc[256], s_sh[256];
  const uint32_t u0 = blockIdx.x * 256u;
  const uint32_t pl0 = fdiv(u0, fdU);
  const uint32_t npl = fdiv(min(u0 + 255u, n - 1u), fdU) - pl0 + 1u;
  for (uint32_t t = threadIdx.x >> 6; t < npl; t += 4) {   // wave-uniform plane loop
    const uint32_t pl = pl0 + t;
    const int c = (int)(pl - fdiv(pl, fdC) * fdC.d);
    const bool owner = pl < fdC.d && pl * fdU.d >= u0;
    float sc, sh;
    bn_finalise_plane(p.s1, c, total, owner, sc, sh);
    if ((threadIdx.x & 63) == 0) {
      s_sc[t] = sc;
      s_sh[t] = sh;
    }
  }
  __syncthreads();
  const uint32_t i = u0 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = fdiv(i, fdWo), plane = fdiv(r, fdHo);
  const int ow = (int)(i - r * fdWo.d), oh = (int)(r - plane * fdHo.d);
  const float sc = s_sc[plane - pl0], sh = s_sh[plane - pl0];
  const uint32_t base = plane * (uint32_t)(H * W);
  const float* src = p.y + base;
  float best = -INFINITY;
  int bi = 0;
  const int iw = ow * 2;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = oh * 2 - 1 + kh;
    if (ih < 0) continue;                       // ih <= 2*oh + 1 < H (even H)
    const float* row = src + ih * W;
    float v0 = -INFINITY;
    if (iw > 0) v0 = fmaxf(__fmaf_rn(row[iw - 1], sc, sh), 0.f);
    const float2 t = *reinterpret_cast<const float2*>(row + iw);
    const float v1 = fmaxf(__fmaf_rn(t.x, sc, sh), 0.f);
    const float v2 = fmaxf(__fmaf_rn(t.y, sc, sh), 0.f);
    if (kh > 0) *reinterpret_cast<float2*>(act + base + ih * W + iw) = make_float2(v1, v2);
    // strict '>' in (kh, kw) scan order: the first maximum wins (NNlib maxpool)
    if (v0 > best) { best = v0; bi = kh * 3; }
    if (v1 > best) { best = v1; bi = kh * 3 + 1; }
    if (v2 > best) { best = v2; bi = kh * 3 + 2; }
  }
  y[i] = best;
  arg[i] = (unsigned char)bi;
}

int bn_relu_maxpool(const BNApplyFused& p, float* act, int N, int C, int H, int W, float* y,
                    unsigned char* arg, int Ho, int Wo, hipStream_t st) {
  MD2_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && Ho == H / 2 && Wo == W / 2,
                "bn_relu_maxpool: even input, 3x3/2 pad-1 output shape");
  MD2_CHECK_ARG(p.y && p.s1.part && p.s1.parts >= 1 && !p.y2 && !p.res && p.relu,
                "bn_relu_maxpool: BN+ReLU without residual / second branch");
  const long n = (long)N * C * Ho * Wo;
  MD2_TRY(check_u31((long)N * C * H * W));
  const double total = (double)((long)N * H * W);
  hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, p, act, H, W, y,
                     arg, fd(Wo), fd(Ho), fd((long)Ho * Wo), fd(C), (uint32_t)n, total);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
