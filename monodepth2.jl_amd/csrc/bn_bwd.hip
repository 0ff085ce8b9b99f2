// BatchNorm backward (nn.h, BNBwd): g = dout [+ skip | summed from split-K slabs], ReLU-masked;
// dbeta = sum g, dgamma = sum g*xhat, dy = gamma*invstd*(g - dbeta/L - xhat*dgamma/L).  Two passes
// (per-block fp64 partials, then a finalise + apply), or one block per channel where it fits.
#include "bn_device.h"

namespace md2 {

// One block per (channel c, image group p), as bn_stats_partial_kernel walks the forward.
// SLAB: dout formed from the dgrad conv's split-K slabs (sum in split order = the conv's own
// reduction, bit-identical) and written to dout_w
// SKIP: dout + pd.skip over flat elements [pd.skip_lo, pd.skip_hi) (the decoder skip gradient,
// added where axpy used to add it before this pass; same fp add, bit-identical)
template <bool VEC, bool SLAB = false, bool SKIP = false>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(
    const float* __restrict__ dout, const float* __restrict__ mask, const float* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ mgamma,
    const float* __restrict__ mbeta, int C, int HW, int N, int parts, FastDiv fdu,
    double* __restrict__ part, SlabIn sl = SlabIn{}, float* __restrict__ dout_w = nullptr,
    SkipSrc pd = SkipSrc{}) {
  static_assert(!SKIP || (VEC && !SLAB), "SKIP: float4 units of a read dout");
  __shared__ double red[8];
  const int c = blockIdx.x, p = blockIdx.y;
  const int i0 = (int)((long)N * p / parts), i1 = (int)((long)N * (p + 1) / parts);
  const int U = VEC ? HW / 4 : HW;
  const uint32_t nu = (uint32_t)(i1 - i0) * U;
  const float mu = mean[c], is = invstd[c];
  const YMask ym = ymask(mgamma, mbeta, c, mu, is);
  const long sstride = (long)C * N * HW;
  double sg = 0.0, sgx = 0.0;
  // BN_INFLIGHT units per thread and trip (all loads in flight before any is used); the sums take
  // them in the same order as one unit per trip
  for (uint32_t e0 = threadIdx.x; e0 < nu; e0 += 256u * BN_INFLIGHT) {
    float4 gv[BN_INFLIGHT], yv[BN_INFLIGHT];
    bool live[BN_INFLIGHT];
#pragma unroll
    for (int h = 0; h < BN_INFLIGHT; ++h) {
      const uint32_t e = e0 + 256u * h;
      live[h] = e < nu;
      gv[h] = yv[h] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!live[h]) continue;
      const uint32_t im = fdiv(e, fdu), k = e - im * U;
      const long base = ((long)(i0 + im) * C + c) * HW;
      if (SLAB) {
        const long si = (long)c * N * HW + (long)(i0 + im) * HW + (VEC ? 4 * k : k);
        if (VEC) {
#pragma unroll 4
          for (int q = 0; q < sl.splits; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(sl.slab + q * sstride + si);
            gv[h].x += t.x; gv[h].y += t.y; gv[h].z += t.z; gv[h].w += t.w;
          }
          *reinterpret_cast<float4*>(dout_w + base + 4 * k) = gv[h];
        } else {
          for (int q = 0; q < sl.splits; ++q) gv[h].x += sl.slab[q * sstride + si];
          dout_w[base + k] = gv[h].x;
        }
      }
      if (VEC) {
        const long i = base + 4 * k;
        if (!SLAB) gv[h] = *reinterpret_cast<const float4*>(dout + i);
        if (SKIP) gv[h] = add_skip4(pd, (uint32_t)i, gv[h]);
        yv[h] = *reinterpret_cast<const float4*>(y + i);
        if (mask) {
          const float4 m = *reinterpret_cast<const float4*>(mask + i);
          if (!(m.x > 0.f)) gv[h].x = 0.f;
          if (!(m.y > 0.f)) gv[h].y = 0.f;
          if (!(m.z > 0.f)) gv[h].z = 0.f;
          if (!(m.w > 0.f)) gv[h].w = 0.f;
        }
      } else {
        const long i = base + k;
        if (!SLAB) gv[h].x = dout[i];
        yv[h].x = y[i];
        if (mask && !(mask[i] > 0.f)) gv[h].x = 0.f;
      }
    }
#pragma unroll
    for (int h = 0; h < BN_INFLIGHT; ++h) {
      if (!live[h]) continue;
      float4 g = gv[h];
      const float4 v = yv[h];
      if (VEC) {
        g.x = ymasked(g.x, v.x, ym);
        g.y = ymasked(g.y, v.y, ym);
        g.z = ymasked(g.z, v.z, ym);
        g.w = ymasked(g.w, v.w, ym);
        sg += (double)g.x + (double)g.y + (double)g.z + (double)g.w;
        sgx += (double)g.x * (double)((v.x - mu) * is) + (double)g.y * (double)((v.y - mu) * is) +
               (double)g.z * (double)((v.z - mu) * is) + (double)g.w * (double)((v.w - mu) * is);
      } else {
        g.x = ymasked(g.x, v.x, ym);
        sg += g.x;
        sgx += (double)g.x * (double)((v.x - mu) * is);
      }
    }
  }
  sg = wave_sum_d(sg);
  sgx = wave_sum_d(sgx);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[wid] = sg;
    red[4 + wid] = sgx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[((long)c * parts + p) * 2 + 0] = red[0] + red[1] + red[2] + red[3];
    part[((long)c * parts + p) * 2 + 1] = red[4] + red[5] + red[6] + red[7];
  }
}

// (b.gamma doubles as the mask re-derivation's gamma: ymask reads it only when b.mbeta is set)
int bn_bwd_partial(const BNBwd& b, int N, int C, long HW, BNStatsWs ws, hipStream_t st) {
  MD2_TRY(check_u31((long)N * C * HW));
  MD2_CHECK_ARG(ws.parts >= 1 && ws.parts <= N, "bn_bwd: parts must split the images");
  const int vec = HW % 4 == 0;
  const FastDiv fdu = fd(vec ? HW / 4 : HW);
  const SkipAdd& sk = b.skip;
  MD2_CHECK_ARG(!sk.skip || (vec && sk.lo >= 0 && sk.lo <= sk.hi && sk.hi <= (long)N * C * HW),
                "bn_bwd: skip range / HW % 4");
  if (sk.skip)
    hipLaunchKernelGGL((bn_bwd_partial_kernel<true, false, true>), dim3(C, ws.parts), dim3(256), 0,
                       st, b.dout, b.mask, b.y, b.mean, b.invstd, b.gamma, b.mbeta, C, (int)HW, N,
                       ws.parts, fdu, ws.partials, SlabIn{}, (float*)nullptr, skip_src(sk));
  else if (vec)
    hipLaunchKernelGGL(bn_bwd_partial_kernel<true>, dim3(C, ws.parts), dim3(256), 0, st, b.dout,
                       b.mask, b.y, b.mean, b.invstd, b.gamma, b.mbeta, C, (int)HW, N, ws.parts, fdu,
                       ws.partials);
  else
    hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, dim3(C, ws.parts), dim3(256), 0, st, b.dout,
                       b.mask, b.y, b.mean, b.invstd, b.gamma, b.mbeta, C, (int)HW, N, ws.parts, fdu,
                       ws.partials);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int bn_bwd_partial_slabs(const BNBwd& b, float* dout, int N, int C, long HW, BNStatsWs ws,
                         hipStream_t st) {
  MD2_TRY(check_u31((long)N * C * HW));
  MD2_CHECK_ARG(ws.parts >= 1 && ws.parts <= N, "bn_bwd: parts must split the images");
  const SlabIn& sl = b.slabs;
  MD2_CHECK_ARG(sl.slab && sl.splits >= 1 && dout, "bn_bwd_partial_slabs: slabs / output");
  const int vec = HW % 4 == 0;
  const FastDiv fdu = fd(vec ? HW / 4 : HW);
  if (vec)
    hipLaunchKernelGGL((bn_bwd_partial_kernel<true, true>), dim3(C, ws.parts), dim3(256), 0, st,
                       (const float*)nullptr, (const float*)nullptr, b.y, b.mean, b.invstd, b.gamma,
                       b.mbeta, C, (int)HW, N, ws.parts, fdu, ws.partials, sl, dout);
  else
    hipLaunchKernelGGL((bn_bwd_partial_kernel<false, true>), dim3(C, ws.parts), dim3(256), 0, st,
                       (const float*)nullptr, (const float*)nullptr, b.y, b.mean, b.invstd, b.gamma,
                       b.mbeta, C, (int)HW, N, ws.parts, fdu, ws.partials, sl, dout);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// ---- fused finalise + backward apply.  A block covers 256 * UPT consecutive units, i.e. up to
// 256 planes; wave w sums the backward partials of the channels of planes pl0+w, pl0+w+4, ... in
// one fixed order (lane l takes partials l, l+64, ..., then the wave reduction: the same dgamma /
// dbeta bits in every block), and the owner block of each channel (first unit of image 0's
// plane) stores dgamma[c] / dbeta[c].
template <bool VEC, bool SKIP = false, int UPT = 1>
__global__ __launch_bounds__(256) void bn_bwd_apply_fused_kernel(
    const float* __restrict__ dout, const float* __restrict__ mask, const float* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const double* __restrict__ part, int parts,
    float* __restrict__ dgamma, float* __restrict__ dbeta, uint32_t nu, FastDiv fdU, FastDiv fdC,
    float invL, float* __restrict__ dy, float* __restrict__ dres, int dres_acc,
    const float* __restrict__ mbeta, SkipSrc pd = SkipSrc{}) {
  static_assert(!SKIP || VEC, "SKIP: float4 units of a read dout");
  static_assert(VEC || UPT == 1, "scalar units: one per thread");
  __shared__ float s_k0[256], s_db[256], s_dg[256], s_mu[256], s_is[256], s_msc[256], s_msh[256];
  const uint32_t u0 = blockIdx.x * (256u * UPT);
  const uint32_t pl0 = fdiv(u0, fdU);
  const uint32_t npl = fdiv(min(u0 + 256u * UPT - 1u, nu - 1u), fdU) - pl0 + 1u;
  for (uint32_t t = threadIdx.x >> 6; t < npl; t += 4) {   // one wave per plane (see bn_finalise_plane)
    const uint32_t pl = pl0 + t;
    const int c = (int)(pl - fdiv(pl, fdC) * fdC.d);
    double sg = 0.0, sgx = 0.0;
    const double* q = part + (long)c * parts * 2;
    for (int p = threadIdx.x & 63; p < parts; p += 64) {
      sg += q[2 * p];
      sgx += q[2 * p + 1];
    }
    sg = wave_sum_d(sg);
    sgx = wave_sum_d(sgx);
    if ((threadIdx.x & 63) == 0) {
      const float dbf = (float)sg, dgf = (float)sgx;
      if (pl < fdC.d && pl * fdU.d >= u0) {
        dbeta[c] = dbf;
        dgamma[c] = dgf;
      }
      const float is = invstd[c];
      s_k0[t] = gamma[c] * is;
      s_db[t] = dbf * invL;
      s_dg[t] = dgf * invL;
      s_mu[t] = mean[c];
      s_is[t] = is;
      const YMask ym = ymask(gamma, mbeta, c, mean[c], is);
      s_msc[t] = ym.sc;
      s_msh[t] = ym.sh;
    }
  }
  __syncthreads();
  if (VEC) {
    // every load of the thread's UPT units in flight before the first is used
    float4 t[UPT], mv[UPT], v[UPT], qd[UPT];
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      const uint32_t u = u0 + threadIdx.x + 256u * j;
      const long i = 4L * (u < nu ? u : 0u);
      t[j] = *reinterpret_cast<const float4*>(dout + i);
      if (SKIP) t[j] = add_skip4(pd, (uint32_t)i, t[j]);
      if (mask) mv[j] = *reinterpret_cast<const float4*>(mask + i);
      v[j] = *reinterpret_cast<const float4*>(y + i);
      if (dres && dres_acc) qd[j] = *reinterpret_cast<const float4*>(dres + i);
    }
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      const uint32_t u = u0 + threadIdx.x + 256u * j;
      if (u >= nu) break;
      const long i = 4L * u;
      const uint32_t li = fdiv(u, fdU) - pl0;
      const float k0 = s_k0[li], db = s_db[li], dg = s_dg[li], mu = s_mu[li], is = s_is[li];
      const YMask ym{s_msc[li], s_msh[li], mbeta != nullptr};
      float g[4] = {t[j].x, t[j].y, t[j].z, t[j].w};
      if (mask) {
        const float4 m = mv[j];
        if (!(m.x > 0.f)) g[0] = 0.f;
        if (!(m.y > 0.f)) g[1] = 0.f;
        if (!(m.z > 0.f)) g[2] = 0.f;
        if (!(m.w > 0.f)) g[3] = 0.f;
      }
      const float yv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = ymasked(g[k], yv[k], ym);
      float r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = k0 * (g[k] - db - (yv[k] - mu) * is * dg);
      *reinterpret_cast<float4*>(dy + i) = make_float4(r[0], r[1], r[2], r[3]);
      if (dres) {
        float4 o = make_float4(g[0], g[1], g[2], g[3]);
        if (dres_acc) {
          const float4 q = qd[j];
          o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
        }
        *reinterpret_cast<float4*>(dres + i) = o;
      }
    }
  } else {
    const uint32_t u = u0 + threadIdx.x;
    if (u >= nu) return;
    const uint32_t li = fdiv(u, fdU) - pl0;
    const float k0 = s_k0[li], db = s_db[li], dg = s_dg[li], mu = s_mu[li], is = s_is[li];
    const YMask ym{s_msc[li], s_msh[li], mbeta != nullptr};
    float g = dout[u];
    if (mask && !(mask[u] > 0.f)) g = 0.f;
    g = ymasked(g, y[u], ym);
    const float xh = (y[u] - mu) * is;
    dy[u] = k0 * (g - db - xh * dg);
    if (dres) {
      if (dres_acc)
        dres[u] += g;
      else
        dres[u] = g;
    }
  }
}

int bn_bwd_apply_fused(const BNBwd& b, int N, int C, long HW, BNStatsWs ws, hipStream_t st) {
  const long n = (long)N * C * HW;
  MD2_TRY(check_u31(n));
  MD2_CHECK_ARG(ws.partials && ws.parts >= 1, "bn_bwd_apply_fused: missing partials");
  const SkipAdd& sk = b.skip;
  MD2_CHECK_ARG(!sk.skip || (HW % 4 == 0 && sk.lo >= 0 && sk.lo <= sk.hi && sk.hi <= n),
                "bn_bwd: skip range / HW % 4");
  const float invL = 1.f / (float)((long)N * HW);
  if (HW % 4 == 0) {
    const long nu = n / 4;
    const int upt = bn_upt(nu, HW / 4);
    const dim3 grid(cdiv(nu, 256L * upt));
#define MD2_BWDA(SK, U)                                                                           \
  hipLaunchKernelGGL((bn_bwd_apply_fused_kernel<true, SK, U>), grid, dim3(256), 0, st, b.dout, b.mask, \
                     b.y, b.mean, b.invstd, b.gamma, ws.partials, ws.parts, b.dgamma, b.dbeta,   \
                     (uint32_t)nu, fd(HW / 4), fd(C), invL, b.dy, b.dres, b.dres_accumulate,     \
                     b.mbeta, skip_src(sk))
    if (sk.skip) {
      if (upt == 8) MD2_BWDA(true, 8);
      else if (upt == 4) MD2_BWDA(true, 4);
      else if (upt == 2) MD2_BWDA(true, 2);
      else MD2_BWDA(true, 1);
    } else {
      if (upt == 8) MD2_BWDA(false, 8);
      else if (upt == 4) MD2_BWDA(false, 4);
      else if (upt == 2) MD2_BWDA(false, 2);
      else MD2_BWDA(false, 1);
    }
#undef MD2_BWDA
  } else
    hipLaunchKernelGGL(bn_bwd_apply_fused_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, st,
                       b.dout, b.mask, b.y, b.mean, b.invstd, b.gamma, ws.partials, ws.parts,
                       b.dgamma, b.dbeta, (uint32_t)n, fd(HW), fd(C), invL, b.dy, b.dres,
                       b.dres_accumulate, b.mbeta);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// ---- whole BN backward in one kernel when a channel fits in a block: one 1024-thread block per
// channel holds the channel's g (= dout [+ skip | summed from split-K slabs], ReLU-masked) and y
// in registers -- BN_CH_UNITS float4 units per thread -- sums them, stores dgamma/dbeta and
// applies, so each tensor is read once and the partials never leave the block.
// The fp64 sums run in one fixed order for every form (a thread's units in order, wave
// reduction, the waves in order): plain, SKIP and SLAB steps stay bit-identical to each other.  The
// apply spells its roundings out (no contraction that could differ between instantiations).
// Against the two-pass path the sums run in another order: dgamma/dbeta/dy agree to the last
// bits, not bitwise (as MD2_FUSE_BNSTATS for the forward).
template <bool SLAB, bool SKIP>
__global__ __launch_bounds__(BN_CH_THREADS) void bn_bwd_channel_kernel(
    const float* __restrict__ dout, const float* __restrict__ mask, const float* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ mbeta, int C, int N, FastDiv fdu,
    float invL, float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dy,
    float* __restrict__ dres, int dres_acc, SlabIn sl, SkipSrc pd) {
  static_assert(!(SLAB && SKIP), "SLAB: no skip addend (and no mask tensor)");
  constexpr int NW = BN_CH_THREADS / 64;
  __shared__ double red[2 * NW];
  const int c = blockIdx.x;
  const uint32_t U = fdu.d, HW = 4u * U, nu = (uint32_t)N * U;
  const float mu = mean[c], is = invstd[c];
  const YMask ym = ymask(gamma, mbeta, c, mu, is);
  const long sstride = (long)C * N * HW;
  float4 gv[BN_CH_UNITS], yv[BN_CH_UNITS];
  uint32_t off[BN_CH_UNITS];
  // every load of the channel in flight before the first is used
#pragma unroll
  for (int h = 0; h < BN_CH_UNITS; ++h) {
    const uint32_t e = threadIdx.x + (uint32_t)BN_CH_THREADS * h;
    gv[h] = yv[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    off[h] = 0;
    if (e >= nu) continue;
    const uint32_t im = fdiv(e, fdu), k = e - im * U;
    const uint32_t i = (im * (uint32_t)C + (uint32_t)c) * HW + 4u * k;
    off[h] = i;
    if (!SLAB) gv[h] = *reinterpret_cast<const float4*>(dout + i);
    if (SKIP) gv[h] = add_skip4(pd, i, gv[h]);
    yv[h] = *reinterpret_cast<const float4*>(y + i);
    if (mask) {
      const float4 m = *reinterpret_cast<const float4*>(mask + i);
      if (!(m.x > 0.f)) gv[h].x = 0.f;
      if (!(m.y > 0.f)) gv[h].y = 0.f;
      if (!(m.z > 0.f)) gv[h].z = 0.f;
      if (!(m.w > 0.f)) gv[h].w = 0.f;
    }
  }
  if (SLAB) {
    // split by split, a split's units all in flight: each element still adds its slabs in split
    // order from 0 (bn_bwd_partial_kernel<.., SLAB>'s order, the conv's own reduction)
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
        gv[h].x += t[h].x; gv[h].y += t[h].y; gv[h].z += t[h].z; gv[h].w += t[h].w;
      }
    }
  }
  double sg = 0.0, sgx = 0.0;
#pragma unroll
  for (int h = 0; h < BN_CH_UNITS; ++h) {
    if (threadIdx.x + (uint32_t)BN_CH_THREADS * h >= nu) continue;
    float4& g = gv[h];
    const float4 v = yv[h];
    g.x = ymasked(g.x, v.x, ym);
    g.y = ymasked(g.y, v.y, ym);
    g.z = ymasked(g.z, v.z, ym);
    g.w = ymasked(g.w, v.w, ym);
    // (the fp64 product of two floats is exact: an fma contraction changes no bit)
    sg += (double)g.x + (double)g.y + (double)g.z + (double)g.w;
    sgx += (double)g.x * (double)((v.x - mu) * is) + (double)g.y * (double)((v.y - mu) * is) +
           (double)g.z * (double)((v.z - mu) * is) + (double)g.w * (double)((v.w - mu) * is);
  }
  sg = wave_sum_d(sg);
  sgx = wave_sum_d(sgx);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[wid] = sg;
    red[NW + wid] = sgx;
  }
  __syncthreads();
  double tg = red[0], tgx = red[NW];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    tg += red[w];
    tgx += red[NW + w];
  }
  const float dbf = (float)tg, dgf = (float)tgx;
  if (threadIdx.x == 0) {
    dbeta[c] = dbf;
    dgamma[c] = dgf;
  }
  const float k0 = __fmul_rn(gamma[c], is), db = __fmul_rn(dbf, invL), dg = __fmul_rn(dgf, invL);
#pragma unroll
  for (int h = 0; h < BN_CH_UNITS; ++h) {
    if (threadIdx.x + (uint32_t)BN_CH_THREADS * h >= nu) continue;
    const uint32_t i = off[h];
    const float g[4] = {gv[h].x, gv[h].y, gv[h].z, gv[h].w};
    const float v[4] = {yv[h].x, yv[h].y, yv[h].z, yv[h].w};
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xh = __fmul_rn(__fsub_rn(v[k], mu), is);
      r[k] = __fmul_rn(k0, __fmaf_rn(-xh, dg, __fsub_rn(g[k], db)));
    }
    *reinterpret_cast<float4*>(dy + i) = make_float4(r[0], r[1], r[2], r[3]);
    if (dres) {
      float4 o = gv[h];
      if (dres_acc) {
        const float4 q = *reinterpret_cast<const float4*>(dres + i);
        o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
      }
      *reinterpret_cast<float4*>(dres + i) = o;
    }
  }
}

int bn_bwd_channel(const BNBwd& b, int N, int C, long HW, hipStream_t st) {
  const long n = (long)N * C * HW;
  MD2_TRY(check_u31(n));
  MD2_CHECK_ARG(bn_channel_fits(N, HW), "bn_bwd_channel: a channel must fit in a block");
  const SlabIn& sl = b.slabs;
  const SkipAdd& sk = b.skip;
  MD2_CHECK_ARG((sl.slab != nullptr) != (b.dout != nullptr) &&
                    (!sl.slab || (sl.splits >= 1 && !sk.skip && !b.mask)),
                "bn_bwd_channel: dout or slabs (slabs without skip / mask tensor)");
  MD2_CHECK_ARG(!sk.skip || (sk.lo >= 0 && sk.lo <= sk.hi && sk.hi <= n), "bn_bwd: skip range");
  const float invL = 1.f / (float)((long)N * HW);
#define MD2_BWDC(SL, SK)                                                                          \
  hipLaunchKernelGGL((bn_bwd_channel_kernel<SL, SK>), dim3(C), dim3(BN_CH_THREADS), 0, st, b.dout, \
                     b.mask, b.y, b.mean, b.invstd, b.gamma, b.mbeta, C, N, fd(HW / 4), invL,     \
                     b.dgamma, b.dbeta, b.dy, b.dres, b.dres_accumulate, sl, skip_src(sk))
  if (sl.slab) MD2_BWDC(true, false);
  else if (sk.skip) MD2_BWDC(false, true);
  else MD2_BWDC(false, false);
#undef MD2_BWDC
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
