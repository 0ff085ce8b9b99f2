// The forward / data-gradient kernels, their split-K reduction and launchers: shared by conv_fwd.hip
// (launch_px<0>) and conv_dgrad.hip (launch_px<1>).
#pragma once
#include "conv_plan.h"

namespace md2 {

#include "conv_px.inc"
#include "conv_px2.inc"
#include "conv_px16.inc"
#include "conv_px3.inc"

// split-K reduction + epilogue for fwd / dgrad, four consecutive pixels of one output plane per
// thread (plain output mapping, pixels per image % 4 == 0): float4 slab loads, one store
template <int P_ = 0>
__global__ __launch_bounds__(256) void splitk_reduce_px4_kernel(ConvArgs a, int splits) {
  const long idx = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
  const long total = (long)a.g.M * a.g.N;
  if (idx >= total) return;
  const int m = (int)(idx / a.g.N);
  const long nn = idx - (long)m * a.g.N;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int s = 0; s < splits; ++s) {
    const float4 t = *reinterpret_cast<const float4*>(a.slab + (long)s * total + idx);
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  const TensorOut& o = a.out;
  const int img = (int)fdiv((uint32_t)nn, a.fd_pix);
  const long pix = nn - (long)img * a.fd_pix.d, HoWo = a.fd_pix.d;
  float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (o.bias) r[q] += o.bias[m];
    r[q] = apply_act(r[q], o.act);
  }
  float* dst = (m < o.c0) ? o.p0 + (long)img * o.bs0 + (long)m * HoWo + pix
                          : o.p1 + (long)img * o.bs1 + (long)(m - o.c0) * HoWo + pix;
  float4 w = make_float4(r[0], r[1], r[2], r[3]);
  if (o.accumulate) {
    const float4 d = *reinterpret_cast<const float4*>(dst);
    w.x = d.x + w.x; w.y = d.y + w.y; w.z = d.z + w.z; w.w = d.w + w.w;
  }
  *reinterpret_cast<float4*>(dst) = w;
}

// split-K reduction + epilogue for fwd / dgrad (32-bit index math with magic-number divisions --
// the 64-bit divisions cost 10-22 us per stride-2 dgrad -- and four split loads in flight, summed
// in split order: the order of the fused BN passes that read the same slabs, bit-identical)
template <int P_ = 0>   // template: instantiated in the fwd and dgrad translation units
__global__ __launch_bounds__(256) void splitk_reduce_px_kernel(ConvArgs a, int splits, int phase, FastDiv fdN,
                                                               FastDiv fdT) {
  uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  const uint32_t total = fdT.d;   // M * N
  // merged stride-2 dgrad classes (a.ph_S > 0): slabs [class][split][M][N]
  int cls = 0, y0 = a.ph_y0, x0 = a.ph_x0;
  if (phase && a.ph_S > 0) {
    cls = (int)fdiv(idx, fdT);
    if (cls >= 4) return;
    idx -= (uint32_t)cls * total;
    y0 = a.ph_y0c[cls];
    x0 = a.ph_x0c[cls];
  } else if (idx >= total) {
    return;
  }
  const int m = (int)fdiv(idx, fdN);
  const uint32_t nn = idx - (uint32_t)m * fdN.d;
  const float* p = a.slab + (size_t)cls * splits * total + idx;
  float v = 0.f;
  int s = 0;
  for (; s + 3 < splits; s += 4) {
    const float t0 = p[(size_t)s * total], t1 = p[(size_t)(s + 1) * total];
    const float t2 = p[(size_t)(s + 2) * total], t3 = p[(size_t)(s + 3) * total];
    v += t0;
    v += t1;
    v += t2;
    v += t3;
  }
  for (; s < splits; ++s) v += p[(size_t)s * total];
  int img;
  long pix, plane;
  out_pixel(a, phase != 0, y0, x0, (long)nn, img, pix, plane);
  store_out(a.out, m, img, pix, plane, v);
}

template <int MODE, int BM, int BN, int WM, int WN>
int launch_px_tile(const ConvShape& s, const ConvArgs& a, PxArith arith, bool tap, int bk, dim3 grid,
                   hipStream_t st) {
  const bool v2 = arith == ARITH_PX2, v3 = arith == ARITH_PX3;
#define MD2_PX_CASE(KS, SS, RR)                                                                  \
  if (s.KH == KS && s.stride == SS && s.reflect == RR) {                                         \
    if constexpr (BM >= 32 && BN % 64 == 0 && WM * WN == 4) {                                    \
      if (v3) {                                                                                  \
        conv_arith_ref() = 6;                                                                    \
        conv_note_kernel("px3");                                                                 \
        if (px3_terms() == 6)                                                                    \
          hipLaunchKernelGGL((conv_px3_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 16, 6>), grid, \
                             dim3(256), 0, st, a);                                               \
        else                                                                                     \
          hipLaunchKernelGGL((conv_px3_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 16, 9>), grid, \
                             dim3(256), 0, st, a);                                               \
        MD2_LAUNCH_CHECK();                                                                      \
        return MD2_OK;                                                                           \
      }                                                                                          \
    }                                                                                            \
    if constexpr (BM >= 64 && BN % 64 == 0) {                                                    \
      if (v2) {                                                                                  \
        conv_arith_ref() = 1;                                                                    \
        conv_note_kernel("px2");                                                                 \
        if (bk == 32)                                                                            \
          hipLaunchKernelGGL((conv_px2_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 32>), grid,  \
                             dim3(256), 0, st, a);                                               \
        else                                                                                     \
          hipLaunchKernelGGL((conv_px2_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 16>), grid,  \
                             dim3(256), 0, st, a);                                               \
        MD2_LAUNCH_CHECK();                                                                      \
        return MD2_OK;                                                                           \
      }                                                                                          \
    }                                                                                            \
    if (v2) {                                                                                    \
      set_error("conv: k-contiguous kernel needs a tile with BM >= 64");                         \
      return MD2_EINVAL;                                                                         \
    }                                                                                            \
    conv_arith_ref() = 1;                                                                        \
    conv_note_kernel("px");                                                                      \
    if (tap && bk == 32)                                                                         \
      hipLaunchKernelGGL((conv_px_kernel<MODE, 1, BM, BN, 32, WM, WN, KS, KS, SS, RR>), grid,    \
                         dim3(256), 0, st, a);                                                   \
    else if (tap)                                                                                \
      hipLaunchKernelGGL((conv_px_kernel<MODE, 1, BM, BN, 16, WM, WN, KS, KS, SS, RR>), grid,    \
                         dim3(256), 0, st, a);                                                   \
    else                                                                                         \
      hipLaunchKernelGGL((conv_px_kernel<MODE, 0, BM, BN, 16, WM, WN, KS, KS, SS, RR>), grid,    \
                         dim3(256), 0, st, a);                                                   \
    MD2_LAUNCH_CHECK();                                                                          \
    return MD2_OK;                                                                               \
  }
  MD2_CONV_COMBOS(MD2_PX_CASE)
#undef MD2_PX_CASE
  set_error("conv: unsupported (kernel, stride, padding) combination");
  return MD2_ENOTSUP;
}

// M <= 16 convs on the 16x16x4 MFMA kernel (conv_px16.inc): no split-K, BN 128 (6 blocks per CU
// by LDS; BN 256 ran 20% slower on the full-resolution branch)
template <int MODE>
int launch_px16(const ConvShape& s, ConvArgs& a, hipStream_t st) {
  a.slab = nullptr;
  conv_arith_ref() = 1;
  conv_note_kernel("px16");
  a.g.kper = (int)round_up(a.g.K, 16);
  const dim3 grid(cdiv(a.g.N, 128));
#define MD2_P16_CASE(KS, SS, RR)                                                                 \
  if constexpr (SS == 1) {                                                                       \
    if (s.KH == KS && s.stride == SS && s.reflect == RR) {                                       \
      hipLaunchKernelGGL((conv_px16_kernel<MODE, 128, KS, KS, SS, RR>), grid, dim3(256), 0, st, a); \
      MD2_LAUNCH_CHECK();                                                                        \
      return MD2_OK;                                                                             \
    }                                                                                            \
  }
  MD2_P16_CASE(3, 1, 0) MD2_P16_CASE(3, 1, 1)
#undef MD2_P16_CASE
  set_error("conv: 16-row kernel supports 3x3 stride 1 only");
  return MD2_ENOTSUP;
}

// the kernel the route names: the 16-row kernel, an LDS-halo kernel (r.halo) or the tile `tile`
// (r.tile, or a parity class's own), then the split-K reduction unless the caller takes the slabs
template <int MODE>
int launch_px(const ConvShape& s, ConvArgs& a, const PxRoute& r, const Plan& tile, ConvWorkspace ws,
              hipStream_t st, SplitKDefer* defer = nullptr) {
  double* const stats = defer ? defer->stats : nullptr;
  const bool keep_reduce = defer && defer->keep_reduce;
  if (defer) *defer = SplitKDefer{};
  if (r.kind == PX_PX16) return launch_px16<MODE>(s, a, st);
  const bool halo = r.kind == PX_HALO || r.kind == PX_HALO2D || r.kind == PX_REFLECT_HALO;
  const HaloPlan& hp = r.halo;
  Plan p = tile;
  if (halo) {
    p.splits = hp.splits;
    p.kper = hp.cper * 16;   // only the slab count matters below
  }
  a.g.kper = p.kper;
  a.slab = nullptr;
  if (p.splits > 1) {
    MD2_CHECK_ARG(ws.ptr && ws.bytes >= r.ws_bytes, "conv split-K workspace too small");
    a.slab = (float*)ws.ptr;
  }
  const int ncls = (MODE == 1 && a.ph_S > 0) ? 4 : 1;   // merged stride-2 dgrad classes
  if (ncls > 1) a.ph_S = p.splits;
  dim3 grid(cdiv(a.g.N, p.BN), cdiv(a.g.M, p.BM), p.splits * ncls);
  const bool tap = r.tap;
  int rc;
  if (halo) {
    a.hx_cper = hp.cper;
    // BN statistics in the epilogue: forward, no split-K, a plain contiguous output
    const TensorOut& oo = a.out;
    const bool bnst = MODE == 0 && stats && !hp.d2 && hp.splits == 1 && !s.reflect && !oo.bias && oo.act == ACT_NONE &&
                      !oo.accumulate && oo.c0 >= a.g.M && oo.bs0 == (long)a.g.M * a.fd_pix.d;
    a.bn_part = bnst ? stats : nullptr;
    conv_arith_ref() = 6;
    conv_note_kernel(MODE == 1 && a.hx_ext ? "halo_rfl_dgrad" : hp.d2 ? "halo2d" : "halo");
    rc = hp.d2 ? halo2d_launch(MODE, a, hp.mw, hp.splits, s.reflect, st)
               : halo_launch(MODE, a, hp.items, hp.splits, s.reflect, st);
    a.bn_part = nullptr;
    if (rc == MD2_OK && bnst) {
      defer->stats = stats;
      defer->stats_parts = (int)cdiv(a.g.N, 256);
    }
  } else switch (p.tile) {
#define MD2_PX_TILE_CASE(NAME, BM, BN, WM, WN) \
    case NAME: rc = launch_px_tile<MODE, BM, BN, WM, WN>(s, a, r.arith, tap, p.BK, grid, st); break;
    MD2_PX_TILES(MD2_PX_TILE_CASE)
#undef MD2_PX_TILE_CASE
    default:
      set_error("conv: the plan names a tile that has no launcher");
      return MD2_EINVAL;
  }
  if (rc) return rc;
  const TensorOut& o = a.out;
  if (defer && !keep_reduce && p.splits > 1 && ncls == 1 && (MODE == 0 || s.stride == 1) && !o.bias && o.act == ACT_NONE &&
      !o.accumulate && o.c0 >= a.g.M && o.bs0 == (long)a.g.M * a.fd_pix.d) {
    defer->slab = a.slab;
    defer->splits = p.splits;
    return MD2_OK;
  }
  const int phase = (int)(MODE == 1 && s.stride == 2 && tap);
  const bool aligned4 = a.fd_pix.d % 4 == 0 && o.bs0 % 4 == 0 && (!o.p1 || o.bs1 % 4 == 0) &&
                        ((uintptr_t)o.p0 % 16) == 0 && (!o.p1 || ((uintptr_t)o.p1 % 16) == 0);
  if (p.splits > 1 && ncls == 1 && !phase && aligned4) {
    const long total4 = (long)a.g.M * a.g.N / 4;
    hipLaunchKernelGGL(splitk_reduce_px4_kernel<0>, dim3(cdiv(total4, 256)), dim3(256), 0, st, a,
                       p.splits);
    MD2_LAUNCH_CHECK();
    return MD2_OK;
  }
  if (p.splits > 1) {
    const long total = (long)a.g.M * a.g.N * ncls;
    MD2_CHECK_ARG(total < (1L << 31), "conv: split-K reduction index exceeds 2^31");
    hipLaunchKernelGGL(splitk_reduce_px_kernel<0>, dim3(cdiv(total, 256)), dim3(256), 0, st, a, p.splits,
                       phase, make_fastdiv((uint32_t)a.g.N), make_fastdiv((uint32_t)((long)a.g.M * a.g.N)));
    MD2_LAUNCH_CHECK();
  }
  return MD2_OK;
}

}  // namespace md2
