// Implicit-GEMM conv: the filter-gradient pass -- kernels, launchers, conv_wgrad.
#include <type_traits>
#include "conv_plan.h"

namespace md2 {

#include "conv_wgrad_kernels.inc"
#include "conv_wpx3.inc"

// bias gradient db[c] = sum over images and pixels of dY[img][c][:], two stages:
// grid (C, parts) partial sums over contiguous slices of the N*HW elements, then per channel.
__global__ __launch_bounds__(256) void bias_grad_partial_kernel(const float* __restrict__ dy, int C,
                                                                long HW, long total, int parts,
                                                                float* __restrict__ part) {
  __shared__ float red[4];
  const int c = blockIdx.x, p = blockIdx.y;
  const long beg = total * p / parts, end = total * (p + 1) / parts;
  float s = 0.f;
  for (long e = beg + threadIdx.x; e < end; e += 256) {
    const long img = e / HW, pix = e - img * HW;
    s += dy[(img * C + c) * HW + pix];
  }
  float v[1] = {s};
  block_sum256<1>(v, red);
  if (threadIdx.x == 0) part[(long)c * parts + p] = v[0];
}

// the tap-major wgrad on the bf16 split-product MFMA (conv_wpx3.inc) wherever its pixel pairs fit:
// CW % 32 == 0 and an even pixel count per image (MD2_WPX3=0 with MD2_TUNING=1: the fp32 kernel)
static bool wgrad_px3_on() {
  static const int v = tuning_knob("MD2_WPX3", 1);
  return v != 0;
}

template <int BM, int BN, int WM, int WN, int KS, int SS, int RR, int CW, int PX>
void launch_wpx3(const ConvArgs& a, dim3 grid, hipStream_t st) {
  if (px3_terms() == 6)
    hipLaunchKernelGGL((conv_wgrad_px3_kernel<BM, BN, WM, WN, KS, KS, SS, RR, CW, 6, PX>), grid,
                       dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv_wgrad_px3_kernel<BM, BN, WM, WN, KS, KS, SS, RR, CW, 9, PX>), grid,
                       dim3(256), 0, st, a);
}

template <int BM, int BN, int WM, int WN, int KS, int SS, int RR, int CW>
void launch_w_cw(const ConvArgs& a, dim3 grid, hipStream_t st) {
  // pixel pairs per lane (conv_wpx3.inc; 4 pixels per lane with 16-byte loads measured no faster
  // on the stride-1 layers and 30% slower on the stride-2 ones, profiles/r04_wgrad_px3.txt)
  if constexpr (CW <= BN && CW % 32 == 0 && BM % 32 == 0 && BN % 32 == 0) {
    if (wgrad_px3_on() && a.HoWo % 2 == 0) {
      conv_arith_ref() = 6;
      conv_note_kernel("wgrad_px3", BM, BN, CW);
      launch_wpx3<BM, BN, WM, WN, KS, SS, RR, CW, 2>(a, grid, st);
      return;
    }
  }
  conv_arith_ref() = 1;
  if constexpr (CW <= BN) {
    conv_note_kernel("wgrad_tile", BM, BN, CW);
    hipLaunchKernelGGL((conv_wgrad_tap_kernel<BM, BN, 32, WM, WN, KS, KS, SS, RR, CW>), grid,
                       dim3(256), 0, st, a);
  }
}

template <int BM, int BN, int WM, int WN, int KS, int SS, int RR>
int launch_w(int cw, const ConvArgs& a, dim3 grid, hipStream_t st) {
  if constexpr (BN == 192) {
    // three 64-channel taps per column tile: the 3x3 convs' 64-channel tap blocks only
    if constexpr (KS == 3) {
      if (cw == 64) {
        launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 64>(a, grid, st);
        MD2_LAUNCH_CHECK();
        return MD2_OK;
      }
    }
    return MD2_ENOTSUP;
  } else {
    switch (cw) {
      case 0:
        conv_arith_ref() = 1;
        conv_note_kernel("wgrad_tile", BM, BN, 0);
        hipLaunchKernelGGL((conv_wgrad_kernel<BM, BN, 32, WM, WN, KS, KS, SS, RR>), grid, dim3(256), 0,
                           st, a);
        break;
      case 16: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 16>(a, grid, st); break;
      case 32: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 32>(a, grid, st); break;
      case 64: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 64>(a, grid, st); break;
      case 128: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 128>(a, grid, st); break;
      default: return MD2_ENOTSUP;
    }
    MD2_LAUNCH_CHECK();
    return MD2_OK;
  }
}

// W_HEAD: the batched kernel where this call's alignment and store mode fit it
static int wgrad_head(const ConvShape& s, const TensorIn& x, const float* dy, float* dw, float* db,
                      int accumulate, ConvWorkspace ws, hipStream_t st) {
  conv_arith_ref() = 0;
  HeadJob j = conv_head_job(s);
  j.x = conv_head_in(x);
  j.dy = dy;
  j.dw = dw;
  j.db = db;
  if (s.reflect && !accumulate && !heads_job_unfit(j)) {
    conv_note_kernel("head_batched");
    return heads_bwd(&j, 1, ws.ptr, ws.bytes, st);
  }
  conv_note_kernel("head_fallback");
  return head_wgrad(j, s.reflect, accumulate, ws.ptr, ws.bytes, st);
}

// W_TILE: the generic tiles of the plan (conv_plan.h, MD2_W_TILES: one case per built tile)
static int launch_w_tile(const ConvShape& s, const WPlan& p, const ConvArgs& a, dim3 grid, hipStream_t st) {
#define MD2_W_TILE_CASE(NAME, BM, BN, WM, WN, ID) \
  case NAME: return launch_w<BM, BN, WM, WN, KS, SS, RR>(p.cw, a, grid, st);
#define MD2_W_CASE(KS_, SS_, RR_)                                                                  \
  if (s.KH == KS_ && s.stride == SS_ && s.reflect == RR_) {                                        \
    constexpr int KS = KS_, SS = SS_, RR = RR_;                                                    \
    switch (p.tile) {                                                                              \
      MD2_W_TILES(MD2_W_TILE_CASE)                                                                 \
      default:                                                                                     \
        set_error("conv_wgrad: the plan names a tile that has no launcher");                       \
        return MD2_EINVAL;                                                                         \
    }                                                                                              \
  }
  MD2_CONV_COMBOS(MD2_W_CASE)
#undef MD2_W_CASE
#undef MD2_W_TILE_CASE
  return MD2_ENOTSUP;
}

int conv_wgrad(const ConvShape& s, const TensorIn& x, const float* dy, float* dw, float* db,
               int accumulate, ConvWorkspace ws, hipStream_t st, const float* db_part,
               int db_parts) {
  MD2_TRY(check_shape(s));
  MD2_CHECK_ARG(x.p0 && dy && dw, "conv_wgrad pointers");
  MD2_CHECK_ARG(x.c0 >= s.Cin || x.p1 != nullptr, "conv_wgrad: second input tensor missing");
  const WRoute rt = conv_wgrad_narrow(conv_wgrad_route(s, x.c0), s, x);
  if (rt.kind == W_HEAD) return wgrad_head(s, x, dy, dw, db, accumulate, ws, st);
  const WPlan& p = rt.tile;
  const WHaloPlan& hx = rt.halo;
  const bool tap = p.cw > 0;
  ConvArgs a{};
  fill_common(a, s);
  const long Kpix = (long)s.N * s.Ho * s.Wo;
  a.g.M = s.Cout;
  a.g.N = (long)s.Cin * s.KH * s.KW;
  a.g.K = (int)Kpix;
  a.fd_pix = make_fastdiv((uint32_t)(s.Ho * s.Wo));
  a.fd_row = make_fastdiv((uint32_t)s.Wo);
  a.fd_bdiv = make_fastdiv((uint32_t)std::min(x.bdiv, 1 << 30));
  a.in = x;
  a.dy = dy;
  {
    long ext0 = 0;
    for (int b = 0; b < s.N; ++b)
      ext0 = std::max(ext0, (long)(b % x.bdiv) * x.bs0 + (long)(b / x.bdiv) * x.bhi);
    ext0 += (long)std::min(x.c0, s.Cin) * s.H * s.W;
    const long ext1 = x.p1 ? (long)(s.N - 1) * x.bs1 + (long)(s.Cin - x.c0) * s.H * s.W : 0;
    const long extd = (long)s.N * s.Cout * s.Ho * s.Wo;
    MD2_CHECK_ARG(ext0 * 4 < (long)OOB && ext1 * 4 < (long)OOB && extd * 4 < (long)OOB,
                  "conv_wgrad: tensor exceeds 2 GB");
    a.b0_bytes = (uint32_t)(ext0 * 4);
    a.b1_bytes = (uint32_t)(ext1 * 4);
    a.A_bytes = (uint32_t)(extd * 4);
  }
  a.g.kper = p.kper;
  MD2_CHECK_ARG(ws.ptr && ws.bytes >= rt.ws_bytes, "conv_wgrad workspace too small");
  a.slab = (float*)ws.ptr;
  const long total = (long)a.g.M * a.g.N;
  const int nsplit = rt.nsplit;
  float* bpart = a.slab + (long)nsplit * total;
  dim3 grid((unsigned)p.ntiles_n, cdiv(a.g.M, p.BM), p.splits);
  int rc = MD2_ENOTSUP;
  switch (rt.kind) {
    case W_WHALO:
      a.hx_r = hx.r;
      a.hx_nchunk = hx.nchunk;
      a.hx_cper = hx.cper;
      conv_arith_ref() = 6;
      conv_note_kernel("whalo");
      rc = whalo_launch(a, hx.items, cdiv(hx.r * s.W, 16), hx.splits, st);
      break;
    case W_STEM_S2D:   // the stem on the space-to-depth kernel (conv_stem.inc): one slab per block
      conv_arith_ref() = 6;
      conv_note_kernel("stem_wgrad_s2d");
      rc = stem_wgrad_s2d_launch(s, a, st);
      break;
    case W_STEM: {
      conv_arith_ref() = 1;
      conv_note_kernel("stem_wgrad");
      const dim3 gs((unsigned)p.splits);
      switch (s.Cin) {
        case 1: hipLaunchKernelGGL(conv_wgrad_stem_kernel<1>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
        case 2: hipLaunchKernelGGL(conv_wgrad_stem_kernel<2>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
        case 3: hipLaunchKernelGGL(conv_wgrad_stem_kernel<3>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
        case 4: hipLaunchKernelGGL(conv_wgrad_stem_kernel<4>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
        default: break;
      }
      break;
    }
    case W_WGRAD16:
      conv_arith_ref() = 1;
      conv_note_kernel("wgrad16");
      grid.y = 1;
      if (p.BM == 64) {
        if (s.reflect)
          hipLaunchKernelGGL((conv_wgrad16_kernel<4, 3, 3, 1>), grid, dim3(256), 0, st, a);
        else
          hipLaunchKernelGGL((conv_wgrad16_kernel<4, 3, 3, 0>), grid, dim3(256), 0, st, a);
      } else if (p.BM == 32) {
        if (s.reflect)
          hipLaunchKernelGGL((conv_wgrad16_kernel<2, 3, 3, 1>), grid, dim3(256), 0, st, a);
        else
          hipLaunchKernelGGL((conv_wgrad16_kernel<2, 3, 3, 0>), grid, dim3(256), 0, st, a);
      } else {
        if (s.reflect)
          hipLaunchKernelGGL((conv_wgrad16_kernel<1, 3, 3, 1>), grid, dim3(256), 0, st, a);
        else
          hipLaunchKernelGGL((conv_wgrad16_kernel<1, 3, 3, 0>), grid, dim3(256), 0, st, a);
      }
      rc = MD2_OK;
      break;
    default: rc = launch_w_tile(s, p, a, grid, st); break;
  }
  if (rc == MD2_ENOTSUP) set_error("conv_wgrad: unsupported (kernel, stride, padding) combination");
  if (rc) return rc;
  MD2_LAUNCH_CHECK();
  WRed r{};
  r.slab = a.slab;
  r.splits = nsplit;
  r.total = total;
  r.dw = dw;
  r.acc = accumulate;
  r.ncols = (int)a.g.N;
  r.tapc = (tap || rt.kind == W_WHALO) ? s.Cin : 0;
  r.KK = s.KH * s.KW;
  r.cinw = weight_cin(s);
  r.out_total = (long)s.Cout * r.cinw * r.KK;
  MD2_CHECK_ARG(r.cinw == s.Cin || tap, "conv_wgrad: padded input channels need the tap-major kernels");
  int nbias = 0;
  if (db) {
    int parts = db_parts;
    if (db_part) {
      r.bpart = db_part;
    } else {
      parts = bias_parts(s.Cout, Kpix);
      hipLaunchKernelGGL(bias_grad_partial_kernel, dim3(s.Cout, parts), dim3(256), 0, st, dy, s.Cout,
                         (long)s.Ho * s.Wo, Kpix, parts, bpart);
      MD2_LAUNCH_CHECK();
      r.bpart = bpart;
    }
    r.bparts = parts;
    r.Cout = s.Cout;
    r.db = db;
    nbias = cdiv(s.Cout, 256);
  }
  // 4 lanes per output once there are enough splits to share (more loads in flight per output)
  if (nsplit >= 8) {
    r.nmain = (int)cdiv(total, 64);
    hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3(r.nmain + nbias), dim3(256), 0, st, r);
  } else {
    r.nmain = (int)cdiv(r.out_total, 256);
    hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3(r.nmain + nbias), dim3(256), 0, st, r);
  }
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
