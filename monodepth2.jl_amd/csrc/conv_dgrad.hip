// Implicit-GEMM conv: the data-gradient pass (kernels, launchers: conv_px_launch.h), the reflect fold.
#include "conv_px_launch.h"

namespace md2 {

// pad_reflect(x, 1)'s adjoint (src/depth_decoder.jl:5, NNlib pad_reflect), second half of the
// reflect-padded dgrad: the full adjoint on the padded grid -- `splits` split-K slabs summed here
// (element (n, c, r, q) of slab k at src + k * ss + n * sn + c * sc + r * (W + 2) + q) -- folded
// onto dX [N][C][H][W]: padded row 0 is input row 1, padded row H+1 input row H-2 (likewise
// columns), stored / accumulated through the conv's TensorOut (concat split, image strides).
// Flat grid over the N * C * H * W outputs, one per thread (a planes-by-blocks grid of small maps
// was workgroup-dispatch bound; 4 outputs x 9 candidate loads per thread latency bound: 10-20 us
// for 1-5 MB); 32-bit index math.  Candidates per split: rows {i+1, reflected}, columns likewise
// -- 4 loads issued back to back (absent ones read the centre and are dropped); SMALL (H or W ==
// 3: a row / column reflected twice) takes the 3 x 3 set.
template <bool SMALL>
__global__ __launch_bounds__(256) void fold_reflect_kernel(const float* __restrict__ src, int splits, long ss,
                                                           long sn, long sc, TensorOut o, FastDiv fd_hw,
                                                           FastDiv fd_w, FastDiv fd_c, uint32_t total) {
  constexpr int NR = SMALL ? 3 : 2;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= total) return;
  const int H = (int)fd_hw.d / (int)fd_w.d, W = (int)fd_w.d, P = W + 2;
  const uint32_t nc = fdiv(idx, fd_hw);
  const int pix = (int)(idx - nc * fd_hw.d);
  const int n = (int)fdiv(nc, fd_c), c = (int)(nc - n * fd_c.d);
  const int i = (int)fdiv((uint32_t)pix, fd_w), j = pix - i * W;
  const float* p = src + n * sn + c * sc;
  // rows mapping to i: {i+1} + the reflected ones; columns likewise (fixed summation order)
  const int rows[3] = {i + 1, i == 1 ? 0 : (i == H - 2 ? H + 1 : -1), (i == H - 2 && i == 1) ? H + 1 : -1};
  const int cols[3] = {j + 1, j == 1 ? 0 : (j == W - 2 ? W + 1 : -1), (j == W - 2 && j == 1) ? W + 1 : -1};
  int off[NR * NR];
  bool use[NR * NR];
#pragma unroll
  for (int a_ = 0; a_ < NR; ++a_)
#pragma unroll
    for (int b_ = 0; b_ < NR; ++b_) {
      use[NR * a_ + b_] = rows[a_] >= 0 && cols[b_] >= 0;
      off[NR * a_ + b_] = use[NR * a_ + b_] ? rows[a_] * P + cols[b_] : (i + 1) * P + j + 1;
    }
  float v = 0.f;
#pragma unroll 2
  for (int k = 0; k < splits; ++k, p += ss) {
    float t[NR * NR];
#pragma unroll
    for (int u = 0; u < NR * NR; ++u) t[u] = p[off[u]];
#pragma unroll
    for (int u = 0; u < NR * NR; ++u) v += use[u] ? t[u] : 0.f;
  }
  float* dst = (c < o.c0) ? o.p0 + (long)n * o.bs0 + (long)c * fd_hw.d + pix
                          : o.p1 + (long)n * o.bs1 + (long)(c - o.c0) * fd_hw.d + pix;
  if (o.accumulate)
    *dst += v;
  else
    *dst = v;
}

// Four consecutive pixels of one row per thread (W % 4 == 0): where all four are interior (the
// row is not 1 / H-2, the columns 2 .. W-3) each split is ONE 4-float load of the padded image
// (dword-aligned) instead of four 2x2 candidate gathers per pixel; border quads take the generic
// per-pixel path.  The same fp sums in the same order as fold_reflect_kernel (bit-identical).
template <int P_ = 0>
__global__ __launch_bounds__(256) void fold_reflect4_kernel(const float* __restrict__ src, int splits, long ss,
                                                            long sn, long sc, TensorOut o, FastDiv fd_hw,
                                                            FastDiv fd_w4, FastDiv fd_c, int H, uint32_t total4) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= total4) return;
  const int W4 = (int)fd_w4.d, W = 4 * W4, P = W + 2;
  const uint32_t HW4 = (uint32_t)(H * W4);
  const uint32_t nc = idx / HW4;
  const int q = (int)(idx - nc * HW4);
  const int n = (int)fdiv(nc, fd_c), c = (int)(nc - n * fd_c.d);
  const int i = (int)fdiv((uint32_t)q, fd_w4), j0 = 4 * (q - i * W4);
  const float* p = src + n * sn + c * sc;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (i != 1 && i != H - 2 && j0 >= 2 && j0 + 3 <= W - 3) {
    const float* r = p + (i + 1) * P + j0 + 1;
#pragma unroll 2
    for (int k = 0; k < splits; ++k, r += ss) {
      float t[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = r[e];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += t[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      const int rows[2] = {i + 1, i == 1 ? 0 : (i == H - 2 ? H + 1 : -1)};
      const int cols[2] = {j + 1, j == 1 ? 0 : (j == W - 2 ? W + 1 : -1)};
      const float* pp = p;
      for (int k = 0; k < splits; ++k, pp += ss) {
#pragma unroll
        for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
          for (int b_ = 0; b_ < 2; ++b_)
            if (rows[a_] >= 0 && cols[b_] >= 0) v[e] += pp[rows[a_] * P + cols[b_]];
      }
    }
  }
  const int pix = i * W + j0;
  float* dst = (c < o.c0) ? o.p0 + (long)n * o.bs0 + (long)c * fd_hw.d + pix
                          : o.p1 + (long)n * o.bs1 + (long)(c - o.c0) * fd_hw.d + pix;
  float4 r4 = make_float4(v[0], v[1], v[2], v[3]);
  if (o.accumulate) {
    const float4 d = *reinterpret_cast<const float4*>(dst);
    r4 = make_float4(d.x + r4.x, d.y + r4.y, d.z + r4.z, d.w + r4.w);
  }
  *reinterpret_cast<float4*>(dst) = r4;
}

// PX_HEAD: the batched kernel where this call's alignment and store mode fit it
static int dgrad_head(const ConvShape& s, const PxRoute& r, const float* dy, const float* wpacked_d,
                      const TensorOut& dx, hipStream_t st) {
  MD2_CHECK_ARG(r.layout == 0 && !r.tap, "head: packed layout");
  conv_arith_ref() = 0;
  HeadJob j = conv_head_job(s);
  j.wd = conv_head_w(s, 1, wpacked_d);
  j.dy = dy;
  j.dx = dx.p0;
  j.dxbs = dx.bs0;
  if (s.reflect && !dx.accumulate && !heads_job_unfit(j)) {
    conv_note_kernel("head_batched");
    return heads_bwd(&j, 1, nullptr, 0, st);
  }
  conv_note_kernel("head_fallback");
  return head_dgrad(j, s.reflect, dx.accumulate, st);
}

// PX_REFLECT_HALO: the full adjoint on the padded grid (split-K slabs first in the workspace, the
// padded image after them), then pad_reflect's adjoint into dX
static int dgrad_reflect_halo(const ConvShape& s, const PxRoute& r, const ConvArgs& a, const TensorOut& dx,
                              ConvWorkspace ws, hipStream_t st) {
  const ConvShape& e = r.ext;
  const HaloPlan& h = r.halo;
  const long Ne = (long)s.N * e.H * e.W;
  const size_t slab_b = (size_t)(h.splits > 1 ? h.splits : 0) * s.Cin * Ne * sizeof(float);
  MD2_CHECK_ARG(ws.ptr && ws.bytes >= r.ws_bytes, "conv_dgrad: reflect workspace too small");
  float* dxp = (float*)((char*)ws.ptr + slab_b);
  ConvArgs ae = a;
  fill_common(ae, e);
  ae.Ho = s.Ho;
  ae.Wo = s.Wo;
  ae.HoWo = (long)s.Ho * s.Wo;
  ae.HoWo4 = (uint32_t)(ae.HoWo * 4);
  ae.g.N = Ne;
  ae.fd_pix = make_fastdiv((uint32_t)(e.H * e.W));
  ae.fd_row = make_fastdiv((uint32_t)e.W);
  ae.hx_ext = 1;
  TensorOut po{};
  po.p0 = dxp;
  po.c0 = s.Cin;
  po.bs0 = (long)s.Cin * e.H * e.W;
  ae.out = po;
  MD2_CHECK_ARG((long)s.N * s.Cin * (s.H + 2) * (s.W + 2) < (1L << 31), "conv_dgrad: reflect fold index");
  // split-K: the slabs [split][Cin][N][H+2][W+2] go straight to the fold (no reduce pass)
  SplitKDefer df;
  MD2_TRY(launch_px<1>(e, ae, r, r.tile, ws, st, &df));
  const long HWp = (long)e.H * e.W;
  const bool sl = df.slab != nullptr;
  const long total = (long)s.N * s.Cin * s.H * s.W;
  const bool small = s.H == 3 || s.W == 3;
  // (four pixels per thread: W % 4 == 0, 16-byte aligned destination planes)
  static const int f4on = tuning_knob("MD2_FOLD4", 1);
  const bool f4 = f4on && !small && s.W % 4 == 0 && s.H >= 4 && s.W >= 8 && ((long)s.H * s.W) % 4 == 0 &&
                  ((uintptr_t)dx.p0 % 16) == 0 && dx.bs0 % 4 == 0 &&
                  (!dx.p1 || (((uintptr_t)dx.p1 % 16) == 0 && dx.bs1 % 4 == 0));
  if (f4)
    hipLaunchKernelGGL(fold_reflect4_kernel<0>, dim3(cdiv(total / 4, 256)), dim3(256), 0, st,
                       sl ? df.slab : dxp, sl ? df.splits : 1, (long)s.Cin * Ne, sl ? HWp : s.Cin * HWp,
                       sl ? Ne : HWp, dx, make_fastdiv((uint32_t)(s.H * s.W)),
                       make_fastdiv((uint32_t)(s.W / 4)), make_fastdiv((uint32_t)s.Cin), s.H,
                       (uint32_t)(total / 4));
  else
    hipLaunchKernelGGL(small ? fold_reflect_kernel<true> : fold_reflect_kernel<false>, dim3(cdiv(total, 256)),
                       dim3(256), 0, st, sl ? df.slab : dxp, sl ? df.splits : 1, (long)s.Cin * Ne,
                       sl ? HWp : s.Cin * HWp, sl ? Ne : HWp, dx, make_fastdiv((uint32_t)(s.H * s.W)),
                       make_fastdiv((uint32_t)s.W), make_fastdiv((uint32_t)s.Cin), (uint32_t)total);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// PX_HALO_S2: the four output-parity classes from one staged dY image (conv_halo3s2_kernel): the
// kernel iterates the dY grid; its split-K slabs [split][Cin][N H W] reduce as any dgrad's
static int dgrad_halo_s2(const ConvShape& s, const PxRoute& r, const ConvArgs& a, ConvWorkspace ws,
                         hipStream_t st) {
  const HaloS2Plan& h2 = r.s2;
  ConvArgs ak = a;
  ak.g.N = (long)s.N * s.Ho * s.Wo;
  ak.fd_pix = make_fastdiv((uint32_t)(s.Ho * s.Wo));
  ak.fd_row = make_fastdiv((uint32_t)s.Wo);
  ak.hx_cper = h2.cper;
  ak.slab = nullptr;
  if (h2.splits > 1) {
    MD2_CHECK_ARG(ws.ptr && ws.bytes >= r.ws_bytes, "conv_dgrad: stride-2 halo workspace too small");
    ak.slab = (float*)ws.ptr;
  }
  conv_arith_ref() = 6;
  conv_note_kernel("halo_s2");
  MD2_TRY(halo_s2_launch(ak, h2.items, h2.splits, st));
  if (h2.splits > 1) {
    ConvArgs ar = a;
    ar.slab = ak.slab;
    const TensorOut& o = a.out;
    const bool aligned4 = a.fd_pix.d % 4 == 0 && o.bs0 % 4 == 0 && (!o.p1 || o.bs1 % 4 == 0) &&
                          ((uintptr_t)o.p0 % 16) == 0 && (!o.p1 || ((uintptr_t)o.p1 % 16) == 0);
    const long total = (long)a.g.M * a.g.N;
    MD2_CHECK_ARG(total < (1L << 31), "conv_dgrad: split-K reduction index exceeds 2^31");
    if (aligned4)
      hipLaunchKernelGGL(splitk_reduce_px4_kernel<0>, dim3(cdiv(total / 4, 256)), dim3(256), 0, st, ar,
                         h2.splits);
    else
      hipLaunchKernelGGL(splitk_reduce_px_kernel<0>, dim3(cdiv(total, 256)), dim3(256), 0, st, ar,
                         h2.splits, 0, make_fastdiv((uint32_t)a.g.N), make_fastdiv((uint32_t)total));
    MD2_LAUNCH_CHECK();
  }
  return MD2_OK;
}

// one output-parity class of the stride-2 dgrad as the GEMM extents of `ac`
static void class_extents(ConvArgs& ac, const ConvShape& s, const PhaseClass& c) {
  ac.g.N = (long)s.N * c.Hc * c.Wc;
  ac.fd_pix = make_fastdiv((uint32_t)(c.Hc * c.Wc));
  ac.fd_row = make_fastdiv((uint32_t)c.Wc);
}

int conv_dgrad(const ConvShape& s, const float* dy, const float* wpacked_d, const TensorOut& dx,
               ConvWorkspace ws, hipStream_t st, SplitKDefer* defer) {
  if (defer) *defer = SplitKDefer{};
  MD2_TRY(check_shape(s));
  MD2_CHECK_ARG(dy && wpacked_d && dx.p0, "conv_dgrad pointers");
  MD2_CHECK_ARG(!dx.bias && dx.act == ACT_NONE, "conv_dgrad: no bias/activation on dX");
  const PxRoute r = conv_dgrad_narrow(conv_route(s, 1), s, dx);
  if (r.kind == PX_HEAD) return dgrad_head(s, r, dy, wpacked_d, dx, st);
  ConvArgs a{};
  fill_common(a, s);
  a.g.M = s.Cin;
  a.g.N = (long)s.N * s.H * s.W;
  a.g.K = s.Cout * s.KH * s.KW;
  a.g.Mpad = r.Mpad;
  a.fd_pix = make_fastdiv((uint32_t)(s.H * s.W));
  a.fd_row = make_fastdiv((uint32_t)s.W);
  a.fd_bdiv = make_fastdiv(1u << 30);
  a.dy = dy;
  a.A = wpacked_d;
  a.out = dx;
  a.A_bytes = (uint32_t)(r.packed_elems * sizeof(float));
  MD2_CHECK_ARG((long)s.N * s.Cout * s.Ho * s.Wo * 4 < (long)OOB, "conv_dgrad: tensor exceeds 2 GB");
  a.b0_bytes = (uint32_t)((long)s.N * s.Cout * s.Ho * s.Wo * 4);
  a.b1_bytes = 0;
  switch (r.kind) {
    case PX_REFLECT_HALO: return dgrad_reflect_halo(s, r, a, dx, ws, st);
    case PX_HALO_S2: return dgrad_halo_s2(s, r, a, ws, st);
    case PX_CLASSES_MERGED: {
      // ONE launch: equal extents, K of the largest class; smaller classes' surplus splits write
      // zero slabs
      ConvArgs ac = a;
      int kmax = 0;
      for (int cls = 0; cls < 4; ++cls) {
        const PhaseClass& c = r.cls[cls];
        ac.ph_y0c[cls] = c.y0;
        ac.ph_x0c[cls] = c.x0;
        ac.ph_ntc[cls] = c.ntaps;
        for (int t = 0; t < 4; ++t) ac.ph_taps[4 * cls + t] = t < c.ntaps ? c.taps[t] : 0;
        kmax = std::max(kmax, c.ntaps);
      }
      class_extents(ac, s, r.cls[0]);
      ac.g.K = kmax * s.Cout;
      ac.ph_S = 1;
      return launch_px<1>(s, ac, r, r.cls_plan[0], ws, st);
    }
    case PX_CLASSES4:
      for (int cls = 0; cls < 4; ++cls) {
        const PhaseClass& c = r.cls[cls];
        if (c.Hc <= 0 || c.Wc <= 0 || (c.ntaps == 0 && dx.accumulate)) continue;
        ConvArgs ac = a;
        ac.ph_y0 = c.y0;
        ac.ph_x0 = c.x0;
        for (int t = 0; t < 16; ++t) ac.ph_taps[t] = t < c.ntaps ? c.taps[t] : 0;
        class_extents(ac, s, c);
        ac.g.K = c.ntaps * s.Cout;
        MD2_TRY(launch_px<1>(s, ac, r, r.cls_plan[cls], ws, st));
      }
      return MD2_OK;
    case PX_PX16:
    case PX_HALO:
    case PX_HALO2D:
    case PX_TILE:
      return launch_px<1>(s, a, r, r.tile, ws, st, defer);
    default:
      set_error("conv_dgrad: not a data-gradient route");
      return MD2_EINVAL;
  }
}

}  // namespace md2
