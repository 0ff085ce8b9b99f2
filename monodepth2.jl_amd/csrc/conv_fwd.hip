// Implicit-GEMM conv: the forward pass (kernels and launchers: conv_px_launch.h).
#include "conv_px_launch.h"

namespace md2 {

// PX_HEAD: the batched kernel where this call's alignment and store mode fit it
static int fwd_head(const ConvShape& s, const PxRoute& r, const TensorIn& x, const float* wpacked,
                    const TensorOut& y, hipStream_t st) {
  MD2_CHECK_ARG(r.layout == 0, "head: packed layout");
  conv_arith_ref() = 0;
  HeadJob j = conv_head_job(s);
  j.x = conv_head_in(x);
  j.wf = conv_head_w(s, 0, wpacked);
  j.bias = y.bias;
  j.y = y.p0;
  j.ybs = y.bs0;
  if (s.reflect && !y.accumulate && !heads_job_unfit(j)) {
    conv_note_kernel("head_batched");
    return heads_fwd(&j, 1, y.act, st);
  }
  conv_note_kernel("head_fallback");
  return head_fwd(j, s.reflect, y.act, y.accumulate, st);
}

int conv_fwd(const ConvShape& s, const TensorIn& x, const float* wpacked, const TensorOut& y,
             ConvWorkspace ws, hipStream_t st, SplitKDefer* defer) {
  if (defer) {
    const SplitKDefer req = *defer;   // kept: launch_px reads the request
    *defer = SplitKDefer{};
    defer->stats = req.stats;
    defer->keep_reduce = req.keep_reduce;
  }
  MD2_TRY(check_shape(s));
  MD2_CHECK_ARG(x.p0 && wpacked && y.p0, "conv_fwd pointers");
  MD2_CHECK_ARG(x.c0 == s.Cin || x.p1 != nullptr, "conv_fwd: second input tensor missing");
  const PxRoute r = conv_fwd_narrow(conv_route(s, 0), s, x, y);
  MD2_CHECK_ARG(x.c0 >= s.Cin || !r.tap || x.c0 % 16 == 0,
                "conv_fwd: concat split must be a multiple of 16 channels");
  if (r.kind == PX_HEAD) return fwd_head(s, r, x, wpacked, y, st);
  ConvArgs a{};
  fill_common(a, s);
  a.g.M = s.Cout;
  a.g.N = (long)s.N * s.Ho * s.Wo;
  a.g.K = s.Cin * s.KH * s.KW;
  a.g.Mpad = r.Mpad;
  a.fd_pix = make_fastdiv((uint32_t)(s.Ho * s.Wo));
  a.fd_row = make_fastdiv((uint32_t)s.Wo);
  a.fd_bdiv = make_fastdiv((uint32_t)std::min(x.bdiv, 1 << 30));
  a.in = x;
  a.A = wpacked;
  a.out = y;
  a.A_bytes = (uint32_t)(r.packed_elems * sizeof(float));
  {
    long ext0 = 0;
    for (int b = 0; b < s.N; ++b)
      ext0 = std::max(ext0, (long)(b % x.bdiv) * x.bs0 + (long)(b / x.bdiv) * x.bhi);
    ext0 += (long)x.c0 * s.H * s.W;
    const long ext1 = x.p1 ? (long)(s.N - 1) * x.bs1 + (long)(s.Cin - x.c0) * s.H * s.W : 0;
    MD2_CHECK_ARG(ext0 * 4 < (long)OOB && ext1 * 4 < (long)OOB, "conv_fwd: tensor exceeds 2 GB");
    a.b0_bytes = (uint32_t)(ext0 * 4);
    a.b1_bytes = (uint32_t)(ext1 * 4);
  }
  switch (r.kind) {
    case PX_STEM_S2D:   // (statistics: the separate pass)
      conv_arith_ref() = 6;
      conv_note_kernel("stem_s2d");
      return stem_s2d_launch(s, a, st);
    case PX_PX16:
    case PX_HALO:
    case PX_HALO2D:
    case PX_TILE:
      return launch_px<0>(s, a, r, r.tile, ws, st, defer);
    default:
      set_error("conv_fwd: not a forward route");
      return MD2_EINVAL;
  }
}

}  // namespace md2
