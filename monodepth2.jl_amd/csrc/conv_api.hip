// C ABI of the conv passes with the executor's operand forms (include/md2.h md2_conv2d_*_ex):
// concat inputs, split / strided / accumulating outputs, padded input channels, frame-major
// images, deferred split-K, epilogue statistics, bias partials; the label of the kernel that ran.
#include "../../include/md2.h"

#include <algorithm>

#include "conv_plan.h"

using namespace md2;

namespace {

size_t align_up(size_t b) { return (b + 255) & ~size_t(255); }

ConvShape ex_shape(const md2_conv_desc* d, const md2_conv_operands* o) {
  ConvShape s{};
  s.N = d->n;
  s.Cin = d->cin;
  s.H = d->h;
  s.W = d->w;
  s.Cout = d->cout;
  s.KH = d->kh;
  s.KW = d->kw;
  s.stride = d->stride;
  s.pad = d->pad;
  s.reflect = d->reflect;
  if (d->stride > 0) {
    s.Ho = (d->h + 2 * d->pad - d->kh) / d->stride + 1;
    s.Wo = (d->w + 2 * d->pad - d->kw) / d->stride + 1;
  }
  s.cin_w = o ? o->cin_w : 0;
  return s;
}

size_t packed_bytes(const ConvShape& s) {
  return align_up(std::max(conv_fwd_packed_elems(s), conv_dgrad_packed_elems(s)) * sizeof(float));
}
size_t slab_bytes(const ConvShape& s) {
  return align_up(std::max(conv_fwd_workspace(s), std::max(conv_dgrad_workspace(s), conv_wgrad_workspace(s))));
}

// the shape and cin_w (no HIP call)
int ex_check_shape(const ConvShape& s) {
  MD2_CHECK_ARG(s.stride == 1 || s.stride == 2, "conv2d_ex: stride 1/2");
  MD2_TRY(check_shape(s));
  MD2_CHECK_ARG(s.cin_w == 0 || s.cin_w == s.Cin || s.Cin % 16 == 0,
                "conv2d_ex: padded input channels (cin_w < cin) need cin % 16 == 0");
  return MD2_OK;
}

int ex_input(const ConvShape& s, const md2_conv_operands* o, const float* x, bool fwd, TensorIn* in) {
  const long HW = (long)s.H * s.W;
  TensorIn t;
  t.p0 = x;
  t.c0 = s.Cin;
  if (o) {
    MD2_CHECK_ARG(o->in_c0 >= 0 && o->in_c0 <= s.Cin, "conv2d_ex: in_c0 must be in 0..cin");
    if (o->in_c0 > 0) t.c0 = o->in_c0;
    MD2_CHECK_ARG(t.c0 == s.Cin || o->in1 != nullptr, "conv2d_ex: in_c0 < cin needs the second input tensor in1");
    MD2_CHECK_ARG(!fwd || t.c0 == s.Cin || s.Cin % 16 != 0 || t.c0 % 16 == 0,
                  "conv2d_ex: the concat split in_c0 must be a multiple of 16 channels when cin % 16 == 0");
    MD2_CHECK_ARG(s.cin_w == 0 || s.cin_w == s.Cin || t.c0 == s.Cin || t.c0 % 16 == 0,
                  "conv2d_ex: cin_w < cin needs a concat split in_c0 that is a multiple of 16");
    MD2_CHECK_ARG(o->in_bs0 >= 0 && o->in_bs1 >= 0 && o->in_bhi >= 0 && o->in_bdiv >= 0,
                  "conv2d_ex: negative input stride or in_bdiv");
    if (t.c0 < s.Cin) {
      t.p1 = o->in1;
      t.bs1 = o->in_bs1 > 0 ? (long)o->in_bs1 : (long)(s.Cin - t.c0) * HW;
    }
    t.bs0 = o->in_bs0 > 0 ? (long)o->in_bs0 : (long)t.c0 * HW;
    if (o->in_bdiv > 0) t.bdiv = o->in_bdiv;
    t.bhi = (long)o->in_bhi;
  } else {
    t.bs0 = (long)s.Cin * HW;
  }
  *in = t;
  return MD2_OK;
}

// rows M = cout (fwd) / cin (dgrad) of `pix` pixels per image
int ex_output(int M, long pix, const md2_conv_operands* o, float* y, TensorOut* out) {
  TensorOut t;
  t.p0 = y;
  t.bs0 = (long)M * pix;
  if (o) {
    MD2_CHECK_ARG(o->out_c0 >= 0 && o->out_c0 <= M, "conv2d_ex: out_c0 must be in 0..rows of the output");
    const int c0 = o->out_c0 > 0 ? o->out_c0 : M;
    MD2_CHECK_ARG(c0 == M || o->out1 != nullptr, "conv2d_ex: out_c0 below the output rows needs the second output tensor out1");
    MD2_CHECK_ARG(o->accumulate == 0 || o->accumulate == 1, "conv2d_ex: accumulate must be 0 or 1");
    MD2_CHECK_ARG(o->out_bs0 == 0 || o->out_bs0 >= (long long)c0 * pix, "conv2d_ex: out_bs0 smaller than the rows it holds");
    MD2_CHECK_ARG(o->out_bs1 == 0 || o->out_bs1 >= (long long)(M - c0) * pix, "conv2d_ex: out_bs1 smaller than the rows it holds");
    t.bs0 = o->out_bs0 > 0 ? (long)o->out_bs0 : (long)c0 * pix;
    if (c0 < M) {
      t.c0 = c0;
      t.p1 = o->out1;
      t.bs1 = o->out_bs1 > 0 ? (long)o->out_bs1 : (long)(M - c0) * pix;
    }
    t.accumulate = o->accumulate;
  }
  *out = t;
  return MD2_OK;
}

int ex_workspace(const ConvShape& s, void* workspace, size_t bytes, ConvWorkspace* ws) {
  const size_t pb = packed_bytes(s);
  MD2_CHECK_ARG(bytes >= pb + slab_bytes(s), "conv2d_ex: workspace smaller than md2_conv2d_ex_workspace_size");
  MD2_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "conv2d_ex: the workspace must be 16-byte aligned");
  *ws = ConvWorkspace{(char*)workspace + pb, bytes - pb};
  return MD2_OK;
}

}  // namespace

extern "C" {

size_t md2_conv2d_ex_workspace_size(const md2_conv_desc* d, const md2_conv_operands* ops) {
  if (!d) return 0;
  const ConvShape s = ex_shape(d, ops);
  if (ex_check_shape(s) != MD2_OK) return 0;
  return packed_bytes(s) + slab_bytes(s);
}

int md2_conv2d_fwd_ex(const md2_conv_desc* d, const md2_conv_operands* ops, const float* x,
                      const float* w, const float* bias, float* y, double* stats,
                      md2_conv_defer* defer, void* workspace, size_t workspace_bytes, void* stream) {
  MD2_CHECK_ARG(d && x && w && y && workspace, "conv2d_fwd_ex: null pointer");
  MD2_CHECK_ARG(!stats || defer, "conv2d_fwd_ex: stats needs defer (stats_parts is returned there)");
  const ConvShape s = ex_shape(d, ops);
  MD2_TRY(ex_check_shape(s));
  TensorIn in;
  TensorOut out;
  ConvWorkspace ws;
  MD2_TRY(ex_input(s, ops, x, true, &in));
  MD2_TRY(ex_output(s.Cout, (long)s.Ho * s.Wo, ops, y, &out));
  MD2_TRY(ex_workspace(s, workspace, workspace_bytes, &ws));
  out.bias = bias;
  out.act = d->act;
  hipStream_t st = (hipStream_t)stream;
  MD2_TRY(conv_pack_fwd(s, w, (float*)workspace, st));
  if (!defer) return conv_fwd(s, in, (const float*)workspace, out, ws, st);
  SplitKDefer df;
  df.stats = stats;
  df.keep_reduce = !defer->defer_reduce;
  defer->slab = nullptr;
  defer->splits = 0;
  defer->stats_parts = 0;
  MD2_TRY(conv_fwd(s, in, (const float*)workspace, out, ws, st, &df));
  defer->slab = df.slab;
  defer->splits = df.splits;
  defer->stats_parts = df.stats_parts;
  return MD2_OK;
}

int md2_conv2d_dgrad_ex(const md2_conv_desc* d, const md2_conv_operands* ops, const float* dy,
                        const float* w, float* dx, md2_conv_defer* defer, void* workspace,
                        size_t workspace_bytes, void* stream) {
  MD2_CHECK_ARG(d && dy && w && dx && workspace, "conv2d_dgrad_ex: null pointer");
  const ConvShape s = ex_shape(d, ops);
  MD2_TRY(ex_check_shape(s));
  TensorOut out;
  ConvWorkspace ws;
  MD2_TRY(ex_output(s.Cin, (long)s.H * s.W, ops, dx, &out));
  MD2_TRY(ex_workspace(s, workspace, workspace_bytes, &ws));
  hipStream_t st = (hipStream_t)stream;
  MD2_TRY(conv_pack_dgrad(s, w, (float*)workspace, st));
  const bool ask = defer && defer->defer_reduce;
  if (defer) {
    defer->slab = nullptr;
    defer->splits = 0;
    defer->stats_parts = 0;
  }
  SplitKDefer df;
  MD2_TRY(conv_dgrad(s, dy, (const float*)workspace, out, ws, st, ask ? &df : nullptr));
  if (ask) {
    defer->slab = df.slab;
    defer->splits = df.splits;
  }
  return MD2_OK;
}

int md2_conv2d_wgrad_ex(const md2_conv_desc* d, const md2_conv_operands* ops, const float* x,
                        const float* dy, float* dw, float* db, const float* db_part, int db_parts,
                        void* workspace, size_t workspace_bytes, void* stream) {
  MD2_CHECK_ARG(d && x && dy && dw && workspace, "conv2d_wgrad_ex: null pointer");
  MD2_CHECK_ARG(!db_part || db, "conv2d_wgrad_ex: db_part without db");
  MD2_CHECK_ARG(!db_part || db_parts >= 1, "conv2d_wgrad_ex: db_parts must be >= 1 with db_part");
  MD2_CHECK_ARG(!ops || ops->accumulate == 0 || ops->accumulate == 1, "conv2d_wgrad_ex: accumulate must be 0 or 1");
  const ConvShape s = ex_shape(d, ops);
  MD2_TRY(ex_check_shape(s));
  TensorIn in;
  ConvWorkspace ws;
  MD2_TRY(ex_input(s, ops, x, false, &in));
  MD2_TRY(ex_workspace(s, workspace, workspace_bytes, &ws));
  return conv_wgrad(s, in, dy, dw, db, ops ? ops->accumulate : 0, ws, (hipStream_t)stream, db_part,
                    db_part ? db_parts : 0);
}

int md2_act_bias_parts(int c, int n, long long hw) {
  if (c < 1 || n < 1 || hw < 1) return 0;
  return act_bias_parts(c, n, (long)hw);
}

int md2_act_backward_bias(const float* out, const float* dout, float* dpre, int n, int c,
                          long long hw, int act, float* part, void* stream) {
  MD2_CHECK_ARG(out && dout && dpre && part, "act_backward_bias: null pointer");
  MD2_CHECK_ARG(n >= 1 && c >= 1 && hw >= 1, "act_backward_bias: n, c, hw must be positive");
  MD2_CHECK_ARG(act >= ACT_NONE && act <= ACT_SIGMOID, "act_backward_bias: act");
  MD2_CHECK_ARG(hw % 4 == 0 && (long long)n * c * hw < (1LL << 31), "act_backward_bias: hw % 4, size");
  MD2_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)dout & 15) == 0 && ((uintptr_t)dpre & 15) == 0,
                "act_backward_bias: 16-byte aligned tensors");
  return act_backward_bias(out, dout, dpre, n, c, (long)hw, act, part, (hipStream_t)stream);
}

const char* md2_conv_last_kernel(void) { return conv_last_kernel(); }

}  // extern "C"
