// C ABI of the BatchNorm passes with the executor's operand forms (include/md2.h md2_bn_*_ex,
// md2_maxpool3s2_bwd_ex): split-K slab inputs, caller statistics partials (optionally collapsed),
// the downsample branch, residual, ReLU from a mask tensor or re-derived from y, dres stored or
// accumulated, the skip addend, the stem tail with its max pool.  Thin wrappers over nn.h: the
// route the executor takes from its switches is an argument here, and the call reports what ran.
#include "../../include/md2.h"

#include "bn_device.h"

using namespace md2;

namespace {

size_t align_up(size_t b) { return (b + 255) & ~size_t(255); }

// workspace: [own / backward partials][second branch's partials][collapsed caller partials]
struct BnWs {
  size_t part_bytes, col_bytes;
  size_t total() const { return 2 * part_bytes + col_bytes; }
};

int bn_check_desc(const md2_bn_desc* d, const char* what) {
  MD2_CHECK_ARG(d != nullptr, std::string(what) + ": null pointer");
  MD2_CHECK_ARG(d->n >= 1 && d->c >= 1 && d->h >= 1 && d->w >= 1, std::string(what) + ": n, c, h, w must be positive");
  MD2_CHECK_ARG((long long)d->n * d->c * d->h * d->w < (1LL << 31), std::string(what) + ": tensor larger than 2^31 elements");
  MD2_CHECK_ARG(d->route >= 0 && d->route <= 2, std::string(what) + ": route must be 0, 1 or 2");
  MD2_CHECK_ARG(d->collapse == 0 || d->collapse == 1, std::string(what) + ": collapse must be 0 or 1");
  MD2_CHECK_ARG(d->route != 2 || bn_channel_fits(d->n, (long)d->h * d->w),
                std::string(what) + ": route 2 needs a channel that fits in a block");
  return MD2_OK;
}

BnWs bn_ws_layout(const md2_bn_desc* d) {
  const long HW = (long)d->h * d->w;
  BnWs w;
  w.part_bytes = align_up(sizeof(double) * 2 * (size_t)d->c * bn_parts(d->c, d->n, HW));
  w.col_bytes = align_up(sizeof(double) * 2 * (size_t)d->c);
  return w;
}

int bn_check_ws(const BnWs& w, const void* workspace, size_t bytes, const char* what) {
  MD2_CHECK_ARG(workspace != nullptr, std::string(what) + ": null pointer");
  MD2_CHECK_ARG(bytes >= w.total(), std::string(what) + ": workspace smaller than md2_bn_ex_workspace_size");
  MD2_CHECK_ARG(((uintptr_t)workspace & 15) == 0, std::string(what) + ": the workspace must be 16-byte aligned");
  return MD2_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t md2_bn_ex_workspace_size(const md2_bn_desc* d) {
  if (bn_check_desc(d, "bn_ex_workspace_size") != MD2_OK) return 0;
  return bn_ws_layout(d).total();
}

int md2_bn_channel_fits(int n, long long hw) {
  if (n < 1 || hw < 1) return 0;
  return bn_channel_fits(n, (long)hw) ? 1 : 0;
}

int md2_bn_forward_ex(const md2_bn_desc* d, const md2_bn_fwd_operands* o, md2_bn_info* info,
                      void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "bn_forward_ex";
  MD2_TRY(bn_check_desc(d, what));
  MD2_CHECK_ARG(o && o->gamma && o->beta && o->mean && o->invstd && o->out, "bn_forward_ex: null pointer");
  MD2_CHECK_ARG((o->y != nullptr) != (o->slab != nullptr), "bn_forward_ex: exactly one of y and slab");
  MD2_CHECK_ARG(!o->slab || (o->splits >= 1 && o->y_out), "bn_forward_ex: slab needs splits >= 1 and y_out");
  MD2_CHECK_ARG(!o->slab || !o->part, "bn_forward_ex: slab with caller partials");
  MD2_CHECK_ARG(!o->part || o->parts >= 1, "bn_forward_ex: parts must be >= 1 with part");
  MD2_CHECK_ARG(!d->collapse || o->part, "bn_forward_ex: collapse without caller partials");
  MD2_CHECK_ARG(d->route != 2 || !o->part, "bn_forward_ex: route 2 with caller partials");
  MD2_CHECK_ARG(!o->y2 || (o->gamma2 && o->beta2 && o->mean2 && o->invstd2),
                "bn_forward_ex: y2 needs gamma2, beta2, mean2 and invstd2");
  MD2_CHECK_ARG((o->run_mean != nullptr) == (o->run_var != nullptr), "bn_forward_ex: run_mean and run_var go together");
  MD2_CHECK_ARG(o->relu == 0 || o->relu == 1, "bn_forward_ex: relu must be 0 or 1");
  const bool pool = o->pool_y || o->pool_arg;
  if (pool) {
    MD2_CHECK_ARG(o->pool_y && o->pool_arg, "bn_forward_ex: pool_y and pool_arg go together");
    MD2_CHECK_ARG(d->h % 2 == 0 && d->w % 2 == 0, "bn_forward_ex: pool outputs need even h and w");
    MD2_CHECK_ARG(!o->y2 && !o->res && o->relu == 1, "bn_forward_ex: pool outputs need relu without y2 / res");
    MD2_CHECK_ARG(d->route != 2, "bn_forward_ex: route 2 with pool outputs");
  }
  const int N = d->n, C = d->c;
  const long HW = (long)d->h * d->w;
  const bool vec = HW % 4 == 0;
  MD2_CHECK_ARG(!vec || (aligned16(o->y) && aligned16(o->slab) && aligned16(o->y_out) && aligned16(o->y2) &&
                         aligned16(o->res) && aligned16(o->out)),
                "bn_forward_ex: 16-byte aligned tensors");
  const BnWs wl = bn_ws_layout(d);
  MD2_TRY(bn_check_ws(wl, workspace, workspace_bytes, what));

  hipStream_t st = (hipStream_t)stream;
  double* ws1 = (double*)workspace;
  double* ws2 = (double*)((char*)workspace + wl.part_bytes);
  double* wcol = (double*)((char*)workspace + 2 * wl.part_bytes);
  const int own_parts = bn_parts(C, N, HW);

  BNApplyFused p{};
  p.y = o->slab ? o->y_out : o->y;
  p.s1.eps = d->eps;
  p.s1.momentum = d->momentum;
  p.s1.gamma = o->gamma;
  p.s1.beta = o->beta;
  p.s1.mean = o->mean;
  p.s1.invstd = o->invstd;
  p.s1.run_mean = o->run_mean;
  p.s1.run_var = o->run_var;
  p.res = o->res;
  p.relu = o->relu;
  if (o->y2) {   // the downsample branch: its own statistics pass, as in the model
    p.y2 = o->y2;
    p.s2.eps = d->eps;
    p.s2.momentum = d->momentum;
    p.s2.gamma = o->gamma2;
    p.s2.beta = o->beta2;
    p.s2.mean = o->mean2;
    p.s2.invstd = o->invstd2;
    p.s2.part = ws2;
    p.s2.parts = own_parts;
    MD2_TRY(bn_stats_partial(o->y2, N, C, HW, BNStatsWs{ws2, own_parts}, st));
  }
  const SlabIn sl = o->slab ? SlabIn{o->slab, o->splits} : SlabIn{};
  md2_bn_info inf{};
  inf.vec = vec ? 1 : 0;
  const bool one = !pool && (d->route == 2 || (d->route == 0 && !o->part && bn_channel_fits(N, HW)));
  if (one) {
    inf.family = 2;
    MD2_TRY(bn_fwd_channel(sl, o->y_out, p, o->out, N, C, HW, st));
  } else {
    if (o->part) {
      inf.parts = o->parts;
      if (d->collapse) {
        MD2_TRY(bn_partials_collapse(o->part, C, o->parts, wcol, st));
        p.s1.part = wcol;
        p.s1.parts = 1;
      } else {
        p.s1.part = o->part;
        p.s1.parts = o->parts;
      }
    } else {
      inf.parts = own_parts;
      p.s1.part = ws1;
      p.s1.parts = own_parts;
      if (o->slab)
        MD2_TRY(bn_stats_partial_slabs(sl, o->y_out, N, C, HW, BNStatsWs{ws1, own_parts}, st));
      else
        MD2_TRY(bn_stats_partial(o->y, N, C, HW, BNStatsWs{ws1, own_parts}, st));
    }
    inf.fin_parts = p.s1.parts;
    if (pool) {
      inf.family = 3;
      inf.upt = 1;
      MD2_TRY(bn_relu_maxpool(p, o->out, N, C, d->h, d->w, o->pool_y, o->pool_arg, d->h / 2, d->w / 2, st));
    } else {
      inf.family = 1;
      inf.upt = vec ? bn_upt((long)N * C * HW / 4, HW / 4) : 1;
      MD2_TRY(bn_apply_fused(p, o->out, N, C, HW, st));
    }
  }
  if (info) *info = inf;
  return MD2_OK;
}

int md2_bn_backward_ex(const md2_bn_desc* d, const md2_bn_bwd_operands* o, md2_bn_info* info,
                       void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "bn_backward_ex";
  MD2_TRY(bn_check_desc(d, what));
  MD2_CHECK_ARG(o && o->y && o->mean && o->invstd && o->gamma && o->dgamma && o->dbeta && o->dy,
                "bn_backward_ex: null pointer");
  MD2_CHECK_ARG((o->dout != nullptr) != (o->slab != nullptr), "bn_backward_ex: exactly one of dout and slab");
  MD2_CHECK_ARG(!o->slab || o->splits >= 1, "bn_backward_ex: slab needs splits >= 1");
  MD2_CHECK_ARG(!o->slab || (!o->mask && !o->skip), "bn_backward_ex: slab with a mask or a skip");
  MD2_CHECK_ARG(!o->mask || !o->mbeta, "bn_backward_ex: mask together with mbeta");
  MD2_CHECK_ARG(o->dres_accumulate == 0 || o->dres_accumulate == 1, "bn_backward_ex: dres_accumulate must be 0 or 1");
  const int N = d->n, C = d->c;
  const long HW = (long)d->h * d->w;
  const long n = (long)N * C * HW;
  const bool vec = HW % 4 == 0;
  if (o->skip) {
    MD2_CHECK_ARG(vec, "bn_backward_ex: a skip needs h*w % 4 == 0");
    MD2_CHECK_ARG(o->skip_lo >= 0 && o->skip_lo <= o->skip_hi && o->skip_hi <= (long long)n,
                  "bn_backward_ex: skip range outside the tensor");
    MD2_CHECK_ARG(o->skip_lo % 4 == 0 && o->skip_hi % 4 == 0,
                  "bn_backward_ex: skip_lo and skip_hi must be multiples of 4");
  }
  const bool one = d->route == 2 || (d->route == 0 && bn_channel_fits(N, HW));
  MD2_CHECK_ARG(!o->slab || one || o->dout_w, "bn_backward_ex: slab on two passes needs dout_w");
  MD2_CHECK_ARG(!vec || (aligned16(o->dout) && aligned16(o->slab) && aligned16(o->dout_w) && aligned16(o->mask) &&
                         aligned16(o->y) && aligned16(o->dy) && aligned16(o->dres) && aligned16(o->skip)),
                "bn_backward_ex: 16-byte aligned tensors");
  const BnWs wl = bn_ws_layout(d);
  MD2_TRY(bn_check_ws(wl, workspace, workspace_bytes, what));

  hipStream_t st = (hipStream_t)stream;
  BNBwd b;
  b.dout = o->dout;
  if (o->slab) b.slabs = SlabIn{o->slab, o->splits};
  b.mask = o->mask;
  b.y = o->y;
  b.mean = o->mean;
  b.invstd = o->invstd;
  b.gamma = o->gamma;
  b.mbeta = o->mbeta;
  b.dgamma = o->dgamma;
  b.dbeta = o->dbeta;
  b.dy = o->dy;
  b.dres = o->dres;
  b.dres_accumulate = o->dres_accumulate;
  if (o->skip) {
    b.skip.skip = o->skip;
    b.skip.lo = (long)o->skip_lo;
    b.skip.hi = (long)o->skip_hi;
  }
  md2_bn_info inf{};
  inf.vec = vec ? 1 : 0;
  if (one) {
    inf.family = 2;
    MD2_TRY(bn_bwd_channel(b, N, C, HW, st));
  } else {
    BNStatsWs w{(double*)workspace, bn_parts(C, N, HW)};
    inf.family = 1;
    inf.parts = inf.fin_parts = w.parts;
    inf.upt = vec ? bn_upt(n / 4, HW / 4) : 1;
    if (o->slab) {   // conv_d_bn's form: the partial pass writes the sum, the apply reads it
      MD2_TRY(bn_bwd_partial_slabs(b, o->dout_w, N, C, HW, w, st));
      b.slabs = SlabIn{};
      b.dout = o->dout_w;
    } else {
      MD2_TRY(bn_bwd_partial(b, N, C, HW, w, st));
    }
    MD2_TRY(bn_bwd_apply_fused(b, N, C, HW, w, st));
  }
  if (info) *info = inf;
  return MD2_OK;
}

int md2_maxpool3s2_bwd_ex(const float* dy, const unsigned char* arg, int n, int c, int h, int w,
                          float* dx, const float* skip, long long skip_lo, long long skip_hi,
                          void* stream) {
  MD2_CHECK_ARG(dy && arg && dx, "maxpool3s2_bwd_ex: null pointer");
  MD2_CHECK_ARG(n > 0 && c > 0 && h > 0 && w > 0, "maxpool3s2_bwd_ex: n, c, h, w must be positive");
  const long long total = (long long)n * c * h * w, hw = (long long)h * w;
  MD2_CHECK_ARG(total < (1LL << 31), "maxpool3s2_bwd_ex: tensor larger than 2^31 elements");
  SkipAdd sk;
  if (skip) {
    MD2_CHECK_ARG(w % 2 == 0, "maxpool3s2_bwd_ex: a skip needs an even w");
    MD2_CHECK_ARG(skip_lo >= 0 && skip_lo <= skip_hi && skip_hi <= total && skip_lo % hw == 0 && skip_hi % hw == 0,
                  "maxpool3s2_bwd_ex: skip range (whole planes inside the tensor)");
    MD2_CHECK_ARG((((uintptr_t)skip | (uintptr_t)dx) & 7) == 0, "maxpool3s2_bwd_ex: 8-byte aligned dx and skip");
    sk.skip = skip;
    sk.lo = (long)skip_lo;
    sk.hi = (long)skip_hi;
  }
  return maxpool_bwd(dy, arg, n, c, h, w, (h + 1) / 2, (w + 1) / 2, dx, (hipStream_t)stream, sk);
}

}  // extern "C"
