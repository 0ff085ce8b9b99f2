// Backward pass: filter and data gradients, BatchNorm backward, and the six backward segments
// (decoders, layer 4 ... layer 1, stem) of model_backward_segment (model_impl.h).
#include "model_impl.h"

namespace md2 {

int Model::y_claim(int j, hipStream_t st) {
  if (ov.y_pending[j]) MD2_HIP(hipStreamWaitEvent(st, ov.ev_y[j], 0));
  ov.y_pending[j] = false;
  return MD2_OK;
}

int Model::conv_w(RConv& c, int nimg, const TensorIn& in, const float* dy, hipStream_t st) {
  const ConvShape s = shape(c, nimg);
  hipEvent_t e = pf.begin(st);
  MD2_TRY(conv_wgrad(s, in, dy, grads + c.p.w, Gd(c.p.b), 0, ws_conv(), st, c.p.b >= 0 ? bp_pending : nullptr,
                     bp_parts));
  bp_pending = nullptr;
  prof_conv(e, c, s, "wgrad", st);
  return MD2_OK;
}

// filter and data gradient of one conv from the same dY.  (Running the filter gradient on a
// second stream overlapped them but each slowed by as much, and the cross-queue fork/join
// added ~1.3 ms/step of idle gaps: measured slower, so both stay on `st`.)
int Model::conv_wd(RConv& c, int nimg, const TensorIn& in, const float* dy, float* dx, long dx_bs, int acc,
                   hipStream_t st, float* dx1, long dx1_bs, int c0) {
  MD2_TRY(conv_w(c, nimg, in, dy, st));
  return conv_d(c, nimg, dy, dx, dx_bs, acc, st, dx1, dx1_bs, c0);
}

// filter gradient on the side stream (its own scratch) once `st` has reached `ready`; `done`
// marks the side's last read of dy
int Model::conv_w_side(RConv& c, int nimg, const TensorIn& in, const float* dy, hipEvent_t ready,
                       hipEvent_t done, hipStream_t st) {
  MD2_TRY(stream_wait(st, ov.side, ready));
  {
    SideScratch side(ov);
    MD2_TRY(conv_w(c, nimg, in, dy, ov.side));
  }
  MD2_HIP(hipEventRecord(done, ov.side));
  return MD2_OK;
}

int Model::conv_d(RConv& c, int nimg, const float* dy, float* dx, long dx_bs, int acc, hipStream_t st,
                  float* dx1, long dx1_bs, int c0) {
  const ConvShape s = shape(c, nimg);
  TensorOut o;
  o.p0 = dx;
  o.bs0 = dx_bs;
  o.p1 = dx1;
  o.bs1 = dx1_bs;
  o.c0 = c0;
  o.accumulate = acc;
  hipEvent_t e = pf.begin(st);
  MD2_TRY(conv_dgrad(s, dy, c.wpd, o, ws_conv(), st));
  prof_conv(e, c, s, "dgrad", st);
  return MD2_OK;
}

// dgrad into DA followed by the backward of the residual-free BN+ReLU that produced the conv's
// input (ReLU mask re-derived from y): a split-K dgrad leaves its slabs to bn_bwd_partial, which
// forms DA in the same pass (profile bracket includes it, as conv_f_bn)
int Model::conv_d_bn(RConv& c, int nimg, const float* dy, float* da, long da_bs, RBN& bn, const float* y,
                     long HW, float* dyprev, hipStream_t st) {
  const ConvShape s = shape(c, nimg);
  TensorOut o;
  o.p0 = da;
  o.bs0 = da_bs;
  SplitKDefer d;
  hipEvent_t e = pf.begin(st);
  MD2_TRY(conv_dgrad(s, dy, c.wpd, o, ws_conv(), st, sw.fuse_splitk ? &d : nullptr));
  if (d.splits == 0) {
    prof_conv(e, c, s, "dgrad", st);
    return bn_bwd(bn, da, nullptr, y, nimg, HW, dyprev, nullptr, 0, st, true);
  }
  BNBwd b = bn_bwd_desc(bn, y, dyprev, true);
  b.slabs = SlabIn{d.slab, d.splits};
  if (sw.fuse_bn_bwd && bn_channel_fits(nimg, HW)) {
    // the slabs are summed in the block's registers: DA (read by this backward alone) is not written
    MD2_TRY(bn_bwd_channel(b, nimg, bn.p.c, HW, st));
    prof_conv(e, c, s, "dgrad", st);
    return MD2_OK;
  }
  BNStatsWs w = bnws;
  w.parts = bn_parts(bn.p.c, nimg, HW);
  MD2_TRY(bn_bwd_partial_slabs(b, da, nimg, bn.p.c, HW, w, st));
  prof_conv(e, c, s, "dgrad", st);
  b.slabs = SlabIn{};
  b.dout = da;
  return bn_bwd_apply_fused(b, nimg, bn.p.c, HW, w, st);
}

int Model::act_bias(const float* out, const float* dout, float* dpre, int nimg, int C, long HW, int act,
                    hipStream_t st, float* bp_buf) {
  if (HW % 4 != 0 || (long)C * act_bias_parts(C, nimg, HW) > BP_WS) {
    bp_pending = nullptr;
    return act_backward(out, dout, dpre, (long)nimg * C * HW, act, st);
  }
  float* bp = bp_buf ? bp_buf : ws_bp();
  MD2_TRY(act_backward_bias(out, dout, dpre, nimg, C, HW, act, bp, st));
  bp_pending = bp;
  bp_parts = act_bias_parts(C, nimg, HW);
  return MD2_OK;
}

// the operands every backward of `bn` shares; relu_from_y: a residual-free BN+ReLU (stem,
// intra-block), whose ReLU mask is re-derived from y (bit-exact, one read less)
BNBwd Model::bn_bwd_desc(RBN& bn, const float* y, float* dy, bool relu_from_y) {
  BNBwd b;
  b.y = y;
  b.mean = bn.mean;
  b.invstd = bn.invstd;
  b.gamma = P(bn.p.g);
  b.mbeta = relu_from_y ? P(bn.p.b) : nullptr;
  b.dgamma = Gd(bn.p.g);
  b.dbeta = Gd(bn.p.b);
  b.dy = dy;
  return b;
}

// mask: the BN+ReLU output whose ReLU gates dout (ignored with relu_from_y)
int Model::bn_bwd(RBN& bn, const float* dout, const float* mask, const float* y, int nimg, long HW, float* dy,
                  float* dres, int dres_acc, hipStream_t st, bool relu_from_y, SkipAdd sk, int slot) {
  BNStatsWs w = bnws;
  w.partials += slot * bn_slot;
  w.parts = bn_parts(bn.p.c, nimg, HW);
  BNBwd b = bn_bwd_desc(bn, y, dy, relu_from_y);
  b.dout = dout;
  b.mask = relu_from_y ? nullptr : mask;
  b.dres = dres;
  b.dres_accumulate = dres_acc;
  b.skip = sk;
  if (sw.fuse_bn_bwd && bn_channel_fits(nimg, HW))   // layers 3-4 at the bench shape: one launch
    return bn_bwd_channel(b, nimg, bn.p.c, HW, st);
  MD2_TRY(bn_bwd_partial(b, nimg, bn.p.c, HW, w, st));
  return bn_bwd_apply_fused(b, nimg, bn.p.c, HW, w, st);
}

// the decoder skip gradient d_skip[si] on the target slice of encoder feature si (si = 1..3, the
// input of stage si = the output of stage si-1): added by stage si-1's last-block BN backward
// when fused (MD2_FUSE_SKIP_BWD, HW % 4 == 0), else by an axpy after stage si's backward
bool Model::skip_fused(int si) const {
  return sw.fuse_skip_bwd && si >= 1 && si <= 3 && d_skip[si] && ((long)featH[si] * featW[si]) % 4 == 0;
}

SkipAdd Model::skip_add(int si) const {
  SkipAdd sk;
  if (!skip_fused(si)) return sk;
  const long fsz = (long)featC[si] * featH[si] * featW[si];
  sk.skip = d_skip[si];
  sk.lo = (long)T0 * fsz;
  sk.hi = (long)(T0 + N) * fsz;
  return sk;
}

int Model::block_bwd(EncBlock& b, hipStream_t st, SkipAdd sk, bool eov) {
  const int nimg = B;
  const long ohw = (long)b.H * b.W, ihw = (long)b.Hin * b.Win;
  const int ns = (int)b.st.size();
  EncStage& last = b.st.back();
  // last BN (+ residual, ReLU): g = (d_out [+ skip]) * relu'(out)
  MD2_TRY(y_claim(ov.ycur, st));
  MD2_TRY(bn_bwd(last.bn, b.d_out, last.a, last.y, nimg, ohw, ybuf(ov.ycur), b.down ? G : b.d_in, 0, st,
                 false, sk));
  const bool dov = b.down && down_overlap();
  if (b.down) {
    // downsample branch: BN backward (partials slot 1) + the 1x1 conv's filter and data
    // gradients (d_in written whole; the chain's first conv adds to it below)
    hipStream_t sd = dov ? ov.side : st;
    if (dov) MD2_TRY(stream_wait(st, ov.side, ov.fork_ev));
    MD2_TRY(bn_bwd(b.dbn, G, nullptr, b.yd, nimg, ohw, DYD, nullptr, 0, sd, false, SkipAdd{}, 1));
    {
      SideScratch side(ov);
      MD2_TRY(conv_wd(b.dconv, nimg, tin(b.in, b.Cin, ihw), DYD, b.d_in, (long)b.Cin * ihw, 0, sd));
    }
    if (dov) MD2_HIP(hipEventRecord(ov.join_ev, ov.side));
  }
  for (int k = ns - 1; k >= 0; --k) {
    EncStage& e = b.st[k];
    const float* xin = k == 0 ? b.in : b.st[k - 1].a;
    const int cin = e.conv.p.cin;
    const long hin = (long)e.conv.s.H * e.conv.s.W;
    float* dy = ybuf(ov.ycur);
    // MD2_ENC_WGRAD_MAIN0=1 (tuning): the first conv's filter gradient of each block stays on
    // the model stream, after its data gradient (balances the side stream's share)
    const bool wmain = eov && k == 0 && sw.enc_wgrad_main0;
    if (eov && !wmain) {   // filter gradient beside the data gradient; dy untouched until ev_y[ycur]
      MD2_TRY(conv_w_side(e.conv, nimg, tin(xin, cin, hin), dy, ov.fork_ev, ov.ev_y[ov.ycur], st));
      ov.y_pending[ov.ycur] = true;
    } else if (!wmain) {
      MD2_TRY(conv_w(e.conv, nimg, tin(xin, cin, hin), dy, st));
    }
    if (k > 0) {
      EncStage& pe = b.st[k - 1];
      const int nx = ov.ycur ^ 1;
      MD2_TRY(y_claim(nx, st));
      MD2_TRY(conv_d_bn(e.conv, nimg, dy, DA, (long)cin * hin, pe.bn, pe.y, hin, ybuf(nx), st));
      ov.ycur = nx;
    } else {
      if (dov) MD2_HIP(hipStreamWaitEvent(st, ov.join_ev, 0));   // b.d_in written by the 1x1 dgrad
      MD2_TRY(conv_d(e.conv, nimg, dy, b.d_in, (long)cin * hin, 1, st));
      if (wmain) MD2_TRY(conv_w(e.conv, nimg, tin(xin, cin, hin), dy, st));
    }
  }
  return MD2_OK;
}

// PoseDecoder backward: d_pose -> pose parameter gradients and the layer-4 feature gradient
// d_f4 (written whole by the squeezer's dgrad; the DepthDecoder's first branch adds to it)
int Model::pose_bwd(hipStream_t st) {
  SideScratch side(ov);
  const long hw4 = (long)featH[4] * featW[4];
  float* DP = DPRE_side;
  MD2_TRY(pose_head_bwd(d_pose, 2 * N, 256, hw4, P(spec.p3.w), means, DP, Gd(spec.p3.w),
                        Gd(spec.p3.b), st));
  MD2_TRY(act_bias(pc2, DP, DP, 2 * N, 256, hw4, ACT_RELU, st));
  MD2_TRY(conv_wd(p2, 2 * N, tin(pc1, 256, hw4), DP, d_pc1, 256 * hw4, 0, st));
  MD2_TRY(act_bias(pc1, d_pc1, d_pc1, 2 * N, 256, hw4, ACT_RELU, st));
  MD2_TRY(conv_wd(p1, 2 * N, pose_pairs_in(hw4), d_pc1, d_pin, 512 * hw4, 0, st));
  MD2_TRY(pair_grad_gather(d_pin, N, 256, hw4, pa, pb, d_sq, st));
  MD2_TRY(act_bias(sqo, d_sq, d_sq, B, 256, hw4, ACT_RELU, st));
  float* d_f4 = stages[3].back().d_out;
  return conv_wd(sq, B, tin(feat[4], featC[4], hw4), d_sq, d_f4, (long)featC[4] * hw4, 0, st);
}

int Model::seg_decoder(hipStream_t st) {
  // ---- PoseDecoder backward: beside the DepthDecoder's on the side stream, or first
  const bool pov = pose_overlap();
  if (pov) {
    MD2_TRY(stream_wait(st, ov.side, ov.fork_ev));
    MD2_TRY(pose_bwd(ov.side));
    MD2_HIP(hipEventRecord(ov.join_ev, ov.side));
  } else {
    MD2_TRY(pose_bwd(st));
  }
  float* d_f4 = stages[3].back().d_out;
  // ---- DepthDecoder backward (reverse branch order), over ND decoder images
  const int nb = (int)br.size();
  {
    // every head's data + filter gradient first (their d_head all come from the loss tail):
    // d_o2 of a head branch is then the head's dx, and the next branch's c1 dgrad adds to it
    HeadJob jobs[MAX_HEADS];
    const int nh = head_jobs(jobs, ND);
    hipEvent_t e = pf.begin(st);
    MD2_TRY(heads_bwd(jobs, nh, hws, heads_bwd_workspace(jobs, nh) + 256, st));
    pf.end(e, PROF_CONV_OTHER, 2.0 * heads_flops(ND), st, "heads bwd");
  }
  const bool wov = wgrad_overlap();
  float* const bpc2 = bp_dec[0];
  float* const bpc1 = bp_dec[1];
  for (int i = nb - 1; i >= 0; --i) {
    DecBranch& d = br[i];
    const long hw = (long)d.h * d.w, hw2 = 4 * hw;
    const int co = d.b.cout;
    if (wov && i < nb - 1) MD2_HIP(hipStreamWaitEvent(st, ov.ev_c2, 0));   // DPRE, bpc2 free
    MD2_TRY(act_bias(d.o2, d.d_o2, DPRE, ND, co, hw2, ACT_ELU, st, wov ? bpc2 : nullptr));
    TensorIn in = tin(d.up, co, hw2);
    float* dskip = nullptr;
    long skip_bs = 0;
    if (d.b.cskip > 0) {
      const int fi = 4 - d.b.bid;
      if (E > 0) {
        in.p1 = emb_in[fi];
        in.bs1 = (long)(featC[fi] + Ep) * hw2;
        dskip = d_emb[fi];
        skip_bs = (long)(featC[fi] + Ep) * hw2;
      } else {
        in.p1 = feat[fi] + (long)T0 * featC[fi] * hw2;
        in.bs1 = (long)featC[fi] * hw2;
        dskip = d_skip[fi];
        skip_bs = (long)featC[fi] * hw2;
      }
    }
    if (wov) {
      MD2_TRY(conv_w_side(d.c2, ND, in, DPRE, ov.ev_a, ov.ev_c2, st));
      MD2_TRY(conv_d(d.c2, ND, DPRE, DUP, co * hw2, 0, st, dskip, skip_bs, co));
    } else {
      MD2_TRY(conv_wd(d.c2, ND, in, DPRE, DUP, co * hw2, 0, st, dskip, skip_bs, co));
    }
    if (E > 0 && d.b.cskip > 0) {
      // _repeat pullback: the skip gradient of the target features = sum over the planes
      const int fi = 4 - d.b.bid;
      MD2_TRY(plane_sum(d_emb[fi], N, NP, featC[fi] + Ep, featC[fi], hw2, d_skip[fi], 0, st));
    }
    if (wov && i < nb - 1) MD2_HIP(hipStreamWaitEvent(st, ov.ev_c1, 0));   // DO1, bpc1 free
    MD2_TRY(upsample2_bwd(DUP, ND, co, d.h, d.w, DO1, st));
    MD2_TRY(act_bias(d.o1, DO1, DO1, ND, co, hw, ACT_ELU, st, wov ? bpc1 : nullptr));
    const float* xin;
    int cin;
    float* dx;
    int acc;
    if (i == 0 && pov) MD2_HIP(hipStreamWaitEvent(st, ov.join_ev, 0));   // d_f4 written by the squeezer
    if (i == 0 && E > 0) {
      cin = featC[4] + Ep;
      xin = emb_in[4];
      dx = d_emb[4];
      acc = 0;
    } else if (i == 0) {
      cin = featC[4];
      xin = feat[4] + (long)T0 * cin * hw;
      dx = d_f4 + (long)T0 * cin * hw;
      acc = 1;
    } else {
      cin = br[i - 1].b.cout;
      xin = br[i - 1].o2;
      dx = br[i - 1].d_o2;
      acc = br[i - 1].head >= 0 ? 1 : 0;   // on top of the head's dx
    }
    if (wov) {
      MD2_TRY(conv_w_side(d.c1, ND, tin(xin, cin, hw), DO1, ov.ev_b, ov.ev_c1, st));
      MD2_TRY(conv_d(d.c1, ND, DO1, dx, (long)cin * hw, acc, st));
    } else {
      MD2_TRY(conv_wd(d.c1, ND, tin(xin, cin, hw), DO1, dx, (long)cin * hw, acc, st));
    }
    if (i == 0 && E > 0)
      MD2_TRY(plane_sum(d_emb[4], N, NP, cin, featC[4], hw, d_f4 + (long)T0 * featC[4] * hw, 1, st));
  }
  // every decoder filter gradient final: the side runs in order, so its last event covers all
  if (wov) MD2_HIP(hipStreamWaitEvent(st, ov.ev_c1, 0));
  return MD2_OK;
}

int Model::seg_stage(int si, hipStream_t st) {
  auto& sg = stages[si];
  for (int k = (int)sg.size() - 1; k >= 0; --k)
    MD2_TRY(block_bwd(sg[k], st, k == (int)sg.size() - 1 ? skip_add(si + 1) : SkipAdd{}, enc_overlap(si)));
  for (int j = 0; j < 2; ++j) MD2_TRY(y_claim(j, st));   // the stage's filter gradients final
  if (si >= 1 && !skip_fused(si)) {
    // d f_si (= block 0's d_in) += decoder skip gradient on the target slice
    const long n = (long)N * featC[si] * featH[si] * featW[si];
    MD2_TRY(axpy(sg[0].d_in + (long)T0 * featC[si] * featH[si] * featW[si], d_skip[si], n, st));
  }
  return MD2_OK;
}

int Model::seg_stem(hipStream_t st) {
  const long hw0 = (long)H0 * W0;
  const long n = (long)N * 64 * hw0;
  if (W0 % 2 == 0 && sw.fuse_pool_bwd && d_skip[0]) {
    // the decoder skip gradient added by the max-pool adjoint itself (no axpy pass)
    SkipAdd sk;
    sk.skip = d_skip[0];
    sk.lo = (long)T0 * 64 * hw0;
    sk.hi = sk.lo + n;
    MD2_TRY(maxpool_bwd(d_mp, mp_arg, B, 64, H0, W0, Hm, Wm, d_f0, st, sk));
  } else {
    MD2_TRY(maxpool_bwd(d_mp, mp_arg, B, 64, H0, W0, Hm, Wm, d_f0, st));
    MD2_TRY(axpy(d_f0 + (long)T0 * 64 * hw0, d_skip[0], n, st));
  }
  MD2_TRY(bn_bwd(stem_bn, d_f0, f0, y0, B, hw0, DY, nullptr, 0, st, true));
  return conv_w(stem, B, frames_in(cur_x), DY, st);
}

// caller cotangents (d disp per level, d pose) of a forward-only call: the head pullback and
// the pose gradient buffers the backward segments read, as the fused loss tail writes them
int Model::set_cotangents(const float* const* d_disp, const float* d_pose_in, hipStream_t st) {
  for (size_t li = 0; li < heads.size(); ++li) {
    DecBranch& d = *heads[li];
    MD2_TRY(sigmoid_cotangent(d_disp ? d_disp[li] : nullptr, d.disp, d.d_head, (long)ND * 4 * d.h * d.w, st));
  }
  if (d_pose_in) MD2_HIP(hipMemcpyAsync(d_pose, d_pose_in, sizeof(float) * 12 * N, hipMemcpyDefault, st));
  else MD2_HIP(hipMemsetAsync(d_pose, 0, sizeof(float) * 12 * N, st));
  return MD2_OK;
}

}  // namespace md2
