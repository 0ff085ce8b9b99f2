// Forward pass: the conv calls, BatchNorm statistics, encoder, DepthDecoder, PoseDecoder and the
// loss tail (model_impl.h).
#include "model_impl.h"

namespace md2 {

// ops of `st2` wait for everything enqueued on `st1` so far
int Model::stream_wait(hipStream_t st1, hipStream_t st2, hipEvent_t e) {
  MD2_HIP(hipEventRecord(e, st1));
  MD2_HIP(hipStreamWaitEvent(st2, e, 0));
  return MD2_OK;
}

TensorIn Model::tin(const float* p, int C, long HW) {
  TensorIn t;
  t.p0 = p;
  t.c0 = C;
  t.bs0 = (long)C * HW;
  return t;
}

TensorIn Model::frames_in(const float* x) const {
  const long fs = (long)cfg.arch.in_ch * cfg.H * cfg.W;
  TensorIn in;
  in.p0 = x;
  in.c0 = cfg.arch.in_ch;
  in.bdiv = N;          // image b = l*N + n  ->  x[n][l]
  in.bs0 = 3 * fs;
  in.bhi = fs;
  return in;
}

// closes the profile bracket of one conv pass (algorithmic FLOP)
void Model::prof_conv(hipEvent_t e, const RConv& c, const ConvShape& s, const char* pass, hipStream_t st) {
  const double flops = 2.0 * s.N * (double)s.Ho * s.Wo * s.Cout * weight_cin(s) * s.KH * s.KW;
  pf.end(e, c.cat, flops, st, pass, &s);
}

// wp / bias: other operands than the conv's own (test mode: the folded pack and t)
int Model::conv_f(RConv& c, int nimg, const TensorIn& in, float* out, long out_bs, int act, hipStream_t st,
                  const float* wp, const float* bias) {
  const ConvShape s = shape(c, nimg);
  TensorOut o;
  o.p0 = out;
  o.bs0 = out_bs;
  o.bias = wp ? bias : P(c.p.b);
  o.act = act;
  hipEvent_t e = pf.begin(st);
  MD2_TRY(conv_fwd(s, in, wp ? wp : c.wpf, o, ws_conv(), st));
  prof_conv(e, c, s, "fwd", st);
  return MD2_OK;
}

// conv + BatchNorm statistics: a split-K conv leaves its slabs to the statistics pass, which
// sums them (bit-identical to the conv's own reduction), writes y and takes the partials in one
// launch.  The profile bracket then includes that fused pass (conservative for the roofline).
// With a tail (the apply that follows) and a channel that fits in a block, statistics and apply
// are one kernel, from the slabs or from y (MD2_FUSE_BN_FWD; not when the conv's epilogue took the
// statistics); the bracket then includes the apply as well.
int Model::conv_f_bn(RConv& c, int nimg, const TensorIn& in, float* y, long out_bs, RBN& bn, long HW,
                     hipStream_t st, int slot, BNTail* tail) {
  const ConvShape s = shape(c, nimg);
  TensorOut o;
  o.p0 = y;
  o.bs0 = out_bs;
  o.bias = P(c.p.b);
  SplitKDefer d;
  // the LDS-halo forward without split-K takes the statistics in its epilogue (MD2_FUSE_BNSTATS=0:
  // the separate bn_stats_partial pass; within 1 ulp of mean / invstd, not bit-identical: the
  // fp64 sums run in another order)
  BNStatsWs wst = bn_ws(bn, nimg, HW, slot);
  if (sw.fuse_bnstats) d.stats = wst.partials;
  d.keep_reduce = !sw.fuse_splitk;
  hipEvent_t e = pf.begin(st);
  MD2_TRY(conv_fwd(s, in, c.wpf, o, ws_conv(), st, sw.fuse_splitk || sw.fuse_bnstats ? &d : nullptr));
  if (d.stats_parts > 0) {
    // (the apply passes finalise the tile partials per block, behind their own loads;
    // MD2_BN_COLLAPSE=1: one collapse launch first)
    if (sw.bn_collapse) {
      MD2_CHECK_ARG(bn.p.c <= 4096, "conv_f_bn: BN channels");
      double* col = bn_collapsed + (long)slot * 2 * 4096;
      MD2_TRY(bn_partials_collapse(wst.partials, bn.p.c, d.stats_parts, col, st));
      bn.part = col;
      bn.parts = 1;
    } else {
      bn.part = wst.partials;
      bn.parts = d.stats_parts;
    }
    prof_conv(e, c, s, "fwd", st);
    return MD2_OK;
  }
  if (tail && sw.fuse_bn_fwd && bn_channel_fits(nimg, HW)) {   // layers 3-4 at the bench shape
    if (tail->join) MD2_HIP(hipStreamWaitEvent(st, tail->join, 0));
    tail->a.y = y;
    tail->a.s1 = bn_in(bn);   // (its partials are not read)
    MD2_TRY(bn_fwd_channel(d.splits > 0 ? SlabIn{d.slab, d.splits} : SlabIn{}, y, tail->a, tail->out,
                           nimg, bn.p.c, HW, st));
    prof_conv(e, c, s, "fwd", st);
    tail->done = true;
    return MD2_OK;
  }
  if (d.splits > 0) {
    BNStatsWs w = bn_ws(bn, nimg, HW, slot);
    MD2_TRY(bn_stats_partial_slabs(SlabIn{d.slab, d.splits}, y, nimg, bn.p.c, HW, w, st));
    prof_conv(e, c, s, "fwd", st);
    return MD2_OK;
  }
  prof_conv(e, c, s, "fwd", st);
  return bn_fwd(bn, y, nimg, HW, st, slot);
}

// statistics partials only; the finalise is fused into the apply (bn_apply_fused)
BNStatsWs Model::bn_ws(RBN& bn, int nimg, long HW, int slot) {
  BNStatsWs w = bnws;
  w.partials += slot * bn_slot;
  w.parts = bn_parts(bn.p.c, nimg, HW);
  bn.part = w.partials;
  bn.parts = w.parts;
  return w;
}

int Model::bn_fwd(RBN& bn, const float* y, int nimg, long HW, hipStream_t st, int slot) {
  return bn_stats_partial(y, nimg, bn.p.c, HW, bn_ws(bn, nimg, HW, slot), st);
}

BNStatsIn Model::bn_in(const RBN& bn) {
  BNStatsIn s;
  s.part = bn.part;
  s.parts = bn.parts;
  s.gamma = P(bn.p.g);
  s.beta = P(bn.p.b);
  s.mean = bn.mean;
  s.invstd = bn.invstd;
  s.run_mean = bn.rmean;
  s.run_var = bn.rvar;
  return s;
}

// the downsample branch's conv + BN statistics (slot 1), on `st`
int Model::down_fwd(EncBlock& b, int nimg, hipStream_t st) {
  SideScratch side(ov);
  const long ohw = (long)b.H * b.W;
  return conv_f_bn(b.dconv, nimg, tin(b.in, b.Cin, (long)b.Hin * b.Win), b.yd, (long)b.C * ohw, b.dbn, ohw, st, 1);
}

int Model::encoder(const TensorIn& in, int nimg, hipStream_t st) {
  return tm.on ? encoder_fwd_test(in, nimg, st) : encoder_fwd(in, nimg, st);
}

// ---- encoder forward over nimg images (input already mapped by `in`)
int Model::encoder_fwd(const TensorIn& in, int nimg, hipStream_t st) {
  const long hw0 = (long)H0 * W0;
  MD2_TRY(conv_f_bn(stem, nimg, in, y0, 64 * hw0, stem_bn, hw0, st));
  BNApplyFused ap{};
  ap.y = y0; ap.s1 = bn_in(stem_bn); ap.relu = 1;
  if (H0 % 2 == 0 && W0 % 2 == 0 && sw.fuse_pool_fwd) {   // BN + ReLU + max pool in one pass
    MD2_TRY(bn_relu_maxpool(ap, f0, nimg, 64, H0, W0, mp, mp_arg, Hm, Wm, st));
  } else {
    MD2_TRY(bn_apply_fused(ap, f0, nimg, 64, hw0, st));
    MD2_TRY(maxpool_fwd(f0, nimg, 64, H0, W0, mp, mp_arg, Hm, Wm, st));
  }
  for (auto& sg : stages)
    for (auto& b : sg) {
      const float* x = b.in;
      int C = b.Cin;
      long HW = (long)b.Hin * b.Win;
      const bool dov = b.down && down_overlap();
      if (dov) {
        MD2_TRY(stream_wait(st, ov.side, ov.fork_ev));
        MD2_TRY(down_fwd(b, nimg, ov.side));
        MD2_HIP(hipEventRecord(ov.join_ev, ov.side));
      }
      for (size_t k = 0; k < b.st.size(); ++k) {
        EncStage& e = b.st[k];
        const long ohw = (long)e.conv.s.Ho * e.conv.s.Wo;
        const bool last = k + 1 == b.st.size();
        // the apply after this conv's BN: BN + ReLU inside the block; the block's last one adds
        // the identity residual or the downsample branch's BN before the ReLU
        BNTail t;
        t.out = e.a;
        t.a.relu = 1;
        if (last && !b.down) t.a.res = b.in;
        // The one-kernel forward reads yd, so the branch is enqueued before the conv (on the side
        // stream it is already) and the wait for it moves in front of that kernel.
        bool down_ready = false;
        if (last && b.down && sw.fuse_bn_fwd && bn_channel_fits(nimg, ohw)) {
          if (dov)
            t.join = ov.join_ev;
          else
            MD2_TRY(down_fwd(b, nimg, st));
          t.a.y2 = b.yd; t.a.s2 = bn_in(b.dbn);
          down_ready = true;
        }
        MD2_TRY(conv_f_bn(e.conv, nimg, tin(x, C, HW), e.y, (long)e.conv.p.cout * ohw, e.bn, ohw, st, 0, &t));
        if (!t.done) {   // statistics taken by conv_f_bn: the apply pass
          if (last && b.down) {
            if (dov)
              MD2_HIP(hipStreamWaitEvent(st, ov.join_ev, 0));
            else if (!down_ready)
              MD2_TRY(down_fwd(b, nimg, st));
            t.a.y2 = b.yd; t.a.s2 = bn_in(b.dbn);
          }
          t.a.y = e.y; t.a.s1 = bn_in(e.bn);
          MD2_TRY(bn_apply_fused(t.a, t.out, nimg, e.conv.p.cout, ohw, st));
        }
        x = e.a;
        C = e.conv.p.cout;
        HW = ohw;
      }
    }
  return MD2_OK;
}

// MPI mode: the decoder inputs of all levels from the target features of the last forward
int Model::mpi_embed(int nimg, int img0, hipStream_t st) {
  for (int fi = 0; fi < 5; ++fi)
    if (emb_in[fi]) {
      const long hw = (long)featH[fi] * featW[fi];
      MD2_TRY(mpi_embed_features(feat[fi] + (long)img0 * featC[fi] * hw, (long)featC[fi] * hw, nimg,
                                 featC[fi], featH[fi], featW[fi], bins, NP, (E - 1) / 2, emb_in[fi], st,
                                 featC[fi] + Ep));
    }
  return MD2_OK;
}

// ---- depth decoder over nimg images whose features start at image offset `img0`
int Model::decoder_fwd(int nimg, int img0, hipStream_t st) {
  const float* x = feat[4] + (long)img0 * featC[4] * featH[4] * featW[4];
  int C = featC[4];
  if (E > 0) {                       // decoder batch: nimg * P plane images
    MD2_TRY(mpi_embed(nimg, img0, st));
    x = emb_in[4];
    C = featC[4] + Ep;
    nimg *= NP;
  }
  for (auto& d : br) {
    const long hw = (long)d.h * d.w, hw2 = 4 * hw;
    const int co = d.b.cout;
    MD2_TRY(conv_f(d.c1, nimg, tin(x, C, hw), d.o1, co * hw, ACT_ELU, st));
    MD2_TRY(upsample2_fwd(d.o1, nimg, co, d.h, d.w, d.up, st));
    TensorIn in = tin(d.up, co, hw2);
    if (d.b.cskip > 0) {
      const int fi = 4 - d.b.bid;
      if (E > 0) {
        in.p1 = emb_in[fi];
        in.bs1 = (long)(featC[fi] + Ep) * hw2;
      } else {
        in.p1 = feat[fi] + (long)img0 * featC[fi] * hw2;
        in.bs1 = (long)featC[fi] * hw2;
      }
    }
    MD2_TRY(conv_f(d.c2, nimg, in, d.o2, co * hw2, ACT_ELU, st));
    x = d.o2;
    C = co;
  }
  HeadJob jobs[MAX_HEADS];
  const int nh = head_jobs(jobs, nimg);
  hipEvent_t e = pf.begin(st);
  MD2_TRY(heads_fwd(jobs, nh, ACT_SIGMOID, st));
  pf.end(e, PROF_CONV_OTHER, heads_flops(nimg), st, "heads fwd");
  return MD2_OK;
}

int Model::head_jobs(HeadJob* jobs, int nimg) {
  int n = 0;
  for (DecBranch* h : heads) {
    DecBranch& d = *h;
    HeadJob& j = jobs[n++];
    j = HeadJob{};
    const long hw2 = 4L * d.h * d.w;
    j.x = conv_head_in(tin(d.o2, d.b.cout, hw2));
    j.wf = conv_head_w(d.hc.s, 0, d.hc.wpf);
    j.wd = conv_head_w(d.hc.s, 1, d.hc.wpd);
    j.Cin = d.b.cout;
    j.H = 2 * d.h;
    j.W = 2 * d.w;
    j.N = nimg;
    j.bias = P(d.hc.p.b);
    j.y = d.disp;
    j.ybs = hw2;
    j.dy = d.d_head;
    j.dx = d.d_o2;
    j.dxbs = (long)d.b.cout * hw2;
    j.dw = grads + d.hc.p.w;
    j.db = Gd(d.hc.p.b);
  }
  return n;
}

double Model::heads_flops(int nimg) const {
  double f = 0.0;
  for (const DecBranch* d : heads) f += 2.0 * nimg * 4.0 * d->h * d->w * 9.0 * d->b.cout;
  return f;
}

// PoseDecoder input of the 2N pairs: in place for the default ids, else the gathered pin
TensorIn Model::pose_pairs_in(long hw4) {
  if (!pairs_inplace) return tin(pin, 512, hw4);
  TensorIn in = tin(sqo, 256, hw4);
  in.p1 = sqo + (long)N * 256 * hw4;   // pair (frame s, frame s+1) = images (q, q+N)
  in.bs1 = 256 * hw4;
  return in;
}

int Model::pose_fwd(hipStream_t st) {
  SideScratch side(ov);
  const long hw4 = (long)featH[4] * featW[4];
  MD2_TRY(conv_f(sq, B, tin(feat[4], featC[4], hw4), sqo, 256 * hw4, ACT_RELU, st));
  if (!pairs_inplace) MD2_TRY(pair_gather(sqo, N, 256, hw4, pa, pb, pin, st));
  MD2_TRY(conv_f(p1, 2 * N, pose_pairs_in(hw4), pc1, 256 * hw4, ACT_RELU, st));
  MD2_TRY(conv_f(p2, 2 * N, tin(pc1, 256, hw4), pc2, 256 * hw4, ACT_RELU, st));
  return pose_head_fwd(pc2, 2 * N, 256, hw4, P(spec.p3.w), P(spec.p3.b), means, pose, st);
}

// Pose-only inference on n consecutive frames (images 0..n-1 of `in`): the encoder, the squeezer on
// the n images, then the PoseDecoder on the n-1 pairs (i, i+1).  Consecutive pairs need no gather:
// the second half of pair i is image i+1, one image stride further into sqo (pose_pairs_in's trick
// with a shift of 1 instead of N).  Fits the buffers for n <= 2N+1 (<= 3N images, <= 2N pairs).
int Model::eval_pose(const TensorIn& in, int n, hipStream_t st) {
  MD2_TRY(encoder(in, n, st));
  SideScratch side(ov);   // the pose convs' workspace is the side one (pose_fwd)
  const long hw4 = (long)featH[4] * featW[4];
  MD2_TRY(conv_f(sq, n, tin(feat[4], featC[4], hw4), sqo, 256 * hw4, ACT_RELU, st));
  TensorIn pairs = tin(sqo, 256, hw4);
  pairs.p1 = sqo + 256 * hw4;
  pairs.bs1 = 256 * hw4;
  MD2_TRY(conv_f(p1, n - 1, pairs, pc1, 256 * hw4, ACT_RELU, st));
  MD2_TRY(conv_f(p2, n - 1, tin(pc1, 256, hw4), pc2, 256 * hw4, ACT_RELU, st));
  return pose_head_fwd(pc2, n - 1, 256, hw4, P(spec.p3.w), P(spec.p3.b), means, pose, st);
}

// (m)(x, source_ids, target_id) (src/model.jl:31-55): encoder on the 3N frames, DepthDecoder on
// the targets, PoseDecoder on the pairs -- disparities and poses, no loss tail
int Model::forward(const float* x, hipStream_t st) {
  MD2_TRY(encoder(frames_in(x), B, st));
  if (pose_overlap()) {
    MD2_TRY(stream_wait(st, ov.side, ov.fork_ev));
    MD2_TRY(pose_fwd(ov.side));
    MD2_TRY(decoder_fwd(N, T0, st));
    MD2_TRY(stream_wait(ov.side, st, ov.join_ev));
  } else {
    MD2_TRY(decoder_fwd(N, T0, st));
    MD2_TRY(pose_fwd(st));
  }
  return MD2_OK;
}

// x_net feeds the networks; the automask and the loss tail read x (x_net == x: the plain step)
int Model::ensure_stereo_ws() {
  if (tail_src_ws) return MD2_OK;
  float* q;
  MD2_TRY(alloc(&q, loss_tail_sources_workspace_bytes(tail, MAX_SOURCES) / sizeof(float) + 64));
  tail_src_ws = q;
  if (!amask) MD2_TRY(alloc(&amask, (long)N * cfg.H * cfg.W));
  return MD2_OK;
}

// stereo: the loss tail and the automask run over (src0, src1, stereo frame) -- MS -- or over the
// stereo frame alone -- S, where the pose network's cotangent is zero; the networks never see it
int Model::forward_loss(const float* x, const float* x_net, const float* automask, float* loss, float* terms,
                        hipStream_t st, const StereoIn* stereo) {
  MD2_TRY(forward(x_net, st));
  const float* disps[MAX_SCALES] = {};
  LossTailOut o{};
  for (size_t li = 0; li < heads.size(); ++li) {
    disps[li] = heads[li]->disp;
    o.d_disp[li] = heads[li]->d_head;
  }
  o.loss = loss ? loss : loss_buf;
  o.terms = terms;
  o.d_pose = E > 0 ? d_pose_rep : d_pose;
  hipEvent_t pev[2 * MAX_SCALES] = {};
  if (pf.on) {
    for (int k = 0; k < 2; ++k) pev[k] = pf.ev();
    o.photo_events = pev;
  }
  // the sources form of the tail: a stereo source, or per-sample intrinsics (set_intrinsics), which
  // always run on the kernel over sources -- M is then {src0, src1} learned
  if (stereo || intr_on) {
    const long fs = tail.x_frame_stride, ss = tail.x_sample_stride;
    LossSource src[MAX_SOURCES];
    int S = 0;
    if (!stereo || stereo->temporal) {
      src[S++] = LossSource{x + tail.src0 * fs, ss, 0, tail.invert_mask & 1, nullptr};
      src[S++] = LossSource{x + tail.src1 * fs, ss, 1, (tail.invert_mask >> 1) & 1, nullptr};
    }
    if (stereo) src[S++] = LossSource{stereo->x, fs, -1, 0, stereo->Rt};
    const float* target = x + tail.target * fs;
    if (cfg.automask && !automask) {   // over the same sources the loss uses
      const float* fr[MAX_SOURCES];
      long fss[MAX_SOURCES];
      for (int s = 0; s < S; ++s) {
        fr[s] = src[s].frames;
        fss[s] = src[s].sample_stride;
      }
      MD2_TRY(launch_automask_sources(target, ss, fr, fss, S, N, cfg.arch.in_ch, cfg.H, cfg.W, amask, st));
      automask = amask;
    }
    // S: no learned source, so the tail writes no d_pose; the pose network still runs its backward
    // (the segments, the DP buckets and the graph keep their shape) on a zero cotangent
    if (stereo && !stereo->temporal) MD2_HIP(hipMemsetAsync(d_pose, 0, sizeof(float) * 2 * N * 6, st));
    MD2_TRY(loss_tail_sources_run(tail, S, src, target, ss, disps, pose, cfg.automask ? automask : nullptr, 1.f,
                                  o, tail_src_ws, st, intr_on ? Kn : nullptr, intr_on ? invKn : nullptr));
    if (pf.on) {
      const double bytes = (double)tail.nscales * ND * cfg.H * cfg.W * (8.0 + 4.0 * (1 + S) * cfg.arch.in_ch);
      pf.recs.push_back({pev[0], pev[1], PROF_PHOTO, bytes, "photometric over sources (all scales)"});
    }
    return MD2_OK;
  }
  if (cfg.automask && !automask) {
    // automasking_loss(ssim, x, target; source_ids) (src/training.jl:9-11): identity
    // reprojection of the raw sources, the third candidate of every scale's per-pixel min
    MD2_TRY(launch_automask(x, tail.x_sample_stride, tail.x_frame_stride, tail.target, tail.src0,
                            tail.src1, N, cfg.arch.in_ch, cfg.H, cfg.W, amask, st));
    automask = amask;
  }
  const float* tail_pose = pose;
  if (E > 0) {
    // every plane of a sample warps with that sample's poses and is compared with its frames
    MD2_TRY(repeat_rows(pose, 2L * N, 6, NP, pose_rep, st));
    tail_pose = pose_rep;
    if (cfg.automask) {
      MD2_TRY(repeat_rows(automask, N, cfg.H * cfg.W, NP, amask_rep, st));
      automask = amask_rep;
    }
  }
  MD2_TRY(loss_tail_run(tail, disps, tail_pose, x, cfg.automask ? automask : nullptr, 1.f, o, tail_ws, st));
  if (E > 0) MD2_TRY(repeat_rows_adjoint(d_pose_rep, 2L * N, 6, NP, d_pose, st));
  if (pf.on) {
    // one launch for all scales; algorithmic bytes per full-res pixel and scale:
    // disparity 4 + target 4C + two sources 8C + d_disp 4
    const double bytes = (double)tail.nscales * ND * cfg.H * cfg.W * (8.0 + 12.0 * cfg.arch.in_ch);
    pf.recs.push_back({pev[0], pev[1], PROF_PHOTO, bytes, "photometric (all scales)"});
  }
  return MD2_OK;
}

}  // namespace md2
