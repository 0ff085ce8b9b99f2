// Test mode: the BatchNorm-folded inference encoder and the running statistics as model state
// (TestMode in model_impl.h, testmode.h).
#include "model_impl.h"

namespace md2 {

int Model::testmode_alloc() {
  if (tm.wfold) return MD2_OK;
  MD2_TRY(alloc(&tm.wfold, spec.depth_begin));
  MD2_TRY(alloc(&tm.st, bn_layout.off[bn_layout.n]));
  std::vector<FoldJob> fj;
  std::vector<PackJob> pj;
  int k = 0;
  auto job = [&](RConv* c, RBN& bn) -> int {
    bn.ts = tm.st + bn_layout.off[k++];
    bn.tt = bn.ts + bn.p.c;
    FoldJob j;
    j.gamma = P(bn.p.g); j.beta = P(bn.p.b);
    j.mean = bn.rmean; j.var = bn.rvar;
    j.s = bn.ts; j.t = bn.tt;
    j.Cout = bn.p.c;
    if (c) {
      const long per = (long)c->p.cin * c->p.k * c->p.k;
      MD2_CHECK_ARG(per % 4 == 0 && c->p.cout == bn.p.c, "test mode: conv weight rows of 4n floats");
      j.w = params + c->p.w;
      j.wf = tm.wfold + c->p.w;
      j.per4 = (int)(per / 4);
      MD2_TRY(alloc(&c->wpt, conv_fwd_packed_elems(c->s)));
      MD2_HIP(hipMemset(c->wpt, 0, conv_fwd_packed_elems(c->s) * sizeof(float)));
      pj.push_back(conv_pack_job(c->s, j.wf, c->wpt, nullptr));
    }
    fj.push_back(j);
    return MD2_OK;
  };
  MD2_TRY(job(nullptr, stem_bn));
  for (auto& sg : stages)
    for (auto& b : sg) {
      for (auto& e : b.st) MD2_TRY(job(&e.conv, e.bn));
      if (b.down) MD2_TRY(job(&b.dconv, b.dbn));
    }
  tm.fold_blocks = 0;
  for (auto& j : fj) {
    j.block_begin = tm.fold_blocks;
    tm.fold_blocks += bn_fold_job_blocks(j);
  }
  tm.pack_blocks = 0;
  for (auto& j : pj) {
    j.block_begin = tm.pack_blocks;
    tm.pack_blocks += conv_pack_job_blocks(j);
  }
  MD2_TRY(upload(fj, &tm.fold_jobs, true));
  tm.fold_njobs = (int)fj.size();
  MD2_TRY(upload(pj, &tm.pack_jobs, true));
  tm.pack_njobs = (int)pj.size();
  return MD2_OK;
}

// (s, t) and the folded packs from the current parameters and running statistics
int Model::refold(hipStream_t st) {
  MD2_TRY(bn_fold_batch(tm.fold_jobs, tm.fold_njobs, tm.fold_blocks, 1e-5, st));
  return conv_pack_batch(tm.pack_jobs, tm.pack_njobs, tm.pack_blocks, st);
}

// a folded conv: bias t, ReLU where one follows directly
int Model::conv_f_t(RConv& c, int nimg, const TensorIn& in, float* out, const RBN& bn, int act, hipStream_t st) {
  return conv_f(c, nimg, in, out, (long)c.s.Cout * c.s.Ho * c.s.Wo, act, st, c.wpt, bn.tt);
}

// The test-mode encoder: no statistics or apply pass.  The activations land in the buffers of
// the train-mode forward (md2_model_features / md2_model_debug_tensor read them as before;
// "....conv<k>.y" of a conv followed by a ReLU is not written).  The downsample branch runs on
// the model stream (three or four 1x1 convs per forward: the side-stream overlap is dropped
// here); the pose branch keeps its overlap (forward()).
int Model::encoder_fwd_test(const TensorIn& in, int nimg, hipStream_t st) {
  const long hw0 = (long)H0 * W0;
  MD2_TRY(conv_f(stem, nimg, in, y0, 64 * hw0, ACT_NONE, st));
  {
    hipEvent_t e = pf.begin(st);
    MD2_TRY(affine_relu_maxpool(y0, stem_bn.ts, stem_bn.tt, nimg, 64, H0, W0, f0, mp, st));
    pf.end(e, PROF_NCAT, 4.0 * nimg * 64 * (2.0 * hw0 + (double)Hm * Wm), st, "affine_relu_maxpool");
  }
  for (auto& sg : stages)
    for (auto& b : sg) {
      const float* x = b.in;
      int C = b.Cin;
      long HW = (long)b.Hin * b.Win;
      for (size_t k = 0; k < b.st.size(); ++k) {
        EncStage& e = b.st[k];
        const bool last = k + 1 == b.st.size();
        MD2_TRY(conv_f_t(e.conv, nimg, tin(x, C, HW), last ? e.y : e.a, e.bn, last ? ACT_NONE : ACT_RELU, st));
        x = e.a;
        C = e.conv.p.cout;
        HW = (long)e.conv.s.Ho * e.conv.s.Wo;
      }
      EncStage& last = b.st.back();
      const float* res = b.in;
      if (b.down) {
        SideScratch side(ov);   // the downsample conv's split-K workspace is sized on the side set
        MD2_TRY(conv_f_t(b.dconv, nimg, tin(b.in, b.Cin, (long)b.Hin * b.Win), b.yd, b.dbn, ACT_NONE, st));
        res = b.yd;
      }
      const long n = (long)nimg * b.C * b.H * b.W;
      hipEvent_t e = pf.begin(st);
      MD2_TRY(add_relu(last.y, res, last.a, n, st));
      pf.end(e, PROF_NCAT, 12.0 * n, st, "add_relu");
    }
  return MD2_OK;
}

int model_get_bn_stats(Model* m, float* out, hipStream_t st) {
  MD2_CHECK_ARG(m && out, "get_bn_stats args");
  MD2_TRY(m->adam_join(st));
  MD2_HIP(hipMemcpyAsync(out, m->bn_stats, sizeof(float) * (size_t)m->bn_layout.off[m->bn_layout.n],
                         hipMemcpyDeviceToDevice, st));
  return MD2_OK;
}

int model_set_bn_stats(Model* m, const float* in, hipStream_t st) {
  MD2_CHECK_ARG(m && in && in != m->bn_stats, "set_bn_stats args");
  MD2_TRY(m->adam_join(st));
  // checked on the device; only the 4-byte verdict crosses to the host
  MD2_HIP(hipMemsetAsync(m->bn_flag, 0, sizeof(int), st));
  MD2_TRY(bn_stats_validate(in, m->bn_layout, m->bn_flag, st));
  int bad = 0;
  MD2_HIP(hipMemcpyAsync(&bad, m->bn_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  MD2_HIP(hipStreamSynchronize(st));
  MD2_CHECK_ARG(!bad, "set_bn_stats: a variance is negative or an entry is not finite (state unchanged)");
  MD2_HIP(hipMemcpyAsync(m->bn_stats, in, sizeof(float) * (size_t)m->bn_layout.off[m->bn_layout.n],
                         hipMemcpyDeviceToDevice, st));
  return m->tm.on ? m->refold(st) : MD2_OK;
}

int model_set_testmode(Model* m, int on, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  if (!on) {
    m->tm.on = false;   // the train-mode packs and the running statistics were never touched
    return MD2_OK;
  }
  if (m->E > 0) {
    set_error("set_testmode: the MPI mode has no inference path (eval_disparity is unsupported there)");
    return MD2_ENOTSUP;
  }
  MD2_TRY(m->adam_join(st));
  MD2_TRY(m->testmode_alloc());
  MD2_TRY(m->refold(st));
  m->tm.on = true;
  m->cur_x = nullptr;      // a pending train forward is discarded, as by eval_disparity
  return MD2_OK;
}

int model_testmode(Model* m) { return m && m->tm.on ? 1 : 0; }

}  // namespace md2
