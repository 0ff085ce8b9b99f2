// Model executor entry points (model.h): create / destroy, forward, cotangents, the graph step,
// the optimiser, outputs and the profiler.  The executor itself is model_impl.h.
#include "model_impl.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace md2 {

int model_create(const ModelCfg& cfg, float* params, float* grads, Model** out) {
  MD2_CHECK_ARG(out != nullptr && params != nullptr && grads != nullptr, "model_create args");
  MD2_CHECK_ARG(cfg.arch.arch == 18 || cfg.arch.arch == 34 || cfg.arch.arch == 50, "arch 18/34/50");
  MD2_CHECK_ARG(cfg.arch.in_ch == 1 || cfg.arch.in_ch == 3, "in_channels 1 or 3");
  MD2_CHECK_ARG(cfg.N >= 1 && cfg.W % 32 == 0 && cfg.H % 32 == 0 && cfg.W >= 64 && cfg.H >= 64,
                "width/height must be multiples of 32 (>= 64)");
  // TrainCache(target_id, source_ids) over triplets (src/Monodepth.jl:49-60): any frames of 3
  MD2_CHECK_ARG(cfg.target >= 0 && cfg.target < 3 && cfg.src0 >= 0 && cfg.src0 < 3 && cfg.src1 >= 0 &&
                    cfg.src1 < 3, "target / source ids must be frames of the triplet (1-based 1:3)");
  MD2_TRY(check_scale_levels(cfg.arch));
  MD2_CHECK_ARG(cfg.arch.emb == 0 || (cfg.arch.emb > 0 && cfg.arch.emb % 2 == 1),
                "embedding_levels must be 0 or 2L+1 (x, sin, cos of L octaves)");
  if (cfg.arch.emb > 0) {
    MD2_CHECK_ARG(cfg.num_bins >= 1, "num_bins >= 1");
    if (cfg.N != 1) {
      // src/training.jl:42-56 with planes merged into the batch is shape-consistent only for one
      // sample: Project / grid_sample broadcast the N = 1 poses and frames
      set_error("MPI mode (embedding_levels > 0) trains one sample per step (batch must be 1)");
      return MD2_ENOTSUP;
    }
  }
  Model* m = new Model();
  m->cfg = cfg;
  m->params = params;
  m->grads = grads;
  int rc = m->build();
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return MD2_OK;
}

void model_destroy(Model* m) { delete m; }

// every training entry point in test mode: the activations a backward needs are not kept and the
// folded packs do not follow an update
static int refuse_testmode(const Model* m, const char* what) {
  if (!m->tm.on) return MD2_OK;
  set_error(std::string(what) + ": the model is in test mode (md2_model_set_testmode(m, 0, stream) "
            "returns to training)");
  return MD2_ESTATE;
}

// a separate network input is not wired through the MPI-mode plane replication
static int refuse_mpi_net(const Model* m, const float* x_net, const char* what) {
  if (!x_net || m->E == 0) return MD2_OK;
  set_error(std::string(what) + ": x_net is not supported in MPI mode (embedding_levels > 0)");
  return MD2_ENOTSUP;
}

int model_forward_loss_aug(Model* m, const float* x, const float* x_net, const float* automask, float* loss,
                           float* terms, hipStream_t st) {
  MD2_CHECK_ARG(m && x, "model/x");
  MD2_TRY(refuse_testmode(m, "forward_loss"));
  MD2_TRY(refuse_mpi_net(m, x_net, "forward_loss_aug"));
  if (!x_net) x_net = x;
  MD2_TRY(m->adam_join(st));   // pending per-segment updates (model_adam_segment)
  m->cur_x = x_net;            // the stem's filter gradient reads what the stem's forward read
  m->cot_ready = 1;
  return m->forward_loss(x, x_net, automask, loss, terms, st);
}

static int check_stereo_args(const Model* m, const float* x_stereo, const float* stereo_Rt, int temporal,
                             const char* what) {
  if (m->E > 0) {
    set_error(std::string(what) + ": stereo supervision is not supported in MPI mode (embedding_levels > 0)");
    return MD2_ENOTSUP;
  }
  MD2_CHECK_ARG(x_stereo && stereo_Rt, "x_stereo / stereo_Rt");
  MD2_CHECK_ARG(temporal == 0 || temporal == 1, "temporal must be 0 (S) or 1 (MS)");
  return MD2_OK;
}

int model_forward_loss_stereo(Model* m, const float* x, const float* x_net, const float* x_stereo,
                              const float* stereo_Rt, int temporal, const float* automask, float* loss,
                              float* terms, hipStream_t st) {
  MD2_CHECK_ARG(m && x, "model/x");
  MD2_TRY(refuse_testmode(m, "forward_loss_stereo"));
  MD2_TRY(check_stereo_args(m, x_stereo, stereo_Rt, temporal, "forward_loss_stereo"));
  if (!x_net) x_net = x;
  MD2_TRY(m->ensure_stereo_ws());
  MD2_TRY(m->adam_join(st));
  m->cur_x = x_net;
  m->cot_ready = 1;
  const StereoIn si{x_stereo, stereo_Rt, temporal};
  return m->forward_loss(x, x_net, automask, loss, terms, st, &si);
}

int model_forward_loss(Model* m, const float* x, const float* automask, float* loss, float* terms,
                       hipStream_t st) {
  return model_forward_loss_aug(m, x, nullptr, automask, loss, terms, st);
}

int model_forward(Model* m, const float* x, hipStream_t st) {
  MD2_CHECK_ARG(m && x, "model/x");
  MD2_TRY(m->adam_join(st));   // pending per-segment updates (model_adam_segment)
  // test mode: forward only -- nothing a backward could start from is kept
  m->cur_x = m->tm.on ? nullptr : x;
  m->cot_ready = 0;
  return m->forward(x, st);
}

int model_set_cotangents(Model* m, const float* const* d_disp, const float* d_pose, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(refuse_testmode(m, "set_cotangents"));
  if (!m->cur_x) {
    set_error("set_cotangents: no pending forward (none yet, or eval_disparity ran since)");
    return MD2_ESTATE;
  }
  MD2_TRY(m->set_cotangents(d_disp, d_pose, st));
  m->cot_ready = 1;
  return MD2_OK;
}

int model_num_segments(Model* m) { return m ? 6 : 0; }

// ---------------------------------------------------------------------------------------------
// Graph-captured train step (forward + loss + every backward segment + ADAM + weight repack as
// ONE hipGraph): the ~320 launches of a step replay without per-launch host work.  Captured on
// the executor's own stream on first use (and again when adam_m / adam_v / lr / the presence of
// the automask input or of x_net, or the gradient guard's (on, max_norm) change); each call copies x (and auto_loss, x_net) into the
// executor's input buffers, replays
// on `st`, and copies the loss out.  ADAM's step count lives on the device (adam_prep), re-set
// only when the caller's `step` is not the one the graph expects next.
static int capture_step(Model* m, bool with_auto, bool with_net, float* adam_m, float* adam_v, float lr,
                        int stereo_mode = 0) {
  auto& g = m->g;
  if (g.exec) {
    MD2_HIP(hipGraphExecDestroy(g.exec));
    g.exec = nullptr;
  }
  if (!g.st) MD2_HIP(hipStreamCreateWithFlags(&g.st, hipStreamNonBlocking));
  if (!g.x) {
    const long xn = (long)m->N * 3 * m->cfg.arch.in_ch * m->cfg.H * m->cfg.W;
    MD2_TRY(m->alloc(&g.x, xn));
    MD2_TRY(m->alloc(&g.autoloss, (long)m->N * m->cfg.H * m->cfg.W));
    MD2_TRY(m->alloc(&g.loss, 4));
    MD2_TRY(m->alloc(&g.bc, 4));
    MD2_TRY(m->alloc(&g.step, 4));
  }
  if (with_net && !g.x_net)
    MD2_TRY(m->alloc(&g.x_net, (long)m->N * 3 * m->cfg.arch.in_ch * m->cfg.H * m->cfg.W));
  const float* net = with_net ? g.x_net : g.x;
  if (stereo_mode && !g.x_stereo) {
    MD2_TRY(m->alloc(&g.x_stereo, (long)m->N * m->cfg.arch.in_ch * m->cfg.H * m->cfg.W));
    MD2_TRY(m->alloc(&g.stereo_Rt, (long)m->N * 12));
  }
  if (stereo_mode) MD2_TRY(m->ensure_stereo_ws());
  const StereoIn si{g.x_stereo, g.stereo_Rt, stereo_mode == 1 ? 1 : 0};
  MD2_HIP(hipStreamBeginCapture(g.st, hipStreamCaptureModeThreadLocal));
  auto body = [&]() -> int {
    m->cur_x = net;
    m->cot_ready = 1;
    MD2_TRY(m->forward_loss(g.x, net, with_auto ? g.autoloss : nullptr, g.loss, nullptr, g.st,
                            stereo_mode ? &si : nullptr));
    for (int k = 0; k < model_num_segments(m); ++k) MD2_TRY(model_backward_segment(m, k, nullptr, nullptr, g.st));
    // the step counter advances whether or not the guard lets the update through (md2.h)
    MD2_TRY(adam_prep(g.step, g.bc, 0.9f, 0.999f, g.st));
    if (m->gd.on) {
      MD2_TRY(grad_norm(m->grads, m->spec.total, 1.f, m->gd.max_norm, m->gd.state, m->gd.ws, g.st));
      MD2_TRY(adam_step_dev_guarded(m->params, m->grads, adam_m, adam_v, m->spec.total, lr, 0.9f, 0.999f,
                                    1e-8f, g.bc, m->gd.state, g.st));
    }
    else
      MD2_TRY(adam_step_dev(m->params, m->grads, adam_m, adam_v, m->spec.total, lr, 0.9f, 0.999f, 1e-8f,
                            g.bc, 1.f, g.st));
    return m->repack(g.st);
  };
  const int rc = body();
  hipGraph_t graph = nullptr;
  const hipError_t e = hipStreamEndCapture(g.st, &graph);
  if (rc) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  MD2_HIP(e);
  const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  MD2_HIP(ei);
  g.adam_m = adam_m;
  g.adam_v = adam_v;
  g.lr = lr;
  g.with_auto = with_auto ? 1 : 0;
  g.with_net = with_net ? 1 : 0;
  g.stereo_mode = stereo_mode;
  g.intrinsics = m->intr_on ? 1 : 0;
  g.guard_on = m->gd.on ? 1 : 0;
  g.guard_max = m->gd.max_norm;
  g.next_step = -1;
  return MD2_OK;
}

// stereo_mode 0: x_stereo / stereo_Rt are not read (train_step_graph, _aug); 1 MS, 2 S
static int train_step_graph_impl(Model* m, const float* x, const float* x_net, const float* x_stereo,
                                 const float* stereo_Rt, int stereo_mode, const float* auto_loss, float* adam_m,
                                 float* adam_v, float lr, int step, float* loss, hipStream_t st) {
  MD2_CHECK_ARG(m && x && adam_m && adam_v && loss && step >= 1, "train_step_graph args");
  MD2_TRY(refuse_testmode(m, "train_step_graph"));
  MD2_TRY(refuse_mpi_net(m, x_net, "train_step_graph_aug"));
  if (x_net == x) x_net = nullptr;   // the plain step: one input buffer, the plain capture
  auto& g = m->g;
  const bool with_auto = auto_loss != nullptr;
  const bool with_net = x_net != nullptr;
  if (m->pf.on) {   // per-launch HIP events cannot live in a replayed graph: eager step
    if (stereo_mode)
      MD2_TRY(model_forward_loss_stereo(m, x, x_net, x_stereo, stereo_Rt, stereo_mode == 1, auto_loss, loss,
                                        nullptr, st));
    else
    MD2_TRY(model_forward_loss_aug(m, x, x_net, auto_loss, loss, nullptr, st));
    for (int k = 0; k < model_num_segments(m); ++k) MD2_TRY(model_backward_segment(m, k, nullptr, nullptr, st));
    return model_adam(m, adam_m, adam_v, lr, 0.9f, 0.999f, 1e-8f, step, 1.f, st);
  }
  // the replay reads and writes params, adam_m / adam_v and the packed weights: order it after
  // pending per-segment updates (outside the capture: the event lives outside the graph)
  MD2_TRY(m->adam_join(st));
  if (!g.exec || g.adam_m != adam_m || g.adam_v != adam_v || g.lr != lr || g.with_auto != (int)with_auto ||
      g.with_net != (int)with_net || g.stereo_mode != stereo_mode || g.intrinsics != (int)m->intr_on ||
      g.guard_on != (int)m->gd.on ||
      (m->gd.on && g.guard_max != m->gd.max_norm))
    MD2_TRY(capture_step(m, with_auto, with_net, adam_m, adam_v, lr, stereo_mode));
  const size_t xb = sizeof(float) * (size_t)m->N * 3 * m->cfg.arch.in_ch * m->cfg.H * m->cfg.W;
  if (x != g.x) MD2_HIP(hipMemcpyAsync(g.x, x, xb, hipMemcpyDeviceToDevice, st));
  if (with_net && x_net != g.x_net) MD2_HIP(hipMemcpyAsync(g.x_net, x_net, xb, hipMemcpyDeviceToDevice, st));
  if (stereo_mode) {
    MD2_HIP(hipMemcpyAsync(g.x_stereo, x_stereo, xb / 3, hipMemcpyDeviceToDevice, st));
    MD2_HIP(hipMemcpyAsync(g.stereo_Rt, stereo_Rt, sizeof(float) * (size_t)m->N * 12, hipMemcpyDeviceToDevice, st));
  }
  if (with_auto)
    MD2_HIP(hipMemcpyAsync(g.autoloss, auto_loss, sizeof(float) * (size_t)m->N * m->cfg.H * m->cfg.W,
                           hipMemcpyDeviceToDevice, st));
  if (step != g.next_step) MD2_TRY(set_device_int(g.step, step - 1, st));
  MD2_HIP(hipGraphLaunch(g.exec, st));
  MD2_HIP(hipMemcpyAsync(loss, g.loss, sizeof(float), hipMemcpyDeviceToDevice, st));
  m->cur_x = with_net ? g.x_net : g.x;
  m->cot_ready = 1;
  g.next_step = step + 1;
  return MD2_OK;
}

int model_train_step_graph_aug(Model* m, const float* x, const float* x_net, const float* auto_loss,
                               float* adam_m, float* adam_v, float lr, int step, float* loss, hipStream_t st) {
  return train_step_graph_impl(m, x, x_net, nullptr, nullptr, 0, auto_loss, adam_m, adam_v, lr, step, loss, st);
}

int model_train_step_graph_stereo(Model* m, const float* x, const float* x_net, const float* x_stereo,
                                  const float* stereo_Rt, int temporal, const float* auto_loss, float* adam_m,
                                  float* adam_v, float lr, int step, float* loss, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(check_stereo_args(m, x_stereo, stereo_Rt, temporal, "train_step_graph_stereo"));
  return train_step_graph_impl(m, x, x_net, x_stereo, stereo_Rt, temporal ? 1 : 2, auto_loss, adam_m, adam_v, lr,
                               step, loss, st);
}

int model_train_step_graph(Model* m, const float* x, const float* auto_loss, float* adam_m,
                           float* adam_v, float lr, int step, float* loss, hipStream_t st) {
  return model_train_step_graph_aug(m, x, nullptr, auto_loss, adam_m, adam_v, lr, step, loss, st);
}

int model_backward_segment(Model* m, int k, long* off, long* len, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(refuse_testmode(m, "backward_segment"));
  if (!m->cur_x) {
    set_error("backward_segment: no pending forward_loss (none yet, or eval_disparity ran since)");
    return MD2_ESTATE;
  }
  if (!m->cot_ready) {
    set_error("backward_segment: forward-only call without cotangents (md2_model_set_cotangents)");
    return MD2_ESTATE;
  }
  MD2_CHECK_ARG(k >= 0 && k < 6, "segment index");
  long b = 0, e = 0;
  switch (k) {
    case 0: MD2_TRY(m->seg_decoder(st)); break;
    case 1: MD2_TRY(m->seg_stage(3, st)); break;
    case 2: MD2_TRY(m->seg_stage(2, st)); break;
    case 3: MD2_TRY(m->seg_stage(1, st)); break;
    case 4: MD2_TRY(m->seg_stage(0, st)); break;
    default: MD2_TRY(m->seg_stem(st)); break;
  }
  m->segment_range(k, b, e);
  if (off) *off = b;
  if (len) *len = e - b;
  return MD2_OK;
}

// ---- optimiser
// ADAM over segment k's parameters + the re-pack of its conv weights on `upd`, ordered after
// everything enqueued on st so far (its backward segment, and a DP caller's all-reduce of the
// bucket when st waits on it)
int Model::adam_segment(int k, float* am, float* av, float lr, float b1, float b2, float eps, float bc1,
                        float bc2, float gscale, hipStream_t st) {
  long b0, e0;
  segment_range(k, b0, e0);
  MD2_TRY(stream_wait(st, ov.upd, ov.seg_ev));
  MD2_TRY(adam_step(params + b0, grads + b0, am + b0, av + b0, e0 - b0, lr, b1, b2, eps, bc1, bc2,
                    gscale, ov.upd));
  const PackTable& t = seg_pack[k];
  if (t.njobs) MD2_TRY(conv_pack_batch(t.jobs, t.njobs, t.blocks, ov.upd));
  MD2_HIP(hipEventRecord(ov.upd_ev, ov.upd));
  ov.upd_recorded = true;
  return MD2_OK;
}

// st waits for every update enqueued by adam_segment.  The ordering is per stream, so once an
// update was ever recorded EVERY join waits (an entry point on another stream -- a Python
// executor sharing the parameters, a user stream for eval or get_params -- must see it too);
// waiting on a completed event costs next to nothing.
int Model::adam_join(hipStream_t st) {
  if (ov.upd_recorded) MD2_HIP(hipStreamWaitEvent(st, ov.upd_ev, 0));
  return MD2_OK;
}

int model_adam(Model* m, float* adam_m, float* adam_v, float lr, float b1, float b2, float eps,
               int step, float grad_scale, hipStream_t st) {
  MD2_CHECK_ARG(m && adam_m && adam_v && step >= 1, "adam args");
  MD2_TRY(refuse_testmode(m, "adam"));
  MD2_TRY(m->adam_join(st));   // pending per-segment updates (model_adam_segment)
  const double bc1 = 1.0 - std::pow((double)b1, step), bc2 = 1.0 - std::pow((double)b2, step);
  if (m->gd.on) {
    MD2_CHECK_ARG(std::isfinite(grad_scale) && grad_scale > 0.f, "guarded adam: grad_scale must be finite and positive");
    MD2_TRY(grad_norm(m->grads, m->spec.total, grad_scale, m->gd.max_norm, m->gd.state, m->gd.ws, st));
    MD2_TRY(adam_step_guarded(m->params, m->grads, adam_m, adam_v, m->spec.total, lr, b1, b2, eps, (float)bc1,
                              (float)bc2, m->gd.state, st));
  }
  else
    MD2_TRY(adam_step(m->params, m->grads, adam_m, adam_v, m->spec.total, lr, b1, b2, eps, (float)bc1,
                      (float)bc2, grad_scale, st));
  return m->repack(st);
}

// ---- gradient guard
int model_set_grad_guard(Model* m, int on, float max_norm) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(refuse_testmode(m, "set_grad_guard"));
  if (m->E > 0) {
    set_error("set_grad_guard: not available in MPI mode (embedding_levels > 0)");
    return MD2_ENOTSUP;
  }
  if (on) {
    MD2_CHECK_ARG(max_norm > 0.f, "set_grad_guard: max_norm must be positive (+inf: no clipping)");   // false for NaN
    MD2_CHECK_ARG(m->spec.total >= 1 && m->spec.total <= (1LL << 31), "set_grad_guard: parameter count");
    if (!m->gd.state) {
      MD2_TRY(m->alloc(&m->gd.state, 1));
      MD2_TRY(m->alloc_bytes(&m->gd.ws, 1, grad_norm_workspace_bytes(m->spec.total), true));
    }
  }
  if (m->gd.state) {
    // `skipped` starts again; the device is idle around the write, so no stream can be mid-step
    MD2_HIP(hipDeviceSynchronize());
    MD2_HIP(hipMemset(m->gd.state, 0, sizeof(md2_guard_state)));
    MD2_HIP(hipDeviceSynchronize());
  }
  m->gd.on = on != 0;
  if (on) m->gd.max_norm = max_norm;
  return MD2_OK;
}

bool model_grad_guard_on(const Model* m) { return m && m->gd.on; }

int model_grad_guard_state(Model* m, const md2_guard_state** dev) {
  MD2_CHECK_ARG(m && dev, "grad_guard_state args");
  if (!m->gd.state) {
    set_error("grad_guard_state: the guard was never switched on (md2_model_set_grad_guard)");
    return MD2_ESTATE;
  }
  *dev = m->gd.state;
  return MD2_OK;
}

int model_adam_segment(Model* m, int k, float* adam_m, float* adam_v, float lr, float b1, float b2,
                       float eps, int step, float grad_scale, hipStream_t st) {
  MD2_CHECK_ARG(m && adam_m && adam_v && step >= 1, "adam_segment args");
  MD2_CHECK_ARG(k >= 0 && k < 6, "segment index");
  MD2_TRY(refuse_testmode(m, "adam_segment"));
  if (m->gd.on) {
    set_error("adam_segment: the gradient guard is on -- a segment's update cannot know the global norm "
              "(md2_model_adam takes the whole step)");
    return MD2_ENOTSUP;
  }
  const double bc1 = 1.0 - std::pow((double)b1, step), bc2 = 1.0 - std::pow((double)b2, step);
  return m->adam_segment(k, adam_m, adam_v, lr, b1, b2, eps, (float)bc1, (float)bc2, grad_scale, st);
}

int model_adam_join(Model* m, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  return m->adam_join(st);
}

bool model_segment_update_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("MD2_SEG_UPDATE");
    return e && e[0] == '1';
  }();
  return on;
}

int model_repack(Model* m, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(m->adam_join(st));   // pending per-segment updates write the same packed weights
  MD2_TRY(m->repack(st));
  return m->tm.on ? m->refold(st) : MD2_OK;
}

int model_debug_tensor(Model* m, int index, const char** name, const void** ptr, int* dims) {
  MD2_CHECK_ARG(m && ptr && dims, "debug_tensor arguments");
  struct T {
    std::string name;
    const void* p;
    int n, c, h, w, u8;
  };
  const int B = m->B, N = m->N;
  std::vector<T> ts;
  ts.push_back({"stem.y", m->y0, B, 64, m->H0, m->W0, 0});
  ts.push_back({"stem.out", m->f0, B, 64, m->H0, m->W0, 0});
  ts.push_back({"maxpool.out", m->mp, B, 64, m->Hm, m->Wm, 0});
  ts.push_back({"maxpool.arg", m->mp_arg, B, 64, m->Hm, m->Wm, 1});
  for (size_t si = 0; si < m->stages.size(); ++si)
    for (size_t bi = 0; bi < m->stages[si].size(); ++bi) {
      auto& b = m->stages[si][bi];
      const std::string pre = "layer" + std::to_string(si + 1) + "." + std::to_string(bi);
      for (size_t k = 0; k < b.st.size(); ++k) {
        auto& e = b.st[k];
        const bool last = k + 1 == b.st.size();
        ts.push_back({pre + ".conv" + std::to_string(k + 1) + ".y", e.y, B, e.conv.p.cout,
                      e.conv.s.Ho, e.conv.s.Wo, 0});
        ts.push_back({pre + (last ? std::string(".out") : ".relu" + std::to_string(k + 1)), e.a, B,
                      e.conv.p.cout, e.conv.s.Ho, e.conv.s.Wo, 0});
      }
      if (b.down) ts.push_back({pre + ".down.y", b.yd, B, b.C, b.H, b.W, 0});
      ts.push_back({pre + ".d_out", b.d_out, B, b.C, b.H, b.W, 0});
    }
  const int h4 = m->featH[4], w4 = m->featW[4];
  ts.push_back({"pose.sq", m->sqo, B, 256, h4, w4, 0});
  ts.push_back({"pose.conv1", m->pc1, 2 * N, 256, h4, w4, 0});
  ts.push_back({"pose.conv2", m->pc2, 2 * N, 256, h4, w4, 0});
  for (int f = 0; f < 4; ++f)
    if (m->d_skip[f])
      ts.push_back({"d_skip" + std::to_string(f), m->d_skip[f], N, m->featC[f], m->featH[f],
                    m->featW[f], 0});
  // DepthDecoder intermediates of the last forward (forward-accuracy bisection, tools/forward_bisect.py)
  for (auto& d : m->br) {
    const std::string pre = "depth.branch" + std::to_string(d.b.bid);
    ts.push_back({pre + ".c1", d.o1, m->ND, d.b.cout, d.h, d.w, 0});
    ts.push_back({pre + ".up", d.up, m->ND, d.b.cout, 2 * d.h, 2 * d.w, 0});
    ts.push_back({pre + ".c2", d.o2, m->ND, d.b.cout, 2 * d.h, 2 * d.w, 0});
  }
  ts.push_back({"d_mp", m->d_mp, B, 64, m->Hm, m->Wm, 0});
  ts.push_back({"d_f0", m->d_f0, B, 64, m->H0, m->W0, 0});
  if (index < 0 || index >= (int)ts.size()) {
    set_error("debug_tensor: index out of range");
    return MD2_EINVAL;
  }
  m->dbg_name = ts[index].name;
  if (name) *name = m->dbg_name.c_str();
  *ptr = ts[index].p;
  dims[0] = ts[index].n;
  dims[1] = ts[index].c;
  dims[2] = ts[index].h;
  dims[3] = ts[index].w;
  dims[4] = ts[index].u8;
  return MD2_OK;
}

int model_outputs(Model* m, const float** disp, int* dw, int* dh, const float** pose) {
  MD2_CHECK_ARG(m, "model");
  for (size_t li = 0; li < m->heads.size(); ++li) {
    const DecBranch& d = *m->heads[li];
    if (disp) disp[li] = d.disp;
    if (dw) dw[li] = 2 * d.w;
    if (dh) dh[li] = 2 * d.h;
  }
  if (pose) *pose = m->pose;
  return MD2_OK;
}

int model_features(Model* m, const float** feat, int* c, int* h, int* w) {
  MD2_CHECK_ARG(m, "model");
  for (int k = 0; k < 5; ++k) {
    feat[k] = m->feat[k];
    c[k] = m->featC[k];
    h[k] = m->featH[k];
    w[k] = m->featW[k];
  }
  return MD2_OK;
}

int model_eval_disparity(Model* m, const float* x, int n, float** disp_out, hipStream_t st) {
  MD2_CHECK_ARG(m && x && n >= 1 && n <= m->N, "eval_disparity: 1 <= n <= batch");
  MD2_TRY(m->adam_join(st));   // pending per-segment updates (model_adam_segment)
  if (m->E > 0) {
    // src/model.jl:63 runs the decoder on the bare encoder features, which an
    // embedding_levels > 0 DepthDecoder cannot take (defect D4)
    set_error("eval_disparity: the MPI-mode DepthDecoder (embedding_levels > 0) has no mono input");
    return MD2_ENOTSUP;
  }
  // inference reuses the executor's activation buffers: a pending train forward is gone, and a
  // backward after this must fail instead of differentiating the eval batch
  m->cur_x = nullptr;
  TensorIn in = Model::tin(x, m->cfg.arch.in_ch, (long)m->cfg.H * m->cfg.W);
  MD2_TRY(m->encoder(in, n, st));
  MD2_TRY(m->decoder_fwd(n, 0, st));
  if (disp_out)
    for (size_t li = 0; li < m->heads.size(); ++li) disp_out[li] = m->heads[li]->disp;
  return MD2_OK;
}

int model_eval_pose(Model* m, const float* x, int n, const float** pose_out, hipStream_t st) {
  MD2_CHECK_ARG(m && x, "eval_pose: model/x");
  MD2_CHECK_ARG(n >= 2 && n - 1 <= 2 * m->N, "eval_pose: 2 <= n <= 2 * batch + 1");
  MD2_TRY(m->adam_join(st));   // pending per-segment updates (model_adam_segment)
  if (m->E > 0) {
    set_error("eval_pose: not available in MPI mode (embedding_levels > 0)");
    return MD2_ENOTSUP;
  }
  // as eval_disparity: the executor's activation buffers are reused, a pending train forward is gone
  m->cur_x = nullptr;
  MD2_TRY(m->eval_pose(Model::tin(x, m->cfg.arch.in_ch, (long)m->cfg.H * m->cfg.W), n, st));
  if (pose_out) *pose_out = m->pose;
  return MD2_OK;
}

// Flux-layout flat vectors (src/model.jl @functor order, conv weights as true convolutions) <->
// the library's flat vectors: a copy with every conv weight's taps reversed (md2_model_*_params)
static int flux_flip_copy(const Model* m, const float* src, float* dst, hipStream_t st) {
  MD2_CHECK_ARG(src && dst && src != dst, "params: distinct source and destination required");
  MD2_HIP(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)m->spec.total, hipMemcpyDeviceToDevice, st));
  for (const ParamEntry& e : m->spec.table)
    if (e.ndim == 4 && e.shape[2] * e.shape[3] > 1)
      MD2_TRY(flip_taps(src + e.offset, dst + e.offset, (long)e.shape[0] * e.shape[1], e.shape[2],
                        e.shape[3], st));
  return MD2_OK;
}

int model_set_params_flux(Model* m, const float* flux, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(m->adam_join(st));   // pending per-segment updates (model_adam_segment)
  MD2_TRY(flux_flip_copy(m, flux, m->params, st));
  MD2_TRY(m->repack(st));
  return m->tm.on ? m->refold(st) : MD2_OK;
}

int model_get_params_flux(Model* m, float* flux, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(m->adam_join(st));   // pending per-segment updates (model_adam_segment)
  return flux_flip_copy(m, m->params, flux, st);
}

int model_get_grads_flux(Model* m, float* flux, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(m->adam_join(st));   // a DP per-segment update is ordered after its bucket's all-reduce
  return flux_flip_copy(m, m->grads, flux, st);
}

// train_loss pullback with an upstream cotangent: the fused loss tail formed d loss / d (disp,
// pose) for dloss = 1 during the forward; scale them before backward segment 0
int model_scale_loss_cotangent(Model* m, float dloss, hipStream_t st) {
  MD2_CHECK_ARG(m, "model");
  MD2_TRY(refuse_testmode(m, "loss_cotangent"));
  MD2_CHECK_ARG(m->cur_x && m->cot_ready, "loss cotangent before forward_loss");
  if (dloss == 1.f) return MD2_OK;
  for (DecBranch* d : m->heads) MD2_TRY(scale_inplace(d->d_head, (long)m->ND * 4 * d->h * d->w, dloss, st));
  return scale_inplace(m->d_pose, 2L * m->N * 6, dloss, st);
}

int model_set_bins(Model* m, const float* bins, hipStream_t st) {
  MD2_CHECK_ARG(m && bins, "set_bins args");
  if (m->E == 0) {
    set_error("set_bins: the model is not in MPI mode (embedding_levels = 0)");
    return MD2_ESTATE;
  }
  MD2_HIP(hipMemcpyAsync(m->bins, bins, sizeof(float) * m->N * m->NP, hipMemcpyDefault, st));
  return MD2_OK;
}

int model_set_intrinsics(Model* m, const float* K, const float* invK, hipStream_t st) {
  MD2_CHECK_ARG((K == nullptr) == (invK == nullptr), "set_intrinsics: K and invK come together (both null clears)");
  MD2_CHECK_ARG(m, "model");
  if (!K) {
    m->intr_on = false;
    return MD2_OK;
  }
  if (m->E > 0) {
    set_error("set_intrinsics: per-sample intrinsics are not supported in MPI mode (embedding_levels > 0)");
    return MD2_ENOTSUP;
  }
  if (!m->Kn) {
    MD2_TRY(m->alloc(&m->Kn, (size_t)m->N * 9));
    MD2_TRY(m->alloc(&m->invKn, (size_t)m->N * 9));
  }
  MD2_TRY(m->ensure_stereo_ws());   // the sources form's workspace and the automask buffer
  const size_t b = sizeof(float) * (size_t)m->N * 9;
  MD2_HIP(hipMemcpyAsync(m->Kn, K, b, hipMemcpyDeviceToDevice, st));
  MD2_HIP(hipMemcpyAsync(m->invKn, invK, b, hipMemcpyDeviceToDevice, st));
  m->intr_on = true;
  return MD2_OK;
}

long model_param_count(Model* m) { return m ? m->spec.total : 0; }
float* model_grads(Model* m) { return m ? m->grads : nullptr; }
size_t model_device_bytes(Model* m) { return m ? m->bytes : 0; }

// ---- HIP-event profiler
hipEvent_t Profiler::ev() {
  if (evi == evpool.size()) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    evpool.push_back(e);
  }
  return evpool[evi++];
}

hipEvent_t Profiler::begin(hipStream_t st) {
  if (!on) return nullptr;
  hipEvent_t e = ev();
  (void)hipEventRecord(e, st);
  return e;
}

void Profiler::end(hipEvent_t a, int cat, double work, hipStream_t st, const char* pass, const ConvShape* s) {
  if (!on) return;
  hipEvent_t b = ev();
  (void)hipEventRecord(b, st);
  Rec r{a, b, cat, work, {0}};
  if (pass && s) {
    const int ar = conv_last_arith();
    snprintf(r.tag, sizeof(r.tag), "%s %dx%d/%d%s %d->%d %dx%d n%d [%s]", pass, s->KH, s->KW, s->stride,
             s->reflect ? "r" : "", s->Cin, s->Cout, s->H, s->W, s->N,
             ar == 6 ? "bf16x6" : ar == 1 ? "fp32" : "valu");
  }
  else if (pass)
    snprintf(r.tag, sizeof(r.tag), "%s", pass);
  recs.push_back(r);
}

void Profiler::reset() {
  recs.clear();
  evi = 0;
}

Profiler::~Profiler() {
  for (hipEvent_t e : evpool) (void)hipEventDestroy(e);
}

int Profiler::records(int max, double* ms, double* work, int* cat, char* tags, int tag_len, int* count) {
  int k = 0;
  for (auto& r : recs) {
    if (k >= max) break;
    MD2_HIP(hipEventSynchronize(r.b));
    float t = 0.f;
    MD2_HIP(hipEventElapsedTime(&t, r.a, r.b));
    ms[k] = t;
    work[k] = r.work;
    cat[k] = r.cat;
    if (tags && tag_len > 0) {
      strncpy(tags + (long)k * tag_len, r.tag, tag_len - 1);
      tags[(long)k * tag_len + tag_len - 1] = 0;
    }
    ++k;
  }
  *count = k;
  reset();
  return MD2_OK;
}

int Profiler::read(double* out, int ncat) {
  for (int c = 0; c < ncat * 3; ++c) out[c] = 0.0;
  for (auto& r : recs) {
    MD2_HIP(hipEventSynchronize(r.b));
    float ms = 0.f;
    MD2_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    if (r.cat < ncat) {
      out[r.cat * 3 + 0] += ms;
      out[r.cat * 3 + 1] += r.work;
      out[r.cat * 3 + 2] += 1.0;
    }
  }
  reset();
  return MD2_OK;
}

int model_set_profiling(Model* m, int on) {
  MD2_CHECK_ARG(m, "model");
  m->pf.on = on != 0;
  m->pf.reset();
  return MD2_OK;
}

int model_profile_records(Model* m, int max, double* ms, double* work, int* cat, char* tags,
                          int tag_len, int* count) {
  MD2_CHECK_ARG(m && ms && work && cat && count && max >= 0, "profile_records args");
  return m->pf.records(max, ms, work, cat, tags, tag_len, count);
}

int model_profile_read(Model* m, double* out, int ncat) {
  MD2_CHECK_ARG(m && out && ncat > 0, "profile_read args");
  return m->pf.read(out, ncat);
}

}  // namespace md2
