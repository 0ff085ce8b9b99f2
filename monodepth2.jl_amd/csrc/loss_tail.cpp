// Loss-tail orchestration (src/training.jl:21-78 after the model call).
#include "loss_tail.h"

#include <cstring>

namespace md2 {

namespace {
inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

struct TailLayout {
  size_t Rt, dRt, Rtl, dRtl, g_full[MAX_SCALES], mean, photo[MAX_SCALES], smooth[MAX_SCALES],
      tsum[MAX_SCALES], terms, total;
};

TailLayout layout(const LossTailCfg& c, int S) {
  TailLayout L{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += align256(bytes);
    return o;
  };
  L.Rt = take(sizeof(float) * S * c.N * 12);
  L.dRt = take(sizeof(float) * S * c.N * 12);
  L.Rtl = take(sizeof(float) * S * c.N * 12);    // learned sources only, in pose-block order
  L.dRtl = take(sizeof(float) * S * c.N * 12);
  L.mean = take(sizeof(double) * (size_t)c.nscales * c.N * MEAN_PARTS);
  for (int s = 0; s < c.nscales; ++s) {
    L.g_full[s] = take(sizeof(float) * (size_t)c.N * c.W * c.H);
    L.photo[s] = take(sizeof(float) * (1 + 12 * S) * photometric_blocks(c.W, c.H, c.N, c.nscales));
    L.smooth[s] = take(sizeof(float) * 2 * smooth_blocks(c.W, c.H, c.N));
    L.tsum[s] = take(sizeof(double) * smooth_blocks(c.W, c.H, c.N));
  }
  L.terms = take(sizeof(float) * 2 * MAX_SCALES);
  L.total = off;
  return L;
}

inline float ratio(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

Geom make_geom(const float* K, const float* invK, float min_depth, float max_depth, int W, int H) {
  Geom g;
  std::memcpy(g.K, K, sizeof(g.K));
  std::memcpy(g.invK, invK, sizeof(g.invK));
  g.min_disp = (float)(1.0 / max_depth);
  g.disp_range = (float)(1.0 / min_depth - 1.0 / max_depth);
  g.W = W;
  g.H = H;
  g.wm1 = (float)(W - 1);
  g.hm1 = (float)(H - 1);
  return g;
}

// A one-row disparity map is upsampled like any other; a one-column map is not supported: the
// photometric pass reads the two column taps of the upsample as one 8-byte pair.  Checked before
// anything is launched.
int check_scale_dims(const LossTailCfg& c) {
  for (int s = 0; s < c.nscales; ++s)
    MD2_CHECK_ARG(c.dw[s] >= 2 && c.dh[s] >= 1 && c.dw[s] <= c.W && c.dh[s] <= c.H,
                  "scale dims: a disparity map must be 2..width columns by 1..height rows");
  return MD2_OK;
}

// The loss tail over S sources.  x != nullptr: the sources and the target are frames c.src0 /
// c.src1 / c.target of x, and the photometric pass is the packed two-source kernel (photo.hip);
// otherwise it is the kernel over sources (photo_sources.hip).  Kn / invKn (device [N][9] each, both
// or neither, sources form only): per-sample intrinsics, c.K / c.invK are then not read by any
// kernel.  Everything else is one sequence.
int run(const LossTailCfg& c, int S, const LossSource* src, const float* target,
        long target_sample_stride, const float* x, const float* Kn, const float* invKn,
        const float* const* disp, const float* pose,
        const float* automask, float dloss, const LossTailOut& o, void* workspace, hipStream_t st) {
  MD2_CHECK_ARG(S >= 1 && S <= MAX_SOURCES, "nsrc must be 1, 2 or 3");
  MD2_CHECK_ARG(src != nullptr, "sources: null pointer");
  MD2_CHECK_ARG(c.N > 0 && c.W > 2 && c.H > 2, "loss tail dims");
  MD2_CHECK_ARG(c.nscales >= 1 && c.nscales <= MAX_SCALES, "nscales");
  MD2_CHECK_ARG(c.C == 1 || c.C == 3, "channels must be 1 or 3");
  MD2_CHECK_ARG(workspace != nullptr && disp != nullptr && target != nullptr, "null pointer");
  MD2_CHECK_ARG((Kn == nullptr) == (invKn == nullptr) && !(x && Kn),
                "per-sample intrinsics: K and invK come together, on the sources form");
  // the learned sources' blocks of `pose` are 0..n_learned-1, each once
  int n_learned = 0, seen = 0, invert_mask = 0;
  bool in_place = true;     // every learned source s has pose block s: composeT writes Rt itself
  for (int s = 0; s < S; ++s) {
    MD2_CHECK_ARG(src[s].frames != nullptr, "source without frames");
    if (src[s].pose_block >= 0) {
      MD2_CHECK_ARG(pose != nullptr, "a learned source needs pose");
      MD2_CHECK_ARG(src[s].pose_block < S && !((seen >> src[s].pose_block) & 1),
                    "pose_block must be distinct and below the number of learned sources");
      seen |= 1 << src[s].pose_block;
      if (src[s].invert) invert_mask |= 1 << src[s].pose_block;
      in_place &= src[s].pose_block == s;
      ++n_learned;
    } else {
      MD2_CHECK_ARG(src[s].pose_block == -1, "pose_block must be >= 0 (learned) or -1 (fixed)");
      MD2_CHECK_ARG(src[s].Rt != nullptr, "a fixed source needs Rt");
    }
  }
  MD2_CHECK_ARG(seen == (1 << n_learned) - 1,
                "pose_block must be distinct and below the number of learned sources");
  MD2_TRY(check_scale_dims(c));

  float* d_pose = n_learned > 0 ? o.d_pose : nullptr;
  const TailLayout L = layout(c, S);
  char* ws = (char*)workspace;
  float* Rt = (float*)(ws + L.Rt);
  float* dRt = (float*)(ws + L.dRt);
  // learned rows in pose-block order: Rt / dRt themselves where that is the sources' order
  float* Rtl = in_place ? Rt : (float*)(ws + L.Rtl);
  float* dRtl = in_place ? dRt : (float*)(ws + L.dRtl);
  double* mean = (double*)(ws + L.mean);
  const Geom g = make_geom(c.K, c.invK, c.min_depth, c.max_depth, c.W, c.H);

  // Rt [S][N][12]: learned rows from composeT, fixed rows from the caller
  const size_t rt_bytes = sizeof(float) * c.N * 12;
  if (n_learned > 0) MD2_TRY(launch_so3_fwd(pose, n_learned * c.N, c.N, invert_mask, Rtl, st));
  for (int s = 0; s < S; ++s) {
    if (in_place && src[s].pose_block >= 0) continue;
    const float* from = src[s].pose_block >= 0 ? Rtl + (size_t)src[s].pose_block * c.N * 12 : src[s].Rt;
    MD2_HIP(hipMemcpyAsync(Rt + (size_t)s * c.N * 12, from, rt_bytes, hipMemcpyDeviceToDevice, st));
  }

  const float up = dloss / c.divisor;
  const long photo_blk = photometric_blocks(c.W, c.H, c.N, c.nscales);
  const long smooth_blk = smooth_blocks(c.W, c.H, c.N);
  FinalizeArgs fa{};
  fa.nscales = c.nscales;
  fa.N = c.N;
  fa.nsrc = S;
  fa.photo_scale = 1.f / ((float)c.N * c.W * c.H);
  fa.terms = o.terms ? o.terms : (float*)(ws + L.terms);
  fa.divisor = c.divisor;

  PhotoSrcArgs pa{};
  pa.nscales = c.nscales;
  pa.nsrc = S;
  pa.target = target;
  pa.target_sample_stride = target_sample_stride;
  for (int s = 0; s < S; ++s) {
    pa.src[s] = src[s].frames;
    pa.src_sample_stride[s] = src[s].sample_stride;
  }
  pa.Rt = Rt;
  pa.automask = automask;
  pa.wloss = up / ((float)c.N * c.W * c.H);
  pa.N = c.N;
  pa.Kn = Kn;
  pa.invKn = invKn;
  const size_t plane = (size_t)c.N * c.W * c.H;
  DispSumBatch db{};
  db.W = c.W;
  db.H = c.H;
  db.N = c.N;
  db.parts = MEAN_PARTS;
  for (int s = 0; s < c.nscales; ++s) {
    PhotoScale& ps = pa.sc[s];
    ps.disp = disp[s];
    ps.dw = c.dw[s];
    ps.dh = c.dh[s];
    ps.rx = ratio(c.dw[s], c.W);
    ps.ry = ratio(c.dh[s], c.H);
    ps.g_disp = (float*)(ws + L.g_full[s]);
    ps.partials = (float*)(ws + L.photo[s]);
    ps.loss_map = o.vis_loss ? o.vis_loss + s * plane : nullptr;
    ps.sel_map = o.vis_sel ? o.vis_sel + s * plane : nullptr;
    ps.cell_map = o.vis_cell ? o.vis_cell + (size_t)S * s * plane : nullptr;
    db.s[s] = DispSumArgs{disp[s], c.dw[s], c.dh[s], ps.rx, ps.ry, mean + (size_t)s * c.N * MEAN_PARTS};
  }
  MD2_TRY(launch_disp_sum(db, c.nscales, st));   // every scale's mean in one launch
  // all scales' warp + SSIM + L1 forward and pullback in one launch
  if (o.photo_events) MD2_HIP(hipEventRecord(o.photo_events[0], st));
  if (x) {
    PhotoArgs px{};
    std::memcpy(px.sc, pa.sc, sizeof(px.sc));
    px.nscales = c.nscales;
    px.x = x;
    px.x_sample_stride = c.x_sample_stride;
    px.x_frame_stride = c.x_frame_stride;
    px.target = c.target;
    px.src0 = c.src0;
    px.src1 = c.src1;
    px.Rt = Rt;
    px.automask = automask;
    px.wloss = pa.wloss;
    px.N = c.N;
    MD2_TRY(launch_photometric(px, g, c.C, st));
  } else {
    MD2_TRY(launch_photometric_sources(pa, g, c.C, st));
  }
  if (o.photo_events) MD2_HIP(hipEventRecord(o.photo_events[1], st));
  if (o.vis_warped) MD2_TRY(launch_warp_vis(pa, c.nscales - 1, g, c.C, o.vis_warped, st));

  // smoothness and the upsample adjoint: every scale in one launch each (scale = grid z)
  SmoothArgs sas[MAX_SCALES];
  UpAdjArgs uas[MAX_SCALES];
  int nua = 0;
  for (int s = 0; s < c.nscales; ++s) {
    const PhotoScale& ps = pa.sc[s];
    double* mp = mean + (size_t)s * c.N * MEAN_PARTS;
    float* sp = (float*)(ws + L.smooth[s]);
    double* tp = (double*)(ws + L.tsum[s]);
    SmoothArgs& sa = sas[s];
    sa = SmoothArgs{};
    sa.disp = disp[s];
    sa.dw = c.dw[s];
    sa.dh = c.dh[s];
    sa.rx = ps.rx;
    sa.ry = ps.ry;
    sa.img = target;
    sa.img_sample_stride = target_sample_stride;
    sa.mean_partials = c.smooth_normalize ? mp : nullptr;
    sa.mean_parts = c.smooth_normalize ? MEAN_PARTS : 0;
    sa.ws = up * c.smooth_w[s];
    sa.g_disp = ps.g_disp;
    sa.partials = sp;
    sa.tsum = c.smooth_normalize ? tp : nullptr;
    sa.N = c.N;
    sa.W = c.W;
    sa.H = c.H;

    UpAdjArgs ua{};
    ua.g_full = ps.g_disp;
    ua.disp = disp[s];
    ua.dw = c.dw[s];
    ua.dh = c.dh[s];
    ua.rx = ps.rx;
    ua.ry = ps.ry;
    ua.mean_partials = mp;
    ua.mean_parts = MEAN_PARTS;
    ua.smooth_tsum = c.smooth_normalize ? tp : nullptr;
    ua.smooth_parts = (int)(smooth_blk / c.N);
    ua.ws = sa.ws;
    ua.sigmoid = c.sigmoid_grad;
    ua.accumulate = 0;
    ua.out = o.d_disp[s];
    ua.N = c.N;
    ua.W = c.W;
    ua.H = c.H;
    if (o.d_disp[s]) uas[nua++] = ua;

    fa.photo_partials[s] = ps.partials;
    fa.photo_blocks[s] = photo_blk;
    fa.smooth_partials[s] = sp;
    fa.smooth_blocks[s] = smooth_blk;
    fa.smooth_scale[s] = c.smooth_w[s];
  }
  MD2_TRY(launch_smooth(sas, c.nscales, c.C, st));
  if (nua > 0) MD2_TRY(launch_up_adjoint(uas, nua, st));
  MD2_TRY(launch_loss_finalize(fa, d_pose ? dRt : nullptr, o.loss, st));
  if (d_pose) {
    // only the learned sources are differentiated: their dRt rows, in pose-block order
    for (int s = 0; s < S && !in_place; ++s)
      if (src[s].pose_block >= 0)
        MD2_HIP(hipMemcpyAsync(dRtl + (size_t)src[s].pose_block * c.N * 12, dRt + (size_t)s * c.N * 12,
                               rt_bytes, hipMemcpyDeviceToDevice, st));
    MD2_TRY(launch_so3_bwd(pose, n_learned * c.N, c.N, invert_mask, dRtl, d_pose, 0, st));
  }
  return MD2_OK;
}
}  // namespace

size_t loss_tail_workspace_bytes(const LossTailCfg& c) { return layout(c, 2).total; }

size_t loss_tail_sources_workspace_bytes(const LossTailCfg& c, int nsrc) {
  if (nsrc < 1 || nsrc > MAX_SOURCES) return 0;
  return layout(c, nsrc).total;
}

int loss_tail_sources_run(const LossTailCfg& c, int S, const LossSource* src, const float* target,
                          long target_sample_stride, const float* const* disp, const float* pose,
                          const float* automask, float dloss, const LossTailOut& o, void* workspace,
                          hipStream_t st, const float* Kn, const float* invKn) {
  return run(c, S, src, target, target_sample_stride, nullptr, Kn, invKn, disp, pose, automask, dloss,
             o, workspace, st);
}

// the two sources are frames c.src0 / c.src1 of x, learned, with pose blocks 0 and 1
int loss_tail_run(const LossTailCfg& c, const float* const* disp, const float* pose,
                  const float* x, const float* automask, float dloss, const LossTailOut& o,
                  void* workspace, hipStream_t st) {
  MD2_CHECK_ARG(pose != nullptr && x != nullptr, "null pointer");
  const LossSource src[2] = {
      {x + c.src0 * c.x_frame_stride, c.x_sample_stride, 0, c.invert_mask & 1, nullptr},
      {x + c.src1 * c.x_frame_stride, c.x_sample_stride, 1, (c.invert_mask >> 1) & 1, nullptr}};
  return run(c, 2, src, x + c.target * c.x_frame_stride, c.x_sample_stride, x, nullptr, nullptr, disp,
             pose, automask, dloss, o, workspace, st);
}


// ---------------------------------------------------------------------------------------------
// Op-level warp + photometric loss of ONE scale (src/training.jl:43-62): upsample the disparity,
// depth, backproject, project with each composed pose, border grid_sample, SSIM + L1, min over
// the two sources (and the automask).  Forward: the per-pixel warp_loss map; pullback: from a
// per-pixel cotangent map to the disparity and to the composed poses Rt.
// ---------------------------------------------------------------------------------------------
size_t warp_op_workspace_bytes(int N, int W, int H) {
  return align256(sizeof(float) * (size_t)N * W * H) +
         align256(sizeof(float) * 25 * photometric_blocks(W, H, N, 1));
}

int warp_op_run(const WarpOpCfg& c, const float* disp, const float* Rt, const float* x,
                const float* automask, const float* d_loss, float* loss_map, signed char* sel_map,
                float* d_disp, float* d_Rt, void* workspace, hipStream_t st) {
  MD2_CHECK_ARG(c.N > 0 && c.W > 2 && c.H > 2 && c.dw >= 1 && c.dh >= 1 && c.dw <= c.W && c.dh <= c.H,
                "warp_photometric dims");
  MD2_CHECK_ARG(c.C == 1 || c.C == 3, "channels must be 1 or 3");
  MD2_CHECK_ARG(disp && Rt && x && workspace, "warp_photometric: null pointer");
  char* ws = (char*)workspace;
  float* g_full = (float*)ws;
  float* part = (float*)(ws + align256(sizeof(float) * (size_t)c.N * c.W * c.H));
  const Geom g = make_geom(c.K, c.invK, c.min_depth, c.max_depth, c.W, c.H);
  PhotoArgs pa{};
  pa.nscales = 1;
  PhotoScale& ps = pa.sc[0];
  ps.disp = disp;
  ps.dw = c.dw;
  ps.dh = c.dh;
  ps.rx = ratio(c.dw, c.W);
  ps.ry = ratio(c.dh, c.H);
  ps.g_disp = g_full;
  ps.partials = part;
  ps.loss_map = loss_map;
  ps.sel_map = sel_map;
  pa.x = x;
  pa.x_sample_stride = c.x_sample_stride;
  pa.x_frame_stride = c.x_frame_stride;
  pa.target = c.target;
  pa.src0 = c.src0;
  pa.src1 = c.src1;
  pa.Rt = Rt;
  pa.automask = automask;
  pa.wloss = d_loss ? 1.f : 0.f;
  pa.gmap = d_loss;
  pa.N = c.N;
  MD2_TRY(launch_photometric(pa, g, c.C, st));
  if (!d_loss) return MD2_OK;
  if (d_disp) {
    UpAdjArgs ua{};
    ua.g_full = g_full;
    ua.disp = disp;
    ua.dw = c.dw;
    ua.dh = c.dh;
    ua.rx = ps.rx;
    ua.ry = ps.ry;
    ua.out = d_disp;
    ua.N = c.N;
    ua.W = c.W;
    ua.H = c.H;
    MD2_TRY(launch_up_adjoint(&ua, 1, st));
  }
  if (d_Rt) {
    FinalizeArgs fa{};
    fa.nscales = 1;
    fa.N = c.N;
    fa.nsrc = 2;
    fa.photo_partials[0] = part;
    fa.photo_blocks[0] = photometric_blocks(c.W, c.H, c.N, 1);
    MD2_TRY(launch_pose_grad_reduce(fa, d_Rt, st));
  }
  return MD2_OK;
}

}  // namespace md2
