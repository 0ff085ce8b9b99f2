// Model construction: the switches, streams and events, every device allocation of build(), and
// the weight re-pack tables (model_impl.h).
#include "model_impl.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace md2 {

// the one rule of the on/off switches: on unless the value starts with '0'
static bool env_on(const char* name) {
  const char* v = getenv(name);
  return !(v && v[0] == '0');
}

Switches Switches::from_env() {
  Switches s;
  s.pose_stream = env_on("MD2_POSE_STREAM");
  s.down_stream = env_on("MD2_DOWN_STREAM");
  s.dec_wgrad_stream = env_on("MD2_DEC_WGRAD_STREAM");
  s.enc_wgrad_stream = env_on("MD2_ENC_WGRAD_STREAM");
  s.fuse_skip_bwd = env_on("MD2_FUSE_SKIP_BWD");
  s.fuse_pool_fwd = env_on("MD2_FUSE_POOL_FWD");
  s.fuse_pool_bwd = env_on("MD2_FUSE_POOL_BWD");
  s.fuse_bnstats = env_on("MD2_FUSE_BNSTATS");
  s.fuse_bn_bwd = env_on("MD2_FUSE_BN_BWD");
  s.fuse_bn_fwd = env_on("MD2_FUSE_BN_FWD");
  s.fuse_splitk = env_on("MD2_FUSE_SPLITK");
  s.bn_collapse = tuning_knob("MD2_BN_COLLAPSE", 0) != 0;
  s.enc_wgrad_from = tuning_knob("MD2_ENC_WGRAD_FROM", 1);
  s.enc_wgrad_main0 = tuning_knob("MD2_ENC_WGRAD_MAIN0", 1) != 0;
  return s;
}

int Overlap::create() {
  MD2_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
  MD2_HIP(hipStreamCreateWithFlags(&upd, hipStreamNonBlocking));
  for (hipEvent_t* e : {&seg_ev, &upd_ev, &fork_ev, &join_ev, &ev_a, &ev_b, &ev_c2, &ev_c1, &ev_y[0], &ev_y[1]})
    MD2_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  return MD2_OK;
}

Overlap::~Overlap() {
  if (side) (void)hipStreamDestroy(side);
  if (upd) (void)hipStreamDestroy(upd);
  for (hipEvent_t e : {seg_ev, upd_ev, fork_ev, join_ev, ev_a, ev_b, ev_c2, ev_c1, ev_y[0], ev_y[1]})
    if (e) (void)hipEventDestroy(e);
}

Model::Model() : sw(Switches::from_env()) {}

Model::~Model() {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.st) (void)hipStreamDestroy(g.st);
  for (void* p : allocs) (void)hipFree(p);
}

// n elements of `elem` bytes; `counted` ones add to model_device_bytes
int Model::alloc_bytes(void** p, size_t elem, size_t n, bool counted) {
  void* q = nullptr;
  MD2_HIP(hipMalloc(&q, std::max<size_t>(n, 1) * elem));
  allocs.push_back(q);
  if (counted) bytes += n * elem;
  *p = q;
  return MD2_OK;
}

int Model::make_conv(RConv& r, const PConv& p, int H, int W, bool dgrad, int cin_pad) {
  r.p = p;
  r.s.N = 0;
  r.s.Cin = cin_pad > 0 ? cin_pad : p.cin;   // cin_pad: zero input channels beyond the weights' p.cin
  r.s.cin_w = cin_pad > 0 ? p.cin : 0;
  r.s.Cout = p.cout;
  r.s.H = H;
  r.s.W = W;
  r.s.KH = r.s.KW = p.k;
  r.s.stride = p.stride;
  r.s.pad = p.pad;
  r.s.reflect = p.reflect;
  r.s.Ho = out_dim(H, p.k, p.stride, p.pad);
  r.s.Wo = out_dim(W, p.k, p.stride, p.pad);
  // packed weights: the repack writes only real elements, the padding stays zero from here
  MD2_TRY(alloc(&r.wpf, conv_fwd_packed_elems(r.s)));
  MD2_HIP(hipMemset(r.wpf, 0, conv_fwd_packed_elems(r.s) * sizeof(float)));
  if (dgrad) {
    MD2_TRY(alloc(&r.wpd, conv_dgrad_packed_elems(r.s)));
    MD2_HIP(hipMemset(r.wpd, 0, conv_dgrad_packed_elems(r.s) * sizeof(float)));
  }
  return MD2_OK;
}

void Model::need_ws(const RConv& r, int nimg, size_t& ws_need, bool dgrad) {
  const ConvShape s = shape(r, nimg);
  ws_need = std::max(ws_need, conv_fwd_workspace(s));
  ws_need = std::max(ws_need, conv_wgrad_workspace(s));
  if (dgrad) ws_need = std::max(ws_need, conv_dgrad_workspace(s));
}

int Model::make_bn(RBN& r, const PBN& p) {
  r.p = p;
  MD2_TRY(alloc(&r.mean, p.c));
  MD2_TRY(alloc(&r.invstd, p.c));
  MD2_CHECK_ARG(bn_layout.n < MAX_BN, "make_bn: too many BatchNorm layers");
  r.rmean = bn_stats + bn_layout.off[bn_layout.n];
  r.rvar = r.rmean + p.c;
  bn_layout.off[bn_layout.n + 1] = bn_layout.off[bn_layout.n] + 2 * p.c;
  ++bn_layout.n;
  MD2_HIP(hipMemset(r.rmean, 0, p.c * sizeof(float)));
  std::vector<float> ones(p.c, 1.f);
  MD2_HIP(hipMemcpy(r.rvar, ones.data(), p.c * sizeof(float), hipMemcpyHostToDevice));
  return MD2_OK;
}

int Model::build() {
  const ArchCfg& A = cfg.arch;
  spec = build_spec(A);
  N = cfg.N;
  B = 3 * N;
  E = A.emb;
  NP = E > 0 ? cfg.num_bins : 1;
  Ep = E > 0 ? (E + 15) / 16 * 16 : 0;
  ND = N * NP;
  const int C = A.in_ch;
  size_t wsn = 0, wsn_side = 0, scratch = 0;   // wsn_side: side-stream convs (downsample, pose, decoder wgrad)
  long bnmax = 0;
  auto track = [&](long n) { scratch = std::max(scratch, (size_t)n); };
  auto bnws_need = [&](int Cc, long HW) {
    bnmax = std::max(bnmax, (long)Cc * bn_parts(Cc, B, HW) * 2);
    bnmax = std::max(bnmax, (long)Cc * ((B * HW + 255) / 256) * 2);   // per-tile epilogue partials
  };
  // ---- encoder
  long nst = 0;
  for (auto& e : spec.table)
    if (is_gamma(e)) nst += 2 * e.numel;
  MD2_TRY(alloc(&bn_stats, nst));
  MD2_TRY(alloc(&bn_flag, 16));
  MD2_TRY(make_conv(stem, spec.stem, cfg.H, cfg.W, false));
  need_ws(stem, B, wsn, false);
  MD2_TRY(make_bn(stem_bn, spec.stem_bn));
  H0 = stem.s.Ho;
  W0 = stem.s.Wo;
  Hm = out_dim(H0, 3, 2, 1);
  Wm = out_dim(W0, 3, 2, 1);
  const long n0 = (long)B * 64 * H0 * W0, nm = (long)B * 64 * Hm * Wm;
  MD2_TRY(alloc(&y0, n0));
  MD2_TRY(alloc(&f0, n0));
  MD2_TRY(alloc(&d_f0, n0));
  MD2_TRY(alloc(&mp, nm));
  MD2_TRY(alloc(&d_mp, nm));
  MD2_TRY(alloc(&mp_arg, nm, false));
  track(n0);
  bnws_need(64, (long)H0 * W0);
  feat[0] = f0; featC[0] = 64; featH[0] = H0; featW[0] = W0;
  float* cur = mp;
  float* dcur = d_mp;
  int cC = 64, cH = Hm, cW = Wm;
  stages.resize(4);
  for (int si = 0; si < 4; ++si) {
    for (auto& bs : spec.stages[si]) {
      EncBlock eb;
      eb.in = cur;
      eb.d_in = dcur;
      eb.Cin = cC; eb.Hin = cH; eb.Win = cW;
      int h = cH, w = cW;
      for (size_t k = 0; k < bs.convs.size(); ++k) {
        EncStage es;
        MD2_TRY(make_conv(es.conv, bs.convs[k], h, w, true));
        es.conv.cat = bs.convs[k].k == 3 ? PROF_CONV3_ENC : PROF_CONV_OTHER;
        need_ws(es.conv, B, wsn, true);
        need_ws(es.conv, B, wsn_side, false);   // filter gradient on the side (enc_overlap)
        MD2_TRY(make_bn(es.bn, bs.bns[k]));
        h = es.conv.s.Ho;
        w = es.conv.s.Wo;
        const long n = (long)B * bs.convs[k].cout * h * w;
        MD2_TRY(alloc(&es.y, n));
        MD2_TRY(alloc(&es.a, n));
        track(n);
        bnws_need(bs.convs[k].cout, (long)h * w);
        eb.st.push_back(es);
      }
      if (bs.down) {
        eb.down = true;
        MD2_TRY(make_conv(eb.dconv, bs.dconv, cH, cW, true));
        need_ws(eb.dconv, B, wsn_side, true);
        MD2_TRY(make_bn(eb.dbn, bs.dbn));
        MD2_TRY(alloc(&eb.yd, (long)B * bs.cout * h * w));
      }
      eb.C = bs.cout; eb.H = h; eb.W = w;
      MD2_TRY(alloc(&eb.d_out, (long)B * bs.cout * h * w));
      cur = eb.st.back().a;
      dcur = eb.d_out;
      cC = bs.cout; cH = h; cW = w;
      stages[si].push_back(eb);
    }
    feat[si + 1] = cur;
    featC[si + 1] = cC; featH[si + 1] = cH; featW[si + 1] = cW;
  }
  // ---- depth decoder (ND = N target images, times P planes in MPI mode)
  if (E > 0) {
    MD2_TRY(alloc(&bins, (long)N * NP));
    MD2_HIP(hipMemset(bins, 0, sizeof(float) * N * NP));
    MD2_TRY(alloc(&emb_in[4], (long)ND * (featC[4] + Ep) * featH[4] * featW[4]));
    MD2_TRY(alloc(&d_emb[4], (long)ND * (featC[4] + Ep) * featH[4] * featW[4]));
  }
  int h = featH[4], w = featW[4];
  for (auto& bs : spec.branches) {
    DecBranch d;
    d.b = bs;
    d.h = h;
    d.w = w;
    // MPI mode: the inputs carrying embedding channels run padded (Ep)
    const int pad1 = (E > 0 && bs.bid == 1) ? bs.c1.cin - E + Ep : 0;
    const int pad2 = (E > 0 && bs.cskip > 0) ? bs.c2.cin - E + Ep : 0;
    MD2_TRY(make_conv(d.c1, bs.c1, h, w, true, pad1));
    need_ws(d.c1, ND, wsn, true);
    MD2_TRY(make_conv(d.c2, bs.c2, 2 * h, 2 * w, true, pad2));
    need_ws(d.c2, ND, wsn, true);
    need_ws(d.c1, ND, wsn_side, false);   // filter gradients on the side stream (wgrad_overlap)
    need_ws(d.c2, ND, wsn_side, false);
    MD2_TRY(alloc(&d.o1, (long)ND * bs.cout * h * w));
    MD2_TRY(alloc(&d.up, (long)ND * bs.cout * 4 * h * w));
    MD2_TRY(alloc(&d.o2, (long)ND * bs.cout * 4 * h * w));
    MD2_TRY(alloc(&d.d_o2, (long)ND * bs.cout * 4 * h * w));
    track((long)ND * d.c2.s.Cin * 4 * h * w);
    if (bs.head >= 0) {
      d.head = bs.head;
      MD2_TRY(make_conv(d.hc, spec.heads[bs.head], 2 * h, 2 * w, true));
      need_ws(d.hc, ND, wsn, true);
      MD2_TRY(alloc(&d.disp, (long)ND * 4 * h * w));
      MD2_TRY(alloc(&d.d_head, (long)ND * 4 * h * w));
    }
    if (bs.bid <= 4) {
      const int fi = 4 - bs.bid;
      if (featH[fi] != 2 * h || featW[fi] != 2 * w) {
        set_error("decoder/encoder resolution mismatch (image sides must be multiples of 32)");
        return MD2_EINVAL;
      }
      MD2_TRY(alloc(&d_skip[fi], (long)N * featC[fi] * 4 * h * w));
      if (E > 0) {
        MD2_TRY(alloc(&emb_in[fi], (long)ND * (featC[fi] + Ep) * 4 * h * w));
        MD2_TRY(alloc(&d_emb[fi], (long)ND * (featC[fi] + Ep) * 4 * h * w));
      }
    }
    h *= 2;
    w *= 2;
    br.push_back(d);
  }
  for (auto& d : br)
    if (d.head >= 0) heads.push_back(&d);
  {
    HeadJob jobs[MAX_HEADS];
    const int nh = head_jobs(jobs, ND);
    if (nh > 0) MD2_TRY(alloc(&hws, heads_bwd_workspace(jobs, nh) / sizeof(float) + 64));
  }
  // ---- pose decoder (2N pairs)
  const int h4 = featH[4], w4 = featW[4];
  const long hw4 = (long)h4 * w4;
  MD2_TRY(make_conv(sq, spec.squeezer, h4, w4, true));
  need_ws(sq, B, wsn_side, true);
  MD2_TRY(make_conv(p1, spec.p1, h4, w4, true));
  need_ws(p1, 2 * N, wsn_side, true);
  MD2_TRY(make_conv(p2, spec.p2, h4, w4, true));
  need_ws(p2, 2 * N, wsn_side, true);
  p1.cat = p2.cat = PROF_CONV3_ENC;     // zero-padded 3x3 like the encoder's (same kernels)
  MD2_TRY(alloc(&sqo, (long)B * 256 * hw4));
  MD2_TRY(alloc(&d_sq, (long)B * 256 * hw4));
  MD2_TRY(alloc(&pc1, 2L * N * 256 * hw4));
  MD2_TRY(alloc(&d_pc1, 2L * N * 256 * hw4));
  MD2_TRY(alloc(&pc2, 2L * N * 256 * hw4));
  MD2_TRY(alloc(&d_pin, 2L * N * 512 * hw4));
  for (int j = 0; j < 2; ++j) {
    const int s = j ? cfg.src1 : cfg.src0;
    pa[j] = std::min(s, cfg.target);
    pb[j] = std::max(s, cfg.target);
  }
  pairs_inplace = pa[0] == 0 && pa[1] == 1 && pb[0] == 1 && pb[1] == 2;
  if (!pairs_inplace) MD2_TRY(alloc(&pin, 2L * N * 512 * hw4));
  T0 = cfg.target * N;
  MD2_TRY(alloc(&means, 2L * N * 256));
  MD2_TRY(alloc(&pose, 2L * N * 6));
  MD2_TRY(alloc(&d_pose, 2L * N * 6));
  track(2L * N * 512 * hw4);
  // ---- scratch / workspaces
  for (float** p : {&DA, &DY, &DY2, &G, &DYD, &DPRE, &DUP, &DO1}) MD2_TRY(alloc(p, scratch));
  auto workspace = [&](ConvWorkspace& ws, size_t need) -> int {
    float* q;
    MD2_TRY(alloc(&q, need / sizeof(float) + 64));
    ws.ptr = q;
    ws.bytes = need + 256;
    return MD2_OK;
  };
  MD2_TRY(workspace(cws, wsn));
  MD2_TRY(alloc(&bp_ws, BP_WS));
  MD2_TRY(workspace(cws_side, wsn_side));
  MD2_TRY(alloc(&bp_ws_side, BP_WS));
  MD2_TRY(alloc(&DPRE_side, 2L * N * 256 * hw4));
  MD2_TRY(ov.create());
  MD2_TRY(alloc(&bp_dec[0], BP_WS));
  MD2_TRY(alloc(&bp_dec[1], BP_WS));
  bn_slot = std::max<long>(bnmax, 2);
  MD2_TRY(alloc(&bnws.partials, 2 * bn_slot, false));
  MD2_TRY(alloc(&bn_collapsed, 2 * 4096 * 2, false));
  // ---- loss tail (src/training.jl:21-78).  MPI mode: the ND plane disparities are the batch
  // (training.jl:42-51 reshapes depth to (1, W*H, dn) with dn = num_bins*N); the poses and the
  // frames of the one sample broadcast over its planes (Project's batched_mul of the 3x3x1 R,
  // grid_sample and SSIM against the N = 1 images): x sample stride 0, poses / automask
  // repeated per plane
  if (E > 0) {
    MD2_TRY(alloc(&pose_rep, 2L * ND * 6));
    MD2_TRY(alloc(&d_pose_rep, 2L * ND * 6));
    if (cfg.automask) MD2_TRY(alloc(&amask_rep, (long)ND * cfg.H * cfg.W));
  }
  tail.N = ND;
  tail.C = C;
  tail.W = cfg.W;
  tail.H = cfg.H;
  tail.nscales = A.nlevels;
  for (size_t li = 0; li < heads.size(); ++li) {
    tail.dw[li] = 2 * heads[li]->w;
    tail.dh[li] = 2 * heads[li]->h;
    tail.smooth_w[li] = cfg.smoothness * cfg.scales[li];
  }
  tail.divisor = (float)A.nlevels;
  tail.smooth_normalize = 1;
  std::memcpy(tail.K, cfg.K, sizeof(tail.K));
  std::memcpy(tail.invK, cfg.invK, sizeof(tail.invK));
  tail.min_depth = cfg.min_depth;
  tail.max_depth = cfg.max_depth;
  tail.x_frame_stride = (long)C * cfg.H * cfg.W;
  tail.x_sample_stride = E > 0 ? 0 : 3 * tail.x_frame_stride;   // MPI: N == 1, planes share x
  tail.target = cfg.target;
  tail.src0 = cfg.src0;
  tail.src1 = cfg.src1;
  tail.invert_mask = (cfg.src0 < cfg.target ? 1 : 0) | (cfg.src1 < cfg.target ? 2 : 0);
  tail.sigmoid_grad = 1;
  {
    float* q;
    MD2_TRY(alloc(&q, loss_tail_workspace_bytes(tail) / sizeof(float) + 64));
    tail_ws = q;
  }
  MD2_TRY(alloc(&loss_buf, 16));
  if (cfg.automask) MD2_TRY(alloc(&amask, (long)N * cfg.H * cfg.W));
  return build_pack_table();
}

int Model::build_pack_table() {
  std::vector<PackJob> jobs;
  auto pk = [&](RConv& c) { jobs.push_back(conv_pack_job(c.s, params + c.p.w, c.wpf, c.wpd)); };
  pk(stem);
  for (auto& sg : stages)
    for (auto& b : sg) {
      for (auto& e : b.st) pk(e.conv);
      if (b.down) pk(b.dconv);
    }
  for (auto& d : br) {
    pk(d.c1);
    pk(d.c2);
    if (d.head >= 0) pk(d.hc);
  }
  pk(sq);
  pk(p1);
  pk(p2);
  // a table's jobs numbered from block 0, on the device
  auto table = [&](std::vector<PackJob>& js, PackTable& t) -> int {
    t = PackTable{};
    if (js.empty()) return MD2_OK;
    for (auto& j : js) {
      j.block_begin = t.blocks;
      t.blocks += conv_pack_job_blocks(j);
    }
    t.njobs = (int)js.size();
    return upload(js, &t.jobs, false);
  };
  MD2_TRY(table(jobs, pack));
  for (int k = 0; k < 6; ++k) {
    long b0, e0;
    segment_range(k, b0, e0);
    std::vector<PackJob> sj;
    for (const PackJob& j : jobs) {
      const long off = (long)(j.w - params);
      if (off >= b0 && off < e0) sj.push_back(j);
    }
    MD2_TRY(table(sj, seg_pack[k]));
  }
  return MD2_OK;
}

void Model::segment_range(int k, long& b, long& e) const {
  const ArchSpec& S = spec;
  switch (k) {
    case 0: b = S.depth_begin; e = S.total; break;
    case 1: b = S.stage_begin[4]; e = S.depth_begin; break;
    case 2: b = S.stage_begin[3]; e = S.stage_begin[4]; break;
    case 3: b = S.stage_begin[2]; e = S.stage_begin[3]; break;
    case 4: b = S.stage_begin[1]; e = S.stage_begin[2]; break;
    default: b = 0; e = S.stage_begin[1]; break;
  }
}

}  // namespace md2
