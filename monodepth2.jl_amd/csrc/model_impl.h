// The executor behind model.h: the runtime structures and the one declaration of Model.  Data
// members and signatures only; the definitions are one translation unit per phase:
//   model_build.cpp     allocation, build(), the pack tables, the switches, streams and events
//   model_forward.cpp   conv_f*, BatchNorm statistics, encoder / decoder / pose forward, the loss
//   model_backward.cpp  conv_w / conv_d*, BatchNorm backward, the backward segments, cotangents
//   model_testmode.cpp  the folded inference encoder and the running statistics
//   model.cpp           the model_* entry points, the optimiser plumbing and the profiler
//
// Data layout in HBM (all fp32, NCHW == Julia (W,H,C,N)):
//   * encoder batch is FRAME-MAJOR: image b = l*N + n holds frame l of sample n (the stem reads
//     x[n][l] through a batch map), so the target frames form the contiguous slice [N, 2N) that
//     the DepthDecoder reads as skips, and pose pairs (frame s, frame s+1) are (b, b+N).  BatchNorm
//     statistics run over all 3N frames exactly like ResNet.jl on reshape(x, (W,H,C,L*N)).
//   * parameters / gradients are caller-owned flat fp32 vectors in the order of
//     oracle/md2_oracle.py param_spec; conv weights are re-packed K-major after each update.
#pragma once
#include "head.h"
#include "model_spec.h"
#include "testmode.h"

namespace md2 {

struct RConv {
  PConv p;
  ConvShape s{};          // N filled per call
  float* wpf = nullptr;   // packed forward weights
  float* wpd = nullptr;   // packed dgrad weights
  float* wpt = nullptr;   // test mode: packed forward weights of the BatchNorm-folded copy
  int cat = PROF_CONV_OTHER;
};
struct RBN {
  PBN p;
  float *mean = nullptr, *invstd = nullptr, *rmean = nullptr, *rvar = nullptr;
  const double* part = nullptr;   // statistics partials of the current forward (bn_fwd)
  int parts = 0;
  float *ts = nullptr, *tt = nullptr;   // test mode: the folded affine map (s, t)
};
// The apply that follows a conv's BatchNorm, handed to conv_f_bn: where a channel fits in a block
// (bn_channel_fits) statistics and apply are one kernel there, and `done` says so; otherwise the
// caller runs bn_apply_fused as before.  a.y and a.s1 are conv_f_bn's to fill.
struct BNTail {
  BNApplyFused a;
  float* out = nullptr;
  hipEvent_t join = nullptr;   // the side stream's event behind a.y2, awaited before the one kernel
  bool done = false;
};
struct EncStage {
  RConv conv;
  RBN bn;
  float* y = nullptr;     // conv output
  float* a = nullptr;     // post BN (+ReLU); block output for the last stage
};
struct EncBlock {
  std::vector<EncStage> st;
  bool down = false;
  RConv dconv;
  RBN dbn;
  float* yd = nullptr;
  float* in = nullptr;
  float* d_in = nullptr;
  float* d_out = nullptr;
  int C = 0, H = 0, W = 0;      // output
  int Cin = 0, Hin = 0, Win = 0;
};
struct DecBranch {
  BranchSpec b;
  RConv c1, c2;
  int h = 0, w = 0;             // c1 resolution (input); output 2h x 2w
  float *o1 = nullptr, *up = nullptr, *o2 = nullptr, *d_o2 = nullptr;
  int head = -1;
  RConv hc;
  float* disp = nullptr;
  float* d_head = nullptr;      // gradient w.r.t. the head pre-activation (from the loss tail)
};

// On/off switches, read once per Model at construction (an executor keeps its setting when the
// variable changes afterwards).  MD2_<NAME>=0 switches a default-on path off: the stream switches
// run everything on the model stream, the fuse switches restore the separate passes (A/B
// measurements, tests/test_gpu_fusion.py).  The last three are tuning knobs (MD2_TUNING=1 only).
struct Switches {
  bool pose_stream, down_stream, dec_wgrad_stream, enc_wgrad_stream;
  bool fuse_skip_bwd;    // 0: the axpy of the decoder skip gradients (bit-identical)
  bool fuse_pool_fwd;    // 0: bn_apply_fused + maxpool_fwd for the stem (bit-identical)
  bool fuse_pool_bwd;    // 0: the stem's separate skip-gradient axpy after maxpool_bwd (bit-identical)
  bool fuse_bnstats;     // 0: the statistics pass after the LDS-halo forward convs
  // 0: the two-pass BN backward (partials + apply) where a channel fits in one block of
  // bn_bwd_channel (closeness test: the fp64 sums run in another order)
  bool fuse_bn_bwd;
  // 0: the two-pass BN forward (statistics partials + apply) where a channel fits in one block of
  // bn_fwd_channel and the conv took no statistics in its epilogue (closeness test, as above)
  bool fuse_bn_fwd;
  bool fuse_splitk;     // 0: the separate reduction launches (A/B measurement)
  bool bn_collapse;      // MD2_BN_COLLAPSE=1: one collapse launch first -- measured slower, 6 us per launch
  // (round 6, with the LDS-halo kernels: from layer 2 (si = 1) 6.194 vs 6.211 ms and 6.159 vs 6.19
  // against layer 4 only, interleaved; from layer 1 6.167)
  int enc_wgrad_from;
  // (1: -45 us per step, 6.555 vs 6.60 ms interleaved; the side stream was the longer path of the
  // layer-4 segment)
  bool enc_wgrad_main0;
  static Switches from_env();
};

// Side stream for independent branches, each with its OWN scratch (split-K workspace,
// bias-gradient partials, activation-pullback buffer, BN partials slot 1) so they can run
// beside the model stream:
//  * the PoseDecoder depends only on the encoder's layer-4 features (forward) and on d_pose
//    from the loss tail (backward): it runs beside the DepthDecoder and joins before the loss
//    tail (poses) and before the decoder's first-branch dgrad accumulates into the layer-4
//    feature gradient the squeezer's dgrad wrote (MD2_POSE_STREAM);
//  * a downsampling block's 1x1 conv + BN depends only on the block input: its forward runs
//    beside the block's 3x3 chain and joins before the residual BN apply; its backward runs
//    beside the chain's backward and joins before the first conv's dgrad accumulates into the
//    block's input gradient the 1x1 dgrad wrote (MD2_DOWN_STREAM);
//  * the DepthDecoder's filter gradients beside its data gradients (MD2_DEC_WGRAD_STREAM): each
//    conv's on the side beside its data gradient and the rest of the branch (the decoder convs
//    fill a fraction of the chip).  The side reads DPRE / DO1 and the bias partials of the
//    act_bias before it, so those buffers are reused only after the side's event (ev_c2 / ev_c1;
//    bias partials double-buffered: bp_dec[0] for c2, [1] for c1);
//  * the encoder backward of the last stages (stages >= enc_wgrad_from: layers 2-4 by default; the
//    convs are small and split-K): each block conv's filter gradient beside its data gradient
//    (interleaved A/B, 3 x 60 steps: off 1481, from layer 4 1493, from layer 3 1490, from layer 2
//    1478 images/s -- the larger layers' convs fill the chip and only time-share).  The conv's dY
//    alternates between DY and DY2 so the data gradient's BN backward can write the next dY while
//    the side still reads the current one; a dY buffer is written again only after the side's
//    event for its last read (ev_y[j]); every stage segment ends with the side joined
//    (MD2_ENC_WGRAD_STREAM).
// The arithmetic is unchanged (same kernels, same buffers' contents): the step is
// bit-identical with any switch off (=0, tests/test_gpu_fusion.py) and under the HIP-event
// probe, which runs everything on the model stream so that its brackets time kernels alone.
//
// Update stream (model_adam_segment): ADAM over a backward segment's parameter range and the
// re-pack of that segment's conv weights, on a stream of their own as soon as the segment's
// gradient is final -- beside the remaining backward instead of after it.  Safe: no later backward
// segment reads an earlier segment's parameters or packed weights (the segments are decoders,
// layer 4, ..., stem: each reads only its own), and the next forward waits for the updates
// (model_adam_join).
struct Overlap {
  hipStream_t side = nullptr, upd = nullptr;
  hipEvent_t seg_ev = nullptr, upd_ev = nullptr, fork_ev = nullptr, join_ev = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c2 = nullptr, ev_c1 = nullptr;
  hipEvent_t ev_y[2] = {nullptr, nullptr};
  bool upd_recorded = false;   // upd_ev holds the newest adam_segment's completion
  bool y_pending[2] = {false, false};
  int ycur = 0;
  bool side_ws = false;        // conv / act_bias calls of a side branch: its own scratch
  int create();
  ~Overlap();
};
// the conv / act_bias calls in its scope use the side scratch, on every exit path
struct SideScratch {
  bool& flag;
  const bool was;
  explicit SideScratch(Overlap& ov) : flag(ov.side_ws), was(ov.side_ws) { flag = true; }
  ~SideScratch() { flag = was; }
};

// optional HIP-event profiling of the hot kernels (bench.py roofline)
struct Profiler {
  struct Rec {
    hipEvent_t a, b;
    int cat;
    double work;
    char tag[64];   // pass + shape of a conv record (per-layer table), "" otherwise
  };
  bool on = false;
  std::vector<Rec> recs;
  std::vector<hipEvent_t> evpool;
  size_t evi = 0;
  hipEvent_t ev();
  hipEvent_t begin(hipStream_t st);
  void end(hipEvent_t a, int cat, double work, hipStream_t st, const char* pass = nullptr,
           const ConvShape* s = nullptr);
  void reset();
  int read(double* out, int ncat);
  // per-record view of the same events (per-layer table); clears like read
  int records(int max, double* ms, double* work, int* cat, char* tags, int tag_len, int* count);
  ~Profiler();
};

// Test mode (Flux testmode!, md2_model_set_testmode): BatchNorm on the running statistics.  Each
// encoder BatchNorm is folded into the conv before it -- a scratch copy of the encoder's conv
// weights scaled by s (bn_fold_batch, which also writes the t vectors), packed by the unchanged
// conv_pack_batch into a SECOND set of forward packs (wpt); the train-mode packs are never
// written.  The stem keeps its space-to-depth kernel (no bias operand): its (s, t) are applied by
// affine_relu_maxpool.  Everything is allocated at the first switch to test mode.
struct TestMode {
  bool on = false;
  float* wfold = nullptr;       // [spec.depth_begin]: folded conv weights at their parameter offsets
  float* st = nullptr;          // (s, t) of every BatchNorm, laid out like bn_stats
  FoldJob* fold_jobs = nullptr;
  int fold_njobs = 0;
  long fold_blocks = 0;
  PackJob* pack_jobs = nullptr;
  int pack_njobs = 0;
  long pack_blocks = 0;
};

// graph-captured single-GPU step (model_train_step_graph): the executor owns the input copy,
// the loss slot and the device ADAM step counter, so one capture replays for every batch/step
struct StepGraph {
  hipGraphExec_t exec = nullptr;
  hipStream_t st = nullptr;
  float *x = nullptr, *x_net = nullptr, *autoloss = nullptr, *loss = nullptr, *bc = nullptr;
  float *x_stereo = nullptr, *stereo_Rt = nullptr;   // train_step_graph_stereo's input copies
  int stereo_mode = -1;   // part of the capture: 0 no stereo source, 1 MS (temporal), 2 S
  int intrinsics = -1;    // so is whether per-sample intrinsics are set (their values are not)
  int* step = nullptr;
  float *adam_m = nullptr, *adam_v = nullptr;
  float lr = 0.f;
  int with_auto = -1;
  int with_net = -1;   // a separate network input (train_step_graph_aug) is part of the capture
  int guard_on = -1;   // the gradient guard and its max_norm are part of the capture too
  float guard_max = 0.f;
  int next_step = -1;
};

// The stereo source of one forward_loss (md2_model_forward_loss_stereo): the partner camera's frame
// x [N][C][H][W], its fixed transform Rt [N][12], and whether the temporal sources take part (MS) or
// not (S).  Only the loss tail and the automask read it.
struct StereoIn {
  const float* x;
  const float* Rt;
  int temporal;
};

// Gradient guard (md2_model_set_grad_guard): between the backward and ADAM, grad_norm over the whole
// flat gradient writes `state`, which the guarded ADAM reads.  Both buffers are allocated at the
// first switch-on and kept.
struct GradGuard {
  bool on = false;
  float max_norm = 0.f;
  md2_guard_state* state = nullptr;
  void* ws = nullptr;
};

class Model {
 public:
  Model();
  ~Model();

  // ---- configuration and geometry
  ModelCfg cfg;
  ArchSpec spec;
  float* params = nullptr;
  float* grads = nullptr;
  int N = 0, B = 0;             // samples, encoder images (3N)
  // MPI mode (src/model.jl:31-55): E embedding channels, NP planes per sample, ND = N*NP decoder
  // images (image n*NP + p).  emb_in[f] = cat(repeat(target features f, P), repeat(embed(bins),
  // h, w)) is the decoder's input / skip of level f; d_emb[f] its gradient, block-summed over the
  // planes into the target features' gradient (the _repeat pullback, src/repeat.jl:44-53).
  int E = 0, NP = 1, ND = 0;
  // MPI mode: the E embedding channels of every decoder input are stored padded to Ep = E rounded
  // up to 16 (zero channels with zero weights), so C + Ep stays a multiple of 16 and the decoder
  // convs run on the tap-major kernels (conv_tap_major); the weights keep the reference's E
  int Ep = 0;
  int H0 = 0, W0 = 0;           // stem output
  int Hm = 0, Wm = 0;           // maxpool output
  float* feat[5] = {};
  int featC[5] = {}, featH[5] = {}, featW[5] = {};
  int T0 = 0;                   // image offset of the target frame's slice (target * N)
  // pose pair j of sample q = frames (pa[j], pb[j]) (src/model.jl:57-70); the default (target 2,
  // sources 1, 3) pairs are images (q, q+N) and read sqo in place, other ids gather into pin
  int pa[2] = {0, 1}, pb[2] = {1, 2};
  bool pairs_inplace = true;
  LossTailCfg tail{};

  // ---- device memory: everything build() and testmode_alloc() allocate, freed by ~Model
  std::vector<void*> allocs;
  size_t bytes = 0;             // model_device_bytes: the counted allocations
  int alloc_bytes(void** p, size_t elem, size_t n, bool counted);
  template <class T>
  int alloc(T** p, size_t n, bool counted = true) { return alloc_bytes((void**)p, sizeof(T), n, counted); }
  // a host table on the device
  template <class T>
  int upload(const std::vector<T>& v, T** p, bool counted) {
    MD2_TRY(alloc(p, v.size(), counted));
    MD2_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return MD2_OK;
  }
  float* P(long off) { return off >= 0 ? params + off : nullptr; }
  float* Gd(long off) { return off >= 0 ? grads + off : nullptr; }

  // ---- layers and activations
  RConv stem;
  RBN stem_bn;
  float *y0 = nullptr, *f0 = nullptr, *mp = nullptr, *d_mp = nullptr, *d_f0 = nullptr;
  unsigned char* mp_arg = nullptr;
  std::vector<std::vector<EncBlock>> stages;
  std::vector<DecBranch> br;
  std::vector<DecBranch*> heads;    // the branches a disparity head follows: heads[li] is level li
  float* d_skip[4] = {};
  float* emb_in[5] = {};
  float* d_emb[5] = {};
  float* bins = nullptr;                        // [N][P]
  float *pose_rep = nullptr, *d_pose_rep = nullptr, *amask_rep = nullptr;
  RConv sq, p1, p2, p3;             // pose
  float *sqo = nullptr, *pc1 = nullptr, *pc2 = nullptr, *means = nullptr, *pose = nullptr;
  float *d_pose = nullptr, *d_pc1 = nullptr, *d_pin = nullptr, *d_sq = nullptr;
  float* pin = nullptr;
  float* hws = nullptr;         // the DepthDecoder's disparity heads run as one batch per pass (head.h)
  void* tail_ws = nullptr;
  void* tail_src_ws = nullptr;  // the sources form's workspace (3 sources), allocated at first use
  int ensure_stereo_ws();
  // per-sample intrinsics (md2_model_set_intrinsics): executor-owned [N][9] copies, allocated at the
  // first set; while intr_on every forward_loss runs the sources form of the loss tail with them
  float *Kn = nullptr, *invKn = nullptr;
  bool intr_on = false;
  float* loss_buf = nullptr;
  float* amask = nullptr;       // automasking_loss of the current batch when the caller passes none
  // Running statistics of every BatchNorm in ONE flat vector (the layout of
  // md2_model_get_bn_stats: per BatchNorm C means then C variances, in the order of the gamma
  // entries of the parameter table -- the order make_bn is called in)
  float* bn_stats = nullptr;
  BNStatLayout bn_layout{};
  int* bn_flag = nullptr;       // device flag of the set_bn_stats check
  // one batched launch re-packs every conv weight (forward and dgrad layouts) after an update;
  // each weight is read once and written to both layouts.  seg_pack: the same jobs grouped by the
  // backward segment that owns their parameters (each group with its own block numbering)
  struct PackTable {
    PackJob* jobs = nullptr;
    int njobs = 0;
    long blocks = 0;
  } pack, seg_pack[6];

  // ---- scratch
  float *DA = nullptr, *DY = nullptr, *DY2 = nullptr, *G = nullptr, *DYD = nullptr;
  float *DPRE = nullptr, *DUP = nullptr, *DO1 = nullptr, *DPRE_side = nullptr;
  ConvWorkspace cws{}, cws_side{};
  static constexpr long BP_WS = 8192;
  float *bp_ws = nullptr, *bp_ws_side = nullptr;
  float* bp_dec[2] = {nullptr, nullptr};
  BNStatsWs bnws{};
  long bn_slot = 0;                 // doubles per partials slot (slot 1: the downsample BN of a block)
  double* bn_collapsed = nullptr;   // [2 slots][4096 channels][2]: collapsed epilogue partials

  const Switches sw;
  Overlap ov;
  Profiler pf;
  TestMode tm;
  StepGraph g;
  GradGuard gd;

  // ---- step state
  const float* cur_x = nullptr;
  // 0: the last forward was forward-only (the backward needs md2_model_set_cotangents first);
  // 1: the backward's cotangents are in place (forward_loss, or set_cotangents after forward)
  int cot_ready = 0;
  // activation pullback fused with the bias-gradient partials of the conv that produced `out`
  // (act_bias; consumed by that conv's next conv_w)
  const float* bp_pending = nullptr;
  int bp_parts = 0;
  std::string dbg_name;   // storage behind model_debug_tensor's name

  // ---- overlap predicates and scratch selection (the HIP-event probe switches every overlap off)
  bool pose_overlap() const { return sw.pose_stream && ov.side && !pf.on; }
  bool wgrad_overlap() const { return sw.dec_wgrad_stream && ov.side && !pf.on; }
  bool down_overlap() const { return sw.down_stream && ov.side && !pf.on; }
  bool enc_overlap(int si) const { return sw.enc_wgrad_stream && ov.side && !pf.on && si >= sw.enc_wgrad_from; }
  ConvWorkspace& ws_conv() { return ov.side_ws ? cws_side : cws; }
  float* ws_bp() { return ov.side_ws ? bp_ws_side : bp_ws; }
  float* ybuf(int j) { return j ? DY2 : DY; }
  int y_claim(int j, hipStream_t st);   // the model stream is about to write dY buffer j
  int stream_wait(hipStream_t st1, hipStream_t st2, hipEvent_t e);   // st2 waits for st1 so far

  // ---- build (model_build.cpp)
  int make_conv(RConv& r, const PConv& p, int H, int W, bool dgrad, int cin_pad = 0);
  void need_ws(const RConv& r, int nimg, size_t& ws_need, bool dgrad);
  int make_bn(RBN& r, const PBN& p);
  int build();
  int build_pack_table();
  void segment_range(int k, long& b, long& e) const;   // parameter range [b, e) of backward segment k

  // ---- shared by the passes (model_forward.cpp)
  static TensorIn tin(const float* p, int C, long HW);
  TensorIn frames_in(const float* x) const;   // the 3N frame-major encoder images of x [N][3][C][H][W]
  static ConvShape shape(const RConv& c, int nimg) { ConvShape s = c.s; s.N = nimg; return s; }
  void prof_conv(hipEvent_t e, const RConv& c, const ConvShape& s, const char* pass, hipStream_t st);
  int head_jobs(HeadJob* jobs, int nimg);
  double heads_flops(int nimg) const;
  TensorIn pose_pairs_in(long hw4);

  // ---- forward (model_forward.cpp)
  int conv_f(RConv& c, int nimg, const TensorIn& in, float* out, long out_bs, int act, hipStream_t st,
             const float* wp = nullptr, const float* bias = nullptr);
  int conv_f_bn(RConv& c, int nimg, const TensorIn& in, float* y, long out_bs, RBN& bn, long HW,
                hipStream_t st, int slot = 0, BNTail* tail = nullptr);
  BNStatsWs bn_ws(RBN& bn, int nimg, long HW, int slot);
  int bn_fwd(RBN& bn, const float* y, int nimg, long HW, hipStream_t st, int slot = 0);
  BNStatsIn bn_in(const RBN& bn);
  int down_fwd(EncBlock& b, int nimg, hipStream_t st);
  int encoder(const TensorIn& in, int nimg, hipStream_t st);
  int encoder_fwd(const TensorIn& in, int nimg, hipStream_t st);
  int mpi_embed(int nimg, int img0, hipStream_t st);
  int decoder_fwd(int nimg, int img0, hipStream_t st);
  int pose_fwd(hipStream_t st);
  int eval_pose(const TensorIn& in, int n, hipStream_t st);
  int forward(const float* x, hipStream_t st);
  int forward_loss(const float* x, const float* x_net, const float* automask, float* loss, float* terms,
                   hipStream_t st, const StereoIn* stereo = nullptr);

  // ---- backward (model_backward.cpp)
  int conv_w(RConv& c, int nimg, const TensorIn& in, const float* dy, hipStream_t st);
  int conv_d(RConv& c, int nimg, const float* dy, float* dx, long dx_bs, int acc, hipStream_t st,
             float* dx1 = nullptr, long dx1_bs = 0, int c0 = 1 << 30);
  int conv_wd(RConv& c, int nimg, const TensorIn& in, const float* dy, float* dx, long dx_bs, int acc,
              hipStream_t st, float* dx1 = nullptr, long dx1_bs = 0, int c0 = 1 << 30);
  int conv_w_side(RConv& c, int nimg, const TensorIn& in, const float* dy, hipEvent_t ready, hipEvent_t done,
                  hipStream_t st);
  int conv_d_bn(RConv& c, int nimg, const float* dy, float* da, long da_bs, RBN& bn, const float* y,
                long HW, float* dyprev, hipStream_t st);
  int act_bias(const float* out, const float* dout, float* dpre, int nimg, int C, long HW, int act,
               hipStream_t st, float* bp_buf = nullptr);
  BNBwd bn_bwd_desc(RBN& bn, const float* y, float* dy, bool relu_from_y);
  int bn_bwd(RBN& bn, const float* dout, const float* mask, const float* y, int nimg, long HW, float* dy,
             float* dres, int dres_acc, hipStream_t st, bool relu_from_y = false, SkipAdd sk = SkipAdd{},
             int slot = 0);
  bool skip_fused(int si) const;
  SkipAdd skip_add(int si) const;
  int block_bwd(EncBlock& b, hipStream_t st, SkipAdd sk = SkipAdd{}, bool eov = false);
  int pose_bwd(hipStream_t st);
  int seg_decoder(hipStream_t st);
  int seg_stage(int si, hipStream_t st);
  int seg_stem(hipStream_t st);
  int set_cotangents(const float* const* d_disp, const float* d_pose_in, hipStream_t st);

  // ---- test mode (model_testmode.cpp)
  int testmode_alloc();
  int refold(hipStream_t st);
  int conv_f_t(RConv& c, int nimg, const TensorIn& in, float* out, const RBN& bn, int act, hipStream_t st);
  int encoder_fwd_test(const TensorIn& in, int nimg, hipStream_t st);

  // ---- optimiser plumbing (model.cpp)
  int adam_segment(int k, float* am, float* av, float lr, float b1, float b2, float eps, float bc1,
                   float bc2, float gscale, hipStream_t st);
  int adam_join(hipStream_t st);
  int repack(hipStream_t st) { return conv_pack_batch(pack.jobs, pack.njobs, pack.blocks, st); }
};

}  // namespace md2
