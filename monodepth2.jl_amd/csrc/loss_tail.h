// Host orchestration of the loss tail: composeT -> per scale {mean, warp+SSIM, smoothness,
// upsample adjoint} -> deterministic reductions -> composeT/so3 backward.  One body runs both
// entry points below; they differ in where the sources come from and in the photometric kernel.
#pragma once
#include "loss_kernels.h"

namespace md2 {

struct LossTailCfg {
  int N, C, W, H;             // samples, channels, target resolution
  int nscales;
  int dw[MAX_SCALES], dh[MAX_SCALES];
  float smooth_w[MAX_SCALES]; // forward weight of the smooth term (train_loss: smoothness*scale)
  float divisor;              // train_loss: nscales (src/training.jl:77); slow_depth: 1
  int smooth_normalize;       // divide the disparity by its per-image mean (training.jl:64-65)
  float K[9], invK[9];
  float min_depth, max_depth;
  long x_sample_stride, x_frame_stride;
  int target, src0, src1;     // 0-based frame indices
  int invert_mask;            // bit s: source s uses the inverse transform (src < target)
  int sigmoid_grad;           // 1: d_disp is w.r.t. the head pre-activation (s(1-s) fused)
};

constexpr int MEAN_PARTS = 64;

size_t loss_tail_workspace_bytes(const LossTailCfg& c);

struct LossTailOut {
  float* loss;
  float* terms;
  float* d_disp[MAX_SCALES];
  float* d_pose;
  float* vis_loss;
  signed char* vis_sel;
  float* vis_warped;                    // [nsrc][N][C][H][W] warped sources at the last scale or nullptr
  int* vis_cell;                        // [nscales][nsrc][N][H][W] bilinear cells (diagnostics) or nullptr
  hipEvent_t* photo_events = nullptr;   // optional [2]: around the (all-scale) photometric launch
};

// Two learned sources, frames c.src0 / c.src1 of x with pose blocks 0 and 1, on the packed
// two-source photometric kernel (photo.hip).  disp[s]: [N][dh][dw] sigmoid outputs; pose: [2N][6]
// (rvec, tvec) per (source, sample); x: frames; automask: [N][H][W] or nullptr.  dloss: upstream
// scalar gradient.
int loss_tail_run(const LossTailCfg& c, const float* const* disp, const float* pose,
                  const float* x, const float* automask, float dloss, const LossTailOut& o,
                  void* workspace, hipStream_t st);

// The loss tail over 1..MAX_SOURCES sources, each LEARNED (its pose comes from the pose network
// and gets a gradient) or FIXED (a caller-supplied transform, data), on the photometric kernel over
// sources (photo_sources.hip), nsrc = 2 included.  c.target / src0 / src1 / invert_mask /
// x_*_stride are not read.
struct LossSource {
  const float* frames;        // sample i's [C][H][W] frame at frames + i * sample_stride
  long sample_stride;
  int pose_block;             // >= 0: learned, poses at rows pose[pose_block * N + i]; -1: fixed
  int invert;                 // learned: composeT's inverse transform
  const float* Rt;            // fixed: device [N][12] (R row-major, t)
};
size_t loss_tail_sources_workspace_bytes(const LossTailCfg& c, int nsrc);
// pose: [n_learned * N][6] (may be nullptr without learned sources); o.d_pose [n_learned * N][6],
// rows as in pose; o.vis_warped [nsrc][N][C][H][W]; o.vis_cell [nscales][nsrc][N][H][W];
// o.vis_sel holds 0..nsrc-1 or -1.  The learned sources' pose blocks must be 0..n_learned-1, each
// once; with the learned sources first and in block order composeT writes and reads Rt / dRt in
// place, any other order stages its rows through copies.
// Kn / invKn: per-sample intrinsics, device [N][9] each (row-major, read only), both or neither.
// Set, sample i is warped by Kn + 9 i / invKn + 9 i and c.K / c.invK are not read; rows all equal
// to c.K / c.invK give the bits of the call without them.
int loss_tail_sources_run(const LossTailCfg& c, int nsrc, const LossSource* src, const float* target,
                          long target_sample_stride, const float* const* disp, const float* pose,
                          const float* automask, float dloss, const LossTailOut& o, void* workspace,
                          hipStream_t st, const float* Kn = nullptr, const float* invKn = nullptr);

// Op-level per-scale warp + photometric loss (md2_warp_photometric_*).
struct WarpOpCfg {
  int N, C, W, H, dw, dh;
  float K[9], invK[9];
  float min_depth, max_depth;
  long x_sample_stride, x_frame_stride;
  int target, src0, src1;
};
size_t warp_op_workspace_bytes(int N, int W, int H);
// d_loss == nullptr: forward only (loss_map / sel_map); else also the pullback of sum(d_loss .*
// warp_loss) into d_disp [N][dh][dw] and d_Rt [2N][12] (each optional).
int warp_op_run(const WarpOpCfg& c, const float* disp, const float* Rt, const float* x,
                const float* automask, const float* d_loss, float* loss_map, signed char* sel_map,
                float* d_disp, float* d_Rt, void* workspace, hipStream_t st);

}  // namespace md2
