// Non-GEMM layers of the train step, one section per translation unit: BatchNorm forward
// (bn_fwd.hip) and backward (bn_bwd.hip), max pool / x2 upsample / concat (spatial.hip), the
// MPI-mode helpers (mpi_nn.hip), the pose head (pose_head.hip), small elementwise helpers
// (elementwise.hip), ADAM (optim.hip) and the gradient guard (grad_guard.hip).
#pragma once
#include "common.h"

namespace md2 {

// ---- shared operand types ----
struct BNStatsWs {
  double* partials;   // [C][parts][2]
  int parts;
};
// Split-K slabs [splits][C][N*HW] of the conv that produced a BN input (conv_fwd / conv_dgrad
// with a SplitKDefer): the BN kernels below sum them in split order -- the conv's own reduction,
// bit-identical -- write the tensor and take its partials in the same pass (the launch-boundary
// reduce: one launch and one full read of the tensor fewer)
struct SlabIn {
  const float* slab = nullptr;
  int splits = 0;
};
// optional addend of a BN backward's dout: skip[e - lo] over flat elements [lo, hi)
struct SkipAdd {
  const float* skip = nullptr;
  long lo = 0, hi = 0;
};
// device-side form of a SkipAdd (nn_util.h skip_src)
struct SkipSrc {
  const float* skip = nullptr;
  uint32_t skip_lo = 0, skip_hi = 0;
};

// ---- bn_fwd.hip: BatchNorm, Flux train mode (batch mean / biased var, eps), per channel over
// N*HW.  bn_stats_partial writes the per-(channel, image group) fp64 partials; bn_apply_fused
// derives mean/invstd from them inside every block (one wave per channel: lane l sums partials
// l, l+64, ... in order, then the wave reduction -- the same bits in every block), applies the
// affine map (+ the downsample branch, residual, ReLU) and writes mean/invstd/running stats
// (momentum, unbiased var; when run_mean != nullptr) once per channel.
// out = act(gamma*(y-mean)*invstd + beta [+ gamma2*(y2-mean2)*invstd2 + beta2] [+ res])
struct BNStatsIn {
  const double* part = nullptr;   // [C][parts][2] from bn_stats_partial
  int parts = 0;
  float eps = 1e-5f, momentum = 0.1f;
  const float* gamma = nullptr; const float* beta = nullptr;
  float* mean = nullptr; float* invstd = nullptr;          // [C] outputs (for the backward)
  float* run_mean = nullptr; float* run_var = nullptr;     // running stats (nullable)
};
struct BNApplyFused {
  const float* y = nullptr; BNStatsIn s1;
  const float* y2 = nullptr; BNStatsIn s2;                 // downsample branch (nullable y2)
  const float* res = nullptr;
  int relu = 0;
};
int bn_parts(int C, long N, long HW);
int bn_stats_partial(const float* y, int N, int C, long HW, BNStatsWs ws, hipStream_t st);
int bn_stats_partial_slabs(SlabIn sl, float* y, int N, int C, long HW, BNStatsWs ws, hipStream_t st);
// [C][parts][2] statistics partials -> [C][1][2] (fixed order per channel), so the apply passes'
// per-block finalise reads one partial instead of `parts` (the conv epilogue's per-tile partials)
int bn_partials_collapse(const double* part, int C, int parts, double* out, hipStream_t st);
int bn_apply_fused(const BNApplyFused& p, float* out, int N, int C, long HW, hipStream_t st);
// A channel fits in one block of the one-kernel BN passes below (bn_fwd_channel, bn_bwd_channel):
// HW % 4 == 0 and N*HW/4 float4 units within a 1024-thread block's registers (8192 values).  One
// predicate, so a layer's forward and backward always agree.
bool bn_channel_fits(int N, long HW);
// Statistics + apply in one launch for such a BN: bn_stats_partial[_slabs] + bn_apply_fused with y
// read once.  The input is p.y, or sl (the conv's split-K slabs, summed in split order into y,
// which is written bit-identically to bn_stats_partial_slabs'; p.y is not read).  p.s1's partials
// are not used: the block sums the channel in fp64 in its own fixed order and finalises with
// bn_apply_fused's code (mean / invstd / running statistics stored once per channel) -- mean and
// invstd within an ulp of the two passes, not bitwise.  p.y2 / p.s2 (the downsample branch, from
// its own statistics partials), p.res and p.relu as in bn_apply_fused.
int bn_fwd_channel(SlabIn sl, float* y, const BNApplyFused& p, float* out, int N, int C, long HW,
                   hipStream_t st);
// stem tail: act = relu(BN(p.y)) (statistics finalised from p.s1's partials) and its 3x3/2/pad-1
// max pool (y, argmax) in one pass; even H, W; bit-identical to bn_apply_fused + maxpool_fwd
int bn_relu_maxpool(const BNApplyFused& p, float* act, int N, int C, int H, int W, float* y,
                    unsigned char* arg, int Ho, int Wo, hipStream_t st);

// ---- bn_bwd.hip: g = (dout [+ skip]) * (mask > 0 if mask) * (relu'(BN(y)) if mbeta);
// dbeta = sum g, dgamma = sum g*xhat; dy = gamma*invstd*(g - dbeta/L - xhat*dgamma/L)
struct BNBwd {
  const float* dout = nullptr;    // gradient of the BN output, or
  SlabIn slabs;                   // the dgrad's split-K slabs it is the sum of (split order)
  const float* mask = nullptr;    // BN(+res)+ReLU output whose ReLU gates dout (nullable)
  const float* y = nullptr;       // the BN input
  const float* mean = nullptr; const float* invstd = nullptr; const float* gamma = nullptr;
  // beta of a residual-free BN+ReLU (and mask null): the ReLU mask is re-derived from y
  // bit-exactly (bn_apply_fused's explicit roundings) instead of read back; null: no re-derivation
  const float* mbeta = nullptr;
  float* dgamma = nullptr; float* dbeta = nullptr;   // [C], written once per channel
  float* dy = nullptr;
  float* dres = nullptr;          // optional: g stored (or added, dres_accumulate) here
  int dres_accumulate = 0;
  SkipAdd skip;
};
// Two passes: the per-(channel, image group) partials of dbeta / dgamma, then bn_bwd_apply_fused,
// which sums them per block in one fixed order and applies.  bn_bwd_partial_slabs forms dout from
// b.slabs and writes it (b.dout is not read; no mask tensor / skip); the apply then reads it.
int bn_bwd_partial(const BNBwd& b, int N, int C, long HW, BNStatsWs ws, hipStream_t st);
int bn_bwd_partial_slabs(const BNBwd& b, float* dout, int N, int C, long HW, BNStatsWs ws,
                         hipStream_t st);
int bn_bwd_apply_fused(const BNBwd& b, int N, int C, long HW, BNStatsWs ws, hipStream_t st);
// The whole backward in one launch for a BN whose channel fits in a block (bn_channel_fits):
// partial sums, dgamma/dbeta and the apply, each tensor read once.  b.dout, or b.slabs (then no
// mask / skip, and nothing but dy and dgamma/dbeta is written).  The fp64 sums run in the block's
// own fixed order: last-bit differences to the two passes at most.
int bn_bwd_channel(const BNBwd& b, int N, int C, long HW, hipStream_t st);

// ---- spatial.hip: MaxPool((3,3); stride 2, pad 1) ----
int maxpool_fwd(const float* x, int N, int C, int H, int W, float* y, unsigned char* arg,
                int Ho, int Wo, hipStream_t st);
// optional skip: dx += skip over whole images (the decoder skip gradient; even W)
int maxpool_bwd(const float* dy, const unsigned char* arg, int N, int C, int H, int W, int Ho,
                int Wo, float* dx, hipStream_t st, SkipAdd skip = SkipAdd{});
// upsample_bilinear(x, (2,2)), align_corners = true
int upsample2_fwd(const float* x, int N, int C, int h, int w, float* y, hipStream_t st);
int upsample2_bwd(const float* dy, int N, int C, int h, int w, float* dx, hipStream_t st);
// channel concatenation cat(a, b; dims=3) of [N][ca][hw] and [N][cb][hw]
int concat_channels(const float* a, int ca, const float* b, int cb, int N, long hw, float* out,
                    hipStream_t st);

// ---- mpi_nn.hip ----
// MPI-mode decoder input (src/model.jl:39-50): out[(b*P + p)][0:C] = feat[b], out[..][C + e] =
// embed(bins[b][p])[e] broadcast over h x w (e < 2L+1: x, sin(2^i x), cos(2^i x))
// Ctot: channels per output image (>= C + 2L + 1; the channels past C + 2L + 1 are written as
// zeros -- the executor's padded layout); 0 = C + 2L + 1
int mpi_embed_features(const float* feat, long sample_stride, int N, int C, int h, int w,
                       const float* bins, int P, int L, float* out, hipStream_t st, int Ctot = 0);
// the _repeat pullback (src/repeat.jl:44-53): out[b][c] (+)= sum_p in[b*P + p][c] for c < C of the
// Cin channels per image
int plane_sum(const float* in, int N, int P, int Cin, int C, long hw, float* out, int accumulate,
              hipStream_t st);
// dst[r*P + p][:] = src[r][:] for a [rows][cols] matrix, and its adjoint dst[r] = sum_p src[r*P + p]
int repeat_rows(const float* src, long rows, int cols, int P, float* dst, hipStream_t st);
int repeat_rows_adjoint(const float* src, long rows, int cols, int P, float* dst, hipStream_t st);

// ---- pose_head.hip: pose[q][k] = 0.01 * (b[k] + sum_c W[k][c] * mean_hw(x[q][c])) ----
int pose_head_fwd(const float* x, int Q, int C, long HW, const float* w, const float* b,
                  float* means, float* pose, hipStream_t st);
int pose_head_bwd(const float* dpose, int Q, int C, long HW, const float* w, const float* means,
                  float* dx, float* dw, float* db, hipStream_t st);
// pose pairs (a_j, b_j) of frames: PoseDecoder input gather / its gradient scatter
int pair_gather(const float* sq, int N, int C, long HW, const int a[2], const int b[2], float* pin,
                hipStream_t st);
int pair_grad_gather(const float* dpin, int N, int C, long HW, const int a[2], const int b[2],
                     float* dsq, hipStream_t st);

// ---- elementwise.hip ----
int axpy(float* y, const float* x, long n, hipStream_t st);               // y += x
int scale_inplace(float* x, long n, float s, hipStream_t st);             // x *= s
// out = g .* (s .* (1 - s)) (g == nullptr: 0), the sigmoid head's pullback
int sigmoid_cotangent(const float* g, const float* s, float* out, long n, hipStream_t st);
// [planes][kh][kw] with both spatial axes reversed (Flux true-convolution <-> cross-correlation)
int flip_taps(const float* src, float* dst, long planes, int kh, int kw, hipStream_t st);

// ---- optim.hip: Flux ADAM over the flat parameter vector ----
int adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
              float eps, float bc1, float bc2, float gscale, hipStream_t st);
// graph-replayable ADAM: *step += 1 and bc = (1 - b1^t, 1 - b2^t) on the device, then the update
int adam_prep(int* step, float* bc, float b1, float b2, hipStream_t st);
int set_device_int(int* p, int v, hipStream_t st);
int adam_step_dev(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                  float eps, const float* bc, float gscale, hipStream_t st);
// adam_step / adam_step_dev with gscale and the verdict read from *gs (the guarded step, md2.h)
int adam_step_guarded(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                      float eps, float bc1, float bc2, const md2_guard_state* gs, hipStream_t st);
int adam_step_dev_guarded(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                          float eps, const float* bc, const md2_guard_state* gs, hipStream_t st);

// ---- grad_guard.hip (md2.h, md2_grad_norm): writes the state the guarded steps read ----
size_t grad_norm_workspace_bytes(long long n);   // 0 for n outside 1..2^31
// the two launches; arguments validated by the caller
int grad_norm(const float* g, long long n, float grad_scale, float max_norm, md2_guard_state* state,
              void* workspace, hipStream_t st);

}  // namespace md2
