// BatchNorm test mode (Flux testmode!): with fixed running statistics a BatchNorm is the
// per-channel affine map y*s + t, s = gamma / sqrt(var + eps), t = beta - mean*s.  The encoder's
// convs take it into their weights (w' = w*s, bias t); what is left of the normalisation layers is
// the stem's affine + ReLU + max pool and the residual add of a block's tail.
#pragma once
#include "common.h"

namespace md2 {

// Flat layout of the running statistics (md2_model_get_bn_stats): BatchNorm k owns
// [off[k], off[k+1]) = C means then C variances, in the order of the gamma entries of the
// parameter table.
constexpr int MAX_BN = 64;
struct BNStatLayout {
  int n = 0;
  int off[MAX_BN + 1] = {};
};
// *flag (device int, zeroed by the caller) = 1 when a variance is negative or any entry is not
// finite; nothing is copied to the host
int bn_stats_validate(const float* stats, const BNStatLayout& L, int* flag, hipStream_t st);

// One fold of a BatchNorm into the conv before it.  w == nullptr: the statistics only (the stem,
// whose space-to-depth conv kernel takes no bias: its (s, t) go to affine_relu_maxpool).
struct FoldJob {
  const float* w = nullptr;   // [Cout][per] conv weights (per = Cin*KH*KW, a multiple of 4)
  float* wf = nullptr;        // folded copy, same layout
  const float* gamma = nullptr; const float* beta = nullptr;
  const float* mean = nullptr; const float* var = nullptr;   // running statistics [Cout]
  float* s = nullptr; float* t = nullptr;                    // [Cout] outputs
  int Cout = 0;
  int per4 = 0;               // per / 4
  long block_begin = 0;       // first block of this job in the batched grid
};
long bn_fold_job_blocks(const FoldJob& j);
// every fold of a model in ONE launch over a device-resident job table: s and t formed in fp64 and
// rounded once, wf[co][:] = w[co][:] * s[co]
int bn_fold_batch(const FoldJob* dev_jobs, int njobs, long total_blocks, double eps, hipStream_t st);

// stem tail in test mode: act = relu(y*s[c] + t[c]) (the decoder skip) and pool = its 3x3/2/pad-1
// max pool, one pass, no argmax.  y, act [N][C][H][W]; pool [N][C][H/2][W/2]; H even, W % 4 == 0
int affine_relu_maxpool(const float* y, const float* s, const float* t, int N, int C, int H, int W,
                        float* act, float* pool, hipStream_t st);
// block tail in test mode: out = relu(a + b) over n elements (n % 4 == 0, 16-byte aligned)
int add_relu(const float* a, const float* b, float* out, long n, hipStream_t st);

}  // namespace md2
