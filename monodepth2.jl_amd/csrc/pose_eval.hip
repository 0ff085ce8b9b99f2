// md2_pose_eval: Monodepth2's odometry metric on the device -- trajectory snippets chained from
// per-pair poses, the scale-aligned absolute trajectory error and the rotation chord of each snippet,
// and per-sequence means.  include/md2.h states the semantics operation by operation.
//
// Built with -ffp-contract=off and correctly rounded division / square root: every product and sum
// below is rounded on its own, in the order the header gives, so the float32 NumPy restatement of
// the tests gets the same bits.
//
// Passes, each over all sequences:
//   steps      (rvec, tvec) -> (R, t): so3_fwd_kernel, the kernel behind md2_so3_compose_fwd
//              (loss_kernels.hip; fp64 inside, rounded once), with one invert flag for all steps
//   snippets   one thread per snippet.  It chains its L-1 steps twice -- once for num / den, once for
//              the residual, which needs the scale -- rather than keep 2 x 16 positions in scratch:
//              at most 15 small products per chain, and the same operations give the same bits
//   sequences  one block per sequence: count, fp64 sums in a fixed order, two-pass deviation
// No atomics and no counters: the result is bitwise reproducible.  The sequence offsets travel by
// value in the kernels' arguments, so there is no copy and no host synchronisation.
#include "loss_kernels.h"

#include <cmath>

namespace md2 {
namespace pose_eval {

struct Seqs {
  int off[MD2_POSE_EVAL_MAX_SEQ + 1];    // steps: offsets <= 2^24 fit
  int soff[MD2_POSE_EVAL_MAX_SEQ + 1];   // snippets: prefix sums of max(m - L + 2, 0)
  int nseq;
};

namespace {

// (R, t) <- (R, t) o (R', t') = (R R', R t' + t), d = (R' row-major, t')
__device__ __forceinline__ void compose(float (&R)[9], float (&t)[3], const float* __restrict__ d) {
  float Rn[9], tn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (R[3 * i] * d[j] + R[3 * i + 1] * d[3 + j]) + R[3 * i + 2] * d[6 + j];
    tn[i] = ((R[3 * i] * d[9] + R[3 * i + 1] * d[10]) + R[3 * i + 2] * d[11]) + t[i];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = tn[k];
}

__device__ __forceinline__ void identity(float (&R)[9], float (&t)[3]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = (k % 4) == 0 ? 1.f : 0.f;
  t[0] = t[1] = t[2] = 0.f;
}

__global__ __launch_bounds__(256) void snippet_kernel(const Seqs S, const float* __restrict__ rt_pred,
                                                      const float* __restrict__ rt_gt, int L,
                                                      float* __restrict__ out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= S.soff[S.nseq]) return;
  int s = 0;
  while (g >= S.soff[s + 1]) ++s;   // soff[nseq] > g: stops at s < nseq; empty sequences are passed over
  const float* dp = rt_pred + (size_t)(S.off[s] + (g - S.soff[s])) * 12;   // steps i .. i+L-2, inside the sequence
  const float* dq = rt_gt + (size_t)(S.off[s] + (g - S.soff[s])) * 12;

  float Rp[9], p[3], Rq[9], q[3];
  identity(Rp, p);
  identity(Rq, q);
  float num = 0.f, den = 0.f;   // p_0 = q_0 = 0: the sums start at j = 1
  for (int j = 1; j < L; ++j) {
    compose(Rp, p, dp + (j - 1) * 12);
    compose(Rq, q, dq + (j - 1) * 12);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      num = num + q[c] * p[c];
      den = den + p[c] * p[c];
    }
  }
  float chord = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float d = Rp[k] - Rq[k];
    chord = chord + d * d;
  }
  const float scale = den > 0.f ? __fdiv_rn(num, den) : 0.f;   // false for a NaN den

  identity(Rp, p);
  identity(Rq, q);
  float res = 0.f;
  for (int j = 1; j < L; ++j) {
    compose(Rp, p, dp + (j - 1) * 12);
    compose(Rq, q, dq + (j - 1) * 12);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e = p[c] * scale - q[c];
      res = res + e * e;
    }
  }
  out[(size_t)g * 3 + 0] = __fdiv_rn(sqrtf(res), (float)L);
  out[(size_t)g * 3 + 1] = scale;
  out[(size_t)g * 3 + 2] = sqrtf(chord);
}

__device__ __forceinline__ bool finite3(float a, float b, float c) {
  return fabsf(a) <= 3.402823466e38f && fabsf(b) <= 3.402823466e38f && fabsf(c) <= 3.402823466e38f;
}

__global__ __launch_bounds__(256) void sequence_kernel(const Seqs S, const float* __restrict__ out,
                                                       float* __restrict__ summary, int* __restrict__ counts) {
  __shared__ double red[4 * 4];
  __shared__ double mean_s;
  const int s = blockIdx.x;
  const int n = S.soff[s + 1] - S.soff[s];
  const float* o = out + (size_t)S.soff[s] * 3;
  double v[4] = {0.0, 0.0, 0.0, 0.0};   // ate, scale, chord, finite snippets (exact in fp64)
  for (int i = threadIdx.x; i < n; i += 256) {
    const float a = o[3 * i], sc = o[3 * i + 1], ch = o[3 * i + 2];
    if (finite3(a, sc, ch)) {
      v[0] += (double)a;
      v[1] += (double)sc;
      v[2] += (double)ch;
      v[3] += 1.0;
    }
  }
  block_sum256_d<4>(v, red);
  if (threadIdx.x == 0) mean_s = v[3] > 0.0 ? v[0] / v[3] : 0.0;
  __syncthreads();
  const double mean = mean_s;
  double w[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += 256) {
    const float a = o[3 * i], sc = o[3 * i + 1], ch = o[3 * i + 2];
    if (finite3(a, sc, ch)) {
      const double d = (double)a - mean;
      w[0] += d * d;
    }
  }
  block_sum256_d<1>(w, red);
  if (threadIdx.x == 0) {
    const double cnt = v[3];
    const float nan = __int_as_float(0x7fc00000);
    summary[4 * s + 0] = cnt > 0.0 ? (float)(v[0] / cnt) : nan;
    summary[4 * s + 1] = cnt > 0.0 ? (float)sqrt(w[0] / cnt) : nan;
    summary[4 * s + 2] = cnt > 0.0 ? (float)(v[1] / cnt) : nan;
    summary[4 * s + 3] = cnt > 0.0 ? (float)(v[2] / cnt) : nan;
    counts[2 * s + 0] = n;
    counts[2 * s + 1] = n - (int)cnt;
  }
}

}  // namespace
}  // namespace pose_eval
}  // namespace md2

using namespace md2;
using namespace md2::pose_eval;

extern "C" {

size_t md2_pose_eval_workspace_size(long long m) {
  if (m < 0 || m > (1LL << 24)) return 0;
  return sizeof(float) * 12 * (size_t)(m > 0 ? m : 1);
}

int md2_pose_eval(const float* pred, const float* gt_rel, const long long* offsets, int nseq, int track_length,
                  int invert, float* out, float* summary, int* counts, float* rt_out, void* workspace,
                  void* stream) {
  // validation first, without a HIP call
  MD2_CHECK_ARG(offsets && summary && counts && workspace, "pose_eval: null pointer");
  MD2_CHECK_ARG(nseq >= 1 && nseq <= MD2_POSE_EVAL_MAX_SEQ, "pose_eval: nseq must be in 1..64");
  MD2_CHECK_ARG(track_length >= 2 && track_length <= MD2_POSE_EVAL_MAX_TRACK,
                "pose_eval: track_length must be in 2..16");
  MD2_CHECK_ARG(invert == 0 || invert == 1, "pose_eval: invert must be 0 or 1");
  MD2_CHECK_ARG(offsets[0] == 0, "pose_eval: offsets[0] must be 0");
  for (int i = 0; i < nseq; ++i)
    MD2_CHECK_ARG(offsets[i + 1] >= offsets[i], "pose_eval: offsets must not decrease");
  const long long M = offsets[nseq];
  MD2_CHECK_ARG(M <= (1LL << 24), "pose_eval: offsets[nseq] exceeds 2^24");
  MD2_CHECK_ARG((pred && gt_rel) || M == 0, "pose_eval: null pred or gt_rel");
  Seqs S;
  S.nseq = nseq;
  S.soff[0] = 0;
  for (int i = 0; i <= MD2_POSE_EVAL_MAX_SEQ; ++i) S.off[i] = (int)offsets[i < nseq ? i : nseq];
  for (int i = 0; i < MD2_POSE_EVAL_MAX_SEQ; ++i) {
    const int m = S.off[i + 1] - S.off[i], snip = m - track_length + 2;   // 0 past nseq
    S.soff[i + 1] = S.soff[i] + (i < nseq && snip > 0 ? snip : 0);
  }
  const int total = S.soff[nseq];
  MD2_CHECK_ARG(out || total == 0, "pose_eval: null out");

  hipStream_t st = (hipStream_t)stream;
  float* rt = rt_out ? rt_out : (float*)workspace;
  if (M > 0) MD2_TRY(launch_so3_fwd(pred, (int)M, (int)M, invert, rt, st));   // one source: bit 0 of the mask
  if (total > 0)
    hipLaunchKernelGGL(snippet_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, S, (const float*)rt, gt_rel,
                       track_length, out);
  hipLaunchKernelGGL(sequence_kernel, dim3(nseq), dim3(256), 0, st, S, (const float*)out, summary, counts);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // extern "C"
