// md2_depth_eval: the Monodepth2 / Eigen depth evaluation (median scaling, crop, seven error
// metrics) of a batch of disparities against ground-truth depth, on the device (include/md2.h).
//
// Nothing is compacted: every pass recomputes a pixel's (gt, pred, mask) from disp and gt through
// ONE device function, eval_pixel, so a pixel has the same bits in the selection passes and in the
// metrics pass (this file is built with -ffp-contract=off; every fused multiply-add is an explicit
// fmaf).  Passes, each one launch over all images (image index on a grid axis):
//   hist<1>, scan<1>   11-bit histogram of the top bits of gt and of pred; count, the two middle
//                      ranks and the bin that holds each
//   hist<2>, scan<2>   the next 11 bits of the keys that share a wanted prefix
//   hist<3>, scan<3>   the last 10 bits; the medians and the ratio
//   metrics            per-block partial sums of the four error sums and the three threshold counts
//   final              fixed-order fp64 combine of the partials; writes metrics and counts
// Histograms and counters use integer atomics only (order-independent); every floating-point
// reduction has a fixed order, so the result is bitwise reproducible from call to call.
#include "common.h"

#include <cmath>

namespace md2 {
namespace depth_eval {

// MSB-first radix split of an fp32 bit pattern: 11 / 11 / 10 bits
constexpr int L1_SHIFT = 21, L2_SHIFT = 10;
constexpr int NB1 = 2048, NB2 = 2048, NB3 = 1024;

// per-image histogram words (uint32).  Level 1: one histogram per key (both ranks share the
// empty prefix).  Levels 2 and 3: one per (key, rank).  key 0 = gt, key 1 = pred; rank 0 = lower
// middle element, rank 1 = upper middle element.
constexpr int H1_OFF = 0;
constexpr int H2_OFF = H1_OFF + 2 * NB1;
constexpr int H3_OFF = H2_OFF + 4 * NB2;
constexpr int HIST_WORDS = H3_OFF + 4 * NB3;   // 16384

// per-image selection state (uint32 words)
enum {
  ST_COUNT = 0,      // valid pixels
  ST_PREFIX = 1,     // [4] key*2 + rank: the bits of the wanted element decided so far
  ST_RANK = 5,       // [4] its 0-based rank among the keys that share the prefix
  ST_MED = 9,        // [2] float bits: median of gt, of pred
  ST_RATIO = 11,     // float bits
  ST_WORDS = 16
};

// per-block partial of the metrics pass: 4 fp32 sums, 3 threshold counts, 1 pad
constexpr int PART_WORDS = 8;

constexpr int MAX_GRID = 2048;        // blocks of one launch, all images together
constexpr int PIX_PER_BLOCK = 1024;   // 256 threads x 4 pixels before the grid stride starts

struct Layout {
  int gx;               // blocks per image
  size_t hist_off;      // uint32 [n][HIST_WORDS]   zeroed inside the call
  size_t nbad_off;      // uint32 [n]               zeroed inside the call (contiguous with hist)
  size_t zero_bytes;    // bytes from hist_off that the call clears
  size_t state_off;     // uint32 [n][ST_WORDS]
  size_t part_off;      // uint32/float [n][gx][PART_WORDS]
  size_t total;
};

// nullptr when cfg is valid, else the reason (no HIP call)
static const char* invalid_reason(const md2_depth_eval_cfg* c) {
  if (!c) return "depth_eval: null cfg";
  if (c->n <= 0 || c->n > 65535) return "depth_eval: n must be in 1..65535";
  if (c->h < 1 || c->w < 1 || c->gt_h < 1 || c->gt_w < 1) return "depth_eval: sizes must be at least 1";
  if ((long long)c->gt_h * c->gt_w > (1LL << 24)) return "depth_eval: gt_h * gt_w exceeds 2^24";
  if ((long long)c->h * c->w > (1LL << 30)) return "depth_eval: h * w exceeds 2^30";
  if (!(c->y0 >= 0 && c->y0 < c->y1 && c->y1 <= c->gt_h && c->x0 >= 0 && c->x0 < c->x1 && c->x1 <= c->gt_w))
    return "depth_eval: crop must be non-empty and inside the ground truth";
  if (!(c->min_depth > 0.f && c->min_depth < c->max_depth && std::isfinite(c->max_depth)))
    return "depth_eval: need 0 < min_depth < max_depth < inf";
  if (!(c->eval_min > 0.f && c->eval_min < c->eval_max && std::isfinite(c->eval_max)))
    return "depth_eval: need 0 < eval_min < eval_max < inf";
  if (!c->median_scaling && !(c->scale > 0.f && std::isfinite(c->scale)))
    return "depth_eval: scale must be positive and finite when median_scaling is 0";
  return nullptr;
}

static inline size_t a256(size_t b) { return (b + 255) & ~size_t(255); }

static Layout layout(const md2_depth_eval_cfg& c) {
  Layout L;
  const long npix = (long)(c.y1 - c.y0) * (c.x1 - c.x0);
  const int cap = MAX_GRID / c.n > 1 ? MAX_GRID / c.n : 1;
  long gx = (npix + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK;
  L.gx = (int)(gx < 1 ? 1 : (gx > cap ? cap : gx));
  L.hist_off = 0;
  L.nbad_off = L.hist_off + sizeof(uint32_t) * (size_t)c.n * HIST_WORDS;
  L.zero_bytes = L.nbad_off + sizeof(uint32_t) * (size_t)c.n - L.hist_off;
  L.state_off = a256(L.nbad_off + sizeof(uint32_t) * (size_t)c.n);
  L.part_off = a256(L.state_off + sizeof(uint32_t) * (size_t)c.n * ST_WORDS);
  L.total = a256(L.part_off + sizeof(uint32_t) * (size_t)c.n * L.gx * PART_WORDS);
  return L;
}

namespace {

struct Args {
  const float* disp;
  const float* gt;
  int h, w, Hg, Wg;
  int y0, x0, cw, npix;   // crop origin, crop width, crop pixels
  FastDiv cwdiv;
  double ry, rx;          // h / Hg, w / Wg
  int identity;           // h == Hg && w == Wg
  float a, b;             // scaled disparity = disp * a + b
  float emin, emax;
  int median_scaling;
  float scale;
  uint32_t* hist;
  uint32_t* nbad;
  uint32_t* state;
  uint32_t* part;
  int gx;
};

enum { PX_OUT = 0, PX_VALID = 1, PX_BAD = 2 };
struct Px {
  float g, p;
  int kind;
};

// THE definition of a pixel's ground truth, prediction and mask (md2.h, steps 1-3); idx counts the
// crop rectangle row by row
__device__ __forceinline__ Px eval_pixel(const Args& A, int img, int idx) {
  Px r;
  const uint32_t yy = fdiv((uint32_t)idx, A.cwdiv);
  const int Y = A.y0 + (int)yy, X = A.x0 + (idx - (int)yy * A.cw);
  r.g = A.gt[((long)img * A.Hg + Y) * A.Wg + X];
  r.p = 0.f;
  r.kind = PX_OUT;
  if (!(r.g > A.emin && r.g < A.emax)) return r;   // false for NaN
  const float* d = A.disp + (long)img * A.h * A.w;
  float sd;
  if (A.identity) {
    sd = fmaf(d[Y * A.w + X], A.a, A.b);
  } else {
    const double sy = fmin(fmax((Y + 0.5) * A.ry - 0.5, 0.0), (double)(A.h - 1));
    const double sx = fmin(fmax((X + 0.5) * A.rx - 0.5, 0.0), (double)(A.w - 1));
    const int iy0 = (int)sy, ix0 = (int)sx;        // sy, sx >= 0: truncation is floor
    const int iy1 = min(iy0 + 1, A.h - 1), ix1 = min(ix0 + 1, A.w - 1);
    const float fy = (float)(sy - (double)iy0), fx = (float)(sx - (double)ix0);
    const float v00 = fmaf(d[iy0 * A.w + ix0], A.a, A.b), v01 = fmaf(d[iy0 * A.w + ix1], A.a, A.b);
    const float v10 = fmaf(d[iy1 * A.w + ix0], A.a, A.b), v11 = fmaf(d[iy1 * A.w + ix1], A.a, A.b);
    const float top = fmaf(fx, v01 - v00, v00), bot = fmaf(fx, v11 - v10, v10);
    sd = fmaf(fy, bot - top, top);
  }
  r.p = 1.0f / sd;
  r.kind = (r.p > 0.f && r.p <= 3.402823466e38f) ? PX_VALID : PX_BAD;   // finite and positive
  return r;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int LEVEL>
struct Lvl;
template <>
struct Lvl<1> {
  static constexpr int NB = NB1, NH = 2, OFF = H1_OFF, SHIFT = L1_SHIFT, BITS = 11;
};
template <>
struct Lvl<2> {
  static constexpr int NB = NB2, NH = 4, OFF = H2_OFF, SHIFT = L2_SHIFT, UP = L1_SHIFT, BITS = 11;
};
template <>
struct Lvl<3> {
  static constexpr int NB = NB3, NH = 4, OFF = H3_OFF, SHIFT = 0, UP = L2_SHIFT, BITS = 10;
};

// Histogram of the LEVEL-th digit of the gt and pred bit patterns of the valid pixels (levels 2, 3:
// of those whose higher bits equal the prefix of a wanted rank).  Per-block LDS histogram, flushed
// with integer atomics.  Level 1 also counts the bad pixels.
template <int LEVEL>
__global__ __launch_bounds__(256) void hist_kernel(const Args A) {
  using V = Lvl<LEVEL>;
  __shared__ uint32_t lh[V::NH * V::NB];
  const int img = blockIdx.y, tid = threadIdx.x;
  const uint32_t* st = A.state + (long)img * ST_WORDS;
  uint32_t pre[4] = {0, 0, 0, 0};
  bool same[2] = {true, true};
  if (LEVEL > 1) {
    if (st[ST_COUNT] == 0) return;   // uniform over the block
#pragma unroll
    for (int q = 0; q < 4; ++q) pre[q] = st[ST_PREFIX + q];
    same[0] = pre[0] == pre[1];
    same[1] = pre[2] == pre[3];
  }
  for (int i = tid; i < V::NH * V::NB; i += 256) lh[i] = 0;
  __syncthreads();
  int bad = 0;
  for (int idx = blockIdx.x * 256 + tid; idx < A.npix; idx += gridDim.x * 256) {
    const Px q = eval_pixel(A, img, idx);
    bad += q.kind == PX_BAD;
    if (q.kind != PX_VALID) continue;
    const uint32_t key[2] = {__float_as_uint(q.g), __float_as_uint(q.p)};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if constexpr (LEVEL == 1) {
        atomicAdd(&lh[k * V::NB + (key[k] >> V::SHIFT)], 1u);
      } else {
        const uint32_t up = key[k] >> V::UP, bin = (key[k] >> V::SHIFT) & (V::NB - 1);
        if (up == pre[2 * k]) atomicAdd(&lh[(2 * k) * V::NB + bin], 1u);
        // both ranks in one bin so far: scan reads rank 1 from rank 0's histogram
        if (!same[k] && up == pre[2 * k + 1]) atomicAdd(&lh[(2 * k + 1) * V::NB + bin], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* gh = A.hist + (long)img * HIST_WORDS + V::OFF;
  for (int i = tid; i < V::NH * V::NB; i += 256) {
    const uint32_t v = lh[i];
    if (v) atomicAdd(&gh[i], v);
  }
  if (LEVEL == 1) {
    bad = wave_sum_i(bad);
    if ((tid & 63) == 0 && bad) atomicAdd(&A.nbad[img], (uint32_t)bad);
  }
}

// One block per image, one wave per (key, rank): find the bin that holds the wanted rank, extend
// its prefix and make the rank relative to that bin.  Level 3 ends with the medians and the ratio.
template <int LEVEL>
__global__ __launch_bounds__(256) void scan_kernel(const Args A) {
  using V = Lvl<LEVEL>;
  constexpr int CH = V::NB / 64;
  __shared__ uint32_t s_key[4];
  const int img = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63, k = q >> 1, r = q & 1;
  uint32_t* st = A.state + (long)img * ST_WORDS;
  const uint32_t* gh = A.hist + (long)img * HIST_WORDS + V::OFF;
  const uint32_t* hq;
  uint32_t count = 0, rank = 0, pre = 0;
  if (LEVEL == 1) {
    hq = gh + k * V::NB;
  } else {
    count = st[ST_COUNT];
    rank = st[ST_RANK + q];
    pre = st[ST_PREFIX + q];
    const bool same = st[ST_PREFIX + 2 * k] == st[ST_PREFIX + 2 * k + 1];
    hq = gh + ((r == 1 && same) ? 2 * k : q) * V::NB;
    __syncthreads();   // every wave has read the old state before any wave writes the new one
  }
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) s += hq[lane * CH + j];
  uint32_t inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  const uint32_t excl = inc - s;
  if (LEVEL == 1) {
    count = __shfl(inc, 63, 64);   // the same for gt and pred: every valid pixel has both keys
    rank = count ? (r == 0 ? (count - 1) / 2 : count / 2) : 0;
    if (q == 0 && lane == 0) st[ST_COUNT] = count;
  }
  if (count == 0) {
    if (lane == 0) {
      st[ST_PREFIX + q] = 0;
      st[ST_RANK + q] = 0;
      if (LEVEL == 3) s_key[q] = 0;
    }
  } else if (rank >= excl && rank < inc) {   // exactly one lane
    uint32_t c = excl;
    for (int j = 0; j < CH; ++j) {
      const uint32_t v = hq[lane * CH + j];
      if (rank < c + v) {
        const uint32_t np = LEVEL == 1 ? (uint32_t)(lane * CH + j)
                                       : ((pre << V::BITS) | (uint32_t)(lane * CH + j));
        st[ST_PREFIX + q] = np;
        st[ST_RANK + q] = rank - c;
        if (LEVEL == 3) s_key[q] = np;
        break;
      }
      c += v;
    }
  }
  if (LEVEL == 3) {
    __syncthreads();
    if (threadIdx.x == 0) {
      float mg = nanf(""), mp = nanf(""), ratio = nanf("");
      if (count) {
        const float gl = __uint_as_float(s_key[0]), gh_ = __uint_as_float(s_key[1]);
        const float pl = __uint_as_float(s_key[2]), ph = __uint_as_float(s_key[3]);
        mg = (count & 1) ? gl : 0.5f * (gl + gh_);
        mp = (count & 1) ? pl : 0.5f * (pl + ph);
        ratio = A.median_scaling ? mg / mp : A.scale;
      }
      st[ST_MED + 0] = __float_as_uint(mg);
      st[ST_MED + 1] = __float_as_uint(mp);
      st[ST_RATIO] = __float_as_uint(ratio);
    }
  }
}

// Error sums and threshold counts of the valid pixels: per-thread fp32 sums and integer counts,
// wave reduction by shuffles, waves combined through LDS in a fixed order, one partial per block.
__global__ __launch_bounds__(256) void metrics_kernel(const Args A) {
  __shared__ float red_f[4][4];
  __shared__ int red_i[4][3];
  const int img = blockIdx.y, tid = threadIdx.x;
  const uint32_t* st = A.state + (long)img * ST_WORDS;
  if (st[ST_COUNT] == 0) return;   // uniform over the block; final writes NaNs without the partials
  const float ratio = __uint_as_float(st[ST_RATIO]);
  float sf[4] = {0.f, 0.f, 0.f, 0.f};
  int si[3] = {0, 0, 0};
  for (int idx = blockIdx.x * 256 + tid; idx < A.npix; idx += gridDim.x * 256) {
    const Px q = eval_pixel(A, img, idx);
    if (q.kind != PX_VALID) continue;
    const float g = q.g, p = fminf(fmaxf(q.p * ratio, A.emin), A.emax);
    const float d = g - p, dl = logf(g) - logf(p), t = fmaxf(g / p, p / g);
    sf[0] += fabsf(d) / g;
    sf[1] += d * d / g;
    sf[2] += d * d;
    sf[3] += dl * dl;
    si[0] += t < 1.25f;
    si[1] += t < 1.5625f;
    si[2] += t < 1.953125f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sf[i] = wave_sum(sf[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) si[i] = wave_sum_i(si[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) red_f[tid >> 6][i] = sf[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) red_i[tid >> 6][i] = si[i];
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t* out = A.part + ((long)img * A.gx + blockIdx.x) * PART_WORDS;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      out[i] = __float_as_uint((red_f[0][i] + red_f[1][i]) + (red_f[2][i] + red_f[3][i]));
#pragma unroll
    for (int i = 0; i < 3; ++i) out[4 + i] = (uint32_t)(red_i[0][i] + red_i[1][i] + red_i[2][i] + red_i[3][i]);
  }
}

// One wave per image: the block partials in a fixed order, in fp64
__global__ __launch_bounds__(64) void final_kernel(const Args A, float* __restrict__ metrics,
                                                   int* __restrict__ counts) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const uint32_t* st = A.state + (long)img * ST_WORDS;
  const uint32_t count = st[ST_COUNT];
  float* m = metrics + (long)img * MD2_DEPTH_EVAL_NMETRIC;
  if (lane == 0) {
    counts[2 * img + 0] = (int)count;
    counts[2 * img + 1] = (int)A.nbad[img];
  }
  if (count == 0) {
    if (lane < MD2_DEPTH_EVAL_NMETRIC) m[lane] = nanf("");
    return;
  }
  double sf[4] = {0., 0., 0., 0.};
  int si[3] = {0, 0, 0};
  const uint32_t* part = A.part + (long)img * A.gx * PART_WORDS;
  for (int b = lane; b < A.gx; b += 64) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sf[i] += (double)__uint_as_float(part[b * PART_WORDS + i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) si[i] += (int)part[b * PART_WORDS + 4 + i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sf[i] = wave_sum_d(sf[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) si[i] = wave_sum_i(si[i]);
  if (lane == 0) {
    const double inv = 1.0 / (double)count;
    m[0] = (float)(sf[0] * inv);
    m[1] = (float)(sf[1] * inv);
    m[2] = (float)sqrt(sf[2] * inv);
    m[3] = (float)sqrt(sf[3] * inv);
    m[4] = (float)(si[0] * inv);
    m[5] = (float)(si[1] * inv);
    m[6] = (float)(si[2] * inv);
    m[7] = __uint_as_float(st[ST_RATIO]);
    m[8] = __uint_as_float(st[ST_MED + 0]);
    m[9] = __uint_as_float(st[ST_MED + 1]);
  }
}

}  // namespace
}  // namespace depth_eval
}  // namespace md2

using namespace md2;
using namespace md2::depth_eval;

extern "C" {

size_t md2_depth_eval_workspace_size(const md2_depth_eval_cfg* cfg) {
  if (invalid_reason(cfg)) return 0;
  return layout(*cfg).total;
}

int md2_depth_eval(const md2_depth_eval_cfg* cfg, const float* disp, const float* gt, float* metrics,
                   int* counts, void* workspace, void* stream) {
  // validation first, without a HIP call
  MD2_CHECK_ARG(cfg && disp && gt && metrics && counts && workspace, "depth_eval: null pointer");
  const char* why = invalid_reason(cfg);
  MD2_CHECK_ARG(why == nullptr, why);
  const md2_depth_eval_cfg& c = *cfg;
  const Layout L = layout(c);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;

  Args A;
  A.disp = disp;
  A.gt = gt;
  A.h = c.h;
  A.w = c.w;
  A.Hg = c.gt_h;
  A.Wg = c.gt_w;
  A.y0 = c.y0;
  A.x0 = c.x0;
  A.cw = c.x1 - c.x0;
  A.npix = (c.y1 - c.y0) * (c.x1 - c.x0);
  A.cwdiv = make_fastdiv((uint32_t)A.cw);
  A.ry = (double)c.h / (double)c.gt_h;
  A.rx = (double)c.w / (double)c.gt_w;
  A.identity = c.h == c.gt_h && c.w == c.gt_w;
  A.a = (float)(1.0 / (double)c.min_depth - 1.0 / (double)c.max_depth);
  A.b = (float)(1.0 / (double)c.max_depth);
  A.emin = c.eval_min;
  A.emax = c.eval_max;
  A.median_scaling = c.median_scaling != 0;
  A.scale = c.scale;
  A.hist = (uint32_t*)(ws + L.hist_off);
  A.nbad = (uint32_t*)(ws + L.nbad_off);
  A.state = (uint32_t*)(ws + L.state_off);
  A.part = (uint32_t*)(ws + L.part_off);
  A.gx = L.gx;

  MD2_HIP(hipMemsetAsync(ws + L.hist_off, 0, L.zero_bytes, st));
  const dim3 gpix(L.gx, c.n), gimg(c.n), blk(256);
  hipLaunchKernelGGL(hist_kernel<1>, gpix, blk, 0, st, A);
  hipLaunchKernelGGL(scan_kernel<1>, gimg, blk, 0, st, A);
  hipLaunchKernelGGL(hist_kernel<2>, gpix, blk, 0, st, A);
  hipLaunchKernelGGL(scan_kernel<2>, gimg, blk, 0, st, A);
  hipLaunchKernelGGL(hist_kernel<3>, gpix, blk, 0, st, A);
  hipLaunchKernelGGL(scan_kernel<3>, gimg, blk, 0, st, A);
  hipLaunchKernelGGL(metrics_kernel, gpix, blk, 0, st, A);
  hipLaunchKernelGGL(final_kernel, gimg, dim3(64), 0, st, A, metrics, counts);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // extern "C"
