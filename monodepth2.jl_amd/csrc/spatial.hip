// Spatial resampling layers (nn.h): the stem max pool, the x2 bilinear upsample (forward and its
// two backward forms) and the channel concat.  HBM-bound streaming kernels.
#include "nn_util.h"

namespace md2 {

// ---------------------------------------------------------------------------------------------
// MaxPool 3x3 / stride 2 / pad 1 (ResNet stem); argmax kept as the window index 0..8
// ---------------------------------------------------------------------------------------------
// one output per thread; with an even input width the window columns 2ow, 2ow+1 are one float2
template <bool EVENW>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, int H, int W,
                                                          float* __restrict__ y,
                                                          unsigned char* __restrict__ arg, int Ho,
                                                          FastDiv fdWo, FastDiv fdHo, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = fdiv(i, fdWo), plane = fdiv(r, fdHo);
  const int ow = (int)(i - r * fdWo.d), oh = (int)(r - plane * fdHo.d);
  const float* p = x + plane * (uint32_t)(H * W);
  float best = -INFINITY;
  int bi = 0;
  const int iw = ow * 2;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = oh * 2 - 1 + kh;
    if (ih < 0 || ih >= H) continue;
    const float* row = p + ih * W;
    float v0 = -INFINITY, v1, v2 = -INFINITY;
    if (iw > 0) v0 = row[iw - 1];
    if (EVENW) {
      const float2 t = *reinterpret_cast<const float2*>(row + iw);
      v1 = t.x;
      v2 = t.y;
    } else {
      v1 = row[iw];
      if (iw + 1 < W) v2 = row[iw + 1];
    }
    // strict '>' in (kh, kw) scan order: the first maximum wins (NNlib maxpool)
    if (v0 > best) { best = v0; bi = kh * 3; }
    if (v1 > best) { best = v1; bi = kh * 3 + 1; }
    if (v2 > best) { best = v2; bi = kh * 3 + 2; }
  }
  y[i] = best;
  arg[i] = (unsigned char)bi;
}

// Gather over 2x2 input blocks: input rows {2i, 2i+1} x columns {2j, 2j+1} are touched only by
// outputs (i..i+1, j..j+1) -- even rows/columns are tap 1 of output i, odd ones tap 2 of output
// i and tap 0 of output i+1 -- so each thread reads 4 (arg, dy) pairs and writes 4 inputs.
// SKIP (even W): dx += skip over flat elements [sk.skip_lo, sk.skip_hi) -- the decoder skip
// gradient on the target images, added here instead of by a separate axpy (same fp add)
template <bool EVENW, bool SKIP = false>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy,
                                                          const unsigned char* __restrict__ arg,
                                                          int H, int W, int Ho, FastDiv fdWo,
                                                          FastDiv fdHo, float* __restrict__ dx,
                                                          uint32_t n, SkipSrc sk = SkipSrc{}) {
  static_assert(!SKIP || EVENW, "SKIP: even width");
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const uint32_t r = fdiv(t, fdWo), plane = fdiv(r, fdHo);
  const int Wo = (int)fdWo.d;
  const int j = (int)(t - r * fdWo.d), i = (int)(r - plane * fdHo.d);
  const bool hasr = i + 1 < Ho, hasc = j + 1 < Wo;
  const uint32_t o = t;
  const int a00 = arg[o];
  const float g00 = dy[o];
  int a01 = -1, a10 = -1, a11 = -1;
  float g01 = 0.f, g10 = 0.f, g11 = 0.f;
  if (hasc) { a01 = arg[o + 1]; g01 = dy[o + 1]; }
  if (hasr) { a10 = arg[o + Wo]; g10 = dy[o + Wo]; }
  if (hasr && hasc) { a11 = arg[o + Wo + 1]; g11 = dy[o + Wo + 1]; }
  const float e00 = a00 == 4 ? g00 : 0.f;
  const float e01 = (a00 == 5 ? g00 : 0.f) + (a01 == 3 ? g01 : 0.f);
  const float e10 = (a00 == 7 ? g00 : 0.f) + (a10 == 1 ? g10 : 0.f);
  const float e11 = (a00 == 8 ? g00 : 0.f) + (a01 == 6 ? g01 : 0.f) + (a10 == 2 ? g10 : 0.f) +
                    (a11 == 0 ? g11 : 0.f);
  const uint32_t qi = plane * (uint32_t)(H * W) + (2 * i) * W + 2 * j;
  float* q = dx + qi;
  if (EVENW) {
    float2 r0 = make_float2(e00, e01), r1 = make_float2(e10, e11);
    if (SKIP && qi >= sk.skip_lo && qi < sk.skip_hi) {   // image-uniform: both rows in range
      const float2 k0 = *reinterpret_cast<const float2*>(sk.skip + (qi - sk.skip_lo));
      r0.x += k0.x; r0.y += k0.y;
      if (2 * i + 1 < H) {
        const float2 k1 = *reinterpret_cast<const float2*>(sk.skip + (qi + W - sk.skip_lo));
        r1.x += k1.x; r1.y += k1.y;
      }
    }
    *reinterpret_cast<float2*>(q) = r0;
    if (2 * i + 1 < H) *reinterpret_cast<float2*>(q + W) = r1;
  } else {
    q[0] = e00;
    if (2 * j + 1 < W) q[1] = e01;
    if (2 * i + 1 < H) {
      q[W] = e10;
      if (2 * j + 1 < W) q[W + 1] = e11;
    }
  }
}

int maxpool_fwd(const float* x, int N, int C, int H, int W, float* y, unsigned char* arg, int Ho,
                int Wo, hipStream_t st) {
  const long n = (long)N * C * Ho * Wo;
  MD2_TRY(check_u31((long)N * C * H * W));
  if (W % 2 == 0)
    hipLaunchKernelGGL(maxpool_fwd_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, st, x, H, W, y,
                       arg, Ho, fd(Wo), fd(Ho), (uint32_t)n);
  else
    hipLaunchKernelGGL(maxpool_fwd_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, st, x, H, W, y,
                       arg, Ho, fd(Wo), fd(Ho), (uint32_t)n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int maxpool_bwd(const float* dy, const unsigned char* arg, int N, int C, int H, int W, int Ho,
                int Wo, float* dx, hipStream_t st, SkipAdd skip) {
  MD2_CHECK_ARG(Ho == (H + 1) / 2 && Wo == (W + 1) / 2, "maxpool_bwd: 3x3/2 pad-1 output shape");
  const long n = (long)N * C * Ho * Wo;
  MD2_TRY(check_u31((long)N * C * H * W));
  MD2_CHECK_ARG(!skip.skip || (W % 2 == 0 && skip.lo >= 0 && skip.lo <= skip.hi &&
                               skip.hi <= (long)N * C * H * W && skip.lo % ((long)H * W) == 0 &&
                               skip.hi % ((long)H * W) == 0),
                "maxpool_bwd: skip range (whole images, even W)");
  if (skip.skip)
    hipLaunchKernelGGL((maxpool_bwd_kernel<true, true>), dim3(cdiv(n, 256)), dim3(256), 0, st, dy, arg, H,
                       W, Ho, fd(Wo), fd(Ho), dx, (uint32_t)n, skip_src(skip));
  else if (W % 2 == 0)
    hipLaunchKernelGGL(maxpool_bwd_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, st, dy, arg, H,
                       W, Ho, fd(Wo), fd(Ho), dx, (uint32_t)n);
  else
    hipLaunchKernelGGL(maxpool_bwd_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, st, dy, arg, H,
                       W, Ho, fd(Wo), fd(Ho), dx, (uint32_t)n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// ---------------------------------------------------------------------------------------------
// upsample_bilinear(x, (2,2)) with align_corners = true (src/depth_decoder.jl:18-19)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void src_idx(int o, float r, int in, int& i0, int& i1, float& f) {
  const float s = r * (float)o;
  i0 = min((int)s, in - 1);
  i1 = min(i0 + 1, in - 1);
  f = s - (float)i0;
}

__global__ __launch_bounds__(256) void upsample2_fwd_kernel(const float* __restrict__ x, int h,
                                                            int w, float ry, float rx, FastDiv fdW2,
                                                            FastDiv fdH2, float* __restrict__ y,
                                                            uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = fdiv(i, fdW2), plane = fdiv(r, fdH2);
  const int ox = (int)(i - r * fdW2.d), oy = (int)(r - plane * fdH2.d);
  const float* p = x + (long)plane * h * w;
  int y0, y1, x0, x1;
  float fy, fx;
  src_idx(oy, ry, h, y0, y1, fy);
  src_idx(ox, rx, w, x0, x1, fx);
  y[i] = (1.f - fy) * ((1.f - fx) * p[y0 * w + x0] + fx * p[y0 * w + x1]) +
         fy * ((1.f - fx) * p[y1 * w + x0] + fx * p[y1 * w + x1]);
}

// Adjoint as a gather.  For the x2 align-corners map s = r*o, r = (n-1)/(2n-1), 1/r = 2+1/(n-1):
// input i receives from outputs with floor(s) in {i-1, i}, i.e. o in [2i-2, 2i+3] (r*o is never
// within float rounding of an integer except at the end points, which stay inside the range).
// The six per-axis weights are computed once, with the forward's exact float arithmetic.
__device__ __forceinline__ void up_adj_weights(int i, float r, int in, int out, int& o0,
                                               float wv[6]) {
  o0 = 2 * i - 2;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int o = o0 + q;
    float wq = 0.f;
    if (o >= 0 && o < out) {
      int i0, i1;
      float f;
      src_idx(o, r, in, i0, i1, f);
      wq = (i0 == i ? 1.f - f : 0.f) + (i1 == i ? f : 0.f);
    }
    wv[q] = wq;
  }
}

__global__ __launch_bounds__(256) void upsample2_bwd_kernel(const float* __restrict__ dy, int h,
                                                            int w, float ry, float rx, FastDiv fdw,
                                                            FastDiv fdh, float* __restrict__ dx,
                                                            uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int W2 = 2 * w, H2 = 2 * h;
  const uint32_t r = fdiv(i, fdw), plane = fdiv(r, fdh);
  const int ix = (int)(i - r * fdw.d), iy = (int)(r - plane * fdh.d);
  const float* g = dy + plane * (uint32_t)(H2 * W2);
  int oy0, ox0;
  float wy[6], wx[6];
  up_adj_weights(iy, ry, h, H2, oy0, wy);
  up_adj_weights(ix, rx, w, W2, ox0, wx);
  // explicit fmas (the tiled kernel's order and roundings; a skipped zero weight is an exact
  // fma(0, x, acc) = acc there)
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    if (wy[a] == 0.f) continue;
    const float* row = g + (oy0 + a) * W2;
    float acc = 0.f;
#pragma unroll
    for (int b = 0; b < 6; ++b)
      if (wx[b] != 0.f) acc = fmaf(wx[b], row[ox0 + b], acc);
    s = fmaf(wy[a], acc, s);
  }
  dx[i] = s;
}

// Tiled adjoint over the STACKED planes: the N*C input planes of h rows are one (N*C*h) x w
// image, and input row r (plane r / h, local row r % h) reads output rows 2r-2 .. 2r+3 of the
// equally stacked (N*C*2h) x 2w gradient, whatever plane they belong to -- an output row of a
// neighbouring plane gets weight 0 from up_adj_weights (local index outside [0, 2h)), so a tile
// may straddle planes and the small coarse levels (13 x 4 planes) fill whole blocks.  A block of
// TW x (RPT * 256 / TW) input pixels stages its (2 TH + 4) x (2 TW + 4) output window in LDS with
// every thread's loads issued before any LDS store, then each thread contracts RPT vertically
// adjacent input pixels of one column (its six column weights computed once) from LDS with the
// same weights and the same summation order as upsample2_bwd_kernel (bit-identical).  RPT = 4
// (round 6): a quarter of the blocks, 4x the loads in flight per block and 4.5 instead of 5.3
// staged floats per input pixel -- the one-row tiles were latency-bound (~1 TB/s).
template <int TW, int RPT>
__global__ __launch_bounds__(256) void upsample2_bwd_tile_kernel(const float* __restrict__ dy, int h,
                                                                 int w, long rows, float ry, float rx,
                                                                 float* __restrict__ dx) {
  constexpr int TY = 256 / TW, TH = TY * RPT, FR = 2 * TH + 4, FC = 2 * TW + 4;
  constexpr int NL = (FR * FC + 255) / 256;
  __shared__ float t[FR][FC + 1];
  const int W2 = 2 * w;
  const int ix0 = blockIdx.x * TW;
  const long r0 = (long)blockIdx.y * TH;
  const long oyb = 2 * r0 - 2, orows = 2 * rows;
  const int oxb = 2 * ix0 - 2;
  float v[NL];
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    const int e = threadIdx.x + 256 * q;
    const int r = e / FC, c = e - r * FC;
    const long oy = oyb + r;
    const int ox = oxb + c;
    v[q] = (e < FR * FC && oy >= 0 && oy < orows && ox >= 0 && ox < W2) ? dy[oy * W2 + ox] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    const int e = threadIdx.x + 256 * q;
    const int r = e / FC, c = e - r * FC;
    if (e < FR * FC) t[r][c] = v[q];
  }
  __syncthreads();
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const int ix = ix0 + tx;
  if (ix >= w) return;
  int ox0;
  float wx[6];
  up_adj_weights(ix, rx, w, W2, ox0, wx);
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int ly = ty * RPT + k;
    const long row = r0 + ly;
    if (row >= rows) break;
    const int iy = (int)(row % h);
    int oy0;
    float wy[6];
    up_adj_weights(iy, ry, h, 2 * h, oy0, wy);
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      float acc = 0.f;
#pragma unroll
      for (int b = 0; b < 6; ++b) acc = fmaf(wx[b], t[2 * ly + a][2 * tx + b], acc);
      s = fmaf(wy[a], acc, s);
    }
    dx[row * w + ix] = s;
  }
}

static inline float up_ratio(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

int upsample2_fwd(const float* x, int N, int C, int h, int w, float* y, hipStream_t st) {
  const long n = (long)N * C * 4 * h * w;
  MD2_TRY(check_u31(n));
  hipLaunchKernelGGL(upsample2_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, h, w,
                     up_ratio(h, 2 * h), up_ratio(w, 2 * w), fd(2 * w), fd(2 * h), y, (uint32_t)n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int upsample2_bwd(const float* dy, int N, int C, int h, int w, float* dx, hipStream_t st) {
  const long n = (long)N * C * h * w;
  MD2_TRY(check_u31(4 * n));
  static const int tiled = tuning_knob("MD2_UP_TILED", 1);
  const long rows = (long)N * C * h;
  if (tiled && w > 16 && cdiv(rows, 32) <= 65535)
    hipLaunchKernelGGL((upsample2_bwd_tile_kernel<32, 4>), dim3(cdiv(w, 32), cdiv(rows, 32)), dim3(256), 0, st, dy,
                       h, w, rows, up_ratio(h, 2 * h), up_ratio(w, 2 * w), dx);
  else if (tiled && cdiv(rows, 16) <= 65535)   // (4 rows per thread: 13.7 vs 10.3 us on the 4x13 maps)
    hipLaunchKernelGGL((upsample2_bwd_tile_kernel<16, 1>), dim3(cdiv(w, 16), cdiv(rows, 16)), dim3(256), 0, st, dy,
                       h, w, rows, up_ratio(h, 2 * h), up_ratio(w, 2 * w), dx);
  else
    hipLaunchKernelGGL(upsample2_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dy, h, w,
                       up_ratio(h, 2 * h), up_ratio(w, 2 * w), fd(w), fd(h), dx, (uint32_t)n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// ---------------------------------------------------------------------------------------------
// channel concatenation cat(a, b; dims=3)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void concat_kernel(const float* __restrict__ a, int ca,
                                                     const float* __restrict__ b, int cb, long hw,
                                                     float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long px = i % hw, t = i / hw;
  const int c = (int)(t % (ca + cb));
  const long img = t / (ca + cb);
  out[i] = c < ca ? a[(img * ca + c) * hw + px] : b[(img * cb + (c - ca)) * hw + px];
}

int concat_channels(const float* a, int ca, const float* b, int cb, int N, long hw, float* out,
                    hipStream_t st) {
  const long n = (long)N * (ca + cb) * hw;
  MD2_TRY(check_u31(n));
  hipLaunchKernelGGL(concat_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a, ca, b, cb, hw, out, n);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
