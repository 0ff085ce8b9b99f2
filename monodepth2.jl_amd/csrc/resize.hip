// md2_resize_frames: a batch of decoded images, each of its own size, resized to one target size
// and written as float planes (and optionally N0f8 bytes).  include/md2.h states the semantics of
// both filters; the file is built with -ffp-contract=off, so every product and sum below is rounded
// on its own, in the order the header gives, and the float64 NumPy restatement of the tests and the
// host imresize of png_io.cpp get the same bits.
//
// One launch, one block per (128 output columns, 8 output rows, image):
//   weights   the block forms its tap tables in LDS once: wx[k][column] for its 128 columns, wy[j][t]
//             for its 8 rows, and the 256 values byte / 255.0.  Both filters are tap lists: imresize
//             is the two taps (i0, 1 - f), (i1, f), and top * (1 - fy) + bot * fy is the ordered sum
//             0.0 + wy_0 * top + wy_1 * bot (0.0 + a is a for a >= 0).  A tap index past the last
//             source line is the last line (imresize's clamp; antialias never produces one).
//   stage     the source rows of the band, as many as fit in 16 KB of LDS per pass, are loaded as
//             whole aligned 4-byte words: a row starts at any byte, so each row carries its own
//             0..3-byte shift.  Every word of a row segment is loaded once, by one lane.
//   stream    rows in ascending order: a thread forms the horizontal sum of its column, per channel,
//             and adds wy * sum into the accumulators of the band rows that use this source row.
//             Ascending source rows is the stated vertical order, so the accumulators ARE the result.
// No intermediate goes through memory, no atomics, no workspace: bitwise reproducible.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace md2 {
namespace resize {

constexpr int TW = 128;              // output columns per block = threads per block
constexpr int TR = 8;                // output rows per block
constexpr int STAGE_WORDS = 4096;    // 16 KB of staged source rows per pass
constexpr int MAX_SIDE = 8192;
constexpr int MAX_REDUCTION = 16;    // n_in <= 16 * n_out: at most 33 taps per axis

struct Images {
  long long off[MD2_RESIZE_MAX_IMAGES];
  int w[MD2_RESIZE_MAX_IMAGES], h[MD2_RESIZE_MAX_IMAGES];
  unsigned char flip[MD2_RESIZE_MAX_IMAGES];
};

// the taps of output index i of one axis: source lines lo .. lo + nt - 1 (clamped to n_in - 1)
struct Taps {
  int lo, nt;
  double center, fs, ww;   // antialias
  double f;                // imresize
};

// most taps an axis can have: hi - lo < 2 * fs + 1 (md2.h); imresize has two
inline int max_taps(int filter, int n_in, int n_out) {
  if (filter == MD2_RESIZE_IMRESIZE) return 2;
  const double scale = (double)n_in / (double)n_out;
  return (int)std::floor(2.0 * (scale > 1.0 ? scale : 1.0)) + 1;
}

namespace {

__device__ __forceinline__ double aa_raw(const Taps& t, int k) {
  const double d = (((double)k - t.center) + 0.5) / t.fs;
  return fmax(0.0, 1.0 - fabs(d));
}

__device__ __forceinline__ Taps make_taps(int filter, int i, int n_in, int n_out) {
  Taps t;
  if (filter == MD2_RESIZE_IMRESIZE) {
    const double sf = (double)n_in / (double)n_out;
    double p = sf * ((double)(i + 1) - 0.5) + 0.5;
    if (sf < 1.0) p = fmin(fmax(p, 1.0), (double)n_in);
    p -= 1.0;
    const int a = min((int)floor(p), n_in - 1);
    t.lo = a;
    t.nt = 2;
    t.f = p - (double)a;
    t.center = t.fs = t.ww = 0.0;
    return t;
  }
  const double scale = (double)n_in / (double)n_out;
  t.fs = fmax(scale, 1.0);
  t.center = ((double)i + 0.5) * scale;
  t.lo = max((int)((t.center - t.fs) + 0.5), 0);
  const int hi = min((int)((t.center + t.fs) + 0.5), n_in);
  t.nt = hi - t.lo;
  t.f = 0.0;
  double ww = 0.0;
  for (int k = t.lo; k < hi; ++k) ww += aa_raw(t, k);
  t.ww = ww;
  return t;
}

// the weight of tap k (0-based within the taps) -- the same bits wherever it is formed
__device__ __forceinline__ double tap_weight(int filter, const Taps& t, int k) {
  if (filter == MD2_RESIZE_IMRESIZE) return k == 0 ? 1.0 - t.f : t.f;
  return aa_raw(t, t.lo + k) / t.ww;
}

template <int C>
__global__ __launch_bounds__(TW) void resize_kernel(const Images S, const unsigned char* __restrict__ src,
                                                    float* __restrict__ out, unsigned char* __restrict__ out_u8,
                                                    int out_h, int out_w, int filter, int quantize, int ntx,
                                                    int nty) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // carve: every offset a multiple of 16
  double* lut = reinterpret_cast<double*>(smem);                 // [256]
  double* wx = lut + 256;                                        // [ntx][TW]
  double* wy = wx + (size_t)ntx * TW;                            // [TR][nty]
  int* ylo = reinterpret_cast<int*>(wy + (size_t)((TR * nty + 1) & ~1));   // [TR] first source row
  int* ynt = ylo + TR;                                           // [TR] taps
  uint32_t* stage = reinterpret_cast<uint32_t*>(ynt + TR);       // [STAGE_WORDS]
  const unsigned char* stage_b = reinterpret_cast<const unsigned char*>(stage);

  const int tid = threadIdx.x;
  const int img = blockIdx.z;
  const int w_in = S.w[img], h_in = S.h[img];
  const unsigned char* base = src + S.off[img];
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TR;
  const int x = x0 + tid;
  const bool live = x < out_w;
  const int rows = min(TR, out_h - y0);

  // ---- weights ---------------------------------------------------------------------------------
  for (int b = tid; b < 256; b += TW) lut[b] = (double)b / 255.0;
  Taps tx = make_taps(filter, live ? x : out_w - 1, w_in, out_w);
  tx.nt = min(tx.nt, ntx);   // never cuts (max_taps bounds nt); keeps the table in bounds
  for (int k = 0; k < tx.nt; ++k) wx[k * TW + tid] = tap_weight(filter, tx, k);
  if (tid < rows) {
    Taps ty = make_taps(filter, y0 + tid, h_in, out_h);
    ty.nt = min(ty.nt, nty);
    ylo[tid] = ty.lo;
    ynt[tid] = ty.nt;
    for (int t = 0; t < ty.nt; ++t) wy[tid * nty + t] = tap_weight(filter, ty, t);
  }
  // the source columns of the tile and the source rows of the band (lo and hi grow with the index)
  const Taps tfirst = make_taps(filter, x0, w_in, out_w);
  const Taps tlast = make_taps(filter, min(x0 + TW, out_w) - 1, w_in, out_w);
  const int xlo = tfirst.lo, xhi = min(tlast.lo + tlast.nt, w_in);
  const Taps bfirst = make_taps(filter, y0, h_in, out_h);
  const Taps blast = make_taps(filter, y0 + rows - 1, h_in, out_h);
  const int sy_lo = bfirst.lo, sy_hi = min(blast.lo + blast.nt, h_in);
  const int seg_bytes = (xhi - xlo) * C;
  const int row_words = (seg_bytes + 6) >> 2;           // a shift of up to 3 bytes in front
  const int rows_per_pass = STAGE_WORDS / row_words;    // >= 2 for every admitted size (host check)
  if (rows_per_pass < 1) return;                        // cannot happen; nothing is read or written
  __syncthreads();

  double acc[C][TR];
#pragma unroll
  for (int ch = 0; ch < C; ++ch)
#pragma unroll
    for (int j = 0; j < TR; ++j) acc[ch][j] = 0.0;

  const size_t pitch = (size_t)w_in * C;
  const int last_row = h_in - 1, last_col = w_in - 1;

  for (int pass_lo = sy_lo; pass_lo < sy_hi; pass_lo += rows_per_pass) {
    const int pass_n = min(rows_per_pass, sy_hi - pass_lo);
    // ---- stage ---------------------------------------------------------------------------------
    for (int r = 0; r < pass_n; ++r) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(base + (size_t)(pass_lo + r) * pitch + (size_t)xlo * C);
      const uint32_t* g = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
      const int nw = ((int)(a & 3) + seg_bytes + 3) >> 2;   // <= row_words
      for (int i = tid; i < nw; i += TW) stage[r * row_words + i] = g[i];
    }
    __syncthreads();
    // ---- stream --------------------------------------------------------------------------------
    for (int r = 0; r < pass_n; ++r) {
      const int sy = pass_lo + r;
      // block-uniform: imresize skips source rows when it reduces.  A clamped tap (lo + t past the
      // last row) reads the last row, which lies in [lo, lo + nt) as well.
      bool used = false;
#pragma unroll
      for (int j = 0; j < TR; ++j)
        if (j < rows) used = used || (sy >= ylo[j] && sy < ylo[j] + ynt[j]);
      if (!used) continue;
      const uintptr_t a = reinterpret_cast<uintptr_t>(base + (size_t)sy * pitch + (size_t)xlo * C);
      const unsigned char* row = stage_b + (size_t)r * row_words * 4 + (a & 3);
      double hsum[C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) hsum[ch] = 0.0;
      for (int k = 0; k < tx.nt; ++k) {
        const double wgt = wx[k * TW + tid];
        const unsigned char* px = row + (min(tx.lo + k, last_col) - xlo) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) hsum[ch] += wgt * lut[px[ch]];
      }
#pragma unroll
      for (int j = 0; j < TR; ++j) {
        if (j < rows) {
          const int lo = ylo[j], nt = ynt[j];
          // every tap of row j that reads source row sy, in tap order (two only at imresize's clamp)
          for (int t = max(sy - lo, 0); t < nt && min(lo + t, last_row) == sy; ++t) {
            const double wgt = wy[j * nty + t];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch][j] += wgt * hsum[ch];
          }
        }
      }
    }
    __syncthreads();   // the next pass overwrites the stage
  }

  if (!live) return;
  const int xo = S.flip[img] ? out_w - 1 - x : x;
  const size_t plane = (size_t)out_h * out_w;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const size_t o = ((size_t)img * C + ch) * plane + (size_t)y0 * out_w + xo;
#pragma unroll
    for (int j = 0; j < TR; ++j) {
      if (j < rows) {
        const double r = acc[ch][j];
        if (quantize) {
          const double q = rint(r * 255.0);   // ties to even
          out[o + (size_t)j * out_w] = __fdiv_rn((float)q, 255.0f);
          if (out_u8) out_u8[o + (size_t)j * out_w] = (unsigned char)(int)q;
        } else {
          out[o + (size_t)j * out_w] = (float)r;
        }
      }
    }
  }
}

}  // namespace
}  // namespace resize
}  // namespace md2

using namespace md2;
using namespace md2::resize;

extern "C" {

int md2_resize_frames(const md2_resize_cfg* cfg, const unsigned char* src, const long long* offsets,
                      const int* src_w, const int* src_h, const unsigned char* flip, float* out,
                      unsigned char* out_u8, void* stream) {
  // validation first, without a HIP call
  MD2_CHECK_ARG(cfg, "resize_frames: null cfg");
  MD2_CHECK_ARG(src && offsets && src_w && src_h && out, "resize_frames: null pointer");
  const md2_resize_cfg& c = *cfg;
  MD2_CHECK_ARG(c.m >= 1 && c.m <= MD2_RESIZE_MAX_IMAGES, "resize_frames: m must be in 1..64");
  MD2_CHECK_ARG(c.c == 1 || c.c == 3, "resize_frames: c must be 1 or 3");
  MD2_CHECK_ARG(c.out_h >= 1 && c.out_h <= MAX_SIDE && c.out_w >= 1 && c.out_w <= MAX_SIDE,
                "resize_frames: out_h and out_w must be in 1..8192");
  MD2_CHECK_ARG(c.filter == MD2_RESIZE_IMRESIZE || c.filter == MD2_RESIZE_ANTIALIAS,
                "resize_frames: unknown filter");
  MD2_CHECK_ARG(c.quantize == 0 || c.quantize == 1, "resize_frames: quantize must be 0 or 1");
  MD2_CHECK_ARG(!out_u8 || c.quantize, "resize_frames: out_u8 needs quantize");
  MD2_CHECK_ARG(((uintptr_t)out & 15) == 0, "resize_frames: out must be 16-byte aligned");
  Images S;
  int ntx = 2, nty = 2;
  for (int i = 0; i < c.m; ++i) {
    MD2_CHECK_ARG(offsets[i] >= 0, "resize_frames: negative offset");
    MD2_CHECK_ARG(src_w[i] >= 1 && src_w[i] <= MAX_SIDE && src_h[i] >= 1 && src_h[i] <= MAX_SIDE,
                  "resize_frames: source sizes must be in 1..8192");
    MD2_CHECK_ARG(src_w[i] <= MAX_REDUCTION * c.out_w && src_h[i] <= MAX_REDUCTION * c.out_h,
                  "resize_frames: a source side exceeds 16 times the target's");
    S.off[i] = offsets[i];
    S.w[i] = src_w[i];
    S.h[i] = src_h[i];
    S.flip[i] = flip ? (flip[i] != 0) : 0;
    ntx = std::max(ntx, max_taps(c.filter, src_w[i], c.out_w));
    nty = std::max(nty, max_taps(c.filter, src_h[i], c.out_h));
  }
  for (int i = c.m; i < MD2_RESIZE_MAX_IMAGES; ++i) {
    S.off[i] = 0;
    S.w[i] = S.h[i] = 1;
    S.flip[i] = 0;
  }
  // a staged row segment is at most (128 * 16 + 2 * 16 + 2) pixels of 3 bytes = 6.3 KB: two fit
  const size_t lds = sizeof(double) * (256 + (size_t)ntx * TW + (size_t)((TR * nty + 1) & ~1)) +
                     sizeof(int) * 2 * TR + sizeof(uint32_t) * STAGE_WORDS;   // <= 53 KB
  const dim3 grid(cdiv(c.out_w, TW), cdiv(c.out_h, TR), c.m);
  hipStream_t st = (hipStream_t)stream;
  if (c.c == 1)
    hipLaunchKernelGGL(resize_kernel<1>, grid, dim3(TW), lds, st, S, src, out, out_u8, c.out_h, c.out_w, c.filter,
                       c.quantize, ntx, nty);
  else
    hipLaunchKernelGGL(resize_kernel<3>, grid, dim3(TW), lds, st, S, src, out, out_u8, c.out_h, c.out_w, c.filter,
                       c.quantize, ntx, nty);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // extern "C"
