// Implicit-GEMM convolution kernels for gfx950 (see conv.h).  Compiled as four translation units
// (conv.hip: packing/planning/workspaces, conv_fwd.hip, conv_dgrad.hip, conv_wgrad.hip) selected by
// MD2_CONV_PART so the template instantiations of the three passes build in parallel.
//
// All three passes are one GEMM shape  C[M][N] = sum_k A[k][m] * B[k][n]  computed with the
// exact-fp32 MFMA v_mfma_f32_32x32x2_f32 (64 lanes: A[i=l&31][k=l>>5], B[k=l>>5][j=l&31]; C/D:
// col j = lane&31, row i = (r&3) + 8(r>>2) + 4(lane>>5)).  The N (lane) dimension is always the
// pixel or filter-column axis, so every epilogue store writes 32 consecutive floats per register.
//
//   forward : M = Cout, N = images*Ho*Wo,  K = Cin*KH*KW     A = packed W^T,  B = im2col(x)
//   dgrad   : M = Cin,  N = images*H*W,    K = Cout*KH*KW    A = packed W,    B = gather(dY)
//   wgrad   : M = Cout, N = Cin*KH*KW,     K = images*Ho*Wo  A = dY^T,        B = im2col(x)^T
//
// Tiles are staged global -> registers -> LDS (double buffered, one barrier per K step); the
// im2col / gather address maths runs on SALU (wave-uniform k decode) and VALU in the shadow of
// the 64-cycle f32 MFMAs.  Small-M / huge-K shapes (layer4, wgrad) use split-K slabs reduced by
// a second kernel that also applies the epilogue (deterministic, no atomics).
#include <type_traits>

#include "conv.h"
#include "conv_lds.h"
#include "head.h"

namespace md2 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KPAD = 32;    // packed weight K padding
constexpr int MPAD = 128;   // packed weight M padding

static inline long round_up(long a, long b) { return (a + b - 1) / b * b; }

__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(v, 0.f);
    case ACT_ELU: return v > 0.f ? v : expm1f(v);
    case ACT_SIGMOID: return 1.f / (1.f + expf(-v));
    default: return v;
  }
}

// exact three-way bf16 split of an fp32 value (conv_px3.inc): bit patterns with the bf16 in the
// high half; x == hi + mid + lo exactly for every x of normal magnitude (the tail below 2^-126 of
// a remainder is truncated)
__device__ __forceinline__ void split3(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = __float_as_uint(x) & 0xffff0000u;
  const float r1 = x - __uint_as_float(h);
  m = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(m);
  l = __float_as_uint(r2) & 0xffff0000u;
}

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
// forward:  Wt[k][m] = W[m][c][tap]   ([Kpad][Mpad]);   dgrad: Wd[k][ci] = W[co][ci][tap]
// ([Kdpad][Cinpad]); k = tap*C + c (tap-major) or c*KK + tap, C = Cin (forward) / Cout (dgrad)
#if MD2_CONV_PART == 0
struct PackOne {
  const float* w;
  float* out;
  int mode, tap, layout, Cout, Cin, KK, Kpad, Mpad;
  int Cinw;   // the weights' Cin (<= Cin)
};

__device__ __forceinline__ long packed_index(int k, int m, int layout, int Mpad) {
  return layout ? ((long)(k >> 4) * Mpad + m) * 16 + (k & 15) : (long)k * Mpad + m;
}
// layout 2 (conv_px3): [K/16][3 parts][Mpad][16] bf16, the three exact split terms of W
__device__ __forceinline__ void pack_store(float* out, int k, int m, int layout, int Mpad, float v) {
  if (layout == 2) {
    uint16_t* o = reinterpret_cast<uint16_t*>(out);
    uint32_t h, md, l;
    split3(v, h, md, l);
    const long base = ((long)(k >> 4) * 3 * Mpad + m) * 16 + (k & 15), ps = (long)Mpad * 16;
    o[base] = (uint16_t)(h >> 16);
    o[base + ps] = (uint16_t)(md >> 16);
    o[base + 2 * ps] = (uint16_t)(l >> 16);
  } else {
    out[packed_index(k, m, layout, Mpad)] = v;
  }
}

// single-operand pack (op-level ABI): destination order, writes the zero padding too
__global__ __launch_bounds__(256) void pack_one_kernel(PackOne j) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)j.Kpad * j.Mpad) return;
  int k, m;
  if (j.layout == 2) {
    k = (int)(idx / j.Mpad);
    m = (int)(idx % j.Mpad);
  } else if (j.layout) {
    const long chunk = (long)j.Mpad * 16;
    const int kc = (int)(idx / chunk);
    const int r = (int)(idx - kc * chunk);
    m = r >> 4;
    k = kc * 16 + (r & 15);
  } else {
    k = (int)(idx / j.Mpad);
    m = (int)(idx % j.Mpad);
  }
  const int C = j.mode == 0 ? j.Cin : j.Cout;     // reduction channels
  const int Mr = j.mode == 0 ? j.Cout : j.Cin;    // rows
  float v = 0.f;
  if (k < C * j.KK && m < Mr) {
    int c, tap;
    if (j.tap) {
      tap = k / C;
      c = k - tap * C;
    } else {
      c = k / j.KK;
      tap = k - c * j.KK;
    }
    const long co = j.mode == 0 ? m : c, ci = j.mode == 0 ? c : m;
    if (ci < j.Cinw) v = j.w[(co * j.Cinw + ci) * j.KK + tap];   // padded input channels: 0
  }
  if (j.layout == 2)
    pack_store(j.out, k, m, 2, j.Mpad, v);
  else
    j.out[idx] = v;
}

// packed layout of each operand: 0 [Kpad][Mpad] fp32, 1 [Kpad/16][Mpad][16] fp32 (conv_px2 /
// conv_px16), 2 [Kpad/16][3][Mpad][16] bf16 split terms (conv_px3: 1.5x the fp32 bytes)
static int pack_layout(const ConvShape& s, int mode) {
  if (conv_px3_used(s, mode)) return 2;
  return (conv_px2_used(s, mode) || conv_px16_used(s, mode)) ? 1 : 0;
}
size_t conv_fwd_packed_elems(const ConvShape& s) {
  const size_t e = (size_t)round_up((long)s.Cin * s.KH * s.KW, KPAD) * round_up(s.Cout, MPAD);
  return pack_layout(s, 0) == 2 ? e / 2 * 3 : e;
}
size_t conv_dgrad_packed_elems(const ConvShape& s) {
  const size_t e = (size_t)round_up((long)s.Cout * s.KH * s.KW, KPAD) * round_up(s.Cin, MPAD);
  return pack_layout(s, 1) == 2 ? e / 2 * 3 : e;
}

static int pack_single(const ConvShape& s, int mode, const float* w, float* packed, hipStream_t st) {
  PackOne j{};
  j.w = w;
  j.out = packed;
  j.mode = mode;
  j.tap = conv_tap_major(s, mode) ? 1 : 0;
  j.layout = pack_layout(s, mode);
  j.Cout = s.Cout;
  j.Cin = s.Cin;
  j.Cinw = weight_cin(s);
  j.KK = s.KH * s.KW;
  j.Kpad = (int)(mode == 0 ? round_up((long)s.Cin * j.KK, KPAD) : round_up((long)s.Cout * j.KK, KPAD));
  j.Mpad = (int)(mode == 0 ? round_up(s.Cout, MPAD) : round_up(s.Cin, MPAD));
  hipLaunchKernelGGL(pack_one_kernel, dim3(cdiv((long)j.Kpad * j.Mpad, 256)), dim3(256), 0, st, j);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}
int conv_pack_fwd(const ConvShape& s, const float* w, float* packed, hipStream_t st) {
  return pack_single(s, 0, w, packed, st);
}
int conv_pack_dgrad(const ConvShape& s, const float* w, float* packed, hipStream_t st) {
  return pack_single(s, 1, w, packed, st);
}

PackJob conv_pack_job(const ConvShape& s, const float* w, float* out_f, float* out_d) {
  PackJob j{};
  j.w = w;
  j.Cout = s.Cout;
  j.Cin = s.Cin;
  j.Cinw = weight_cin(s);
  j.KK = s.KH * s.KW;
  j.f = PackDst{out_f, conv_tap_major(s, 0) ? 1 : 0, pack_layout(s, 0), (int)round_up(s.Cout, MPAD)};
  j.d = PackDst{out_d, conv_tap_major(s, 1) ? 1 : 0, pack_layout(s, 1), (int)round_up(s.Cin, MPAD)};
  auto kc = [](const PackDst& d) { return !d.out || (d.tap && d.layout); };
  j.tiled = j.Cinw == s.Cin && s.Cin % 16 == 0 && s.Cout % 16 == 0 && j.KK <= 9 && kc(j.f) && kc(j.d) &&
            (j.f.out || j.d.out);
  return j;
}

long conv_pack_job_blocks(const PackJob& j) {
  return j.tiled ? (long)(j.Cout / 16) * (j.Cin / 16) : cdiv((long)j.Cout * j.Cinw * j.KK, 256);
}

// Tiled job: a block owns 16 output x 16 input channels x KK taps.  It reads the 16 source rows
// of 16*KK contiguous floats (coalesced) into LDS and writes, per tap, the 16 x 16 k-contiguous
// chunk of each packed operand -- 256 consecutive floats in both layouts (k = tap*C + c with
// C % 16 == 0 keeps a chunk inside one 16-deep K block).
__device__ void pack_tile(const PackJob& j, int blk) {
  __shared__ float T[16][16 * 9 + 1];   // KK <= 9 (tiled jobs)
  const int ncb = j.Cin / 16;
  const int co0 = blk / ncb * 16, ci0 = blk % ncb * 16;
  const int KK = j.KK, RL = 16 * KK;
  for (int e = threadIdx.x; e < 16 * RL; e += 256) {
    const int co = e / RL, r = e - co * RL;
    T[co][r] = j.w[((long)(co0 + co) * j.Cin + ci0) * KK + r];
  }
  __syncthreads();
  const int hi = threadIdx.x >> 4, lo = threadIdx.x & 15;
  auto put = [&](const PackDst& d, long k16, int row0, float v) {
    if (d.layout == 2) {   // the three split terms, 16 x 16 bf16 each
      uint16_t* o = reinterpret_cast<uint16_t*>(d.out);
      uint32_t h, md, l;
      split3(v, h, md, l);
      const long base = (k16 * 3 * d.Mpad + row0) * 16 + threadIdx.x, ps = (long)d.Mpad * 16;
      o[base] = (uint16_t)(h >> 16);
      o[base + ps] = (uint16_t)(md >> 16);
      o[base + 2 * ps] = (uint16_t)(l >> 16);
    } else {
      d.out[(k16 * d.Mpad + row0) * 16 + threadIdx.x] = v;
    }
  };
  for (int tap = 0; tap < KK; ++tap) {
    if (j.f.out)   // rows co, k = tap*Cin + ci
      put(j.f, ((long)tap * j.Cin + ci0) / 16, co0, T[hi][lo * KK + tap]);
    if (j.d.out)   // rows ci, k = tap*Cout + co
      put(j.d, ((long)tap * j.Cout + co0) / 16, ci0, T[lo][hi * KK + tap]);
  }
}

// Source-ordered: consecutive threads read consecutive weights (coalesced, each weight read
// once); the two scattered writes of a block land in a few packed rows that L2 merges into
// full lines.  Destination padding is never touched (zeroed at allocation).
__global__ __launch_bounds__(256) void pack_batch_kernel(const PackJob* __restrict__ jobs, int njobs) {
  __shared__ int s_job;
  if (threadIdx.x == 0) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (jobs[mid].block_begin <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_job = lo;
  }
  __syncthreads();
  const PackJob& j = jobs[__builtin_amdgcn_readfirstlane(s_job)];
  if (j.tiled) {
    pack_tile(j, (int)(blockIdx.x - j.block_begin));
    return;
  }
  const unsigned e = (unsigned)(blockIdx.x - j.block_begin) * 256u + threadIdx.x;
  const unsigned KK = (unsigned)j.KK, Cinw = (unsigned)j.Cinw;   // source layout [Cout][Cinw][KK]
  if (e >= (unsigned)j.Cout * Cinw * KK) return;
  const float v = j.w[e];
  const unsigned row = e / KK;
  const int tap = (int)(e - row * KK);
  const int co = (int)(row / Cinw);
  const int ci = (int)(row - (unsigned)co * Cinw);
  if (j.f.out) {
    const int k = j.f.tap ? tap * j.Cin + ci : ci * j.KK + tap;
    pack_store(j.f.out, k, co, j.f.layout, j.f.Mpad, v);
  }
  if (j.d.out) {
    const int k = j.d.tap ? tap * j.Cout + co : co * j.KK + tap;
    pack_store(j.d.out, k, ci, j.d.layout, j.d.Mpad, v);
  }
}

int& conv_arith_ref() {
  static thread_local int v = 1;
  return v;
}
int conv_last_arith() { return conv_arith_ref(); }

int conv_pack_batch(const PackJob* dev_jobs, int njobs, long total_blocks, hipStream_t st) {
  if (njobs == 0) return MD2_OK;
  hipLaunchKernelGGL(pack_batch_kernel, dim3(total_blocks), dim3(256), 0, st, dev_jobs, njobs);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

#endif  // MD2_CONV_PART == 0

// ---------------------------------------------------------------------------------------------
// kernel arguments
// ---------------------------------------------------------------------------------------------
struct GemmDims {
  int M;
  long N;       // pixels (fwd/dgrad) or filter columns (wgrad)
  int K;        // reduction length (fwd/dgrad); wgrad: pixels (long fits int here)
  int kper;     // K elements per split (multiple of BK)
  int Mpad;     // packed A leading dimension (fwd/dgrad)
};

struct ConvArgs {
  GemmDims g;
  int Cin, H, W, Cout, Ho, Wo, stride, pad;
  long HW, HoWo;
  FastDiv fd_pix;    // pixels per image of the N axis (Ho*Wo fwd/wgrad, H*W dgrad)
  FastDiv fd_row;    // row length of the N axis (Wo fwd/wgrad, W dgrad)
  FastDiv fd_bdiv;
  TensorIn in;
  const float* A;    // packed weights (fwd/dgrad)
  const float* dy;   // dgrad / wgrad
  TensorOut out;
  float* slab;       // split-K partials [splits][M][N] or nullptr
  // byte extents of the buffer resources (raw buffer loads: an offset past the extent reads 0,
  // which implements the zero padding of the gathers without branches)
  uint32_t A_bytes, b0_bytes, b1_bytes;
  uint32_t HW4, HoWo4;   // channel strides in bytes (scalar soffset steps of the tap-major gathers)
  // stride-2 dgrad by output-parity class (tap-major only): the N axis enumerates the input
  // pixels (ph_y0 + 2j, ph_x0 + 2i) of one class (fd_pix / fd_row are the class extents) and K
  // runs over that class's taps ph_taps[0..ntaps) only
  int ph_y0, ph_x0;
  int ph_taps[16];       // <= ceil(7/2)^2 taps per class
  // merged launch of the four classes (3x3 / 1x1 kernels, even H and W: equal class extents):
  // ph_S > 0 = split-K factor per class; class c has origin (ph_y0c, ph_x0c), ph_ntc taps at
  // ph_taps[4c..], K = ph_ntc * Cout; its blocks are z = c * ph_S + split
  int ph_S;
  int ph_y0c[4], ph_x0c[4], ph_ntc[4];
  int xcd;               // XCD-aware block -> tile order (conv_px2 kernels; MD2_XCD)
  int hx_cper;           // conv_halo3: 16-channel reduction chunks per split; conv_whalo: pixel
                         // chunks per split
  int hx_r, hx_nchunk;   // conv_whalo: image rows per pixel chunk, chunks in all
  int hx_ext;            // conv_halo3 dgrad on the zero-ring-padded dY (reflect adjoint, first half)
  double* bn_part;       // conv_halo3 forward: per-tile BN partials [Cout][gridDim.x][2] (or nullptr)
};

// (image, pixel-in-plane) of N-axis element nn for fwd / dgrad outputs
__device__ __forceinline__ void out_pixel(const ConvArgs& a, bool phase, int y0, int x0, long nn,
                                          int& img, long& pix, long& plane) {
  // y0, x0: origin of the stride-2 dgrad parity class (phase)
  img = (int)fdiv((uint32_t)nn, a.fd_pix);
  const long r = nn - (long)img * a.fd_pix.d;
  if (phase) {
    const int jy = (int)fdiv((uint32_t)r, a.fd_row);
    const int jx = (int)(r - (long)jy * a.fd_row.d);
    pix = (long)(y0 + 2 * jy) * a.W + x0 + 2 * jx;
    plane = a.HW;
  } else {
    pix = r;
    plane = a.fd_pix.d;
  }
}

__device__ __forceinline__ void out_pixel(const ConvArgs& a, bool phase, long nn, int& img, long& pix,
                                          long& plane) {
  out_pixel(a, phase, a.ph_y0, a.ph_x0, nn, img, pix, plane);
}

template <int TM, int TN, int BK>
__device__ __forceinline__ void mma_chunk(const float* __restrict__ As, int lda,
                                          const float* __restrict__ Bs, int ldb, int am0, int bn0,
                                          int lane, f32x16 (&acc)[TM][TN]) {
  const int kh = lane >> 5, l = lane & 31;
  // fragments of k-step kk+1 are read while the MFMAs of kk issue (register double buffer;
  // fully unrolled so every index is static)
  float a[2][TM], b[2][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) a[0][i] = As[kh * lda + am0 + i * 32 + l];
#pragma unroll
  for (int j = 0; j < TN; ++j) b[0][j] = Bs[kh * ldb + bn0 + j * 32 + l];
#pragma unroll
  for (int kk = 0; kk < BK / 2; ++kk) {
    const int cur = kk & 1, nxt = cur ^ 1;
    if (kk + 1 < BK / 2) {
#pragma unroll
      for (int i = 0; i < TM; ++i) a[nxt][i] = As[(2 * kk + 2 + kh) * lda + am0 + i * 32 + l];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[nxt][j] = Bs[(2 * kk + 2 + kh) * ldb + bn0 + j * 32 + l];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
  }
}

// Epilogue of one accumulator element (m, n) for the NCHW-style outputs of fwd / dgrad.
__device__ __forceinline__ void store_out(const TensorOut& o, int m, int img, long pix, long HoWo,
                                          float v) {
  if (o.bias) v += o.bias[m];
  v = apply_act(v, o.act);
  float* dst = (m < o.c0) ? o.p0 + (long)img * o.bs0 + (long)m * HoWo + pix
                          : o.p1 + (long)img * o.bs1 + (long)(m - o.c0) * HoWo + pix;
  if (o.accumulate)
    *dst += v;
  else
    *dst = v;
}

#include "conv_px.inc"
#include "conv_px2.inc"
#include "conv_px16.inc"
#include "conv_px3.inc"
#include "conv_wpx3.inc"

// Launch of a kernel whose dynamic LDS is laid out in conv_lds.h: the opt-in ceiling is set once
// per instantiation, and a launch whose kernel would index past its allocation is refused (it
// would compute garbage without a fault).
struct LdsSize {
  long need, bytes, cap;   // conv_lds.h: need(...), bytes(...), cap of the kernel's geometry
};
template <auto KERNEL, typename... Args>
int lds_launch(dim3 grid, dim3 block, const LdsSize& z, hipStream_t st, const Args&... args) {
  MD2_CHECK_ARG(z.need <= z.bytes && z.bytes <= z.cap, "conv: kernel indexes past its dynamic LDS (conv_lds.h)");
  static bool attr = false;
  if (!attr) {
    MD2_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)z.cap));
    attr = true;
  }
  hipLaunchKernelGGL(KERNEL, grid, block, (size_t)z.bytes, st, args...);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// the LDS-halo kernels (conv_halo.inc, its own translation unit conv_halo.hip)
int halo_launch(int mode, const ConvArgs& a, int items, int splits, int reflect, hipStream_t st);
int halo2d_launch(int mode, const ConvArgs& a, int mw, int splits, int reflect, hipStream_t st);
int halo_s2_launch(const ConvArgs& a, int items, int splits, hipStream_t st);
int whalo_launch(const ConvArgs& a, int items, int ksteps, int splits, hipStream_t st);
// arithmetic of the last conv kernel this host thread launched (profiling labels, conv.h)
int& conv_arith_ref();
// the ResNet stem forward on the space-to-depth grid (conv_stem.inc, translation unit conv_stem.hip)
bool stem_s2d_applies(const ConvShape& s, const TensorIn& x, const TensorOut& y);
int stem_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st);
bool stem_wgrad_s2d_applies(const ConvShape& s, const TensorIn& x);
int stem_wgrad_blocks(const ConvShape& s);
int stem_wgrad_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st);

// split-K reduction + epilogue for fwd / dgrad, four consecutive pixels of one output plane per
// thread (plain output mapping, pixels per image % 4 == 0): float4 slab loads, one store
template <int P_ = 0>
__global__ __launch_bounds__(256) void splitk_reduce_px4_kernel(ConvArgs a, int splits) {
  const long idx = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
  const long total = (long)a.g.M * a.g.N;
  if (idx >= total) return;
  const int m = (int)(idx / a.g.N);
  const long nn = idx - (long)m * a.g.N;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int s = 0; s < splits; ++s) {
    const float4 t = *reinterpret_cast<const float4*>(a.slab + (long)s * total + idx);
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  const TensorOut& o = a.out;
  const int img = (int)fdiv((uint32_t)nn, a.fd_pix);
  const long pix = nn - (long)img * a.fd_pix.d, HoWo = a.fd_pix.d;
  float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (o.bias) r[q] += o.bias[m];
    r[q] = apply_act(r[q], o.act);
  }
  float* dst = (m < o.c0) ? o.p0 + (long)img * o.bs0 + (long)m * HoWo + pix
                          : o.p1 + (long)img * o.bs1 + (long)(m - o.c0) * HoWo + pix;
  float4 w = make_float4(r[0], r[1], r[2], r[3]);
  if (o.accumulate) {
    const float4 d = *reinterpret_cast<const float4*>(dst);
    w.x = d.x + w.x; w.y = d.y + w.y; w.z = d.z + w.z; w.w = d.w + w.w;
  }
  *reinterpret_cast<float4*>(dst) = w;
}

// split-K reduction + epilogue for fwd / dgrad (32-bit index math with magic-number divisions --
// the 64-bit divisions cost 10-22 us per stride-2 dgrad -- and four split loads in flight, summed
// in split order: the order of the fused BN passes that read the same slabs, bit-identical)
template <int P_ = 0>   // template: instantiated in the fwd and dgrad translation units
__global__ __launch_bounds__(256) void splitk_reduce_px_kernel(ConvArgs a, int splits, int phase, FastDiv fdN,
                                                               FastDiv fdT) {
  uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  const uint32_t total = fdT.d;   // M * N
  // merged stride-2 dgrad classes (a.ph_S > 0): slabs [class][split][M][N]
  int cls = 0, y0 = a.ph_y0, x0 = a.ph_x0;
  if (phase && a.ph_S > 0) {
    cls = (int)fdiv(idx, fdT);
    if (cls >= 4) return;
    idx -= (uint32_t)cls * total;
    y0 = a.ph_y0c[cls];
    x0 = a.ph_x0c[cls];
  } else if (idx >= total) {
    return;
  }
  const int m = (int)fdiv(idx, fdN);
  const uint32_t nn = idx - (uint32_t)m * fdN.d;
  const float* p = a.slab + (size_t)cls * splits * total + idx;
  float v = 0.f;
  int s = 0;
  for (; s + 3 < splits; s += 4) {
    const float t0 = p[(size_t)s * total], t1 = p[(size_t)(s + 1) * total];
    const float t2 = p[(size_t)(s + 2) * total], t3 = p[(size_t)(s + 3) * total];
    v += t0;
    v += t1;
    v += t2;
    v += t3;
  }
  for (; s < splits; ++s) v += p[(size_t)s * total];
  int img;
  long pix, plane;
  out_pixel(a, phase != 0, y0, x0, (long)nn, img, pix, plane);
  store_out(a.out, m, img, pix, plane, v);
}

// pad_reflect(x, 1)'s adjoint (src/depth_decoder.jl:5, NNlib pad_reflect), second half of the
// reflect-padded dgrad: the full adjoint on the padded grid -- `splits` split-K slabs summed here
// (element (n, c, r, q) of slab k at src + k * ss + n * sn + c * sc + r * (W + 2) + q) -- folded
// onto dX [N][C][H][W]: padded row 0 is input row 1, padded row H+1 input row H-2 (likewise
// columns), stored / accumulated through the conv's TensorOut (concat split, image strides).
// Flat grid over the N * C * H * W outputs, one per thread (a planes-by-blocks grid of small maps
// was workgroup-dispatch bound; 4 outputs x 9 candidate loads per thread latency bound: 10-20 us
// for 1-5 MB); 32-bit index math.  Candidates per split: rows {i+1, reflected}, columns likewise
// -- 4 loads issued back to back (absent ones read the centre and are dropped); SMALL (H or W ==
// 3: a row / column reflected twice) takes the 3 x 3 set.
template <bool SMALL>
__global__ __launch_bounds__(256) void fold_reflect_kernel(const float* __restrict__ src, int splits, long ss,
                                                           long sn, long sc, TensorOut o, FastDiv fd_hw,
                                                           FastDiv fd_w, FastDiv fd_c, uint32_t total) {
  constexpr int NR = SMALL ? 3 : 2;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= total) return;
  const int H = (int)fd_hw.d / (int)fd_w.d, W = (int)fd_w.d, P = W + 2;
  const uint32_t nc = fdiv(idx, fd_hw);
  const int pix = (int)(idx - nc * fd_hw.d);
  const int n = (int)fdiv(nc, fd_c), c = (int)(nc - n * fd_c.d);
  const int i = (int)fdiv((uint32_t)pix, fd_w), j = pix - i * W;
  const float* p = src + n * sn + c * sc;
  // rows mapping to i: {i+1} + the reflected ones; columns likewise (fixed summation order)
  const int rows[3] = {i + 1, i == 1 ? 0 : (i == H - 2 ? H + 1 : -1), (i == H - 2 && i == 1) ? H + 1 : -1};
  const int cols[3] = {j + 1, j == 1 ? 0 : (j == W - 2 ? W + 1 : -1), (j == W - 2 && j == 1) ? W + 1 : -1};
  int off[NR * NR];
  bool use[NR * NR];
#pragma unroll
  for (int a_ = 0; a_ < NR; ++a_)
#pragma unroll
    for (int b_ = 0; b_ < NR; ++b_) {
      use[NR * a_ + b_] = rows[a_] >= 0 && cols[b_] >= 0;
      off[NR * a_ + b_] = use[NR * a_ + b_] ? rows[a_] * P + cols[b_] : (i + 1) * P + j + 1;
    }
  float v = 0.f;
#pragma unroll 2
  for (int k = 0; k < splits; ++k, p += ss) {
    float t[NR * NR];
#pragma unroll
    for (int u = 0; u < NR * NR; ++u) t[u] = p[off[u]];
#pragma unroll
    for (int u = 0; u < NR * NR; ++u) v += use[u] ? t[u] : 0.f;
  }
  float* dst = (c < o.c0) ? o.p0 + (long)n * o.bs0 + (long)c * fd_hw.d + pix
                          : o.p1 + (long)n * o.bs1 + (long)(c - o.c0) * fd_hw.d + pix;
  if (o.accumulate)
    *dst += v;
  else
    *dst = v;
}

// Four consecutive pixels of one row per thread (W % 4 == 0): where all four are interior (the
// row is not 1 / H-2, the columns 2 .. W-3) each split is ONE 4-float load of the padded image
// (dword-aligned) instead of four 2x2 candidate gathers per pixel; border quads take the generic
// per-pixel path.  The same fp sums in the same order as fold_reflect_kernel (bit-identical).
template <int P_ = 0>
__global__ __launch_bounds__(256) void fold_reflect4_kernel(const float* __restrict__ src, int splits, long ss,
                                                            long sn, long sc, TensorOut o, FastDiv fd_hw,
                                                            FastDiv fd_w4, FastDiv fd_c, int H, uint32_t total4) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= total4) return;
  const int W4 = (int)fd_w4.d, W = 4 * W4, P = W + 2;
  const uint32_t HW4 = (uint32_t)(H * W4);
  const uint32_t nc = idx / HW4;
  const int q = (int)(idx - nc * HW4);
  const int n = (int)fdiv(nc, fd_c), c = (int)(nc - n * fd_c.d);
  const int i = (int)fdiv((uint32_t)q, fd_w4), j0 = 4 * (q - i * W4);
  const float* p = src + n * sn + c * sc;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (i != 1 && i != H - 2 && j0 >= 2 && j0 + 3 <= W - 3) {
    const float* r = p + (i + 1) * P + j0 + 1;
#pragma unroll 2
    for (int k = 0; k < splits; ++k, r += ss) {
      float t[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = r[e];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += t[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      const int rows[2] = {i + 1, i == 1 ? 0 : (i == H - 2 ? H + 1 : -1)};
      const int cols[2] = {j + 1, j == 1 ? 0 : (j == W - 2 ? W + 1 : -1)};
      const float* pp = p;
      for (int k = 0; k < splits; ++k, pp += ss) {
#pragma unroll
        for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
          for (int b_ = 0; b_ < 2; ++b_)
            if (rows[a_] >= 0 && cols[b_] >= 0) v[e] += pp[rows[a_] * P + cols[b_]];
      }
    }
  }
  const int pix = i * W + j0;
  float* dst = (c < o.c0) ? o.p0 + (long)n * o.bs0 + (long)c * fd_hw.d + pix
                          : o.p1 + (long)n * o.bs1 + (long)(c - o.c0) * fd_hw.d + pix;
  float4 r4 = make_float4(v[0], v[1], v[2], v[3]);
  if (o.accumulate) {
    const float4 d = *reinterpret_cast<const float4*>(dst);
    r4 = make_float4(d.x + r4.x, d.y + r4.y, d.z + r4.z, d.w + r4.w);
  }
  *reinterpret_cast<float4*>(dst) = r4;
}

// ---------------------------------------------------------------------------------------------
// wgrad kernel: lanes along the pixel (K) axis for both operands, transposed into LDS
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int BK, int WM, int WN, int KH, int KW, int S, int RFL>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(ConvArgs a) {
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int KK = KH * KW;
  constexpr int RP = 256 / BK;          // rows per pass
  constexpr int A_EL = BM / RP, B_EL = BN / RP;
  constexpr int LDA = BM + 1, LDB = BN + 1;
  static_assert(A_EL >= 1 && B_EL >= 1, "tile");
  __shared__ float As[2][BK][LDA];
  __shared__ float Bs[2][BK][LDB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int m0 = blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;
  const long kbeg = (long)blockIdx.z * a.g.kper;
  const long Ktot = a.g.K;
  const long kend = min(Ktot, kbeg + (long)a.g.kper);
  const int nk = (int)((kend - kbeg + BK - 1) / BK);
  const int kl = tid % BK;
  const int rg = tid / BK;

  // per-thread filter columns of B (fixed for the whole kernel)
  float areg[A_EL], breg[B_EL];

  auto load = [&](long k0) {
    const long p = k0 + kl;
    const bool pv = p < kend;
    int img = 0, oy = 0, ox = 0;
    if (pv) {
      img = (int)fdiv((uint32_t)p, a.fd_pix);
      const int pix = (int)(p - (long)img * a.fd_pix.d);
      oy = (int)fdiv((uint32_t)pix, a.fd_row);
      ox = pix - oy * (int)a.fd_row.d;
    }
    const float* dyb = a.dy + (long)img * a.Cout * a.HoWo + (long)oy * a.Wo + ox;
#pragma unroll
    for (int j = 0; j < A_EL; ++j) {
      const int m = m0 + rg + j * RP;
      areg[j] = (pv && m < a.g.M) ? dyb[(long)m * a.HoWo] : 0.f;
    }
    const int q = (int)fdiv((uint32_t)img, a.fd_bdiv);
    const float* b0 = a.in.p0 + (long)(img - q * (int)a.fd_bdiv.d) * a.in.bs0 + (long)q * a.in.bhi;
    const float* b1 = a.in.p1 ? a.in.p1 + (long)img * a.in.bs1 : nullptr;
    const int py = oy * S - a.pad, px = ox * S - a.pad;
#pragma unroll
    for (int j = 0; j < B_EL; ++j) {
      const int nidx = n0 + rg + j * RP;
      float v = 0.f;
      if (pv && nidx < a.g.N) {
        const int c = nidx / KK;
        const int r = nidx - c * KK;
        const int kh = r / KW, kw = r - (r / KW) * KW;
        int iy = py + kh, ix = px + kw;
        bool ok = true;
        if (RFL) {
          iy = refl(iy, a.H);
          ix = refl(ix, a.W);
        } else {
          ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        }
        const float* src = (c < a.in.c0) ? b0 + (long)c * a.HW : b1 + (long)(c - a.in.c0) * a.HW;
        if (ok) v = src[iy * a.W + ix];
      }
      breg[j] = v;
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int j = 0; j < A_EL; ++j) As[buf][kl][rg + j * RP] = areg[j];
#pragma unroll
    for (int j = 0; j < B_EL; ++j) Bs[buf][kl][rg + j * RP] = breg[j];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    load(kbeg);
    store_tiles(0);
  }
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    if (t + 1 < nk) load(kbeg + (long)(t + 1) * BK);
    mma_chunk<TM, TN, BK>(&As[cur][0][0], LDA, &Bs[cur][0][0], LDB, wm * TM * 32, wn * TN * 32, lane, acc);
    if (t + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }

  float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long nn = n0 + wn * TN * 32 + j * 32 + (lane & 31);
    if (nn >= a.g.N) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < a.g.M) sl[(long)m * a.g.N + nn] = acc[i][j][r];
      }
  }
}

// tap-major wgrad: filter columns n = tap*Cin + c.  A block covers TT = BN/CW consecutive taps
// x CW channels (CW | Cin, and CW | the concat split, so the block reads one tensor): row j of a
// thread is tap (RP*j)/CW and channel (RP*j)%CW + rg, both compile-time up to the block base.
// Per K chunk each thread computes one gather offset per tap (TT of them); every element is then
// a buffer load with that offset and a scalar channel soffset -- no VALU per element.  The slab
// is written in (m, n) tap-major order; the final reduction permutes to [Cout][Cin][KH][KW].
template <int BM, int BN, int BK, int WM, int WN, int KH, int KW, int S, int RFL, int CW>
__global__ __launch_bounds__(256) void conv_wgrad_tap_kernel(ConvArgs a) {
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int KK = KH * KW;
  constexpr int RP = 256 / BK;          // rows per pass
  constexpr int A_EL = BM / RP, B_EL = BN / RP;
  constexpr int TT = BN / CW;           // taps per block
  constexpr int LDA = BM + 1, LDB = BN + 1;
  static_assert(A_EL >= 1 && B_EL >= 1 && TT >= 1 && CW % RP == 0, "tile");
  __shared__ float As[2][BK][LDA];
  __shared__ float Bs[2][BK][LDB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int m0 = blockIdx.y * BM;
  const int ncb = a.Cin / CW;
  const int tb = (int)blockIdx.x / ncb * TT;           // first tap of the block
  const int cbk = ((int)blockIdx.x % ncb) * CW;        // first channel of the block
  const int kbeg = blockIdx.z * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;
  const int kl = tid % BK;
  const int rg = tid / BK;
  const int mlim = a.g.M - m0 - rg;     // row j of dY valid iff RP*j < mlim

  const bool sec = cbk >= a.in.c0;      // block-uniform concat side
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(a.dy, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rx = sec ? make_rsrc(a.in.p1, a.b1_bytes) : make_rsrc(a.in.p0, a.b0_bytes);
  const uint32_t cso = (uint32_t)(sec ? cbk - a.in.c0 : cbk) * a.HW4;

  float areg[A_EL], breg[B_EL];

  // all offsets in 32 bits: every extent is < 2 GB (checked on the host)
#define MD2_W_LOAD(K0)                                                                            \
  {                                                                                               \
    const int p = (K0) + kl;                                                                      \
    const bool pv = p < kend;                                                                     \
    const uint32_t pc = (uint32_t)(pv ? p : kbeg);                                                \
    const uint32_t img = fdiv(pc, a.fd_pix);                                                      \
    const uint32_t pix = pc - img * a.fd_pix.d;                                                   \
    const uint32_t oy = fdiv(pix, a.fd_row);                                                      \
    const uint32_t ox = pix - oy * a.fd_row.d;                                                    \
    const uint32_t va = pv ? ((img * (uint32_t)a.Cout + rg) * (uint32_t)a.HoWo + pix) * 4u : OOB; \
    _Pragma("unroll") for (int j = 0; j < A_EL; ++j)                                              \
      areg[j] = bload_s(rdy, RP * j < mlim ? va : OOB, (uint32_t)(m0 + RP * j) * a.HoWo4);        \
    uint32_t vb;                                                                                  \
    if (sec) {                                                                                    \
      vb = (img * (uint32_t)a.in.bs1 + rg * (uint32_t)a.HW) * 4u;                                 \
    } else {                                                                                      \
      const uint32_t q = fdiv(img, a.fd_bdiv);                                                    \
      vb = ((img - q * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + q * (uint32_t)a.in.bhi +               \
            rg * (uint32_t)a.HW) * 4u;                                                            \
    }                                                                                             \
    const int py = (int)oy * S - a.pad, px = (int)ox * S - a.pad;                                 \
    uint32_t vt[TT];                                                                              \
    _Pragma("unroll") for (int t = 0; t < TT; ++t) {                                              \
      const int tap = tb + t;                                                                     \
      const int kh = tap / KW, kw = tap - (tap / KW) * KW;                                        \
      int iy = py + kh, ix = px + kw;                                                             \
      bool ok;                                                                                    \
      if (RFL) {                                                                                  \
        iy = refl(iy, a.H);                                                                       \
        ix = refl(ix, a.W);                                                                       \
        ok = pv;                                                                                  \
      } else {                                                                                    \
        ok = pv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;                  \
      }                                                                                           \
      vt[t] = (ok && tap < KK) ? vb + (uint32_t)(iy * a.W + ix) * 4u : OOB;                       \
    }                                                                                             \
    _Pragma("unroll") for (int j = 0; j < B_EL; ++j)                                              \
      breg[j] = bload_s(rx, vt[(RP * j) / CW], cso + (uint32_t)((RP * j) % CW) * a.HW4);         \
  }
#define MD2_W_STORE(BUF)                                                                          \
  _Pragma("unroll") for (int j = 0; j < A_EL; ++j) As[BUF][kl][rg + j * RP] = areg[j];            \
  _Pragma("unroll") for (int j = 0; j < B_EL; ++j) Bs[BUF][kl][rg + j * RP] = breg[j];

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    MD2_W_LOAD(kbeg);
    MD2_W_STORE(0);
  }
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    if (t + 1 < nk) MD2_W_LOAD(kbeg + (t + 1) * BK);
    mma_chunk<TM, TN, BK>(&As[cur][0][0], LDA, &Bs[cur][0][0], LDB, wm * TM * 32, wn * TN * 32, lane, acc);
    if (t + 1 < nk) {
      MD2_W_STORE(cur ^ 1);
    }
    __syncthreads();
  }
#undef MD2_W_LOAD
#undef MD2_W_STORE

  float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wn * TN * 32 + j * 32 + (lane & 31);
    const int tap = tb + nl / CW;
    if (tap >= KK) continue;
    const long nn = (long)tap * a.Cin + cbk + nl % CW;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < a.g.M) sl[(long)m * a.g.N + nn] = acc[i][j][r];
      }
  }
}

// Weight gradient of a Cout <= 32, 3x3 stride-1 tap-major conv (the high-resolution
// DepthDecoder convs): dW[m][tap*Cin + c] = sum_p dY[m][p] X[c][gather(p, tap)].  32-row x
// 128-column MFMA tiles would leave rows idle (Cout 16) and waste up to 7/16 of the 144 = 9 taps
// x 16 channels, so here one block owns ALL 16*MT rows x ALL 9 taps of a 16-channel group and
// the four waves split the pixel (K) dimension instead: per 64-pixel chunk the block stages
// A[64 px][16*MT m] and B[9 taps][64 px][16 ch] in LDS (coalesced 64-pixel loads, wave-uniform
// row / channel soffsets, one gather offset per tap), wave w contracts pixels 16w..16w+15 on
// v_mfma_f32_16x16x4_f32 into MT x 9 accumulators (each B fragment feeds MT MFMAs), and a
// fixed-order LDS sum over the waves writes the block's split-K slab (tap-major, finalised by
// wgrad_reduce_kernel).  Every MFMA row and column is useful work.
template <int MT, int KH, int KW, int RFL>
__global__ __launch_bounds__(256) void conv_wgrad16_kernel(ConvArgs a) {
  constexpr int KK = KH * KW, BK = 64, LD = 17, LDA = 16 * MT + 1, RW = 4 * MT;
  static_assert(4 * KK * 4 * 64 <= KK * BK * LD, "reduction buffer");
  __shared__ float As[BK * LDA];
  __shared__ float Bs[KK * BK * LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cbk = (int)blockIdx.x * 16;
  const int kbeg = blockIdx.z * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;

  const bool sec = cbk >= a.in.c0;
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(a.dy, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rx = sec ? make_rsrc(a.in.p1, a.b1_bytes) : make_rsrc(a.in.p0, a.b0_bytes);
  // wave w loads dY rows RW*w..RW*w+RW-1 and X channels cbk+4w..cbk+4w+3 (wave-uniform soffsets)
  const uint32_t cso = (uint32_t)((sec ? cbk - a.in.c0 : cbk) + 4 * wid) * a.HW4;
  const uint32_t mso = (uint32_t)(RW * wid) * a.HoWo4;

  float areg[RW], breg[KK][4];
  auto load = [&](int k0) {
    const int p = k0 + lane;
    const bool pv = p < kend;
    const uint32_t pc = (uint32_t)(pv ? p : kbeg);
    const uint32_t img = fdiv(pc, a.fd_pix);
    const uint32_t pix = pc - img * a.fd_pix.d;
    const uint32_t oy = fdiv(pix, a.fd_row);
    const uint32_t ox = pix - oy * a.fd_row.d;
    const uint32_t va = pv ? (img * (uint32_t)a.Cout * (uint32_t)a.HoWo + pix) * 4u : OOB;
#pragma unroll
    for (int r = 0; r < RW; ++r)
      areg[r] = bload_s(rdy, RW * wid + r < a.g.M ? va : OOB, mso + (uint32_t)r * a.HoWo4);
    uint32_t vb;
    if (sec) {
      vb = img * (uint32_t)a.in.bs1 * 4u;
    } else {
      const uint32_t q = fdiv(img, a.fd_bdiv);
      vb = ((img - q * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + q * (uint32_t)a.in.bhi) * 4u;
    }
    const int py = (int)oy - a.pad, px = (int)ox - a.pad;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      int iy = py + t / KW, ix = px + t % KW;
      bool ok;
      if (RFL) {
        iy = refl(iy, a.H);
        ix = refl(ix, a.W);
        ok = pv;
      } else {
        ok = pv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      }
      const uint32_t vt = ok ? vb + (uint32_t)(iy * a.W + ix) * 4u : OOB;
#pragma unroll
      for (int c = 0; c < 4; ++c) breg[t][c] = bload_s(rx, vt, cso + (uint32_t)c * a.HW4);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int r = 0; r < RW; ++r) As[lane * LDA + RW * wid + r] = areg[r];
#pragma unroll
    for (int t = 0; t < KK; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) Bs[(t * BK + lane) * LD + 4 * wid + c] = breg[t][c];
  };

  f32x4 acc[MT][KK];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int i = lane & 15, g = lane >> 4;
  if (nk > 0) load(kbeg);
  for (int t = 0; t < nk; ++t) {
    store();
    __syncthreads();
    if (t + 1 < nk) load(kbeg + (t + 1) * BK);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const int k = 16 * wid + 4 * s4 + g;
      float av[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) av[mt] = As[k * LDA + 16 * mt + i];
#pragma unroll
      for (int tp = 0; tp < KK; ++tp) {
        const float bv = Bs[(tp * BK + k) * LD + i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv, acc[mt][tp], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // fixed-order sum over the four waves' K quarters, one 16-row tile at a time (Bs reused)
  float* red = Bs;
  float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int tp = 0; tp < KK; ++tp)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((wid * KK + tp) * 4 + r) * 64 + lane] = acc[mt][tp][r];
    __syncthreads();
    for (int o = tid; o < KK * 4 * 64; o += 256) {
      const int l = o & 63, r = (o >> 6) & 3, tp = o >> 8;
      const int m = 16 * mt + 4 * (l >> 4) + r, j = l & 15;
      const float v = red[((0 * KK + tp) * 4 + r) * 64 + l] + red[((1 * KK + tp) * 4 + r) * 64 + l] +
                      red[((2 * KK + tp) * 4 + r) * 64 + l] + red[((3 * KK + tp) * 4 + r) * 64 + l];
      if (m < a.g.M) sl[(long)m * a.g.N + (long)tp * a.Cin + cbk + j] = v;
    }
    if (mt + 1 < MT) __syncthreads();
  }
}

// Weight gradient of the ResNet stem (7x7 / stride 2, Cin <= 4 image channels, Cout = 64):
// dW[m][c*49 + tap] = sum_p dY[m][p] X[c][gather(p, tap)] with K = every output pixel (479k at
// B=12).  The generic 64x128 tiles pad its 147 filter columns to 256 (42% idle MFMA columns) and
// index every element of B; here one block owns ALL 64 rows x ALL Cin*49 columns (NT 16-column
// tiles: 147 -> 160) of a K slice, wave w the 16 rows 16w.. on v_mfma_f32_16x16x4_f32.  Per
// 64-pixel chunk: A[64 px][64 m] (coalesced dY rows, wave w its own 16) and B[64 px][NT*16] (one
// gather offset base per lane, the tap / channel parts wave-uniform) staged through LDS from
// registers loaded during the previous chunk's MFMAs.  Columns come out channel-major, i.e. in
// the final [Cout][Cin][KH][KW] order (wgrad_reduce_kernel with tapc = 0).
template <int CIN>
__global__ __launch_bounds__(256) void conv_wgrad_stem_kernel(ConvArgs a) {
  constexpr int KK = 49, BK = 64, LDA = 64 + 1, NT = (CIN * KK + 15) / 16, NB = NT * 16, LDB = NB + 1;
  constexpr int JB = (NB + 3) / 4;                  // B columns per thread (wave w: w, w+4, ...)
  __shared__ float As[BK * LDA];
  __shared__ float Bs[BK * LDB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kbeg = blockIdx.x * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;
  constexpr int ncol = CIN * KK;                    // filter columns
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(a.dy, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.in.p0, a.b0_bytes);
  const uint32_t mso = (uint32_t)(16 * wid) * a.HoWo4;

  float areg[16], breg[JB];
  auto load = [&](int k0) {
    const int p = k0 + lane;
    const bool pv = p < kend;
    const uint32_t pc = (uint32_t)(pv ? p : kbeg);
    const uint32_t img = fdiv(pc, a.fd_pix);
    const uint32_t pix = pc - img * a.fd_pix.d;
    const uint32_t oy = fdiv(pix, a.fd_row);
    const uint32_t ox = pix - oy * a.fd_row.d;
    const uint32_t va = pv ? (img * (uint32_t)a.Cout * (uint32_t)a.HoWo + pix) * 4u : OOB;
#pragma unroll
    for (int r = 0; r < 16; ++r) areg[r] = bload_s(rdy, va, mso + (uint32_t)r * a.HoWo4);
    const uint32_t q = fdiv(img, a.fd_bdiv);
    const int ibase = (int)((img - q * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + q * (uint32_t)a.in.bhi);
    const int y0 = (int)oy * 2 - a.pad, x0 = (int)ox * 2 - a.pad;
    // image extents laundered per chunk: the per-column offsets below are re-derived by a few
    // scalar ops each chunk instead of being hoisted into scalar registers
    int Wd = a.W, Hd = a.H, HWd = (int)a.HW;
    asm volatile("" : "+s"(Wd), "+s"(Hd), "+s"(HWd));
    const int rowbase = ibase + y0 * Wd + x0;
    // per-lane validity of the 7 rows / 7 columns of the window as bit masks (integer VGPRs, not
    // 49 lane masks)
    uint32_t rb = 0, cb = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      rb |= ((unsigned)(y0 + k) < (unsigned)Hd ? 1u : 0u) << k;
      cb |= ((unsigned)(x0 + k) < (unsigned)Wd ? 1u : 0u) << k;
    }
    if (!pv) rb = 0;
    // wave w gathers columns w, w+4, ...: a compile-time column set per wave (switch below)
    auto gather = [&](auto Wc) {
      constexpr int WV = decltype(Wc)::value;
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        const int n = 4 * j + WV;
        const int c = n / KK, tap = n - c * KK;
        const int kh = tap / 7, kw = tap - kh * 7;
        // out-of-window elements get bit 31 set: past every extent, the buffer load returns 0
        // (no lane masks: plain integer ops)
        const uint32_t bad = (n < ncol) ? (~((rb >> kh) & (cb >> kw)) & 1u) : 1u;
        const uint32_t off = ((uint32_t)(rowbase + c * HWd + kh * Wd + kw) << 2) | (bad << 31);
        breg[j] = bload(rx, off);
      }
    };
    switch (wid) {
      case 0: gather(std::integral_constant<int, 0>{}); break;
      case 1: gather(std::integral_constant<int, 1>{}); break;
      case 2: gather(std::integral_constant<int, 2>{}); break;
      default: gather(std::integral_constant<int, 3>{}); break;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int r = 0; r < 16; ++r) As[lane * LDA + 16 * wid + r] = areg[r];
#pragma unroll
    for (int j = 0; j < JB; ++j)
      if (4 * j + wid < NB) Bs[lane * LDB + 4 * j + wid] = breg[j];
  };

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int i = lane & 15, g = lane >> 4;
  if (nk > 0) load(kbeg);
  for (int t = 0; t < nk; ++t) {
    store();
    __syncthreads();
    if (t + 1 < nk) load(kbeg + (t + 1) * BK);
#pragma unroll
    for (int s4 = 0; s4 < BK / 4; ++s4) {
      const int k = 4 * s4 + g;
      const float av = As[k * LDA + 16 * wid + i];
#pragma unroll
      for (int tn = 0; tn < NT; ++tn)
        acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bs[k * LDB + 16 * tn + i], acc[tn], 0, 0, 0);
    }
    __syncthreads();
  }
  float* sl = a.slab + (long)blockIdx.x * a.g.M * a.g.N;
#pragma unroll
  for (int tn = 0; tn < NT; ++tn) {
    const int n = 16 * tn + i;
    if (n >= ncol) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) sl[(long)(16 * wid + 4 * g + r) * ncol + n] = acc[tn][r];
  }
}

// One-launch wgrad finalise: the split-K slab sum (SUB lanes per output, each a fixed split
// subsequence, combined in a fixed order: deterministic), the tap-major -> [Cout][Cin][KK]
// remap, accumulate, and -- in the trailing blocks -- the bias-gradient finalise over the
// bias_grad_partial_kernel partials (launched before this kernel).
struct WRed {
  const float* slab;
  int splits;
  long total;
  float* dw;
  int acc;
  int ncols, tapc, KK;
  int cinw;             // the weights' Cin (< tapc: columns of padded input channels dropped)
  long out_total;       // outputs written: Cout * cinw * KK
  const float* bpart;   // [Cout][bparts] or nullptr
  int bparts, Cout;
  float* db;
  int nmain;            // blocks of the slab reduction
};

template <int SUB>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WRed r) {
  constexpr int OPB = 256 / SUB;   // outputs per block
  if ((int)blockIdx.x >= r.nmain) {
    const int c = ((int)blockIdx.x - r.nmain) * 256 + threadIdx.x;
    if (c >= r.Cout) return;
    float sb = 0.f;
    for (int p = 0; p < r.bparts; ++p) sb += r.bpart[(long)c * r.bparts + p];
    if (r.acc)
      r.db[c] += sb;
    else
      r.db[c] = sb;
    return;
  }
  __shared__ float red[SUB][OPB];
  const int j = threadIdx.x % OPB, g = threadIdx.x / OPB;
  // SUB == 1 (few slabs): thread order = OUTPUT order, coalesced dw stores, the tap-major slab
  // column gathered; SUB == 4 (many slabs): slab order, coalesced reads of every slab, the one
  // store per output scattered (measured: each order is the faster one on its side)
  long o = (long)blockIdx.x * OPB + j, idx = o;
  bool live = o < (SUB == 1 ? r.out_total : r.total);
  if (r.tapc > 0 && live) {
    const int ocols = r.cinw * r.KK;                 // output row length
    if (SUB == 1) {                                  // o: output order
      const long m = o / ocols;
      const int n = (int)(o - m * ocols);
      const int c = n / r.KK, tp = n - c * r.KK;
      idx = m * r.ncols + (long)tp * r.tapc + c;
    } else {                                         // o: slab order
      const long m = o / r.ncols;
      const int n = (int)(o - m * r.ncols);
      const int tp = n / r.tapc, c = n - tp * r.tapc;
      live = c < r.cinw;
      o = m * ocols + (long)c * r.KK + tp;
    }
  }
  // eight slab loads in flight per thread (the pass is latency-bound on the L2/MALL-resident
  // slabs: two in flight reached ~1.3 TB/s), eight fixed-order partial sums
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    int sp = g;
    for (; sp + 7 * SUB < r.splits; sp += 8 * SUB) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = r.slab[(long)(sp + u * SUB) * r.total + idx];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += t[u];
    }
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = sp + u * SUB < r.splits ? r.slab[(long)(sp + u * SUB) * r.total + idx] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] += t[u];
  }
  float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  if (SUB > 1) {
    red[g][j] = v;
    __syncthreads();
    if (g != 0) return;
    v = red[0][j];
#pragma unroll
    for (int k = 1; k < SUB; ++k) v += red[k][j];
  }
  if (!live) return;
  if (r.acc)
    r.dw[o] += v;
  else
    r.dw[o] = v;
}

// bias gradient db[c] = sum over images and pixels of dY[img][c][:], two stages:
// grid (C, parts) partial sums over contiguous slices of the N*HW elements, then per channel.
#if MD2_CONV_PART == 3
__global__ __launch_bounds__(256) void bias_grad_partial_kernel(const float* __restrict__ dy, int C,
                                                                long HW, long total, int parts,
                                                                float* __restrict__ part) {
  __shared__ float red[4];
  const int c = blockIdx.x, p = blockIdx.y;
  const long beg = total * p / parts, end = total * (p + 1) / parts;
  float s = 0.f;
  for (long e = beg + threadIdx.x; e < end; e += 256) {
    const long img = e / HW, pix = e - img * HW;
    s += dy[(img * C + c) * HW + pix];
  }
  float v[1] = {s};
  block_sum256<1>(v, red);
  if (threadIdx.x == 0) part[(long)c * parts + p] = v[0];
}

#endif  // MD2_CONV_PART == 3

static int bias_parts(int C, long total) {
  return (int)std::max(1L, std::min((long)std::max(1, 1024 / C), total / 4096 + 1));
}

#if MD2_CONV_PART == 0
__global__ __launch_bounds__(256) void act_backward_kernel(const float* __restrict__ out,
                                                           const float* __restrict__ dout,
                                                           float* __restrict__ dpre, long n,
                                                           int act) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float o = out[i], g = dout[i];
  float d;
  switch (act) {
    case ACT_RELU: d = o > 0.f ? g : 0.f; break;
    case ACT_ELU: d = o > 0.f ? g : g * (o + 1.f); break;      // elu'(x) = exp(x) = out + 1
    case ACT_SIGMOID: d = g * o * (1.f - o); break;
    default: d = g;
  }
  dpre[i] = d;
}

#endif  // MD2_CONV_PART == 0

// ---------------------------------------------------------------------------------------------
// host side: tile selection, split-K planning, dispatch
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int TARGET_BLOCKS = 1536;  // ~6 blocks (waves per SIMD) per CU on 256 CUs

// T128x64q: 128x64 with the 4 waves stacked along M (each 32 rows x 64 columns: its A rows are its
// own, B shared through LDS)
enum TileCfg { T128x128 = 0, T64x256 = 1, T32x256 = 2, T64x128 = 3, T128x64 = 4, T64x64 = 5, T32x128 = 6,
               T128x64q = 7 };
const int TILE_BM[] = {128, 64, 32, 64, 128, 64, 32, 128};
const int TILE_BN[] = {128, 256, 256, 128, 64, 64, 128, 64};

// debugging / tuning overrides of the planner (read once; honoured only under MD2_TUNING=1,
// common.h tuning_knob): MD2_PX_TILE=<TileCfg>, MD2_PX_TARGET=<target blocks for split-K>, ...
int env_int(const char* name, int dflt) { return tuning_knob(name, dflt); }

struct Plan {
  int tile;
  int BM, BN, BK;
  int splits;
  int kper;
};

Plan plan_px(int M, long N, int K, bool bk32_ok = false, bool prefer32 = false) {
  // Small tiles, many blocks: at B=12 the GEMMs are ~0.5 chip of 128x128 tiles; 64x64 tiles
  // (30 VGPR + 16 AGPR, 8 waves/SIMD) with ~1536 blocks keep 4-6 waves per SIMD in flight and
  // ran 10-50% faster than 128x128 / 64x256 on every encoder shape (tools/sweep_px.sh, r01).
  static const int tile_override = env_int("MD2_PX_TILE", -1);
  static const int target = env_int("MD2_PX_TARGET", TARGET_BLOCKS);
  Plan p{};
  p.tile = M > 32 ? T64x64 : T32x128;
  if (tile_override >= 0 && tile_override <= T128x64q &&
      ((M > 32 && TILE_BM[tile_override] >= 64) || (M <= 32 && TILE_BM[tile_override] == 32)))
    p.tile = tile_override;
  p.BM = TILE_BM[p.tile];
  p.BN = TILE_BN[p.tile];
  static const int bk_override = env_int("MD2_PX_BK", 0);
  p.BK = ((bk_override == 32 || (prefer32 && bk_override != 16)) && bk32_ok) ? 32 : 16;
  if (K <= 0) {                // a parity class without taps: the kernel only writes zeros
    p.splits = 1;
    p.kper = p.BK;
    return p;
  }
  // a split keeps >= MD2_PX_MINCH (default 8) K chunks
  static const int minch = std::max(1, env_int("MD2_PX_MINCH", 8));
  const long tiles = (long)cdiv(M, p.BM) * cdiv(N, p.BN);
  int splits = 1;
  while (tiles * splits * 2 <= target && K / (splits * 2) >= minch * p.BK) splits *= 2;
  p.kper = (int)round_up(cdiv(K, splits), p.BK);
  p.splits = cdiv(K, p.kper);
  return p;
}

// conv_halo3 (conv_halo.inc): stride-1 3x3 zero-padded fwd / dgrad on the bf16x6 products with
// the LDS halo -- 64 x 256 tiles, split over 16-channel chunks until ~2 blocks per CU
// (MD2_HALO=0 with MD2_TUNING=1: conv_px3 instead; MD2_HX_TARGET: target blocks)
struct HaloPlan {
  bool ok = false;
  int items = 0, splits = 1, cper = 1;
  bool d2 = false;   // the 2D-tile kernel (conv_halo2d_kernel): 8 x 32 pixel tiles, mw = M tiles of 32 per block
  int mw = 2;
};
HaloPlan plan_halo(const ConvShape& s, int mode) {
  HaloPlan h;
  static const int on = env_int("MD2_HALO", 1);
  static const int target = env_int("MD2_HX_TARGET", 256);   // blocks: one round of 512-thread blocks (one per CU); 512: 2 rounds, 2-10% slower on layers 3-4
  // reflect padding (the decoder blocks): forward only -- the dgrad's reflect adjoint folds the
  // border rows and columns back (conv_px3's border gathers)
  if (!on || mode > 1 || s.KH != 3 || s.KW != 3 || s.stride != 1 || s.pad != 1 || (s.reflect && mode == 1)) return h;
  if (!conv_px3_used(s, mode) || !conv_tap_major(s, mode)) return h;
  const int M = mode == 0 ? s.Cout : s.Cin, C = mode == 0 ? s.Cin : s.Cout;
  if (C % 16 || s.cin_w) return h;
  const int hrmax = Halo3Lds::rows(s.W);                 // halo rows of 256 consecutive pixels
  const bool flat = M % 64 == 0 && Halo3Lds::fits(s.W) && cdiv((long)hrmax * s.W, 512) <= 2;
  // otherwise the 2D-tile kernel (maps too wide for the flattened image, 32-row M tiles;
  // bf16x6 only).  MD2_HALO2D (MD2_TUNING=1): bit 0 forward (default), bit 1 data gradient --
  // the reflect dgrad on it (the padded 66 x 210 grid in 8 x 32 tiles + the fold) measured
  // 6.532 vs 6.488 ms per step against conv_px3's direct reflect gathers (3 interleaved triples)
  static const int d2on = env_int("MD2_HALO2D", 1);
  const bool d2 = !flat && (d2on >> mode & 1) && M % 32 == 0 && tuning_knob("MD2_PX3_TERMS", 6) != 9 &&
                  2L * s.H * s.W >= (long)round_up(s.H, 8) * round_up(s.W, 32);   // tiles >= half full
  if (!flat && !d2) return h;
  long tiles;
  int tgt = target;
  if (flat) {
    h.items = cdiv((long)hrmax * s.W, 512);               // staged pixels per thread (512 threads)
    tiles = (long)(M / 64) * cdiv((long)s.N * s.H * s.W, 256);
  } else {
    h.d2 = true;
    h.mw = M % 64 == 0 ? 2 : 1;
    tiles = (long)(M / (32 * h.mw)) * s.N * cdiv(s.H, 8) * cdiv(s.W, 32);
    tgt = h.mw == 1 ? 2 * target : target;                // 4-wave blocks: two per CU
  }
  const int nch = C / 16;
  int splits = 1;
  while (tiles * splits * 2 <= tgt && nch / (splits * 2) >= 2) splits *= 2;
  h.cper = cdiv(nch, splits);
  h.splits = cdiv(nch, h.cper);
  h.ok = true;
  return h;
}

// conv_halo3s2 (conv_halo.inc): the stride-2 3x3 data gradient, all four output-parity classes
// of dX from one staged dY image per 16-channel chunk; 64 x 128 tiles over the dY grid, split
// over chunks to ~256 blocks (MD2_HALO_S2=0 with MD2_TUNING=1: conv_px3's merged classes)
struct HaloS2Plan {
  bool ok = false;
  int items = 0, splits = 1, cper = 1;
};
HaloS2Plan plan_halo_s2(const ConvShape& s) {
  HaloS2Plan h;
  static const int on = env_int("MD2_HALO_S2", 1);
  if (!on || s.KH != 3 || s.KW != 3 || s.stride != 2 || s.pad != 1 || s.reflect || s.cin_w) return h;
  if (s.H != 2 * s.Ho || s.W != 2 * s.Wo || s.Cin % 64 || s.Cout % 16) return h;
  if (!conv_px3_used(s, 1) || !conv_tap_major(s, 1) || tuning_knob("MD2_PX3_TERMS", 6) == 9) return h;
  if (!Halo3s2Lds::fits(s.Wo)) return h;                 // (then <= 413 staged pixels: one per thread)
  h.items = 1;
  const long tiles = (long)(s.Cin / 64) * cdiv((long)s.N * s.Ho * s.Wo, 128);
  const int nch = s.Cout / 16;
  int splits = 1;
  while (tiles * splits * 2 <= 256 && nch / (splits * 2) >= 2) splits *= 2;
  h.cper = cdiv(nch, splits);
  h.splits = cdiv(nch, h.cper);
  h.ok = true;
  return h;
}

// conv_whalo (conv_halo.inc): stride-1 3x3 zero-padded filter gradient on the LDS halo, 64
// filters x 32 channels x 9 taps per block, K in chunks of r whole rows (r | H, r * W <= 112),
// split to ~MD2_WHX_TARGET (256) blocks with >= 2 chunks each (MD2_WHALO=0: off)
struct WHaloPlan {
  bool ok = false;
  int r = 0, items = 0, nchunk = 0, splits = 1, cper = 1;
};
WHaloPlan plan_whalo(const ConvShape& s, int c0) {
  WHaloPlan h;
  static const int on = env_int("MD2_WHALO", 1);
  static const int target = env_int("MD2_WHX_TARGET", 256);   // 128 / 192 / 384 / 512: 7.05 / 6.89 / 6.83 / 6.76 vs 6.69 ms per step (profiles/r05_whalo_ab.txt)
  if (!on || s.KH != 3 || s.KW != 3 || s.stride != 1 || s.pad != 1 || s.reflect) return h;
  if (s.Cin % 32 || s.Cout % 64 || c0 < s.Cin || (s.cin_w && s.cin_w != s.Cin) || s.W > 112) return h;
  if (tuning_knob("MD2_PX3_TERMS", 6) == 9) return h;     // the 9-product variant: conv_wgrad_px3
  int r = 0;
  for (int d = 1; d <= s.H; ++d)
    if (s.H % d == 0 && d * s.W <= 112) r = d;
  // (16-byte dY loads of 4-pixel groups: chunk starts and image planes on 4-float boundaries)
  // (and 4..7 16-pixel k-steps per chunk: the X staging rides behind the first four)
  if (r == 0 || (r * s.W) % 4 || (s.H * s.W) % 4 || r * s.W < 49) return h;
  if (!WHaloLds::fits(r, s.W)) return h;
  // (4 staged items -- layer 1's 104-wide rows -- take 198 VGPRs, one 6-wave block per CU: 91 vs
  // 81 us against conv_wgrad_px3 until the staging loads' per-lane soffset (a waterfall loop) was
  // moved into the voffset; since then 77 vs 88 us, the step 6.145 vs 6.205 ms;
  // profiles/r05_whalo_ab.txt.  MD2_WHX_MAXITEMS=3 leaves layer 1 to conv_wgrad_px3)
  static const int maxit = env_int("MD2_WHX_MAXITEMS", 4);
  h.items = cdiv(4L * (r + 2) * s.W, 384);
  if (h.items > std::min(4, maxit)) return h;
  h.r = r;
  h.nchunk = s.N * s.H / r;
  const long tiles = (long)(s.Cin / 32) * (s.Cout / 64);
  long splits = std::max(1L, (long)target / tiles);
  splits = std::min(splits, std::max(1L, (long)h.nchunk / 2));
  h.cper = cdiv(h.nchunk, splits);
  h.splits = cdiv(h.nchunk, h.cper);
  h.ok = true;
  return h;
}

// reflect-padded 3x3 dgrad (the decoder blocks) on the halo kernel: the zero-padded same-size
// dgrad of the (H+2) x (W+2) grid (conv_halo3 EXT) into a workspace image, then the fold
ConvShape reflect_ext_shape(const ConvShape& s) {
  ConvShape e = s;
  e.H = s.H + 2;
  e.W = s.W + 2;
  e.Ho = e.H;
  e.Wo = e.W;
  e.reflect = 0;
  return e;
}
bool reflect_dgrad_on_halo(const ConvShape& s, HaloPlan* hp = nullptr) {
  static const int on = env_int("MD2_HALO_RFL_DGRAD", 1);
  if (!on || !s.reflect || s.KH != 3 || s.stride != 1 || s.pad != 1 || s.cin_w || s.H < 2 || s.W < 2) return false;
  const HaloPlan h = plan_halo(reflect_ext_shape(s), 1);
  if (hp) *hp = h;
  return h.ok;
}
size_t reflect_dgrad_ws(const ConvShape& s) {
  HaloPlan h;
  if (!reflect_dgrad_on_halo(s, &h)) return 0;
  const long Ne = (long)s.N * (s.H + 2) * (s.W + 2);
  return ((size_t)(h.splits > 1 ? h.splits : 0) + 1) * s.Cin * Ne * sizeof(float);
}

// wgrad tiles (BM x BN, 4 waves as WM x WN); columns are tap-major (tap groups x CW channels)
enum WTileCfg { W64x128 = 0, W32x256 = 1, W64x64 = 2, W32x128 = 3, W16x144 = 4, WSTEM = 5, W64x192 = 6 };
const int WT_BM[] = {64, 32, 64, 32, 16, 64, 64};
const int WT_BN[] = {128, 256, 64, 128, 144, 64, 192};

struct WPlan {
  int tile, BM, BN;
  int cw;          // channels per tap block (0: channel-major kernel)
  long ntiles_n;   // column tiles
  int splits, kper;
};

// channels per tap block of the tap-major wgrad: largest of 128/64/32/16 (<= BN) dividing Cin and
// the concat split
int wgrad_cw(const ConvShape& s, int c0, int BN) {
  for (int cw = 128; cw >= 16; cw /= 2)
    if (cw <= BN && s.Cin % cw == 0 && (c0 >= s.Cin || c0 % cw == 0)) return cw;
  return 0;
}

WPlan plan_wgrad(const ConvShape& s, int c0) {
  static const int tile_override = env_int("MD2_W_TILE", -1);
  static const int target = env_int("MD2_W_TARGET", 0);
  WPlan p{};
  // Cout <= 16 * MD2_W16 (1, 2 or 4; default 2), 3x3 stride 1, tap-major with 16-channel
  // groups: conv_wgrad16_kernel (MD2_W16=0 falls back to the 32x128 tiles; MD2_W16_TARGET =
  // blocks to split K towards)
  // the ResNet stem (7x7/2, <= 4 image channels, 64 filters): conv_wgrad_stem_kernel, split-K
  // over all output pixels to ~MD2_WSTEM_TARGET blocks (MD2_WSTEM=0: the generic tiles)
  static const int wstem = env_int("MD2_WSTEM", 1);
  static const int tstem = env_int("MD2_WSTEM_TARGET", 512);
  if (wstem && s.KH == 7 && s.KW == 7 && s.stride == 2 && !s.reflect && s.Cin <= 4 && s.Cout == 64 &&
      c0 >= s.Cin) {
    p.tile = WSTEM;
    p.BM = 64;
    p.BN = s.Cin * 49;
    p.cw = 0;
    p.ntiles_n = 1;
    const long K = (long)s.N * s.Ho * s.Wo;
    long splits = std::min((long)tstem, std::max(1L, K / (4 * 64)));
    p.kper = (int)round_up((K + splits - 1) / splits, 64);
    p.splits = (int)((K + p.kper - 1) / p.kper);
    return p;
  }
  static const int w16 = env_int("MD2_W16", 2);
  static const int t16 = env_int("MD2_W16_TARGET", 512);
  if (w16 && s.Cout <= 16 * w16 && s.KH == 3 && s.KW == 3 && s.stride == 1 && conv_tap_major(s, 2) &&
      s.Cin % 16 == 0 && (c0 >= s.Cin || c0 % 16 == 0)) {
    p.tile = W16x144;
    p.BM = s.Cout > 32 ? 64 : s.Cout > 16 ? 32 : 16;
    p.BN = 144;
    p.cw = 16;
    p.ntiles_n = s.Cin / 16;
    const long K = (long)s.N * s.Ho * s.Wo;
    long splits = std::max(1L, (long)t16 / p.ntiles_n);
    splits = std::min(splits, std::max(1L, K / (4 * 64)));
    p.kper = (int)round_up((K + splits - 1) / splits, 64);
    p.splits = (int)((K + p.kper - 1) / p.kper);
    return p;
  }
  const int M = s.Cout;
  const int KK = s.KH * s.KW;
  auto ntiles = [&](int tile, int& cw) {
    cw = conv_tap_major(s, 2) ? wgrad_cw(s, c0, WT_BN[tile]) : 0;
    const long nt = cw ? (long)cdiv(KK, WT_BN[tile] / cw) * (s.Cin / cw) : cdiv((long)s.Cin * KK, WT_BN[tile]);
    return (long)cdiv(M, WT_BM[tile]) * nt;
  };
  // M <= 32: 32x128 (1024 blocks); else 64x128 with split-K to ~512 blocks, or 64x64 when the
  // grid is already >= 256 tiles without splitting (tools/sweep_w.sh, r01)
  int tgt = 512;
  if (M <= 32) {
    p.tile = W32x128;
    tgt = 1024;
  } else {
    int cw;
    p.tile = ntiles(W64x128, cw) >= 256 ? W64x64 : W64x128;
    static const int t64 = env_int("MD2_W64_TARGET", 1728);
    if (p.tile == W64x64) tgt = t64;
    // channel-major (the 3-channel 7x7 stem, 147 columns): 64-wide column tiles pad 147 to 192
    // instead of 256 (MD2_W_CM64=1: on -- measured neutral-to-slower, off by default)
    static const int cm64 = env_int("MD2_W_CM64", 0);
    static const int cmt = env_int("MD2_W_CM_TARGET", 768);
    const long ncol = (long)s.Cin * KK;
    if (cm64 && cw == 0 && p.tile == W64x128 && round_up(ncol, 64) < round_up(ncol, 128)) {
      p.tile = W64x64;
      tgt = cmt;
    }
  }
  // 64-channel 3x3 tap-major convs: 64x128 tiles hold 2 taps, so the 9 taps take 5 column tiles
  // with one tap slot in ten idle; 64x192 tiles (3 taps x 64 channels, TN = 3) cover them in 3
  // with no idle column (MD2_W192=0: off)
  static const int w192 = env_int("MD2_W192", 1);
  if (w192 && p.tile == W64x128 && KK == 9 && conv_tap_major(s, 2) && wgrad_cw(s, c0, 128) == 64 &&
      wgrad_cw(s, c0, 192) == 64)
    p.tile = W64x192;
  if (tile_override >= 0 && tile_override <= W32x128) p.tile = tile_override;
  if (target > 0) tgt = target;
  p.BM = WT_BM[p.tile];
  p.BN = WT_BN[p.tile];
  const long tiles = ntiles(p.tile, p.cw);
  p.ntiles_n = tiles / cdiv(M, p.BM);
  const long K = (long)s.N * s.Ho * s.Wo;
  const int BK = 32;
  static const int minch = std::max(1, env_int("MD2_W_MINCH", 4));   // K chunks per split, at least (8 -> 4: +0.6% step, tools/minch_sweep.sh)
  long splits = std::max(1L, (long)tgt / tiles);
  splits = std::min(splits, std::max(1L, K / (minch * BK)));
  p.kper = (int)round_up((K + splits - 1) / splits, BK);
  p.splits = (int)((K + p.kper - 1) / p.kper);
  return p;
}

void fill_common(ConvArgs& a, const ConvShape& s) {
  static const int xcd = env_int("MD2_XCD", 0);
  a.xcd = xcd;
  a.Cin = s.Cin; a.H = s.H; a.W = s.W; a.Cout = s.Cout; a.Ho = s.Ho; a.Wo = s.Wo;
  a.stride = s.stride; a.pad = s.pad;
  a.HW = (long)s.H * s.W;
  a.HoWo = (long)s.Ho * s.Wo;
  a.HW4 = (uint32_t)(a.HW * 4);
  a.HoWo4 = (uint32_t)(a.HoWo * 4);
}

int check_shape(const ConvShape& s) {
  MD2_CHECK_ARG(s.N > 0 && s.Cin > 0 && s.Cout > 0 && s.H > 0 && s.W > 0, "conv dims");
  MD2_CHECK_ARG(s.KH == s.KW && (s.KH == 1 || s.KH == 3 || s.KH == 7), "kernel size 1/3/7");
  MD2_CHECK_ARG(s.stride == 1 || s.stride == 2, "stride 1/2");
  MD2_CHECK_ARG(s.Ho == (s.H + 2 * s.pad - s.KH) / s.stride + 1 &&
                    s.Wo == (s.W + 2 * s.pad - s.KW) / s.stride + 1, "output size");
  MD2_CHECK_ARG(!s.reflect || (s.KH == 3 && s.stride == 1 && s.pad == 1 && s.H >= 2 && s.W >= 2),
                "reflect padding needs 3x3/1 pad 1");
  MD2_CHECK_ARG((long)s.N * s.H * s.W < (1L << 31) && (long)s.N * s.Ho * s.Wo < (1L << 31),
                "pixel count");
  MD2_CHECK_ARG(s.cin_w >= 0 && s.cin_w <= s.Cin && (s.cin_w == 0 || s.Cout > 1),
                "weight channels (cin_w) must be <= Cin (and no padded head convs)");
  return MD2_OK;
}

// (KH, S, RFL) combos instantiated
#define MD2_CONV_COMBOS(X) X(1, 1, 0) X(1, 2, 0) X(3, 1, 0) X(3, 1, 1) X(3, 2, 0) X(7, 2, 0)

// the bf16x9 kernel runs 16-deep chunks even where the planner asks for 32 (the stride-2 dgrad):
// its BK=32 form was measured 98 vs 69 us per layer-2..4 stride-2 dgrad and 3-8% slower elsewhere
static int px3_terms() {
  static const int t = tuning_knob("MD2_PX3_TERMS", 6) == 9 ? 9 : 6;
  return t;
}

template <int MODE, int BM, int BN, int WM, int WN>
int launch_px_tile(const ConvShape& s, const ConvArgs& a, bool tap, int bk, dim3 grid, hipStream_t st) {
  const bool v2 = conv_px2_used(s, MODE);
  const bool v3 = conv_px3_used(s, MODE);
#define MD2_PX_CASE(KS, SS, RR)                                                                  \
  if (s.KH == KS && s.stride == SS && s.reflect == RR) {                                         \
    if constexpr (BM >= 32 && BN % 64 == 0 && WM * WN == 4) {                                    \
      if (v3) {                                                                                  \
        conv_arith_ref() = 6;                                                                    \
        if (px3_terms() == 6)                                                                    \
          hipLaunchKernelGGL((conv_px3_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 16, 6>), grid, \
                             dim3(256), 0, st, a);                                               \
        else                                                                                     \
          hipLaunchKernelGGL((conv_px3_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 16, 9>), grid, \
                             dim3(256), 0, st, a);                                               \
        MD2_LAUNCH_CHECK();                                                                      \
        return MD2_OK;                                                                           \
      }                                                                                          \
    }                                                                                            \
    if constexpr (BM >= 64 && BN % 64 == 0) {                                                    \
      if (v2) {                                                                                  \
        conv_arith_ref() = 1;                                                                    \
        if (bk == 32)                                                                            \
          hipLaunchKernelGGL((conv_px2_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 32>), grid,  \
                             dim3(256), 0, st, a);                                               \
        else                                                                                     \
          hipLaunchKernelGGL((conv_px2_kernel<MODE, BM, BN, WM, WN, KS, KS, SS, RR, 16>), grid,  \
                             dim3(256), 0, st, a);                                               \
        MD2_LAUNCH_CHECK();                                                                      \
        return MD2_OK;                                                                           \
      }                                                                                          \
    }                                                                                            \
    if (v2) {                                                                                    \
      set_error("conv: k-contiguous kernel needs a tile with BM >= 64");                         \
      return MD2_EINVAL;                                                                         \
    }                                                                                            \
    conv_arith_ref() = 1;                                                                        \
    if (tap && bk == 32)                                                                         \
      hipLaunchKernelGGL((conv_px_kernel<MODE, 1, BM, BN, 32, WM, WN, KS, KS, SS, RR>), grid,    \
                         dim3(256), 0, st, a);                                                   \
    else if (tap)                                                                                \
      hipLaunchKernelGGL((conv_px_kernel<MODE, 1, BM, BN, 16, WM, WN, KS, KS, SS, RR>), grid,    \
                         dim3(256), 0, st, a);                                                   \
    else                                                                                         \
      hipLaunchKernelGGL((conv_px_kernel<MODE, 0, BM, BN, 16, WM, WN, KS, KS, SS, RR>), grid,    \
                         dim3(256), 0, st, a);                                                   \
    MD2_LAUNCH_CHECK();                                                                          \
    return MD2_OK;                                                                               \
  }
  MD2_CONV_COMBOS(MD2_PX_CASE)
#undef MD2_PX_CASE
  set_error("conv: unsupported (kernel, stride, padding) combination");
  return MD2_ENOTSUP;
}

// M <= 16 convs on the 16x16x4 MFMA kernel (conv_px16.inc): no split-K, BN 128 (6 blocks per CU
// by LDS; BN 256 ran 20% slower on the full-resolution branch)
template <int MODE>
int launch_px16(const ConvShape& s, ConvArgs& a, hipStream_t st) {
  a.slab = nullptr;
  conv_arith_ref() = 1;
  a.g.kper = (int)round_up(a.g.K, 16);
  static const int bn = env_int("MD2_PX16_BN", 128);   // 128 measured faster on every decoder shape
  const bool big = bn == 256;
  const dim3 grid(cdiv(a.g.N, big ? 256 : 128));
#define MD2_P16_CASE(KS, SS, RR)                                                                 \
  if constexpr (SS == 1) {                                                                       \
    if (s.KH == KS && s.stride == SS && s.reflect == RR) {                                       \
      if (big)                                                                                   \
        hipLaunchKernelGGL((conv_px16_kernel<MODE, 256, KS, KS, SS, RR>), grid, dim3(256), 0, st, a); \
      else                                                                                       \
        hipLaunchKernelGGL((conv_px16_kernel<MODE, 128, KS, KS, SS, RR>), grid, dim3(256), 0, st, a); \
      MD2_LAUNCH_CHECK();                                                                        \
      return MD2_OK;                                                                             \
    }                                                                                            \
  }
  MD2_P16_CASE(3, 1, 0) MD2_P16_CASE(3, 1, 1)
#undef MD2_P16_CASE
  set_error("conv: 16-row kernel supports 3x3 stride 1 only");
  return MD2_ENOTSUP;
}

template <int MODE>
int launch_px(const ConvShape& s, ConvArgs& a, const Plan& p_in, ConvWorkspace ws, hipStream_t st,
              SplitKDefer* defer = nullptr) {
  double* const stats = defer ? defer->stats : nullptr;
  const bool keep_reduce = defer && defer->keep_reduce;
  if (defer) *defer = SplitKDefer{};
  if (conv_px16_used(s, MODE)) return launch_px16<MODE>(s, a, st);
  // the LDS-halo kernel where it applies (plain input: one tensor, no frame-strided images)
  HaloPlan hp = plan_halo(s, MODE);
  // (forward input: no frame-strided images; a concat split on a 16-channel chunk boundary)
  if (hp.ok && MODE == 0 && (a.in.bdiv < s.N || (a.in.p1 && a.in.c0 < s.Cin && a.in.c0 % 16))) hp.ok = false;
  Plan p = p_in;
  if (hp.ok) {
    p.splits = hp.splits;
    p.kper = hp.cper * 16;   // only the slab count matters below
  }
  a.g.kper = p.kper;
  a.slab = nullptr;
  if (p.splits > 1) {
    const size_t need = (size_t)p.splits * a.g.M * a.g.N * sizeof(float);
    MD2_CHECK_ARG(ws.ptr && ws.bytes >= need, "conv split-K workspace too small");
    a.slab = (float*)ws.ptr;
  }
  const int ncls = (MODE == 1 && a.ph_S > 0) ? 4 : 1;   // merged stride-2 dgrad classes
  if (ncls > 1) {
    a.ph_S = p.splits;
    MD2_CHECK_ARG(p.splits == 1 || (ws.ptr && ws.bytes >= 4 * (size_t)p.splits * a.g.M * a.g.N * sizeof(float)),
                  "conv split-K workspace too small");
  }
  dim3 grid(cdiv(a.g.N, p.BN), cdiv(a.g.M, p.BM), p.splits * ncls);
  const bool tap = conv_tap_major(s, MODE);
  int rc;
  if (hp.ok && ncls == 1) {
    a.hx_cper = hp.cper;
    // BN statistics in the epilogue: forward, no split-K, a plain contiguous output
    const TensorOut& oo = a.out;
    const bool bnst = MODE == 0 && stats && !hp.d2 && hp.splits == 1 && !s.reflect && !oo.bias && oo.act == ACT_NONE &&
                      !oo.accumulate && oo.c0 >= a.g.M && oo.bs0 == (long)a.g.M * a.fd_pix.d;
    a.bn_part = bnst ? stats : nullptr;
    conv_arith_ref() = 6;
    rc = hp.d2 ? halo2d_launch(MODE, a, hp.mw, hp.splits, s.reflect, st)
               : halo_launch(MODE, a, hp.items, hp.splits, s.reflect, st);
    a.bn_part = nullptr;
    if (rc == MD2_OK && bnst) {
      defer->stats = stats;
      defer->stats_parts = (int)cdiv(a.g.N, 256);
    }
  } else switch (p.tile) {
    case T128x128: rc = launch_px_tile<MODE, 128, 128, 2, 2>(s, a, tap, p.BK, grid, st); break;
    case T64x256: rc = launch_px_tile<MODE, 64, 256, 1, 4>(s, a, tap, p.BK, grid, st); break;
    case T64x128: rc = launch_px_tile<MODE, 64, 128, 2, 2>(s, a, tap, p.BK, grid, st); break;
    case T128x64: rc = launch_px_tile<MODE, 128, 64, 2, 2>(s, a, tap, p.BK, grid, st); break;
    case T64x64: rc = launch_px_tile<MODE, 64, 64, 2, 2>(s, a, tap, p.BK, grid, st); break;
    case T32x128: rc = launch_px_tile<MODE, 32, 128, 1, 4>(s, a, tap, p.BK, grid, st); break;
    case T128x64q: rc = launch_px_tile<MODE, 128, 64, 4, 1>(s, a, tap, p.BK, grid, st); break;
    default: rc = launch_px_tile<MODE, 32, 256, 1, 4>(s, a, tap, p.BK, grid, st); break;
  }
  if (rc) return rc;
  const TensorOut& o = a.out;
  if (defer && !keep_reduce && p.splits > 1 && ncls == 1 && (MODE == 0 || s.stride == 1) && !o.bias && o.act == ACT_NONE &&
      !o.accumulate && o.c0 >= a.g.M && o.bs0 == (long)a.g.M * a.fd_pix.d) {
    defer->slab = a.slab;
    defer->splits = p.splits;
    return MD2_OK;
  }
  const int phase = (int)(MODE == 1 && s.stride == 2 && conv_tap_major(s, 1));
  const bool aligned4 = a.fd_pix.d % 4 == 0 && o.bs0 % 4 == 0 && (!o.p1 || o.bs1 % 4 == 0) &&
                        ((uintptr_t)o.p0 % 16) == 0 && (!o.p1 || ((uintptr_t)o.p1 % 16) == 0);
  if (p.splits > 1 && ncls == 1 && !phase && aligned4) {
    const long total4 = (long)a.g.M * a.g.N / 4;
    hipLaunchKernelGGL(splitk_reduce_px4_kernel<0>, dim3(cdiv(total4, 256)), dim3(256), 0, st, a,
                       p.splits);
    MD2_LAUNCH_CHECK();
    return MD2_OK;
  }
  if (p.splits > 1) {
    const long total = (long)a.g.M * a.g.N * ncls;
    MD2_CHECK_ARG(total < (1L << 31), "conv: split-K reduction index exceeds 2^31");
    hipLaunchKernelGGL(splitk_reduce_px_kernel<0>, dim3(cdiv(total, 256)), dim3(256), 0, st, a, p.splits,
                       (int)(MODE == 1 && s.stride == 2 && conv_tap_major(s, 1)),
                       make_fastdiv((uint32_t)a.g.N), make_fastdiv((uint32_t)((long)a.g.M * a.g.N)));
    MD2_LAUNCH_CHECK();
  }
  return MD2_OK;
}

// the tap-major wgrad on the bf16 split-product MFMA (conv_wpx3.inc) wherever its pixel pairs fit:
// CW % 32 == 0 and an even pixel count per image (MD2_WPX3=0 with MD2_TUNING=1: the fp32 kernel)
static bool wgrad_px3_on() {
  static const int v = tuning_knob("MD2_WPX3", 1);
  return v != 0;
}

template <int BM, int BN, int WM, int WN, int KS, int SS, int RR, int CW, int PX>
void launch_wpx3(const ConvArgs& a, dim3 grid, hipStream_t st) {
  if (px3_terms() == 6)
    hipLaunchKernelGGL((conv_wgrad_px3_kernel<BM, BN, WM, WN, KS, KS, SS, RR, CW, 6, PX>), grid,
                       dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv_wgrad_px3_kernel<BM, BN, WM, WN, KS, KS, SS, RR, CW, 9, PX>), grid,
                       dim3(256), 0, st, a);
}

template <int BM, int BN, int WM, int WN, int KS, int SS, int RR, int CW>
void launch_w_cw(const ConvArgs& a, dim3 grid, hipStream_t st) {
  // pixel pairs per lane (conv_wpx3.inc; 4 pixels per lane with 16-byte loads measured no faster
  // on the stride-1 layers and 30% slower on the stride-2 ones, profiles/r04_wgrad_px3.txt)
  if constexpr (CW <= BN && CW % 32 == 0 && BM % 32 == 0 && BN % 32 == 0) {
    if (wgrad_px3_on() && a.HoWo % 2 == 0) {
      conv_arith_ref() = 6;
      launch_wpx3<BM, BN, WM, WN, KS, SS, RR, CW, 2>(a, grid, st);
      return;
    }
  }
  conv_arith_ref() = 1;
  if constexpr (CW <= BN)
    hipLaunchKernelGGL((conv_wgrad_tap_kernel<BM, BN, 32, WM, WN, KS, KS, SS, RR, CW>), grid,
                       dim3(256), 0, st, a);
}

template <int BM, int BN, int WM, int WN, int KS, int SS, int RR>
int launch_w(int cw, const ConvArgs& a, dim3 grid, hipStream_t st) {
  switch (cw) {
    case 0:
      conv_arith_ref() = 1;
      hipLaunchKernelGGL((conv_wgrad_kernel<BM, BN, 32, WM, WN, KS, KS, SS, RR>), grid, dim3(256), 0,
                         st, a);
      break;
    case 16: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 16>(a, grid, st); break;
    case 32: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 32>(a, grid, st); break;
    case 64: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 64>(a, grid, st); break;
    case 128: launch_w_cw<BM, BN, WM, WN, KS, SS, RR, 128>(a, grid, st); break;
    default: return MD2_ENOTSUP;
  }
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

// stride-2 dgrad output-parity class (cy, cx): input pixels iy = y0 + 2j with (iy + pad) % 2 ==
// cy receive exactly the taps kh % 2 == cy (same for columns)
struct PhaseClass {
  int y0, x0, Hc, Wc, ntaps;
  int taps[16];
};

PhaseClass phase_class(const ConvShape& s, int cy, int cx) {
  PhaseClass c{};
  c.y0 = (cy + s.pad) & 1;
  c.x0 = (cx + s.pad) & 1;
  c.Hc = (s.H - c.y0 + 1) / 2;
  c.Wc = (s.W - c.x0 + 1) / 2;
  static_assert(sizeof(c.taps) / sizeof(c.taps[0]) >= 16, "taps of a 7x7 class");
  for (int kh = cy; kh < s.KH; kh += 2)
    for (int kw = cx; kw < s.KW; kw += 2) c.taps[c.ntaps++] = kh * s.KW + kw;
  return c;
}

}  // namespace

#if MD2_CONV_PART == 0
// the k-contiguous kernel (conv_px2.inc) runs every tap-major fwd / dgrad with M > 32 (tiles with
// BM >= 64); MD2_PX_V2=0 selects the previous kernel (A/B)
bool conv_px2_used(const ConvShape& s, int mode) {
  static const int v2 = tuning_knob("MD2_PX_V2", 1);
  if (!v2 || mode > 1 || !conv_tap_major(s, mode)) return false;
  return (mode == 0 ? s.Cout : s.Cin) > 32;
}
// the exact-product bf16 kernel (conv_px3.inc) takes the conv_px2 shapes (MD2_PX3=0: conv_px2)
// bf16x9 (conv_px3) vs exact-fp32 MFMA (conv_px2) on the conv_px2 shapes: the bf16x9 kernel has
// 1.78x less MFMA time per K chunk but more VALU (the B split); in the train step it is faster on
// every conv_px2 shape (interleaved A/B at B=12, 3 x 60 steps: 1565 vs 1540 images/s with the
// 8x26 / 4x13 maps left on conv_px2, 1488 all conv_px2; profiles/r04_px3_ab.txt -- the op-level
// per-layer times there include the per-call weight split, which makes the layer-4 shapes look
// slower in isolation).  Its products are exact and its sums fp32: 3x lower error vs fp64 than the
// fp32 MFMA kernel (same file).
// MD2_PX3 (with MD2_TUNING=1): 0 = conv_px2 everywhere, 1 = conv_px3 on every conv_px2 shape
// (default), -1 = conv_px3 only where the GEMM's per-image N pixels >= 512.
bool conv_px3_used(const ConvShape& s, int mode) {
  static const int v3 = tuning_knob("MD2_PX3", 1);
  if (!v3) return false;
  if (!conv_px2_used(s, mode)) {
    // the 32-row forward tiles too (Cout in (16, 32], stride 1: the decoder's Cout = 32 convs,
    // otherwise on the fp32 conv_px kernel): d4c2 forward 127.6 -> 114.9 us; the Cin = 32 data
    // gradients (K = 144) ran slower (34 -> 51 us) and stay (MD2_PX3_M32=0: off)
    static const int m32 = tuning_knob("MD2_PX3_M32", 1);
    if (!m32 || mode != 0 || !conv_tap_major(s, mode) || s.stride != 1) return false;
    const int M = mode == 0 ? s.Cout : s.Cin;
    return M > 16 && M <= 32;
  }
  if (v3 > 0) return true;
  const long pix = mode == 0 ? (long)s.Ho * s.Wo : (long)s.H * s.W;
  return pix >= 512;
}

bool conv_tap_major(const ConvShape& s, int mode) {
  // MD2_CONV_CHANNEL_MAJOR=<bitmask of modes> forces the channel-major order (debugging)
  static const int forced = tuning_knob("MD2_CONV_CHANNEL_MAJOR", 0);
  if (forced & (1 << mode)) return false;
  switch (mode) {
    case 0: return s.Cin % 16 == 0;                                   // px chunk BK = 16
    case 1: return s.Cout % 16 == 0 && (!s.reflect || (s.H != 3 && s.W != 3));
    default: return s.Cin % 16 == 0;                                  // wgrad CW >= 16
  }
}

#endif  // MD2_CONV_PART == 0

// Cout = 1 3x3 convs (disparity heads) run the VALU kernels of head.hip; MD2_HEAD=0 disables
static bool head_path(const ConvShape& s) {
  static const int on = tuning_knob("MD2_HEAD", 1);
  return on && head_conv_ok(s);
}
// tap (c, t) of the packed operand: forward rows m = 0, k = t*Cin + c or c*9 + t; dgrad
// k = co*9 + t = t (Cout = 1, channel-major), row c
static HeadW head_w(const ConvShape& s, int mode, const float* packed) {
  HeadW w{packed, 0, 0};
  if (mode == 0) {
    const long Mpad = round_up(s.Cout, MPAD);
    if (conv_tap_major(s, 0)) { w.sc = Mpad; w.st = (long)s.Cin * Mpad; }
    else { w.sc = 9 * Mpad; w.st = Mpad; }
  } else {
    w.sc = 1;
    w.st = round_up(s.Cin, MPAD);
  }
  return w;
}
static HeadIn head_in(const TensorIn& x) { return HeadIn{x.p0, x.bs0, x.bdiv, x.bhi}; }
#if MD2_CONV_PART == 0
HeadIn conv_head_in(const TensorIn& x) { return head_in(x); }
HeadW conv_head_w(const ConvShape& s, int mode, const float* packed) { return head_w(s, mode, packed); }
#endif

#if MD2_CONV_PART == 0
// the 16-row kernel (conv_px16.inc) runs tap-major 3x3 / stride-1 fwd (Cout <= 16, not a Cout = 1
// head) and dgrad (Cin <= 16); MD2_PX16=0 falls back to the 32-row tiles
bool conv_px16_used(const ConvShape& s, int mode) {
  // bit 0: forward, bit 1: dgrad (off: the 32-row tile's dgrad measured as fast, 99 vs 103 us)
  static const int on = env_int("MD2_PX16", 1);
  if (mode > 1 || !(on & (1 << mode)) || !conv_tap_major(s, mode) || s.KH != 3 || s.stride != 1) return false;
  const int M = mode == 0 ? s.Cout : s.Cin;
  if (M > 16) return false;
  return !(mode == 0 && head_path(s));
}
#endif

#if MD2_CONV_PART == 0

size_t conv_fwd_workspace(const ConvShape& s) {
  const long N = (long)s.N * s.Ho * s.Wo;
  const Plan p = plan_px(s.Cout, N, s.Cin * s.KH * s.KW);   // BK does not change the split count
  const HaloPlan h = plan_halo(s, 0);
  const int splits = std::max(p.splits, h.ok ? h.splits : 1);
  return splits > 1 ? (size_t)splits * s.Cout * N * sizeof(float) : 0;
}

size_t conv_dgrad_workspace(const ConvShape& s) {
  const HaloS2Plan h2 = plan_halo_s2(s);
  if (h2.ok) return h2.splits > 1 ? (size_t)h2.splits * s.Cin * s.N * s.H * s.W * sizeof(float) : 0;
  if (s.stride == 2 && conv_tap_major(s, 1) && conv_px2_used(s, 1) && s.KH <= 3 && s.H % 2 == 0 &&
      s.W % 2 == 0) {
    const long N = (long)s.N * (s.H / 2) * (s.W / 2);
    const Plan p = plan_px(s.Cin, 4 * N, ((s.KH + 1) / 2) * ((s.KW + 1) / 2) * s.Cout, s.Cout % 32 == 0, true);
    return p.splits > 1 ? 4 * (size_t)p.splits * s.Cin * N * sizeof(float) : 0;
  }
  if (s.stride == 2 && conv_tap_major(s, 1)) {
    size_t b = 0;
    for (int cls = 0; cls < 4; ++cls) {
      const PhaseClass c = phase_class(s, cls >> 1, cls & 1);
      const long N = (long)s.N * c.Hc * c.Wc;
      const Plan p = plan_px(s.Cin, N, c.ntaps * s.Cout);
      if (p.splits > 1) b = std::max(b, (size_t)p.splits * s.Cin * N * sizeof(float));
    }
    return b;
  }
  const long N = (long)s.N * s.H * s.W;
  const Plan p = plan_px(s.Cin, N, s.Cout * s.KH * s.KW);
  const HaloPlan h = plan_halo(s, 1);
  const int splits = std::max(p.splits, h.ok ? h.splits : 1);
  return std::max(splits > 1 ? (size_t)splits * s.Cin * N * sizeof(float) : (size_t)0, reflect_dgrad_ws(s));
}

static size_t wgrad_ws_bytes(const ConvShape& s, int c0) {
  const long K = (long)s.N * s.Ho * s.Wo;
  const long Nc = (long)s.Cin * s.KH * s.KW;
  const WPlan p = plan_wgrad(s, c0);
  const WHaloPlan h = plan_whalo(s, c0);
  const int splits = std::max({p.splits, h.ok ? h.splits : 1, p.tile == WSTEM ? stem_wgrad_blocks(s) : 1});
  return (size_t)splits * s.Cout * Nc * sizeof(float) +
         (size_t)s.Cout * bias_parts(s.Cout, K) * sizeof(float) + 256;
}

// the split count depends on the concat split only through CW: size for every possible CW
size_t conv_wgrad_workspace(const ConvShape& s) {
  if (head_path(s)) return head_wgrad_workspace(s);
  size_t b = wgrad_ws_bytes(s, s.Cin);
  for (int c0 = 16; c0 <= 128; c0 *= 2) b = std::max(b, wgrad_ws_bytes(s, c0));
  return b;
}

#endif  // MD2_CONV_PART == 0

#if MD2_CONV_PART == 1
int conv_fwd(const ConvShape& s, const TensorIn& x, const float* wpacked, const TensorOut& y,
             ConvWorkspace ws, hipStream_t st, SplitKDefer* defer) {
  if (defer) {
    const SplitKDefer req = *defer;   // kept: launch_px reads the request
    *defer = SplitKDefer{};
    defer->stats = req.stats;
    defer->keep_reduce = req.keep_reduce;
  }
  MD2_TRY(check_shape(s));
  MD2_CHECK_ARG(x.p0 && wpacked && y.p0, "conv_fwd pointers");
  MD2_CHECK_ARG(x.c0 == s.Cin || x.p1 != nullptr, "conv_fwd: second input tensor missing");
  MD2_CHECK_ARG(x.c0 >= s.Cin || !conv_tap_major(s, 0) || x.c0 % 16 == 0,
                "conv_fwd: concat split must be a multiple of 16 channels");
  if (head_path(s) && x.c0 >= s.Cin && y.c0 >= 1) {
    MD2_CHECK_ARG(!conv_px2_used(s, 0), "head: packed layout");
    conv_arith_ref() = 0;
    return head_fwd(s, head_in(x), head_w(s, 0, wpacked), y.bias, y.act, y.p0, y.bs0,
                    y.accumulate, st);
  }
  ConvArgs a{};
  fill_common(a, s);
  a.g.M = s.Cout;
  a.g.N = (long)s.N * s.Ho * s.Wo;
  a.g.K = s.Cin * s.KH * s.KW;
  a.g.Mpad = (int)round_up(s.Cout, MPAD);
  a.fd_pix = make_fastdiv((uint32_t)(s.Ho * s.Wo));
  a.fd_row = make_fastdiv((uint32_t)s.Wo);
  a.fd_bdiv = make_fastdiv((uint32_t)std::min(x.bdiv, 1 << 30));
  a.in = x;
  a.A = wpacked;
  a.out = y;
  a.A_bytes = (uint32_t)(conv_fwd_packed_elems(s) * sizeof(float));
  {
    long ext0 = 0;
    for (int b = 0; b < s.N; ++b)
      ext0 = std::max(ext0, (long)(b % x.bdiv) * x.bs0 + (long)(b / x.bdiv) * x.bhi);
    ext0 += (long)x.c0 * s.H * s.W;
    const long ext1 = x.p1 ? (long)(s.N - 1) * x.bs1 + (long)(s.Cin - x.c0) * s.H * s.W : 0;
    MD2_CHECK_ARG(ext0 * 4 < (long)OOB && ext1 * 4 < (long)OOB, "conv_fwd: tensor exceeds 2 GB");
    a.b0_bytes = (uint32_t)(ext0 * 4);
    a.b1_bytes = (uint32_t)(ext1 * 4);
  }
  if (stem_s2d_applies(s, x, y)) {   // (statistics: the separate pass)
    conv_arith_ref() = 6;
    return stem_s2d_launch(s, a, st);
  }
  const bool bk32 = conv_tap_major(s, 0) && s.Cin % 32 == 0 && (x.c0 >= s.Cin || x.c0 % 32 == 0);
  const Plan p = plan_px(a.g.M, a.g.N, a.g.K, bk32);
  return launch_px<0>(s, a, p, ws, st, defer);
}

#endif  // MD2_CONV_PART == 1

#if MD2_CONV_PART == 2
int conv_dgrad(const ConvShape& s, const float* dy, const float* wpacked_d, const TensorOut& dx,
               ConvWorkspace ws, hipStream_t st, SplitKDefer* defer) {
  if (defer) *defer = SplitKDefer{};
  MD2_TRY(check_shape(s));
  MD2_CHECK_ARG(dy && wpacked_d && dx.p0, "conv_dgrad pointers");
  MD2_CHECK_ARG(!dx.bias && dx.act == ACT_NONE, "conv_dgrad: no bias/activation on dX");
  if (head_path(s) && dx.c0 >= s.Cin) {
    MD2_CHECK_ARG(!conv_px2_used(s, 1) && !conv_tap_major(s, 1), "head: packed layout");
    conv_arith_ref() = 0;
    return head_dgrad(s, dy, head_w(s, 1, wpacked_d), dx.p0, dx.bs0, dx.accumulate, st);
  }
  ConvArgs a{};
  fill_common(a, s);
  a.g.M = s.Cin;
  a.g.N = (long)s.N * s.H * s.W;
  a.g.K = s.Cout * s.KH * s.KW;
  a.g.Mpad = (int)round_up(s.Cin, MPAD);
  a.fd_pix = make_fastdiv((uint32_t)(s.H * s.W));
  a.fd_row = make_fastdiv((uint32_t)s.W);
  a.fd_bdiv = make_fastdiv(1u << 30);
  a.dy = dy;
  a.A = wpacked_d;
  a.out = dx;
  a.A_bytes = (uint32_t)(conv_dgrad_packed_elems(s) * sizeof(float));
  MD2_CHECK_ARG((long)s.N * s.Cout * s.Ho * s.Wo * 4 < (long)OOB, "conv_dgrad: tensor exceeds 2 GB");
  a.b0_bytes = (uint32_t)((long)s.N * s.Cout * s.Ho * s.Wo * 4);
  a.b1_bytes = 0;
  if (reflect_dgrad_on_halo(s)) {
    // the full adjoint on the padded grid (split-K slabs first in the workspace, the padded
    // image after them), then pad_reflect's adjoint into dX
    const ConvShape e = reflect_ext_shape(s);
    HaloPlan h;
    reflect_dgrad_on_halo(s, &h);
    const long Ne = (long)s.N * e.H * e.W;
    const size_t slab_b = (size_t)(h.splits > 1 ? h.splits : 0) * s.Cin * Ne * sizeof(float);
    MD2_CHECK_ARG(ws.ptr && ws.bytes >= slab_b + (size_t)s.Cin * Ne * sizeof(float),
                  "conv_dgrad: reflect workspace too small");
    float* dxp = (float*)((char*)ws.ptr + slab_b);
    ConvArgs ae = a;
    fill_common(ae, e);
    ae.Ho = s.Ho;
    ae.Wo = s.Wo;
    ae.HoWo = (long)s.Ho * s.Wo;
    ae.HoWo4 = (uint32_t)(ae.HoWo * 4);
    ae.g.N = Ne;
    ae.fd_pix = make_fastdiv((uint32_t)(e.H * e.W));
    ae.fd_row = make_fastdiv((uint32_t)e.W);
    ae.hx_ext = 1;
    TensorOut po{};
    po.p0 = dxp;
    po.c0 = s.Cin;
    po.bs0 = (long)s.Cin * e.H * e.W;
    ae.out = po;
    MD2_CHECK_ARG((long)s.N * s.Cin * (s.H + 2) * (s.W + 2) < (1L << 31), "conv_dgrad: reflect fold index");
    const Plan p = plan_px(ae.g.M, ae.g.N, ae.g.K, s.Cout % 32 == 0);
    // split-K: the slabs [split][Cin][N][H+2][W+2] go straight to the fold (no reduce pass)
    SplitKDefer df;
    MD2_TRY(launch_px<1>(e, ae, p, ConvWorkspace{ws.ptr, slab_b}, st, &df));
    const long HWp = (long)e.H * e.W;
    const bool sl = df.slab != nullptr;
    const long total = (long)s.N * s.Cin * s.H * s.W;
    const bool small = s.H == 3 || s.W == 3;
    // (four pixels per thread: W % 4 == 0, 16-byte aligned destination planes)
    static const int f4on = tuning_knob("MD2_FOLD4", 1);
    const bool f4 = f4on && !small && s.W % 4 == 0 && s.H >= 4 && s.W >= 8 && ((long)s.H * s.W) % 4 == 0 &&
                    ((uintptr_t)dx.p0 % 16) == 0 && dx.bs0 % 4 == 0 &&
                    (!dx.p1 || (((uintptr_t)dx.p1 % 16) == 0 && dx.bs1 % 4 == 0));
    if (f4)
      hipLaunchKernelGGL(fold_reflect4_kernel<0>, dim3(cdiv(total / 4, 256)), dim3(256), 0, st,
                         sl ? df.slab : dxp, sl ? df.splits : 1, (long)s.Cin * Ne, sl ? HWp : s.Cin * HWp,
                         sl ? Ne : HWp, dx, make_fastdiv((uint32_t)(s.H * s.W)),
                         make_fastdiv((uint32_t)(s.W / 4)), make_fastdiv((uint32_t)s.Cin), s.H,
                         (uint32_t)(total / 4));
    else
      hipLaunchKernelGGL(small ? fold_reflect_kernel<true> : fold_reflect_kernel<false>, dim3(cdiv(total, 256)),
                         dim3(256), 0, st, sl ? df.slab : dxp, sl ? df.splits : 1, (long)s.Cin * Ne,
                         sl ? HWp : s.Cin * HWp, sl ? Ne : HWp, dx, make_fastdiv((uint32_t)(s.H * s.W)),
                         make_fastdiv((uint32_t)s.W), make_fastdiv((uint32_t)s.Cin), (uint32_t)total);
    MD2_LAUNCH_CHECK();
    return MD2_OK;
  }
  if (const HaloS2Plan h2 = plan_halo_s2(s); h2.ok) {
    // the four output-parity classes from one staged dY image (conv_halo3s2_kernel): the kernel
    // iterates the dY grid; its split-K slabs [split][Cin][N H W] reduce as any dgrad's
    ConvArgs ak = a;
    ak.g.N = (long)s.N * s.Ho * s.Wo;
    ak.fd_pix = make_fastdiv((uint32_t)(s.Ho * s.Wo));
    ak.fd_row = make_fastdiv((uint32_t)s.Wo);
    ak.hx_cper = h2.cper;
    ak.slab = nullptr;
    if (h2.splits > 1) {
      const size_t need = (size_t)h2.splits * a.g.M * a.g.N * sizeof(float);
      MD2_CHECK_ARG(ws.ptr && ws.bytes >= need, "conv_dgrad: stride-2 halo workspace too small");
      ak.slab = (float*)ws.ptr;
    }
    conv_arith_ref() = 6;
    MD2_TRY(halo_s2_launch(ak, h2.items, h2.splits, st));
    if (h2.splits > 1) {
      ConvArgs ar = a;
      ar.slab = ak.slab;
      const TensorOut& o = a.out;
      const bool aligned4 = a.fd_pix.d % 4 == 0 && o.bs0 % 4 == 0 && (!o.p1 || o.bs1 % 4 == 0) &&
                            ((uintptr_t)o.p0 % 16) == 0 && (!o.p1 || ((uintptr_t)o.p1 % 16) == 0);
      const long total = (long)a.g.M * a.g.N;
      MD2_CHECK_ARG(total < (1L << 31), "conv_dgrad: split-K reduction index exceeds 2^31");
      if (aligned4)
        hipLaunchKernelGGL(splitk_reduce_px4_kernel<0>, dim3(cdiv(total / 4, 256)), dim3(256), 0, st, ar,
                           h2.splits);
      else
        hipLaunchKernelGGL(splitk_reduce_px_kernel<0>, dim3(cdiv(total, 256)), dim3(256), 0, st, ar,
                           h2.splits, 0, make_fastdiv((uint32_t)a.g.N), make_fastdiv((uint32_t)total));
      MD2_LAUNCH_CHECK();
    }
    return MD2_OK;
  }
  if (s.stride == 2 && conv_tap_major(s, 1) && conv_px2_used(s, 1) && s.KH <= 3 && s.H % 2 == 0 &&
      s.W % 2 == 0) {
    // the four output-parity classes (each a dense GEMM over only its own taps) in ONE launch:
    // equal extents, K of the largest class; smaller classes' surplus splits write zero slabs
    ConvArgs ac = a;
    int kmax = 0;
    for (int cls = 0; cls < 4; ++cls) {
      const PhaseClass c = phase_class(s, cls >> 1, cls & 1);
      ac.ph_y0c[cls] = c.y0;
      ac.ph_x0c[cls] = c.x0;
      ac.ph_ntc[cls] = c.ntaps;
      for (int t = 0; t < 4; ++t) ac.ph_taps[4 * cls + t] = t < c.ntaps ? c.taps[t] : 0;
      kmax = std::max(kmax, c.ntaps);
      if (cls == 0) {
        ac.g.N = (long)s.N * c.Hc * c.Wc;
        ac.fd_pix = make_fastdiv((uint32_t)(c.Hc * c.Wc));
        ac.fd_row = make_fastdiv((uint32_t)c.Wc);
      }
    }
    ac.g.K = kmax * s.Cout;
    ac.ph_S = 1;
    const Plan p = plan_px(ac.g.M, 4 * ac.g.N, ac.g.K, s.Cout % 32 == 0, true);
    return launch_px<1>(s, ac, p, ws, st);
  }
  if (s.stride == 2 && conv_tap_major(s, 1)) {
    // four dense GEMMs over the output-parity classes, each with only its own taps
    for (int cls = 0; cls < 4; ++cls) {
      const PhaseClass c = phase_class(s, cls >> 1, cls & 1);
      if (c.Hc <= 0 || c.Wc <= 0 || (c.ntaps == 0 && dx.accumulate)) continue;
      ConvArgs ac = a;
      ac.ph_y0 = c.y0;
      ac.ph_x0 = c.x0;
      for (int t = 0; t < 16; ++t) ac.ph_taps[t] = t < c.ntaps ? c.taps[t] : 0;
      ac.g.N = (long)s.N * c.Hc * c.Wc;
      ac.g.K = c.ntaps * s.Cout;
      ac.fd_pix = make_fastdiv((uint32_t)(c.Hc * c.Wc));
      ac.fd_row = make_fastdiv((uint32_t)c.Wc);
      const Plan p = plan_px(ac.g.M, ac.g.N, ac.g.K, s.Cout % 32 == 0);
      MD2_TRY(launch_px<1>(s, ac, p, ws, st));
    }
    return MD2_OK;
  }
  const Plan p = plan_px(a.g.M, a.g.N, a.g.K, conv_tap_major(s, 1) && s.Cout % 32 == 0);
  return launch_px<1>(s, a, p, ws, st, defer);
}

#endif  // MD2_CONV_PART == 2

#if MD2_CONV_PART == 3
int conv_wgrad(const ConvShape& s, const TensorIn& x, const float* dy, float* dw, float* db,
               int accumulate, ConvWorkspace ws, hipStream_t st, const float* db_part,
               int db_parts) {
  MD2_TRY(check_shape(s));
  MD2_CHECK_ARG(x.p0 && dy && dw, "conv_wgrad pointers");
  MD2_CHECK_ARG(x.c0 >= s.Cin || x.p1 != nullptr, "conv_wgrad: second input tensor missing");
  if (head_path(s) && x.c0 >= s.Cin) {
    conv_arith_ref() = 0;
    return head_wgrad(s, head_in(x), dy, dw, db, accumulate, ws.ptr, ws.bytes, st);
  }
  const WPlan p = plan_wgrad(s, x.c0);
  const bool tap = p.cw > 0;
  ConvArgs a{};
  fill_common(a, s);
  const long Kpix = (long)s.N * s.Ho * s.Wo;
  a.g.M = s.Cout;
  a.g.N = (long)s.Cin * s.KH * s.KW;
  a.g.K = (int)Kpix;
  a.fd_pix = make_fastdiv((uint32_t)(s.Ho * s.Wo));
  a.fd_row = make_fastdiv((uint32_t)s.Wo);
  a.fd_bdiv = make_fastdiv((uint32_t)std::min(x.bdiv, 1 << 30));
  a.in = x;
  a.dy = dy;
  {
    long ext0 = 0;
    for (int b = 0; b < s.N; ++b)
      ext0 = std::max(ext0, (long)(b % x.bdiv) * x.bs0 + (long)(b / x.bdiv) * x.bhi);
    ext0 += (long)std::min(x.c0, s.Cin) * s.H * s.W;
    const long ext1 = x.p1 ? (long)(s.N - 1) * x.bs1 + (long)(s.Cin - x.c0) * s.H * s.W : 0;
    const long extd = (long)s.N * s.Cout * s.Ho * s.Wo;
    MD2_CHECK_ARG(ext0 * 4 < (long)OOB && ext1 * 4 < (long)OOB && extd * 4 < (long)OOB,
                  "conv_wgrad: tensor exceeds 2 GB");
    a.b0_bytes = (uint32_t)(ext0 * 4);
    a.b1_bytes = (uint32_t)(ext1 * 4);
    a.A_bytes = (uint32_t)(extd * 4);
  }
  a.g.kper = p.kper;
  const size_t need = conv_wgrad_workspace(s);
  MD2_CHECK_ARG(ws.ptr && ws.bytes >= need, "conv_wgrad workspace too small");
  a.slab = (float*)ws.ptr;
  const long total = (long)a.g.M * a.g.N;
  const WHaloPlan hx = x.bdiv >= s.N ? plan_whalo(s, x.c0) : WHaloPlan{};
  // the stem on the space-to-depth kernel (conv_stem.inc): one slab per block
  const bool stem2 = !hx.ok && p.tile == WSTEM && stem_wgrad_s2d_applies(s, x);
  const int nsplit = hx.ok ? hx.splits : stem2 ? stem_wgrad_blocks(s) : p.splits;
  float* bpart = a.slab + (long)nsplit * total;
  dim3 grid((unsigned)p.ntiles_n, cdiv(a.g.M, p.BM), p.splits);
  int rc = MD2_ENOTSUP;
  if (hx.ok) {
    a.hx_r = hx.r;
    a.hx_nchunk = hx.nchunk;
    a.hx_cper = hx.cper;
    conv_arith_ref() = 6;
    rc = whalo_launch(a, hx.items, cdiv(hx.r * s.W, 16), hx.splits, st);
    if (rc) return rc;
  }
  if (stem2) {
    conv_arith_ref() = 6;
    rc = stem_wgrad_s2d_launch(s, a, st);
  }
  if (rc == MD2_ENOTSUP && p.tile == WSTEM) {
    conv_arith_ref() = 1;
    const dim3 gs((unsigned)p.splits);
    switch (s.Cin) {
      case 1: hipLaunchKernelGGL(conv_wgrad_stem_kernel<1>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
      case 2: hipLaunchKernelGGL(conv_wgrad_stem_kernel<2>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
      case 3: hipLaunchKernelGGL(conv_wgrad_stem_kernel<3>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
      case 4: hipLaunchKernelGGL(conv_wgrad_stem_kernel<4>, gs, dim3(256), 0, st, a); rc = MD2_OK; break;
      default: break;
    }
  }
  if (rc == MD2_ENOTSUP && p.tile == W16x144) {
    conv_arith_ref() = 1;
    grid.y = 1;
    if (p.BM == 64) {
      if (s.reflect)
        hipLaunchKernelGGL((conv_wgrad16_kernel<4, 3, 3, 1>), grid, dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((conv_wgrad16_kernel<4, 3, 3, 0>), grid, dim3(256), 0, st, a);
    } else if (p.BM == 32) {
      if (s.reflect)
        hipLaunchKernelGGL((conv_wgrad16_kernel<2, 3, 3, 1>), grid, dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((conv_wgrad16_kernel<2, 3, 3, 0>), grid, dim3(256), 0, st, a);
    } else {
      if (s.reflect)
        hipLaunchKernelGGL((conv_wgrad16_kernel<1, 3, 3, 1>), grid, dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((conv_wgrad16_kernel<1, 3, 3, 0>), grid, dim3(256), 0, st, a);
    }
    rc = MD2_OK;
  }
#define MD2_W_CASE(KS, SS, RR)                                                                     \
  if (rc == MD2_ENOTSUP && s.KH == KS && s.stride == SS && s.reflect == RR) {                      \
    switch (p.tile) {                                                                              \
      case W32x256: rc = launch_w<32, 256, 1, 4, KS, SS, RR>(p.cw, a, grid, st); break;            \
      case W64x64: rc = launch_w<64, 64, 2, 2, KS, SS, RR>(p.cw, a, grid, st); break;              \
      case W32x128: rc = launch_w<32, 128, 1, 4, KS, SS, RR>(p.cw, a, grid, st); break;            \
      case W64x192:                                                                                \
        if constexpr (KS == 3) {                                                                   \
          if (p.cw == 64) {                                                                        \
            launch_w_cw<64, 192, 2, 2, KS, SS, RR, 64>(a, grid, st);                               \
            rc = MD2_OK;                                                                           \
          }                                                                                        \
        }                                                                                          \
        break;                                                                                     \
      default: rc = launch_w<64, 128, 2, 2, KS, SS, RR>(p.cw, a, grid, st); break;                 \
    }                                                                                              \
  }
  MD2_CONV_COMBOS(MD2_W_CASE)
#undef MD2_W_CASE
  if (rc) {
    set_error("conv_wgrad: unsupported (kernel, stride, padding) combination");
    return rc;
  }
  MD2_LAUNCH_CHECK();
  WRed r{};
  r.slab = a.slab;
  r.splits = nsplit;
  r.total = total;
  r.dw = dw;
  r.acc = accumulate;
  r.ncols = (int)a.g.N;
  r.tapc = (tap || hx.ok) ? s.Cin : 0;
  r.KK = s.KH * s.KW;
  r.cinw = weight_cin(s);
  r.out_total = (long)s.Cout * r.cinw * r.KK;
  MD2_CHECK_ARG(r.cinw == s.Cin || tap, "conv_wgrad: padded input channels need the tap-major kernels");
  int nbias = 0;
  if (db) {
    int parts = db_parts;
    if (db_part) {
      r.bpart = db_part;
    } else {
      parts = bias_parts(s.Cout, Kpix);
      hipLaunchKernelGGL(bias_grad_partial_kernel, dim3(s.Cout, parts), dim3(256), 0, st, dy, s.Cout,
                         (long)s.Ho * s.Wo, Kpix, parts, bpart);
      MD2_LAUNCH_CHECK();
      r.bpart = bpart;
    }
    r.bparts = parts;
    r.Cout = s.Cout;
    r.db = db;
    nbias = cdiv(s.Cout, 256);
  }
  // 4 lanes per output once there are enough splits to share (more loads in flight per output)
  if (nsplit >= 8) {
    r.nmain = (int)cdiv(total, 64);
    hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3(r.nmain + nbias), dim3(256), 0, st, r);
  } else {
    r.nmain = (int)cdiv(r.out_total, 256);
    hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3(r.nmain + nbias), dim3(256), 0, st, r);
  }
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

#endif  // MD2_CONV_PART == 3

#if MD2_CONV_PART == 0
// block (c, p): the float4 units [U*p/parts, U*(p+1)/parts) of channel c's N planes
__device__ __forceinline__ float act_grad(float o, float g, int act) {
  switch (act) {
    case ACT_RELU: return o > 0.f ? g : 0.f;
    case ACT_ELU: return o > 0.f ? g : g * (o + 1.f);
    case ACT_SIGMOID: return g * o * (1.f - o);
    default: return g;
  }
}

__global__ __launch_bounds__(256) void act_bias_kernel(const float* __restrict__ out,
                                                       const float* __restrict__ dout,
                                                       float* __restrict__ dpre, int C, int parts,
                                                       uint32_t U, FastDiv fdq, int act,
                                                       float* __restrict__ part) {
  __shared__ float red[4];
  const int c = blockIdx.x, p = blockIdx.y;
  const uint32_t beg = (uint32_t)((unsigned long long)U * p / parts);
  const uint32_t end = (uint32_t)((unsigned long long)U * (p + 1) / parts);
  const uint32_t Q = fdq.d;   // float4 units per plane
  // four float4 units per thread in flight (the one-unit loop was latency-bound); the partial
  // sum keeps the unit order of the plain loop (u, u + 256, ...), so the result is unchanged
  float s = 0.f;
  constexpr int UN = 4;
  for (uint32_t u0 = beg + threadIdx.x; u0 < end; u0 += 256 * UN) {
    float4 o[UN], g[UN];
    long idx[UN];
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      const uint32_t u = u0 + 256 * q;
      const uint32_t uu = u < end ? u : u0;
      const uint32_t img = fdiv(uu, fdq), k = uu - img * Q;
      idx[q] = ((long)(img * (uint32_t)C + (uint32_t)c) * Q + k) * 4;
      o[q] = *reinterpret_cast<const float4*>(out + idx[q]);
      g[q] = *reinterpret_cast<const float4*>(dout + idx[q]);
    }
#pragma unroll
    for (int q = 0; q < UN; ++q) {
      if (u0 + 256 * q >= end) break;
      float4 d;
      d.x = act_grad(o[q].x, g[q].x, act);
      d.y = act_grad(o[q].y, g[q].y, act);
      d.z = act_grad(o[q].z, g[q].z, act);
      d.w = act_grad(o[q].w, g[q].w, act);
      *reinterpret_cast<float4*>(dpre + idx[q]) = d;
      s += (d.x + d.y) + (d.z + d.w);
    }
  }
  float v[1] = {s};
  block_sum256<1>(v, red);
  if (threadIdx.x == 0) part[(long)c * parts + p] = v[0];
}

int act_bias_parts(int C, int N, long HW) {
  const long U = (long)N * HW / 4;
  return (int)std::max(1L, std::min((long)std::max(1, 2048 / C), U / 1024 + 1));
}

int act_backward_bias(const float* out, const float* dout, float* dpre, int N, int C, long HW,
                      int act, float* part, hipStream_t st) {
  MD2_CHECK_ARG(HW % 4 == 0 && (long)N * C * HW < (1L << 31), "act_backward_bias: HW % 4, size");
  const int parts = act_bias_parts(C, N, HW);
  hipLaunchKernelGGL(act_bias_kernel, dim3(C, parts), dim3(256), 0, st, out, dout, dpre, C, parts,
                     (uint32_t)((long)N * HW / 4), make_fastdiv((uint32_t)(HW / 4)), act, part);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

int act_backward(const float* out, const float* dout, float* dpre, long n, int act,
                 hipStream_t st) {
  hipLaunchKernelGGL(act_backward_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, out, dout, dpre, n,
                     act);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

#endif  // MD2_CONV_PART == 0

}  // namespace md2

#if MD2_CONV_PART == 4
namespace md2 {
#include "conv_halo.inc"
}  // namespace md2
#endif

#if MD2_CONV_PART == 5
namespace md2 {
#include "conv_stem.inc"
}  // namespace md2
#endif
