// Implicit-GEMM convolution kernels for gfx950 (see conv.h).  This header: what all seven conv units
// share (device helpers, kernel arguments, the dynamic-LDS launch).  conv_plan.h: host-only plan
// structs, the route of a pass (PxRoute / WRoute) and declarations.  conv_route.hip (no kernels):
// the planners, the selection predicates, conv_route / conv_wgrad_route and their narrowing by
// the operands of a call, workspace and packed sizes -- the one place a kernel is chosen.
// conv.hip: the pack kernels, the kernel-note helpers, act_backward.  conv_px_launch.h: the fwd /
// dgrad kernels (conv_px*.inc) and launchers of conv_fwd.hip and conv_dgrad.hip, which switch on
// the route's kind.  conv_wgrad.hip: conv_wgrad_kernels.inc, conv_wpx3.inc, launchers, conv_wgrad.
// conv_halo.hip / conv_stem.hip: conv_halo.inc / conv_stem.inc.
// conv_api.hip: the C entry points that carry the executor's operand forms (md2_conv2d_*_ex; no kernels).
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
#pragma once
#include "conv.h"

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

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// exact three-way split of two fp32 values into packed bf16 pairs (hi, mid, lo): each remainder
// of a round-to-nearest bf16 is exact in fp32, and the second remainder has <= 8 significant bits
__device__ __forceinline__ void split3_pk(float a, float b, uint32_t& h, uint32_t& m, uint32_t& l) {
  const f32x2_t x = {a, b};
  const bf16x2_t hb = __builtin_convertvector(x, bf16x2_t);
  const f32x2_t r1 = x - __builtin_convertvector(hb, f32x2_t);
  const bf16x2_t mb = __builtin_convertvector(r1, bf16x2_t);
  const f32x2_t r2 = r1 - __builtin_convertvector(mb, f32x2_t);
  h = __builtin_bit_cast(uint32_t, hb);
  m = __builtin_bit_cast(uint32_t, mb);
  l = __builtin_bit_cast(uint32_t, __builtin_convertvector(r2, bf16x2_t));
}

__device__ __forceinline__ u32x4_t bload16(__amdgpu_buffer_rsrc_t r, uint32_t off_bytes) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off_bytes, 0, 0);
  u32x4_t o;
  o[0] = v[0];
  o[1] = v[1];
  o[2] = v[2];
  o[3] = v[3];
  return o;
}

// two bf16 (high halves of a, b) -> one dword, a in the low half
__device__ __forceinline__ uint32_t pk_bf16(uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xffff0000u); }

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

// arithmetic of the last conv kernel this host thread launched (profiling labels, conv.h)
int& conv_arith_ref();

}  // namespace md2
