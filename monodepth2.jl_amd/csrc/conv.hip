// Implicit-GEMM conv: weight packing, the kernel-note helpers, act_backward (the map of the conv
// files: conv_kernel.h).
#include <cstdio>
#include "conv_plan.h"

namespace md2 {

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
// forward:  Wt[k][m] = W[m][c][tap]   ([Kpad][Mpad]);   dgrad: Wd[k][ci] = W[co][ci][tap]
// ([Kdpad][Cinpad]); k = tap*C + c (tap-major) or c*KK + tap, C = Cin (forward) / Cout (dgrad)
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

// (layout, K order and padded sizes of each operand: the pass's route, conv_route.hip)
static int pack_single(const ConvShape& s, int mode, const float* w, float* packed, hipStream_t st) {
  const PxRoute r = conv_route(s, mode);
  PackOne j{};
  j.w = w;
  j.out = packed;
  j.mode = mode;
  j.tap = r.tap;
  j.layout = r.layout;
  j.Cout = s.Cout;
  j.Cin = s.Cin;
  j.Cinw = weight_cin(s);
  j.KK = s.KH * s.KW;
  j.Kpad = r.Kpad;
  j.Mpad = r.Mpad;
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
  const PxRoute f = conv_route(s, 0), d = conv_route(s, 1);
  j.f = PackDst{out_f, f.tap, f.layout, f.Mpad};
  j.d = PackDst{out_d, d.tap, d.layout, d.Mpad};
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

// a launch site stores four words; the string is put together when it is asked for
struct KernelNote {
  const char* family = "";
  int bm = 0, bn = 0, cw = 0;
  char text[48] = "";
};
static KernelNote& conv_kernel_note() {
  static thread_local KernelNote n;
  return n;
}
void conv_note_kernel(const char* family, int bm, int bn, int cw) {
  KernelNote& n = conv_kernel_note();
  n.family = family;
  n.bm = bm;
  n.bn = bn;
  n.cw = cw;
}
const char* conv_last_kernel() {
  KernelNote& n = conv_kernel_note();
  if (n.bm == 0) return n.family;
  snprintf(n.text, sizeof n.text, "%s:%dx%dc%d", n.family, n.bm, n.bn, n.cw);
  return n.text;
}

int conv_pack_batch(const PackJob* dev_jobs, int njobs, long total_blocks, hipStream_t st) {
  if (njobs == 0) return MD2_OK;
  hipLaunchKernelGGL(pack_batch_kernel, dim3(total_blocks), dim3(256), 0, st, dev_jobs, njobs);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

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

}  // namespace md2
