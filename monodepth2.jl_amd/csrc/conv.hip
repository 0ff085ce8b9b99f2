// Implicit-GEMM conv: weight packing, the planners, selection predicates, workspace sizing,
// act_backward (the map of the conv files: conv_kernel.h).
#include <cstdio>
#include "conv_plan.h"
#include "conv_lds.h"

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

// ---------------------------------------------------------------------------------------------
// host side: tile selection, split-K planning (conv_plan.h)
// ---------------------------------------------------------------------------------------------
// debugging / tuning overrides of the planner (read once; honoured only under MD2_TUNING=1,
// common.h tuning_knob): MD2_PX_TILE=<TileCfg>, MD2_PX_TARGET=<target blocks for split-K>, ...
Plan plan_px(int M, long N, int K, bool bk32_ok, bool prefer32) {
  // Small tiles, many blocks: at B=12 the GEMMs are ~0.5 chip of 128x128 tiles; 64x64 tiles
  // (30 VGPR + 16 AGPR, 8 waves/SIMD) with ~1536 blocks keep 4-6 waves per SIMD in flight and
  // ran 10-50% faster than 128x128 / 64x256 on every encoder shape (tools/sweep_px.sh, r01).
  static const int tile_override = tuning_knob("MD2_PX_TILE", -1);
  static const int target = tuning_knob("MD2_PX_TARGET", TARGET_BLOCKS);
  Plan p{};
  p.tile = M > 32 ? T64x64 : T32x128;
  if (tile_override >= 0 && tile_override <= T128x64q &&
      ((M > 32 && TILE_BM[tile_override] >= 64) || (M <= 32 && TILE_BM[tile_override] == 32)))
    p.tile = tile_override;
  p.BM = TILE_BM[p.tile];
  p.BN = TILE_BN[p.tile];
  static const int bk_override = tuning_knob("MD2_PX_BK", 0);
  p.BK = ((bk_override == 32 || (prefer32 && bk_override != 16)) && bk32_ok) ? 32 : 16;
  if (K <= 0) {                // a parity class without taps: the kernel only writes zeros
    p.splits = 1;
    p.kper = p.BK;
    return p;
  }
  // a split keeps >= MD2_PX_MINCH (default 8) K chunks
  static const int minch = std::max(1, tuning_knob("MD2_PX_MINCH", 8));
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
HaloPlan plan_halo(const ConvShape& s, int mode) {
  HaloPlan h;
  static const int on = tuning_knob("MD2_HALO", 1);
  static const int target = tuning_knob("MD2_HX_TARGET", 256);   // blocks: one round of 512-thread blocks (one per CU); 512: 2 rounds, 2-10% slower on layers 3-4
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
  static const int d2on = tuning_knob("MD2_HALO2D", 1);
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
HaloS2Plan plan_halo_s2(const ConvShape& s) {
  HaloS2Plan h;
  static const int on = tuning_knob("MD2_HALO_S2", 1);
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
WHaloPlan plan_whalo(const ConvShape& s, int c0) {
  WHaloPlan h;
  static const int on = tuning_knob("MD2_WHALO", 1);
  static const int target = tuning_knob("MD2_WHX_TARGET", 256);   // 128 / 192 / 384 / 512: 7.05 / 6.89 / 6.83 / 6.76 vs 6.69 ms per step (profiles/r05_whalo_ab.txt)
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
  static const int maxit = tuning_knob("MD2_WHX_MAXITEMS", 4);
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
bool reflect_dgrad_on_halo(const ConvShape& s, HaloPlan* hp) {
  static const int on = tuning_knob("MD2_HALO_RFL_DGRAD", 1);
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

// channels per tap block of the tap-major wgrad: largest of 128/64/32/16 (<= BN) dividing Cin and
// the concat split
int wgrad_cw(const ConvShape& s, int c0, int BN) {
  for (int cw = 128; cw >= 16; cw /= 2)
    if (cw <= BN && s.Cin % cw == 0 && (c0 >= s.Cin || c0 % cw == 0)) return cw;
  return 0;
}

WPlan plan_wgrad(const ConvShape& s, int c0) {
  static const int tile_override = tuning_knob("MD2_W_TILE", -1);
  static const int target = tuning_knob("MD2_W_TARGET", 0);
  WPlan p{};
  // Cout <= 16 * MD2_W16 (1, 2 or 4; default 2), 3x3 stride 1, tap-major with 16-channel
  // groups: conv_wgrad16_kernel (MD2_W16=0 falls back to the 32x128 tiles; MD2_W16_TARGET =
  // blocks to split K towards)
  // the ResNet stem (7x7/2, <= 4 image channels, 64 filters): conv_wgrad_stem_kernel, split-K
  // over all output pixels to ~MD2_WSTEM_TARGET blocks (MD2_WSTEM=0: the generic tiles)
  static const int wstem = tuning_knob("MD2_WSTEM", 1);
  static const int tstem = tuning_knob("MD2_WSTEM_TARGET", 512);
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
  static const int w16 = tuning_knob("MD2_W16", 2);
  static const int t16 = tuning_knob("MD2_W16_TARGET", 512);
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
    static const int t64 = tuning_knob("MD2_W64_TARGET", 1728);
    if (p.tile == W64x64) tgt = t64;
    // channel-major (the 3-channel 7x7 stem, 147 columns): 64-wide column tiles pad 147 to 192
    // instead of 256 (MD2_W_CM64=1: on -- measured neutral-to-slower, off by default)
    static const int cm64 = tuning_knob("MD2_W_CM64", 0);
    static const int cmt = tuning_knob("MD2_W_CM_TARGET", 768);
    const long ncol = (long)s.Cin * KK;
    if (cm64 && cw == 0 && p.tile == W64x128 && round_up(ncol, 64) < round_up(ncol, 128)) {
      p.tile = W64x64;
      tgt = cmt;
    }
  }
  // 64-channel 3x3 tap-major convs: 64x128 tiles hold 2 taps, so the 9 taps take 5 column tiles
  // with one tap slot in ten idle; 64x192 tiles (3 taps x 64 channels, TN = 3) cover them in 3
  // with no idle column (MD2_W192=0: off)
  static const int w192 = tuning_knob("MD2_W192", 1);
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
  static const int minch = std::max(1, tuning_knob("MD2_W_MINCH", 4));   // K chunks per split, at least (8 -> 4: +0.6% step, tools/minch_sweep.sh)
  long splits = std::max(1L, (long)tgt / tiles);
  splits = std::min(splits, std::max(1L, K / (minch * BK)));
  p.kper = (int)round_up((K + splits - 1) / splits, BK);
  p.splits = (int)((K + p.kper - 1) / p.kper);
  return p;
}

void fill_common(ConvArgs& a, const ConvShape& s) {
  static const int xcd = tuning_knob("MD2_XCD", 0);
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

// the bf16x9 kernel runs 16-deep chunks even where the planner asks for 32 (the stride-2 dgrad):
// its BK=32 form was measured 98 vs 69 us per layer-2..4 stride-2 dgrad and 3-8% slower elsewhere
int px3_terms() {
  static const int t = tuning_knob("MD2_PX3_TERMS", 6) == 9 ? 9 : 6;
  return t;
}

// stride-2 dgrad output-parity class (cy, cx): input pixels iy = y0 + 2j with (iy + pad) % 2 ==
// cy receive exactly the taps kh % 2 == cy (same for columns)
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

int bias_parts(int C, long total) {
  return (int)std::max(1L, std::min((long)std::max(1, 1024 / C), total / 4096 + 1));
}

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

// Cout = 1 3x3 convs (disparity heads) run the VALU kernels of head.hip; MD2_HEAD=0 disables
bool head_path(const ConvShape& s) {
  static const int on = tuning_knob("MD2_HEAD", 1);
  return on && head_conv_ok(s);
}
// tap (c, t) of the packed operand: forward rows m = 0, k = t*Cin + c or c*9 + t; dgrad
// k = co*9 + t = t (Cout = 1, channel-major), row c
HeadW conv_head_w(const ConvShape& s, int mode, const float* packed) {
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
HeadIn conv_head_in(const TensorIn& x) { return HeadIn{x.p0, x.bs0, x.bdiv, x.bhi}; }
HeadJob conv_head_job(const ConvShape& s) {
  HeadJob j{};
  j.Cin = s.Cin;
  j.H = s.H;
  j.W = s.W;
  j.N = s.N;
  return j;
}

// the 16-row kernel (conv_px16.inc) runs tap-major 3x3 / stride-1 fwd (Cout <= 16, not a Cout = 1
// head) and dgrad (Cin <= 16); MD2_PX16=0 falls back to the 32-row tiles
bool conv_px16_used(const ConvShape& s, int mode) {
  // bit 0: forward, bit 1: dgrad (off: the 32-row tile's dgrad measured as fast, 99 vs 103 us)
  static const int on = tuning_knob("MD2_PX16", 1);
  if (mode > 1 || !(on & (1 << mode)) || !conv_tap_major(s, mode) || s.KH != 3 || s.stride != 1) return false;
  const int M = mode == 0 ? s.Cout : s.Cin;
  if (M > 16) return false;
  return !(mode == 0 && head_path(s));
}

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
  if (head_path(s)) {   // the route is known only at the call (alignment, accumulate): the larger need
    float sized;        // a filter gradient is asked for; never written
    HeadJob j = conv_head_job(s);
    j.dw = &sized;
    const size_t batched = s.reflect && !heads_job_unfit(j) ? heads_bwd_workspace(&j, 1) : 0;
    return std::max(head_wgrad_workspace(j), batched);
  }
  size_t b = wgrad_ws_bytes(s, s.Cin);
  for (int c0 = 16; c0 <= 128; c0 *= 2) b = std::max(b, wgrad_ws_bytes(s, c0));
  return b;
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
