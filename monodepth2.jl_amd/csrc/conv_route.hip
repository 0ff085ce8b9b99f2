// Implicit-GEMM conv: which kernel runs a pass.  The planners, the selection predicates, the route
// of a pass (conv_route / conv_wgrad_route: one decision that packing, workspace sizing and the
// launchers read), its narrowing by the operands of one call, and the sizing entry points.  Host
// code only: no kernels (the map of the conv files: conv_kernel.h).
#include "conv_plan.h"
#include "conv_lds.h"

namespace md2 {

// ---------------------------------------------------------------------------------------------
// tile selection, split-K planning (conv_plan.h)
// ---------------------------------------------------------------------------------------------
// debugging / tuning overrides of the planner (read once; honoured only under MD2_TUNING=1,
// common.h tuning_knob): MD2_PX_TARGET=<target blocks for split-K>, MD2_PX_BK=<16 | 32>, ...
static Plan plan_px(int M, long N, int K, bool bk32_ok = false, bool prefer32 = false) {
  // Small tiles, many blocks: at B=12 the GEMMs are ~0.5 chip of 128x128 tiles; 64x64 tiles
  // (30 VGPR + 16 AGPR, 8 waves/SIMD) with ~1536 blocks keep 4-6 waves per SIMD in flight and
  // ran 10-50% faster than 128x128 / 64x256 on every encoder shape (r01); 64x128 / 64x256 /
  // 128x64 under the bf16 split-product kernel 5-17% slower again (profiles/r04_sweep_px3.txt).
  // The two tiles below are the ones built (conv_plan.h, MD2_PX_TILES).
  static const int target = tuning_knob("MD2_PX_TARGET", TARGET_BLOCKS);
  Plan p{};
  p.tile = M > 32 ? T64x64 : T32x128;
  p.BM = TILE_BM(p.tile);
  p.BN = TILE_BN(p.tile);
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

// the bf16x9 kernel runs 16-deep chunks even where the planner asks for 32 (the stride-2 dgrad):
// its BK=32 form was measured 98 vs 69 us per layer-2..4 stride-2 dgrad and 3-8% slower elsewhere
int px3_terms() {
  static const int t = tuning_knob("MD2_PX3_TERMS", 6) == 9 ? 9 : 6;
  return t;
}

// GEMM reduction order.  Tap-major (k = tap*C + c, tap = kh*KW + kw) keeps the filter tap
// constant over a K chunk, so the spatial gather address is computed once per chunk and every
// channel step is a scalar offset; it needs the channel count (and a concat split) to be a
// multiple of the chunk.  Otherwise (the 3-channel stem, 1-channel disparity heads) the order is
// channel-major k = c*KK + tap.  mode: 0 forward (C = Cin), 1 dgrad (C = Cout), 2 wgrad columns.
static bool conv_tap_major(const ConvShape& s, int mode) {
  // MD2_CONV_CHANNEL_MAJOR=<bitmask of modes> forces the channel-major order (debugging)
  static const int forced = tuning_knob("MD2_CONV_CHANNEL_MAJOR", 0);
  if (forced & (1 << mode)) return false;
  switch (mode) {
    case 0: return s.Cin % 16 == 0;                                   // px chunk BK = 16
    case 1: return s.Cout % 16 == 0 && (!s.reflect || (s.H != 3 && s.W != 3));
    default: return s.Cin % 16 == 0;                                  // wgrad CW >= 16
  }
}

// the k-contiguous kernel (conv_px2.inc) runs every tap-major fwd / dgrad with M > 32 (tiles with
// BM >= 64); MD2_PX_V2=0 selects the previous kernel (A/B)
static bool conv_px2_used(const ConvShape& s, int mode) {
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
static bool conv_px3_used(const ConvShape& s, int mode) {
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

// Cout = 1 3x3 convs (disparity heads) run the VALU kernels of head.hip; MD2_HEAD=0 disables
static bool head_path(const ConvShape& s) {
  static const int on = tuning_knob("MD2_HEAD", 1);
  return on && head_conv_ok(s);
}

// the 16-row kernel (conv_px16.inc) runs tap-major 3x3 / stride-1 fwd (Cout <= 16, not a Cout = 1
// head) and dgrad (Cin <= 16); MD2_PX16=0 falls back to the 32-row tiles
static bool conv_px16_used(const ConvShape& s, int mode) {
  // bit 0: forward, bit 1: dgrad (off: the 32-row tile's dgrad measured as fast, 99 vs 103 us)
  static const int on = tuning_knob("MD2_PX16", 1);
  if (mode > 1 || !(on & (1 << mode)) || !conv_tap_major(s, mode) || s.KH != 3 || s.stride != 1) return false;
  const int M = mode == 0 ? s.Cout : s.Cin;
  if (M > 16) return false;
  return !(mode == 0 && head_path(s));
}

// conv_halo3 (conv_halo.inc): stride-1 3x3 zero-padded fwd / dgrad on the bf16x6 products with
// the LDS halo -- 64 x 256 tiles, split over 16-channel chunks until ~2 blocks per CU
// (MD2_HALO=0 with MD2_TUNING=1: conv_px3 instead; MD2_HX_TARGET: target blocks).  px3_tap: the
// shape's tile kernel is conv_px3 on the tap-major order (the packed operand the halo kernels read)
static HaloPlan plan_halo(const ConvShape& s, int mode, bool px3_tap) {
  HaloPlan h;
  static const int on = tuning_knob("MD2_HALO", 1);
  static const int target = tuning_knob("MD2_HX_TARGET", 256);   // blocks: one round of 512-thread blocks (one per CU); 512: 2 rounds, 2-10% slower on layers 3-4
  // reflect padding (the decoder blocks): forward only -- the dgrad's reflect adjoint folds the
  // border rows and columns back (conv_px3's border gathers)
  if (!on || mode > 1 || s.KH != 3 || s.KW != 3 || s.stride != 1 || s.pad != 1 || (s.reflect && mode == 1)) return h;
  if (!px3_tap) return h;
  const int M = mode == 0 ? s.Cout : s.Cin, C = mode == 0 ? s.Cin : s.Cout;
  if (C % 16 || s.cin_w) return h;
  const int hrmax = Halo3Lds::rows(s.W);                 // halo rows of 256 consecutive pixels
  const bool flat = M % 64 == 0 && Halo3Lds::fits(s.W) && cdiv((long)hrmax * s.W, 512) <= 2;
  // otherwise the 2D-tile kernel (maps too wide for the flattened image, 32-row M tiles;
  // bf16x6 only).  MD2_HALO2D (MD2_TUNING=1): bit 0 forward (default), bit 1 data gradient --
  // the reflect dgrad on it (the padded 66 x 210 grid in 8 x 32 tiles + the fold) measured
  // 6.532 vs 6.488 ms per step against conv_px3's direct reflect gathers (3 interleaved triples)
  static const int d2on = tuning_knob("MD2_HALO2D", 1);
  const bool d2 = !flat && (d2on >> mode & 1) && M % 32 == 0 && px3_terms() != 9 &&
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
static HaloS2Plan plan_halo_s2(const ConvShape& s, bool px3_tap) {
  HaloS2Plan h;
  static const int on = tuning_knob("MD2_HALO_S2", 1);
  if (!on || s.KH != 3 || s.KW != 3 || s.stride != 2 || s.pad != 1 || s.reflect || s.cin_w) return h;
  if (s.H != 2 * s.Ho || s.W != 2 * s.Wo || s.Cin % 64 || s.Cout % 16) return h;
  if (!px3_tap || px3_terms() == 9) return h;
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
static WHaloPlan plan_whalo(const ConvShape& s, int c0) {
  WHaloPlan h;
  static const int on = tuning_knob("MD2_WHALO", 1);
  static const int target = tuning_knob("MD2_WHX_TARGET", 256);   // 128 / 192 / 384 / 512: 7.05 / 6.89 / 6.83 / 6.76 vs 6.69 ms per step (profiles/r05_whalo_ab.txt)
  if (!on || s.KH != 3 || s.KW != 3 || s.stride != 1 || s.pad != 1 || s.reflect) return h;
  if (s.Cin % 32 || s.Cout % 64 || c0 < s.Cin || (s.cin_w && s.cin_w != s.Cin) || s.W > 112) return h;
  if (px3_terms() == 9) return h;                         // the 9-product variant: conv_wgrad_px3
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

// channels per tap block of the tap-major wgrad: largest of 128/64/32/16 (<= BN) dividing Cin and
// the concat split
static int wgrad_cw(const ConvShape& s, int c0, int BN) {
  for (int cw = 128; cw >= 16; cw /= 2)
    if (cw <= BN && s.Cin % cw == 0 && (c0 >= s.Cin || c0 % cw == 0)) return cw;
  return 0;
}

// tap: the wgrad columns run tap-major (conv_tap_major, mode 2)
static WPlan plan_wgrad(const ConvShape& s, int c0, bool tap) {
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
  if (w16 && s.Cout <= 16 * w16 && s.KH == 3 && s.KW == 3 && s.stride == 1 && tap &&
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
    cw = tap ? wgrad_cw(s, c0, WT_BN(tile)) : 0;
    const long nt = cw ? (long)cdiv(KK, WT_BN(tile) / cw) * (s.Cin / cw) : cdiv((long)s.Cin * KK, WT_BN(tile));
    return (long)cdiv(M, WT_BM(tile)) * nt;
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
  if (w192 && p.tile == W64x128 && KK == 9 && tap && wgrad_cw(s, c0, 128) == 64 &&
      wgrad_cw(s, c0, 192) == 64)
    p.tile = W64x192;
  if (WT_BM(tile_override)) p.tile = tile_override;   // the number of a built tile (conv_plan.h); others: ignored
  if (target > 0) tgt = target;
  p.BM = WT_BM(p.tile);
  p.BN = WT_BN(p.tile);
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

// the ResNet stem on the space-to-depth kernels (conv_stem.inc): the shape's side of their
// admission (the operands' side: the narrowing below).  MD2_STEM_S2D=0 / MD2_WSTEM_S2D=0: off
static bool stem_s2d_applies(const ConvShape& s) {
  static const int on = tuning_knob("MD2_STEM_S2D", 1);
  if (!on || s.KH != 7 || s.KW != 7 || s.stride != 2 || s.pad != 3 || s.reflect || s.Cin != 3 || s.Cout != 64) return false;
  if (s.cin_w && s.cin_w != 3) return false;
  if (s.H % 2 || s.W % 2 || s.Wo % 16 || s.Ho != s.H / 2 || s.Wo != s.W / 2) return false;
  if (!StemLds::fits(s.Wo)) return false;                // the LDS ring (Wo <= 338: <= 21 subtiles per row)
  return (long)s.N * s.Ho * s.Wo < (1L << 31);
}
// the filter-gradient kernel: the forward's conditions and its own ring (StemWgradLds: the pitch
// P, the combine buffer over the ring)
static bool stem_wgrad_s2d_applies(const ConvShape& s) {
  static const int on = tuning_knob("MD2_WSTEM_S2D", 1);
  if (!on || !stem_s2d_applies(s)) return false;
  return StemWgradLds::fits(s.Wo) && (long)s.N * s.Cout * s.Ho * s.Wo * 4 < (long)OOB;
}

// reflect-padded 3x3 dgrad (the decoder blocks) on the halo kernel: the zero-padded same-size
// dgrad of the (H+2) x (W+2) grid (conv_halo3 EXT) into a workspace image, then the fold
static ConvShape reflect_ext_shape(const ConvShape& s) {
  ConvShape e = s;
  e.H = s.H + 2;
  e.W = s.W + 2;
  e.Ho = e.H;
  e.Wo = e.W;
  e.reflect = 0;
  return e;
}

// stride-2 dgrad output-parity class (cy, cx): input pixels iy = y0 + 2j with (iy + pad) % 2 ==
// cy receive exactly the taps kh % 2 == cy (same for columns)
static PhaseClass phase_class(const ConvShape& s, int cy, int cx) {
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

// ---------------------------------------------------------------------------------------------
// the route of a pass
// ---------------------------------------------------------------------------------------------
// `splits` split-K slabs of M x N floats (none for one split)
static size_t slab_bytes(int splits, long M, long N) {
  return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

PxRoute conv_route(const ConvShape& s, int mode) {
  PxRoute r{};
  const bool tap = conv_tap_major(s, mode), px2 = conv_px2_used(s, mode), px3 = conv_px3_used(s, mode);
  const bool px16 = conv_px16_used(s, mode);
  const int KK = s.KH * s.KW;
  const int M = mode == 0 ? s.Cout : s.Cin, C = mode == 0 ? s.Cin : s.Cout;
  const long N = mode == 0 ? (long)s.N * s.Ho * s.Wo : (long)s.N * s.H * s.W;
  // the packed operand: layout 0 [Kpad][Mpad] fp32, 1 [Kpad/16][Mpad][16] fp32 (conv_px2 /
  // conv_px16), 2 [Kpad/16][3][Mpad][16] bf16 split terms (conv_px3: 1.5x the fp32 bytes)
  r.arith = px3 ? ARITH_PX3 : px2 ? ARITH_PX2 : ARITH_PX;
  r.layout = px3 ? 2 : (px2 || px16) ? 1 : 0;
  r.tap = tap ? 1 : 0;
  r.Kpad = (int)round_up((long)C * KK, KPAD);
  r.Mpad = (int)round_up(M, MPAD);
  r.packed_elems = (size_t)r.Kpad * r.Mpad;
  if (r.layout == 2) r.packed_elems = r.packed_elems / 2 * 3;
  // the tile kernel: the route of everything below that has no kernel of its own, and where the
  // operands of a call veto the first choice (conv_fwd_narrow / conv_dgrad_narrow)
  r.tile = plan_px(M, N, C * KK, tap && C % 32 == 0);
  r.kind = PX_TILE;
  size_t tile_ws = slab_bytes(r.tile.splits, M, N);
  if (mode == 0 && r.tile.BK == 32)   // (a concat split can take the forward back to 16-deep chunks)
    tile_ws = std::max(tile_ws, slab_bytes(plan_px(M, N, C * KK).splits, M, N));
  r.ws_bytes = tile_ws;
  if (head_path(s)) {
    r.kind = PX_HEAD;
    return r;
  }
  if (mode == 0 && stem_s2d_applies(s)) {
    r.kind = PX_STEM_S2D;
    return r;
  }
  if (mode == 1 && s.reflect) {
    static const int on = tuning_knob("MD2_HALO_RFL_DGRAD", 1);
    if (on && s.KH == 3 && s.stride == 1 && s.pad == 1 && !s.cin_w && s.H >= 2 && s.W >= 2) {
      const ConvShape e = reflect_ext_shape(s);
      const HaloPlan h = plan_halo(e, 1, conv_px3_used(e, 1) && conv_tap_major(e, 1));
      if (h.ok) {
        // split-K slabs first in the workspace, the padded image after them
        r.kind = PX_REFLECT_HALO;
        r.ext = e;
        r.halo = h;
        const long Ne = (long)s.N * e.H * e.W;
        r.ws_bytes = slab_bytes(h.splits, M, Ne) + (size_t)M * Ne * sizeof(float);
        return r;
      }
    }
  }
  if (mode == 1 && s.stride == 2) {
    r.s2 = plan_halo_s2(s, px3 && tap);
    if (r.s2.ok) {
      r.kind = PX_HALO_S2;
      r.ws_bytes = slab_bytes(r.s2.splits, M, N);
      return r;
    }
    if (tap) {
      // the output-parity classes, each a dense GEMM over only its own taps
      int kmax = 0;
      for (int cls = 0; cls < 4; ++cls) {
        r.cls[cls] = phase_class(s, cls >> 1, cls & 1);
        kmax = std::max(kmax, r.cls[cls].ntaps);
      }
      if (px2 && s.KH <= 3 && s.H % 2 == 0 && s.W % 2 == 0) {
        // ONE launch: equal extents, K of the largest class
        r.kind = PX_CLASSES_MERGED;
        const long Nc = (long)s.N * r.cls[0].Hc * r.cls[0].Wc;
        r.cls_plan[0] = plan_px(M, 4 * Nc, kmax * s.Cout, s.Cout % 32 == 0, true);
        r.ws_bytes = 4 * slab_bytes(r.cls_plan[0].splits, M, Nc);
        return r;
      }
      r.kind = PX_CLASSES4;
      r.ws_bytes = 0;
      for (int cls = 0; cls < 4; ++cls) {
        const PhaseClass& c = r.cls[cls];
        const long Nc = (long)s.N * c.Hc * c.Wc;
        r.cls_plan[cls] = plan_px(M, Nc, c.ntaps * s.Cout, s.Cout % 32 == 0);
        r.ws_bytes = std::max(r.ws_bytes, slab_bytes(r.cls_plan[cls].splits, M, Nc));
      }
      return r;
    }
  }
  if (px16) {
    r.kind = PX_PX16;   // no split-K
    r.ws_bytes = 0;
    return r;
  }
  r.halo = plan_halo(s, mode, px3 && tap);
  if (r.halo.ok) {
    r.kind = r.halo.d2 ? PX_HALO2D : PX_HALO;
    // the forward can fall back to the tile at the call; the data gradient has no operand veto
    r.ws_bytes = std::max(slab_bytes(r.halo.splits, M, N), mode == 0 ? tile_ws : (size_t)0);
  }
  return r;
}

// what depends on the operands of one call: the kernels with a form of their own for the input
// or output give way to the tile kernel
PxRoute conv_fwd_narrow(PxRoute r, const ConvShape& s, const TensorIn& x, const TensorOut& y) {
  bool veto = false;
  switch (r.kind) {
    case PX_HEAD:      // one input tensor, one output row
      veto = x.c0 < s.Cin || y.c0 < 1;
      break;
    case PX_STEM_S2D:  // one input tensor and a plain output
      veto = x.p1 || x.c0 < s.Cin || y.bias || y.act != ACT_NONE || y.accumulate || y.c0 < s.Cout;
      break;
    case PX_HALO:      // no frame-strided images; a concat split on a 16-channel chunk boundary
    case PX_HALO2D:
      veto = x.bdiv < s.N || (x.p1 && x.c0 < s.Cin && x.c0 % 16);
      break;
    default: break;
  }
  if (veto) r.kind = PX_TILE;
  // 32-deep chunks must not straddle the concat split
  if (r.kind == PX_TILE && r.tile.BK == 32 && x.c0 < s.Cin && x.c0 % 32)
    r.tile = plan_px(s.Cout, (long)s.N * s.Ho * s.Wo, s.Cin * s.KH * s.KW);
  return r;
}
PxRoute conv_dgrad_narrow(PxRoute r, const ConvShape& s, const TensorOut& dx) {
  if (r.kind == PX_HEAD && dx.c0 < s.Cin) r.kind = PX_TILE;   // the head kernels write one tensor
  return r;
}

WRoute conv_wgrad_route(const ConvShape& s, int c0) {
  WRoute r{};
  const long K = (long)s.N * s.Ho * s.Wo;
  const long Nc = (long)s.Cin * s.KH * s.KW;
  if (head_path(s) && c0 >= s.Cin) {
    // batched or fallback is known only at the call (alignment, accumulate): the larger need
    r.kind = r.base = W_HEAD;
    float sized;        // a filter gradient is asked for; never written
    HeadJob j = conv_head_job(s);
    j.dw = &sized;
    const size_t batched = s.reflect && !heads_job_unfit(j) ? heads_bwd_workspace(&j, 1) : 0;
    r.ws_bytes = std::max(head_wgrad_workspace(j), batched);
    return r;
  }
  r.tile = plan_wgrad(s, c0, conv_tap_major(s, 2));
  r.base = r.tile.tile == WSTEM ? W_STEM : r.tile.tile == W16x144 ? W_WGRAD16 : W_TILE;
  r.kind = r.base;
  r.nsplit = r.tile.splits;
  r.halo = plan_whalo(s, c0);
  if (r.halo.ok) {
    r.kind = W_WHALO;
    r.nsplit = r.halo.splits;
  } else if (r.base == W_STEM && stem_wgrad_s2d_applies(s)) {
    r.kind = W_STEM_S2D;   // one slab per block
    r.nsplit = stem_wgrad_blocks(s);
  }
  // the slabs of the route or of the kernel it narrows to, the bias partials behind them
  r.ws_bytes = (size_t)std::max(r.nsplit, r.tile.splits) * s.Cout * Nc * sizeof(float) +
               (size_t)s.Cout * bias_parts(s.Cout, K) * sizeof(float);
  return r;
}

WRoute conv_wgrad_narrow(WRoute r, const ConvShape& s, const TensorIn& x) {
  const bool veto = (r.kind == W_WHALO && x.bdiv < s.N) ||      // no frame-strided images
                    (r.kind == W_STEM_S2D && x.p1 != nullptr);  // one input tensor
  if (veto) {
    r.kind = r.base;
    r.nsplit = r.tile.splits;
  }
  return r;
}

// ---------------------------------------------------------------------------------------------
// sizing (conv.h): the route's numbers
// ---------------------------------------------------------------------------------------------
size_t conv_fwd_packed_elems(const ConvShape& s) { return conv_route(s, 0).packed_elems; }
size_t conv_dgrad_packed_elems(const ConvShape& s) { return conv_route(s, 1).packed_elems; }
size_t conv_fwd_workspace(const ConvShape& s) { return conv_route(s, 0).ws_bytes; }
size_t conv_dgrad_workspace(const ConvShape& s) { return conv_route(s, 1).ws_bytes; }
// the route depends on the concat split only through its divisibility: size for every class (and
// 256 bytes to spare, as callers have always been given).  A head shape is sized for the head
// kernels, which take one tensor: with a concat input it runs the generic route, and conv_wgrad
// refuses the call unless its workspace holds that route's bytes
size_t conv_wgrad_workspace(const ConvShape& s) {
  const WRoute one = conv_wgrad_route(s, s.Cin);
  if (one.kind == W_HEAD) return one.ws_bytes;
  size_t b = one.ws_bytes;
  for (int c0 = 16; c0 <= 128; c0 *= 2) b = std::max(b, conv_wgrad_route(s, c0).ws_bytes);
  return b + 256;
}

// ---------------------------------------------------------------------------------------------
// glue shared by the launchers
// ---------------------------------------------------------------------------------------------
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

int bias_parts(int C, long total) {
  return (int)std::max(1L, std::min((long)std::max(1, 1024 / C), total / 4096 + 1));
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

}  // namespace md2
