// Host side of the conv passes: tile tables, plan structs, the route of a pass (defined once, in
// conv_route.hip: packing, sizing and launching read the same decision) and the cross-unit launchers.
#pragma once
#include "conv_kernel.h"
#include "head.h"

namespace md2 {

constexpr int TARGET_BLOCKS = 1536;  // ~6 blocks (waves per SIMD) per CU on 256 CUs

// The tiles the tile kernels are built for, each stated once.  The enum, the BM / BN lookups and
// the launchers' dispatch (launch_px, launch_w_tile) are generated from these lists: a tile the
// planner can name has a launcher case, and no kernel is built for a tile it cannot name.
// fwd / dgrad: X(name, BM, BN, WM, WN), BM x BN outputs on 4 waves as WM x WN.  64x64 where M > 32,
// 32x128 below (plan_px, with the measurements against larger tiles).
#define MD2_PX_TILES(X) X(T64x64, 64, 64, 2, 2) X(T32x128, 32, 128, 1, 4)
// wgrad: X(name, BM, BN, WM, WN, id); columns are tap-major (tap groups x CW channels).  id is the
// number MD2_W_TILE takes (1 was a 32x256 tile; 4 and 5 are the two routes below)
#define MD2_W_TILES(X) \
  X(W64x128, 64, 128, 2, 2, 0) X(W64x64, 64, 64, 2, 2, 2) X(W32x128, 32, 128, 1, 4, 3) X(W64x192, 64, 192, 2, 2, 6)

#define MD2_TILE_ENUM(name, ...) name,
#define MD2_W_TILE_ENUM(name, BM, BN, WM, WN, id) name = id,
enum TileCfg { MD2_PX_TILES(MD2_TILE_ENUM) };
// W16x144 and WSTEM: routes with kernels of their own (conv_wgrad16_kernel, conv_wgrad_stem_kernel)
enum WTileCfg { MD2_W_TILES(MD2_W_TILE_ENUM) W16x144 = 4, WSTEM = 5 };
#undef MD2_TILE_ENUM
#undef MD2_W_TILE_ENUM

// BM / BN of a tile of the lists; 0: not a built tile
#define MD2_TILE_BM(name, BM, ...) case name: return BM;
#define MD2_TILE_BN(name, BM, BN, ...) case name: return BN;
constexpr int TILE_BM(int tile) { switch (tile) { MD2_PX_TILES(MD2_TILE_BM) default: return 0; } }
constexpr int TILE_BN(int tile) { switch (tile) { MD2_PX_TILES(MD2_TILE_BN) default: return 0; } }
constexpr int WT_BM(int tile) { switch (tile) { MD2_W_TILES(MD2_TILE_BM) default: return 0; } }
constexpr int WT_BN(int tile) { switch (tile) { MD2_W_TILES(MD2_TILE_BN) default: return 0; } }
#undef MD2_TILE_BM
#undef MD2_TILE_BN

// (KH, S, RFL) combos instantiated
#define MD2_CONV_COMBOS(X) X(1, 1, 0) X(1, 2, 0) X(3, 1, 0) X(3, 1, 1) X(3, 2, 0) X(7, 2, 0)

struct Plan {
  int tile;
  int BM, BN, BK;
  int splits;
  int kper;
};
struct HaloPlan {
  bool ok = false;
  int items = 0, splits = 1, cper = 1;
  bool d2 = false;   // the 2D-tile kernel (conv_halo2d_kernel): 8 x 32 pixel tiles, mw = M tiles of 32 per block
  int mw = 2;
};
struct HaloS2Plan {
  bool ok = false;
  int items = 0, splits = 1, cper = 1;
};
struct WHaloPlan {
  bool ok = false;
  int r = 0, items = 0, nchunk = 0, splits = 1, cper = 1;
};
struct WPlan {
  int tile, BM, BN;
  int cw;          // channels per tap block (0: channel-major kernel)
  long ntiles_n;   // column tiles
  int splits, kper;
};
struct PhaseClass {
  int y0, x0, Hc, Wc, ntaps;
  int taps[16];
};

// ---- the route of a pass: which kernel runs it, decided once (conv_route.hip).  Packing, the
// workspace sizes and the launchers all read this; none of them tests a shape again.
enum PxKind { PX_HEAD, PX_STEM_S2D, PX_PX16, PX_HALO, PX_HALO2D, PX_REFLECT_HALO, PX_HALO_S2,
              PX_CLASSES_MERGED, PX_CLASSES4, PX_TILE };
enum PxArith { ARITH_PX, ARITH_PX2, ARITH_PX3 };   // the tile kernel: conv_px / conv_px2 / conv_px3
struct PxRoute {
  PxKind kind;
  PxArith arith;
  // the packed operand: layout 0 [Kpad][Mpad] fp32, 1 [Kpad/16][Mpad][16] fp32, 2 [Kpad/16][3][Mpad][16]
  // bf16 split terms; tap: tap-major K order
  int layout, tap, Kpad, Mpad;
  size_t packed_elems;
  Plan tile;           // always filled: the tile kinds' plan, and the fallback of a vetoed kind
  HaloPlan halo;       // PX_HALO, PX_HALO2D; PX_REFLECT_HALO: the plan of `ext`
  ConvShape ext;       // PX_REFLECT_HALO: the zero-padded dgrad on the (H+2) x (W+2) grid
  HaloS2Plan s2;       // PX_HALO_S2
  PhaseClass cls[4];   // the stride-2 dgrad's output-parity classes
  Plan cls_plan[4];    // PX_CLASSES4: one per class; PX_CLASSES_MERGED: [0], the one launch
  size_t ws_bytes;     // workspace of the kind and of what it can narrow to
};
// forward (mode 0) / data gradient (mode 1): a pure function of the shape and the tuning knobs
PxRoute conv_route(const ConvShape& s, int mode);
// the route that runs with the operands of one call (every operand condition is stated here)
PxRoute conv_fwd_narrow(PxRoute r, const ConvShape& s, const TensorIn& x, const TensorOut& y);
PxRoute conv_dgrad_narrow(PxRoute r, const ConvShape& s, const TensorOut& dx);

enum WKind { W_HEAD, W_WHALO, W_STEM_S2D, W_STEM, W_WGRAD16, W_TILE };
struct WRoute {
  WKind kind;
  WKind base;        // what a vetoed W_WHALO / W_STEM_S2D narrows to (from tile.tile)
  WPlan tile;
  WHaloPlan halo;
  int nsplit;        // slabs of `kind`; the bias partials sit behind them
  size_t ws_bytes;
};
// c0: channels of the first input tensor (>= Cin: one tensor)
WRoute conv_wgrad_route(const ConvShape& s, int c0);
WRoute conv_wgrad_narrow(WRoute r, const ConvShape& s, const TensorIn& x);

void fill_common(ConvArgs& a, const ConvShape& s);
int check_shape(const ConvShape& s);
int px3_terms();     // 6 or 9 products (MD2_PX3_TERMS, read here only)
int bias_parts(int C, long total);

// the LDS-halo kernels (conv_halo.inc, its own translation unit conv_halo.hip)
int halo_launch(int mode, const ConvArgs& a, int items, int splits, int reflect, hipStream_t st);
int halo2d_launch(int mode, const ConvArgs& a, int mw, int splits, int reflect, hipStream_t st);
int halo_s2_launch(const ConvArgs& a, int items, int splits, hipStream_t st);
int whalo_launch(const ConvArgs& a, int items, int ksteps, int splits, hipStream_t st);
// the ResNet stem forward on the space-to-depth grid (conv_stem.inc, translation unit conv_stem.hip)
int stem_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st);
int stem_wgrad_blocks(const ConvShape& s);
int stem_wgrad_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st);

}  // namespace md2
