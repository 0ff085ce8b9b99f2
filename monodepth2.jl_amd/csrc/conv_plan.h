// Host side of the conv passes: tile tables, plan structs, the planners and selection glue (defined
// once, in conv.hip: sizing and launching read the same plan) and the cross-unit launchers.
#pragma once
#include "conv_kernel.h"
#include "head.h"

namespace md2 {

constexpr int TARGET_BLOCKS = 1536;  // ~6 blocks (waves per SIMD) per CU on 256 CUs

// T128x64q: 128x64 with the 4 waves stacked along M (each 32 rows x 64 columns: its A rows are its
// own, B shared through LDS)
enum TileCfg { T128x128 = 0, T64x256 = 1, T32x256 = 2, T64x128 = 3, T128x64 = 4, T64x64 = 5, T32x128 = 6,
               T128x64q = 7 };
const int TILE_BM[] = {128, 64, 32, 64, 128, 64, 32, 128};
const int TILE_BN[] = {128, 256, 256, 128, 64, 64, 128, 64};

// wgrad tiles (BM x BN, 4 waves as WM x WN); columns are tap-major (tap groups x CW channels)
enum WTileCfg { W64x128 = 0, W32x256 = 1, W64x64 = 2, W32x128 = 3, W16x144 = 4, WSTEM = 5, W64x192 = 6 };
const int WT_BM[] = {64, 32, 64, 32, 16, 64, 64};
const int WT_BN[] = {128, 256, 64, 128, 144, 64, 192};

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

Plan plan_px(int M, long N, int K, bool bk32_ok = false, bool prefer32 = false);
HaloPlan plan_halo(const ConvShape& s, int mode);
HaloS2Plan plan_halo_s2(const ConvShape& s);
WHaloPlan plan_whalo(const ConvShape& s, int c0);
WPlan plan_wgrad(const ConvShape& s, int c0);
int wgrad_cw(const ConvShape& s, int c0, int BN);
ConvShape reflect_ext_shape(const ConvShape& s);
bool reflect_dgrad_on_halo(const ConvShape& s, HaloPlan* hp = nullptr);
size_t reflect_dgrad_ws(const ConvShape& s);
PhaseClass phase_class(const ConvShape& s, int cy, int cx);
void fill_common(ConvArgs& a, const ConvShape& s);
int check_shape(const ConvShape& s);
int px3_terms();
int bias_parts(int C, long total);
bool head_path(const ConvShape& s);

// the LDS-halo kernels (conv_halo.inc, its own translation unit conv_halo.hip)
int halo_launch(int mode, const ConvArgs& a, int items, int splits, int reflect, hipStream_t st);
int halo2d_launch(int mode, const ConvArgs& a, int mw, int splits, int reflect, hipStream_t st);
int halo_s2_launch(const ConvArgs& a, int items, int splits, hipStream_t st);
int whalo_launch(const ConvArgs& a, int items, int ksteps, int splits, hipStream_t st);
// the ResNet stem forward on the space-to-depth grid (conv_stem.inc, translation unit conv_stem.hip)
bool stem_s2d_applies(const ConvShape& s, const TensorIn& x, const TensorOut& y);
int stem_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st);
bool stem_wgrad_s2d_applies(const ConvShape& s, const TensorIn& x);
int stem_wgrad_blocks(const ConvShape& s);
int stem_wgrad_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st);

}  // namespace md2
