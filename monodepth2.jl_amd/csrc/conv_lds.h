// Dynamic-LDS geometry of the six conv kernels that size their shared memory at launch
// (conv_halo.inc, conv_stem.inc) -- stated ONCE: the kernels take their plane sizes and offsets
// from here, the planners (conv_route.hip plan_halo / plan_halo_s2 / plan_whalo,
// stem_*_applies) admit a shape with fits(), and the launchers allocate bytes() under the opt-in
// ceiling cap through lds_launch (conv_kernel.h), which refuses a launch with need() > bytes().
// A launcher that allocated another kernel's size used to compute garbage without a fault.
//
// Per kernel:  bytes(...)  the dynamic LDS of the launch
//              need(...)   one past the highest byte the kernel can touch for that geometry
//              cap         hipFuncAttributeMaxDynamicSharedMemorySize of the kernel
//              fits(...)   the planner's admission test (pure geometry)
// Plain constexpr C++17 without HIP types: tests/stubs/conv_lds_check.cpp reads it with a host
// compiler and sweeps  fits => need <= bytes <= cap.
#pragma once

#ifdef __HIPCC__
// (inlined before anything else: the kernels compile to the code of the written-out expressions)
#define MD2_LDS_FN __host__ __device__ __forceinline__ constexpr
#else
#define MD2_LDS_FN constexpr
#endif

namespace md2 {

// ---- conv_halo3 / conv_halo3s2: the flattened halo image of TN consecutive output pixels.
// 2 buffers x 3 part planes (hi, mid, lo) of PX pixels x 16 bf16; halo row pitch W + HX_PAD.
constexpr int HX_PAD = 16;               // halo row pitch = W + HX_PAD pixels (bank-conflict free)

template <int PX, int TN>
struct HaloFlatLds {
  static constexpr int plane = PX * 32;  // bytes per part plane (16 bf16 per pixel)
  static constexpr long cap = 6L * plane;
  MD2_LDS_FN static long bytes() { return cap; }
  MD2_LDS_FN static int pitch(int W) { return W + HX_PAD; }
  MD2_LDS_FN static int rows(int W) { return (TN - 1) / W + 4; }             // halo rows of TN consecutive pixels, at most
  MD2_LDS_FN static int zero_px(int HR, int W) { return HR * pitch(W); }     // zero pixels zero_px .. zero_px + 2
  MD2_LDS_FN static long pixels(int W) { return (long)rows(W) * pitch(W) + 3; }
  MD2_LDS_FN static long need(int W) { return 5L * plane + pixels(W) * 32; }  // the last plane of the second buffer
  MD2_LDS_FN static bool fits(int W) { return pixels(W) <= PX; }
};
constexpr int HX_PX = 736;               // halo pixels per part plane, zero pixels included (W = 104 + 2: the padded decoder grid)
constexpr int HS2_PX = 416;              // conv_halo3s2 (80 KB, not 141: the side stream's blocks still find LDS on its CU)
using Halo3Lds = HaloFlatLds<HX_PX, 256>;
using Halo3s2Lds = HaloFlatLds<HS2_PX, 128>;
constexpr int HX_PLANE = Halo3Lds::plane;
constexpr int HS2_PLANE = Halo3s2Lds::plane;

// ---- conv_halo2d: a fixed 8-row x 32-column tile with its one-pixel halo, planes as above
constexpr int H2_TH = 8, H2_TW = 32, H2_HR = H2_TH + 2, H2_PR = H2_TW + 2;   // tile, halo rows, pitch
constexpr int H2_PX = H2_HR * H2_PR;                                       // 340 staged pixels
constexpr int H2_PLANE = H2_PX * 32;                                       // bytes per part plane
struct Halo2dLds {
  static constexpr long cap = 6L * H2_PLANE;
  MD2_LDS_FN static long bytes() { return cap; }
  MD2_LDS_FN static long need() { return cap; }   // every tile stages all H2_PX pixels
  MD2_LDS_FN static bool fits() { return true; }
};

// ---- conv_whalo: r image rows + 2 halo rows of W + 2 pixels and three zero pixels, 3 part
// planes of 64 B per pixel (32 channels), then the k table (one word per chunk pixel of the
// 16-pixel k-steps)
struct WHaloLds {
  static constexpr long cap = 65536;     // two blocks per CU
  static constexpr int KS_MAX = 7;       // k-steps per chunk, at most (r * W <= 112)
  MD2_LDS_FN static int pitch(int W) { return W + 2; }
  MD2_LDS_FN static int zero_px(int r, int W) { return (r + 2) * pitch(W); }  // zero pixels zero_px .. zero_px + 2
  MD2_LDS_FN static int plane(int zero_px) { return (zero_px + 3) * 64; }    // bytes per part plane
  MD2_LDS_FN static int ktab(int plane) { return 3 * plane; }                 // byte offset of the k table: behind the planes
  MD2_LDS_FN static long need(int r, int W, int ksteps) { return (long)ktab(plane(zero_px(r, W))) + 16L * ksteps * 4; }
  MD2_LDS_FN static long bytes(int r, int W) { return need(r, W, KS_MAX); }
  MD2_LDS_FN static bool fits(int r, int W) { return bytes(r, W) <= cap; }
};

// ---- the stem kernels: a ring of 5 s2d rows of P records (32 B), 3 part planes
struct StemRingLds {
  static constexpr long cap = 163840;    // 160 KB, one block per CU
  MD2_LDS_FN static int plane(int P) { return 5 * P * 32; }
  MD2_LDS_FN static long ring(int P) { return 3L * 5 * P * 32; }
};
// conv_stem_s2d: records for the columns -2 .. Wo (Wo <= 338: <= 21 subtiles per row)
struct StemLds : StemRingLds {
  MD2_LDS_FN static int pitch(int Wo) { return Wo + 3; }
  MD2_LDS_FN static long bytes(int P) { return ring(P); }
  MD2_LDS_FN static long need(int P) { return ring(P); }
  MD2_LDS_FN static bool fits(int Wo) { return bytes(pitch(Wo)) <= cap; }
};
// conv_wgrad_stem_s2d: ring pitch a multiple of 8 records covering round_up(Wo, 32) + 3 columns,
// one record per thread (512); after the last row the ring is overlaid by the K-step-parity
// combine: [4 filter quarters][TILES][4][64 lanes] floats at offset 0
struct StemWgradLds : StemRingLds {
  static constexpr int TILES = 13;
  static constexpr int red_quarter = TILES * 4 * 64;    // floats per filter quarter
  static constexpr long red_bytes = 4L * red_quarter * 4;
  MD2_LDS_FN static int pitch(int Wo) { return ((Wo + 31) / 32 * 32 + 3 + 7) / 8 * 8; }
  MD2_LDS_FN static long need(int P) { return ring(P) > red_bytes ? ring(P) : red_bytes; }
  MD2_LDS_FN static long bytes(int P) { return need(P); }
  MD2_LDS_FN static bool fits(int Wo) { return pitch(Wo) <= 512 && ring(pitch(Wo)) <= cap; }
};

}  // namespace md2
