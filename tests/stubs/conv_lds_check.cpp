// Host-only check of csrc/conv_lds.h (tests/test_conv_lds.py compiles and runs it; no GPU, no
// library): for every geometry a planner can see,
//   fits  =>  need <= bytes <= cap          (a launch gets the LDS its kernel indexes)
//   fits  ==  the planner's admission test as it was written out in the planners (now conv_route.hip)
//             before the geometry moved into the header (kept here literally: no planner
//             decision changes)
// and every bench-shape geometry is still admitted, the fixed sizes are the known ones.
#include <cstdio>
#include <initializer_list>

#include "conv_lds.h"

using namespace md2;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (++failures <= 20) {                  \
        std::printf("FAIL %s: ", #cond);       \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

static long cdiv(long a, long b) { return (a + b - 1) / b; }
static long round_up(long a, long b) { return (a + b - 1) / b * b; }

// plan_whalo's rows per chunk: the largest divisor of H with r * W <= 112 (0: none)
static int whalo_rows(int H, int W) {
  int r = 0;
  for (int d = 1; d <= H; ++d)
    if (H % d == 0 && d * W <= 112) r = d;
  return r;
}

int main() {
  long admitted[5] = {0, 0, 0, 0, 0};

  // conv_halo3: plan_halo's flat path (W includes the padded W + 2 extents of the reflect dgrad)
  for (int W = 1; W <= 512; ++W) {
    const int hrmax = 255 / W + 4;
    const bool was = hrmax * (W + 16) + 3 <= 736;
    CHECK(Halo3Lds::fits(W) == was, "halo3 W=%d", W);
    CHECK(Halo3Lds::rows(W) == hrmax, "halo3 W=%d", W);
    if (!Halo3Lds::fits(W)) continue;
    ++admitted[0];
    CHECK(Halo3Lds::need(W) <= Halo3Lds::bytes() && Halo3Lds::bytes() <= Halo3Lds::cap, "halo3 W=%d need %ld", W, Halo3Lds::need(W));
    CHECK(cdiv((long)hrmax * W, 512) <= 2, "halo3 W=%d: at most two staged pixels per thread", W);
    // the kernel's zero pixels for the most halo rows a block can have end inside a plane
    CHECK((Halo3Lds::zero_px(hrmax, W) + 3) * 32 <= Halo3Lds::plane, "halo3 W=%d", W);
  }
  // conv_halo3s2: plan_halo_s2
  for (int Wo = 1; Wo <= 256; ++Wo) {
    const int hrmax = 127 / Wo + 4;
    const bool was = !(hrmax * (Wo + 16) + 3 > 416);
    CHECK(Halo3s2Lds::fits(Wo) == was, "halo3s2 Wo=%d", Wo);
    if (!Halo3s2Lds::fits(Wo)) continue;
    ++admitted[1];
    CHECK(Halo3s2Lds::need(Wo) <= Halo3s2Lds::bytes() && Halo3s2Lds::bytes() <= Halo3s2Lds::cap, "halo3s2 Wo=%d need %ld", Wo, Halo3s2Lds::need(Wo));
    CHECK((long)hrmax * Wo <= 512, "halo3s2 Wo=%d: one staged pixel per thread", Wo);
    CHECK((Halo3s2Lds::zero_px(hrmax, Wo) + 3) * 32 <= Halo3s2Lds::plane, "halo3s2 Wo=%d", Wo);
  }
  // conv_halo2d: a fixed tile
  CHECK(Halo2dLds::fits() && Halo2dLds::need() <= Halo2dLds::bytes() && Halo2dLds::bytes() <= Halo2dLds::cap, "halo2d");
  CHECK(H2_PX == 340 && H2_PLANE == H2_PX * 32, "halo2d");
  // conv_whalo: plan_whalo with its choice of r
  for (int H = 1; H <= 64; ++H)
    for (int W = 1; W <= 112; ++W) {
      const int r = whalo_rows(H, W);
      if (r == 0) continue;
      const bool was = !(3L * (((r + 2) * (W + 2) + 3) * 64) + 448 > 65536);
      CHECK(WHaloLds::fits(r, W) == was, "whalo H=%d W=%d r=%d", H, W, r);
      if (!WHaloLds::fits(r, W)) continue;
      ++admitted[2];
      const int ksteps = (int)cdiv(r * W, 16);
      CHECK(ksteps <= WHaloLds::KS_MAX, "whalo H=%d W=%d r=%d", H, W, r);
      CHECK(WHaloLds::need(r, W, ksteps) <= WHaloLds::bytes(r, W) && WHaloLds::bytes(r, W) <= WHaloLds::cap,
            "whalo H=%d W=%d r=%d need %ld bytes %ld", H, W, r, WHaloLds::need(r, W, ksteps), WHaloLds::bytes(r, W));
      const int plane = WHaloLds::plane(WHaloLds::zero_px(r, W));   // as the kernel chains them
      CHECK(WHaloLds::ktab(plane) + 448 == WHaloLds::bytes(r, W) && plane == ((r + 2) * (W + 2) + 3) * 64,
            "whalo H=%d W=%d r=%d", H, W, r);
    }
  // the stem forward and filter gradient: stem_s2d_applies / stem_wgrad_s2d_applies
  for (int Wo = 16; Wo <= 512; Wo += 16) {
    const bool was = !(3L * 5 * (Wo + 3) * 32 > 163840);
    CHECK(StemLds::fits(Wo) == was, "stem Wo=%d", Wo);
    if (StemLds::fits(Wo)) {
      ++admitted[3];
      const int P = StemLds::pitch(Wo);
      CHECK(P == Wo + 3 && P <= 512, "stem Wo=%d: one record per thread", Wo);
      CHECK(StemLds::need(P) <= StemLds::bytes(P) && StemLds::bytes(P) <= StemLds::cap, "stem Wo=%d", Wo);
      CHECK(3L * StemLds::plane(P) == StemLds::bytes(P), "stem Wo=%d", Wo);
    }
    const long pitch = round_up(round_up(Wo, 32) + 3, 8);
    const bool wwas = pitch <= 512 && 15L * pitch * 32 <= 163840;
    CHECK(StemWgradLds::pitch(Wo) == pitch, "stem wgrad Wo=%d", Wo);
    CHECK(StemWgradLds::fits(Wo) == wwas, "stem wgrad Wo=%d", Wo);
    if (StemWgradLds::fits(Wo)) {
      ++admitted[4];
      const int P = StemWgradLds::pitch(Wo);
      CHECK(StemWgradLds::need(P) <= StemWgradLds::bytes(P) && StemWgradLds::bytes(P) <= StemWgradLds::cap, "stem wgrad Wo=%d", Wo);
      CHECK(StemWgradLds::bytes(P) >= 3L * StemWgradLds::plane(P) && StemWgradLds::bytes(P) >= StemWgradLds::red_bytes, "stem wgrad Wo=%d", Wo);
      // the transposed reads reach record 32 ceil(Wo / 32) + 2 of a ring slot
      CHECK(32 * cdiv(Wo, 32) + 2 < P, "stem wgrad Wo=%d", Wo);
    }
  }
  CHECK(StemWgradLds::red_bytes == 4L * 13 * 4 * 64 * 4, "stem wgrad combine buffer");

  // the bench shapes stay on these kernels
  for (int W : {104, 106, 52, 26, 13}) CHECK(Halo3Lds::fits(W), "bench halo3 W=%d", W);
  for (int Wo : {52, 26, 13}) CHECK(Halo3s2Lds::fits(Wo), "bench halo3s2 Wo=%d", Wo);
  const int whw[4][2] = {{32, 104}, {16, 52}, {8, 26}, {4, 13}};
  for (const auto& hw : whw) {
    const int r = whalo_rows(hw[0], hw[1]);
    CHECK(r > 0 && WHaloLds::fits(r, hw[1]), "bench whalo H=%d W=%d", hw[0], hw[1]);
  }
  CHECK(StemLds::fits(208) && StemWgradLds::fits(208), "bench stem Wo=208");

  // the sizes the launches have always had
  CHECK(Halo3Lds::bytes() == 141312, "halo3 bytes %ld", Halo3Lds::bytes());
  CHECK(Halo3s2Lds::bytes() == 79872, "halo3s2 bytes %ld", Halo3s2Lds::bytes());
  CHECK(Halo2dLds::bytes() == 65280, "halo2d bytes %ld", Halo2dLds::bytes());
  CHECK(WHaloLds::bytes(whalo_rows(32, 104), 104) == 62080, "whalo (32, 104) bytes %ld", WHaloLds::bytes(whalo_rows(32, 104), 104));
  CHECK(WHaloLds::cap == 65536 && StemLds::cap == 163840 && StemWgradLds::cap == 163840, "caps");
  CHECK(StemLds::bytes(StemLds::pitch(208)) == 3L * 5 * 211 * 32, "stem bytes");
  CHECK(StemWgradLds::bytes(StemWgradLds::pitch(208)) == 15L * 232 * 32, "stem wgrad bytes");

  for (int i = 0; i < 5; ++i) CHECK(admitted[i] > 0, "sweep %d admitted nothing", i);
  std::printf("conv_lds_check: admitted halo3 %ld, halo3s2 %ld, whalo %ld, stem %ld, stem wgrad %ld; %d failures\n",
              admitted[0], admitted[1], admitted[2], admitted[3], admitted[4], failures);
  return failures ? 1 : 0;
}
