// ---------------------------------------------------------------------------------------------
// The ResNet stem forward (7x7, stride 2, pad 3, 3 image channels, 64 filters; ResNet.jl's first
// conv, src/model.jl:31 runs it on every frame) on bf16x6 split products with 16x16x32 MFMAs
// (its own translation unit, conv_stem.hip).
//
// conv_px_kernel ran it as an fp32-MFMA implicit GEMM over K = 147 gathered (c, ky, kx) columns:
// 154 us per step at the bench shape, 37% of the fp32 MFMA peak.  Here it is a stride-1 4x4 conv
// over the SPACE-TO-DEPTH grid of the image:
//   ky = 2 dY + py + 3, kx = 2 dX + px + 3   (dY, dX in -2..1; py, px in 0..1)
//   x[c][2y - 3 + ky][2x - 3 + kx] = S[c, py, px][y + dY][x + dX],  S[c,py,px][Y][X] = x[c][2Y+py][2X+px]
// so output row y reads the four s2d rows y-2..y+1 and every tap is an aligned record shift.
//
//   Block: a band of consecutive output rows (one block per CU, 512 threads = 8 waves: 4 filter
//      quarters x 2 subtile parities), the s2d rows in a 5-slot LDS ring: each new row costs one
//      staged s2d row, loaded behind the previous row's MFMAs.
//   LDS image: ring slots of W/2 + 3 records (columns -2 .. Wo; outside the image the records are
//      zero), three part planes (hi, mid, lo bf16).  A record is 16 bf16 slots = two
//      halves: h0 = py 1 [(px 1: c0 c1 c2) (px 0: c0 c1 c2) 0 0], h1 = py 0 likewise.
//   K: 16x16x32 MFMAs take 8 k-values per 16-lane group, and each group may read its own record
//      half: the 147 weights fill 28 "quarter units" (tap, half) -- h0 of all 16 taps, h1 of the
//      12 taps with dY >= -1 (dY = -2 rows exist only at py = 1) -- i.e. 7 K-steps of 32 instead
//      of ceil(147 / 16) = 10 zero-padded 16-deep chunks of 49-tap gathers.
//   A (weights): built once per block straight from the packed fp32 weights ([Kpad][Mpad],
//      k = c * 49 + ky * 7 + kx) and split in registers: 7 K-steps x 3 parts = 84 VGPRs.
//   Epilogue: the fp32 rows.  (BatchNorm statistics in this epilogue -- fp64 per value, two
//      partials per block, collapsed -- measured 6.29 vs 6.27 ms per step against the separate
//      statistics pass: the fp64 sums cost the kernel ~30 us, the pass ~18; not kept.)
// ---------------------------------------------------------------------------------------------

typedef float stem_f32x4 __attribute__((ext_vector_type(4)));

// quarter unit u (K-step u / 4, lane group u % 4) -> tap (dY, dX) and record half h.  The two
// groups sharing a ds_read_b128 phase (0/1, 2/3) read different halves where the counts allow
// (12 of 14 pairs): then their 16-byte reads cover 16 distinct bank groups.
__device__ __forceinline__ void stem_unit(int u, int& dY, int& dX, int& h) {
  const int k = u >> 1, mem = u & 1;
  int tap;
  if (k < 12) {
    tap = mem == 0 ? k : 4 + k;            // (h0 of tap k, h1 of tap 4 + k)
    h = mem;
  } else {
    tap = 12 + 2 * (k - 12) + mem;         // the last four h0 units
    h = 0;
  }
  dY = (tap >> 2) - 2;
  dX = (tap & 3) - 2;
}

// B fragments of K-step s for the subtiles t and t + 2 (clamped to the row: a single-subtile
// item reads a real subtile twice) into buffer set `set`
__device__ __forceinline__ void stem_read_b(u32x4_t (&fb)[2][2][3], int set, const uint8_t* lds, uint32_t plane,
                                            uint32_t off, int t, int T) {
  const uint32_t o0 = off + (uint32_t)t * 512u, o1 = off + (uint32_t)min(t + 2, T - 1) * 512u;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    fb[set][0][p] = *reinterpret_cast<const u32x4_t*>(lds + p * plane + o0);
    fb[set][1][p] = *reinterpret_cast<const u32x4_t*>(lds + p * plane + o1);
  }
}

// One item: G output subtiles of 16 pixels (t, t + 2) x this wave's 16 filters.  Its K-step 0
// fragments were read into set P0 by the previous item (or the row prologue); K-step s + 1's
// (and at the last K-step the NEXT item's first, when tn >= 0) are issued before K-step s's
// MFMAs -- a scheduling barrier pins that order (hipcc otherwise moved each read next to its
// first use and waited for it there).
template <int G, int P0, int FL>
__device__ __forceinline__ void stem_item(u32x4_t (&fb)[2][2][3], const uint8_t* lds, uint32_t plane,
                                          const uint32_t (&uoff)[7], int t, int tn, int T,
                                          const u32x4_t (&ah)[7], const u32x4_t (&am)[7],
                                          const u32x4_t (&al)[7], float* outp, long HoWo, int mrow,
                                          int n) {
  stem_f32x4 c0[G], c1[G];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) c0[g][i] = c1[g][i] = 0.f;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int cur = (P0 + s) & 1;
    if (s < 6)
      stem_read_b(fb, cur ^ 1, lds, plane, uoff[s + 1], t, T);
    else if (tn >= 0)
      stem_read_b(fb, cur ^ 1, lds, plane, uoff[0], tn, T);
    if constexpr ((FL & 16) == 0) __builtin_amdgcn_sched_barrier(0);
    const bf16x8_t Ah = __builtin_bit_cast(bf16x8_t, ah[s]);
    const bf16x8_t Am = __builtin_bit_cast(bf16x8_t, am[s]);
    const bf16x8_t Al = __builtin_bit_cast(bf16x8_t, al[s]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bf16x8_t Bh = __builtin_bit_cast(bf16x8_t, fb[cur][g][0]);
      const bf16x8_t Bm = __builtin_bit_cast(bf16x8_t, fb[cur][g][1]);
      const bf16x8_t Bl = __builtin_bit_cast(bf16x8_t, fb[cur][g][2]);
      if constexpr ((FL & 2) != 0) {     // timing only: no MFMAs
        c1[g][0] += __builtin_bit_cast(float, fb[cur][g][0][0] ^ fb[cur][g][1][1] ^ fb[cur][g][2][2] ^ ah[s][0] ^ am[s][1] ^ al[s][2]);
        continue;
      }
      stem_f32x4 c = c1[g];
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Am, Bm, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Am, Bh, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bm, c, 0, 0, 0);
      c1[g] = c;
      c0[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, c0[g], 0, 0, 0);
    }
  }
  if constexpr ((FL & 4) != 0) {         // timing only: no stores
    if (c0[0][0] + c1[0][0] != 1234.5f) return;
  }
  // C layout: lane (n, q) holds rows 4q + i, column n
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int x = (t + 2 * g) * 16 + n;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = c0[g][i] + c1[g][i];
      outp[(long)(mrow + i) * HoWo + x] = v;
    }
  }
}

// Persistent bands: block b computes the output rows L0 .. L1 - 1 of the flattened (image, row)
// sequence (NR / gridDim rows each) with the s2d rows in a 5-slot LDS ring (row Y in slot
// (Y + 10) % 5): the four rows of the first row (and of each new image) are staged up front,
// then every row's compute overlaps the loads of the one new s2d row the next row needs, which
// is split and written into the slot the current row no longer reads.  8 waves: wave w holds
// filters 16 (w & 3) .. + 15 and takes every other 16-pixel subtile of a row (the parity
// alternates with the row, so the two waves of a filter quarter share the odd subtile count).
// FL: timing-only kernels (results wrong): bit 1 = no MFMAs, bit 2 = no output stores, bit 3 = no
// per-row staging; bit 4 (a valid result): no scheduling barrier in the K-steps.  Only FL = 0 is
// in the library; a -DMD2_TIMING_VARIANTS=1 build of this unit (tools/build_variant.sh) adds the
// variants of stem_s2d_launch, selected there by MD2_TUNING=1 MD2_STEM_DBG=k
template <int FL>
__global__ __launch_bounds__(512, 1) void conv_stem_s2d_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = wv & 3, sp = wv >> 2;
  const int Ho = a.Ho, Wo = a.Wo, W = a.W;
  const int P = StemLds::pitch(Wo);                      // records per s2d row (columns -2 .. Wo)
  const uint32_t plane = (uint32_t)StemLds::plane(P);    // bytes per part plane (5 ring slots)
  const uint32_t NR = (uint32_t)(a.g.N / Wo);            // output rows of all images
  const uint32_t nb = gridDim.x, b = blockIdx.x;
  const uint32_t L0 = (uint32_t)((uint64_t)b * NR / nb), L1 = (uint32_t)((uint64_t)(b + 1) * NR / nb);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.in.p0, a.b0_bytes);
  const uint32_t W4 = (uint32_t)W * 4u;

  // ---- one record per thread (tid < P) of s2d row Y of image img: six 8-byte loads (c, py) of
  // the pixel pair (2X, 2X + 1); outside the image the offset is OOB (zeros)
  auto rec_off = [&](uint32_t img, int Y) -> uint32_t {
    const uint32_t qb = fdiv(img, a.fd_bdiv);
    const uint32_t ibase = (img - qb * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + qb * (uint32_t)a.in.bhi;
    const int X = tid - 2;
    const bool ok = tid < P && Y >= 0 && Y < Ho && X >= 0 && X < Wo;
    return ok ? (ibase + (uint32_t)(2 * Y) * (uint32_t)W + 2u * (uint32_t)X) * 4u : OOB;
  };
  // v[2 c + py] = (column 2X, column 2X + 1) of channel c, row 2Y + py
  auto stage_load = [&](uint32_t voff, float2* v) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int py = 0; py < 2; ++py) v[2 * c + py] = bload2_s(rx, voff, (uint32_t)c * a.HW4 + (uint32_t)py * W4);
  };
  // split into the record halves (slots: px 1 (c0 c1 c2), px 0 (c0 c1 c2), 0, 0; .y = column
  // 2X + 1) and write the three part planes of ring slot (Y + 10) % 5
  auto stage_write = [&](int Y, const float2* v) {
    uint8_t* rec = lds + (uint32_t)(((Y + 10) % 5) * P + tid) * 32u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int py = 1 - h;
      uint32_t p0h, p0m, p0l, p1h, p1m, p1l, p2h, p2m, p2l;
      split3_pk(v[py].y, v[2 + py].y, p0h, p0m, p0l);
      split3_pk(v[4 + py].y, v[py].x, p1h, p1m, p1l);
      split3_pk(v[2 + py].x, v[4 + py].x, p2h, p2m, p2l);
      uint8_t* dst = rec + (uint32_t)h * 16u;
      *reinterpret_cast<u32x4_t*>(dst) = u32x4_t{p0h, p1h, p2h, 0u};
      *reinterpret_cast<u32x4_t*>(dst + plane) = u32x4_t{p0m, p1m, p2m, 0u};
      *reinterpret_cast<u32x4_t*>(dst + 2 * plane) = u32x4_t{p0l, p1l, p2l, 0u};
    }
  };

  // ---- A fragments (once per block): lane (n, q) holds filter 16 fq + n, the 8 slots of unit
  // 4 s + q; the unit's tap row dY and record offset are kept for the per-row ring addresses
  const int n = lane & 15, q = lane >> 4;
  const int m = fq * 16 + n;
  const int Mpad = a.g.Mpad;
  u32x4_t ah[7], am[7], al[7];
  int udy[7];
  uint32_t ucol[7];
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    int dY, dX, h;
    stem_unit(4 * s + q, dY, dX, h);
    udy[s] = dY;
    ucol[s] = (uint32_t)((dX + 2 + n) * 32 + h * 16);
    const int py = 1 - h, ky = 2 * dY + py + 3;
    float v[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int px = jj < 3 ? 1 : 0, c = jj % 3, kx = 2 * dX + px + 3;
      const bool ok = jj < 6 && ky >= 0 && ky <= 6 && kx >= 0 && kx <= 6;
      const float w = a.A[ok ? (long)(c * 49 + ky * 7 + kx) * Mpad + m : 0];   // always a valid address
      v[jj] = ok ? w : 0.f;
    }
    uint32_t hh[4], mm[4], ll[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) split3_pk(v[2 * p], v[2 * p + 1], hh[p], mm[p], ll[p]);
    ah[s] = u32x4_t{hh[0], hh[1], hh[2], hh[3]};
    am[s] = u32x4_t{mm[0], mm[1], mm[2], mm[3]};
    al[s] = u32x4_t{ll[0], ll[1], ll[2], ll[3]};
  }

  const int T = Wo >> 4;
  const long HoWo = (long)Ho * Wo;
  const int mrow = fq * 16 + 4 * q;
  uint32_t cur = 0xffffffffu;
  for (uint32_t L = L0; L < L1; ++L) {
    const uint32_t img = L / (uint32_t)Ho;
    const int y = (int)(L - img * (uint32_t)Ho);
    if (img != cur) {                      // block-uniform: the four rows of a first row
      float2 v4[24];
#pragma unroll
      for (int j = 0; j < 4; ++j) stage_load(rec_off(img, y - 2 + j), v4 + 6 * j);
      if (tid < P) {
#pragma unroll
        for (int j = 0; j < 4; ++j) stage_write(y - 2 + j, v4 + 6 * j);
      }
      __syncthreads();
      cur = img;
    }
    // the next row continues this image: its new s2d row y + 2 (zeros past the image) is
    // loaded behind this row's MFMAs
    const bool pipe = (FL & 8) == 0 && L + 1 < L1 && y + 1 < Ho;
    float2 vn[6];
    stage_load(pipe ? rec_off(img, y + 2) : OOB, vn);
    uint32_t uoff[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) uoff[s] = (uint32_t)(((y + udy[s] + 10) % 5) * P) * 32u + ucol[s];
    float* outp = a.out.p0 + (long)img * a.out.bs0 + (long)y * Wo;
    // items (t0 + 4k, t0 + 4k + 2), k = 0..5 (T <= 21), the last one possibly a single subtile;
    // unrolled (a runtime loop here made hipcc drain vmcnt at its header, i.e. wait for the
    // staging loads above before the first MFMA)
    const int t0 = (sp + (int)(L - L0)) & 1;
    u32x4_t fb[2][2][3];
    stem_read_b(fb, 0, lds, plane, uoff[0], t0, T);
#define MD2_STEM_ITEM(K)                                                                         \
    {                                                                                            \
      const int t = t0 + 4 * K, tn = t + 4 < T ? t + 4 : -1;                                     \
      if (t + 2 < T)                                                                             \
        stem_item<2, K & 1, FL>(fb, lds, plane, uoff, t, tn, T, ah, am, al, outp, HoWo, mrow, n); \
      else if (t < T)                                                                            \
        stem_item<1, K & 1, FL>(fb, lds, plane, uoff, t, tn, T, ah, am, al, outp, HoWo, mrow, n); \
    }
    MD2_STEM_ITEM(0) MD2_STEM_ITEM(1) MD2_STEM_ITEM(2) MD2_STEM_ITEM(3) MD2_STEM_ITEM(4) MD2_STEM_ITEM(5)
#undef MD2_STEM_ITEM
    if (pipe && tid < P) stage_write(y + 2, vn);   // slot of row y - 3: not read by row y
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// The stem's filter gradient on the same s2d rows: dW[m][c][ky][kx] = sum_p dY[m][p] x[c][...],
// as C[m][column] = sum_p dY[m][p] S[column](p) on 16x16x32 bf16x6 MFMAs with K = output pixels.
//   Columns: "quads" of the s2d record -- 4 slots (channels 0..2 + one zero) of one (py, px) at
//      tap (dY, dX); 49 quads carry the 147 weights (py = 0 needs dY >= -1, px = 0 needs dX >= -1).
//      An N tile of 16 columns = 4 quads: the 9 full taps (dY, dX >= -1) one tile each, three
//      tiles mixing one (py 1, px 1) / (py 1, px 0) / (py 0, px 1) quad of the edge taps (+ one
//      discarded quad), and the four (dY = -2, py 1, px 1) quads: 13 tiles (196 live columns).
//   B: ds_read_b64_tr_b16 -- lane 4q + p of a 16-lane group addresses pixel row q, quad p (8 B):
//      each lane of a group may take its own tap, so a tile's quads come from any (dY, dX).
//      K order: the 32 pixels of a K-step enumerate as (t, g, q) -> 16 t + 4 g + q, so the two
//      groups of a 32-lane half read 8 consecutive pixel records (256 B: conflict-free on the
//      full-tap tiles) -- and dY's A fragment is the same permutation (two 16-byte loads).
//   Record layout (wgrad): slots 4 Qd + c, Qd = 2 (1 - py) + (1 - px); the ring pitch P is a
//      multiple of 8 records (slots on 256-byte boundaries) covering pixels up to round_up(Wo, 32).
//   Waves: 8 = 4 filter quarters x 2 tile parities (7 / 6 tiles, one of each on every SIMD);
//      bands of rows per block as the forward kernel; rows are ceil(Wo / 32) K-steps of 32 pixels
//      (ragged tail: dY reads zeros past Wo, the staged records there are zero).  Output: the block's slab [block][64][147] (channel-major
//      columns c * 49 + ky * 7 + kx), summed by wgrad_reduce_kernel.
// ---------------------------------------------------------------------------------------------
typedef short stem_v4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 stem_tr16(const uint8_t* p) {
  const stem_v4s v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) stem_v4s*)p);
  return __builtin_bit_cast(uint2, v);
}

__device__ __forceinline__ void stem_wquad(int T, int p, int& dY, int& dX, int& Qd) {
  if (T < 9) {
    dY = T / 3 - 1;
    dX = T % 3 - 1;
    Qd = p;
  } else if (T < 12) {
    const int d = T - 10;
    if (p == 1) {
      dY = -2;
      dX = d;
    } else {
      dY = d;
      dX = -2;
    }
    Qd = p;                               // p = 3: a discarded quad (a valid address)
  } else {
    dY = -2;
    dX = p - 2;
    Qd = 0;
  }
}

// DBG (timing only; results wrong): bit 0 no MFMAs, bit 1 no dY loads, bit 2 no transposed B
// reads, bit 3 no per-row staging.  Only DBG = 0 is in the library; a -DMD2_TIMING_VARIANTS=1
// build of this unit (tools/build_variant.sh) adds the variants of stem_wgrad_s2d_launch,
// selected there by MD2_TUNING=1 MD2_WSTEM_DBG=k
template <int DBG = 0>
__global__ __launch_bounds__(512, 1) void conv_wgrad_stem_s2d_kernel(ConvArgs a, int P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = wv & 3, sp = wv >> 2;                  // filter quarter, K-step parity
  const int Ho = a.Ho, Wo = a.Wo, W = a.W;
  const uint32_t plane = (uint32_t)StemWgradLds::plane(P);
  const uint32_t NR = (uint32_t)((long)a.g.K / Wo);      // output rows of all images
  const uint32_t nb = gridDim.x, b = blockIdx.x;
  const uint32_t L0 = (uint32_t)((uint64_t)b * NR / nb), L1 = (uint32_t)((uint64_t)(b + 1) * NR / nb);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.in.p0, a.b0_bytes);
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(a.dy, a.A_bytes);
  const uint32_t W4 = (uint32_t)W * 4u;
  const uint32_t HoWo = (uint32_t)(Ho * Wo);

  auto rec_off = [&](uint32_t img, int Y) -> uint32_t {
    const uint32_t qb = fdiv(img, a.fd_bdiv);
    const uint32_t ibase = (img - qb * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + qb * (uint32_t)a.in.bhi;
    const int X = tid - 2;
    const bool ok = tid < P && Y >= 0 && Y < Ho && X >= 0 && X < Wo;
    return ok ? (ibase + (uint32_t)(2 * Y) * (uint32_t)W + 2u * (uint32_t)X) * 4u : OOB;
  };
  auto stage_load = [&](uint32_t voff, float2* v) {   // v[2 c + py] = (column 2X, 2X + 1)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int py = 0; py < 2; ++py) v[2 * c + py] = bload2_s(rx, voff, (uint32_t)c * a.HW4 + (uint32_t)py * W4);
  };
  // quads Qd = 0 (py 1, px 1), 1 (py 1, px 0), 2 (py 0, px 1), 3 (py 0, px 0): [c0 c1 c2 0] each
  auto stage_write = [&](int Y, const float2* v) {
    uint8_t* rec = lds + (uint32_t)(((Y + 10) % 5) * P + tid) * 32u;
    float q[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      q[0][c] = v[2 * c + 1].y;
      q[1][c] = v[2 * c + 1].x;
      q[2][c] = v[2 * c].y;
      q[3][c] = v[2 * c].x;
    }
    uint32_t hp[8], mp[8], lp[8];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      split3_pk(q[d][0], q[d][1], hp[2 * d], mp[2 * d], lp[2 * d]);
      split3_pk(q[d][2], 0.f, hp[2 * d + 1], mp[2 * d + 1], lp[2 * d + 1]);
    }
    *reinterpret_cast<u32x4_t*>(rec) = u32x4_t{hp[0], hp[1], hp[2], hp[3]};
    *reinterpret_cast<u32x4_t*>(rec + 16) = u32x4_t{hp[4], hp[5], hp[6], hp[7]};
    *reinterpret_cast<u32x4_t*>(rec + plane) = u32x4_t{mp[0], mp[1], mp[2], mp[3]};
    *reinterpret_cast<u32x4_t*>(rec + plane + 16) = u32x4_t{mp[4], mp[5], mp[6], mp[7]};
    *reinterpret_cast<u32x4_t*>(rec + 2 * plane) = u32x4_t{lp[0], lp[1], lp[2], lp[3]};
    *reinterpret_cast<u32x4_t*>(rec + 2 * plane + 16) = u32x4_t{lp[4], lp[5], lp[6], lp[7]};
  };

  // ---- this lane's quads: tile T = i, quad p = lane & 3, pixel row q = (lane >> 2) & 3.  The two
  // waves of a filter quarter (on one SIMD) take the even / odd K-steps of every row over all 13
  // tiles, so each dY fragment is loaded and split once (two waves splitting tile halves loaded and
  // split every fragment twice); their partial sums meet in LDS at the end.
  const int p4 = lane & 3, q4 = (lane >> 2) & 3, g = lane >> 4, n = lane & 15;
  constexpr int NT = StemWgradLds::TILES;
  int tdy[NT];
  uint32_t tcol[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    int dY, dX, Qd;
    stem_wquad(i, p4, dY, dX, Qd);
    tdy[i] = dY;
    tcol[i] = (uint32_t)((dX + 2 + 4 * g + q4) * 32 + Qd * 8);
  }
  const int m = mt * 16 + n;                             // A row (dY filter) of this lane

  stem_f32x4 c0[NT], c1[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) c0[i][e] = c1[i][e] = 0.f;

  uint32_t cur = 0xffffffffu;
  for (uint32_t L = L0; L < L1; ++L) {
    const uint32_t img = L / (uint32_t)Ho;
    const int y = (int)(L - img * (uint32_t)Ho);
    if (img != cur) {                      // block-uniform: the four rows of a first row
      float2 v4[24];
#pragma unroll
      for (int j = 0; j < 4; ++j) stage_load(rec_off(img, y - 2 + j), v4 + 6 * j);
      if (tid < P) {
#pragma unroll
        for (int j = 0; j < 4; ++j) stage_write(y - 2 + j, v4 + 6 * j);
      }
      __syncthreads();
      cur = img;
    }
    const bool pipe = (DBG & 8) == 0 && L + 1 < L1 && y + 1 < Ho;
    float2 vn[6];
    stage_load(pipe ? rec_off(img, y + 2) : OOB, vn);
    uint32_t tb[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) tb[i] = (uint32_t)(((y + tdy[i] + 10) % 5) * P) * 32u + tcol[i];
    // dY row y of filter m: pixels 32 kk + 4 g + (0..3) and 32 kk + 16 + 4 g + (0..3)
    const uint32_t yrow = (img * (uint32_t)a.Cout + (uint32_t)m) * HoWo + (uint32_t)(y * Wo);
    auto load_a = [&](int kk, float4& u0, float4& u1) {
      const int x0 = 32 * kk + 4 * g;
      if constexpr ((DBG & 2) != 0) {
        u0 = make_float4((float)x0, 1.f, 2.f, 3.f);
        u1 = make_float4(4.f, (float)kk, 6.f, 7.f);
        return;
      }
      u0 = bload4(ry, x0 < Wo ? (yrow + (uint32_t)x0) * 4u : OOB);
      u1 = bload4(ry, x0 + 16 < Wo ? (yrow + (uint32_t)(x0 + 16)) * 4u : OOB);
    };
    float4 an0, an1;
    const int KS = (Wo + 31) >> 5;         // K-steps of 32 pixels per row (<= 11: Wo <= 338)
    if (sp < KS) load_a(sp, an0, an1);
#pragma unroll
    for (int k2 = 0; k2 < 6; ++k2) {
      const int kk = sp + 2 * k2;
      if (kk >= KS) break;
      uint32_t ah[4], am[4], al[4];
      split3_pk(an0.x, an0.y, ah[0], am[0], al[0]);
      split3_pk(an0.z, an0.w, ah[1], am[1], al[1]);
      split3_pk(an1.x, an1.y, ah[2], am[2], al[2]);
      split3_pk(an1.z, an1.w, ah[3], am[3], al[3]);
      if (kk + 2 < KS) load_a(kk + 2, an0, an1);
      const bf16x8_t Ah = __builtin_bit_cast(bf16x8_t, u32x4_t{ah[0], ah[1], ah[2], ah[3]});
      const bf16x8_t Am = __builtin_bit_cast(bf16x8_t, u32x4_t{am[0], am[1], am[2], am[3]});
      const bf16x8_t Al = __builtin_bit_cast(bf16x8_t, u32x4_t{al[0], al[1], al[2], al[3]});
      const uint32_t kofs = (uint32_t)kk * 1024u;
      // B of tile i: two transposed reads (pixels 16 t + 4 g + q) x three parts
      auto read_b = [&](int i, u32x4_t (&fb)[3]) {
#pragma unroll
        for (int part = 0; part < 3; ++part) {
          const uint8_t* base = lds + part * plane + tb[i] + kofs;
          if constexpr ((DBG & 4) != 0) {
            fb[part] = u32x4_t{tb[i], kofs, (uint32_t)part, (uint32_t)i};
            continue;
          }
          const uint2 lo = stem_tr16(base), hi = stem_tr16(base + 512);
          fb[part] = u32x4_t{lo.x, lo.y, hi.x, hi.y};
        }
      };
      u32x4_t fb[2][3];
      read_b(0, fb[0]);
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        if (i + 1 < NT) read_b(i + 1, fb[(i + 1) & 1]);
        {
          const bf16x8_t Bh = __builtin_bit_cast(bf16x8_t, fb[i & 1][0]);
          const bf16x8_t Bm = __builtin_bit_cast(bf16x8_t, fb[i & 1][1]);
          const bf16x8_t Bl = __builtin_bit_cast(bf16x8_t, fb[i & 1][2]);
          if constexpr ((DBG & 1) != 0) {
            c1[i][0] += __builtin_bit_cast(float, fb[i & 1][0][0] ^ fb[i & 1][1][1] ^ fb[i & 1][2][2] ^ ah[0] ^ am[1] ^ al[2]);
            continue;
          }
          stem_f32x4 c = c1[i];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Am, Bm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Am, Bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bm, c, 0, 0, 0);
          c1[i] = c;
          c0[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, c0[i], 0, 0, 0);
        }
      }
    }
    if (pipe && tid < P) stage_write(y + 2, vn);
    __syncthreads();
  }

  // ---- the odd-K-step waves' sums through LDS (the ring is free after the last barrier), added
  // by the even ones: (c0 + c1)_even + (c0 + c1)_odd, a fixed order
  float* red = reinterpret_cast<float*>(lds) + mt * StemWgradLds::red_quarter + lane;
  if (sp == 1) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[(i * 4 + e) * 64] = c0[i][e] + c1[i][e];
  }
  __syncthreads();
  if (sp == 1) return;
  // ---- this block's slab: lane (n, g) holds filters 16 mt + 4 g + e, column n of each tile
  float* sl = a.slab + (long)b * 64 * 147;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int T = i, pq = n >> 2, c = n & 3;
    int dY, dX, Qd;
    stem_wquad(T, pq, dY, dX, Qd);
    const int py = Qd < 2 ? 1 : 0, px = (Qd & 1) ? 0 : 1;
    const int ky = 2 * dY + py + 3, kx = 2 * dX + px + 3;
    const bool live = c < 3 && !(T >= 9 && T < 12 && pq == 3) && ky >= 0 && kx >= 0;
    if (live) {
      const int k = c * 49 + ky * 7 + kx;
#pragma unroll
      for (int e = 0; e < 4; ++e) sl[(long)(mt * 16 + 4 * g + e) * 147 + k] = (c0[i][e] + c1[i][e]) + red[(i * 4 + e) * 64];
    }
  }
}

// (which shapes and operands run these kernels: conv_route.hip)
// blocks: one per CU (256), at most one per output row
static int stem_blocks(const ConvShape& s) { return (int)std::min<long>(256, (long)s.N * s.Ho); }

int stem_wgrad_blocks(const ConvShape& s) { return stem_blocks(s); }
int stem_wgrad_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st) {
  const int P = StemWgradLds::pitch(s.Wo);
  const dim3 grid(stem_blocks(s)), block(512);
  const LdsSize z{StemWgradLds::need(P), StemWgradLds::bytes(P), StemWgradLds::cap};
#if MD2_TIMING_VARIANTS
  static const int dbg = tuning_knob("MD2_WSTEM_DBG", 0);   // MD2_TUNING=1; results wrong
  switch (dbg) {
    case 1: return lds_launch<conv_wgrad_stem_s2d_kernel<1>>(grid, block, z, st, a, P);
    case 2: return lds_launch<conv_wgrad_stem_s2d_kernel<2>>(grid, block, z, st, a, P);
    case 4: return lds_launch<conv_wgrad_stem_s2d_kernel<4>>(grid, block, z, st, a, P);
    case 6: return lds_launch<conv_wgrad_stem_s2d_kernel<6>>(grid, block, z, st, a, P);
    case 7: return lds_launch<conv_wgrad_stem_s2d_kernel<7>>(grid, block, z, st, a, P);
    case 15: return lds_launch<conv_wgrad_stem_s2d_kernel<15>>(grid, block, z, st, a, P);
    default: break;
  }
#endif
  return lds_launch<conv_wgrad_stem_s2d_kernel<0>>(grid, block, z, st, a, P);
}

int stem_s2d_launch(const ConvShape& s, const ConvArgs& a, hipStream_t st) {
  const int P = StemLds::pitch(a.Wo);
  const dim3 grid(stem_blocks(s)), block(512);
  const LdsSize z{StemLds::need(P), StemLds::bytes(P), StemLds::cap};
#if MD2_TIMING_VARIANTS
  static const int dbg = tuning_knob("MD2_STEM_DBG", 0);    // MD2_TUNING=1; results wrong but 16
  switch (dbg) {
    case 2: return lds_launch<conv_stem_s2d_kernel<2>>(grid, block, z, st, a);
    case 4: return lds_launch<conv_stem_s2d_kernel<4>>(grid, block, z, st, a);
    case 8: return lds_launch<conv_stem_s2d_kernel<8>>(grid, block, z, st, a);
    case 14: return lds_launch<conv_stem_s2d_kernel<14>>(grid, block, z, st, a);
    case 16: return lds_launch<conv_stem_s2d_kernel<16>>(grid, block, z, st, a);
    default: break;
  }
#endif
  return lds_launch<conv_stem_s2d_kernel<0>>(grid, block, z, st, a);
}
