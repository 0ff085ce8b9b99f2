// ---------------------------------------------------------------------------------------------
// forward / dgrad implicit-GEMM kernel on the bf16 MFMA with EXACT fp32 products (bf16x9);
// included by conv_px_launch.h after conv_px2.inc.  MODE 0 = forward, MODE 1 = dgrad; tap-major K.
//
// Every fp32 operand x is split exactly into three bf16 terms, x = hi + mid + lo: hi = x rounded
// to bf16, mid = the exact remainder x - hi rounded to bf16, lo = the rest (<= 8 significant
// bits, so it is itself a bf16; the weights use the equivalent truncating split3).  The product of two split operands is
// the sum of the nine bf16 x bf16 partial products, each exact in the MFMA's fp32 arithmetic, so
// the contraction computes the same fp32-rounded sums of exact products as the fp32 MFMA
// (v_mfma_f32_32x32x2_f32) -- at the bf16 rate: nine v_mfma_f32_32x32x16_bf16 (9 x 32 cycles)
// cover a 16-deep K chunk that takes eight f32 MFMAs (8 x 64 cycles).  hi x hi accumulates in its
// own register tile and the eight smaller cross terms (2^-8 and below) in a second one, added in
// the epilogue: the cross terms' roundings stay 2^-8 below the main sum's.
//
//   A (weights): packed pre-split at repack time, layout 2 = [K/16][3 parts][Mpad][16] bf16.  A
//      lane (i, h) of the MFMA needs A[row i][k = 8h .. 8h+7] -- one 16-byte load per part,
//      straight from L1/L2 into its fragment registers (no LDS: each A row is read by the WN = 2
//      waves of its row half).
//   B (activations / dY): gathered as in conv_px2 (wave w loads channels 4w..4w+3 of the chunk
//      for its lane's pixel), split in registers two channels at a time (v_cvt_pk_bf16_f32 rounds
//      a pair to packed bf16, v_pk_add_f32 forms both remainders: 9 VALU per pair, already in the
//      packed LDS format), and stored as three k-contiguous bf16 images Bs[part][n][k] (48-byte
//      rows: the 16-lane phases of a ds_read_b128 hit distinct banks).
// ---------------------------------------------------------------------------------------------

// BK = 16 or 32: K depth per chunk (32: two 16-deep halves per barrier, the gather address maths
// shared by 8 channels of one tap; needs the reduction channels % 32 == 0)
// NT = 6 (default): the six split products down to 2^-16 relative (hi.hi, hi.mid, mid.hi, hi.lo,
// lo.hi, mid.mid); the three dropped (mid.lo, lo.mid, lo.lo) are <= 2^-24, 2^-24, 2^-32 of |a||b|,
// i.e. at most ~2x the rounding of one fp32 product -- the fp32 accuracy class, with a third less
// MFMA work (and power) than NT = 9, where every product is exact (MD2_PX3_TERMS=9)
template <int MODE, int BM, int BN, int WM, int WN, int KH, int KW, int S, int RFL, int BK = 16, int NT = 9>
__global__ __launch_bounds__(256) void conv_px3_kernel(ConvArgs a) {
  static_assert(NT == 9 || NT == 6, "split products");
  static_assert(BK == 16 || BK == 32, "chunk depth");
  constexpr int NH = BK / 16;                  // 16-deep halves per chunk
  constexpr int LDB = BK + 8;                  // bf16 row stride of the B images (48 / 80 bytes)
  constexpr bool PHASE = MODE == 1 && S == 2;
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int PPT = BN / 64;                 // B pixels per lane
  static_assert(PPT >= 1 && TM >= 1 && TN >= 1 && BN % 64 == 0 && WM * WN == 4, "tile");
  __shared__ __attribute__((aligned(16))) uint16_t Bs[2][3][BN][LDB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wq / WN, wn = wq % WN;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (a.xcd) {
    const int gx = gridDim.x, gy = gridDim.y;
    const int T = gx * gy * gridDim.z, q = T >> 3;
    int id = bx + gx * (by + gy * bz);
    if (id < 8 * q) id = (id & 7) * q + (id >> 3);
    bx = id % gx;
    by = (id / gx) % gy;
    bz = id / (gx * gy);
  }
  const int bslab = bz;
  int ph_y0 = a.ph_y0, ph_x0 = a.ph_x0, ph_tb = 0, ph_tl = 15, Kc = a.g.K;
  if (PHASE && a.ph_S > 0) {
    const int cls = bz / a.ph_S;
    bz -= cls * a.ph_S;
    ph_y0 = a.ph_y0c[cls];
    ph_x0 = a.ph_x0c[cls];
    ph_tb = 4 * cls;
    ph_tl = 3;
    Kc = a.ph_ntc[cls] * a.Cout;
  }
  const int m0 = by * BM;
  const int n0 = bx * BN;
  const int kbeg = bz * a.g.kper;
  const int kend = min(Kc, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;

  int py[PPT], px[PPT];
  bool nvalid[PPT];
  uint32_t boff0[PPT], boff1[PPT];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int n = n0 + lane + 64 * p;
    nvalid[p] = n < (int)a.g.N;
    py[p] = px[p] = -0x10000;
    boff0[p] = boff1[p] = 0;
    if (nvalid[p]) {
      const int img = (int)fdiv((uint32_t)n, a.fd_pix);
      const int pix = n - img * (int)a.fd_pix.d;
      const int oy = (int)fdiv((uint32_t)pix, a.fd_row);
      const int ox = pix - oy * (int)a.fd_row.d;
      if (MODE == 0) {
        py[p] = oy * S - a.pad;
        px[p] = ox * S - a.pad;
        const int q = (int)fdiv((uint32_t)img, a.fd_bdiv);
        boff0[p] = (uint32_t)((long)(img - q * (int)a.fd_bdiv.d) * a.in.bs0 + (long)q * a.in.bhi) * 4u;
        boff1[p] = (uint32_t)((long)img * a.in.bs1) * 4u;
      } else {
        py[p] = PHASE ? ph_y0 + 2 * oy : oy;
        px[p] = PHASE ? ph_x0 + 2 * ox : ox;
        boff0[p] = (uint32_t)((long)img * a.Cout * a.HoWo) * 4u;
      }
    }
  }
  bool wborder = false;
  if (MODE == 1 && RFL) {
    bool bd = false;
#pragma unroll
    for (int p = 0; p < PPT; ++p)
      bd |= nvalid[p] && (py[p] == 1 || py[p] == a.H - 2 || px[p] == 1 || px[p] == a.W - 2);
    wborder = __ballot(bd) != 0;
  }
  const __amdgpu_buffer_rsrc_t rA = make_rsrc(a.A, a.A_bytes);
  const __amdgpu_buffer_rsrc_t r0 = make_rsrc(MODE == 0 ? (const void*)a.in.p0 : (const void*)a.dy, a.b0_bytes);
  const __amdgpu_buffer_rsrc_t r1 = make_rsrc(a.in.p1 ? a.in.p1 : a.in.p0, a.b1_bytes);

  const int Ck = MODE == 0 ? a.Cin : a.Cout;
  int ti = kbeg / Ck;
  int cb = kbeg - ti * Ck;
  int tap = PHASE ? (nk > 0 ? a.ph_taps[ph_tb + min(ti, ph_tl)] : 0) : ti;
  int arow = tap * Ck + cb;

  const int fi = lane & 31, fh = lane >> 5;
  // this lane's A rows (one per M sub-tile) and the byte offset of its 16 bytes inside a
  // [part][Mpad][16] bf16 chunk block
  uint32_t aoff[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) aoff[i] = (uint32_t)(((m0 + wm * TM * 32 + i * 32 + fi) * 16 + 8 * fh) * 2);
  const uint32_t apart = (uint32_t)a.g.Mpad * 32u;     // bytes per part of one K chunk
  const uint32_t achunk = 3u * apart;                  // bytes per K chunk

  constexpr int D = 2;
  u32x4_t areg[D][TM][NH][3];
  float breg[D][NH][PPT][4];

#define MD2_PX3_ADVANCE()                                                                         \
  {                                                                                               \
    ++kc;                                                                                         \
    cb += BK;                                                                                     \
    if (cb == Ck) {                                                                               \
      cb = 0;                                                                                     \
      ++ti;                                                                                       \
      tap = PHASE ? a.ph_taps[ph_tb + min(ti, ph_tl)] : ti;                                       \
    }                                                                                             \
    arow = tap * Ck + cb;                                                                         \
  }
#define MD2_PX3_LOAD(SET)                                                                         \
  {                                                                                               \
    const bool kv = kc < nk;                                                                      \
    _Pragma("unroll") for (int hh = 0; hh < NH; ++hh) {                                           \
      const uint32_t cbase = (uint32_t)((arow >> 4) + hh) * achunk;                               \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                              \
      _Pragma("unroll") for (int q = 0; q < 3; ++q)                                               \
        areg[SET][i][hh][q] = bload16(rA, kv ? cbase + (uint32_t)q * apart + aoff[i] : OOB);      \
      px2_gather<MODE, KW, S, RFL, PPT>(a, kv, tap, cb + 16 * hh, wq, py, px, nvalid, wborder,    \
                                        boff0, boff1, r0, r1, breg[SET][hh]);                     \
    }                                                                                             \
  }
#define MD2_PX3_STORE(BUF, SET)                                                                   \
  {                                                                                               \
    _Pragma("unroll") for (int hh = 0; hh < NH; ++hh)                                             \
    _Pragma("unroll") for (int p = 0; p < PPT; ++p) {                                             \
      uint32_t h0, m0, l0, h1, m1, l1;                                                            \
      split3_pk(breg[SET][hh][p][0], breg[SET][hh][p][1], h0, m0, l0);                            \
      split3_pk(breg[SET][hh][p][2], breg[SET][hh][p][3], h1, m1, l1);                            \
      const int ko = 16 * hh + wq * 4;                                                            \
      *reinterpret_cast<uint2*>(&Bs[BUF][0][lane + 64 * p][ko]) = make_uint2(h0, h1);             \
      *reinterpret_cast<uint2*>(&Bs[BUF][1][lane + 64 * p][ko]) = make_uint2(m0, m1);             \
      *reinterpret_cast<uint2*>(&Bs[BUF][2][lane + 64 * p][ko]) = make_uint2(l0, l1);             \
    }                                                                                             \
  }

  f32x16 acc0[TM][TN], acc1[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[i][j][r] = acc1[i][j][r] = 0.f;

  int kc = 0;
  MD2_PX3_LOAD(0);
#pragma unroll
  for (int u = 1; u < D; ++u) {
    MD2_PX3_ADVANCE();
    MD2_PX3_LOAD(u);
  }
  MD2_PX3_STORE(0, 0);
  __syncthreads();
  const int nkp = (nk + D - 1) / D * D;
  for (int t0 = 0; t0 < nkp; t0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int cur = (t0 + u) & 1;
      // chunk t0+u: MFMAs straight from ring set u, which is refilled (chunk t0+u+D) after them
      // -- no register copy of the A fragments; the other waves of the SIMD cover the shorter
      // lookahead
#define fa areg[u]
#pragma unroll
      for (int hh = 0; hh < NH; ++hh) {
      u32x4_t fb[TN][3];
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          fb[j][q] = *reinterpret_cast<const u32x4_t*>(&Bs[cur][q][wn * TN * 32 + j * 32 + fi][16 * hh + 8 * fh]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const bf16x8_t ah = __builtin_bit_cast(bf16x8_t, fa[i][hh][0]);
          const bf16x8_t am = __builtin_bit_cast(bf16x8_t, fa[i][hh][1]);
          const bf16x8_t al = __builtin_bit_cast(bf16x8_t, fa[i][hh][2]);
          const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, fb[j][0]);
          const bf16x8_t bm = __builtin_bit_cast(bf16x8_t, fb[j][1]);
          const bf16x8_t bl = __builtin_bit_cast(bf16x8_t, fb[j][2]);
          // the cross terms smallest first, then the main product in its own tile
          f32x16 c = acc1[i][j];
          if constexpr (NT == 9) {
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bm, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bl, c, 0, 0, 0);
          }
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
          acc1[i][j] = c;
          acc0[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc0[i][j], 0, 0, 0);
        }
      }
#undef fa
      __builtin_amdgcn_sched_barrier(0);
      MD2_PX3_ADVANCE();
      MD2_PX3_LOAD(u);
      MD2_PX3_STORE(cur ^ 1, (u + 1) % D);
      __syncthreads();
    }
  }
#undef MD2_PX3_ADVANCE
#undef MD2_PX3_LOAD
#undef MD2_PX3_STORE

  // ---- epilogue (accumulator layout of conv_px2)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long nn = (long)n0 + wn * TN * 32 + j * 32 + (lane & 31);
    if (nn >= a.g.N) continue;
    if (a.slab) {
      float* sl = a.slab + (long)bslab * a.g.M * a.g.N;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (m < a.g.M) sl[(long)m * a.g.N + nn] = acc0[i][j][r] + acc1[i][j][r];
        }
    } else {
      int img;
      long pix, plane;
      out_pixel(a, PHASE, ph_y0, ph_x0, nn, img, pix, plane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (m < a.g.M) store_out(a.out, m, img, pix, plane, acc0[i][j][r] + acc1[i][j][r]);
        }
    }
  }
}
