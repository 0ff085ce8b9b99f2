// ---------------------------------------------------------------------------------------------
// forward / dgrad implicit-GEMM kernel, k-contiguous LDS images (tap-major K only); included by
// conv_px_launch.h after conv_px.inc.  MODE 0 = forward, MODE 1 = dgrad.
//
// Per 16-deep K chunk the LDS holds As[m][k] and Bs[n][k] with k contiguous (rows of 20 floats:
// the 80-byte stride keeps each 8-lane ds_read_b128 phase on distinct 16-byte bank groups).  The
// MFMA v_mfma_f32_32x32x2_f32 step kk of a chunk contracts physical k = {kk, kk+8}: lane (i, h)
// supplies A[i][8h+kk] / B[8h+kk][j], so a lane's eight A (or B) values of the chunk are two
// ds_read_b128 -- one LDS wait per chunk instead of one per MFMA pair.
//   A: packed weights in [K/16][Mpad][16] (conv_pack: layout 1), one float4 = 4 consecutive k.
//   B: wave w gathers channels 4w..4w+3 of the chunk (wave-uniform scalar soffsets) for its
//      BN/64 pixels per lane and writes them as one ds_write_b128 per pixel.
// ---------------------------------------------------------------------------------------------

// LDS row stride (floats) of the k-contiguous images: BK + 4 (20 / 36 floats; both keep the
// ds_read_b128 phases on distinct 16-byte bank groups)
#ifndef PX2_DEPTH
#define PX2_DEPTH 2          // chunks of global-load lookahead (register ring depth)
#endif

// B gather of one chunk for PPT pixels per lane: out[p][q] = B[channel cb + 4w + q][pixel p]
template <int MODE, int KW, int S, int RFL, int PPT>
__device__ __forceinline__ void px2_gather(const ConvArgs& a, bool kv, int tap, int cb, int wq,
                                           const int (&py)[PPT], const int (&px)[PPT],
                                           const bool (&nvalid)[PPT], bool wborder,
                                           const uint32_t (&boff0)[PPT], const uint32_t (&boff1)[PPT],
                                           __amdgpu_buffer_rsrc_t r0, __amdgpu_buffer_rsrc_t r1,
                                           float (&out)[PPT][4]) {
  const int kh = tap / KW, kw = tap - (tap / KW) * KW;
  if (MODE == 0) {
    const bool second = cb >= a.in.c0;             // wave-uniform concat split
    const uint32_t cs = (uint32_t)((second ? cb - a.in.c0 : cb) + 4 * wq);
    const __amdgpu_buffer_rsrc_t r = second ? r1 : r0;
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      int iy = py[p] + kh, ix = px[p] + kw;
      bool ok;
      if (RFL) {
        iy = refl(iy, a.H);
        ix = refl(ix, a.W);
        ok = nvalid[p];
      } else {
        ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      }
      const uint32_t voff = (ok && kv) ? (second ? boff1[p] : boff0[p]) + (uint32_t)(iy * a.W + ix) * 4u : OOB;
#pragma unroll
      for (int q = 0; q < 4; ++q) out[p][q] = bload_s(r, voff, (cs + q) * a.HW4);
    }
  } else {
    const uint32_t cs = (uint32_t)(cb + 4 * wq);
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      if (!RFL) {
        const int ohn = py[p] + a.pad - kh, own = px[p] + a.pad - kw;
        bool ok;
        int oh, ow;
        if (S == 1) {
          oh = ohn;
          ow = own;
          ok = (unsigned)oh < (unsigned)a.Ho && (unsigned)ow < (unsigned)a.Wo;
        } else {
          oh = ohn >> 1;
          ow = own >> 1;
          ok = ohn >= 0 && own >= 0 && !(ohn & 1) && !(own & 1) && oh < a.Ho && ow < a.Wo;
        }
        const uint32_t voff = (ok && kv) ? boff0[p] + (uint32_t)(oh * a.Wo + ow) * 4u : OOB;
#pragma unroll
        for (int q = 0; q < 4; ++q) out[p][q] = bload_s(r0, voff, (cs + q) * a.HoWo4);
      } else if (!wborder) {
        const int oh = py[p] + 1 - kh, ow = px[p] + 1 - kw;
        const bool ok = kv && nvalid[p] && (unsigned)oh < (unsigned)a.Ho && (unsigned)ow < (unsigned)a.Wo;
        const uint32_t voff = ok ? boff0[p] + (uint32_t)(oh * a.Wo + ow) * 4u : OOB;
#pragma unroll
        for (int q = 0; q < 4; ++q) out[p][q] = bload_s(r0, voff, (cs + q) * a.HoWo4);
      } else {
        // pad_reflect adjoint (see px_gather_tap)
        const int qy1 = py[p] == 1 ? 0 : (py[p] == a.H - 2 ? a.H + 1 : -1000);
        const int qx1 = px[p] == 1 ? 0 : (px[p] == a.W - 2 ? a.W + 1 : -1000);
        uint32_t voff[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int oh = ((u & 1) ? qy1 : py[p] + 1) - kh, ow = ((u & 2) ? qx1 : px[p] + 1) - kw;
          const bool ok = kv && nvalid[p] && (unsigned)oh < (unsigned)a.Ho && (unsigned)ow < (unsigned)a.Wo;
          voff[u] = ok ? boff0[p] + (uint32_t)(oh * a.Wo + ow) * 4u : OOB;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t so = (cs + q) * a.HoWo4;
          out[p][q] = (bload_s(r0, voff[0], so) + bload_s(r0, voff[1], so)) +
                      (bload_s(r0, voff[2], so) + bload_s(r0, voff[3], so));
        }
      }
    }
  }
}

// A-tile thread map: thread idx carries float4 k4 = (idx >> 4) & 3 of row m = px2_am(idx), so the 16
// lanes of one ds_write_b128 phase store 16 different rows of the same k4 -- at the 80-byte row
// stride those are 16 distinct 16-byte bank groups (the previous map, 4 rows x 4 k4 per phase,
// wrapped row 3 onto row 0's banks: 2-way conflicts).  A wave still loads 16 whole packed rows
// (1 KB contiguous), so the global reads stay fully coalesced.
__device__ __forceinline__ int px2_am(int idx) { return (idx & 15) | ((idx >> 6) << 4); }

template <int MODE, int BM, int BN, int WM, int WN, int KH, int KW, int S, int RFL, int BK = 16>
__global__ __launch_bounds__(256) void conv_px2_kernel(ConvArgs a) {
  static_assert(BK == 16 || BK == 32, "chunk depth");
  constexpr int PX2_LD = BK + 4;
  constexpr int NH = BK / 16;                 // 16-deep halves per chunk (packed A rows, gathers)
  constexpr bool PHASE = MODE == 1 && S == 2;
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int A_F4H = BM * 4 / 256;         // float4 of A per thread per 16-deep half
  constexpr int A_F4 = A_F4H * NH;
  constexpr int PPT = BN / 64;                // B pixels per lane
  static_assert(A_F4H >= 1 && PPT >= 1 && TM >= 1 && TN >= 1 && BM * 4 % 256 == 0 && BN % 64 == 0, "tile");
  __shared__ __attribute__((aligned(16))) float As[2][BM][PX2_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][BN][PX2_LD];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave id (uniform)
  const int wm = wq / WN, wn = wq % WN;
  // XCD-aware tile order (a.xcd): workgroups are dealt round-robin to the 8 XCDs by linear id,
  // so linear id i runs tile (i % 8) * q + i / 8: each XCD's L2 sees a contiguous tile range
  // (shared input halos, one weight slice per split)
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
  // stride-2 dgrad: the parity class of this block (merged launch: z = class * ph_S + split,
  // taps of class c at ph_taps[4c..4c+ntaps)), or the launch's single class
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

  // ---- B pixels of this lane: n0 + lane + 64 p
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

  // chunk state: k0 = ti * C + cb; tap = ti (or the parity class's ti-th tap); arow = packed row
  const int Ck = MODE == 0 ? a.Cin : a.Cout;
  int ti = kbeg / Ck;
  int cb = kbeg - ti * Ck;
  int tap = PHASE ? (nk > 0 ? a.ph_taps[ph_tb + min(ti, ph_tl)] : 0) : ti;
  int arow = tap * Ck + cb;

  // D-deep register ring: the loads of chunk t+D are issued while chunk t computes, so a chunk's
  // global loads have D chunks of MFMA work to land before their LDS store (the kernel is
  // load-latency bound at the ~4 waves/SIMD these grids give)
  constexpr int D = PX2_DEPTH;
  float4 areg[D][A_F4];
  float breg[D][NH][PPT][4];

#define MD2_PX2_ADVANCE()                                                                         \
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
  // chunks past nk (ring padding / lookahead past the end) load through OOB offsets: zeros
#define MD2_PX2_LOAD(SET)                                                                         \
  {                                                                                               \
    const bool kv = kc < nk;                                                                      \
    _Pragma("unroll") for (int j = 0; j < A_F4; ++j) {                                            \
      const int idx = tid + 256 * (j % A_F4H), m = px2_am(idx), k4 = (idx >> 4) & 3, hh = j / A_F4H;         \
      areg[SET][j] = bload4(rA, kv ? (uint32_t)((((arow >> 4) + hh) * a.g.Mpad + m0 + m) * 16 + k4 * 4) * 4u \
                                   : OOB);                                                        \
    }                                                                                             \
    _Pragma("unroll") for (int hh = 0; hh < NH; ++hh)                                             \
      px2_gather<MODE, KW, S, RFL, PPT>(a, kv, tap, cb + 16 * hh, wq, py, px, nvalid, wborder,    \
                                        boff0, boff1, r0, r1, breg[SET][hh]);                     \
  }
#define MD2_PX2_STORE(BUF, SET)                                                                   \
  {                                                                                               \
    _Pragma("unroll") for (int j = 0; j < A_F4; ++j) {                                            \
      const int idx = tid + 256 * (j % A_F4H), m = px2_am(idx), k4 = (idx >> 4) & 3, hh = j / A_F4H;         \
      *reinterpret_cast<float4*>(&As[BUF][m][16 * hh + k4 * 4]) = areg[SET][j];                   \
    }                                                                                             \
    _Pragma("unroll") for (int hh = 0; hh < NH; ++hh)                                             \
    _Pragma("unroll") for (int p = 0; p < PPT; ++p)                                               \
      *reinterpret_cast<float4*>(&Bs[BUF][lane + 64 * p][16 * hh + wq * 4]) =                     \
          make_float4(breg[SET][hh][p][0], breg[SET][hh][p][1], breg[SET][hh][p][2],              \
                      breg[SET][hh][p][3]);                                                       \
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int fi = lane & 31, fh = lane >> 5;
  // prologue: chunks 0..D-1 into sets 0..D-1, chunk 0 to LDS 0.  The ring runs a whole number of
  // D-chunk rounds with unconditional prefetch: identical pending-load order on every path, so the
  // compiler's vmcnt before each LDS store waits for exactly the older set.
  int kc = 0;
  MD2_PX2_LOAD(0);
#pragma unroll
  for (int u = 1; u < D; ++u) {
    MD2_PX2_ADVANCE();
    MD2_PX2_LOAD(u);
  }
  MD2_PX2_STORE(0, 0);
  __syncthreads();
  const int nkp = (nk + D - 1) / D * D;
  for (int t0 = 0; t0 < nkp; t0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int cur = (t0 + u) & 1;
      MD2_PX2_ADVANCE();          // set u held chunk t0+u (already in LDS): refill with t0+u+D
      MD2_PX2_LOAD(u);
      __builtin_amdgcn_sched_barrier(0);   // keep the refill ahead of this chunk's LDS store
      // lane half fh supplies k = fh*BK/2 + kk of the chunk: BK/8 float4 per fragment
      constexpr int NF = BK / 8;
      float4 fa[TM][NF], fb[TN][NF];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const float* src = &As[cur][wm * TM * 32 + i * 32 + fi][fh * (BK / 2)];
#pragma unroll
        for (int f = 0; f < NF; ++f) fa[i][f] = *reinterpret_cast<const float4*>(src + 4 * f);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const float* src = &Bs[cur][wn * TN * 32 + j * 32 + fi][fh * (BK / 2)];
#pragma unroll
        for (int f = 0; f < NF; ++f) fb[j][f] = *reinterpret_cast<const float4*>(src + 4 * f);
      }
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const float av = (&fa[i][kk >> 2].x)[kk & 3];
            const float bv = (&fb[j][kk >> 2].x)[kk & 3];
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i][j], 0, 0, 0);
          }
      __builtin_amdgcn_sched_barrier(0);
      MD2_PX2_STORE(cur ^ 1, (u + 1) % D);
      __syncthreads();
    }
  }
#undef MD2_PX2_ADVANCE
#undef MD2_PX2_LOAD
#undef MD2_PX2_STORE

  // ---- epilogue (same accumulator layout as conv_px_kernel)
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
          if (m < a.g.M) sl[(long)m * a.g.N + nn] = acc[i][j][r];
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
          if (m < a.g.M) store_out(a.out, m, img, pix, plane, acc[i][j][r]);
        }
    }
  }
}
