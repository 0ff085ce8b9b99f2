// ---------------------------------------------------------------------------------------------
// forward / dgrad implicit-GEMM kernel (B operand lanes along pixels); included by conv_px_launch.h.
// MODE 0 = forward (im2col of x), MODE 1 = dgrad (gather of dY).
//
// Operands come in through raw buffer loads with 32-bit byte offsets; a tap outside the image
// is given an out-of-range offset so the load itself returns 0 (zero padding without exec-mask
// branches).  TAP = 1 (tap-major K, see conv_tap_major): the filter tap is constant over a K
// chunk, so each thread computes its spatial offset ONCE per chunk and the BK channel steps are
// scalar soffsets -- no VALU per gathered element.  TAP = 0 (channel-major, stem and 1-channel
// heads): (c, kh, kw) decoded on SALU per element, one VALU add + compare + select per gather.  Staging registers are plain unrolled arrays (no
// lambdas: a captured staging array was demoted to scratch and serialised every K step).
// ---------------------------------------------------------------------------------------------

#define MD2_PX_LOAD_A(K0)                                                                         \
  _Pragma("unroll") for (int j = 0; j < A_F4; ++j) {                                              \
    const int idx = tid + 256 * j;                                                                \
    if (A_TOT % 256 == 0 || idx < A_TOT) {                                                        \
      const int row = idx / (BM / 4), c4 = idx % (BM / 4);                                        \
      areg[j] = bload4(rA, (uint32_t)(((K0) + row) * a.g.Mpad + m0 + c4 * 4) * 4u);              \
    }                                                                                             \
  }

#define MD2_PX_STORE(BUF)                                                                         \
  _Pragma("unroll") for (int j = 0; j < A_F4; ++j) {                                              \
    const int idx = tid + 256 * j;                                                                \
    if (A_TOT % 256 == 0 || idx < A_TOT) {                                                        \
      const int row = idx / (BM / 4), c4 = idx % (BM / 4);                                        \
      *reinterpret_cast<float4*>(&As[BUF][row][c4 * 4]) = areg[j];                                \
    }                                                                                             \
  }                                                                                               \
  _Pragma("unroll") for (int j = 0; j < B_EL; ++j) Bs[BUF][brow + j * B_RS][bn] = breg[j];

template <int MODE, int KH, int KW, int S, int RFL>
__device__ __forceinline__ float px_gather(const ConvArgs& a, int k, int kend, int py, int px,
                                           bool nvalid, uint32_t boff0, uint32_t boff1,
                                           __amdgpu_buffer_rsrc_t r0, __amdgpu_buffer_rsrc_t r1) {
  constexpr int KK = KH * KW;
  if (k >= kend) return 0.f;                      // wave-uniform
  const int c = k / KK;
  const int r = k - c * KK;
  const int kh = r / KW, kw = r - (r / KW) * KW;
  if (MODE == 0) {
    int iy = py + kh, ix = px + kw;
    bool ok;
    if (RFL) {
      iy = refl(iy, a.H);
      ix = refl(ix, a.W);
      ok = nvalid;
    } else {
      ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
    }
    const bool second = c >= a.in.c0;             // wave-uniform concat split
    const uint32_t cb = (uint32_t)((second ? c - a.in.c0 : c) * a.HW) * 4u;
    const uint32_t off = ok ? (second ? boff1 : boff0) + cb + (uint32_t)(iy * a.W + ix) * 4u : OOB;
    return bload(second ? r1 : r0, off);
  } else {
    const uint32_t cb = boff0 + (uint32_t)(c * a.HoWo) * 4u;
    if (!RFL) {
      const int ohn = py + a.pad - kh, own = px + a.pad - kw;
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
      return bload(r0, ok ? cb + (uint32_t)(oh * a.Wo + ow) * 4u : OOB);
    } else {
      if (!nvalid) return 0.f;
      // pad_reflect adjoint: padded rows q with reflect(q-1) == iy are iy+1, 0 (iy == 1) and
      // H+1 (iy == H-2); same for columns (stride 1, pad 1)
      if (py != 1 && py != a.H - 2 && px != 1 && px != a.W - 2) {
        const int oh = py + 1 - kh, ow = px + 1 - kw;
        const bool ok = (unsigned)oh < (unsigned)a.Ho && (unsigned)ow < (unsigned)a.Wo;
        return bload(r0, ok ? cb + (uint32_t)(oh * a.Wo + ow) * 4u : OOB);
      }
      const int qy[3] = {py + 1, (py == 1) ? 0 : -1000, (py == a.H - 2) ? a.H + 1 : -1000};
      const int qx[3] = {px + 1, (px == 1) ? 0 : -1000, (px == a.W - 2) ? a.W + 1 : -1000};
      float v = 0.f;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int oh = qy[u] - kh;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          const int ow = qx[w] - kw;
          const bool ok = (unsigned)oh < (unsigned)a.Ho && (unsigned)ow < (unsigned)a.Wo;
          v += bload(r0, ok ? cb + (uint32_t)(oh * a.Wo + ow) * 4u : OOB);
        }
      }
      return v;
    }
  }
}

// tap-major chunk gather: channels c = cb + brow + j*B_RS (cb wave-uniform, chunk-aligned, on one
// side of the concat split), tap (kh, kw) wave-uniform; one voffset per thread and chunk.
template <int MODE, int KW, int S, int RFL, int B_EL, int B_RS>
__device__ __forceinline__ void px_gather_tap(const ConvArgs& a, int tap, int cb, int brow, int py,
                                              int px, bool nvalid, bool wborder, uint32_t boff0,
                                              uint32_t boff1, __amdgpu_buffer_rsrc_t r0,
                                              __amdgpu_buffer_rsrc_t r1, float (&breg)[B_EL]) {
  const int kh = tap / KW, kw = tap - (tap / KW) * KW;
  if (MODE == 0) {
    int iy = py + kh, ix = px + kw;
    bool ok;
    if (RFL) {
      iy = refl(iy, a.H);
      ix = refl(ix, a.W);
      ok = nvalid;
    } else {
      ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
    }
    const bool second = cb >= a.in.c0;             // wave-uniform concat split
    const uint32_t voff = ok ? (second ? boff1 : boff0) + (uint32_t)(iy * a.W + ix) * 4u : OOB;
    const uint32_t cs = (uint32_t)((second ? cb - a.in.c0 : cb) + brow);
    const __amdgpu_buffer_rsrc_t r = second ? r1 : r0;
#pragma unroll
    for (int j = 0; j < B_EL; ++j) breg[j] = bload_s(r, voff, (cs + j * B_RS) * a.HW4);
  } else {
    const uint32_t cs = (uint32_t)(cb + brow);
    if (!RFL) {
      const int ohn = py + a.pad - kh, own = px + a.pad - kw;
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
      const uint32_t voff = ok ? boff0 + (uint32_t)(oh * a.Wo + ow) * 4u : OOB;
#pragma unroll
      for (int j = 0; j < B_EL; ++j) breg[j] = bload_s(r0, voff, (cs + j * B_RS) * a.HoWo4);
    } else if (!wborder) {
      // no lane of this wave sits on a reflected row/column: one source tap per output
      const int oh = py + 1 - kh, ow = px + 1 - kw;
      const bool ok = nvalid && (unsigned)oh < (unsigned)a.Ho && (unsigned)ow < (unsigned)a.Wo;
      const uint32_t voff = ok ? boff0 + (uint32_t)(oh * a.Wo + ow) * 4u : OOB;
#pragma unroll
      for (int j = 0; j < B_EL; ++j) breg[j] = bload_s(r0, voff, (cs + j * B_RS) * a.HoWo4);
    } else {
      // pad_reflect adjoint: padded rows q with reflect(q-1) == iy are iy+1 and one of 0 (iy ==
      // 1) / H+1 (iy == H-2) (H, W != 3, checked on the host); same for columns
      const int qy1 = py == 1 ? 0 : (py == a.H - 2 ? a.H + 1 : -1000);
      const int qx1 = px == 1 ? 0 : (px == a.W - 2 ? a.W + 1 : -1000);
      uint32_t voff[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int oh = ((u & 1) ? qy1 : py + 1) - kh, ow = ((u & 2) ? qx1 : px + 1) - kw;
        const bool ok = nvalid && (unsigned)oh < (unsigned)a.Ho && (unsigned)ow < (unsigned)a.Wo;
        voff[u] = ok ? boff0 + (uint32_t)(oh * a.Wo + ow) * 4u : OOB;
      }
#pragma unroll
      for (int j = 0; j < B_EL; ++j) {
        const uint32_t so = (cs + j * B_RS) * a.HoWo4;
        breg[j] = (bload_s(r0, voff[0], so) + bload_s(r0, voff[1], so)) +
                  (bload_s(r0, voff[2], so) + bload_s(r0, voff[3], so));
      }
    }
  }
}

template <int MODE, int TAP, int BM, int BN, int BK, int WM, int WN, int KH, int KW, int S, int RFL>
__global__ __launch_bounds__(256) void conv_px_kernel(ConvArgs a) {
  // tap-major stride-2 dgrad runs per output-parity class (ConvArgs::ph_*)
  constexpr bool PHASE = MODE == 1 && S == 2 && TAP;
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int A_TOT = BK * BM / 4;
  constexpr int A_F4 = (A_TOT + 255) / 256;
  constexpr int B_RS = 256 / BN;
  constexpr int B_EL = BK / B_RS;
  static_assert(A_F4 >= 1 && B_EL >= 1 && TM >= 1 && TN >= 1, "tile");
  __shared__ __attribute__((aligned(16))) float As[2][BK][BM];
  __shared__ float Bs[2][BK][BN];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int m0 = blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;
  const int kbeg = blockIdx.z * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;

  // ---- per-thread pixel of the B operand
  const int bn = tid % BN;
  const int brow = __builtin_amdgcn_readfirstlane(tid / BN);
  const int n = n0 + bn;
  const bool nvalid = n < (int)a.g.N;
  int py = -0x10000, px = -0x10000;     // invalid pixel: every tap out of range
  uint32_t boff0 = 0, boff1 = 0;
  if (nvalid) {
    const int img = (int)fdiv((uint32_t)n, a.fd_pix);
    const int pix = n - img * (int)a.fd_pix.d;
    const int oy = (int)fdiv((uint32_t)pix, a.fd_row);
    const int ox = pix - oy * (int)a.fd_row.d;
    if (MODE == 0) {
      py = oy * S - a.pad;
      px = ox * S - a.pad;
      const int q = (int)fdiv((uint32_t)img, a.fd_bdiv);
      boff0 = (uint32_t)((long)(img - q * (int)a.fd_bdiv.d) * a.in.bs0 + (long)q * a.in.bhi) * 4u;
      boff1 = (uint32_t)((long)img * a.in.bs1) * 4u;
    } else {
      py = PHASE ? a.ph_y0 + 2 * oy : oy;
      px = PHASE ? a.ph_x0 + 2 * ox : ox;
      boff0 = (uint32_t)((long)img * a.Cout * a.HoWo) * 4u;
    }
  }
  const __amdgpu_buffer_rsrc_t rA = make_rsrc(a.A, a.A_bytes);
  const __amdgpu_buffer_rsrc_t r0 = make_rsrc(MODE == 0 ? (const void*)a.in.p0 : (const void*)a.dy, a.b0_bytes);
  const __amdgpu_buffer_rsrc_t r1 = make_rsrc(a.in.p1 ? a.in.p1 : a.in.p0, a.b1_bytes);

  float4 areg[A_F4];
  float breg[B_EL];
  // tap-major chunk state (wave-uniform): chunk k0 = ti * C + cb, tap = ti (or the class's
  // ti-th tap); arow = packed A row of the chunk
  const int Ck = MODE == 0 ? a.Cin : a.Cout;
  int ti = TAP ? kbeg / Ck : 0;
  int cb = TAP ? kbeg - ti * Ck : 0;
  int tap = PHASE ? (nk > 0 ? a.ph_taps[ti] : 0) : ti;
  int arow = TAP ? tap * Ck + cb : kbeg;
  bool wborder = false;
  if (TAP && MODE == 1 && RFL)
    wborder = __ballot(nvalid && (py == 1 || py == a.H - 2 || px == 1 || px == a.W - 2)) != 0;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  MD2_PX_LOAD_A(arow);
  if (TAP) {
    px_gather_tap<MODE, KW, S, RFL, B_EL, B_RS>(a, tap, cb, brow, py, px, nvalid, wborder, boff0,
                                                boff1, r0, r1, breg);
  } else {
#pragma unroll
    for (int j = 0; j < B_EL; ++j)
      breg[j] = px_gather<MODE, KH, KW, S, RFL>(a, kbeg + brow + j * B_RS, kend, py, px, nvalid, boff0, boff1, r0, r1);
  }
  MD2_PX_STORE(0);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    const int kn = kbeg + (t + 1) * BK;
    if (t + 1 < nk) {
      if (TAP) {
        cb += BK;
        if (cb == Ck) {
          cb = 0;
          ++ti;
          tap = PHASE ? a.ph_taps[ti] : ti;
        }
        arow = tap * Ck + cb;
      } else {
        arow = kn;
      }
      MD2_PX_LOAD_A(arow);
      if (TAP) {
        px_gather_tap<MODE, KW, S, RFL, B_EL, B_RS>(a, tap, cb, brow, py, px, nvalid, wborder,
                                                    boff0, boff1, r0, r1, breg);
      } else {
#pragma unroll
        for (int j = 0; j < B_EL; ++j)
          breg[j] = px_gather<MODE, KH, KW, S, RFL>(a, kn + brow + j * B_RS, kend, py, px, nvalid, boff0, boff1, r0, r1);
      }
    }
#ifdef MD2_SETPRIO
    __builtin_amdgcn_s_setprio(1);
#endif
    mma_chunk<TM, TN, BK>(&As[cur][0][0], BM, &Bs[cur][0][0], BN, wm * TM * 32, wn * TN * 32, lane, acc);
#ifdef MD2_SETPRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    if (t + 1 < nk) {
      MD2_PX_STORE(cur ^ 1);
    }
    __syncthreads();
  }

  // ---- epilogue
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long nn = (long)n0 + wn * TN * 32 + j * 32 + (lane & 31);
    if (nn >= a.g.N) continue;
    if (a.slab) {
      float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
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
      out_pixel(a, PHASE, nn, img, pix, plane);
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

#undef MD2_PX_LOAD_A
#undef MD2_PX_STORE

