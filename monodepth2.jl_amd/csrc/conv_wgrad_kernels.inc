// The fp32 wgrad kernels and the one-launch split-K finalise; included by conv_wgrad.hip.
// ---------------------------------------------------------------------------------------------
// wgrad kernel: lanes along the pixel (K) axis for both operands, transposed into LDS
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int BK, int WM, int WN, int KH, int KW, int S, int RFL>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(ConvArgs a) {
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int KK = KH * KW;
  constexpr int RP = 256 / BK;          // rows per pass
  constexpr int A_EL = BM / RP, B_EL = BN / RP;
  constexpr int LDA = BM + 1, LDB = BN + 1;
  static_assert(A_EL >= 1 && B_EL >= 1, "tile");
  __shared__ float As[2][BK][LDA];
  __shared__ float Bs[2][BK][LDB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int m0 = blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;
  const long kbeg = (long)blockIdx.z * a.g.kper;
  const long Ktot = a.g.K;
  const long kend = min(Ktot, kbeg + (long)a.g.kper);
  const int nk = (int)((kend - kbeg + BK - 1) / BK);
  const int kl = tid % BK;
  const int rg = tid / BK;

  // per-thread filter columns of B (fixed for the whole kernel)
  float areg[A_EL], breg[B_EL];

  auto load = [&](long k0) {
    const long p = k0 + kl;
    const bool pv = p < kend;
    int img = 0, oy = 0, ox = 0;
    if (pv) {
      img = (int)fdiv((uint32_t)p, a.fd_pix);
      const int pix = (int)(p - (long)img * a.fd_pix.d);
      oy = (int)fdiv((uint32_t)pix, a.fd_row);
      ox = pix - oy * (int)a.fd_row.d;
    }
    const float* dyb = a.dy + (long)img * a.Cout * a.HoWo + (long)oy * a.Wo + ox;
#pragma unroll
    for (int j = 0; j < A_EL; ++j) {
      const int m = m0 + rg + j * RP;
      areg[j] = (pv && m < a.g.M) ? dyb[(long)m * a.HoWo] : 0.f;
    }
    const int q = (int)fdiv((uint32_t)img, a.fd_bdiv);
    const float* b0 = a.in.p0 + (long)(img - q * (int)a.fd_bdiv.d) * a.in.bs0 + (long)q * a.in.bhi;
    const float* b1 = a.in.p1 ? a.in.p1 + (long)img * a.in.bs1 : nullptr;
    const int py = oy * S - a.pad, px = ox * S - a.pad;
#pragma unroll
    for (int j = 0; j < B_EL; ++j) {
      const int nidx = n0 + rg + j * RP;
      float v = 0.f;
      if (pv && nidx < a.g.N) {
        const int c = nidx / KK;
        const int r = nidx - c * KK;
        const int kh = r / KW, kw = r - (r / KW) * KW;
        int iy = py + kh, ix = px + kw;
        bool ok = true;
        if (RFL) {
          iy = refl(iy, a.H);
          ix = refl(ix, a.W);
        } else {
          ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        }
        const float* src = (c < a.in.c0) ? b0 + (long)c * a.HW : b1 + (long)(c - a.in.c0) * a.HW;
        if (ok) v = src[iy * a.W + ix];
      }
      breg[j] = v;
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int j = 0; j < A_EL; ++j) As[buf][kl][rg + j * RP] = areg[j];
#pragma unroll
    for (int j = 0; j < B_EL; ++j) Bs[buf][kl][rg + j * RP] = breg[j];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    load(kbeg);
    store_tiles(0);
  }
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    if (t + 1 < nk) load(kbeg + (long)(t + 1) * BK);
    mma_chunk<TM, TN, BK>(&As[cur][0][0], LDA, &Bs[cur][0][0], LDB, wm * TM * 32, wn * TN * 32, lane, acc);
    if (t + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }

  float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long nn = n0 + wn * TN * 32 + j * 32 + (lane & 31);
    if (nn >= a.g.N) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < a.g.M) sl[(long)m * a.g.N + nn] = acc[i][j][r];
      }
  }
}

// tap-major wgrad: filter columns n = tap*Cin + c.  A block covers TT = BN/CW consecutive taps
// x CW channels (CW | Cin, and CW | the concat split, so the block reads one tensor): row j of a
// thread is tap (RP*j)/CW and channel (RP*j)%CW + rg, both compile-time up to the block base.
// Per K chunk each thread computes one gather offset per tap (TT of them); every element is then
// a buffer load with that offset and a scalar channel soffset -- no VALU per element.  The slab
// is written in (m, n) tap-major order; the final reduction permutes to [Cout][Cin][KH][KW].
template <int BM, int BN, int BK, int WM, int WN, int KH, int KW, int S, int RFL, int CW>
__global__ __launch_bounds__(256) void conv_wgrad_tap_kernel(ConvArgs a) {
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int KK = KH * KW;
  constexpr int RP = 256 / BK;          // rows per pass
  constexpr int A_EL = BM / RP, B_EL = BN / RP;
  constexpr int TT = BN / CW;           // taps per block
  constexpr int LDA = BM + 1, LDB = BN + 1;
  static_assert(A_EL >= 1 && B_EL >= 1 && TT >= 1 && CW % RP == 0, "tile");
  __shared__ float As[2][BK][LDA];
  __shared__ float Bs[2][BK][LDB];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int m0 = blockIdx.y * BM;
  const int ncb = a.Cin / CW;
  const int tb = (int)blockIdx.x / ncb * TT;           // first tap of the block
  const int cbk = ((int)blockIdx.x % ncb) * CW;        // first channel of the block
  const int kbeg = blockIdx.z * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;
  const int kl = tid % BK;
  const int rg = tid / BK;
  const int mlim = a.g.M - m0 - rg;     // row j of dY valid iff RP*j < mlim

  const bool sec = cbk >= a.in.c0;      // block-uniform concat side
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(a.dy, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rx = sec ? make_rsrc(a.in.p1, a.b1_bytes) : make_rsrc(a.in.p0, a.b0_bytes);
  const uint32_t cso = (uint32_t)(sec ? cbk - a.in.c0 : cbk) * a.HW4;

  float areg[A_EL], breg[B_EL];

  // all offsets in 32 bits: every extent is < 2 GB (checked on the host)
#define MD2_W_LOAD(K0)                                                                            \
  {                                                                                               \
    const int p = (K0) + kl;                                                                      \
    const bool pv = p < kend;                                                                     \
    const uint32_t pc = (uint32_t)(pv ? p : kbeg);                                                \
    const uint32_t img = fdiv(pc, a.fd_pix);                                                      \
    const uint32_t pix = pc - img * a.fd_pix.d;                                                   \
    const uint32_t oy = fdiv(pix, a.fd_row);                                                      \
    const uint32_t ox = pix - oy * a.fd_row.d;                                                    \
    const uint32_t va = pv ? ((img * (uint32_t)a.Cout + rg) * (uint32_t)a.HoWo + pix) * 4u : OOB; \
    _Pragma("unroll") for (int j = 0; j < A_EL; ++j)                                              \
      areg[j] = bload_s(rdy, RP * j < mlim ? va : OOB, (uint32_t)(m0 + RP * j) * a.HoWo4);        \
    uint32_t vb;                                                                                  \
    if (sec) {                                                                                    \
      vb = (img * (uint32_t)a.in.bs1 + rg * (uint32_t)a.HW) * 4u;                                 \
    } else {                                                                                      \
      const uint32_t q = fdiv(img, a.fd_bdiv);                                                    \
      vb = ((img - q * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + q * (uint32_t)a.in.bhi +               \
            rg * (uint32_t)a.HW) * 4u;                                                            \
    }                                                                                             \
    const int py = (int)oy * S - a.pad, px = (int)ox * S - a.pad;                                 \
    uint32_t vt[TT];                                                                              \
    _Pragma("unroll") for (int t = 0; t < TT; ++t) {                                              \
      const int tap = tb + t;                                                                     \
      const int kh = tap / KW, kw = tap - (tap / KW) * KW;                                        \
      int iy = py + kh, ix = px + kw;                                                             \
      bool ok;                                                                                    \
      if (RFL) {                                                                                  \
        iy = refl(iy, a.H);                                                                       \
        ix = refl(ix, a.W);                                                                       \
        ok = pv;                                                                                  \
      } else {                                                                                    \
        ok = pv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;                  \
      }                                                                                           \
      vt[t] = (ok && tap < KK) ? vb + (uint32_t)(iy * a.W + ix) * 4u : OOB;                       \
    }                                                                                             \
    _Pragma("unroll") for (int j = 0; j < B_EL; ++j)                                              \
      breg[j] = bload_s(rx, vt[(RP * j) / CW], cso + (uint32_t)((RP * j) % CW) * a.HW4);         \
  }
#define MD2_W_STORE(BUF)                                                                          \
  _Pragma("unroll") for (int j = 0; j < A_EL; ++j) As[BUF][kl][rg + j * RP] = areg[j];            \
  _Pragma("unroll") for (int j = 0; j < B_EL; ++j) Bs[BUF][kl][rg + j * RP] = breg[j];

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    MD2_W_LOAD(kbeg);
    MD2_W_STORE(0);
  }
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    if (t + 1 < nk) MD2_W_LOAD(kbeg + (t + 1) * BK);
    mma_chunk<TM, TN, BK>(&As[cur][0][0], LDA, &Bs[cur][0][0], LDB, wm * TM * 32, wn * TN * 32, lane, acc);
    if (t + 1 < nk) {
      MD2_W_STORE(cur ^ 1);
    }
    __syncthreads();
  }
#undef MD2_W_LOAD
#undef MD2_W_STORE

  float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wn * TN * 32 + j * 32 + (lane & 31);
    const int tap = tb + nl / CW;
    if (tap >= KK) continue;
    const long nn = (long)tap * a.Cin + cbk + nl % CW;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < a.g.M) sl[(long)m * a.g.N + nn] = acc[i][j][r];
      }
  }
}

// Weight gradient of a Cout <= 32, 3x3 stride-1 tap-major conv (the high-resolution
// DepthDecoder convs): dW[m][tap*Cin + c] = sum_p dY[m][p] X[c][gather(p, tap)].  32-row x
// 128-column MFMA tiles would leave rows idle (Cout 16) and waste up to 7/16 of the 144 = 9 taps
// x 16 channels, so here one block owns ALL 16*MT rows x ALL 9 taps of a 16-channel group and
// the four waves split the pixel (K) dimension instead: per 64-pixel chunk the block stages
// A[64 px][16*MT m] and B[9 taps][64 px][16 ch] in LDS (coalesced 64-pixel loads, wave-uniform
// row / channel soffsets, one gather offset per tap), wave w contracts pixels 16w..16w+15 on
// v_mfma_f32_16x16x4_f32 into MT x 9 accumulators (each B fragment feeds MT MFMAs), and a
// fixed-order LDS sum over the waves writes the block's split-K slab (tap-major, finalised by
// wgrad_reduce_kernel).  Every MFMA row and column is useful work.
template <int MT, int KH, int KW, int RFL>
__global__ __launch_bounds__(256) void conv_wgrad16_kernel(ConvArgs a) {
  constexpr int KK = KH * KW, BK = 64, LD = 17, LDA = 16 * MT + 1, RW = 4 * MT;
  static_assert(4 * KK * 4 * 64 <= KK * BK * LD, "reduction buffer");
  __shared__ float As[BK * LDA];
  __shared__ float Bs[KK * BK * LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cbk = (int)blockIdx.x * 16;
  const int kbeg = blockIdx.z * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;

  const bool sec = cbk >= a.in.c0;
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(a.dy, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rx = sec ? make_rsrc(a.in.p1, a.b1_bytes) : make_rsrc(a.in.p0, a.b0_bytes);
  // wave w loads dY rows RW*w..RW*w+RW-1 and X channels cbk+4w..cbk+4w+3 (wave-uniform soffsets)
  const uint32_t cso = (uint32_t)((sec ? cbk - a.in.c0 : cbk) + 4 * wid) * a.HW4;
  const uint32_t mso = (uint32_t)(RW * wid) * a.HoWo4;

  float areg[RW], breg[KK][4];
  auto load = [&](int k0) {
    const int p = k0 + lane;
    const bool pv = p < kend;
    const uint32_t pc = (uint32_t)(pv ? p : kbeg);
    const uint32_t img = fdiv(pc, a.fd_pix);
    const uint32_t pix = pc - img * a.fd_pix.d;
    const uint32_t oy = fdiv(pix, a.fd_row);
    const uint32_t ox = pix - oy * a.fd_row.d;
    const uint32_t va = pv ? (img * (uint32_t)a.Cout * (uint32_t)a.HoWo + pix) * 4u : OOB;
#pragma unroll
    for (int r = 0; r < RW; ++r)
      areg[r] = bload_s(rdy, RW * wid + r < a.g.M ? va : OOB, mso + (uint32_t)r * a.HoWo4);
    uint32_t vb;
    if (sec) {
      vb = img * (uint32_t)a.in.bs1 * 4u;
    } else {
      const uint32_t q = fdiv(img, a.fd_bdiv);
      vb = ((img - q * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + q * (uint32_t)a.in.bhi) * 4u;
    }
    const int py = (int)oy - a.pad, px = (int)ox - a.pad;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      int iy = py + t / KW, ix = px + t % KW;
      bool ok;
      if (RFL) {
        iy = refl(iy, a.H);
        ix = refl(ix, a.W);
        ok = pv;
      } else {
        ok = pv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      }
      const uint32_t vt = ok ? vb + (uint32_t)(iy * a.W + ix) * 4u : OOB;
#pragma unroll
      for (int c = 0; c < 4; ++c) breg[t][c] = bload_s(rx, vt, cso + (uint32_t)c * a.HW4);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int r = 0; r < RW; ++r) As[lane * LDA + RW * wid + r] = areg[r];
#pragma unroll
    for (int t = 0; t < KK; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) Bs[(t * BK + lane) * LD + 4 * wid + c] = breg[t][c];
  };

  f32x4 acc[MT][KK];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int i = lane & 15, g = lane >> 4;
  if (nk > 0) load(kbeg);
  for (int t = 0; t < nk; ++t) {
    store();
    __syncthreads();
    if (t + 1 < nk) load(kbeg + (t + 1) * BK);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const int k = 16 * wid + 4 * s4 + g;
      float av[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) av[mt] = As[k * LDA + 16 * mt + i];
#pragma unroll
      for (int tp = 0; tp < KK; ++tp) {
        const float bv = Bs[(tp * BK + k) * LD + i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv, acc[mt][tp], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // fixed-order sum over the four waves' K quarters, one 16-row tile at a time (Bs reused)
  float* red = Bs;
  float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int tp = 0; tp < KK; ++tp)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((wid * KK + tp) * 4 + r) * 64 + lane] = acc[mt][tp][r];
    __syncthreads();
    for (int o = tid; o < KK * 4 * 64; o += 256) {
      const int l = o & 63, r = (o >> 6) & 3, tp = o >> 8;
      const int m = 16 * mt + 4 * (l >> 4) + r, j = l & 15;
      const float v = red[((0 * KK + tp) * 4 + r) * 64 + l] + red[((1 * KK + tp) * 4 + r) * 64 + l] +
                      red[((2 * KK + tp) * 4 + r) * 64 + l] + red[((3 * KK + tp) * 4 + r) * 64 + l];
      if (m < a.g.M) sl[(long)m * a.g.N + (long)tp * a.Cin + cbk + j] = v;
    }
    if (mt + 1 < MT) __syncthreads();
  }
}

// Weight gradient of the ResNet stem (7x7 / stride 2, Cin <= 4 image channels, Cout = 64):
// dW[m][c*49 + tap] = sum_p dY[m][p] X[c][gather(p, tap)] with K = every output pixel (479k at
// B=12).  The generic 64x128 tiles pad its 147 filter columns to 256 (42% idle MFMA columns) and
// index every element of B; here one block owns ALL 64 rows x ALL Cin*49 columns (NT 16-column
// tiles: 147 -> 160) of a K slice, wave w the 16 rows 16w.. on v_mfma_f32_16x16x4_f32.  Per
// 64-pixel chunk: A[64 px][64 m] (coalesced dY rows, wave w its own 16) and B[64 px][NT*16] (one
// gather offset base per lane, the tap / channel parts wave-uniform) staged through LDS from
// registers loaded during the previous chunk's MFMAs.  Columns come out channel-major, i.e. in
// the final [Cout][Cin][KH][KW] order (wgrad_reduce_kernel with tapc = 0).
template <int CIN>
__global__ __launch_bounds__(256) void conv_wgrad_stem_kernel(ConvArgs a) {
  constexpr int KK = 49, BK = 64, LDA = 64 + 1, NT = (CIN * KK + 15) / 16, NB = NT * 16, LDB = NB + 1;
  constexpr int JB = (NB + 3) / 4;                  // B columns per thread (wave w: w, w+4, ...)
  __shared__ float As[BK * LDA];
  __shared__ float Bs[BK * LDB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kbeg = blockIdx.x * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;
  constexpr int ncol = CIN * KK;                    // filter columns
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(a.dy, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.in.p0, a.b0_bytes);
  const uint32_t mso = (uint32_t)(16 * wid) * a.HoWo4;

  float areg[16], breg[JB];
  auto load = [&](int k0) {
    const int p = k0 + lane;
    const bool pv = p < kend;
    const uint32_t pc = (uint32_t)(pv ? p : kbeg);
    const uint32_t img = fdiv(pc, a.fd_pix);
    const uint32_t pix = pc - img * a.fd_pix.d;
    const uint32_t oy = fdiv(pix, a.fd_row);
    const uint32_t ox = pix - oy * a.fd_row.d;
    const uint32_t va = pv ? (img * (uint32_t)a.Cout * (uint32_t)a.HoWo + pix) * 4u : OOB;
#pragma unroll
    for (int r = 0; r < 16; ++r) areg[r] = bload_s(rdy, va, mso + (uint32_t)r * a.HoWo4);
    const uint32_t q = fdiv(img, a.fd_bdiv);
    const int ibase = (int)((img - q * a.fd_bdiv.d) * (uint32_t)a.in.bs0 + q * (uint32_t)a.in.bhi);
    const int y0 = (int)oy * 2 - a.pad, x0 = (int)ox * 2 - a.pad;
    // image extents laundered per chunk: the per-column offsets below are re-derived by a few
    // scalar ops each chunk instead of being hoisted into scalar registers
    int Wd = a.W, Hd = a.H, HWd = (int)a.HW;
    asm volatile("" : "+s"(Wd), "+s"(Hd), "+s"(HWd));
    const int rowbase = ibase + y0 * Wd + x0;
    // per-lane validity of the 7 rows / 7 columns of the window as bit masks (integer VGPRs, not
    // 49 lane masks)
    uint32_t rb = 0, cb = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      rb |= ((unsigned)(y0 + k) < (unsigned)Hd ? 1u : 0u) << k;
      cb |= ((unsigned)(x0 + k) < (unsigned)Wd ? 1u : 0u) << k;
    }
    if (!pv) rb = 0;
    // wave w gathers columns w, w+4, ...: a compile-time column set per wave (switch below)
    auto gather = [&](auto Wc) {
      constexpr int WV = decltype(Wc)::value;
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        const int n = 4 * j + WV;
        const int c = n / KK, tap = n - c * KK;
        const int kh = tap / 7, kw = tap - kh * 7;
        // out-of-window elements get bit 31 set: past every extent, the buffer load returns 0
        // (no lane masks: plain integer ops)
        const uint32_t bad = (n < ncol) ? (~((rb >> kh) & (cb >> kw)) & 1u) : 1u;
        const uint32_t off = ((uint32_t)(rowbase + c * HWd + kh * Wd + kw) << 2) | (bad << 31);
        breg[j] = bload(rx, off);
      }
    };
    switch (wid) {
      case 0: gather(std::integral_constant<int, 0>{}); break;
      case 1: gather(std::integral_constant<int, 1>{}); break;
      case 2: gather(std::integral_constant<int, 2>{}); break;
      default: gather(std::integral_constant<int, 3>{}); break;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int r = 0; r < 16; ++r) As[lane * LDA + 16 * wid + r] = areg[r];
#pragma unroll
    for (int j = 0; j < JB; ++j)
      if (4 * j + wid < NB) Bs[lane * LDB + 4 * j + wid] = breg[j];
  };

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int i = lane & 15, g = lane >> 4;
  if (nk > 0) load(kbeg);
  for (int t = 0; t < nk; ++t) {
    store();
    __syncthreads();
    if (t + 1 < nk) load(kbeg + (t + 1) * BK);
#pragma unroll
    for (int s4 = 0; s4 < BK / 4; ++s4) {
      const int k = 4 * s4 + g;
      const float av = As[k * LDA + 16 * wid + i];
#pragma unroll
      for (int tn = 0; tn < NT; ++tn)
        acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bs[k * LDB + 16 * tn + i], acc[tn], 0, 0, 0);
    }
    __syncthreads();
  }
  float* sl = a.slab + (long)blockIdx.x * a.g.M * a.g.N;
#pragma unroll
  for (int tn = 0; tn < NT; ++tn) {
    const int n = 16 * tn + i;
    if (n >= ncol) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) sl[(long)(16 * wid + 4 * g + r) * ncol + n] = acc[tn][r];
  }
}

// One-launch wgrad finalise: the split-K slab sum (SUB lanes per output, each a fixed split
// subsequence, combined in a fixed order: deterministic), the tap-major -> [Cout][Cin][KK]
// remap, accumulate, and -- in the trailing blocks -- the bias-gradient finalise over the
// bias_grad_partial_kernel partials (launched before this kernel).
struct WRed {
  const float* slab;
  int splits;
  long total;
  float* dw;
  int acc;
  int ncols, tapc, KK;
  int cinw;             // the weights' Cin (< tapc: columns of padded input channels dropped)
  long out_total;       // outputs written: Cout * cinw * KK
  const float* bpart;   // [Cout][bparts] or nullptr
  int bparts, Cout;
  float* db;
  int nmain;            // blocks of the slab reduction
};

template <int SUB>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WRed r) {
  constexpr int OPB = 256 / SUB;   // outputs per block
  if ((int)blockIdx.x >= r.nmain) {
    const int c = ((int)blockIdx.x - r.nmain) * 256 + threadIdx.x;
    if (c >= r.Cout) return;
    float sb = 0.f;
    for (int p = 0; p < r.bparts; ++p) sb += r.bpart[(long)c * r.bparts + p];
    if (r.acc)
      r.db[c] += sb;
    else
      r.db[c] = sb;
    return;
  }
  __shared__ float red[SUB][OPB];
  const int j = threadIdx.x % OPB, g = threadIdx.x / OPB;
  // SUB == 1 (few slabs): thread order = OUTPUT order, coalesced dw stores, the tap-major slab
  // column gathered; SUB == 4 (many slabs): slab order, coalesced reads of every slab, the one
  // store per output scattered (measured: each order is the faster one on its side)
  long o = (long)blockIdx.x * OPB + j, idx = o;
  bool live = o < (SUB == 1 ? r.out_total : r.total);
  if (r.tapc > 0 && live) {
    const int ocols = r.cinw * r.KK;                 // output row length
    if (SUB == 1) {                                  // o: output order
      const long m = o / ocols;
      const int n = (int)(o - m * ocols);
      const int c = n / r.KK, tp = n - c * r.KK;
      idx = m * r.ncols + (long)tp * r.tapc + c;
    } else {                                         // o: slab order
      const long m = o / r.ncols;
      const int n = (int)(o - m * r.ncols);
      const int tp = n / r.tapc, c = n - tp * r.tapc;
      live = c < r.cinw;
      o = m * ocols + (long)c * r.KK + tp;
    }
  }
  // eight slab loads in flight per thread (the pass is latency-bound on the L2/MALL-resident
  // slabs: two in flight reached ~1.3 TB/s), eight fixed-order partial sums
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    int sp = g;
    for (; sp + 7 * SUB < r.splits; sp += 8 * SUB) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = r.slab[(long)(sp + u * SUB) * r.total + idx];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += t[u];
    }
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = sp + u * SUB < r.splits ? r.slab[(long)(sp + u * SUB) * r.total + idx] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] += t[u];
  }
  float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  if (SUB > 1) {
    red[g][j] = v;
    __syncthreads();
    if (g != 0) return;
    v = red[0][j];
#pragma unroll
    for (int k = 1; k < SUB; ++k) v += red[k][j];
  }
  if (!live) return;
  if (r.acc)
    r.dw[o] += v;
  else
    r.dw[o] = v;
}
