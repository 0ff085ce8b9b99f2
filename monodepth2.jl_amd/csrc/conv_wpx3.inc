// ---------------------------------------------------------------------------------------------
// tap-major weight gradient on the bf16 MFMA with split products (the arithmetic of conv_px3);
// included by conv_wgrad.hip (split3_pk and the bf16 vector types: conv_kernel.h).
//
//   dW[m][tap*Cin + c] = sum_p dY[m][p] X[c][gather(p, tap)]     (K = the N*Ho*Wo pixels)
//
// Same block -> (tap group, channel group, row tile, split) map and the same tap-major split-K
// slab as conv_wgrad_tap_kernel, so the planner, workspace and wgrad_reduce_kernel are shared.
// What differs is the contraction: BOTH operands are activations, so both are split in registers
// (split3_pk: x = hi + mid + lo in bf16, exact) as they are staged, and each 16-pixel chunk runs
// NT (6 or 9) v_mfma_f32_32x32x16_bf16 per 32x32 tile instead of eight v_mfma_f32_32x32x2_f32.
//   * a thread owns PX consecutive PIXELS (2 or 4) of the chunk and rows rg, rg + RP, ... of each
//     operand: consecutive pixels are what packed bf16 dwords hold, so the split writes
//     k-contiguous LDS images As/Bs[part][row][k] directly (conv_px3's B layout: 48-byte rows,
//     ds_read_b128 fragments).
//   * dY rows are one 8- / 16-byte load per lane (a lane's pixels never straddle two images:
//     HoWo % PX == 0), and the X taps of a lane's pixels, adjacent in memory for every stride-1
//     pixel group that does not touch a border or wrap a row, are one 8- / 16-byte load as well;
//     the other groups gather per pixel (PX 4-byte loads, OOB offsets = zero padding).
//   * what bounds it is neither the MFMA nor the split (timing-only builds, profiles/
//     r04_wgrad_px3.txt: dropping 5 of the 6 MFMAs moved a layer 10-15%, dropping the split's
//     remainders 4%) but the staging: the whole-pair 8-byte X loads took 8-17% off every
//     stride-1 layer; PX = 4 (16-byte loads, half the load instructions again) gained nothing
//     more on stride 1 and lost 30% on stride 2.  The launches use PX = 2.
//   * hi.hi accumulates in its own tile, the cross terms in a second (conv_px3's error split).
// ---------------------------------------------------------------------------------------------

template <int PX>
struct WxVec;
template <>
struct WxVec<2> {
  typedef float2 T;
};
template <>
struct WxVec<4> {
  typedef float4 T;
};

__device__ __forceinline__ float2 wx_load(__amdgpu_buffer_rsrc_t r, uint32_t v, uint32_t s, float2*) {
  return bload2_s(r, v, s);
}
__device__ __forceinline__ float4 wx_load(__amdgpu_buffer_rsrc_t r, uint32_t v, uint32_t s, float4*) {
  const auto q = __builtin_amdgcn_raw_buffer_load_b128(r, (int)v, (int)s, 0);
  return make_float4(__uint_as_float(q[0]), __uint_as_float(q[1]), __uint_as_float(q[2]),
                     __uint_as_float(q[3]));
}
__device__ __forceinline__ float& wx_at(float2& v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ float& wx_at(float4& v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

template <int BM, int BN, int WM, int WN, int KH, int KW, int S, int RFL, int CW, int NT, int PX>
__global__ __launch_bounds__(256, 2) void conv_wgrad_px3_kernel(ConvArgs a) {   // >= 2 waves/SIMD
  static_assert(NT == 9 || NT == 6, "split products");
  static_assert(PX == 2 || PX == 4, "pixels per lane");
  typedef typename WxVec<PX>::T vec;
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int KK = KH * KW;
  constexpr int BK = 16, LDK = BK + 8;   // pixels per chunk; bf16 row stride of the LDS images
  constexpr int LPR = BK / PX;           // lanes per row (pixel groups of a chunk)
  constexpr int RP = 256 / LPR;          // rows per pass
  constexpr int A_EL = BM / RP, B_EL = BN / RP;
  constexpr int TT = BN / CW;            // taps per block
  static_assert(TM >= 1 && TN >= 1 && A_EL >= 1 && B_EL >= 1 && TT >= 1 && CW % RP == 0 &&
                    WM * WN == 4, "tile");
  __shared__ __attribute__((aligned(16))) uint16_t As[2][3][BM][LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[2][3][BN][LDK];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wq / WN, wn = wq % WN;
  const int m0 = blockIdx.y * BM;
  const int ncb = a.Cin / CW;
  const int tb = (int)blockIdx.x / ncb * TT;           // first tap of the block
  const int cbk = ((int)blockIdx.x % ncb) * CW;        // first channel of the block
  const int kbeg = blockIdx.z * a.g.kper;
  const int kend = min(a.g.K, kbeg + a.g.kper);
  const int nk = (kend - kbeg + BK - 1) / BK;
  const int kp = tid % LPR;                            // pixel group PX*kp .. PX*kp + PX-1 of the chunk
  // row group; with 8 lanes per row the 8 rows of a wave are permuted so that each 32-lane half
  // writes rows {0,2,4,6} / {1,3,5,7}: their 8-dword windows at a 12-dword row stride fall in
  // disjoint banks (ds_write_b32 banks are (addr/4) % 32 per 32-lane half)
  const int rg = LPR == 8 ? (tid >> 6) * 8 + (((tid >> 3) & 3) << 1) + ((tid >> 5) & 1) : tid / LPR;
  const int mlim = a.g.M - m0 - rg;                    // dY row j valid iff RP*j < mlim

  const bool sec = cbk >= a.in.c0;                     // block-uniform concat side
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(a.dy, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rx = sec ? make_rsrc(a.in.p1, a.b1_bytes) : make_rsrc(a.in.p0, a.b0_bytes);
  const uint32_t cso = (uint32_t)(sec ? cbk - a.in.c0 : cbk) * a.HW4;

  // 2-deep register ring: chunk t is loaded one chunk ahead of its split + LDS store
  constexpr int D = 2;
  vec areg[D][A_EL], breg[D][B_EL];

  // K (pixels) and kper are multiples of PX (HoWo % PX == 0): a pixel group is valid or invalid as a
  // whole, lies in one image, and wraps at most one row (Wo >= PX - 1, checked on the host)
  // the chunks are loaded strictly in order, so a lane's pixel group advances by BK pixels per
  // load: (image, row, column) and the dY element offset are carried forward with adds and two
  // compares instead of re-divided (past kend the state runs on, every offset is then OOB)
  int s_p = kbeg + PX * kp;
  uint32_t s_img = fdiv((uint32_t)s_p, a.fd_pix);
  uint32_t s_oy, s_ox, s_va;
  {
    const uint32_t pix = (uint32_t)s_p - s_img * a.fd_pix.d;
    s_oy = fdiv(pix, a.fd_row);
    s_ox = pix - s_oy * a.fd_row.d;
    s_va = (s_img * (uint32_t)a.Cout + rg) * (uint32_t)a.HoWo + pix;
  }
  const uint32_t d_img = fdiv((uint32_t)BK, a.fd_pix), r_bk = (uint32_t)BK - d_img * a.fd_pix.d;
  const uint32_t d_oy = fdiv(r_bk, a.fd_row), d_ox = r_bk - d_oy * a.fd_row.d;
  const uint32_t va_img = (uint32_t)(a.Cout - 1) * (uint32_t)a.HoWo;   // dY offset step per image
  const uint32_t va_bk = (uint32_t)BK + d_img * va_img;

#define MD2_WX_LOAD(K0, SET)                                                                      \
  {                                                                                               \
    const bool pv = s_p < kend;                                                                   \
    const uint32_t img = s_img, oy = s_oy, ox = s_ox;                                             \
    const uint32_t va = pv ? s_va * 4u : OOB;                                                     \
    _Pragma("unroll") for (int j = 0; j < A_EL; ++j)                                              \
      areg[SET][j] = wx_load(rdy, RP * j < mlim ? va : OOB, (uint32_t)(m0 + RP * j) * a.HoWo4,    \
                             (vec*)nullptr);                                                      \
    const uint32_t qd = fdiv(img, a.fd_bdiv);                                                     \
    const uint32_t vb = sec ? (img * (uint32_t)a.in.bs1 + rg * (uint32_t)a.HW) * 4u               \
                            : ((img - qd * a.fd_bdiv.d) * (uint32_t)a.in.bs0 +                    \
                               qd * (uint32_t)a.in.bhi + rg * (uint32_t)a.HW) * 4u;               \
    int pyi[PX], pxi[PX];                                                                         \
    _Pragma("unroll") for (int i = 0; i < PX; ++i) {                                              \
      const bool wrap = (int)ox + i >= (int)a.fd_row.d;                                           \
      pyi[i] = ((int)oy + (wrap ? 1 : 0)) * S - a.pad;                                            \
      pxi[i] = ((int)ox + i - (wrap ? (int)a.fd_row.d : 0)) * S - a.pad;                          \
    }                                                                                             \
    uint32_t vt[TT][PX];                                                                          \
    bool whole = true;                                                                            \
    _Pragma("unroll") for (int tt = 0; tt < TT; ++tt) {                                           \
      const int tap = tb + tt;                                                                    \
      const int kh = tap / KW, kw = tap - (tap / KW) * KW;                                        \
      _Pragma("unroll") for (int i = 0; i < PX; ++i) {                                            \
        int iy = pyi[i] + kh, ix = pxi[i] + kw;                                                   \
        bool ok;                                                                                  \
        if (RFL) {                                                                                \
          iy = refl(iy, a.H);                                                                     \
          ix = refl(ix, a.W);                                                                     \
          ok = pv;                                                                                \
        } else {                                                                                  \
          ok = pv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;                \
        }                                                                                         \
        vt[tt][i] = (ok && tap < KK) ? vb + (uint32_t)(iy * a.W + ix) * 4u : OOB;                 \
        if (i > 0) whole = whole && vt[tt][i] == vt[tt][0] + 4u * i;                              \
      }                                                                                           \
    }                                                                                             \
    if (S == 1 && whole) {                                                                        \
      _Pragma("unroll") for (int j = 0; j < B_EL; ++j)                                            \
        breg[SET][j] = wx_load(rx, vt[(RP * j) / CW][0], cso + (uint32_t)((RP * j) % CW) * a.HW4, \
                               (vec*)nullptr);                                                    \
    } else {                                                                                      \
      _Pragma("unroll") for (int j = 0; j < B_EL; ++j) {                                          \
        const uint32_t so = cso + (uint32_t)((RP * j) % CW) * a.HW4;                              \
        _Pragma("unroll") for (int i = 0; i < PX; ++i)                                            \
          wx_at(breg[SET][j], i) = bload_s(rx, vt[(RP * j) / CW][i], so);                         \
      }                                                                                           \
    }                                                                                             \
    s_p += BK;                                                                                    \
    s_ox += d_ox;                                                                                 \
    const bool c1 = s_ox >= a.fd_row.d;                                                           \
    s_ox -= c1 ? a.fd_row.d : 0u;                                                                 \
    s_oy += d_oy + (c1 ? 1u : 0u);                                                                \
    const bool c2 = s_oy >= (uint32_t)a.Ho;                                                       \
    s_oy -= c2 ? (uint32_t)a.Ho : 0u;                                                             \
    s_img += d_img + (c2 ? 1u : 0u);                                                              \
    s_va += va_bk + (c2 ? va_img : 0u);                                                           \
  }
  // split into the three packed bf16 images: PX / 2 dwords per part and row
#define MD2_WX_SPLIT_STORE(IMG, ROW, V)                                                           \
  {                                                                                               \
    uint32_t h[PX / 2], md[PX / 2], l[PX / 2];                                                    \
    _Pragma("unroll") for (int e = 0; e < PX / 2; ++e)                                            \
      split3_pk(wx_at(V, 2 * e), wx_at(V, 2 * e + 1), h[e], md[e], l[e]);                         \
    if constexpr (PX == 2) {                                                                      \
      *reinterpret_cast<uint32_t*>(&IMG[0][ROW][PX * kp]) = h[0];                                 \
      *reinterpret_cast<uint32_t*>(&IMG[1][ROW][PX * kp]) = md[0];                                \
      *reinterpret_cast<uint32_t*>(&IMG[2][ROW][PX * kp]) = l[0];                                 \
    } else {                                                                                      \
      *reinterpret_cast<uint2*>(&IMG[0][ROW][PX * kp]) = make_uint2(h[0], h[PX / 2 - 1]);        \
      *reinterpret_cast<uint2*>(&IMG[1][ROW][PX * kp]) = make_uint2(md[0], md[PX / 2 - 1]);      \
      *reinterpret_cast<uint2*>(&IMG[2][ROW][PX * kp]) = make_uint2(l[0], l[PX / 2 - 1]);        \
    }                                                                                             \
  }
#define MD2_WX_STORE(BUF, SET)                                                                    \
  {                                                                                               \
    _Pragma("unroll") for (int j = 0; j < A_EL; ++j)                                              \
      MD2_WX_SPLIT_STORE(As[BUF], rg + RP * j, areg[SET][j]);                                     \
    _Pragma("unroll") for (int j = 0; j < B_EL; ++j)                                              \
      MD2_WX_SPLIT_STORE(Bs[BUF], rg + RP * j, breg[SET][j]);                                     \
  }

  f32x16 acc0[TM][TN], acc1[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[i][j][r] = acc1[i][j][r] = 0.f;

  const int fi = lane & 31, fh = lane >> 5;
  // every chunk's load and store is unconditional: past kend a group is invalid (OOB loads return
  // 0) and a store past the last chunk lands in the buffer nobody reads again
#pragma unroll
  for (int u = 0; u < D; ++u) MD2_WX_LOAD(kbeg + u * BK, u);
  MD2_WX_STORE(0, 0);
  __syncthreads();
  const int nkp = (nk + D - 1) / D * D;
  for (int t0 = 0; t0 < nkp; t0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int t = t0 + u, cur = t & 1;
      if (t < nk) {
        u32x4_t fa[TM][3], fb[TN][3];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int q = 0; q < 3; ++q)
            fa[i][q] = *reinterpret_cast<const u32x4_t*>(&As[cur][q][wm * TM * 32 + i * 32 + fi][8 * fh]);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 3; ++q)
            fb[j][q] = *reinterpret_cast<const u32x4_t*>(&Bs[cur][q][wn * TN * 32 + j * 32 + fi][8 * fh]);
        // chunk t + 1 (set u + 1) into the other LDS buffer
        MD2_WX_STORE(cur ^ 1, (u + 1) % D);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const bf16x8_t ah = __builtin_bit_cast(bf16x8_t, fa[i][0]);
            const bf16x8_t am = __builtin_bit_cast(bf16x8_t, fa[i][1]);
            const bf16x8_t al = __builtin_bit_cast(bf16x8_t, fa[i][2]);
            const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, fb[j][0]);
            const bf16x8_t bm = __builtin_bit_cast(bf16x8_t, fb[j][1]);
            const bf16x8_t bl = __builtin_bit_cast(bf16x8_t, fb[j][2]);
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
        // set u held chunk t (in LDS since the previous chunk): refill it with chunk t + D
        MD2_WX_LOAD(kbeg + (t + D) * BK, u);
      }
      __syncthreads();
    }
  }
#undef MD2_WX_LOAD
#undef MD2_WX_STORE
#undef MD2_WX_SPLIT_STORE

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
        if (m < a.g.M) sl[(long)m * a.g.N + nn] = acc0[i][j][r] + acc1[i][j][r];
      }
  }
}
