// ---------------------------------------------------------------------------------------------
// forward / dgrad implicit-GEMM kernel for M <= 16 (the 16-channel full-resolution DepthDecoder
// convs: Cout = 16 forward, Cin = 16 data gradient); included by conv_px_launch.h after
// conv_px2.inc.  MODE 0 = forward, MODE 1 = dgrad; tap-major K only (C % 16 == 0), no split-K.
//
// A 32-row MFMA tile would leave half its rows idle here, so the contraction runs on
// v_mfma_f32_16x16x4_f32 (16 x 16 outputs, K = 4 per instruction, same 64 FLOP/clk/SIMD).
// Block: 256 threads, 16 output rows x BN pixels; wave w owns pixels [w*BN/4, (w+1)*BN/4) as
// BN/64 MFMA column tiles.  Per 16-deep K chunk the LDS holds As[16][k] and Bs[BN][k]
// k-contiguous (row stride 20 floats, as conv_px2): MFMA step kk contracts physical
// k = {kk, 4+kk, 8+kk, 12+kk} -- lane (i, g) supplies A[i][4g+kk] / B[4g+kk][j] -- so a lane's
// four A (or B) values of the chunk are ONE ds_read_b128.  Every wave loads the 16 x 16 A chunk
// (uniform load counts keep the register ring's vmcnt exact); wave w stores rows 4w..4w+3.  The B gather is conv_px2's
// (px2_gather: wave w loads channels 4w..4w+3 of the chunk, wave-uniform scalar soffsets).
// Output layout of the 16x16x4 MFMA: lane l holds column j = l & 15, rows 4*(l >> 4) + r.
// ---------------------------------------------------------------------------------------------

template <int MODE, int BN, int KH, int KW, int S, int RFL>
__global__ __launch_bounds__(256) void conv_px16_kernel(ConvArgs a) {
  constexpr int BK = 16, LD = 20;
  constexpr int PPT = BN / 64;                // B pixels per lane (gather)
  constexpr int NT = BN / 64;                 // 16-wide MFMA column tiles per wave
  static_assert(BN % 64 == 0 && S == 1, "tile");
  __shared__ __attribute__((aligned(16))) float As[2][16][LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][BN][LD];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * BN;
  const int nk = (a.g.K + BK - 1) / BK;

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
        py[p] = oy - a.pad;
        px[p] = ox - a.pad;
        const int q = (int)fdiv((uint32_t)img, a.fd_bdiv);
        boff0[p] = (uint32_t)((long)(img - q * (int)a.fd_bdiv.d) * a.in.bs0 + (long)q * a.in.bhi) * 4u;
        boff1[p] = (uint32_t)((long)img * a.in.bs1) * 4u;
      } else {
        py[p] = oy;
        px[p] = ox;
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
  int tap = 0, cb = 0, kc = 0;
  constexpr int D = 2;
  float4 areg[D];
  float breg[D][PPT][4];

#define MD2_PX16_ADVANCE()                                                                        \
  {                                                                                               \
    ++kc;                                                                                         \
    cb += BK;                                                                                     \
    if (cb == Ck) {                                                                               \
      cb = 0;                                                                                     \
      ++tap;                                                                                      \
    }                                                                                             \
  }
#define MD2_PX16_LOAD(SET)                                                                        \
  {                                                                                               \
    const bool kv = kc < nk;                                                                      \
    const int arow = tap * Ck + cb;                                                               \
    areg[SET] = bload4(rA, kv ? (uint32_t)(((arow >> 4) * a.g.Mpad + (lane >> 2)) * 16 + (lane & 3) * 4) * 4u \
                              : OOB);                                                             \
    px2_gather<MODE, KW, S, RFL, PPT>(a, kv, tap, cb, wq, py, px, nvalid, wborder, boff0, boff1,  \
                                      r0, r1, breg[SET]);                                         \
  }
#define MD2_PX16_STORE(BUF, SET)                                                                  \
  {                                                                                               \
    if ((lane >> 4) == wq) *reinterpret_cast<float4*>(&As[BUF][lane >> 2][(lane & 3) * 4]) = areg[SET]; \
    _Pragma("unroll") for (int p = 0; p < PPT; ++p)                                               \
      *reinterpret_cast<float4*>(&Bs[BUF][lane + 64 * p][wq * 4]) =                               \
          make_float4(breg[SET][p][0], breg[SET][p][1], breg[SET][p][2], breg[SET][p][3]);        \
  }

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.f;

  const int fi = lane & 15, fg = lane >> 4;
  MD2_PX16_LOAD(0);
  MD2_PX16_ADVANCE();
  MD2_PX16_LOAD(1);
  MD2_PX16_STORE(0, 0);
  __syncthreads();
  const int nkp = (nk + 1) / 2 * 2;
  for (int t0 = 0; t0 < nkp; t0 += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int cur = u;   // chunk t0 + u lives in LDS buffer (t0 + u) & 1 = u
      MD2_PX16_ADVANCE();
      MD2_PX16_LOAD(u);
      __builtin_amdgcn_sched_barrier(0);
      const float4 fa = *reinterpret_cast<const float4*>(&As[cur][fi][fg * 4]);
      float4 fb[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        fb[t] = *reinterpret_cast<const float4*>(&Bs[cur][wq * (BN / 4) + 16 * t + fi][fg * 4]);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32((&fa.x)[kk], (&fb[t].x)[kk], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      MD2_PX16_STORE(cur ^ 1, u ^ 1);
      __syncthreads();
    }
  }
#undef MD2_PX16_ADVANCE
#undef MD2_PX16_LOAD
#undef MD2_PX16_STORE

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const long nn = (long)n0 + wq * (BN / 4) + 16 * t + fi;
    if (nn >= a.g.N) continue;
    int img;
    long pix, plane;
    out_pixel(a, false, 0, 0, nn, img, pix, plane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * fg + r;
      if (m < a.g.M) store_out(a.out, m, img, pix, plane, acc[t][r]);
    }
  }
}
