// ---------------------------------------------------------------------------------------------
// stride-1 3x3 zero-padded forward / dgrad on the bf16x6 split products with an LDS HALO
// (its own translation unit, conv_halo.hip).  MODE 0 = forward (B = X, tap (kh, kw) reads
// (y + kh - 1, x + kw - 1)), MODE 1 = dgrad (B = dY, (y + 1 - kh, x + 1 - kw)).
//
// conv_px3 gathers the B operand once per (tap, 16-channel chunk): every input value is loaded,
// split into its three bf16 terms and written to LDS NINE times, and the block synchronises
// after every 6 MFMAs per wave.  Here a block owns 64 output channels x 256 consecutive output
// pixels (N order = image, row, column) and walks the reduction CHANNEL chunk by channel chunk;
// per chunk it stages the rows its pixels touch plus one halo row above and below -- each input
// value loaded and split ONCE -- and the nine taps read their B fragments from that one LDS
// image at shifted pixel offsets: 9 x 12 MFMAs per wave between two barriers.
//
//   Block: 512 threads = 8 waves (2 along M x 4 along N, 32 x 64 each), ONE block per CU with a
//      double-buffered LDS image (2 x 62 KB): chunk c+1 is loaded, split and written into the
//      other buffer between chunk c's taps; one barrier per chunk.
//   LDS image: three part planes (hi, mid, lo) of [halo pixel][16 channels] bf16; halo pixel
//      hp = r * (W + 16) + (x + 1) for halo row r (flattened row Rf + r of the N axis) and column
//      x in [-1, W]: columns -1 and W (the zero padding) and three zero pixels after the image
//      are written once.  The two 16-byte halves of a pixel are swapped when bit 3 of hp is set:
//      the 16-lane phases of the fragment reads (ds_read_b128, consecutive pixels) then cover 16
//      distinct 16-byte bank groups -- also across a row wrap, because the row pitch W + 16 keeps
//      hp mod 16 continuous from a row's last pixel to the next row's first (a simulation of
//      every bench-shape read: 0.006-0.07 extra LDS cycles per 16-lane phase for W >= 26, where
//      the pitch W + 2 gave 0.23-0.9).
//   Rows: a tap that leaves its image (y + dy outside [0, H)) reads a zero pixel instead (per
//      lane: three row bases per pixel subtile, fixed for the block).
//   A (weights): the pre-split layout 2 of conv_px3 ([K/16][3][Mpad][16] bf16, K tap-major),
//      one 16-byte fragment per part straight from L2, two taps ahead (3-deep register ring).
//   Staging: each thread owns ITEMS halo pixels and loads their 16 channels (lanes = consecutive
//      pixels: coalesced), issued in slices behind the first taps' A loads and split + written
//      behind the later taps, so loads have >= 1 tap of MFMAs to land in.
//   Split-K: blockIdx.z takes a.hx_cper channel chunks; slabs and epilogue as conv_px3.
// ---------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t hx_swz(uint32_t off) { return off ^ ((off >> 4) & 16u); }

// DBG (timing experiments only; results wrong): bit 0 = no A loads, bit 1 = no staging loads /
// LDS image writes, bit 2 = no MFMAs.  Only DBG = 0 is in the library; a -DMD2_TIMING_VARIANTS=1
// build of this unit (tools/build_variant.sh) adds the variants of halo_launch, selected there
// by MD2_TUNING=1 MD2_HX_DBG=k
// RFL (forward only): NNlib pad_reflect(x, 1) + valid conv (the DepthDecoder blocks,
// src/depth_decoder.jl:5): a tap leaving the image reads the mirrored row / column (y = -1 -> 1,
// y = H -> H - 2; likewise x) -- per-lane row bases and column offsets, no extra staging.
// Concat input (forward, TensorIn p1): chunks past c0 channels come from the second tensor.
// EXT (dgrad only): the reflect-padded conv's data gradient, first half -- the "full" adjoint
// dxp[p] = sum_tap W[tap] dY[p - tap] over the PADDED (H + 2) x (W + 2) grid, i.e. this kernel on
// the zero-ring-padded dY: a.H / a.W are the padded extents, a.Ho / a.Wo dY's own; staged pixel
// (Y, X) of the padded grid reads dY (Y - 1, X - 1) or zero.  conv_fold_reflect folds the ring
// back (pad_reflect's adjoint).
template <int MODE, int NT, int ITEMS, int DBG = 0, int RFL = 0, int EXT = 0>
__global__ __launch_bounds__(512, 1) void conv_halo3_kernel(ConvArgs a) {
  static_assert(!RFL || MODE == 0, "reflect padding: forward only");
  static_assert(!EXT || MODE == 1, "padded-grid adjoint: dgrad only");
  static_assert(NT == 6 || NT == 9, "split products");
  static_assert(ITEMS == 1 || ITEMS == 2, "staged pixels per thread");
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];   // 2 buffers x 3 part planes

  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wq >> 2, wn = wq & 3;
  const int fi = lane & 31, fh = lane >> 5;
  const int W = a.W, W2 = Halo3Lds::pitch(a.W), H = a.H;   // W2: halo row pitch (pixels)
  const uint32_t N = (uint32_t)a.g.N;
  const uint32_t n0 = blockIdx.x * 256u;
  const int m0 = blockIdx.y * 64;
  const int C = MODE == 0 ? a.Cin : a.Cout;
  const int nch = C >> 4;
  const int cbeg = blockIdx.z * a.hx_cper;
  const int cend = min(nch, cbeg + a.hx_cper);

  // ---- halo geometry (flattened rows R = image * H + y of the N axis)
  const int Rf = (int)fdiv(n0, a.fd_row) - 1;
  const uint32_t nlast = min(n0 + 255u, N - 1u);
  const int HR = (int)fdiv(nlast, a.fd_row) + 2 - Rf;
  const int NH = (int)fdiv(N, a.fd_row);
  const int ZHP = Halo3Lds::zero_px(HR, W);   // zero pixels ZHP .. ZHP + 2

  // zero padding columns and the zero pixels, both buffers, all three parts (never overwritten)
  for (int i = tid; i < 6 * (2 * HR + 3) * 2; i += 512) {
    const int half = i & 1, r = i >> 1;
    const int plane = r % 6, k = r / 6;
    const int hp = k < 2 * HR ? (k >> 1) * W2 + (k & 1) * (W + 1) : ZHP + (k - 2 * HR);
    *reinterpret_cast<u32x4_t*>(lds + plane * HX_PLANE + hp * 32 + half * 16) = u32x4_t{0u, 0u, 0u, 0u};
  }

  // ---- this thread's staged pixels: global offset (OOB outside the tensor) and LDS offset
  const uint32_t img_stride = MODE == 0 ? (uint32_t)a.in.bs0 : (uint32_t)(a.Cout * a.HoWo);
  const uint32_t img_stride1 = MODE == 0 ? (uint32_t)a.in.bs1 : 0u;   // concat: second tensor
  const bool cat = MODE == 0 && a.in.p1 != nullptr && a.in.c0 < a.Cin;
  const uint32_t ch4 = MODE == 0 ? a.HW4 : a.HoWo4;
  uint32_t goff[ITEMS], goff1[ITEMS];
  int loff[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int q = tid + 512 * it;
    goff[it] = goff1[it] = OOB;
    loff[it] = -1;
    if (q < HR * W) {
      const int rr = (int)fdiv((uint32_t)q, a.fd_row);
      const int x = q - rr * W;
      const int R = Rf + rr;
      if (R >= 0 && R < NH) {
        const uint32_t np = (uint32_t)R * (uint32_t)W + (uint32_t)x;
        const uint32_t img = fdiv(np, a.fd_pix);
        if (EXT) {
          const int Y = R - (int)img * H;     // padded-grid row; dY row Y - 1, column x - 1
          if (Y >= 1 && Y <= a.Ho && x >= 1 && x <= a.Wo)
            goff[it] = (img * img_stride + (uint32_t)((Y - 1) * a.Wo + x - 1)) * 4u;
        } else {
          goff[it] = (img * img_stride + (np - img * (uint32_t)a.fd_pix.d)) * 4u;
          goff1[it] = (img * img_stride1 + (np - img * (uint32_t)a.fd_pix.d)) * 4u;
        }
      }
      loff[it] = (int)hx_swz((uint32_t)(rr * W2 + x + 1) * 32u);
    }
  }

  // ---- this lane's B fragment rows: three row bases (dy = -1, 0, +1) per pixel subtile j
  // (reflect: the mirrored row / column; col[dx + 1][j] = the column offset of tap dx)
  int rb[3][2], col[3][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t n = n0 + (uint32_t)(wn * 64 + j * 32 + fi);
    rb[0][j] = rb[1][j] = rb[2][j] = ZHP + 1;
    col[0][j] = -1;
    col[1][j] = 0;
    col[2][j] = 1;
    if (n < N) {
      const uint32_t R = fdiv(n, a.fd_row);
      const int x = (int)(n - R * (uint32_t)W);
      const uint32_t img = fdiv(n, a.fd_pix);
      const int y = (int)(R - img * (uint32_t)H);
      const int c = ((int)R - Rf) * W2 + x + 1;
      rb[1][j] = c;
      if (RFL) {
        rb[0][j] = y > 0 ? c - W2 : c + W2;
        rb[2][j] = y < H - 1 ? c + W2 : c - W2;
        if (x == 0) col[0][j] = 1;
        if (x == W - 1) col[2][j] = -1;
      } else {
        if (y > 0) rb[0][j] = c - W2;
        if (y < H - 1) rb[2][j] = c + W2;
      }
    }
  }

  const __amdgpu_buffer_rsrc_t rA = make_rsrc(a.A, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(MODE == 0 ? (const void*)a.in.p0 : (const void*)a.dy, a.b0_bytes);
  const __amdgpu_buffer_rsrc_t rB1 = make_rsrc(cat ? (const void*)a.in.p1 : (const void*)a.in.p0, cat ? a.b1_bytes : a.b0_bytes);
  const int c0ch = cat ? a.in.c0 >> 4 : 1 << 30;     // first chunk of the second tensor
  const uint32_t apart = (uint32_t)a.g.Mpad * 32u;
  const uint32_t achunk = 3u * apart;
  const uint32_t aoff = (uint32_t)(((m0 + wm * 32 + fi) * 16 + 8 * fh) * 2);

  float stg[ITEMS][16];
  u32x4_t af[3][3];                        // A fragments: a 3-deep ring, two taps ahead
  f32x16 acc0[2], acc1[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[j][r] = acc1[j][r] = 0.f;

  // the chunk's ITEMS x 16 staged values in four slices s = 0..3.  No condition on the loads
  // (a runtime select makes hipcc branch around each load and drain vmcnt): past the last chunk
  // they read the next channels / the next image (discarded) or, past the tensor, zeros (OOB)
  auto stage_slice = [&](int s, int cc) {
    constexpr int PER = ITEMS * 4;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int li = s * PER + u, it = li >> 4, ch = li & 15;
      // (wave-uniform choice of the concat half: resource and soffset are scalar selects)
      const bool sec = cc >= c0ch;
      stg[it][ch] = (DBG & 2) ? (float)(cc + ch)
                              : bload_s(sec ? rB1 : rB, sec ? goff1[it] : goff[it],
                                        (uint32_t)((sec ? cc - c0ch : cc) * 16 + ch) * ch4);
    }
  };
  // split item `it` into the three part planes of buffer `buf`
  auto stage_write = [&](int it, int buf) {
    if (loff[it] < 0 || (DBG & 2)) return;
    uint32_t hm[3][8];
#pragma unroll
    for (int p = 0; p < 8; ++p) split3_pk(stg[it][2 * p], stg[it][2 * p + 1], hm[0][p], hm[1][p], hm[2][p]);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      uint8_t* dst = lds + (buf * 3 + q) * HX_PLANE;
      *reinterpret_cast<u32x4_t*>(dst + loff[it]) = u32x4_t{hm[q][0], hm[q][1], hm[q][2], hm[q][3]};
      *reinterpret_cast<u32x4_t*>(dst + (loff[it] ^ 16)) = u32x4_t{hm[q][4], hm[q][5], hm[q][6], hm[q][7]};
    }
  };
  // tap 9 (or 10) of chunk cc = tap 0 (1) of chunk cc + 1 (read whatever it is past the end)
  auto load_a = [&](int tap, int cc) {
    if (tap >= 9) {
      tap -= 9;
      ++cc;
    }
    const uint32_t base = (uint32_t)(tap * nch + cc) * achunk + aoff;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      af[tap % 3][q] = (DBG & 1) ? u32x4_t{base, base + 1, base + 2, (uint32_t)q} : bload16(rA, base + (uint32_t)q * apart);
  };

  // prologue: chunk cbeg staged into buffer 0
  if (cbeg < cend) {
#pragma unroll
    for (int s = 0; s < 4; ++s) stage_slice(s, cbeg);
    load_a(0, cbeg);
    load_a(1, cbeg);
    __syncthreads();                       // zero fill done before the first image writes
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) stage_write(it, 0);
  }
  __syncthreads();
  // B fragments of one tap (both pixel subtiles, three parts), double-buffered by tap parity:
  // tap t+1's LDS reads are issued before tap t's MFMAs
  u32x4_t fb[2][2][3];
  auto read_b = [&](int set, const uint8_t* img, int tap) {
    const int kh = tap / 3, kw = tap - 3 * kh;
    const int dyi = MODE == 0 ? kh : 2 - kh;          // index of the row base (dy + 1)
    const int dx = MODE == 0 ? kw - 1 : 1 - kw;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t off = hx_swz((uint32_t)(rb[dyi][j] + col[dx + 1][j]) * 32u + 16u * (uint32_t)fh);
#pragma unroll
      for (int q = 0; q < 3; ++q) fb[set][j][q] = *reinterpret_cast<const u32x4_t*>(img + q * HX_PLANE + off);
    }
  };
  for (int cc = cbeg; cc < cend; ++cc) {
    const int cur = (cc - cbeg) & 1;
    const bool more = cc + 1 < cend;
    const uint8_t* img = lds + cur * 3 * HX_PLANE;
    read_b(0, img, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      // issue order pinned (sched_barrier): A two taps ahead, a slice of the next chunk's
      // staging (waiting for A(t) never waits for a staging load younger than tap t - 3), and
      // the next tap's B fragments from LDS
      load_a(tap + 2, cc);
      if (tap < 4) stage_slice(tap, cc + 1);           // next chunk: loads behind taps 0..3
      if (tap < 8) read_b((tap + 1) & 1, img, tap + 1);
      __builtin_amdgcn_sched_barrier(0);
      // ... split + written into the other buffer behind taps 5 (item 0) and 7 (item 1)
      if (tap == 5 && more) stage_write(0, cur ^ 1);
      if (ITEMS == 2 && tap == 7 && more) stage_write(ITEMS - 1, cur ^ 1);
      const u32x4_t* fa = af[tap % 3];
      const bf16x8_t ah = __builtin_bit_cast(bf16x8_t, fa[0]);
      const bf16x8_t am = __builtin_bit_cast(bf16x8_t, fa[1]);
      const bf16x8_t al = __builtin_bit_cast(bf16x8_t, fa[2]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, fb[tap & 1][j][0]);
        const bf16x8_t bm = __builtin_bit_cast(bf16x8_t, fb[tap & 1][j][1]);
        const bf16x8_t bl = __builtin_bit_cast(bf16x8_t, fb[tap & 1][j][2]);
        if constexpr ((DBG & 4) != 0) {
          acc1[j][0] += __builtin_bit_cast(float, fb[tap & 1][j][0][0]) * __builtin_bit_cast(float, fa[0][0]);
          acc0[j][0] += __builtin_bit_cast(float, fb[tap & 1][j][1][1]) + __builtin_bit_cast(float, fb[tap & 1][j][2][2]) + __builtin_bit_cast(float, fa[1][1] ^ fa[2][2]);
          continue;
        }
        f32x16 c = acc1[j];
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
        acc1[j] = c;
        acc0[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc0[j], 0, 0, 0);
      }
    }
    __syncthreads();                       // the other buffer is complete; this one is free
  }

  // ---- BatchNorm statistics of this tile (forward without split-K, a.bn_part): the 64 x 256
  // outputs -- the values stored below -- through LDS (the image buffers are free after the last
  // barrier), 8 threads per channel summing 32 pixels each in fp64, then the 8 partial sums in a
  // fixed shuffle order; one partial per (channel, tile): part[m][blockIdx.x][2]
  if constexpr (MODE == 0 && !RFL && !EXT) {
    if (a.bn_part) {                       // block-uniform
      constexpr int TP = 257;              // LDS row pitch (floats)
      static_assert(64 * TP * 4 <= Halo3Lds::cap, "the statistics tile overlays the image buffers");
      float* t = reinterpret_cast<float*>(lds);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t nl = (uint32_t)(wn * 64 + j * 32 + fi);
        const bool v = n0 + nl < N;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          t[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh) * TP + nl] = v ? acc0[j][r] + acc1[j][r] : 0.f;
      }
      __syncthreads();
      const int m = tid >> 3, g8 = tid & 7;
      double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
      for (int k = 0; k < 32; ++k) {
        const double v = (double)t[m * TP + g8 * 32 + k];
        s1 += v;
        s2 += v * v;
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
      }
      if (g8 == 0) {
        double* q = a.bn_part + ((long)(m0 + m) * gridDim.x + blockIdx.x) * 2;
        q[0] = s1;
        q[1] = s2;
      }
    }
  }

  // ---- epilogue (accumulator layout of conv_px3: TM = 1, TN = 2)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long nn = (long)n0 + wn * 64 + j * 32 + fi;
    if (nn >= a.g.N) continue;
    if (a.slab) {
      float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        sl[(long)m * a.g.N + nn] = acc0[j][r] + acc1[j][r];
      }
    } else {
      int img;
      long pix, plane;
      out_pixel(a, false, nn, img, pix, plane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        store_out(a.out, m, img, pix, plane, acc0[j][r] + acc1[j][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// stride-2 3x3 (pad 1) data gradient on the LDS halo (round 6).  dX pixel (2y + py, 2x + px)
// receives only the taps whose parity matches (py, px) -- kh = 1 for py = 0, kh in {0, 2} for
// py = 1 (likewise kw) -- each reading dY at (y + dy, x + dx) with dy = (py + 1 - kh) / 2 in
// {0, 1}.  So over the dY grid point (y, x) the four output-parity classes of dX are four
// accumulators fed by the SAME staged dY image: the nine taps of a 16-channel chunk are one tap
// set of the stride-1 kernel (conv_halo3_kernel MODE 1, whose staging, A ring, issue pinning and
// hx_swz layout this follows), each tap adding into its class's accumulator.  conv_px3's parity
// classes gather each dY value once per tap of a class and synchronise after every 6 MFMAs.
//   Block: 64 input channels (M) x 128 dY grid points (N order = image, row, column), 8 waves
//      (2 along M x 4 along N, 32 x 32 each) with one accumulator per class (64 registers; the
//      hi x hi product in the same chain -- a second set per class spilled at 2 waves / SIMD).
//   LDS: 2 buffers x 3 parts of HS2_PX = 416 halo pixels (80 KB, not conv_halo3's 141 KB: the
//      stride-2 dgrad runs beside side-stream kernels, which then still find LDS on its CU).
//   Epilogue: class (py, px) of point (img, y, x) -> dX (img, 2y + py, 2x + px) (H = 2 Ho,
//      W = 2 Wo), stored or written to the split-K slab [split][Cin][N * H * W].
// ---------------------------------------------------------------------------------------------
template <int ITEMS>
__global__ __launch_bounds__(512, 1) void conv_halo3s2_kernel(ConvArgs a) {
  static_assert(ITEMS == 1 || ITEMS == 2, "staged pixels per thread");
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wq >> 2, wn = wq & 3;
  const int fi = lane & 31, fh = lane >> 5;
  const int W = a.Wo, W2 = Halo3s2Lds::pitch(a.Wo), H = a.Ho;   // the dY grid (staged and iterated)
  const uint32_t N = (uint32_t)a.g.N;                  // dY grid points
  const uint32_t n0 = blockIdx.x * 128u;
  const int m0 = blockIdx.y * 64;
  const int nch = a.Cout >> 4;
  const int cbeg = blockIdx.z * a.hx_cper;
  const int cend = min(nch, cbeg + a.hx_cper);

  const int Rf = (int)fdiv(n0, a.fd_row) - 1;
  const uint32_t nlast = min(n0 + 127u, N - 1u);
  const int HR = (int)fdiv(nlast, a.fd_row) + 2 - Rf;
  const int NH = (int)fdiv(N, a.fd_row);
  const int ZHP = Halo3s2Lds::zero_px(HR, W);

  for (int i = tid; i < 6 * (2 * HR + 3) * 2; i += 512) {
    const int half = i & 1, r = i >> 1;
    const int plane = r % 6, k = r / 6;
    const int hp = k < 2 * HR ? (k >> 1) * W2 + (k & 1) * (W + 1) : ZHP + (k - 2 * HR);
    *reinterpret_cast<u32x4_t*>(lds + plane * HS2_PLANE + hp * 32 + half * 16) = u32x4_t{0u, 0u, 0u, 0u};
  }

  const uint32_t img_stride = (uint32_t)(a.Cout * a.HoWo);
  const uint32_t ch4 = a.HoWo4;
  uint32_t goff[ITEMS];
  int loff[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int q = tid + 512 * it;
    goff[it] = OOB;
    loff[it] = -1;
    if (q < HR * W) {
      const int rr = (int)fdiv((uint32_t)q, a.fd_row);
      const int x = q - rr * W;
      const int R = Rf + rr;
      if (R >= 0 && R < NH) {
        const uint32_t np = (uint32_t)R * (uint32_t)W + (uint32_t)x;
        const uint32_t img = fdiv(np, a.fd_pix);
        goff[it] = (img * img_stride + (np - img * (uint32_t)a.fd_pix.d)) * 4u;
      }
      loff[it] = (int)hx_swz((uint32_t)(rr * W2 + x + 1) * 32u);
    }
  }

  // this lane's B fragment: the point's own row base and the row below (or a zero pixel)
  int rb0, rb1;
  {
    const uint32_t n = n0 + (uint32_t)(wn * 32 + fi);
    rb0 = rb1 = ZHP + 1;
    if (n < N) {
      const uint32_t R = fdiv(n, a.fd_row);
      const int x = (int)(n - R * (uint32_t)W);
      const uint32_t img = fdiv(n, a.fd_pix);
      const int y = (int)(R - img * (uint32_t)H);
      rb0 = ((int)R - Rf) * W2 + x + 1;
      if (y < H - 1) rb1 = rb0 + W2;
    }
  }

  const __amdgpu_buffer_rsrc_t rA = make_rsrc(a.A, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rB = make_rsrc((const void*)a.dy, a.b0_bytes);
  const uint32_t apart = (uint32_t)a.g.Mpad * 32u;
  const uint32_t achunk = 3u * apart;
  const uint32_t aoff = (uint32_t)(((m0 + wm * 32 + fi) * 16 + 8 * fh) * 2);

  float stg[ITEMS][16];
  u32x4_t af[3][3];
  f32x16 acc[4];                           // per output-parity class (py * 2 + px)
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  auto stage_slice = [&](int s, int cc) {
    constexpr int PER = ITEMS * 4;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int li = s * PER + u, it = li >> 4, ch = li & 15;
      stg[it][ch] = bload_s(rB, goff[it], (uint32_t)(cc * 16 + ch) * ch4);
    }
  };
  auto stage_write = [&](int it, int buf) {
    if (loff[it] < 0) return;
    uint32_t hm[3][8];
#pragma unroll
    for (int p = 0; p < 8; ++p) split3_pk(stg[it][2 * p], stg[it][2 * p + 1], hm[0][p], hm[1][p], hm[2][p]);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      uint8_t* dst = lds + (buf * 3 + q) * HS2_PLANE;
      *reinterpret_cast<u32x4_t*>(dst + loff[it]) = u32x4_t{hm[q][0], hm[q][1], hm[q][2], hm[q][3]};
      *reinterpret_cast<u32x4_t*>(dst + (loff[it] ^ 16)) = u32x4_t{hm[q][4], hm[q][5], hm[q][6], hm[q][7]};
    }
  };
  auto load_a = [&](int tap, int cc) {
    if (tap >= 9) {
      tap -= 9;
      ++cc;
    }
    const uint32_t base = (uint32_t)(tap * nch + cc) * achunk + aoff;
#pragma unroll
    for (int q = 0; q < 3; ++q) af[tap % 3][q] = bload16(rA, base + (uint32_t)q * apart);
  };

  if (cbeg < cend) {
#pragma unroll
    for (int s = 0; s < 4; ++s) stage_slice(s, cbeg);
    load_a(0, cbeg);
    load_a(1, cbeg);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) stage_write(it, 0);
  }
  __syncthreads();
  u32x4_t fb[2][3];
  // tap (kh, kw): dY offset dy = (py + 1 - kh) / 2 with py = (kh != 1); likewise dx
  auto read_b = [&](int set, const uint8_t* img_l, int tap) {
    const int kh = tap / 3, kw = tap - 3 * kh;
    const int dy = kh == 0 ? 1 : 0, dx = kw == 0 ? 1 : 0;
    const uint32_t off = hx_swz((uint32_t)((dy ? rb1 : rb0) + dx) * 32u + 16u * (uint32_t)fh);
#pragma unroll
    for (int q = 0; q < 3; ++q) fb[set][q] = *reinterpret_cast<const u32x4_t*>(img_l + q * HS2_PLANE + off);
  };
  for (int cc = cbeg; cc < cend; ++cc) {
    const int cur = (cc - cbeg) & 1;
    const bool more = cc + 1 < cend;
    const uint8_t* img_l = lds + cur * 3 * HS2_PLANE;
    read_b(0, img_l, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      load_a(tap + 2, cc);
      if (tap < 4) stage_slice(tap, cc + 1);
      if (tap < 8) read_b((tap + 1) & 1, img_l, tap + 1);
      __builtin_amdgcn_sched_barrier(0);
      if (tap == 5 && more) stage_write(0, cur ^ 1);
      if (ITEMS == 2 && tap == 7 && more) stage_write(ITEMS - 1, cur ^ 1);
      const int kh = tap / 3, kw = tap - 3 * kh;
      const int cls = (kh != 1) * 2 + (kw != 1);
      const u32x4_t* fa = af[tap % 3];
      const bf16x8_t ah = __builtin_bit_cast(bf16x8_t, fa[0]);
      const bf16x8_t am = __builtin_bit_cast(bf16x8_t, fa[1]);
      const bf16x8_t al = __builtin_bit_cast(bf16x8_t, fa[2]);
      const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, fb[tap & 1][0]);
      const bf16x8_t bm = __builtin_bit_cast(bf16x8_t, fb[tap & 1][1]);
      const bf16x8_t bl = __builtin_bit_cast(bf16x8_t, fb[tap & 1][2]);
      f32x16 c = acc[cls];
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
      acc[cls] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: class (py, px) of point (img, y, x) -> dX (img, 2y + py, 2x + px)
  const uint32_t n = n0 + (uint32_t)(wn * 32 + fi);
  if (n >= N) return;
  const uint32_t img = fdiv(n, a.fd_pix);
  const uint32_t r = n - img * (uint32_t)a.fd_pix.d;
  const uint32_t y = fdiv(r, a.fd_row), x = r - y * (uint32_t)W;
  const long HWd = a.HW;
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const long pix = (long)(2 * y + (cls >> 1)) * a.W + 2 * x + (cls & 1);
    if (a.slab) {
      float* sl = a.slab + (long)blockIdx.z * a.g.M * (4L * a.g.N) + (long)img * HWd + pix;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = m0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh;
        sl[(long)m * (4L * a.g.N)] = acc[cls][q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = m0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh;
        store_out(a.out, m, (int)img, pix, HWd, acc[cls][q]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 2D-tile form of conv_halo3 (round 6): the decoder's maps too wide for the flattened halo image
// (64 x 208: a 256-pixel run of rows needs 5 halo rows of 224 pixels) and its 32-row M tiles
// (Cout = 32 forwards, Cin = 96 data gradients).  A block owns 32 MW output channels x an
// 8-row x 32-column pixel tile of one image; per 16-channel chunk it stages the 10 x 34 halo
// (zero, reflect or -- EXT -- the zero-ring-padded dY) as [pixel][16 channels] x 3 bf16 parts,
// each value loaded and split once; a wave's 32-pixel fragment is ONE tile row, so with the
// bit-3 half swap every 16-lane ds_read_b128 phase hits 16 distinct bank groups for any row pitch
// (simulated).  Reflect padding is resolved in the staging (the halo holds the mirrored pixels).
//   MW = 1: 4 waves (one M tile x 4 row pairs), two blocks per CU; MW = 2: 8 waves, one per CU.
//   (Tile and plane sizes H2_*: conv_lds.h.)
// ---------------------------------------------------------------------------------------------
template <int MODE, int MW, int RFL = 0, int EXT = 0>
__global__ __launch_bounds__(256 * MW, 2 / MW) void conv_halo2d_kernel(ConvArgs a) {
  static_assert(!RFL || MODE == 0, "reflect padding: forward only");
  static_assert(!EXT || MODE == 1, "padded-grid adjoint: dgrad only");
  constexpr int NTH = 256 * MW;
  constexpr int ITEMS = (H2_PX + NTH - 1) / NTH;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];   // 2 buffers x 3 part planes

  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wq >> 2, wn = wq & 3;
  const int fi = lane & 31, fh = lane >> 5;
  const int W = a.W, H = a.H;                         // output grid (EXT: the padded grid)
  const int tx_n = (W + H2_TW - 1) / H2_TW, ty_n = (H + H2_TH - 1) / H2_TH;
  const uint32_t bt = blockIdx.x;
  const uint32_t img = bt / (uint32_t)(tx_n * ty_n);
  const int trem = (int)(bt - img * (uint32_t)(tx_n * ty_n));
  const int ty = trem / tx_n, tx = trem - ty * tx_n;
  const int y0 = ty * H2_TH, x0 = tx * H2_TW;
  const int m0 = blockIdx.y * 32 * MW;
  const int C = MODE == 0 ? a.Cin : a.Cout;
  const int nch = C >> 4;
  const int cbeg = blockIdx.z * a.hx_cper;
  const int cend = min(nch, cbeg + a.hx_cper);

  // ---- staged halo pixel (hr, hc) -> source pixel of image img (or OOB)
  const uint32_t img_stride = MODE == 0 ? (uint32_t)a.in.bs0 : (uint32_t)(a.Cout * a.HoWo);
  const uint32_t img_stride1 = MODE == 0 ? (uint32_t)a.in.bs1 : 0u;
  const bool cat = MODE == 0 && a.in.p1 != nullptr && a.in.c0 < a.Cin;
  const uint32_t ch4 = MODE == 0 ? a.HW4 : a.HoWo4;
  uint32_t goff[ITEMS], goff1[ITEMS];
  int loff[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int q = tid + NTH * it;
    goff[it] = goff1[it] = OOB;
    loff[it] = -1;
    if (q < H2_PX) {
      const int hr = q / H2_PR, hc = q - hr * H2_PR;
      int y = y0 + hr - 1, x = x0 + hc - 1;
      if (RFL) {                           // NNlib pad_reflect(x, 1): -1 -> 1, H -> H - 2
        y = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y);
        x = x < 0 ? -x : (x >= W ? 2 * W - 2 - x : x);
      }
      if (EXT) {                           // padded-grid pixel (y, x) reads dY (y - 1, x - 1)
        if (y >= 1 && y <= a.Ho && x >= 1 && x <= a.Wo)
          goff[it] = (img * img_stride + (uint32_t)((y - 1) * a.Wo + x - 1)) * 4u;
      } else if (y >= 0 && y < H && x >= 0 && x < W) {
        const uint32_t pix = (uint32_t)(y * W + x);
        goff[it] = (img * img_stride + pix) * 4u;
        goff1[it] = (img * img_stride1 + pix) * 4u;
      }
      loff[it] = (int)hx_swz((uint32_t)q * 32u);
    }
  }

  const __amdgpu_buffer_rsrc_t rA = make_rsrc(a.A, a.A_bytes);
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(MODE == 0 ? (const void*)a.in.p0 : (const void*)a.dy, a.b0_bytes);
  const __amdgpu_buffer_rsrc_t rB1 = make_rsrc(cat ? (const void*)a.in.p1 : (const void*)a.in.p0, cat ? a.b1_bytes : a.b0_bytes);
  const int c0ch = cat ? a.in.c0 >> 4 : 1 << 30;
  const uint32_t apart = (uint32_t)a.g.Mpad * 32u;
  const uint32_t achunk = 3u * apart;
  const uint32_t aoff = (uint32_t)(((m0 + wm * 32 + fi) * 16 + 8 * fh) * 2);

  float stg[ITEMS][16];
  u32x4_t af[3][3];
  f32x16 acc0[2], acc1[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[j][r] = acc1[j][r] = 0.f;

  auto stage_slice = [&](int s, int cc) {
    constexpr int PER = ITEMS * 4;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int li = s * PER + u, it = li >> 4, ch = li & 15;
      const bool sec = cc >= c0ch;
      stg[it][ch] = bload_s(sec ? rB1 : rB, sec ? goff1[it] : goff[it],
                            (uint32_t)((sec ? cc - c0ch : cc) * 16 + ch) * ch4);
    }
  };
  auto stage_write = [&](int it, int buf) {
    if (loff[it] < 0) return;
    uint32_t hm[3][8];
#pragma unroll
    for (int p = 0; p < 8; ++p) split3_pk(stg[it][2 * p], stg[it][2 * p + 1], hm[0][p], hm[1][p], hm[2][p]);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      uint8_t* dst = lds + (buf * 3 + q) * H2_PLANE;
      *reinterpret_cast<u32x4_t*>(dst + loff[it]) = u32x4_t{hm[q][0], hm[q][1], hm[q][2], hm[q][3]};
      *reinterpret_cast<u32x4_t*>(dst + (loff[it] ^ 16)) = u32x4_t{hm[q][4], hm[q][5], hm[q][6], hm[q][7]};
    }
  };
  auto load_a = [&](int tap, int cc) {
    if (tap >= 9) {
      tap -= 9;
      ++cc;
    }
    const uint32_t base = (uint32_t)(tap * nch + cc) * achunk + aoff;
#pragma unroll
    for (int q = 0; q < 3; ++q) af[tap % 3][q] = bload16(rA, base + (uint32_t)q * apart);
  };

  if (cbeg < cend) {
#pragma unroll
    for (int s = 0; s < 4; ++s) stage_slice(s, cbeg);
    load_a(0, cbeg);
    load_a(1, cbeg);
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) stage_write(it, 0);
  }
  __syncthreads();
  // this lane's fragment pixels: tile row 2 wn + j, column fi; halo record of tap (dy, dx)
  // = (row + 1 + dy) * PR + (fi + 1 + dx)
  const int rowb = (2 * wn + 1) * H2_PR + fi + 1;
  u32x4_t fb[2][2][3];
  auto read_b = [&](int set, const uint8_t* img_l, int tap) {
    const int kh = tap / 3, kw = tap - 3 * kh;
    const int dy = MODE == 0 ? kh - 1 : 1 - kh;
    const int dx = MODE == 0 ? kw - 1 : 1 - kw;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t off = hx_swz((uint32_t)(rowb + (j + dy) * H2_PR + dx) * 32u + 16u * (uint32_t)fh);
#pragma unroll
      for (int q = 0; q < 3; ++q) fb[set][j][q] = *reinterpret_cast<const u32x4_t*>(img_l + q * H2_PLANE + off);
    }
  };
  for (int cc = cbeg; cc < cend; ++cc) {
    const int cur = (cc - cbeg) & 1;
    const bool more = cc + 1 < cend;
    const uint8_t* img_l = lds + cur * 3 * H2_PLANE;
    read_b(0, img_l, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      load_a(tap + 2, cc);
      if (tap < 4) stage_slice(tap, cc + 1);
      if (tap < 8) read_b((tap + 1) & 1, img_l, tap + 1);
      __builtin_amdgcn_sched_barrier(0);
      if (tap == 5 && more) stage_write(0, cur ^ 1);
      if (ITEMS == 2 && tap == 7 && more) stage_write(ITEMS - 1, cur ^ 1);
      const u32x4_t* fa = af[tap % 3];
      const bf16x8_t ah = __builtin_bit_cast(bf16x8_t, fa[0]);
      const bf16x8_t am = __builtin_bit_cast(bf16x8_t, fa[1]);
      const bf16x8_t al = __builtin_bit_cast(bf16x8_t, fa[2]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, fb[tap & 1][j][0]);
        const bf16x8_t bm = __builtin_bit_cast(bf16x8_t, fb[tap & 1][j][1]);
        const bf16x8_t bl = __builtin_bit_cast(bf16x8_t, fb[tap & 1][j][2]);
        f32x16 c = acc1[j];
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
        acc1[j] = c;
        acc0[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc0[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- epilogue (accumulator layout of conv_px3: TM = 1, TN = 2): pixel (y0 + 2 wn + j, x0 + fi)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + 2 * wn + j, x = x0 + fi;
    if (y >= H || x >= W) continue;
    const long nn = (long)img * H * W + (long)y * W + x;
    if (a.slab) {
      float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        sl[(long)m * a.g.N + nn] = acc0[j][r] + acc1[j][r];
      }
    } else {
      int oimg;
      long pix, plane;
      out_pixel(a, false, nn, oimg, pix, plane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        store_out(a.out, m, oimg, pix, plane, acc0[j][r] + acc1[j][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Filter gradient of the stride-1 3x3 zero-padded convs on the LDS halo (bf16x6 split products).
//   dW[m][tap * Cin + c] = sum_p dY[m][p] * X[c][p + (kh - 1, kw - 1)],  K = every output pixel
// conv_wgrad_px3 stages the X operand once per (tap, pixel chunk): every input value is loaded
// and split nine times.  Here a block owns 64 filters (m) x 32 input channels (c) x ALL nine
// taps, and walks K by CHUNKS of r whole image rows (r * W <= 112 pixels, 16-pixel k-steps):
//   X    the chunk's rows plus one halo row above and below, staged ONCE per chunk as an LDS image
//        [halo pixel][32 channels] x 3 bf16 parts (channels contiguous: 64 B per pixel); the B
//        fragment of tap (dy, dx) -- 8 consecutive k (pixels) of one channel per lane -- is read
//        with ds_read_b64_tr_b16 (4 pixel rows x 16 channels per 16-lane group, delivered
//        column-major), so ANY pixel shift is an 8-byte-aligned row address: no per-tap copies;
//        a tap leaving the image reads a zero pixel (per-lane row validity);
//   dY   A fragments straight from global (8 consecutive pixels of one filter's row per lane, two
//        16-byte loads, one k-step ahead) and split in registers;
//   waves  6 = 2 filter halves x 3 kernel rows (kh); a wave's 3 taps (kw = 0..2) share its A
//        fragment; ONE accumulator per tap (the MFMA sums its 16 products and C at full precision
//        and rounds once -- profiles/r05_mfma_rounding.txt -- so 6 roundings per 16 pixels, fewer
//        than a sequential fp32 chain's 16);
//   K split over blocks (blockIdx.z: a.hx_cper chunks each) into the slabs [split][Cout][9 Cin]
//   of the other wgrad kernels (tap-major columns), finalised by wgrad_reduce_kernel.
// Two blocks per CU (<= 64 KB LDS, <= 168 VGPRs): one stages while the other computes.
// ---------------------------------------------------------------------------------------------
typedef short hx_v4s __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint2 hx_tr16(const uint8_t* p) {
  const hx_v4s v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) hx_v4s*)p);
  return __builtin_bit_cast(uint2, v);
}

// DBG (timing experiments only; results wrong): bit 0 = no dY loads, bit 1 = no X staging loads /
// LDS writes, bit 2 = no MFMAs, bit 3 = no B-fragment LDS reads.  Only DBG = 0 is in the library;
// a -DMD2_TIMING_VARIANTS=1 build of this unit (tools/build_variant.sh) adds the variants of
// whalo_launch, selected there by MD2_TUNING=1 MD2_WHX_DBG=k
template <int ITEMS, int KS, int DBG = 0>
__global__ __launch_bounds__(384, 3) void conv_whalo_kernel(ConvArgs a) {   // 3 waves per SIMD: two 6-wave blocks per CU (<= 168 VGPRs)
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mh = wq & 1, dyi = wq >> 1;               // filter half, kernel row kh = dyi
  const int W = a.W, H = a.H, P = WHaloLds::pitch(W); // halo row pitch (pixels)
  const int r = a.hx_r, rW = r * W;                   // rows per chunk, pixels per chunk
  static_assert(KS >= 4, "the X staging rides in 4 slices behind the first k-steps");
  static_assert(KS <= WHaloLds::KS_MAX, "the k table holds 16 KS_MAX words");
  const int c0 = blockIdx.x * 32, m0 = blockIdx.y * 64;
  const int cbeg = blockIdx.z * a.hx_cper, cend = min(a.hx_nchunk, cbeg + a.hx_cper);
  const int HR = r + 2, ZHP = WHaloLds::zero_px(r, W);   // zero pixels ZHP .. ZHP + 2
  const int plane = WHaloLds::plane(ZHP);             // bytes per part plane
  const uint32_t HW = (uint32_t)H * (uint32_t)W;

  // zero padding columns (x = -1, W) of every halo row and the zero pixels, 3 parts, 4 x 16 B
  for (int i = tid; i < 3 * (2 * HR + 3) * 4; i += 384) {
    const int quarter = i & 3, rr = i >> 2;
    const int part = rr % 3, k = rr / 3;
    const int hp = k < 2 * HR ? (k >> 1) * P + (k & 1) * (W + 1) : ZHP + (k - 2 * HR);
    *reinterpret_cast<u32x4_t*>(lds + part * plane + hp * 64 + quarter * 16) = u32x4_t{0u, 0u, 0u, 0u};
  }

  // chunk pixel k -> (row rr << 16 | halo pixel of (rr, x) for dy = 0), all-ones past the chunk
  uint32_t* ktab = reinterpret_cast<uint32_t*>(lds + WHaloLds::ktab(plane));
  for (int k = tid; k < 16 * KS; k += 384) {
    uint32_t v = 0xffffffffu;
    if (k < rW) {
      const int rr = (int)fdiv((uint32_t)k, a.fd_row);
      v = ((uint32_t)rr << 16) | (uint32_t)((rr + 1) * P + (k - rr * W) + 1);
    }
    ktab[k] = v;
  }

  // ---- X staging slots: slot = octet * npix + q (lanes = consecutive pixels of one channel)
  const int npix = HR * W;
  int sq_hr[ITEMS], sq_lo[ITEMS];                     // halo row, LDS byte offset (part 0)
  uint32_t sq_px[ITEMS];                              // pixel offset inside the image plane
  int sq_oct[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int slot = tid + 384 * it;
    sq_lo[it] = -1;
    sq_hr[it] = 0;
    sq_px[it] = 0;
    sq_oct[it] = 0;
    if (slot < 4 * npix) {
      const int o = slot / npix, q = slot - o * npix;
      const int hr = (int)fdiv((uint32_t)q, a.fd_row);
      const int x = q - hr * W;
      sq_oct[it] = o;
      sq_hr[it] = hr;
      sq_px[it] = (uint32_t)((hr - 1) * W + x);        // relative to the chunk's first row
      sq_lo[it] = (hr * P + x + 1) * 64 + o * 16;
    }
  }
  const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.in.p0, a.b0_bytes);
  const __amdgpu_buffer_rsrc_t rY = make_rsrc(a.dy, a.A_bytes);
  const uint32_t ximg = (uint32_t)a.in.bs0;           // X image stride (floats)
  const uint32_t yimg = (uint32_t)a.Cout * HW;        // dY image stride

  float stg[ITEMS][8];
  // chunk q: image img = (q * r) / H, first row y0 = (q * r) % H
  auto chunk_geo = [&](int q, uint32_t& img, int& y0) {
    const uint32_t R0 = (uint32_t)(q * r);
    img = R0 / (uint32_t)H;
    y0 = (int)(R0 - img * (uint32_t)H);
  };
  // the next chunk's X in 4 slices (2 * ITEMS loads each), issued behind k-steps 0..3 so that
  // waiting for an A fragment never waits for a staging load issued in the same k-step
  uint32_t sbase[ITEMS];
  auto stage_addr = [&](int q) {
    uint32_t img;
    int y0;
    chunk_geo(min(q, a.hx_nchunk - 1), img, y0);
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int y = y0 + sq_hr[it] - 1;
      const bool ok = sq_lo[it] >= 0 && y >= 0 && y < H;
      // (the lane's channel octet in the voffset: a per-lane soffset would be a waterfall loop)
      sbase[it] = ok ? (img * ximg + (uint32_t)(y0 * W) + sq_px[it] + (uint32_t)(8 * sq_oct[it]) * HW) * 4u : OOB;
    }
  };
  auto stage_slice = [&](int sl) {
#pragma unroll
    for (int u = 0; u < 2 * ITEMS; ++u) {
      const int li = sl * 2 * ITEMS + u, it = li >> 3, e = li & 7;
      stg[it][e] = (DBG & 2) ? (float)(sl + e) : bload_s(rX, sbase[it], (uint32_t)(c0 + e) * a.HW4);
    }
  };
  auto stage_write = [&]() {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      if (sq_lo[it] < 0 || (DBG & 2)) continue;
      uint32_t hm[3][4];
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) split3_pk(stg[it][2 * pp], stg[it][2 * pp + 1], hm[0][pp], hm[1][pp], hm[2][pp]);
#pragma unroll
      for (int part = 0; part < 3; ++part)
        *reinterpret_cast<u32x4_t*>(lds + part * plane + sq_lo[it]) = u32x4_t{hm[part][0], hm[part][1], hm[part][2], hm[part][3]};
    }
  };

  // ---- A fragments (dY): filter row m, pixels k .. k+7 of the chunk (k = 16 j + 8 fh)
  const int fi = lane & 31, fh = lane >> 5;
  const int m = m0 + 32 * mh + fi;
  float anext[8];
  auto load_a = [&](int q, int j) {
    uint32_t img;
    int y0;
    chunk_geo(min(q, a.hx_nchunk - 1), img, y0);
    const int k = 16 * j + 8 * fh;
    const uint32_t base = (img * yimg + (uint32_t)m * HW + (uint32_t)(y0 * W) + (uint32_t)k) * 4u;
    const float4 v0 = (DBG & 1) ? make_float4((float)base, 1.f, 2.f, 3.f) : bload4(rY, k < rW ? base : OOB);
    const float4 v1 = (DBG & 1) ? make_float4(4.f, (float)k, 6.f, 7.f) : bload4(rY, k + 4 < rW ? base + 16u : OOB);
    anext[0] = v0.x; anext[1] = v0.y; anext[2] = v0.z; anext[3] = v0.w;
    anext[4] = v1.x; anext[5] = v1.y; anext[6] = v1.z; anext[7] = v1.w;
  };

  // ---- B fragment rows of this lane (ds_read_b64_tr_b16): group g = lane >> 4 supplies rows
  // k = 8 (g >> 1) + 4 t + qq, columns (channels) 16 (g & 1) + 4 pp .. + 3
  const int g = lane >> 4, qq = (lane >> 2) & 3, pp4 = lane & 3;
  const int cofs = (16 * (g & 1) + 4 * pp4) * 2;
  const int dy = dyi - 1;

  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  if (cbeg < cend) {
    stage_addr(cbeg);
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) stage_slice(sl);
    load_a(cbeg, 0);
  }
  for (int q = cbeg; q < cend; ++q) {
    uint32_t img;
    int y0;
    chunk_geo(q, img, y0);
    __syncthreads();                       // the previous chunk's reads are done
    stage_write();
    __syncthreads();
    stage_addr(q + 1);
    // B rows of this lane for t = 0, 1 at k-step jj (pixel k, its row validity for this wave's
    // dy); the chunk-invariant k -> (row, halo pixel) map is an LDS table, not 28 hoisted VGPRs.
    // Read one k-step ahead (the table read is off the MFMAs' dependency chain).
    auto hp_of = [&](int jj, int (&hp)[2]) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint32_t v = ktab[16 * jj + 8 * (g >> 1) + 4 * t + qq];
        const int rr = (int)(v >> 16);
        const int y = y0 + rr + dy;
        hp[t] = (v != 0xffffffffu && y >= 0 && y < H) ? (int)(v & 0xffffu) + dy * P : ZHP + 1;
      }
    };
    // the three part fragments of tap kw (ds_read_b64_tr_b16 pairs)
    auto read_b = [&](int kw, const int (&hp)[2], u32x4_t (&b)[3]) {
#pragma unroll
      for (int part = 0; part < 3; ++part) {
        const uint8_t* base = lds + part * plane + cofs + (kw - 1) * 64;
        if constexpr ((DBG & 8) != 0) {
          b[part] = u32x4_t{(uint32_t)hp[0], (uint32_t)hp[1], (uint32_t)part, (uint32_t)kw};
        } else {
          const uint2 lo = hx_tr16(base + hp[0] * 64), hi = hx_tr16(base + hp[1] * 64);
          b[part] = u32x4_t{lo.x, lo.y, hi.x, hi.y};
        }
      }
    };
    int hpc[2];
    hp_of(0, hpc);
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      // A: this k-step's (loaded one step ahead), split; the next one issued, then a slice of
      // the next chunk's X staging (issue order pinned)
      uint32_t ah[4], am[4], al[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) split3_pk(anext[2 * e], anext[2 * e + 1], ah[e], am[e], al[e]);
      if (j + 1 < KS)
        load_a(q, j + 1);
      else
        load_a(q + 1, 0);
      if (j < 4) stage_slice(j);
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8_t Ah = __builtin_bit_cast(bf16x8_t, u32x4_t{ah[0], ah[1], ah[2], ah[3]});
      const bf16x8_t Am = __builtin_bit_cast(bf16x8_t, u32x4_t{am[0], am[1], am[2], am[3]});
      const bf16x8_t Al = __builtin_bit_cast(bf16x8_t, u32x4_t{al[0], al[1], al[2], al[3]});
      // tap kw + 1's fragments are read before tap kw's MFMAs (12 VGPRs more: not with 4 staged
      // items, which would spill at 3 waves per SIMD); the next k-step's rows before tap 0's
      constexpr bool AHEAD = ITEMS <= 3;
      if (!AHEAD && j > 0) hp_of(j, hpc);
      u32x4_t bc[3];
      read_b(0, hpc, bc);
      int hpn[2] = {hpc[0], hpc[1]};
      if (AHEAD && j + 1 < KS) hp_of(j + 1, hpn);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        u32x4_t bn[3];
        if (AHEAD && kw < 2) read_b(kw + 1, hpc, bn);
        if (!AHEAD && kw > 0) read_b(kw, hpc, bc);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8_t Bh = __builtin_bit_cast(bf16x8_t, bc[0]);
        const bf16x8_t Bm = __builtin_bit_cast(bf16x8_t, bc[1]);
        const bf16x8_t Bl = __builtin_bit_cast(bf16x8_t, bc[2]);
        if constexpr ((DBG & 4) != 0) {
          acc[kw][0] += __builtin_bit_cast(float, bc[0][0] ^ bc[1][1] ^ bc[2][2] ^ ah[0] ^ am[1] ^ al[2]);
        } else {
          f32x16 c = acc[kw];
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm, c, 0, 0, 0);
          acc[kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, c, 0, 0, 0);
        }
        if (AHEAD && kw < 2) {
#pragma unroll
          for (int part = 0; part < 3; ++part) bc[part] = bn[part];
        }
      }
      hpc[0] = hpn[0];
      hpc[1] = hpn[1];
    }
  }

  // ---- slab [split][Cout][9 * Cin], tap-major columns tap * Cin + c
  float* sl = a.slab + (long)blockIdx.z * a.g.M * a.g.N;
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const long col = (long)(dyi * 3 + kw) * a.Cin + c0 + fi;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int mm = m0 + 32 * mh + (e & 3) + 8 * (e >> 2) + 4 * fh;
      sl[(long)mm * a.g.N + col] = acc[kw][e];
    }
  }
}

// launch (conv_route.hip plan_halo chose the shape): grid (N / 256, M / 64, splits), 512 threads,
// the two LDS image buffers as dynamic shared memory
template <int MODE, int RFL, int EXT>
static int halo_launch_as(const ConvArgs& a, int items, int splits, hipStream_t st) {
  const dim3 grid(cdiv(a.g.N, 256), a.g.M / 64, splits), block(512);
  const LdsSize z{Halo3Lds::need(a.W), Halo3Lds::bytes(), Halo3Lds::cap};
  const bool one = items == 1;
  if (px3_terms() == 9)
    return one ? lds_launch<conv_halo3_kernel<MODE, 9, 1, 0, RFL, EXT>>(grid, block, z, st, a)
               : lds_launch<conv_halo3_kernel<MODE, 9, 2, 0, RFL, EXT>>(grid, block, z, st, a);
#if MD2_TIMING_VARIANTS
  // timing-only kernels of the plain bf16x6 forms (results wrong): MD2_TUNING=1 MD2_HX_DBG=k
  if constexpr (!RFL && !EXT) {
    static const int dbg = tuning_knob("MD2_HX_DBG", 0);
#define MD2_HX_DBGI(IT, D) lds_launch<conv_halo3_kernel<MODE, 6, IT, D>>(grid, block, z, st, a)
#define MD2_HX_DBGV(D) return one ? MD2_HX_DBGI(1, D) : MD2_HX_DBGI(2, D)
    switch (dbg) {
      case 0: break;
      case 1: MD2_HX_DBGV(1);
      case 2: MD2_HX_DBGV(2);
      case 3: MD2_HX_DBGV(3);
      case 4: MD2_HX_DBGV(4);
      default: MD2_HX_DBGV(6);
    }
#undef MD2_HX_DBGV
#undef MD2_HX_DBGI
  }
#endif
  return one ? lds_launch<conv_halo3_kernel<MODE, 6, 1, 0, RFL, EXT>>(grid, block, z, st, a)
             : lds_launch<conv_halo3_kernel<MODE, 6, 2, 0, RFL, EXT>>(grid, block, z, st, a);
}
int halo_launch(int mode, const ConvArgs& a, int items, int splits, int reflect, hipStream_t st) {
  if (mode == 0 && reflect) return halo_launch_as<0, 1, 0>(a, items, splits, st);
  if (mode == 1 && a.hx_ext) return halo_launch_as<1, 0, 1>(a, items, splits, st);
  return mode == 0 ? halo_launch_as<0, 0, 0>(a, items, splits, st) : halo_launch_as<1, 0, 0>(a, items, splits, st);
}

// stride-2 data-gradient halo kernel: grid (dY points / 128, Cin / 64, splits)
int halo_s2_launch(const ConvArgs& a, int items, int splits, hipStream_t st) {
  const dim3 grid(cdiv(a.g.N, 128), a.g.M / 64, splits);
  const LdsSize z{Halo3s2Lds::need(a.Wo), Halo3s2Lds::bytes(), Halo3s2Lds::cap};
  MD2_CHECK_ARG(items == 1, "conv_halo3s2: one staged pixel per thread");
  return lds_launch<conv_halo3s2_kernel<1>>(grid, dim3(512), z, st, a);
}

// 2D-tile halo kernel (conv_route.hip plan_halo, h.d2): grid (images x tiles, M / (32 MW), splits)
template <int MODE, int RFL, int EXT>
static int halo2d_launch_as(const ConvArgs& a, int mw, int splits, hipStream_t st) {
  const long tiles = (long)cdiv(a.W, H2_TW) * cdiv(a.H, H2_TH);
  const dim3 grid((unsigned)(a.g.N / ((long)a.H * a.W) * tiles), a.g.M / (32 * mw), splits);
  const LdsSize z{Halo2dLds::need(), Halo2dLds::bytes(), Halo2dLds::cap};
  return mw == 1 ? lds_launch<conv_halo2d_kernel<MODE, 1, RFL, EXT>>(grid, dim3(256), z, st, a)
                 : lds_launch<conv_halo2d_kernel<MODE, 2, RFL, EXT>>(grid, dim3(512), z, st, a);
}
int halo2d_launch(int mode, const ConvArgs& a, int mw, int splits, int reflect, hipStream_t st) {
  if (mode == 0) return reflect ? halo2d_launch_as<0, 1, 0>(a, mw, splits, st) : halo2d_launch_as<0, 0, 0>(a, mw, splits, st);
  return a.hx_ext ? halo2d_launch_as<1, 0, 1>(a, mw, splits, st) : halo2d_launch_as<1, 0, 0>(a, mw, splits, st);
}

// filter-gradient halo kernel: grid (Cin / 32, Cout / 64, splits), 384 threads, LDS from the
// chunk geometry (WHaloLds: r rows of W pixels + 2 halo rows, the k table behind the planes)
template <int ITEMS>
static int whalo_launch_it(const ConvArgs& a, int ksteps, int splits, hipStream_t st) {
  const dim3 grid(a.Cin / 32, a.Cout / 64, splits), block(384);
  const LdsSize z{WHaloLds::need(a.hx_r, a.W, ksteps), WHaloLds::bytes(a.hx_r, a.W), WHaloLds::cap};
#if MD2_TIMING_VARIANTS
  // timing-only kernels for the layer-2 shape, 3 items and 7 k-steps (results wrong):
  // MD2_TUNING=1 MD2_WHX_DBG=k
  if constexpr (ITEMS == 3) {
    static const int dbg = tuning_knob("MD2_WHX_DBG", 0);
    if (dbg && ksteps == 7) switch (dbg) {
      case 1: return lds_launch<conv_whalo_kernel<3, 7, 1>>(grid, block, z, st, a);
      case 2: return lds_launch<conv_whalo_kernel<3, 7, 2>>(grid, block, z, st, a);
      case 3: return lds_launch<conv_whalo_kernel<3, 7, 3>>(grid, block, z, st, a);
      case 4: return lds_launch<conv_whalo_kernel<3, 7, 4>>(grid, block, z, st, a);
      case 8: return lds_launch<conv_whalo_kernel<3, 7, 8>>(grid, block, z, st, a);
      case 11: return lds_launch<conv_whalo_kernel<3, 7, 11>>(grid, block, z, st, a);
      default: return lds_launch<conv_whalo_kernel<3, 7, 12>>(grid, block, z, st, a);
    }
  }
#endif
  switch (ksteps) {
    case 4: return lds_launch<conv_whalo_kernel<ITEMS, 4>>(grid, block, z, st, a);
    case 5: return lds_launch<conv_whalo_kernel<ITEMS, 5>>(grid, block, z, st, a);
    case 6: return lds_launch<conv_whalo_kernel<ITEMS, 6>>(grid, block, z, st, a);
    default: return lds_launch<conv_whalo_kernel<ITEMS, 7>>(grid, block, z, st, a);
  }
}
int whalo_launch(const ConvArgs& a, int items, int ksteps, int splits, hipStream_t st) {
  switch (items) {
    case 1: return whalo_launch_it<1>(a, ksteps, splits, st);
    case 2: return whalo_launch_it<2>(a, ksteps, splits, st);
    case 3: return whalo_launch_it<3>(a, ksteps, splits, st);
    default: return whalo_launch_it<4>(a, ksteps, splits, st);
  }
}
