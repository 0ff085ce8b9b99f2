// The photometric pass over S = 1, 2 or 3 sources, each addressed by its own base pointer and
// sample stride (gfx950): the kernel behind md2_loss_fwd_bwd_sources.  A stereo partner frame is a
// separate tensor with a caller-supplied transform; the x[N][3][C][H][W] layout does not change.
//
// Work layout, tiling, phases (P1 warp + gather, P2 window moments / SSIM / L1 / selection / adjoint
// coefficients, P3 pullback), the software pipeline and the parked P1 state in the wave's own LDS
// ring are those of photo.hip; read its header first.  What differs:
//  * every per-source quantity is an array over S and a plain fp32 op per source: the two halves of
//    v_pk_*_f32 fit two sources, not three (a packed 3-source form is future work).  This is the
//    arithmetic of the scalar predecessor of photo.hip, operation for operation, so the S = 2
//    instance gives the packed kernel's bits (tests/test_gpu_photo_sources.py) -- the two-source
//    production path does not come here;
//  * sources are processed in ascending order wherever a sum runs over them (d depth);
//  * selection: first argmin over the sources in the order given (strict <, ties to the earlier
//    source), then the automask, which wins ties; sel_map holds 0..S-1 or -1;
//  * a partials row is 1 + 12 S floats: the loss sum, then (dR (9), dt (3)) per source;
//  * cell_map is [S][N][H][W];
//  * parked LDS per wave: 3 slots x (2 C S + 1) x 64 lanes x 4 B -- 14592 B at S = 3, C = 3.  With
//    the 2 waves per SIMD the S <= 2 instances ask for, 8 waves of a CU hold at most 80 KB of the
//    160 KB; the S = 3 instances ask for one wave per SIMD (they need the registers), 58 KB.
// Built with photo.hip's flags (no implicit contraction; every FMA here is an explicit fmaf).
#include "photo_device.h"

namespace md2 {

//
// PK (per-sample intrinsics): the camera matrices of the block's sample come from a.Kn / a.invKn
// (device [N][9] each, read only) instead of g.K / g.invK.  They are read where g.K / g.invK are --
// the prologue and the Kc products of the partials -- through Kat / iKat below; a block belongs to
// one sample, so the loads are uniform.  Every operation after the read is the same, so equal rows
// give the PK = false instance's bits.
template <int C, int S, bool CELLS, bool PK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(S == 3 ? 1 : 2)))
void photo_sources_kernel(PhotoSrcArgs a, Geom g, PhotoTiling tl) {
  constexpr int NV = 2 * C * S + 1;   // parked P1 state: d val / d ix, d val / d iy (C S each), depth
  constexpr int NM = 2 + 3 * S;       // window moments per channel: y, yy, and x, xx, xy per source
  constexpr int PS = 1 + 12 * S;      // partials row
  __shared__ float s_v1[3 * NV * 64];

  const int lane = threadIdx.x;
  const int W = g.W, H = g.H;
  int b = blockIdx.x;
  const int tx = b % tl.tiles_x;
  b /= tl.tiles_x;
  const int ty = b % tl.tiles_y;
  b /= tl.tiles_y;
  const int n = b % a.N;
  const int s = b / a.N;
  const PhotoScale sc = a.sc[s];
  const int x0 = tx * PW, y0 = ty * tl.rows;
  const int rows = min(tl.rows, H - y0);
  const int KT = rows + 4;        // P1 rows y0-2 .. y0+rows+1

  const uint32_t HW4 = (uint32_t)W * H * 4u, W4 = (uint32_t)W * 4u;
  const float* tgt = a.target + (long)n * a.target_sample_stride;
  const __amdgpu_buffer_rsrc_t rt_ = make_rsrc(tgt, (uint32_t)C * HW4);
  __amdgpu_buffer_rsrc_t rs_[S];
#pragma unroll
  for (int sp = 0; sp < S; ++sp)
    rs_[sp] = make_rsrc(a.src[sp] + (long)n * a.src_sample_stride[sp], (uint32_t)C * HW4);
  const int dw = sc.dw, dh = sc.dh;
  const __amdgpu_buffer_rsrc_t rdsp =
      make_rsrc(sc.disp + (long)n * dw * dh, (uint32_t)dw * dh * 4u);

  [[maybe_unused]] const float* Kn = nullptr;
  [[maybe_unused]] const float* iKn = nullptr;
  if constexpr (PK) {
    Kn = a.Kn + 9 * (long)n;
    iKn = a.invKn + 9 * (long)n;
  }
  auto Kat = [&](int i) -> float {
    if constexpr (PK)
      return Kn[i];
    else
      return g.K[i];
  };
  auto iKat = [&](int i) -> float {
    if constexpr (PK)
      return iKn[i];
    else
      return g.invK[i];
  };

  // pixel -> camera maps per source in centred coordinates, formed in fp64 once per (sample, source)
  // and rounded once (photo.hip).  s_cam[3 sp + i] = Mc row i (x, y, z) and Kct_i of source sp;
  // s_cam[3 S + i] = invK S row i; s_cam[3 S + 3 + sp] = the depth-derivative constants of sp
  const float cxp = vreg(Kat(2)), cyp = vreg(Kat(5));
  // Kc is only read by the partials at the end.  From kernel arguments it is rematerialised there;
  // from memory (PK) it would stay in nine registers for the whole kernel, so it is formed there
  float Kc[9];
  auto make_Kc = [&]() {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Kc[j] = fmaf(-cxp, Kat(6 + j), Kat(j));
      Kc[3 + j] = fmaf(-cyp, Kat(6 + j), Kat(3 + j));
      Kc[6 + j] = Kat(6 + j);
    }
  };
  if constexpr (!PK) make_Kc();
  // row i (a lane's own) of a 3x3 held in registers: PK selects it, so the tables never go to scratch
  auto rowel = [&](const double (&A)[9], int i, int j) -> double {
    if constexpr (PK)
      return i == 0 ? A[j] : (i == 1 ? A[3 + j] : A[6 + j]);
    else
      return A[3 * i + j];
  };
  __shared__ float4 s_cam[4 * S + 3];
  if (lane < 4 * S + 3) {
    const double cxd = Kat(2), cyd = Kat(5);
    double Kd[9], iKS[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Kd[j] = (double)Kat(j) - cxd * Kat(6 + j);
      Kd[3 + j] = (double)Kat(3 + j) - cyd * Kat(6 + j);
      Kd[6 + j] = Kat(6 + j);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      iKS[3 * i] = iKat(3 * i);
      iKS[3 * i + 1] = iKat(3 * i + 1);
      iKS[3 * i + 2] = (double)iKat(3 * i) * cxd + (double)iKat(3 * i + 1) * cyd + iKat(3 * i + 2);
    }
    float4 v;
    if (lane < 3 * S) {
      const int sp = lane / 3, i = lane % 3;
      const float* rt = a.Rt + ((long)sp * a.N + n) * 12;
      double KR[3], m[3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
        KR[j] = rowel(Kd, i, 0) * rt[j] + rowel(Kd, i, 1) * rt[3 + j] + rowel(Kd, i, 2) * rt[6 + j];
#pragma unroll
      for (int j = 0; j < 3; ++j) m[j] = KR[0] * iKS[j] + KR[1] * iKS[3 + j] + KR[2] * iKS[6 + j];
      const double kt = rowel(Kd, i, 0) * rt[9] + rowel(Kd, i, 1) * rt[10] + rowel(Kd, i, 2) * rt[11];
      v = make_float4((float)m[0], (float)m[1], (float)m[2], (float)kt);
    } else if (lane < 3 * S + 3) {
      const int r = lane - 3 * S;
      v = make_float4((float)rowel(iKS, r, 0), (float)rowel(iKS, r, 1), (float)rowel(iKS, r, 2), 0.f);
    } else {
      const int q = lane - (3 * S + 3);
      const float* rt = a.Rt + ((long)q * a.N + n) * 12;
      double kt[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) kt[i] = Kd[3 * i] * rt[9] + Kd[3 * i + 1] * rt[10] + Kd[3 * i + 2] * rt[11];
      v = make_float4((float)(kt[0] - cxd * 1e-7), (float)(kt[1] - cyd * 1e-7), (float)(kt[2] + 1e-7), 0.f);
    }
    s_cam[lane] = v;
  }
  __syncthreads();
  // an opaque LDS base per use site: constant-offset ds_reads, never hoisted out of the row loop
  auto cam_base = [&]() {
    int z = 0;
    asm volatile("" : "+v"(z));
    return s_cam + z;
  };
  // moment shift: the target at the image centre, per channel -- the same for every wave of the
  // sample, so halo rows / columns two waves both evaluate come out bit-identical
  float cc[C];
  {
    const int cx = W / 2, cy = H / 2;
#pragma unroll
    for (int c = 0; c < C; ++c) cc[c] = vreg(tgt[(long)c * W * H + (long)cy * W + cx]);
  }

  // per-lane constants
  const int col = x0 - 2 + lane;
  const int colr = reflect_clamp(col, W);
  const float wcol = (float)(colr + 1) - cxp;
  const bool cvalid = col >= 0 && col < W;
  const bool outl = lane >= 2 && lane < 2 + PW && col < W;
  // reflect adjoint x[-1] = x[1], x[W] = x[W-2], folded into the value columns 0 / W-1 ship
  const float wship = (col == 0 || col == W - 1) ? 2.f : 1.f;
  const float usx = sc.rx * (float)colr;
  const int ux0 = min((int)usx, dw - 1);
  const float ufx = usx - (float)ux0;
  const int uxp = min(ux0, dw - 2);
  const bool uedge = ux0 == dw - 1;
  const float kS = a.wloss * (0.85f / (float)C) * (1.f / 9.f);
  const float kL = a.wloss * (0.15f / (float)C);
  const float inv9 = vreg(1.f / 9.f), c1 = vreg(1e-4f), c2 = vreg(9e-4f), eps7 = vreg(1e-7f);
  const float Wm1 = vreg((float)(W - 1)), Hm1 = vreg((float)(H - 1));
  const float disp_range = vreg(g.disp_range), min_disp = vreg(g.min_disp);

  // ---- pipeline registers --------------------------------------------------------------------
  float dA[4] = {0.f, 0.f, 0.f, 0.f}, fyA = 0.f;   // stage A: disparity loads (2 rows ahead)
  float gv[S][C][4], tv[C];                         // stage B: gathers (1 row ahead)
  float bfx[S], bfy[S], bmx[S], bmy[S], bdepth = 0.f;
  float xr[3][S][C], yr[3][C];                      // shifted warped / target values, rows r-2..r
  float ch[3][S][C][3];                             // horizontal coefficient sums, rows r-3..r-1
  float acc[12 * S];                                // per source: sum dcam_i X_j (9), sum dcam_i (3)
#pragma unroll
  for (int i = 0; i < 12 * S; ++i) acc[i] = 0.f;
  float lsum = 0.f;
  int selc = -1;                                    // P2 decision of the last P2 row
  float gpc = 0.f;                                  // its cotangent

  auto issue_disp = [&](int R) {
    const float sy = sc.ry * (float)reflect_clamp(R, H);
    const int uy0 = min((int)sy, dh - 1), uy1 = min(uy0 + 1, dh - 1);
    fyA = sy - (float)uy0;
    const float2 t = bload2_s(rdsp, (uint32_t)(uy0 * dw + uxp) * 4u, 0u);
    const float2 bb = bload2_s(rdsp, (uint32_t)(uy1 * dw + uxp) * 4u, 0u);
    dA[0] = t.x;
    dA[1] = t.y;
    dA[2] = bb.x;
    dA[3] = bb.y;
  };

  auto issue_gathers = [&](int R) {
    const int Rr = reflect_clamp(R, H);
    const float h = (float)(Rr + 1) - cyp;
    const float d00 = uedge ? dA[1] : dA[0], d10 = uedge ? dA[3] : dA[2];
    const float dtop = fmaf(ufx, dA[1] - d00, d00);
    const float dbot = fmaf(ufx, dA[3] - d10, d10);
    const float d = fmaf(fyA, dbot - dtop, dtop);
    const float depth = frcp(fmaf(d, disp_range, min_disp));   // disparity_to_depth
    bdepth = depth;
    const float4* camc = cam_base();
#pragma unroll
    for (int sp = 0; sp < S; ++sp) {
      float cam[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float4 mk = camc[3 * sp + i];
        cam[i] = fmaf(depth, fmaf(mk.x, wcol, fmaf(mk.y, h, mk.z)), mk.w);
      }
      const float rc = frcp(cam[2] + eps7);
      // normalize + grid_sample unnormalise (align_corners) collapse to u - 1 (0-based)
      const float c2r = cam[2] * rc;
      const float ix = fmaf(cam[0], rc, fmaf(cxp, c2r, -1.f));
      const float iy = fmaf(cam[1], rc, fmaf(cyp, c2r, -1.f));
      const float xc = fminf(fmaxf(ix, 0.f), Wm1), yc = fminf(fmaxf(iy, 0.f), Hm1);  // :border
      const int xi = min((int)xc, W - 2), yi = min((int)yc, H - 2);
      bfx[sp] = xc - (float)xi;
      bfy[sp] = yc - (float)yi;
      bmx[sp] = (ix > 0.f && ix < Wm1) ? 1.f : 0.f;   // clamp gradient masks
      bmy[sp] = (iy > 0.f && iy < Hm1) ? 1.f : 0.f;
      if (CELLS && outl && R >= y0 && R < y0 + rows) {          // parity diagnostics only
        const int fx = ix > 0.f ? (ix < Wm1 ? 0 : 2) : 1, fy = iy > 0.f ? (iy < Hm1 ? 0 : 2) : 1;
        sc.cell_map[(((long)sp * a.N + n) * H + R) * W + col] =
            xi | (yi << PHOTO_CELL_YSHIFT) | (fx << PHOTO_CELL_FXSHIFT) | (fy << PHOTO_CELL_FYSHIFT);
      }
      // xi <= W-2, yi <= H-2: the right / lower taps are always +1 / +W, so each row pair of
      // taps is one 8-byte load
      const uint32_t vo = (uint32_t)(yi * W + xi) * 4u;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t so = (uint32_t)c * HW4;
        const float2 t = bload2_s(rs_[sp], vo, so), bb = bload2_s(rs_[sp], vo, so + W4);
        gv[sp][c][0] = t.x;
        gv[sp][c][1] = t.y;
        gv[sp][c][2] = bb.x;
        gv[sp][c][3] = bb.y;
      }
    }
    const uint32_t to = (uint32_t)(Rr * W + colr) * 4u;
#pragma unroll
    for (int c = 0; c < C; ++c) tv[c] = bload_s(rt_, to, (uint32_t)c * HW4);
  };

  // P1 of row R (its gathers have landed): values -> ring slot SL, derivative terms -> LDS slot SL
  auto finish_p1 = [&](auto Sc) {
    constexpr int SL = decltype(Sc)::value;
    float* v1 = s_v1 + SL * NV * 64 + lane;
#pragma unroll
    for (int c = 0; c < C; ++c) yr[SL][c] = tv[c] - cc[c];
#pragma unroll
    for (int sp = 0; sp < S; ++sp) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float v00 = gv[sp][c][0], v01 = gv[sp][c][1], v10 = gv[sp][c][2], v11 = gv[sp][c][3];
        const float d0 = v01 - v00, d1 = v11 - v10;
        const float top = fmaf(bfx[sp], d0, v00), bot = fmaf(bfx[sp], d1, v10);
        const float dv = bot - top;
        xr[SL][sp][c] = fmaf(bfy[sp], dv, top) - cc[c];
        v1[(sp * C + c) * 64] = fmaf(bfy[sp], d1 - d0, d0) * bmx[sp];      // d val / d ix
        v1[(S * C + sp * C + c) * 64] = dv * bmy[sp];                      // d val / d iy
      }
    }
    v1[(2 * S * C) * 64] = bdepth;
  };

  // P2 head for row p (window rows in ring slots SL+1, SL+2 (= p), SL): SSIM and L1 per source,
  // the adjoint coefficients of every source (cf), first argmin over the sources -> sel
  auto p2_head = [&](auto Sc, int p, float am, float gp, float (&cf)[S][C][3]) -> int {
    constexpr int SL = decltype(Sc)::value;
    constexpr int SP = (SL + 2) % 3;
    constexpr int S0 = (SL + 1) % 3;
    // rows -1 and H are not window centres: zero coefficients (reflect adjoint, P3)
    const float kp = (cvalid && p >= 0 && p < H) ? kS * gp : 0.f;
    float loss[S];
#pragma unroll
    for (int sp = 0; sp < S; ++sp) loss[sp] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      // window moments: vertical 3-sums over the ring, then horizontal 3-sums across lanes
      float m[NM];
      const float y0v = yr[S0][c], y1v = yr[SP][c], y2v = yr[SL][c];
      m[0] = y0v + y1v + y2v;
      m[1] = fmaf(y0v, y0v, fmaf(y1v, y1v, y2v * y2v));
#pragma unroll
      for (int sp = 0; sp < S; ++sp) {
        const float a0 = xr[S0][sp][c], a1 = xr[SP][sp][c], a2 = xr[SL][sp][c];
        m[2 + 3 * sp] = a0 + a1 + a2;
        m[3 + 3 * sp] = fmaf(a0, a0, fmaf(a1, a1, a2 * a2));
        m[4 + 3 * sp] = fmaf(a0, y0v, fmaf(a1, y1v, a2 * y2v));
        loss[sp] = fmaf(0.15f / (float)C, fabsf(y1v - a1), loss[sp]);   // L1, centre
      }
      __builtin_amdgcn_sched_barrier(0);
      hsum3_n(m);
      __builtin_amdgcn_sched_barrier(0);
      const float my = m[0] * inv9;                 // shifted mean of the target window
      const float mty = fmaf(m[0], inv9, cc[c]);
      const float vy = fmaf(m[1], inv9, -my * my);
      const float two_mty = 2.f * mty;
      const float B1y = fmaf(mty, mty, c1), B2y = vy + c2;
#pragma unroll
      for (int sp = 0; sp < S; ++sp) {
        const float mx = m[2 + 3 * sp] * inv9;
        const float mtx = fmaf(m[2 + 3 * sp], inv9, cc[c]);
        const float vx = fmaf(m[3 + 3 * sp], inv9, -mx * mx);
        const float cxy = fmaf(m[4 + 3 * sp], inv9, -mx * my);
        const float A1 = fmaf(mtx, two_mty, c1), A2 = fmaf(2.f, cxy, c2);
        const float B1 = fmaf(mtx, mtx, B1y), B2 = vx + B2y;
        const float rd = frcp(B1 * B2);
        const float r = (A1 * A2) * rd;
        const float val = fmaf(-0.5f, r, 0.5f);
        const float sv = fminf(fmaxf(val, 0.f), 1.f);
        loss[sp] = fmaf(0.85f / (float)C, sv, loss[sp]);
        // d loss/d (mu_x, var_x, cov_xy) of this window (clamp gradient 1 inside [0, 1]); the
        // adjoint at q is g_m + 2 g_v (x_q - mu_x) + g_c (y_q - mu_y) = A + x_q B + y_q Cc
        const float t1 = (val == sv) ? kp * rd : 0.f;
        const float gm = t1 * fmaf(r * mtx, B2, -mty * A2);
        const float gv2 = (r * t1) * B1;            // 2 d/d var_x
        const float gc = -t1 * A1;                  //   d/d cov_xy
        cf[sp][c][0] = fmaf(-gv2, mx, fmaf(-gc, my, gm));
        cf[sp][c][1] = gv2;
        cf[sp][c][2] = gc;
      }
    }
    // first argmin over the sources, then the automask (wins ties), training.jl:60-62
    int sel = 0;
    float lmin = loss[0];
#pragma unroll
    for (int sp = 1; sp < S; ++sp)
      if (loss[sp] < lmin) {
        sel = sp;
        lmin = loss[sp];
      }
    if (a.automask && !(lmin < am)) {
      sel = -1;
      lmin = am;
    }
    const bool own = p >= y0 && p < y0 + rows && outl;
    lsum += own ? lmin : 0.f;
    if (own) {
      const long qq = ((long)n * H + p) * W + col;
      if (sc.loss_map) sc.loss_map[qq] = lmin;
      if (sc.sel_map) sc.sel_map[qq] = (signed char)sel;
    }
    return sel;
  };

  // P2 tail: the selected source's coefficients of row q+1, horizontally summed -> ch[SL]
  auto p2_tail = [&](auto Sc, int sel, const float (&cf)[S][C][3]) {
    constexpr int SL = decltype(Sc)::value;
    constexpr int NT = 3 * C * S;
    float F[NT], G[NT], t[NT];
#pragma unroll
    for (int sp = 0; sp < S; ++sp)
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int f = (sp * C + c) * 3 + k;
          F[f] = (sel == sp) ? cf[sp][c][k] : 0.f;
          G[f] = F[f] * wship;
        }
    // (left + (right + F)) with the weights already in G: the two roundings of
    // fma(wl, left, fma(wr, right, F)), in two passes
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NT; ++i) t[i] = from_right(G[i]) + F[i];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NT; ++i) t[i] = from_left(G[i]) + t[i];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sp = 0; sp < S; ++sp)
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) ch[SL][sp][c][k] = t[(sp * C + c) * 3 + k];
  };

  // P3 of row q (coefficient rows q-1, q, q+1 in ch slots SL+1, SL+2, SL; values in ring slot
  // SL+1; P1 derivative terms in LDS slot SL+1): d/d warped values -> projection pullback
  auto p3 = [&](auto Sc, int q, bool live3, int selq, float gpq) {
    constexpr int SL = decltype(Sc)::value;
    constexpr int SA = (SL + 1) % 3, SB = (SL + 2) % 3;
    const float wa = (q == 1) ? 2.f : 1.f, wb = (q == H - 2) ? 2.f : 1.f;
    const float* v1 = s_v1 + SA * NV * 64 + lane;
    const float kLq = kL * gpq;
    float gx[S], gy[S];
#pragma unroll
    for (int sp = 0; sp < S; ++sp) gx[sp] = gy[sp] = 0.f;
    unsigned l1bits = 0;                           // CELLS only: the L1 branches taken at q
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float yq = yr[SA][c];
      // L1 pullback at q for its selected source: d|y - x|/dx = sign(x - y), abs'(0) = 0
      float xs = xr[SA][0][c];
#pragma unroll
      for (int sp = 1; sp < S; ++sp) xs = (selq == sp) ? xr[SA][sp][c] : xs;
      const float df = xs - yq;
      const float t = df > 0.f ? kLq : (df < 0.f ? -kLq : 0.f);
      if (CELLS) l1bits |= (df > 0.f ? 2u : (df < 0.f ? 1u : 3u)) << (PHOTO_CELL_L1SHIFT + 2 * c);
#pragma unroll
      for (int sp = 0; sp < S; ++sp) {
        float sum[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
          sum[k] = fmaf(wa, ch[SA][sp][c][k], fmaf(wb, ch[SL][sp][c][k], ch[SB][sp][c][k]));
        float dx = fmaf(xr[SA][sp][c], sum[1], fmaf(yq, sum[2], sum[0]));
        dx += (selq == sp) ? t : 0.f;
        gx[sp] = fmaf(dx, v1[(sp * C + c) * 64], gx[sp]);
        gy[sp] = fmaf(dx, v1[(S * C + sp * C + c) * 64], gy[sp]);
      }
    }
    const bool live = live3 && outl;
    if (CELLS && live && selq >= 0) {              // parity diagnostics only (same lane wrote it)
      int* cm = sc.cell_map + (((long)selq * a.N + n) * H + q) * W + col;
      *cm = (int)((unsigned)*cm | l1bits);
    }
    const float depth = v1[(2 * S * C) * 64];
    const float h = (float)(q + 1) - cyp;
    const float4* camc = cam_base();
    float X[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float4 ik = camc[3 * S + i];
      X[i] = depth * fmaf(ik.x, wcol, fmaf(ik.y, h, ik.z));
    }
    float ddepth = 0.f;
#pragma unroll
    for (int sp = 0; sp < S; ++sp) {               // ascending: the order of the sum into ddepth
      const float ggx = live ? gx[sp] : 0.f, ggy = live ? gy[sp] : 0.f;
      float m[3], cam[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float4 mk = camc[3 * sp + i];
        m[i] = fmaf(mk.x, wcol, fmaf(mk.y, h, mk.z));
        cam[i] = fmaf(depth, m[i], mk.w);
      }
      const float rc = frcp(cam[2] + eps7);
      const float4 kd = camc[3 * S + 3 + sp];
      float dc[3];                                 // d loss / d camt
      dc[0] = ggx * rc;
      dc[1] = ggy * rc;
      dc[2] = -fmaf(ggx, cam[0], ggy * cam[1]) * rc * rc;
      const float rc2 = rc * rc;
      ddepth = fmaf(rc2, fmaf(ggx, fmaf(m[0], kd.z, -kd.x * m[2]), ggy * fmaf(m[1], kd.z, -kd.y * m[2])), ddepth);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[12 * sp + 3 * i + j] = fmaf(dc[i], X[j], acc[12 * sp + 3 * i + j]);
        acc[12 * sp + 9 + i] += dc[i];
      }
    }
    // depth = 1/(disp*range + min_disp)  =>  d depth/d disp = -range * depth^2
    if (live) sc.g_disp[((long)n * H + q) * W + col] = -ddepth * disp_range * depth * depth;
  };

  // one row step k: P1 of row R = y0-2+k (slot SL = k % 3), P2 of row R-1, P3 of row R-2
  auto step = [&](auto Sc, auto Pc, int k) {
    constexpr int PH = decltype(Pc)::value;
    const int R = y0 - 2 + k;
    finish_p1(Sc);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PH & PH_P2) {
      const int p = min(max(R - 1, 0), H - 1);
      float am = 0.f, gp = 1.f;
      if (a.automask) am = a.automask[((long)n * H + p) * W + colr];
      if (a.gmap) gp = a.gmap[((long)n * H + p) * W + colr];
      float cf[S][C][3];
      const int sel = p2_head(Sc, R - 1, am, gp, cf);
      issue_gathers(R + 1);                        // rows past the tile are harmless (clamped)
      issue_disp(R + 2);
      p2_tail(Sc, sel, cf);
      if constexpr (PH & PH_P3) p3(Sc, R - 2, k >= 4, selc, gpc);
      selc = sel;
      gpc = gp;
    } else {
      issue_gathers(R + 1);
      issue_disp(R + 2);
    }
    __builtin_amdgcn_sched_barrier(0);             // steps do not interleave (register pressure)
  };

#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int sp = 0; sp < S; ++sp)
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) ch[r][sp][c][k] = 0.f;
  issue_disp(y0 - 2);
  issue_gathers(y0 - 2);
  issue_disp(y0 - 1);
  // rows y0-2, y0-1: P1 only; row y0 (k = 2): + P2 of the halo row y0-1; k = 3: + P2 of row y0
  // (its P3 row y0-1 is a halo row); from k = 4 on every phase, up to the band's last row
  step(Slot<0>{}, std::integral_constant<int, 0>{}, 0);
  step(Slot<1>{}, std::integral_constant<int, 0>{}, 1);
  step(Slot<2>{}, std::integral_constant<int, PH_P2>{}, 2);
  step(Slot<0>{}, std::integral_constant<int, PH_P2>{}, 3);
  for (int k = 4;; k += 3) {
    step(Slot<1>{}, std::integral_constant<int, PH_ALL>{}, k);
    if (k + 1 >= KT) break;
    step(Slot<2>{}, std::integral_constant<int, PH_ALL>{}, k + 1);
    if (k + 2 >= KT) break;
    step(Slot<0>{}, std::integral_constant<int, PH_ALL>{}, k + 2);
    if (k + 3 >= KT) break;
  }

  // ---- per-wave partials: loss sum, then per source dR = Kc^T sum(dcamt X^T), dt = Kc^T sum(dcamt)
  lsum = wave_sum_dpp(lsum);
#pragma unroll
  for (int i = 0; i < 12 * S; ++i) acc[i] = wave_sum_dpp(acc[i]);
  if (lane == 0) {
    if constexpr (PK) make_Kc();
    float* out = sc.partials + (((long)n * tl.tiles_y + ty) * tl.tiles_x + tx) * PS;
    out[0] = lsum;
#pragma unroll
    for (int sp = 0; sp < S; ++sp) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int l = 0; l < 3; ++l)
          out[1 + 12 * sp + 3 * k + l] =
              fmaf(Kc[k], acc[12 * sp + l], fmaf(Kc[3 + k], acc[12 * sp + 3 + l], Kc[6 + k] * acc[12 * sp + 6 + l]));
        out[1 + 12 * sp + 9 + k] =
            fmaf(Kc[k], acc[12 * sp + 9], fmaf(Kc[3 + k], acc[12 * sp + 10], Kc[6 + k] * acc[12 * sp + 11]));
      }
    }
  }
}

namespace {
template <int C, int S, bool PK>
void launch_cs(const PhotoSrcArgs& a, const Geom& g, const PhotoTiling& tl, bool cells, long blocks,
               hipStream_t st) {
  const dim3 grid((unsigned)blocks), block(64);
  if (cells)
    hipLaunchKernelGGL((photo_sources_kernel<C, S, true, PK>), grid, block, 0, st, a, g, tl);
  else
    hipLaunchKernelGGL((photo_sources_kernel<C, S, false, PK>), grid, block, 0, st, a, g, tl);
}
template <int C, bool PK>
void launch_c(const PhotoSrcArgs& a, const Geom& g, const PhotoTiling& tl, bool cells, long blocks,
              hipStream_t st) {
  if (a.nsrc == 1)
    launch_cs<C, 1, PK>(a, g, tl, cells, blocks, st);
  else if (a.nsrc == 2)
    launch_cs<C, 2, PK>(a, g, tl, cells, blocks, st);
  else
    launch_cs<C, 3, PK>(a, g, tl, cells, blocks, st);
}
}  // namespace

int launch_photometric_sources(const PhotoSrcArgs& a, const Geom& g, int C, hipStream_t st) {
  MD2_CHECK_ARG(a.nsrc >= 1 && a.nsrc <= MAX_SOURCES, "photometric: 1 to 3 sources");
  bool cells;
  MD2_TRY(check_photometric(a.sc, a.nscales, g, C, &cells));
  MD2_CHECK_ARG(a.target && a.Rt && a.N > 0, "photometric: null pointer");
  for (int s = 0; s < a.nsrc; ++s) MD2_CHECK_ARG(a.src[s] != nullptr, "photometric: null source");
  const PhotoTiling tl = photo_tiling(g.W, g.H, a.N, a.nscales);
  const long blocks = tl.per_scale() * a.N * a.nscales;
  MD2_CHECK_ARG((a.Kn == nullptr) == (a.invKn == nullptr), "photometric: Kn and invKn come together");
  const bool pk = a.Kn != nullptr;
  if (C == 3)
    pk ? launch_c<3, true>(a, g, tl, cells, blocks, st) : launch_c<3, false>(a, g, tl, cells, blocks, st);
  else
    pk ? launch_c<1, true>(a, g, tl, cells, blocks, st) : launch_c<1, false>(a, g, tl, cells, blocks, st);
  MD2_LAUNCH_CHECK();
  return MD2_OK;
}

}  // namespace md2
