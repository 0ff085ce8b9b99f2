// Single-output-channel 3x3 convolutions (DepthDecoder disparity heads, src/depth_decoder.jl:46)
// on VALU: forward / data gradient / filter gradient.  Routing: the model batches its heads into
// heads_fwd / heads_bwd; conv_fwd / conv_dgrad / conv_wgrad send a head_conv_ok shape there as one
// job when it is reflect-padded, stores (no accumulate) and fits (heads_job_unfit), else to head_*.
#pragma once
#include "conv.h"

namespace md2 {

// input planes of image b start at (b % bdiv) * bs0 + (b / bdiv) * bhi (TensorIn p0 addressing)
struct HeadIn {
  const float* p;
  long bs0;
  int bdiv;
  long bhi;
};
// filter tap (c, tap) = p[c * sc + tap * st] (read straight from the packed GEMM operand)
struct HeadW {
  const float* p;
  long sc, st;
};

// All disparity heads of the DepthDecoder in ONE launch per pass (3x3 reflect-pad, Cout = 1):
// the forward after the whole decoder, the data + filter gradients before the decoder backward.
// Each head is an HBM-bound pass over its input planes; batched, the four heads share one launch
// floor and fill the chip together instead of one small grid at a time.
constexpr int MAX_HEADS = 5;
struct HeadJob {
  HeadIn x;             // input planes (the branch output o2)
  HeadW wf, wd;         // forward / data-gradient views of the packed weights (conv_head_w)
  int Cin, H, W, N;
  const float* bias;
  float* y;             // forward output, image stride ybs
  long ybs;
  const float* dy;      // backward: d loss / d pre-activation, [N][H][W]
  float* dx;            // d loss / d x, image stride dxbs (written, not accumulated); nullptr: none
  long dxbs;
  float* dw;            // [Cin * 9] (written); nullptr: no filter gradient (db is then not written)
  float* db;            // [1] (written) or nullptr
};
// nullptr when the batched kernels take the job, else why not: the shape (H >= 2, W >= 4 and
// even, sizes < 2^31) and the vector alignment of x, y, dy, dx (null pointers pass) and their strides
const char* heads_job_unfit(const HeadJob& j);
int heads_fwd(const HeadJob* jobs, int n, int act, hipStream_t st);
size_t heads_bwd_workspace(const HeadJob* jobs, int n);
int heads_bwd(const HeadJob* jobs, int n, void* ws, size_t ws_bytes, hipStream_t st);

// The pixel-per-lane fallback, one job per call: reflect or zero padding, any H, W >= 2, optional
// accumulation into y / dx / dw, db.
bool head_conv_ok(const ConvShape& s);
size_t head_wgrad_workspace(const HeadJob& j);
int head_fwd(const HeadJob& j, bool reflect, int act, int accumulate, hipStream_t st);
int head_dgrad(const HeadJob& j, bool reflect, int accumulate, hipStream_t st);
int head_wgrad(const HeadJob& j, bool reflect, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);

HeadIn conv_head_in(const TensorIn& x);
HeadW conv_head_w(const ConvShape& s, int mode, const float* packed);
HeadJob conv_head_job(const ConvShape& s);   // the shape fields; the caller adds its operands

}  // namespace md2
