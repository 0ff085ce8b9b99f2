/* md2.h -- C ABI of libmd2hip.so, the MI355X (gfx950) hot path of the Monodepth2.jl train step.
 *
 * Every entry point is extern "C", takes plain pointers/sizes (device pointers unless noted),
 * returns 0 on success or an MD2_E* code, and leaves a message for md2_last_error().
 * `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *
 * Layout: Julia column-major (W,H,C,N) arrays are memory-identical to the C-order [N][C][H][W]
 * arrays used here, so a Julia ccall shim passes pointers without transposes.
 * Small matrices (K, invK, R) are ROW-major 3x3 here; the Julia shim passes permutedims(K).
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   md2_loss_*            src/training.jl:21-78  train_loss after the model call (+ Zygote pullback)
 *   md2_so3_compose_*     src/utils.jl:106-145,185-192  so3_exp_map / hat rrule / composeT
 *   md2_conv2d_*          Flux Conv + NNlib conv / ∇conv_data / ∇conv_filter (depth/pose decoders,
 *                         ResNet.jl encoder)
 *   md2_model_*           src/model.jl:24-70 Model / eval_poses / eval_disparity,
 *                         src/depth_decoder.jl, src/pose_decoder.jl, ResNet.jl ResidualNetwork
 *   md2_model_train_*     the gradient(θ) + update!(ADAM) loop of scripts/script.jl:84-86 and
 *                         src/simple_depth.jl:25-42
 */
#ifndef MD2_H
#define MD2_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on every change to an exported struct layout or signature.  2: md2_loss_out gained
 * vis_cell; md2_model_cfg gained embedding_levels and num_bins.  Bindings refuse a mismatch. */
#define MD2_ABI_VERSION 2

#define MD2_OK 0
#define MD2_EINVAL 1
#define MD2_EHIP 2
#define MD2_ENOTSUP 3
#define MD2_ENOMEM 4
#define MD2_ESTATE 5

int md2_abi_version(void);
/* hash of the sources the library was built from (csrc/Makefile BUILD_ID): bindings recompute it
 * from their source tree and refuse a stale library */
const char* md2_build_id(void);
/* thread-local message of the last failing call (never NULL). */
const char* md2_last_error(void);
/* number of visible HIP devices (host call; does not initialise a context). */
int md2_device_count(int* count);
/* async device-to-device copy on `stream` (used to hand library-owned outputs to the host) */
int md2_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss tail: src/training.jl:25-77 (given the model's disparities and poses) -- forward value
 * AND the Zygote pullback in one pass per scale.
 * ---------------------------------------------------------------------------------------- */
#define MD2_MAX_SCALES 5

typedef struct md2_loss_cfg {
  int n;                       /* samples (Params.batch_size)                                */
  int c;                       /* image channels (1 or 3)                                    */
  int width, height;           /* Params.target_size                                         */
  int nscales;                 /* length(TrainCache.scales)                                  */
  int scale_w[MD2_MAX_SCALES]; /* disparity resolution of each scale: 2 <= scale_w <= width, */
  int scale_h[MD2_MAX_SCALES]; /* 1 <= scale_h <= height (else MD2_EINVAL)                   */
  float smooth_weight[MD2_MAX_SCALES]; /* train_loss: disparity_smoothness * scale           */
  float divisor;               /* train_loss: nscales (training.jl:77); slow_depth: 1         */
  int smooth_normalize;        /* 1: disparity / (mean + 1e-7) (training.jl:64-65)           */
  float K[9];                  /* TrainCache.K, row-major                                    */
  float invK[9];               /* TrainCache.invK, row-major                                 */
  float min_depth, max_depth;  /* Params                                                      */
  long long x_sample_stride;   /* elements between samples of x (L*C*H*W for x[N][L][C][H][W]) */
  long long x_frame_stride;    /* elements between frames (C*H*W)                            */
  int target, src0, src1;      /* 0-based frame ids (TrainCache.target_id-1, source_ids-1)   */
  int invert_mask;             /* bit s set: source s < target (training.jl:29)              */
  int sigmoid_grad;            /* 1: d_disp w.r.t. the sigmoid head pre-activation           */
} md2_loss_cfg;

size_t md2_loss_workspace_size(const md2_loss_cfg* cfg);

/* Outputs of md2_loss_fwd_bwd (device pointers; NULL = not wanted, except loss). */
typedef struct md2_loss_out {
  float* loss;                       /* [1]  train_loss value                                 */
  float* terms;                      /* [nscales][2] mean warp loss, weighted smooth term     */
  float* d_disp[MD2_MAX_SCALES];     /* d loss / d disp[s] (or / d pre-sigmoid, cfg)          */
  float* d_pose;                     /* [2n][6] d loss / d (rvec, tvec)                       */
  float* vis_loss;                   /* [nscales][n][h][w] per-pixel warp loss (vis_loss)     */
  signed char* vis_sel;              /* [nscales][n][h][w] argmin source (-1 = automask)      */
  float* vis_warped;                 /* [2][n][c][h][w] both sources warped by the LAST scale
                                        (train_loss vis_warped, src/training.jl:71-73)        */
  int* vis_cell;                     /* [nscales][2][n][h][w] parity diagnostics: per pixel and
                                        source the grid_sample bilinear cell and border state,
                                        x | y << 11 | sx << 22 | sy << 24 (0-based cell corner;
                                        s = 0 interior, 1 clamped to 0, 2 clamped to W-1 / H-1);
                                        on the selected source, bits 26 + 2c = the L1 branch of
                                        channel c (1 warped < target, 2 >, 3 equal); w, h <= 2048 */
} md2_loss_out;

/* disp[s]: [n][scale_h][scale_w]; pose: [2n][6] = (rvec, tvec) for (source s, sample i) at row
 * s*n+i; x: frames; automask: [n][h][w] identity-reprojection loss or NULL (Params.automasking).
 * dloss: upstream gradient of the scalar loss (1 for gradient(θ)). */
int md2_loss_fwd_bwd(const md2_loss_cfg* cfg, const float* const* disp, const float* pose,
                     const float* x, const float* automask, float dloss,
                     const md2_loss_out* out, void* workspace, void* stream);

/* composeT(so3_exp_map(rvec), tvec, invert) for 2n poses -> Rt [2n][12] (R row-major, t). */
int md2_so3_compose_fwd(const float* pose, int n, int invert_mask, float* Rt, void* stream);
int md2_so3_compose_bwd(const float* pose, int n, int invert_mask, const float* dRt,
                        float* d_pose, void* stream);

/* ------------------------------------------------------------------------------------------
 * Op-level loss primitives at ChainRulesCore rrule granularity (fwd + pullback pairs), for a host
 * that differentiates the reference's ops one at a time (julia/MD2HIP.jl).  Layouts are the Julia
 * arrays read as C-order; small matrices row-major (the shim passes permutedims).
 *
 * md2_automasking_loss   automasking_loss(ssim, x, target; source_ids)   src/training.jl:9-11
 *   x [n][3][c][h][w]; out [n][h][w] = min over the two raw sources of photometric_loss (ties to
 *   the first source); 0-based frame ids.  Not differentiable (data only).
 * md2_ssim_{fwd,bwd}     (ssim::SSIM)(x, y)                                src/utils.jl:29-43
 *   x, y, out, dout, dx, dy: [n][c][h][w] (Julia (W,H,C,N)); dx or dy may be NULL.
 * md2_backproject_{fwd,bwd}   (b::Backproject)(depth, invK)                src/utils.jl:67-69
 *   depth [n][w*h] (Julia (1,W*H,N)); out [n][w*h][3] (Julia (3,W*H,N)); invK row-major; the
 *   invK cotangent is not formed (TrainCache constant).
 * md2_project_{fwd,bwd}   (p::Project)(points, K, R, t)                    src/utils.jl:99-103
 *   points [n][w*h][3]; R [n][9] row-major; t [n][3]; out [n][w*h][2] normalised (-1, 1);
 *   pullback to points, R, t (deterministic per-sample reductions; K's cotangent not formed).
 * md2_grid_sample_border_{fwd,bwd}   NNlib grid_sample(x, grid; padding_mode=:border),
 *   align_corners=true (src/training.jl:56): x [n][c][hi][wi], grid [n][ho][wo][2] (Julia
 *   (2,W,H,N)), out [n][c][ho][wo]; pullback to grid and (if d_x != NULL, by atomic scatter
 *   whose summation order is not fixed) to x.
 * md2_smooth_loss_{fwd,bwd}   smooth_loss(disparity, image)                 src/utils.jl:163-177
 *   disparity [n][h][w], image [n][c][h][w] (c = 1 or 3); loss: one device float.
 * md2_warp_photometric_{fwd,bwd}   one scale of train_loss's loop body     src/training.jl:43-62
 *   upsample (align_corners) -> disparity_to_depth -> Backproject -> Project(R_s, t_s) ->
 *   grid_sample(:border) -> photometric_loss per source -> min over sources [-> _apply_mask].
 *   disp [n][dh][dw]; Rt [2][n][12] = composeT outputs (R row-major, t) of source 0 then 1
 *   (md2_so3_compose_fwd); loss_map [n][h][w]; sel_map (NULL ok) = argmin (0/1, -1 automask).
 *   Pullback of sum(d_loss .* loss_map): d_disp [n][dh][dw], d_Rt [2n][12] (each NULL ok).
 * ---------------------------------------------------------------------------------------- */
int md2_automasking_loss(const float* x, int n, int c, int h, int w, int target, int src0,
                         int src1, float* out, void* stream);
/* find_static(dataset, alpha) (src/dtk.jl:51-69), the per-sample part: scores[i] =
 * mean(automasking_loss(ssim, x_i, x_i[target]; source_ids)) for the n triplets of x
 * [n][3][c][h][w]; the dataset filter keeps samples with scores[i] > alpha (md2hip.find_static).
 * workspace: md2_static_scores_workspace_size(n, h, w) bytes of device memory. */
size_t md2_static_scores_workspace_size(int n, int h, int w);
int md2_static_scores(const float* x, int n, int c, int h, int w, int target, int src0, int src1,
                      float* scores, void* workspace, void* stream);
int md2_ssim_fwd(const float* x, const float* y, int n, int c, int h, int w, float* out,
                 void* stream);
int md2_ssim_bwd(const float* x, const float* y, const float* dout, int n, int c, int h, int w,
                 float* dx, float* dy, void* stream);
int md2_backproject_fwd(const float* depth, int n, int w, int h, const float* invK, float* out,
                        void* stream);
int md2_backproject_bwd(const float* dout, int n, int w, int h, const float* invK, float* d_depth,
                        void* stream);
int md2_project_fwd(const float* points, int n, int w, int h, const float* K, const float* R,
                    const float* t, float* out, void* stream);
size_t md2_project_workspace_size(int n, int w, int h);
int md2_project_bwd(const float* points, int n, int w, int h, const float* K, const float* R,
                    const float* t, const float* dout, float* d_points, float* d_R, float* d_t,
                    void* workspace, void* stream);
int md2_grid_sample_border_fwd(const float* x, const float* grid, int n, int c, int hi, int wi,
                               int ho, int wo, float* out, void* stream);
int md2_grid_sample_border_bwd(const float* x, const float* grid, const float* dout, int n, int c,
                               int hi, int wi, int ho, int wo, float* d_grid, float* d_x,
                               void* stream);
size_t md2_smooth_loss_workspace_size(int n, int w, int h);
int md2_smooth_loss_fwd(const float* disp, const float* img, int n, int c, int h, int w,
                        float* loss, void* workspace, void* stream);
int md2_smooth_loss_bwd(const float* disp, const float* img, int n, int c, int h, int w,
                        float dloss, float* d_disp, void* workspace, void* stream);

typedef struct md2_warp_cfg {
  int n, c, width, height;       /* samples, channels, full (target) resolution              */
  int dw, dh;                    /* resolution of the disparity of this scale                */
  float K[9], invK[9];           /* row-major                                                 */
  float min_depth, max_depth;    /* Params                                                    */
  long long x_sample_stride;     /* elements between samples of x                            */
  long long x_frame_stride;      /* elements between frames                                  */
  int target, src0, src1;        /* 0-based frame ids                                        */
} md2_warp_cfg;
size_t md2_warp_photometric_workspace_size(const md2_warp_cfg* cfg);
int md2_warp_photometric_fwd(const md2_warp_cfg* cfg, const float* disp, const float* Rt,
                             const float* x, const float* automask, float* loss_map,
                             signed char* sel_map, void* workspace, void* stream);
int md2_warp_photometric_bwd(const md2_warp_cfg* cfg, const float* disp, const float* Rt,
                             const float* x, const float* automask, const float* d_loss,
                             float* d_disp, float* d_Rt, void* workspace, void* stream);

/* Data pipeline, host code: PNG files (8-bit, non-interlaced gray / RGB / RGBA)
 * decoded on `threads` host threads straight into the uint8 batch layout (lossless: the bytes of
 * FileIO/PNGFiles' N0f8 arrays).
 * md2_load_triplets_u8   Depth10k (src/dtk.jl:29-46): file i = three frames side by side (3W x H
 *                        RGB) -> out [n][3][3][H][W], frame j = columns [jW, (j+1)W); flip[i]
 *                        (NULL = none) mirrors every frame of sample i (FlipX).
 * md2_load_kitti_u8      KittyDataset (src/kitty.jl:45-61): paths[3i+k] = frame k of sample i
 *                        (8-bit gray) -> out [n][3][1][h][w], each imresize'd to (h, w) and kept
 *                        N0f8 (md2hip/data.py imresize), then flipped if flip[i].
 * md2_load_frames_native_u8   decode only, for md2_resize_frames: file i -> out + i * slot_bytes as
 *                        decoded, rows of interleaved pixels [h][w][c] (no resize, no flip, no
 *                        de-interleave), w[i] and h[i] its size.  c = 1 takes gray files, c = 3 RGB
 *                        and RGBA files (the first three channels); any other file, and one with
 *                        w * h * c > slot_bytes, is an error.
 * Host pointers; errors name the offending file. */
int md2_png_info(const char* path, int* width, int* height, int* channels);
int md2_load_triplets_u8(const char* const* paths, int n, int width, int height,
                         const unsigned char* flip, unsigned char* out, int threads);
int md2_load_kitti_u8(const char* const* paths, int n, int height, int width,
                      const unsigned char* flip, unsigned char* out, int threads);
int md2_load_frames_native_u8(const char* const* paths, int n, int c, unsigned char* out,
                              long long slot_bytes, int* w, int* h, int threads);

/* Data pipeline: N0f8 images -> Float32, out[i] = Float32(in[i]) / 255f0, the
 * `Float32.(channelview(x))` of src/dtk.jl:45 / src/kitty.jl:58 -- batches cross PCIe as bytes.
 * in 4-byte aligned, out 16-byte aligned. */
int md2_unorm8_to_float(const unsigned char* in, float* out, long long n, void* stream);

/* ------------------------------------------------------------------------------------------
 * 2-D convolution (Flux Conv / NNlib conv, ∇conv_data, ∇conv_filter) on gfx950 fp32 MFMA.
 * x [n][cin][h][w], w [cout][cin][kh][kw] (cross-correlation; flip Flux kernels), bias [cout],
 * y [n][cout][ho][wo].  reflect=1: NNlib pad_reflect(x, pad) then a valid conv
 * (src/depth_decoder.jl:5; 3x3, stride 1, pad 1 only).  act: 0 none, 1 relu, 2 elu, 3 sigmoid.
 * ---------------------------------------------------------------------------------------- */
typedef struct md2_conv_desc {
  int n, cin, h, w, cout, kh, kw, stride, pad, reflect;
  int act;
} md2_conv_desc;

size_t md2_conv2d_workspace_size(const md2_conv_desc* d);
int md2_conv2d_fwd(const md2_conv_desc* d, const float* x, const float* w, const float* bias,
                   float* y, void* workspace, void* stream);
/* dx = ∇conv_data(dy_pre) where dy_pre is the gradient w.r.t. the pre-activation output. */
int md2_conv2d_dgrad(const md2_conv_desc* d, const float* dy, const float* w, float* dx,
                     void* workspace, void* stream);
/* dw = ∇conv_filter(x, dy_pre), db = sum(dy_pre) (db may be NULL). */
int md2_conv2d_wgrad(const md2_conv_desc* d, const float* x, const float* dy, float* dw,
                     float* db, void* workspace, void* stream);
/* dpre = dout .* act'(out) from the stored post-activation output (n elements). */
int md2_act_backward(const float* out, const float* dout, float* dpre, long long n, int act,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * The three conv passes with the operand forms the train step feeds them (csrc/conv.h TensorIn /
 * TensorOut / ConvShape.cin_w / SplitKDefer); md2_conv2d_* above are the case ops == NULL.
 * Strides count floats; a stride of 0 means contiguous images of the channels that tensor holds.
 *   input  (fwd, wgrad: x)   channels [0, in_c0) of image b at x + (b % in_bdiv) * in_bs0 +
 *          (b / in_bdiv) * in_bhi, channels [in_c0, cin) at in1 + b * in_bs1.  in_c0 = 0: cin
 *          (one tensor); in_bdiv = 0: no frame split.  The two tensors may overlap.
 *   output (fwd: y, dgrad: dx)   rows [0, out_c0) of image b at y + b * out_bs0, the rest at
 *          out1 + b * out_bs1; out_c0 = 0: one tensor.  accumulate = 1: out += result.
 *   wgrad  accumulate = 1: dw += result, db += result.
 *   cin_w  0 or the input channels of w / dw, [cout][cin_w][kh][kw]: the last cin - cin_w channels
 *          of x are zero padding (their dx rows come out zero, their filter gradients are not
 *          produced).  cin_w < cin needs cin % 16 == 0 and cout > 1.
 * Deferral (fwd, dgrad; defer may be NULL): with defer_reduce = 1 a launch that runs split-K into
 * a plain output (one tensor, contiguous, no bias / activation / accumulate, stride 1 for dgrad)
 * skips its reduction: y / dx is NOT written, slab points at [splits][rows][n * pixels] partials
 * inside the workspace that the caller sums in split order.  splits = 0: declined, the output is
 * complete.  Forward only: stats != NULL offers [cout][ceil(n*ho*wo / 256)][2] doubles; when the
 * LDS-halo kernel runs without split-K it writes per 256-pixel tile the fp64 sum and sum of squares
 * of the fp32 values it stores and sets stats_parts to the tile count (0: not written).
 * MD2_EINVAL, checked before any HIP call: a null pointer, in_c0 / out_c0 outside their channel
 * range or below it without a second pointer, a concat split that is not a multiple of 16 on a
 * cin % 16 == 0 forward, an output stride smaller than its channels, cin_w > cin, cin_w on a
 * cout = 1 conv or with cin % 16 != 0, stats without defer, db_part without db or with
 * db_parts < 1, workspace_bytes < md2_conv2d_ex_workspace_size.
 * ---------------------------------------------------------------------------------------- */
typedef struct md2_conv_operands {
  const float* in1;
  float* out1;
  long long in_bs0, in_bs1, in_bhi;
  long long out_bs0, out_bs1;
  int in_c0, in_bdiv;
  int out_c0, accumulate;
  int cin_w;
} md2_conv_operands;

typedef struct md2_conv_defer {
  const float* slab; /* out */
  int defer_reduce;  /* in  */
  int splits;        /* out */
  int stats_parts;   /* out */
} md2_conv_defer;

size_t md2_conv2d_ex_workspace_size(const md2_conv_desc* d, const md2_conv_operands* ops);
int md2_conv2d_fwd_ex(const md2_conv_desc* d, const md2_conv_operands* ops, const float* x,
                      const float* w, const float* bias, float* y, double* stats,
                      md2_conv_defer* defer, void* workspace, size_t workspace_bytes, void* stream);
int md2_conv2d_dgrad_ex(const md2_conv_desc* d, const md2_conv_operands* ops, const float* dy,
                        const float* w, float* dx, md2_conv_defer* defer, void* workspace,
                        size_t workspace_bytes, void* stream);
/* db_part [cout][db_parts]: bias-gradient partials from md2_act_backward_bias (the pass over dy is
 * then skipped); NULL: summed from dy. */
int md2_conv2d_wgrad_ex(const md2_conv_desc* d, const md2_conv_operands* ops, const float* x,
                        const float* dy, float* dw, float* db, const float* db_part, int db_parts,
                        void* workspace, size_t workspace_bytes, void* stream);
/* md2_act_backward over [n][c][hw] planes (hw % 4 == 0, n*c*hw < 2^31) fused with the per-channel
 * partial sums of dpre: part [c][md2_act_bias_parts(c, n, hw)].  dpre may alias dout. */
int md2_act_bias_parts(int c, int n, long long hw);
int md2_act_backward_bias(const float* out, const float* dout, float* dpre, int n, int c,
                          long long hw, int act, float* part, void* stream);
/* Kernel family of the last conv pass launched by the calling thread ("" before the first): px,
 * px2, px3, px16, halo, halo2d, halo_rfl_dgrad, halo_s2, stem_s2d, head_batched, head_fallback,
 * whalo, wgrad16, wgrad_px3:<BM>x<BN>c<CW>, wgrad_tile:<BM>x<BN>c<CW>, stem_wgrad_s2d, stem_wgrad.
 * The string is owned by the library and changes with the next conv call of the thread. */
const char* md2_conv_last_kernel(void);

/* ------------------------------------------------------------------------------------------
 * Pooling / resampling layers of the networks, [n][c][h][w] planes.
 * MaxPool((3,3), pad=1, stride=2) of the ResNet.jl stem: y [n][c][ho][wo] with
 * ho = (h+1)/2, wo = (w+1)/2, arg = window index kh*3+kw of the first maximum (uint8, kept for
 * the pullback).  upsample_bilinear(x, (2,2)), align_corners (src/depth_decoder.jl:18-19):
 * y [n][c][2h][2w]; the backward is its exact adjoint dx [n][c][h][w].
 * ---------------------------------------------------------------------------------------- */
int md2_maxpool3s2_fwd(const float* x, int n, int c, int h, int w, float* y, unsigned char* arg,
                       void* stream);
int md2_maxpool3s2_bwd(const float* dy, const unsigned char* arg, int n, int c, int h, int w,
                       float* dx, void* stream);
int md2_upsample2_fwd(const float* x, int n, int c, int h, int w, float* y, void* stream);
int md2_upsample2_bwd(const float* dy, int n, int c, int h, int w, float* dx, void* stream);
/* md2_maxpool3s2_bwd with the addend of the stem backward: dx += skip[e - skip_lo] over the flat
 * elements [skip_lo, skip_hi) of dx (whole planes: both multiples of h*w; even w).  skip == NULL:
 * md2_maxpool3s2_bwd.  MD2_EINVAL before any HIP call: a null dy / arg / dx, a size < 1, a range
 * that is not 0 <= skip_lo <= skip_hi <= n*c*h*w on plane boundaries, an odd w with a skip. */
int md2_maxpool3s2_bwd_ex(const float* dy, const unsigned char* arg, int n, int c, int h, int w,
                          float* dx, const float* skip, long long skip_lo, long long skip_hi,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm of the encoder (Flux BatchNorm in trainmode!: batch mean, biased variance, eps) with
 * the operand forms the train step feeds it (csrc/nn.h BNApplyFused / BNBwd), on caller-owned
 * device buffers [n][c][h][w].  These calls launch the executor's kernels; where the executor
 * reads its MD2_FUSE_* switches, the route is an argument here.  Additive: MD2_ABI_VERSION is
 * unchanged.
 *   route     0: the executor's choice -- one kernel where a channel fits in a block (h*w % 4 == 0
 *             and n*h*w <= 8192) and the statistics are the call's own, else two passes;
 *             1: two passes (partials, then finalise + apply); 2: one kernel (MD2_EINVAL where
 *             the channel does not fit, with caller partials, or with pool outputs).
 *   forward   out = act(gamma*(y-mean)*invstd + beta [+ gamma2*(y2-mean2)*invstd2 + beta2] [+ res]).
 *             The input is y, or slab [splits][c][n*h*w] (a conv's split-K partials) summed in
 *             split order into y_out.  The statistics are the call's own, or caller partials part
 *             [c][parts][2] (fp64 sum and sum of squares; a conv epilogue's per-tile form), with
 *             collapse = 1 first reduced to one partial per channel.  The second branch (y2) always
 *             takes its own statistics pass.  mean / invstd (and mean2 / invstd2) are written;
 *             run_mean / run_var (both or neither) are updated with momentum and the unbiased
 *             variance.  pool_y / pool_arg (both or neither; relu = 1, no y2 / res, even h and w)
 *             select the stem tail: out and its 3x3/2/pad-1 max pool [n][c][h/2][w/2] in one pass.
 *   backward  g = (dout [+ skip[e - skip_lo] over flat elements [skip_lo, skip_hi)]) gated by
 *             mask > 0 (the BN+ReLU output) or by the ReLU of BN(y) re-derived with mbeta;
 *             dbeta = sum g, dgamma = sum g*xhat, dy = gamma*invstd*(g - dbeta/L - xhat*dgamma/L);
 *             dres = g (dres_accumulate: += g).  The input is dout, or slab summed in split order;
 *             two passes write that sum to dout_w, one kernel leaves dout_w untouched.
 * Tensors are 16-byte aligned when h*w % 4 == 0 (float4 units; scalar units otherwise).
 * MD2_EINVAL, checked before any HIP call: a null descriptor / operand struct / required pointer;
 * a size < 1 or n*c*h*w >= 2^31; route outside 0..2, collapse / relu / dres_accumulate outside
 * 0..1; route = 2 where the channel does not fit; both or neither of y and slab (dout and slab);
 * slab without splits >= 1 or without y_out (dout_w on two passes); slab with caller partials, a
 * mask or a skip; collapse without caller partials; parts < 1; y2 without gamma2 / beta2 / mean2 /
 * invstd2; one of run_mean / run_var alone; mask together with mbeta; a skip with h*w % 4 != 0,
 * outside 0 <= skip_lo <= skip_hi <= n*c*h*w, or with skip_lo / skip_hi not a multiple of 4 (the
 * kernels read it in float4 units); pool outputs with odd h or w, y2, res, relu = 0 or one of the
 * two alone; a misaligned tensor; a workspace smaller than md2_bn_ex_workspace_size or not
 * 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
typedef struct md2_bn_desc {
  int n, c, h, w;
  float eps, momentum;
  int route;
  int collapse;
} md2_bn_desc;

typedef struct md2_bn_info { /* out: what the call launched */
  int family;    /* 1 two passes, 2 one kernel, 3 stem tail with the max pool */
  int parts;     /* statistics / gradient partials per channel (0: one kernel) */
  int fin_parts; /* partials per channel the apply's finalise walks (1 after a collapse) */
  int upt;       /* units per thread of the apply pass (0: one kernel) */
  int vec;       /* 1: float4 units, 0: scalar units */
} md2_bn_info;

typedef struct md2_bn_fwd_operands {
  const float* y;
  const float* slab;
  float* y_out;
  const double* part;
  const float* gamma;
  const float* beta;
  float* mean;
  float* invstd;
  float* run_mean;
  float* run_var;
  const float* y2;
  const float* gamma2;
  const float* beta2;
  float* mean2;
  float* invstd2;
  const float* res;
  float* out;
  float* pool_y;
  unsigned char* pool_arg;
  int splits, parts;
  int relu;
} md2_bn_fwd_operands;

typedef struct md2_bn_bwd_operands {
  const float* dout;
  const float* slab;
  float* dout_w;
  const float* mask;
  const float* y;
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* mbeta;
  float* dgamma;
  float* dbeta;
  float* dy;
  float* dres;
  const float* skip;
  long long skip_lo, skip_hi;
  int splits, dres_accumulate;
} md2_bn_bwd_operands;

/* bytes of workspace either call needs for this descriptor (0: invalid descriptor) */
size_t md2_bn_ex_workspace_size(const md2_bn_desc* d);
/* 1 where a channel of [n][c][h][w] fits in a block of the one-kernel passes, else 0 */
int md2_bn_channel_fits(int n, long long hw);
int md2_bn_forward_ex(const md2_bn_desc* d, const md2_bn_fwd_operands* o, md2_bn_info* info,
                      void* workspace, size_t workspace_bytes, void* stream);
int md2_bn_backward_ex(const md2_bn_desc* d, const md2_bn_bwd_operands* o, md2_bn_info* info,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * MPI mode (src/model.jl:1-55; forward only upstream).  md2_mpi_embed_features
 * builds the DepthDecoder input of one feature level: out [n*num_bins][c + 2L+1][h][w] with
 * image b*num_bins + p = cat(feat[b], repeat(embed(bins[b][p]), h, w)); embed(x) = [x, sin(2^i x),
 * cos(2^i x) for i in 0:L-1] (src/model.jl:4-15); feat[b] at feat + b*sample_stride.
 * md2_concat_channels: cat(a, b; dims=3) for [n][ca][hw] and [n][cb][hw] (BranchBlock skip).
 * ---------------------------------------------------------------------------------------- */
int md2_mpi_embed_features(const float* feat, long long sample_stride, int n, int c, int h, int w,
                           const float* bins, int num_bins, int L, float* out, void* stream);
int md2_concat_channels(const float* a, int ca, const float* b, int cb, int n, long long hw,
                        float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * MINE plane rendering of the MPI mode (src/render.jl:21-114), forward (the reference defines
 * no pullback).  Arrays are the Julia arrays' bytes (column-major dims listed first):
 *   rgb (W,H,3,N,B)   sigma (W,H,1,N,B)   xyz (3,W,H,N,B)   disparity/depth (N,B)
 *   pose [B][6] = (rvec, tvec) of Pose(rvec (3,B), tvec (3,B))   K, invK 3x3 row-major (host)
 * The reference's semantics are reproduced as written (valid mask = chained comparison
 * u < W*u >= 0, grid normalised (u + 0.5)/(W/2) with no -1, last plane distance 1e3,
 * transmittance over T + 1e-6); see DESIGN.md "MINE rendering".
 * md2_mine_src_xyz   get_src_xyz_from_plane_disparity(create_meshgrid(H,W), disparity, invK)
 *                    (render.jl:21-30) -> xyz (3,W,H,N,B)
 * md2_mine_tgt_xyz   get_tgt_xyz_from_plane_disparity(xyz_src, pose) (render.jl:51-64)
 * md2_mine_sample    sample(src, depth_src, pose, K, K_inv) (render.jl:66-94): src (W,H,c,N*B),
 *                    depth (N,B) -> out (W,H,c,N*B), valid (W*H, N*B) as 0/1 floats
 * md2_plane_volume_rendering  plane_volume_rendering(rgb, sigma, xyz) (render.jl:32-49) ->
 *                    rgb_out (W,H,3,B), transparency_acc (W,H,1,N,B), weights (W,H,1,N,B)
 * md2_render_tgt_rgb_depth  render_tgt_rgb_depth(rgb, sigma, disparity, xyz_tgt, pose, invK, K)
 *                    (render.jl:96-114), one fused kernel, N <= 512 -> rgb (W,H,3,B),
 *                    depth (W,H,1,N,B), mask (W,H,1,1,B) (plane counts of the valid mask)
 * ---------------------------------------------------------------------------------------- */
int md2_mine_src_xyz(const float* disparity, int n_planes, int batch, int h, int w,
                     const float* invK, float* xyz, void* stream);
int md2_mine_tgt_xyz(const float* xyz_src, const float* pose, int n_planes, int batch, int h, int w,
                     float* xyz_tgt, void* stream);
int md2_mine_sample(const float* src, int c, const float* depth, const float* pose, int n_planes,
                    int batch, int h, int w, const float* K, const float* invK, float* out,
                    float* valid, void* stream);
int md2_plane_volume_rendering(const float* rgb, const float* sigma, const float* xyz, int n_planes,
                               int batch, int h, int w, float* rgb_out, float* transparency_acc,
                               float* weights, void* stream);
int md2_render_tgt_rgb_depth(const float* rgb, const float* sigma, const float* disparity,
                             const float* xyz_tgt, const float* pose, const float* invK,
                             const float* K, int n_planes, int batch, int h, int w, float* rgb_out,
                             float* depth, float* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * Model: Model(ResidualNetwork(arch), DepthDecoder(embedding_levels=0), PoseDecoder) in mono
 * mode (src/model.jl:24-70), train_loss (src/training.jl:21-78), its pullback, Flux ADAM.
 * Parameters / gradients are CALLER-owned flat fp32 device vectors; their order is the table
 * of md2_arch_param_info (conv weights cross-correlation [cout][cin][kh][kw], then bias;
 * BatchNorm gamma, beta).  x is [batch][3][c][h][w] (Julia (W,H,C,3,N)).
 * ---------------------------------------------------------------------------------------- */
typedef struct md2_model_cfg {
  int arch;                             /* ResidualNetwork depth: 18, 34 or 50              */
  int in_channels;                      /* 1 (grayscale) or 3                                */
  int batch;                            /* samples per step (triplets)                       */
  int width, height;                    /* Params.target_size (multiples of 32)              */
  int n_levels;                         /* length(scale_levels)                              */
  int scale_levels[MD2_MAX_SCALES];     /* DepthDecoder scale_levels in 1:5, strictly increasing
                                           (repeated / decreasing: MD2_ENOTSUP)               */
  float K[9], invK[9];                  /* TrainCache.K / invK, row-major                    */
  float min_depth, max_depth, disparity_smoothness;   /* Params                              */
  float scales[MD2_MAX_SCALES];         /* TrainCache.scales                                 */
  int automasking;                      /* Params.automasking                                */
  int target, src0, src1;               /* 0-based frame ids in 0:2 (TrainCache target_id /
                                           source_ids minus 1)                                */
  int embedding_levels;                 /* DepthDecoder(; embedding_levels): 0 = mono mode (the
                                           measured step); 2L+1 (21) = MPI mode, model.jl:31-55 */
  int num_bins;                         /* MPI mode: disparity planes per sample (model.jl:31)  */
} md2_model_cfg;

typedef struct md2_model md2_model;

/* host-only queries of the flat parameter table (no device needed) */
int md2_arch_param_count(const md2_model_cfg* cfg, long long* n_entries, long long* n_elems);
int md2_arch_param_info(const md2_model_cfg* cfg, int idx, char* name, int name_len, int* ndim,
                        int* shape4, long long* offset);

int md2_model_create(const md2_model_cfg* cfg, float* params, float* grads, md2_model** out);
int md2_model_destroy(md2_model* m);
size_t md2_model_device_bytes(md2_model* m);
/* re-pack conv weights after the caller changed `params` directly */
int md2_model_repack(md2_model* m, void* stream);
/* Flux-layout flat vectors (the order of md2_arch_param_info; conv weights as Flux stores them:
 * (kw,kh,cin,cout) TRUE-convolution kernels = C-order [cout][cin][kh][kw] with both spatial axes
 * reversed w.r.t. the library's cross-correlation).  set: copies into the model's params (taps
 * flipped) and re-packs; get: params -> Flux layout; get_grads: the flat gradient -> Flux layout
 * (what Zygote returns for Flux.params).  `flux` must not alias the model's vectors. */
int md2_model_set_params(md2_model* m, const float* flux, void* stream);
int md2_model_get_params(md2_model* m, float* flux, void* stream);
int md2_model_get_grads(md2_model* m, float* flux, void* stream);
/* train_loss pullback with an upstream cotangent (ChainRulesCore rrule): after
 * md2_model_forward_loss and before backward segment 0, scale the loss-tail gradients by dloss */
int md2_model_loss_cotangent(md2_model* m, float dloss, void* stream);
/* forward (encoder on 3*batch frames, decoder on targets, poses) + train_loss value + the
 * loss-tail pullback; terms: [n_levels][2] or NULL.  With cfg.automasking, auto_loss [batch][h][w]
 * is the caller's automasking_loss, or NULL: the library computes it from x (md2_automasking_loss). */
int md2_model_forward_loss(md2_model* m, const float* x, const float* auto_loss, float* loss,
                           float* terms, void* stream);
/* backward in segments (0 = pose+depth decoders, 1..4 = layer4..layer1, 5 = stem); after
 * segment k the flat gradient range [off, off+len) is final (bucket for the DP all-reduce) */
/* (m)(x, source_ids, target_id) -> (disparities, poses) (src/model.jl:31-55; called at
 * src/training.jl:26 and, bare, scripts/script.jl:93): the forward only -- encoder, DepthDecoder,
 * PoseDecoder, no loss tail.  disp[level] ([batch*num_bins][h][w]) and *pose ([2*batch][6]) are
 * set to the model's output buffers (either may be NULL), the values md2_model_forward_loss would
 * produce for the same x, bit for bit.  A backward after it needs the outputs' cotangents. */
int md2_model_forward(md2_model* m, const float* x, const float** disp, const float** pose,
                      void* stream);
/* The pullback of md2_model_forward from caller cotangents (a host that differentiates its own
 * loss, e.g. the reference's train_loss through Zygote): d_disp[level] = d L / d disparity of that
 * level, laid out as the outputs (NULL array or entry: zero), d_pose [2*batch][6] (NULL: zero).
 * md2_model_set_cotangents only installs them -- the backward segments then run as after
 * md2_model_forward_loss (DP buckets unchanged); md2_model_backward_from installs them and runs
 * every segment.  The flat gradient equals the fused path's bit for bit when the cotangents equal
 * the loss tail's own (md2_loss_fwd_bwd with sigmoid_grad = 0). */
int md2_model_set_cotangents(md2_model* m, const float* const* d_disp, const float* d_pose,
                             void* stream);
int md2_model_backward_from(md2_model* m, const float* const* d_disp, const float* d_pose,
                            void* stream);
int md2_model_num_segments(md2_model* m);
int md2_model_backward_segment(md2_model* m, int k, long long* off, long long* len,
                               void* stream);
/* update!(ADAM(lr, (beta1, beta2)), θ, ∇) on any flat fp32 device vector of n elements (Flux
 * ADAM, eps on the bias-corrected sqrt(v)); `step` >= 1 counts updates of this vector; the
 * gradient is scaled by grad_scale first (1/world for a summed DP gradient).  The free-variable
 * loop of slow_depth (src/simple_depth.jl:20-43) uses it directly. */
int md2_adam(float* p, const float* g, float* adam_m, float* adam_v, long long n, float lr,
             float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/* Flux ADAM step over the flat vectors (bias correction with `step` >= 1); gradients are
 * multiplied by grad_scale first (1/world_size after a sum all-reduce); re-packs weights */
int md2_model_adam(md2_model* m, float* adam_m, float* adam_v, float lr, float beta1,
                   float beta2, float eps, int step, float grad_scale, void* stream);
/* The update of ONE backward segment's parameters (the range model_backward_segment returned):
 * ADAM as md2_model_adam over that range + the re-pack of its conv weights, enqueued on the
 * executor's own update stream ordered after everything enqueued on `stream` so far -- called
 * right after md2_model_backward_segment(segment) (a DP caller: on the stream its bucket's
 * all-reduce ran on) it runs beside the remaining backward.  Every segment of a step takes the
 * same `step`.  md2_model_adam_join makes `stream` wait for all pending segment updates
 * (md2_model_forward_loss, eval_disparity, md2_model_adam and the parameter copies join first). */
int md2_model_adam_segment(md2_model* m, int segment, float* adam_m, float* adam_v, float lr,
                           float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
int md2_model_adam_join(md2_model* m, void* stream);
/* forward_loss + every backward segment + ADAM (single-GPU step).  By default ONE update runs
 * after the last segment; MD2_SEG_UPDATE=1 opts into each segment's update beside the remaining
 * backward (md2_model_adam_segment; measured 2% slower at N=1) */
int md2_model_train_step(md2_model* m, const float* x, const float* auto_loss, float* adam_m,
                         float* adam_v, float lr, int step, float* loss, void* stream);
/* md2_model_train_step as ONE captured hipGraph (forward, loss, every backward segment, ADAM,
 * weight repack): captured on the executor's own stream at the first call and again when adam_m,
 * adam_v, lr or the presence of auto_loss change; x / auto_loss are copied into executor-owned
 * buffers each call (any pointer may be passed), the loss is copied out; `step` may jump (the
 * device step counter is re-set).  Same arithmetic, same results as md2_model_train_step. */
int md2_model_train_step_graph(md2_model* m, const float* x, const float* auto_loss, float* adam_m,
                               float* adam_v, float lr, int step, float* loss, void* stream);
/* ------------------------------------------------------------------------------------------
 * Data parallelism over RCCL (xGMI), one process (rank) per GPU -- SURVEY.md 8(e).  The
 * reference has no collectives; these replace the torch.distributed plumbing so a Julia host
 * needs only this library.  RCCL is dlopen'ed on first use (MD2_ENOTSUP if absent).
 * md2_comm_get_unique_id: rank 0 creates the 128-byte id and ships it to the other ranks (file,
 * MPI, a TCP store ...); md2_comm_init then joins (collective over all ranks) on `device` (the
 * caller's current device is restored before it returns).
 * md2_model_backward_allreduce: every backward segment on `stream`, each followed by the RCCL
 * sum of its (final) gradient range on the communicator's own stream -- bucketed, overlapped with
 * the rest of the backward; `stream` waits for all buckets before returning.  comm == NULL:
 * plain backward.  md2_model_train_step_dp: forward_loss + that + ADAM with grad_scale 1/nranks
 * (one update after the last bucket by default; MD2_SEG_UPDATE=1: each bucket's ADAM + re-pack
 * on the update stream right after its all-reduce).
 * ---------------------------------------------------------------------------------------- */
#define MD2_COMM_ID_BYTES 128
typedef struct md2_comm md2_comm;
int md2_comm_get_unique_id(char* id);
int md2_comm_init(int rank, int nranks, const char* id, int device, md2_comm** out);
int md2_comm_destroy(md2_comm* comm);
/* rank and size as the RCCL communicator reports them (ncclCommUserRank / ncclCommCount) */
int md2_comm_rank(const md2_comm* comm, int* rank, int* nranks);
/* all-reduces enqueued through this communicator and their payload bytes, cumulative */
int md2_comm_stats(const md2_comm* comm, long long* calls, long long* bytes);
/* in-place sum all-reduce of n floats, on `stream` (RCCL's ordering) */
int md2_comm_allreduce_sum(md2_comm* comm, float* buf, long long n, void* stream);
int md2_model_backward_allreduce(md2_model* m, md2_comm* comm, void* stream);
int md2_model_train_step_dp(md2_model* m, md2_comm* comm, const float* x, const float* auto_loss,
                            float* adam_m, float* adam_v, float lr, float beta1, float beta2,
                            float eps, int step, float* loss, void* stream);

/* MPI mode (embedding_levels > 0; src/model.jl:31-55, batch 1): the decoder runs on
 * num_bins*batch plane images, image n*num_bins + p = cat(target features of sample n,
 * repeat(embed(bins[n][p]), h, w)); the loss treats the planes as the batch, each warped with
 * its sample's poses against its sample's frames (the broadcast of src/training.jl:42-56); the
 * backward block-sums the planes' feature gradients (_repeat pullback, src/repeat.jl:44-53).
 * bins [batch][num_bins] (device or host): uniformly_sample_disparity_from_linspace_bins's draw
 * (src/model.jl:17-21, CUDA.rand there), used by every following forward until set again. */
int md2_model_set_disparity_bins(md2_model* m, const float* bins, void* stream);

/* device pointers of the last forward: disparities per level ([batch*num_bins][h][w] in MPI
 * mode) and poses [2*batch][6] */
int md2_model_outputs(md2_model* m, const float** disp, int* w, int* h, const float** pose);
/* The five encoder stage outputs of the last forward (device memory owned by the model):
 * feat[k] = [3n frame-major images][c[k]][h[k]][w[k]] (image l*n + i = frame l of sample i). */
int md2_model_features(md2_model* m, const float** feat, int* c, int* h, int* w);
/* HIP-event profiling of the hot kernels on the model's stream (bench roofline): categories
 * 0 = zero-padded 3x3 convs (encoder + pose decoder; fwd/dgrad/wgrad incl. their split-K
 * reductions, work = algorithmic FLOP), 1 = other convs,
 * 2 = fused warp+SSIM photometric kernel (work = algorithmic HBM bytes).
 * out[cat*3 + {0,1,2}] = {total ms, total work, launches}; read() clears. */
#define MD2_PROF_NCAT 3
int md2_model_set_profiling(md2_model* m, int on);
int md2_model_profile_read(md2_model* m, double* out, int ncat);
/* the same events one record at a time (per-layer table): ms, work, category and a tag ("fwd
 * 3x3/1 64->64 32x104 n36" for a conv: pass, kernel/stride[r = reflect pad], channels, input
 * size, images); up to `max` records, *count set; clears like md2_model_profile_read. */
int md2_model_profile_records(md2_model* m, int max, double* ms, double* work, int* cat, char* tags,
                              int tag_len, int* count);
/* Diagnostics (parity tests): named internal buffers of the last forward / backward, by index
 * 0..count-1 (MD2_EINVAL past the end): encoder activations ("stem.y", "stem.out",
 * "maxpool.out", "maxpool.arg" = window index kh*3+kw as uint8, "layer<s>.<b>.conv<k>.y",
 * "...relu1", "....out", "....down.y"), block-output gradients "....d_out", pose activations
 * "pose.sq", "pose.conv1", "pose.conv2", decoder skip gradients "d_skip<f>", "d_mp", "d_f0".
 * Images are in the encoder's frame-major order (image = frame*batch + n).
 * dims = {images, channels, height, width, dtype (0 float32, 1 uint8)}; *name valid until the
 * next call. */
int md2_model_debug_tensor(md2_model* m, int index, const char** name, const void** ptr,
                           int* dims);
/* eval_disparity (src/model.jl:63) on x [n][c][h][w], n <= batch; disp: per-level pointers.
 * It reuses the executor's activation buffers: a pending forward_loss is discarded and a later
 * md2_model_backward_segment returns MD2_ESTATE until the next forward_loss. */
int md2_model_eval_disparity(md2_model* m, const float* x, int n, const float** disp,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm running statistics as model state, and test mode (Flux testmode!).
 * Every train-mode forward moves the running mean / variance of each BatchNorm (Flux: momentum
 * 0.1, variance with the m/(m-1) correction; initial state 0 / 1).  They form ONE flat fp32 vector:
 * per BatchNorm, in the order of its gamma entry in md2_arch_param_info, C means then C variances
 * (n_elems = 2 * sum of C).  get / set take device pointers and join pending ADAM segments like
 * md2_model_get_params; set refuses a negative variance or a non-finite entry with MD2_EINVAL
 * (checked on the device; the state is then unchanged).
 * md2_model_set_testmode(m, 1): md2_model_eval_disparity and md2_model_forward normalise with the
 * running statistics (which they no longer modify), each BatchNorm folded into the conv before it
 * (w' = w * s, bias t; s = gamma / sqrt(var + 1e-5), t = beta - mean * s); a sample's result no
 * longer depends on the rest of its batch.  Every training entry point (forward_loss,
 * set_cotangents, backward_*, adam*, train_step*, loss_cotangent) returns MD2_ESTATE until
 * md2_model_set_testmode(m, 0), which restores the train-mode state exactly (the train-mode packed
 * weights are never overwritten; the folded packs are a second set, allocated at the first switch
 * and counted in md2_model_device_bytes from then on).  md2_model_repack, md2_model_set_params and
 * md2_model_set_bn_stats re-fold while test mode is on.
 * ---------------------------------------------------------------------------------------- */
int md2_arch_bn_stat_count(const md2_model_cfg* cfg, long long* n_bn, long long* n_elems);
int md2_model_get_bn_stats(md2_model* m, float* out, void* stream);
int md2_model_set_bn_stats(md2_model* m, const float* in, void* stream);
int md2_model_set_testmode(md2_model* m, int on, void* stream);
int md2_model_testmode(md2_model* m);

/* ------------------------------------------------------------------------------------------
 * Depth evaluation: the Monodepth2 / Eigen protocol (median scaling, crop, seven error metrics)
 * of a batch of predicted disparities against ground-truth depth, entirely on the device.
 * Additive: MD2_ABI_VERSION is unchanged.
 *
 * For each image i of the n: disp[i] is [h][w] fp32, the network's sigmoid disparity (any level);
 * gt[i] is [gt_h][gt_w] fp32 ground-truth depth, where 0 (or anything outside the evaluation
 * range) means "no measurement".  All images of one call share gt_h x gt_w.
 *  1. Scaled disparity  sd = disp * (1/min_depth - 1/max_depth) + 1/max_depth  (the inner term of
 *     disparity_to_depth, src/utils.jl:179-183).
 *  2. sd is resized to gt_h x gt_w by half-pixel-centre bilinear interpolation: at gt pixel (Y, X)
 *     sx = clamp((X + 0.5) * w / gt_w - 0.5, 0, w - 1), sy alike (coordinates in fp64); the
 *     neighbours are floor(sx) and min(floor(sx) + 1, w - 1).  When h == gt_h and w == gt_w the
 *     sample is the input value itself.  pred = 1 / sd_resized.
 *  3. Mask: eval_min < gt < eval_max (strict; false for NaN) and y0 <= Y < y1, x0 <= X < x1.
 *     A masked pixel whose pred is not finite or not > 0 is a BAD pixel: counted in n_bad and
 *     excluded from everything below.  count = the remaining pixels.
 *  4. ratio = median(gt[mask]) / median(pred[mask]) with median_scaling, else cfg.scale.  The
 *     median is exact (as NumPy's): the middle element for an odd count, 0.5f * (lo + hi) of the
 *     two middle elements, in fp32, for an even count.  med_gt and med_pred are reported either way.
 *  5. p = clamp(pred * ratio, eval_min, eval_max).
 *  6. Over the mask, with g = gt:  abs_rel = mean(|g - p| / g),  sq_rel = mean((g - p)^2 / g),
 *     rmse = sqrt(mean((g - p)^2)),  rmse_log = sqrt(mean((ln g - ln p)^2)),
 *     a_k = mean(max(g / p, p / g) < 1.25^k), k = 1, 2, 3.
 *  7. count == 0: the ten metrics are NaN and count = 0 (no fault).
 * Per-pixel arithmetic and partial sums are fp32; block partials are combined in fp64.  Results are
 * BITWISE REPRODUCIBLE from call to call: fixed grid, fixed-order reductions, integer atomics only.
 * The call enqueues on `stream` and never synchronises with the host; it clears what it needs of
 * the workspace itself (md2_depth_eval_workspace_size(cfg) bytes of device memory, any content).
 * MD2_EINVAL (checked before any HIP call): a null pointer, n outside 1..65535, a size < 1,
 * gt_h * gt_w > 2^24 (h * w > 2^30), a crop that is empty or outside the ground truth,
 * min_depth >= max_depth, eval_min >= eval_max, a non-positive or non-finite bound, or
 * median_scaling == 0 with a scale that is not positive and finite.
 * ---------------------------------------------------------------------------------------- */
typedef struct md2_depth_eval_cfg {
  int n, h, w;            /* disparity batch and size                     */
  int gt_h, gt_w;         /* ground-truth size                            */
  int y0, y1, x0, x1;     /* crop rectangle in gt pixels, half-open       */
  float min_depth, max_depth;   /* disparity_to_depth range (0.1, 100)   */
  float eval_min, eval_max;     /* valid gt range, clamp range (1e-3, 80) */
  int median_scaling;     /* 1: per-image median ratio; 0: use scale      */
  float scale;
} md2_depth_eval_cfg;

#define MD2_DEPTH_EVAL_NMETRIC 10
/* metrics[i] = {abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, med_gt, med_pred}
   counts[i]  = {count, n_bad} */
size_t md2_depth_eval_workspace_size(const md2_depth_eval_cfg* cfg);   /* 0 for an invalid cfg */
int md2_depth_eval(const md2_depth_eval_cfg* cfg, const float* disp, const float* gt,
                   float* metrics, int* counts, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ground-truth depth maps from LiDAR scans, and the flip post-processing of disparities -- the two
 * steps around md2_depth_eval in a Monodepth2-style evaluation.  Additive: MD2_ABI_VERSION is
 * unchanged.
 *
 * md2_lidar_depth rasterises n Velodyne scans into n depth maps [h][w]: project, round, "minus
 * one", nearest point wins.  Scan i is points[offsets[i] .. offsets[i+1]-1], four fp32 values per
 * point (x, y, z, reflectance; the last is ignored), points 16-byte aligned; p = P[i] is its
 * row-major 3x4 velodyne -> image matrix (KITTI: P_rect * R_rect * [R|T]).  offsets and P are HOST
 * arrays, read before the call returns.  For each point (X, Y, Z), all arithmetic in fp32, each
 * operation rounded on its own (no fused multiply-add):
 *  1. x = ((p0*X + p1*Y) + p2*Z) + p3;  y likewise from p4..p7;  zc from p8..p11.
 *  2. u = x / zc, v = y / zc, correctly rounded divisions.
 *  3. ix = (int)rintf(u) - 1, iy = (int)rintf(v) - 1 (ties to even; the -1 is the KITTI devkit's
 *     1-based pixel convention, which Monodepth2 keeps).
 *  4. The stored value s = vel_depth ? X : zc.
 *  5. The point is DROPPED if forward_only && X < 0; or s is not finite and > 0; or zc is not finite
 *     and > 0; or u or v is not finite; or (ix, iy) is outside [0, w) x [0, h) -- tested on the
 *     rounded floats, before the conversion to int, so a huge u cannot wrap into the image.
 *  6. depth[i][iy][ix] = the minimum s over the points that land there; a pixel no point lands in
 *     is 0.0f ("no measurement", as md2_depth_eval reads it).
 *  7. counts[i] = {points not dropped, pixels != 0}; counts may be NULL.
 * An empty scan (offsets[i] == offsets[i+1]) gives an all-zero map.  Two departures from
 * Monodepth2's generate_depth_map: that script multiplies a float64 matrix with float32 points,
 * and lets a negative depth win the minimum before zeroing it; here everything is fp32 and a
 * non-positive value never competes.  To rasterise at a size other than the camera's, scale rows
 * 0 and 1 of P.
 * The minimum is an integer atomicMin on the bit pattern (positive finite floats order as unsigned
 * integers) and the counts are integer atomics, so the result is BITWISE REPRODUCIBLE and
 * independent of the order the points arrive in.  The call enqueues a fill, a scatter pass and a
 * finishing pass on `stream`; it allocates nothing, needs no workspace and never synchronises with
 * the host.  offsets and P ride in the scatter kernel's argument block (3.3 KB at 64 scans: the
 * reason for the cap; callers chunk larger batches).
 * MD2_EINVAL (checked before any HIP call): a null cfg, offsets, P or depth; null points unless
 * offsets[n] == 0; points not 16-byte aligned; n outside 1..MD2_LIDAR_MAX_SCANS; h or w < 1 or
 * h * w > 2^24; offsets[0] < 0, a decreasing offset or offsets[n] > 2^27; a non-finite entry of P;
 * forward_only or vel_depth not 0 or 1.
 *
 * md2_disp_post_process blends the disparity of a frame, disp [n][h][w], with the network's output
 * for the horizontally mirrored frame, disp_flipped (as produced: NOT mirrored back), as Monodepth
 * and Monodepth2 do for their "+pp" rows.  At (y, x), in fp32 in this order without contraction:
 *   l = disp[y][x],  r = disp_flipped[y][w-1-x],  t(x) = w > 1 ? (float)x / (float)(w-1) : 0,
 *   ml = 1 - fminf(fmaxf(20 * (t(x) - 0.05f), 0), 1),  mr = the same at w-1-x,
 *   out = (mr*l + ml*r) + ((1 - ml) - mr) * (0.5f * (l + r)).
 * out may alias disp; it must not alias disp_flipped (MD2_EINVAL when the pointers are equal, as
 * for a null pointer or a size < 1).
 * ---------------------------------------------------------------------------------------- */
#define MD2_LIDAR_MAX_SCANS 64
typedef struct md2_lidar_cfg {
  int n;               /* scans = depth maps, 1..MD2_LIDAR_MAX_SCANS                    */
  int h, w;            /* depth-map size                                               */
  int forward_only;    /* 1: drop points with x_velo < 0 (Monodepth2)                  */
  int vel_depth;       /* 1: store x_velo instead of the camera z                      */
} md2_lidar_cfg;
int md2_lidar_depth(const md2_lidar_cfg* cfg,
                    const float* points,        /* device [total][4]: x, y, z, reflectance (ignored) */
                    const long long* offsets,   /* HOST [n+1]: scan i = points offsets[i] .. offsets[i+1]-1 */
                    const float* P,             /* HOST [n][12]: row-major 3x4 velodyne -> image, per scan */
                    float* depth,               /* device [n][h][w]; 0 = no measurement         */
                    int* counts,                /* device [n][2] = {points stored, pixels hit}; NULL ok */
                    void* stream);
int md2_disp_post_process(const float* disp, const float* disp_flipped, int n, int h, int w,
                          float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Colour augmentation of a training batch, and a training forward with a separate network input.
 * Monodepth2 jitters the frames the encoder and the pose network see and computes the photometric
 * loss, SSIM and the automask on the ORIGINAL frames.  Additive: MD2_ABI_VERSION is unchanged.
 *
 * md2_color_jitter applies torchvision's float-tensor ColorJitter to x [n][frames][c][h][w], c = 1
 * or 3, into out (same layout).  params[i] (a HOST array, read before the call returns) holds sample
 * i's four factors, the order of the four operations and whether the sample is changed at all; the
 * same parameters apply to every frame of the sample.  All arithmetic is fp32, each operation
 * rounded on its own (no fused multiply-add; divisions correctly rounded).  With
 *   clamp(v) = fminf(fmaxf(v, 0), 1),   blend(a, b, t) = clamp(t*a + (1 - t)*b),
 *   gray = (0.2989f*r + 0.587f*g) + 0.114f*b     (c == 1: the value itself),
 * the operations, applied to a pixel in the order order[0..3], are
 *  0 brightness  v = clamp(brightness * v) per channel.
 *  1 contrast    v = blend(v, mean, contrast) per channel; mean is the mean of gray over the FRAME
 *                (per frame, as torchvision; not per sample) as it stands when contrast is applied,
 *                i.e. after the operations that precede it in order: mean = (float)(S / (double)(h*w)),
 *                S the fp64 sum of the fp32 gray values in the fixed order given below.
 *                means[i][f] receives it (0 for a sample with apply == 0); means may be NULL.
 *  2 saturation  v = blend(v, gray, saturation) per channel; the identity for c == 1.
 *  3 hue         the identity for c == 1; otherwise
 *     1. mx, mn = the channel max and min;  eq = (mx == mn);  cr = mx - mn.
 *     2. s = cr / (eq ? 1 : mx);  d = eq ? 1 : cr.
 *     3. rc = (mx - r) / d,  gc = (mx - g) / d,  bc = (mx - b) / d.
 *     4. hh = (mx == r) ? bc - gc : (mx == g) ? (2 + rc) - bc : (4 + gc) - rc.
 *     5. t = hh / 6 + 1;  hh = t - floorf(t).
 *     6. t = hh + hue;    hh = t - floorf(t).
 *     7. h6 = hh * 6;  i = floorf(h6);  f = h6 - i;  i = (int)i % 6.
 *     8. p = clamp(mx * (1 - s)),  q = clamp(mx * (1 - s*f)),  tt = clamp(mx * (1 - s*(1 - f))).
 *     9. (r, g, b) = (mx,tt,p), (q,mx,p), (p,mx,tt), (p,q,mx), (tt,p,mx), (mx,p,q) for i = 0..5.
 *    hh may come out as exactly 1.0; then i is 6 -> 0 and f = 0, which is continuous.
 * A sample with apply == 0 is copied bit for bit.
 * The sum S: with B = min(ceil(h*w / 1024), 64) blocks of 256 threads per frame, thread t of block k
 * adds the gray of pixels (k*256 + t) + j * (B*256), j ascending, in fp64; the 64 lanes of a wave
 * are combined by a butterfly (partner lane ^ 32, 16, 8, 4, 2, 1), the block's four waves as
 * (w0 + w1) + (w2 + w3), and the frame's B block sums one after the other, k ascending.  A first
 * launch forms the block sums in the workspace, a second adds them, recomputes the chain from x
 * and writes out.  No floating-point atomics, and a grid that depends on the sizes alone: the
 * result is BITWISE REPRODUCIBLE.  The call enqueues the two launches on `stream`; it allocates
 * nothing, never synchronises with the host, and writes everything it reads of the workspace
 * (md2_color_jitter_workspace_size bytes of 8-byte-aligned device memory, any content; the size
 * is 0 for invalid sizes).  params rides in the kernels' argument block (1.3 KB at
 * MD2_JITTER_MAX_SAMPLES: the reason for the cap; callers chunk larger batches).
 * out == x is allowed (in place).
 * MD2_EINVAL (checked before any HIP call): a null x, out, params or workspace; n, frames, h or
 * w < 1; n > MD2_JITTER_MAX_SAMPLES; frames > 65535; c not 1 or 3; h * w > 2^24; a workspace that
 * is not 8-byte aligned; order not a permutation of 0..3; a non-finite factor; a negative
 * brightness, contrast or saturation; |hue| > 0.5; apply not 0 or 1; out overlapping x without
 * being equal to it.
 *
 * md2_model_forward_loss_aug / md2_model_train_step_graph_aug are md2_model_forward_loss /
 * md2_model_train_step_graph with a second input x_net, laid out as x: the encoder (and so both
 * decoders) runs on x_net and the stem's filter gradient reads x_net back; the automask and the
 * loss tail (warp, SSIM, L1) read x.  x_net == NULL or x_net == x IS the plain call (which is
 * implemented as this one with x_net = x).  The result equals, bit for bit, md2_model_forward(x_net)
 * followed by md2_loss_fwd_bwd on x (sigmoid_grad = 0) and md2_model_backward_from.  The backward
 * segments, md2_model_backward_allreduce and md2_model_adam* follow either unchanged.  The graph
 * variant copies x_net into a second executor-owned buffer each call and re-captures when the
 * presence of x_net changes.  Test mode: MD2_ESTATE, as every training entry.  MPI mode
 * (embedding_levels > 0) with a non-null x_net: MD2_ENOTSUP.
 * ---------------------------------------------------------------------------------------- */
#define MD2_JITTER_MAX_SAMPLES 64
typedef struct md2_jitter {      /* one per sample, HOST array, read before the call returns */
  float brightness, contrast, saturation, hue;  /* factors; hue is a shift in turns, |hue| <= 0.5 */
  unsigned char order[4];        /* a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue */
  int apply;                     /* 0: the sample is copied unchanged */
} md2_jitter;
size_t md2_color_jitter_workspace_size(int n, int frames, int h, int w);
int md2_color_jitter(const float* x, int n, int frames, int c, int h, int w,
                     const md2_jitter* params, float* out, float* means /* [n][frames] or NULL */,
                     void* workspace, void* stream);
int md2_model_forward_loss_aug(md2_model* m, const float* x, const float* x_net,
                               const float* auto_loss, float* loss, float* terms, void* stream);
int md2_model_train_step_graph_aug(md2_model* m, const float* x, const float* x_net,
                                   const float* auto_loss, float* adam_m, float* adam_v,
                                   float lr, int step, float* loss, void* stream);

/* ------------------------------------------------------------------------------------------
 * Odometry evaluation: the poses of consecutive frames without the DepthDecoder, and Monodepth2's
 * KITTI odometry metric -- the scale-aligned absolute trajectory error (ATE) over snippets of
 * track_length frames -- entirely on the device.  Additive: MD2_ABI_VERSION is unchanged.
 *
 * md2_model_eval_pose
 * x [n][c][h][w], 2 <= n <= 2*batch + 1: encoder on the n frames, PoseDecoder on the n-1 pairs
 * (frame i, frame i+1).  *pose -> [n-1][6] = (rvec, tvec) of pair i, the RAW network output,
 * i.e. what md2_model_forward writes for that pair before composeT / inversion.
 * Buffer reuse and the MD2_ESTATE rules are those of md2_model_eval_disparity.
 * The executor's buffers hold 3*batch images and 2*batch pairs, hence the limit (MD2_EINVAL outside
 * it); BatchNorm as md2_model_eval_disparity (running statistics in test mode, else the statistics
 * of the n frames, which then move the running ones); MPI mode (embedding_levels > 0): MD2_ENOTSUP.
 *
 * md2_pose_eval
 * pred [M][6]: raw (rvec, tvec) steps, step k relating frame k and frame k+1 of its sequence;
 * gt_rel [M][12]: ground-truth steps (R row-major, t) in fp32; offsets [nseq+1]: a HOST array, read
 * before the call returns, offsets[0] = 0, sequence s = steps offsets[s] .. offsets[s+1]-1 and
 * M = offsets[nseq].  The ground truth is relative because global KITTI translations reach hundreds
 * of metres: differencing them in fp32 costs millimetres against ATEs of about a centimetre, so the
 * host forms D_k = inv(G_k) G_{k+1} in fp64 and rounds once.
 *  1. Step transforms.  D_k = composeT(so3_exp_map(rvec_k), tvec_k, invert): the kernel of
 *     md2_so3_compose_fwd itself (R = I + f1 S + f2 S^2 with S = hat(rvec), theta = |rvec|,
 *     f1 = sin(theta) / max(theta, 1e-4), f2 = (1 - cos(theta)) / max(theta, 1e-4)^2, evaluated in
 *     fp64 and rounded once to fp32); invert = 1 gives (R^T, R^T (-t)).  The network's output for the
 *     pair (k, k+1) maps camera-k points into camera k+1; the chain below wants the pose of camera
 *     k+1 in camera k's frame, so a caller scoring md2_model_eval_pose passes invert = 1 with a
 *     gt_rel of that convention (D_k = inv(G_k) G_{k+1} for camera-to-world G).  Monodepth2's own
 *     evaluate_pose.py chains the un-inverted output; invert = 0 reproduces it.  rt_out [M][12]
 *     (NULL: not wanted) receives D_k.
 *  2. Snippets.  With L = track_length, a sequence of m steps has S = m - L + 2 snippets (0 when
 *     m < L - 1); snippet i uses steps i .. i+L-2 of its sequence and never crosses a boundary.
 *     C_0 = I, C_{j+1} = C_j o D_{i+j} with (R,t) o (R',t') = (R R', R t' + t); every entry is
 *     rounded in fp32 on its own, in this order: (a0*b0 + a1*b1) + a2*b2, then + t for the
 *     translation.  p_j = the translation of C_j, j = 0..L-1 (p_0 = 0: both chains start at the
 *     origin, so Monodepth2's first-frame offset is zero); q_j likewise from gt_rel.
 *  3. Per snippet, out [S_total][3] = (ate, scale, rot_chord), the snippets of sequence 0 first,
 *     in order.  In fp32, starting from 0 and added one term after the other over j = 1..L-1 then
 *     the component 0..2 (p_0 = q_0 = 0 contribute nothing):  num = sum q*p, den = sum p*p;  scale = den > 0 ? num / den : 0  (Monodepth2 divides regardless
 *     and reports NaN for a motionless prediction; here its ATE is that of the zero trajectory);
 *     ate = sqrtf(sum (p*scale - q)^2) / (float)L  -- Monodepth2's compute_ate: the root of the sum,
 *     divided by the number of frames;  rot_chord = sqrtf(sum over the nine entries, row-major, of
 *     (Rp - Rq)^2) for the rotations of C_{L-1}: the Frobenius distance, 2 sqrt(2) sin(angle / 2)
 *     of the relative rotation.  Division and square roots are correctly rounded; there is no
 *     inverse trigonometry on the device (callers convert the chord to an angle).
 *  4. Per sequence, over the snippets whose three values are all finite (the others are counted in
 *     n_bad): summary [nseq][4] = (mean_ate, std_ate, mean_scale, mean_rot_chord), std_ate the
 *     population deviation (as np.std), two-pass; counts [nseq][2] = (snippets S, n_bad).  A sequence
 *     without a finite snippet gives four NaNs.  The sums are fp64 in a fixed order: one block of 256
 *     threads per sequence; thread t adds the values of snippets t, t + 256, ... ascending (a
 *     skipped snippet adds nothing); the 64 lanes of a wave are combined by a butterfly (partner
 *     lane ^ 32, 16, 8, 4, 2, 1), the four waves as (w0 + w1) + (w2 + w3).  mean = sum / count in
 *     fp64; the second pass sums (ate - mean)^2 the same way, std = sqrt(sum / count); each result is
 *     rounded to fp32 once.
 * Three launches on `stream` (steps, snippets: one thread each; sequences: one block each), no
 * allocation, no host synchronisation, no atomics: BITWISE REPRODUCIBLE.  offsets ride in the
 * kernels' argument block (the reason for the MD2_POSE_EVAL_MAX_SEQ cap; callers chunk longer
 * lists).  The workspace (md2_pose_eval_workspace_size(M) bytes of device memory, 0 for M outside
 * 0..2^24; any content) is written before it is read.
 * MD2_EINVAL (checked before any HIP call): a null offsets, summary, counts or workspace; null pred
 * or gt_rel unless M == 0; null out unless there is no snippet; nseq outside
 * 1..MD2_POSE_EVAL_MAX_SEQ; track_length outside 2..MD2_POSE_EVAL_MAX_TRACK; invert not 0 or 1;
 * offsets[0] != 0, a decreasing offset or M > 2^24.
 * ---------------------------------------------------------------------------------------- */
#define MD2_POSE_EVAL_MAX_SEQ 64
#define MD2_POSE_EVAL_MAX_TRACK 16
int md2_model_eval_pose(md2_model* m, const float* x, int n, const float** pose, void* stream);
size_t md2_pose_eval_workspace_size(long long m);
int md2_pose_eval(const float* pred,            /* device [M][6]                                  */
                  const float* gt_rel,          /* device [M][12]                                 */
                  const long long* offsets,     /* HOST [nseq+1]                                  */
                  int nseq, int track_length, int invert,
                  float* out,                   /* device [S_total][3] = ate, scale, rot_chord    */
                  float* summary,               /* device [nseq][4]                               */
                  int* counts,                  /* device [nseq][2] = snippets, n_bad             */
                  float* rt_out,                /* device [M][12] or NULL                         */
                  void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Guarded optimiser step: the global L2 norm of the flat gradient, clipping by it, and "skip the
 * update if any gradient entry is non-finite" -- between the backward and ADAM, entirely on the
 * device, without a host synchronisation.  Additive: MD2_ABI_VERSION is unchanged.  With the guard
 * off nothing changes; with it on, max_norm = +inf and finite gradients the step writes the same
 * bytes as the plain step.
 *
 * md2_grad_norm: two launches over any flat fp32 device vector g[0..n), 1 <= n <= 2^31.
 *  1. grad_sumsq.  S = the fp64 sum of (double)g_i * (double)g_i over the FINITE entries (each
 *     product is exact in fp64), c = the number of non-finite entries (NaN, +Inf, -Inf), which add
 *     nothing to S.  The order is defined on element indices alone:
 *       B = min(ceil(n / 4096), 1024) blocks of 256 threads (the grid depends on n only);
 *       thread t of block k adds the elements 4 (256 k + t) + j (1024 B) + {0, 1, 2, 3} that lie
 *       below n, for j = 0, 1, ... ascending and the four in index order, one after the other into
 *       one fp64 accumulator that starts at 0;
 *       the 64 lanes of a wave are combined by a butterfly (partner lane ^ 32, 16, 8, 4, 2, 1), the
 *       four waves as (w0 + w1) + (w2 + w3);
 *       block k writes its partial and its count to the workspace.
 *     A 16-byte aligned g is read with 16-byte loads, any other with 4-byte loads; the map from
 *     elements to threads is the same, so the result does not depend on the pointer's alignment.
 *  2. grad_guard_finish, one block of 256 threads: thread t adds the block partials t, t + 256, ...
 *     ascending into an accumulator that starts at 0; the same butterfly and wave order follow.
 *     Thread 0 then writes *state:
 *       sumsq = S;  nonfinite = c;  ok = (c == 0);
 *       norm  = (float)(sqrt(S) * (double)grad_scale)    (fp64 square root and product, one rounding
 *               to fp32): the norm of the gradient ADAM will see, grad_scale * g;
 *       coef  = max_norm / norm when ok, max_norm is finite and norm > max_norm, otherwise 1.0f:
 *               ONE correctly rounded fp32 division.  This is NOT torch's clip_grad_norm_ coefficient
 *               max_norm / (norm + 1e-6): a gradient of exactly max_norm is left alone, and a
 *               clipped one has norm max_norm to one rounding;
 *       gscale = grad_scale * coef, one fp32 multiply (coef == 1 gives grad_scale bit for bit);
 *       skipped += !ok: cumulative, read-modify-written -- the caller zeroes *state once.
 * No atomics, no "last block" counter: BITWISE REPRODUCIBLE.  No allocation, no host
 * synchronisation.  The workspace (md2_grad_norm_workspace_size(n) bytes of device memory, 8-byte
 * aligned; 0 for n outside 1..2^31) may hold anything on entry.  max_norm = +inf: no clipping.
 * MD2_EINVAL (checked before any HIP call): a null g, state or workspace; n outside 1..2^31;
 * max_norm NaN or <= 0; grad_scale not finite and positive; a workspace not 8-byte aligned.
 *
 * md2_adam_guarded: md2_adam driven by a state block.  When !state->ok every thread returns before
 * any load or store of p, adam_m, adam_v; otherwise the arithmetic is md2_adam's with
 * grad_scale = state->gscale (same expressions, same order, same bits).
 *
 * md2_model_set_grad_guard(m, on, max_norm): model state (max_norm as above; ignored when on = 0).
 * While the guard is on, md2_model_adam, md2_model_train_step, md2_model_train_step_graph (and _aug)
 * and md2_model_train_step_dp run md2_grad_norm over the whole flat gradient -- in the DP step after
 * the last bucket's all-reduce, with grad_scale = 1/nranks -- then the guarded ADAM and the re-pack.
 * md2_model_adam_segment returns MD2_ENOTSUP (a segment's update cannot know the global norm) and
 * the MD2_SEG_UPDATE=1 routes take the single update.  (on, max_norm) is part of the captured
 * step's re-capture key.  The state and the workspace are executor-owned, allocated when the guard
 * is first switched on and counted in md2_model_device_bytes from then on.  Every call clears
 * `skipped` (and the rest of the state); it synchronises the device to do so, so it belongs
 * outside the step.  Test mode: MD2_ESTATE, like the other training entries; MPI mode
 * (embedding_levels > 0): MD2_ENOTSUP.
 * Step counting: a skipped step still consumes its step number -- the bias correction uses the
 * caller's `step`, and in the captured step the device counter advances unconditionally -- so the
 * eager and the captured path stay bit-equal and the host never needs to know that a step was
 * skipped.  A skipped step leaves params, adam_m, adam_v unchanged; the re-pack then rewrites the
 * packed weights with the values they already hold.
 * BatchNorm running statistics move in the forward, before the gradient exists: a skipped step
 * does NOT undo that.
 * md2_model_grad_guard_state: the device pointer of the executor's state; its values are those of
 * the last guarded step once the stream has passed it.  MD2_ESTATE if the guard was never on.
 * ---------------------------------------------------------------------------------------- */
typedef struct md2_guard_state {
  double sumsq;          /* S: the fp64 sum of squares of the finite entries              */
  long long nonfinite;   /* c: the number of NaN / Inf entries                            */
  long long skipped;     /* steps with ok == 0 since the state was last zeroed            */
  float norm;            /* (float)(sqrt(S) * grad_scale)                                 */
  float coef;            /* the clip coefficient, 1.0f when nothing is clipped            */
  float gscale;          /* grad_scale * coef: what the guarded ADAM multiplies g by      */
  int ok;                /* c == 0                                                        */
} md2_guard_state;
size_t md2_grad_norm_workspace_size(long long n);
int md2_grad_norm(const float* g, long long n, float grad_scale, float max_norm,
                  md2_guard_state* state /* device */, void* workspace, void* stream);
int md2_adam_guarded(float* p, const float* g, float* adam_m, float* adam_v, long long n, float lr,
                     float beta1, float beta2, float eps, int step,
                     const md2_guard_state* state /* device */, void* stream);
int md2_model_set_grad_guard(md2_model* m, int on, float max_norm);
int md2_model_grad_guard_state(md2_model* m, const md2_guard_state** dev);

/* ------------------------------------------------------------------------------------------
 * Frame resize on the device: m decoded images, each of its own size, resized to one target size
 * and written as planes -- the step between a PNG decoder (md2_load_frames_native_u8) and the
 * batch x[N][3][C][H][W] ([m] = [N*3] frames in order IS that layout).  Additive: MD2_ABI_VERSION
 * is unchanged.
 *
 * Image i is src[offsets[i] ..], src_h[i] rows of src_w[i] interleaved pixels of c bytes, at any
 * byte offset.  offsets, src_w, src_h and flip are HOST arrays, read before the call returns.
 * All arithmetic is fp64, each operation rounded on its own (no fused multiply-add), until the
 * final conversion.  The value of a source byte b is v = (double)b / 255.0.  For output pixel
 * (y, x) of channel ch, with n_in / n_out the source / target length of an axis:
 *
 * MD2_RESIZE_IMRESIZE -- ImageTransformations' imresize as md2hip.data.imresize and
 * md2_load_kitti_u8 restate it (bilinear, outer corners aligned, no antialiasing).  Per axis:
 *  1. sf = (double)n_in / n_out;  p = sf * ((i + 1) - 0.5) + 0.5.
 *  2. if sf < 1: p = min(max(p, 1), n_in).  p = p - 1.
 *  3. i0 = min((int)floor(p), n_in - 1);  f = p - i0;  i1 = min(i0 + 1, n_in - 1).
 * Then top = v(y0,x0) * (1 - fx) + v(y0,x1) * fx, bot the same on row y1, and
 * r = top * (1 - fy) + bot * fy.
 *
 * MD2_RESIZE_ANTIALIAS -- the triangle filter widened by the reduction factor (Pillow's BILINEAR
 * resize; torch's interpolate(mode="bilinear", antialias=True, align_corners=False)).  Per axis:
 *  1. scale = (double)n_in / n_out;  fs = max(scale, 1);  center = (i + 0.5) * scale.
 *  2. lo = max((int)((center - fs) + 0.5), 0);  hi = min((int)((center + fs) + 0.5), n_in); the
 *     conversions truncate toward zero.
 *  3. for k in [lo, hi): w_k = max(0, 1 - |((k - center) + 0.5) / fs|);  ww = the sum of the w_k,
 *     k ascending, from 0.0;  the weight of tap k is w_k / ww.
 * Then the horizontal sum of source row yy is H(yy) = sum over k of wx_k * v(yy, k), k ascending,
 * from 0.0, each term a rounded product followed by a rounded add, and r = sum over yy of
 * wy_yy * H(yy), yy ascending, from 0.0, in the same way.
 *
 * Both filters:
 *  - an image that already has the target size is copied, r = v (what either formula gives);
 *  - quantize = 1: q = rint(r * 255.0) (ties to even); out = (float)q / 255.0f, the bits
 *    md2_unorm8_to_float gives for the byte q; out_u8 (may be NULL) = q.  This is the N0f8
 *    rounding imresize applies; exact ties of r * 255 occur (a 2x reduction has the weights
 *    1/8, 3/8, 3/8, 1/8), which is why the order of the sums is part of the interface;
 *  - quantize = 0: out = (float)r; out_u8 must be NULL;
 *  - flip[i] != 0 writes column x of the result at out_w - 1 - x (flip may be NULL: none).
 * MD2_RESIZE_IMRESIZE with quantize = 1 gives the bytes of md2_load_kitti_u8.
 *
 * One launch for all images (the image index on a grid axis): a block owns 128 output columns
 * and 8 output rows of one image, forms its tap weights once in LDS from the formulas above,
 * stages the source rows it needs in LDS and streams them in ascending order -- a thread forms
 * H(yy) for its column and adds wy * H(yy) into the rows of its band that yy belongs to, so no
 * intermediate leaves the chip.  The staging loads are whole aligned 4-byte words: up to 3 bytes
 * before the first and after the last byte of a source row are read (never past the word that
 * holds a source byte) and ignored.  No workspace, no allocation, no copy, no atomics, no
 * synchronisation with the host; the result is BITWISE REPRODUCIBLE; nothing beyond
 * [m][c][out_h][out_w] of out and out_u8 is written.  The four host arrays ride in the kernel's
 * argument block (1.1 KB at MD2_RESIZE_MAX_IMAGES: the reason for the cap; callers chunk).
 * MD2_EINVAL (checked before any HIP call): a null cfg, src, offsets, src_w, src_h or out; m
 * outside 1..MD2_RESIZE_MAX_IMAGES; c not 1 or 3; out_h, out_w, a src_w[i] or a src_h[i] outside
 * 1..8192; an unknown filter; quantize not 0 or 1; out_u8 without quantize; a negative offset;
 * out not 16-byte aligned; src_w[i] > 16 * out_w or src_h[i] > 16 * out_h (either filter: at
 * most 33 taps per axis).
 * ---------------------------------------------------------------------------------------- */
#define MD2_RESIZE_MAX_IMAGES 64
enum { MD2_RESIZE_IMRESIZE = 0, MD2_RESIZE_ANTIALIAS = 1 };
typedef struct md2_resize_cfg {
  int m;             /* images in this call, 1..MD2_RESIZE_MAX_IMAGES                     */
  int c;             /* 1 or 3; a source image is [h][w][c] bytes, interleaved, as decoded */
  int out_h, out_w;  /* target size, 1..8192                                              */
  int filter;        /* MD2_RESIZE_IMRESIZE | MD2_RESIZE_ANTIALIAS                        */
  int quantize;      /* 1: round the result to N0f8 (the element type imresize keeps)     */
} md2_resize_cfg;
int md2_resize_frames(const md2_resize_cfg* cfg,
                      const unsigned char* src,   /* device: all source images             */
                      const long long* offsets,   /* HOST [m]: byte offset of image i in src */
                      const int* src_w, const int* src_h, /* HOST [m]: 1..8192 each        */
                      const unsigned char* flip,  /* HOST [m] or NULL: mirror after resize */
                      float* out,                 /* device [m][c][out_h][out_w], 16-B aligned */
                      unsigned char* out_u8,      /* device, same shape, or NULL; needs quantize */
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss tail over S = 1..MD2_MAX_SOURCES sources, each LEARNED or FIXED -- Monodepth2's stereo
 * supervision ("MS": both temporal sources and the other camera of the rig; "S": that camera
 * alone).  Additive: MD2_ABI_VERSION is unchanged, and md2_loss_fwd_bwd keeps its code path.
 *
 * A LEARNED source (pose_block >= 0) is warped by composeT(so3_exp_map(rvec), tvec, invert) of
 * row pose[pose_block * n + i] and its pose receives a gradient.  A FIXED source (pose_block == -1)
 * is warped by the caller's transform Rt[i] = (R row-major (9), t (3)) -- for a rectified stereo
 * rig R = I and t = (+-baseline, 0, 0) -- which is data: it is read, never differentiated.
 * The pose blocks of the learned sources must be 0..L-1, each once (L = number of learned
 * sources); pose and out->d_pose are [L * n][6], and with L = 0 both may be NULL (d_pose is not
 * written).
 * Each source is its own tensor: sample i's [c][h][w] frame is at frames + i * sample_stride
 * (floats), so a source may be a frame inside x[n][3][c][h][w] (frames = x + f * c*h*w,
 * sample_stride = 3*c*h*w) or a separate [n][c][h][w] tensor (sample_stride = c*h*w).  Likewise
 * `target` with target_sample_stride.  cfg->target, src0, src1, invert_mask and x_*_stride are
 * not read; everything else in cfg means what it means to md2_loss_fwd_bwd.
 *
 * Per pixel and scale: photometric_loss of every source warped through the scale's depth, then the
 * FIRST argmin over the sources in the order given (strict <: a tie goes to the earlier source),
 * then the automask, which wins ties (lmin < automask keeps the source).  Only the selected
 * source's adjoint is formed.  Sums over sources (d depth) run in ascending source order.
 * Outputs as md2_loss_out states, with: vis_sel 0..S-1 or -1; vis_warped [S][n][c][h][w];
 * vis_cell [nscales][S][n][h][w]; d_pose [L*n][6].
 * With two learned sources that point at frames src0 / src1 of x, every output equals
 * md2_loss_fwd_bwd's bit for bit (the per-source arithmetic is the same, operation for operation).
 *
 * md2_automasking_loss_sources: out [n][h][w] = min over the S raw sources of
 * photometric_loss(source, target), first source on ties; with two sources the bits of
 * md2_automasking_loss.  Only frames and sample_stride of each source are read.
 *
 * MD2_EINVAL (checked before any HIP call): a null cfg, sources, target, disp, out, out->loss or
 * workspace; nsrc outside 1..MD2_MAX_SOURCES; a source without frames; a learned source with a
 * null pose; a fixed source with a null Rt; pose blocks that are not 0..L-1 each once; c not 1
 * or 3; bad dims.  md2_loss_sources_workspace_size returns 0 for a null cfg or a bad nsrc.
 * ---------------------------------------------------------------------------------------- */
#define MD2_MAX_SOURCES 3
typedef struct md2_loss_source {
  const float* frames;        /* device; sample i's frame at frames + i*sample_stride, [c][h][w] */
  long long sample_stride;    /* floats                                                          */
  int pose_block;             /* >= 0: learned, rows pose[pose_block*n + i]; -1: fixed          */
  int invert;                 /* learned only: composeT's inverse_transform                      */
  const float* Rt;            /* fixed only: device [n][12], R row-major then t                  */
} md2_loss_source;
size_t md2_loss_sources_workspace_size(const md2_loss_cfg* cfg, int nsrc);
int md2_loss_fwd_bwd_sources(const md2_loss_cfg* cfg, int nsrc, const md2_loss_source* sources,
                             const float* target, long long target_sample_stride,
                             const float* const* disp, const float* pose, const float* automask,
                             float dloss, const md2_loss_out* out, void* workspace, void* stream);
int md2_automasking_loss_sources(int nsrc, const md2_loss_source* sources, const float* target,
                                 long long target_sample_stride, int n, int c, int h, int w,
                                 float* out, void* stream);

/* Per-sample camera intrinsics.  Additive: MD2_ABI_VERSION is unchanged.
 *
 * md2_loss_fwd_bwd_sources_k is md2_loss_fwd_bwd_sources with sample i back-projected by invK[i] and
 * projected by K[i]: K and invK are device [n][9] each (row-major 3x3 per sample, in the 1-based
 * pixel coordinates of cfg->K), read and never written.  cfg->K / cfg->invK are not read.  The
 * workspace is md2_loss_sources_workspace_size's.  Only the photometric warp (and vis_warped) reads
 * intrinsics; the smoothness term, the automask and the reductions do not.  When every row of K /
 * invK equals cfg->K / cfg->invK, every output equals md2_loss_fwd_bwd_sources' bit for bit (the
 * arithmetic after the read is the same, operation for operation) -- and so, with two learned
 * sources that are frames of x, md2_loss_fwd_bwd's.  It always runs on the kernel over sources,
 * nsrc = 2 included.  The matrices are device data and are not validated.
 * MD2_EINVAL (before any HIP call): a null K or invK, and everything md2_loss_fwd_bwd_sources
 * checks. */
int md2_loss_fwd_bwd_sources_k(const md2_loss_cfg* cfg, int nsrc, const md2_loss_source* sources,
                               const float* target, long long target_sample_stride,
                               const float* K, const float* invK,   /* device [n][9] each */
                               const float* const* disp, const float* pose, const float* automask,
                               float dloss, const md2_loss_out* out, void* workspace, void* stream);

/* Per-sample intrinsics as model state, modelled on md2_model_set_disparity_bins: K and invK
 * (device [batch][9] each) are copied into executor-owned buffers on `stream`, and every following
 * forward_loss -- the plain, _aug and _stereo forms, md2_model_train_step, the train_step_graph
 * family, md2_model_train_step_dp -- warps sample i with row i until they are set again.
 * K == invK == NULL returns to cfg.K / cfg.invK.  While set, the loss tail runs as
 * md2_loss_fwd_bwd_sources_k: the plain step over {src0, src1} learned, MS and S over their sources;
 * the library's own automask is taken over the same sources.  With every row equal to cfg.K /
 * cfg.invK the step's loss, gradient and parameters equal the plain step's bit for bit.  The
 * captured graph reads the executor's buffers: it is captured again when intrinsics come or go, not
 * when their values change.  Test mode is unaffected (inference reads no intrinsics).
 * MD2_EINVAL: exactly one of K, invK null; a null model.  MPI mode (embedding_levels > 0):
 * MD2_ENOTSUP when K is given. */
int md2_model_set_intrinsics(md2_model* m, const float* K, const float* invK, void* stream);

/* The training entry points with a stereo source, modelled on the _aug pair (x_net as there; NULL or
 * x: the networks read x).  x_stereo [batch][c][h][w] is the other camera's frame at the target's
 * time and stereo_Rt [batch][12] its fixed transform (R row-major, t).  The networks never see
 * x_stereo: only the loss tail and the automask read it.
 *   temporal = 1 ("MS"): the sources of the loss are cfg.src0, cfg.src1 (learned, as in the plain
 *     call) and the stereo frame (fixed), in that order -- Monodepth2's [0, -1, 1, "s"].
 *   temporal = 0 ("S"): the only source is the stereo frame.  The pose network still runs and
 *     receives a zero d_pose, so its gradient is exactly zero; backward segments, data-parallel
 *     buckets and the captured graph keep their shape.
 * auto_loss == NULL with cfg.automasking: the library takes the automask over the same sources the
 * loss uses (md2_automasking_loss_sources).  The result equals, bit for bit, md2_model_forward(x_net)
 * followed by md2_loss_fwd_bwd_sources on those sources (sigmoid_grad = 0) and
 * md2_model_backward_from.  The graph variant copies x_stereo and stereo_Rt into executor-owned
 * buffers on each call and re-captures when the presence of the stereo source or `temporal`
 * changes; the gradient guard needs nothing new.  The sources workspace is allocated at the first
 * stereo call.  MD2_EINVAL: a null x_stereo or stereo_Rt, temporal not 0 or 1.  MPI mode
 * (embedding_levels > 0): MD2_ENOTSUP.  Test mode: MD2_ESTATE.  md2_model_train_step_dp has no
 * stereo form. */
int md2_model_forward_loss_stereo(md2_model* m, const float* x, const float* x_net, const float* x_stereo,
                                  const float* stereo_Rt, int temporal, const float* auto_loss,
                                  float* loss, float* terms, void* stream);
int md2_model_train_step_graph_stereo(md2_model* m, const float* x, const float* x_net,
                                      const float* x_stereo, const float* stereo_Rt, int temporal,
                                      const float* auto_loss, float* adam_m, float* adam_v, float lr,
                                      int step, float* loss, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MD2_H */
