"""ctypes binding of libmd2hip.so (include/md2.h).

The product path has NO fallback: if the HIP library is missing or fails to load, every call
raises.  Tensors cross the boundary as raw device pointers (``tensor.data_ptr()``)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MD2HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libmd2hip.so"))

MAX_SCALES = 5
ABI_VERSION = 2          # include/md2.h MD2_ABI_VERSION: the struct layouts below


class LossCfg(C.Structure):
    """``md2_loss_cfg``."""
    _fields_ = [
        ("n", C.c_int), ("c", C.c_int), ("width", C.c_int), ("height", C.c_int),
        ("nscales", C.c_int),
        ("scale_w", C.c_int * MAX_SCALES), ("scale_h", C.c_int * MAX_SCALES),
        ("smooth_weight", C.c_float * MAX_SCALES),
        ("divisor", C.c_float), ("smooth_normalize", C.c_int),
        ("K", C.c_float * 9), ("invK", C.c_float * 9),
        ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("x_sample_stride", C.c_longlong), ("x_frame_stride", C.c_longlong),
        ("target", C.c_int), ("src0", C.c_int), ("src1", C.c_int),
        ("invert_mask", C.c_int), ("sigmoid_grad", C.c_int),
    ]


class LossOut(C.Structure):
    """``md2_loss_out``."""
    _fields_ = [
        ("loss", C.c_void_p), ("terms", C.c_void_p),
        ("d_disp", C.c_void_p * MAX_SCALES), ("d_pose", C.c_void_p),
        ("vis_loss", C.c_void_p), ("vis_sel", C.c_void_p), ("vis_warped", C.c_void_p),
        ("vis_cell", C.c_void_p),
    ]


MAX_SOURCES = 3          # include/md2.h MD2_MAX_SOURCES


class LossSource(C.Structure):
    """``md2_loss_source``."""
    _fields_ = [("frames", C.c_void_p), ("sample_stride", C.c_longlong), ("pose_block", C.c_int),
                ("invert", C.c_int), ("Rt", C.c_void_p)]


class ConvDesc(C.Structure):
    """``md2_conv_desc``."""
    _fields_ = [(n, C.c_int) for n in ("n", "cin", "h", "w", "cout", "kh", "kw", "stride", "pad",
                                       "reflect", "act")]


class ConvOperands(C.Structure):
    """``md2_conv_operands``."""
    _fields_ = [("in1", C.c_void_p), ("out1", C.c_void_p),
                ("in_bs0", C.c_longlong), ("in_bs1", C.c_longlong), ("in_bhi", C.c_longlong),
                ("out_bs0", C.c_longlong), ("out_bs1", C.c_longlong),
                ("in_c0", C.c_int), ("in_bdiv", C.c_int), ("out_c0", C.c_int), ("accumulate", C.c_int),
                ("cin_w", C.c_int)]


class ConvDefer(C.Structure):
    """``md2_conv_defer``."""
    _fields_ = [("slab", C.c_void_p), ("defer_reduce", C.c_int), ("splits", C.c_int), ("stats_parts", C.c_int)]


class BNDesc(C.Structure):
    """``md2_bn_desc``."""
    _fields_ = [("n", C.c_int), ("c", C.c_int), ("h", C.c_int), ("w", C.c_int), ("eps", C.c_float),
                ("momentum", C.c_float), ("route", C.c_int), ("collapse", C.c_int)]


class BNInfo(C.Structure):
    """``md2_bn_info``."""
    _fields_ = [(n, C.c_int) for n in ("family", "parts", "fin_parts", "upt", "vec")]


class BNFwdOperands(C.Structure):
    """``md2_bn_fwd_operands``."""
    _fields_ = [(n, C.c_void_p) for n in ("y", "slab", "y_out", "part", "gamma", "beta", "mean", "invstd",
                                          "run_mean", "run_var", "y2", "gamma2", "beta2", "mean2", "invstd2",
                                          "res", "out", "pool_y", "pool_arg")] + \
               [("splits", C.c_int), ("parts", C.c_int), ("relu", C.c_int)]


class BNBwdOperands(C.Structure):
    """``md2_bn_bwd_operands``."""
    _fields_ = [(n, C.c_void_p) for n in ("dout", "slab", "dout_w", "mask", "y", "mean", "invstd", "gamma",
                                          "mbeta", "dgamma", "dbeta", "dy", "dres", "skip")] + \
               [("skip_lo", C.c_longlong), ("skip_hi", C.c_longlong), ("splits", C.c_int),
                ("dres_accumulate", C.c_int)]


class ModelCfg(C.Structure):
    """``md2_model_cfg``."""
    _fields_ = [
        ("arch", C.c_int), ("in_channels", C.c_int), ("batch", C.c_int),
        ("width", C.c_int), ("height", C.c_int),
        ("n_levels", C.c_int), ("scale_levels", C.c_int * MAX_SCALES),
        ("K", C.c_float * 9), ("invK", C.c_float * 9),
        ("min_depth", C.c_float), ("max_depth", C.c_float), ("disparity_smoothness", C.c_float),
        ("scales", C.c_float * MAX_SCALES),
        ("automasking", C.c_int), ("target", C.c_int), ("src0", C.c_int), ("src1", C.c_int),
        ("embedding_levels", C.c_int), ("num_bins", C.c_int),
    ]


class WarpCfg(C.Structure):
    """``md2_warp_cfg``."""
    _fields_ = [
        ("n", C.c_int), ("c", C.c_int), ("width", C.c_int), ("height", C.c_int),
        ("dw", C.c_int), ("dh", C.c_int),
        ("K", C.c_float * 9), ("invK", C.c_float * 9),
        ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("x_sample_stride", C.c_longlong), ("x_frame_stride", C.c_longlong),
        ("target", C.c_int), ("src0", C.c_int), ("src1", C.c_int),
    ]


class DepthEvalCfg(C.Structure):
    """``md2_depth_eval_cfg``."""
    _fields_ = [
        ("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("gt_h", C.c_int), ("gt_w", C.c_int),
        ("y0", C.c_int), ("y1", C.c_int), ("x0", C.c_int), ("x1", C.c_int),
        ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("eval_min", C.c_float), ("eval_max", C.c_float),
        ("median_scaling", C.c_int), ("scale", C.c_float),
    ]


LIDAR_MAX_SCANS = 64     # include/md2.h MD2_LIDAR_MAX_SCANS


class LidarCfg(C.Structure):
    """``md2_lidar_cfg``."""
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("forward_only", C.c_int), ("vel_depth", C.c_int)]


JITTER_MAX_SAMPLES = 64  # include/md2.h MD2_JITTER_MAX_SAMPLES


class Jitter(C.Structure):
    """``md2_jitter``."""
    _fields_ = [("brightness", C.c_float), ("contrast", C.c_float), ("saturation", C.c_float), ("hue", C.c_float),
                ("order", C.c_ubyte * 4), ("apply", C.c_int)]


POSE_EVAL_MAX_SEQ = 64   # include/md2.h MD2_POSE_EVAL_MAX_SEQ
POSE_EVAL_MAX_TRACK = 16  # include/md2.h MD2_POSE_EVAL_MAX_TRACK



class GuardState(C.Structure):
    """``md2_guard_state`` (40 bytes)."""
    _fields_ = [("sumsq", C.c_double), ("nonfinite", C.c_longlong), ("skipped", C.c_longlong),
                ("norm", C.c_float), ("coef", C.c_float), ("gscale", C.c_float), ("ok", C.c_int)]


RESIZE_MAX_IMAGES = 64   # include/md2.h MD2_RESIZE_MAX_IMAGES
RESIZE_FILTERS = {"imresize": 0, "antialias": 1}   # MD2_RESIZE_IMRESIZE, MD2_RESIZE_ANTIALIAS


class ResizeCfg(C.Structure):
    """``md2_resize_cfg``."""
    _fields_ = [("m", C.c_int), ("c", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int), ("filter", C.c_int),
                ("quantize", C.c_int)]


_lib = None
_load_error = None

CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
INCLUDE_H = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "md2.h")


def source_build_id():
    """The hash csrc/Makefile embeds as md2_build_id(): sha256 of the sorted csrc sources
    (*.hip *.cpp *.h *.inc), the Makefile and include/md2.h, concatenated; None without a tree."""
    import hashlib
    if not os.path.isdir(CSRC):
        return None
    names = sorted(set(n for n in os.listdir(CSRC)
                       if os.path.splitext(n)[1] in (".hip", ".cpp", ".h", ".inc")))
    h = hashlib.sha256()
    for path in [os.path.join(CSRC, n) for n in names] + [os.path.join(CSRC, "Makefile"), INCLUDE_H]:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]

P = C.c_void_p
FP = C.POINTER(C.c_void_p)

_SIGS = {
    "md2_abi_version": (C.c_int, []),
    "md2_last_error": (C.c_char_p, []),
    "md2_build_id": (C.c_char_p, []),
    "md2_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "md2_memcpy_d2d": (C.c_int, [P, P, C.c_size_t, P]),
    "md2_loss_workspace_size": (C.c_size_t, [C.POINTER(LossCfg)]),
    "md2_loss_fwd_bwd": (C.c_int, [C.POINTER(LossCfg), FP, P, P, P, C.c_float, C.POINTER(LossOut), P, P]),
    "md2_so3_compose_fwd": (C.c_int, [P, C.c_int, C.c_int, P, P]),
    "md2_so3_compose_bwd": (C.c_int, [P, C.c_int, C.c_int, P, P, P]),
    "md2_conv2d_workspace_size": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "md2_conv2d_fwd": (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P, P]),
    "md2_conv2d_dgrad": (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P]),
    "md2_conv2d_wgrad": (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P, P]),
    "md2_act_backward": (C.c_int, [P, P, P, C.c_longlong, C.c_int, P]),
    "md2_conv2d_ex_workspace_size": (C.c_size_t, [C.POINTER(ConvDesc), C.POINTER(ConvOperands)]),
    "md2_conv2d_fwd_ex": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvOperands), P, P, P, P, P,
                                     C.POINTER(ConvDefer), P, C.c_size_t, P]),
    "md2_conv2d_dgrad_ex": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvOperands), P, P, P, C.POINTER(ConvDefer), P,
                                       C.c_size_t, P]),
    "md2_conv2d_wgrad_ex": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvOperands), P, P, P, P, P, C.c_int, P,
                                       C.c_size_t, P]),
    "md2_act_bias_parts": (C.c_int, [C.c_int, C.c_int, C.c_longlong]),
    "md2_act_backward_bias": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_longlong, C.c_int, P, P]),
    "md2_conv_last_kernel": (C.c_char_p, []),
    "md2_adam": (C.c_int, [P, P, P, P, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float,
                            C.c_int, C.c_float, P]),
    "md2_maxpool3s2_fwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "md2_maxpool3s2_bwd": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_maxpool3s2_bwd_ex": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, C.c_longlong,
                                        C.c_longlong, P]),
    "md2_bn_ex_workspace_size": (C.c_size_t, [C.POINTER(BNDesc)]),
    "md2_bn_channel_fits": (C.c_int, [C.c_int, C.c_longlong]),
    "md2_bn_forward_ex": (C.c_int, [C.POINTER(BNDesc), C.POINTER(BNFwdOperands), C.POINTER(BNInfo), P,
                                    C.c_size_t, P]),
    "md2_bn_backward_ex": (C.c_int, [C.POINTER(BNDesc), C.POINTER(BNBwdOperands), C.POINTER(BNInfo), P,
                                     C.c_size_t, P]),
    "md2_upsample2_fwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_upsample2_bwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_arch_param_count": (C.c_int, [C.POINTER(ModelCfg), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "md2_arch_param_info": (C.c_int, [C.POINTER(ModelCfg), C.c_int, C.c_char_p, C.c_int,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "md2_model_create": (C.c_int, [C.POINTER(ModelCfg), P, P, C.POINTER(C.c_void_p)]),
    "md2_model_destroy": (C.c_int, [P]),
    "md2_model_device_bytes": (C.c_size_t, [P]),
    "md2_model_repack": (C.c_int, [P, P]),
    "md2_model_forward_loss": (C.c_int, [P, P, P, P, P, P]),
    "md2_model_forward": (C.c_int, [P, P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), P]),
    "md2_model_set_cotangents": (C.c_int, [P, FP, P, P]),
    "md2_model_backward_from": (C.c_int, [P, FP, P, P]),
    "md2_model_num_segments": (C.c_int, [P]),
    "md2_model_backward_segment": (C.c_int, [P, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), P]),
    "md2_model_adam": (C.c_int, [P, P, P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, P]),
    "md2_model_adam_segment": (C.c_int, [P, C.c_int, P, P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                         C.c_float, P]),
    "md2_model_adam_join": (C.c_int, [P, P]),
    "md2_model_train_step": (C.c_int, [P, P, P, P, P, C.c_float, C.c_int, P, P]),
    "md2_model_train_step_graph": (C.c_int, [P, P, P, P, P, C.c_float, C.c_int, P, P]),
    "md2_model_set_params": (C.c_int, [P, P, P]),
    "md2_model_get_params": (C.c_int, [P, P, P]),
    "md2_model_get_grads": (C.c_int, [P, P, P]),
    "md2_model_loss_cotangent": (C.c_int, [P, C.c_float, P]),
    "md2_model_set_disparity_bins": (C.c_int, [P, P, P]),
    "md2_model_set_intrinsics": (C.c_int, [P, P, P, P]),
    "md2_model_outputs": (C.c_int, [P, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_void_p)]),
    "md2_model_eval_disparity": (C.c_int, [P, P, C.c_int, C.POINTER(C.c_void_p), P]),
    "md2_arch_bn_stat_count": (C.c_int, [C.POINTER(ModelCfg), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "md2_model_get_bn_stats": (C.c_int, [P, P, P]),
    "md2_model_set_bn_stats": (C.c_int, [P, P, P]),
    "md2_model_set_testmode": (C.c_int, [P, C.c_int, P]),
    "md2_model_testmode": (C.c_int, [P]),
    "md2_depth_eval_workspace_size": (C.c_size_t, [C.POINTER(DepthEvalCfg)]),
    "md2_depth_eval": (C.c_int, [C.POINTER(DepthEvalCfg), P, P, P, P, P, P]),
    "md2_lidar_depth": (C.c_int, [C.POINTER(LidarCfg), P, C.POINTER(C.c_longlong), C.POINTER(C.c_float), P, P, P]),
    "md2_disp_post_process": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_color_jitter_workspace_size": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "md2_color_jitter": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Jitter), P, P, P, P]),
    "md2_model_forward_loss_aug": (C.c_int, [P, P, P, P, P, P, P]),
    "md2_model_train_step_graph_aug": (C.c_int, [P, P, P, P, P, P, C.c_float, C.c_int, P, P]),
    "md2_model_eval_pose": (C.c_int, [P, P, C.c_int, C.POINTER(C.c_void_p), P]),
    "md2_pose_eval_workspace_size": (C.c_size_t, [C.c_longlong]),
    "md2_pose_eval": (C.c_int, [P, P, C.POINTER(C.c_longlong), C.c_int, C.c_int, C.c_int, P, P, P, P, P, P]),
    "md2_grad_norm_workspace_size": (C.c_size_t, [C.c_longlong]),
    "md2_grad_norm": (C.c_int, [P, C.c_longlong, C.c_float, C.c_float, P, P, P]),
    "md2_adam_guarded": (C.c_int, [P, P, P, P, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_int, P, P]),
    "md2_model_set_grad_guard": (C.c_int, [P, C.c_int, C.c_float]),
    "md2_model_grad_guard_state": (C.c_int, [P, C.POINTER(C.c_void_p)]),
    "md2_model_debug_tensor": (C.c_int, [P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int)]),
    "md2_model_features": (C.c_int, [P, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int)]),
    "md2_mpi_embed_features": (C.c_int, [P, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int,
                                         C.c_int, P, P]),
    "md2_concat_channels": (C.c_int, [P, C.c_int, P, C.c_int, C.c_int, C.c_longlong, P, P]),
    "md2_automasking_loss": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_static_scores_workspace_size": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "md2_static_scores": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "md2_mine_src_xyz": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "md2_mine_tgt_xyz": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_mine_sample": (C.c_int, [P, C.c_int, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P]),
    "md2_plane_volume_rendering": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P]),
    "md2_render_tgt_rgb_depth": (C.c_int, [P, P, P, P, P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P]),
    "md2_ssim_fwd": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_ssim_bwd": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "md2_backproject_fwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P]),
    "md2_backproject_bwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P]),
    "md2_project_fwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P, P, P]),
    "md2_project_workspace_size": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "md2_project_bwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P, P, P]),
    "md2_grid_sample_border_fwd": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "md2_grid_sample_border_bwd": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             P, P, P]),
    "md2_unorm8_to_float": (C.c_int, [P, P, C.c_longlong, P]),
    "md2_png_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "md2_load_triplets_u8": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, P, P, C.c_int]),
    "md2_load_kitti_u8": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, P, P, C.c_int]),
    "md2_load_frames_native_u8": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, P, C.c_longlong,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "md2_resize_frames": (C.c_int, [C.POINTER(ResizeCfg), P, C.POINTER(C.c_longlong), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), P, P, P, P]),
    "md2_smooth_loss_workspace_size": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "md2_smooth_loss_fwd": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "md2_smooth_loss_bwd": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, P, P, P]),
    "md2_warp_photometric_workspace_size": (C.c_size_t, [C.POINTER(WarpCfg)]),
    "md2_warp_photometric_fwd": (C.c_int, [C.POINTER(WarpCfg), P, P, P, P, P, P, P, P]),
    "md2_warp_photometric_bwd": (C.c_int, [C.POINTER(WarpCfg), P, P, P, P, P, P, P, P, P]),
    "md2_loss_sources_workspace_size": (C.c_size_t, [C.POINTER(LossCfg), C.c_int]),
    "md2_loss_fwd_bwd_sources": (C.c_int, [C.POINTER(LossCfg), C.c_int, C.POINTER(LossSource), P, C.c_longlong,
                                           FP, P, P, C.c_float, C.POINTER(LossOut), P, P]),
    "md2_loss_fwd_bwd_sources_k": (C.c_int, [C.POINTER(LossCfg), C.c_int, C.POINTER(LossSource), P, C.c_longlong,
                                             P, P, FP, P, P, C.c_float, C.POINTER(LossOut), P, P]),
    "md2_automasking_loss_sources": (C.c_int, [C.c_int, C.POINTER(LossSource), P, C.c_longlong, C.c_int, C.c_int,
                                               C.c_int, C.c_int, P, P]),
    "md2_model_forward_loss_stereo": (C.c_int, [P, P, P, P, P, C.c_int, P, P, P, P]),
    "md2_model_train_step_graph_stereo": (C.c_int, [P, P, P, P, P, C.c_int, P, P, P, C.c_float, C.c_int, P, P]),
    "md2_model_set_profiling": (C.c_int, [P, C.c_int]),
    "md2_model_profile_read": (C.c_int, [P, C.POINTER(C.c_double), C.c_int]),
    "md2_model_profile_records": (C.c_int, [P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(C.c_int), C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
}


# the sources (stereo) entry points, added without an ABI bump
_SOURCES_SYMS = ("md2_loss_sources_workspace_size", "md2_loss_fwd_bwd_sources", "md2_automasking_loss_sources",
                 "md2_model_forward_loss_stereo", "md2_model_train_step_graph_stereo")
# per-sample intrinsics, added the same way
_INTRINSICS_SYMS = ("md2_loss_fwd_bwd_sources_k", "md2_model_set_intrinsics")
_BN_EX_SYMS = ("md2_maxpool3s2_bwd_ex", "md2_bn_ex_workspace_size", "md2_bn_channel_fits", "md2_bn_forward_ex",
               "md2_bn_backward_ex")


def lib():
    """Load libmd2hip.so once (raises if it is missing: there is no CPU fallback)."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libmd2hip.so not found at {LIB_PATH}: run `make -C monodepth2.jl_amd/csrc` "
                           "(or __graft_entry__.build()); the HIP path has no fallback")
    # torch must be imported first so that its HIP runtime is the one in the process
    import torch  # noqa: F401
    l = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        if name in _SOURCES_SYMS + _INTRINSICS_SYMS + _BN_EX_SYMS and os.environ.get("MD2HIP_LIB") is not None and not hasattr(l, name):
            continue     # an older library given for an A/B: it has no such entry points to call
        f = getattr(l, name)
        f.restype = res
        f.argtypes = args
    got = l.md2_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI version {got}, this binding expects {ABI_VERSION}: "
                           "rebuild the library or update md2hip")
    built = l.md2_build_id().decode()
    want = source_build_id()
    if want is not None and built != want and os.environ.get("MD2HIP_LIB") is None:
        raise RuntimeError(f"{LIB_PATH} was built from other sources (build id {built}, tree {want}): "
                           "stale library -- rebuild with `make -C monodepth2.jl_amd/csrc`")
    _lib = l
    return l


def declare(name, restype, argtypes):
    """Register the signature of an additional exported symbol."""
    _SIGS[name] = (restype, argtypes)
    if _lib is not None:
        f = getattr(_lib, name)
        f.restype = restype
        f.argtypes = argtypes


class MD2Error(RuntimeError):
    pass


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().md2_last_error().decode(errors="replace")
        raise MD2Error(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def ptr_array(ts, n=MAX_SCALES):
    arr = (C.c_void_p * n)()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def stream_of(device=None):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
