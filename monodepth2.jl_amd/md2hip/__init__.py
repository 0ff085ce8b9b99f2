"""md2hip -- MI355X-native hot path of the Monodepth2.jl training step.

Host-side mirror of the reference's Julia API (``Params``, ``TrainCache``, ``Model``,
``ResidualNetwork``, ``DepthDecoder``, ``PoseDecoder``, ``train_loss``, ``eval_disparity``,
``ADAM``) over the C-ABI of ``libmd2hip.so`` (include/md2.h).  There is no CPU fallback: every
op runs the HIP kernels and a missing library raises."""
from ._lib import MD2Error, lib  # noqa: F401
from .loss import (Params, TrainCache, depth10k_intrinsics, loss_tail, pack_poses,  # noqa: F401
                   stereo_transforms)
from .model import (ADAM, DepthDecoder, Model, Pose, PoseDecoder, ResidualNetwork, ResNet,  # noqa: F401
                    decode_guard_state, disparity_bins, eval_disparity, eval_pose, flux_params, grad_norm, gradient, param_table,
                    pullback, set_flux_params, train_loss, train_step)
from .slow_depth import SlowDepth, adam_update, slow_depth  # noqa: F401
from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401
from .data import (DataLoader, DChain, Depth10k, FlipX, KittyDataset, find_static, load_kitti_poses,  # noqa: F401
                   relative_poses)
from .mpi import MPIDepthDecoder, mpi_forward  # noqa: F401
from .evaluate import (METRIC_NAMES, chord_to_degrees, depth_errors, evaluate_depth, evaluate_pose,  # noqa: F401
                       garg_crop, pose_errors, pose_windows)
from .lidar import (kitti_odometry_velo_to_image, kitti_raw_velo_to_image, lidar_depth, load_velodyne,  # noqa: F401
                    post_process_disparity)
from .color import JITTER_DTYPE, ColorJitter, color_jitter, jitter_params  # noqa: F401
from .resize import decode_frames, load_frames, resize_frames  # noqa: F401

__all__ = ["Params", "TrainCache", "depth10k_intrinsics", "loss_tail", "pack_poses", "stereo_transforms", "lib", "MD2Error",
           "ADAM", "DepthDecoder", "Model", "Pose", "PoseDecoder", "ResidualNetwork", "ResNet",
           "disparity_bins", "eval_disparity", "flux_params", "gradient", "param_table", "pullback", "set_flux_params", "train_loss",
           "train_step",
           "SlowDepth", "adam_update", "slow_depth", "load_checkpoint", "save_checkpoint",
           "DataLoader", "DChain", "Depth10k", "FlipX", "KittyDataset", "find_static",
           "MPIDepthDecoder", "mpi_forward",
           "METRIC_NAMES", "depth_errors", "evaluate_depth", "garg_crop",
           "kitti_odometry_velo_to_image", "kitti_raw_velo_to_image", "lidar_depth", "load_velodyne",
           "post_process_disparity",
           "JITTER_DTYPE", "ColorJitter", "color_jitter", "jitter_params",
           "eval_pose", "pose_errors", "evaluate_pose", "pose_windows", "chord_to_degrees",
           "load_kitti_poses", "relative_poses",
           "grad_norm", "decode_guard_state",
           "resize_frames", "load_frames", "decode_frames"]
