"""Ground-truth depth maps from LiDAR scans and the flip post-processing of disparities, on the
device over the C-ABI (``md2_lidar_depth``, ``md2_disp_post_process``; include/md2.h states every
operation).  No CPU fallback.

``lidar_depth`` rasterises a batch of Velodyne scans into the depth maps ``depth_errors`` scores
against; ``post_process_disparity`` is the "+pp" blend of a prediction with the prediction for the
mirrored frame.  The host helpers (NumPy only) read KITTI's scan and calibration files."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import LIDAR_MAX_SCANS, LidarCfg, check, lib, ptr, stream_of


# ---- host helpers -------------------------------------------------------------------------------
def load_velodyne(path):
    """A KITTI ``velodyne/NNNNNN.bin`` scan as float32 ``[M, 4]`` (x, y, z, reflectance)."""
    import os
    size = os.path.getsize(path)
    if size % 16:
        raise ValueError(f"{path}: {size} bytes is not a whole number of 16-byte points")
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def _calib_rows(path, keys):
    """``{key: float64 vector}`` of the ``key: v v v ...`` lines of a KITTI calibration file."""
    out = {}
    with open(path) as f:
        for line in f:
            key, sep, rest = line.partition(":")
            if sep and key.strip() in keys:
                out[key.strip()] = np.array([float(v) for v in rest.split()], dtype=np.float64)
    missing = [k for k in keys if k not in out]
    if missing:
        raise ValueError(f"{path}: no line {', '.join(k + ':' for k in missing)}")
    return out


def _homogeneous(m34):
    return np.vstack([m34, [0.0, 0.0, 0.0, 1.0]])


def kitti_odometry_velo_to_image(calib_path, cam=0):
    """The velodyne -> image matrix of camera ``cam`` (0..3) of a KITTI odometry sequence,
    ``P{cam} @ [Tr; 0 0 0 1]`` from its ``calib.txt``: float32 ``[3, 4]``, composed in float64 and
    rounded once."""
    pk = f"P{int(cam)}"
    rows = _calib_rows(calib_path, (pk, "Tr"))
    if rows[pk].size != 12 or rows["Tr"].size != 12:
        raise ValueError(f"{calib_path}: {pk}: and Tr: must hold 12 values each")
    return (rows[pk].reshape(3, 4) @ _homogeneous(rows["Tr"].reshape(3, 4))).astype(np.float32)


def kitti_raw_velo_to_image(cam_to_cam_path, velo_to_cam_path, cam=2):
    """The velodyne -> image matrix of camera ``cam`` of a KITTI raw drive,
    ``P_rect_0{cam} @ R_rect_00 @ [R|T]`` (``calib_cam_to_cam.txt``, ``calib_velo_to_cam.txt``), as
    Monodepth2's generate_depth_map composes it: float32 ``[3, 4]``, composed in float64 and
    rounded once."""
    pk = f"P_rect_0{int(cam)}"
    cc = _calib_rows(cam_to_cam_path, (pk, "R_rect_00"))
    vc = _calib_rows(velo_to_cam_path, ("R", "T"))
    if cc[pk].size != 12 or cc["R_rect_00"].size != 9 or vc["R"].size != 9 or vc["T"].size != 3:
        raise ValueError("KITTI raw calibration: P_rect needs 12 values, R_rect_00 and R 9, T 3")
    rect = np.eye(4)
    rect[:3, :3] = cc["R_rect_00"].reshape(3, 3)
    velo = _homogeneous(np.hstack([vc["R"].reshape(3, 3), vc["T"].reshape(3, 1)]))
    return (cc[pk].reshape(3, 4) @ rect @ velo).astype(np.float32)


# ---- device -------------------------------------------------------------------------------------
def _points_and_offsets(scans):
    import torch

    def bad(t):
        return (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda"
                or t.dim() != 2 or t.shape[1] != 4)
    # a pair (points, offsets): the second entry is 1-D, which no scan is
    if isinstance(scans, tuple) and len(scans) == 2 and isinstance(scans[0], torch.Tensor) \
            and not (isinstance(scans[1], torch.Tensor) and scans[1].dim() == 2):
        points, offsets = scans
        if bad(points) or not points.is_contiguous():
            raise ValueError("points must be a contiguous [M, 4] float32 CUDA tensor")
        offsets = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets)
        if offsets.ndim != 1 or offsets.size < 2 or offsets.dtype.kind not in "iu":
            raise ValueError("offsets must be a 1-D integer sequence of N + 1 entries")
        offsets = offsets.astype(np.int64)
        if offsets[0] < 0 or (np.diff(offsets) < 0).any() or offsets[-1] > points.shape[0]:
            raise ValueError("offsets must start at >= 0, not decrease and end within points")
        return points, offsets
    if not isinstance(scans, (list, tuple)) or len(scans) == 0:
        raise ValueError("scans must be a non-empty list of [M_i, 4] tensors or a pair (points, offsets)")
    for t in scans:
        if bad(t):
            raise ValueError("every scan must be an [M_i, 4] float32 CUDA tensor")
        if t.device != scans[0].device:
            raise ValueError("all scans must be on the same device")
    offsets = np.concatenate([[0], np.cumsum([int(t.shape[0]) for t in scans])]).astype(np.int64)
    points = scans[0].contiguous() if len(scans) == 1 else torch.cat(list(scans))
    return points, offsets


def lidar_depth(scans, P, height, width, *, forward_only=True, vel_depth=False, return_counts=False):
    """Depth maps ``[N, height, width]`` (float32, on the scans' device; 0 = no measurement) of N
    LiDAR scans: every point is projected with its scan's velodyne -> image matrix, rounded to a
    pixel (KITTI's "minus one" convention) and the nearest point of a pixel wins, as Monodepth2's
    generate_depth_map does; include/md2.h states every operation.

    ``scans`` is a list of ``[M_i, 4]`` float32 CUDA tensors (x, y, z, reflectance; an empty scan
    gives an all-zero map) or a pair ``(points [M, 4], offsets)`` with ``N + 1`` host offsets into
    ``points``.  ``P`` is ``[N, 3, 4]``, or ``[3, 4]`` for all scans, as NumPy or a CPU tensor
    (``kitti_odometry_velo_to_image`` / ``kitti_raw_velo_to_image``); scale its rows 0 and 1 to
    rasterise at another size than the camera's.  ``forward_only`` drops points behind the sensor
    (x < 0); ``vel_depth`` stores the velodyne x instead of the camera z.  ``return_counts`` adds
    ``counts [N, 2] int32 = (points stored, pixels hit)``.  Bitwise reproducible; enqueues on the
    current stream and does not synchronise.  More than 64 scans go through in chunks of 64."""
    import torch
    points, offsets = _points_and_offsets(scans)
    N = int(offsets.size) - 1
    P = np.asarray(P.detach().cpu() if isinstance(P, torch.Tensor) else P)
    if P.dtype.kind != "f":
        raise ValueError("P must be a floating-point array")
    if P.shape == (3, 4):
        P = np.broadcast_to(P, (N, 3, 4))
    if P.shape != (N, 3, 4):
        raise ValueError(f"P must be [3, 4] or [{N}, 3, 4] for {N} scans, got {list(P.shape)}")
    P = np.ascontiguousarray(P, dtype=np.float32)
    H, W = int(height), int(width)
    dev = points.device
    with torch.cuda.device(dev):
        depth = torch.empty(N, H, W, dtype=torch.float32, device=dev)
        counts = torch.empty(N, 2, dtype=torch.int32, device=dev) if return_counts else None
        for a in range(0, N, LIDAR_MAX_SCANS):
            b = min(N, a + LIDAR_MAX_SCANS)
            # offsets relative to the chunk's first point: the library caps offsets[n], not the batch
            base = int(offsets[a])
            off = (C.c_longlong * (b - a + 1))(*(int(o) - base for o in offsets[a:b + 1]))
            cfg = LidarCfg(b - a, H, W, 1 if forward_only else 0, 1 if vel_depth else 0)
            pts = C.c_void_p(points.data_ptr() + 16 * base) if points.numel() else None
            check(lib().md2_lidar_depth(C.byref(cfg), pts, off, P[a:b].ctypes.data_as(C.POINTER(C.c_float)),
                                        ptr(depth[a:b]), None if counts is None else ptr(counts[a:b]),
                                        stream_of(dev)), "md2_lidar_depth")
    return (depth, counts) if return_counts else depth


def post_process_disparity(disp, disp_flipped, *, out=None):
    """Monodepth's flip post-processing ("+pp"): ``disp`` ([N, 1, h, w] or [N, h, w]) blended with
    ``disp_flipped``, the network's output for the horizontally mirrored frame as produced (not
    mirrored back) -- their mean in the middle, each side's own prediction on the 5 % of the width
    next to the edge it sees best, linear ramps in between (include/md2.h).  Returns a tensor of
    ``disp``'s shape; ``out`` may be ``disp`` itself, never ``disp_flipped``.  Enqueues on the
    current stream and does not synchronise."""
    import torch
    for t, what in ((disp, "disp"), (disp_flipped, "disp_flipped")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" \
                or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 CUDA tensor")
    if not (disp.dim() == 3 or (disp.dim() == 4 and disp.shape[1] == 1)):
        raise ValueError("disp must be [N, 1, h, w] or [N, h, w]")
    if disp_flipped.shape != disp.shape or disp_flipped.device != disp.device:
        raise ValueError("disp_flipped must have disp's shape and device")
    if out is None:
        out = torch.empty_like(disp)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != disp.device \
            or out.shape != disp.shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of disp's shape and device")
    if out.data_ptr() == disp_flipped.data_ptr() and out.numel():
        raise ValueError("out must not alias disp_flipped")
    n, h, w = int(disp.shape[0]), int(disp.shape[-2]), int(disp.shape[-1])
    with torch.cuda.device(disp.device):
        check(lib().md2_disp_post_process(ptr(disp), ptr(disp_flipped), n, h, w, ptr(out), stream_of(disp.device)),
              "md2_disp_post_process")
    return out
