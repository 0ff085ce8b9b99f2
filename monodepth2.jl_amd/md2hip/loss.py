"""Host mirror of the reference's loss API (src/Monodepth.jl:37-60, src/training.jl) over the
C-ABI.  Tensors are torch CUDA tensors in C order ([N,C,H,W]; x is [N,L,C,H,W])."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import LossCfg, check, lib, ptr, ptr_array, stream_of


@dataclass
class Params:
    """``Params`` (src/Monodepth.jl:37-47)."""
    target_size: Tuple[int, int]            # (width, height)
    batch_size: int
    min_depth: float = 0.1
    max_depth: float = 100.0
    disparity_smoothness: float = 1e-3
    frame_ids: List[int] = field(default_factory=lambda: [1, 2, 3])
    automasking: bool = True


@dataclass
class TrainCache:
    """``TrainCache`` (src/Monodepth.jl:49-60): intrinsics, frame ids (1-based), scales."""
    K: np.ndarray
    invK: np.ndarray
    target_id: int = 2
    source_ids: Sequence[int] = (1, 3)
    scales: Sequence[float] = (0.125, 0.25, 0.5, 1.0)


def depth10k_intrinsics(width=416, height=128):
    """Depth10k K / invK (src/dtk.jl:15-21)."""
    f = 2648.0 / 4.63461538462
    K = np.array([[f, 0, width / 2.0], [0, f, height / 2.0], [0, 0, 1.0]])
    return K, np.linalg.inv(K)


def _check_ids(cache: TrainCache):
    if len(cache.source_ids) != 2:
        raise ValueError("the HIP loss supports exactly two source frames (TrainCache.source_ids); "
                         "a stereo source is not a frame id -- pass it as x_stereo / stereo_Rt")


def make_loss_cfg(N, C_, W, H, disp_shapes, cache: TrainCache, params: Params, *,
                  smooth_weights=None, divisor=None, smooth_normalize=True,
                  L=3, sigmoid_grad=False) -> LossCfg:
    _check_ids(cache)
    cfg = LossCfg()
    cfg.n, cfg.c, cfg.width, cfg.height = N, C_, W, H
    cfg.nscales = len(disp_shapes)
    if cfg.nscales > _lib.MAX_SCALES:
        raise ValueError("at most 5 scales")
    for s, (h, w) in enumerate(disp_shapes):
        cfg.scale_w[s], cfg.scale_h[s] = w, h
        if smooth_weights is None:
            cfg.smooth_weight[s] = params.disparity_smoothness * float(cache.scales[s])
        else:
            cfg.smooth_weight[s] = smooth_weights[s]
    cfg.divisor = float(len(disp_shapes) if divisor is None else divisor)
    cfg.smooth_normalize = int(smooth_normalize)
    for i in range(9):
        cfg.K[i] = float(np.asarray(cache.K, dtype=np.float64).reshape(-1)[i])
        cfg.invK[i] = float(np.asarray(cache.invK, dtype=np.float64).reshape(-1)[i])
    cfg.min_depth, cfg.max_depth = params.min_depth, params.max_depth
    cfg.x_frame_stride = C_ * H * W
    cfg.x_sample_stride = L * C_ * H * W
    cfg.target = cache.target_id - 1
    cfg.src0, cfg.src1 = cache.source_ids[0] - 1, cache.source_ids[1] - 1
    cfg.invert_mask = sum(1 << s for s, sid in enumerate(cache.source_ids) if sid < cache.target_id)
    cfg.sigmoid_grad = int(sigmoid_grad)
    return cfg


def pack_poses(poses):
    """[(rvec [N,3], tvec [N,3])] x 2  ->  [2N, 6] (row s*N+i)."""
    import torch
    return torch.cat([torch.cat([r, t], 1) for r, t in poses], 0).contiguous()


def stereo_transforms(sides, flips=None, baseline=0.1):
    """Fixed transforms of the stereo partner, one per sample: [N, 12] float32 (NumPy), rows
    (R row-major, t) with R = I and t = (side_sign * flip_sign * baseline, 0, 0).

    sides: "l" / "r" per sample, the camera of the TARGET (side_sign -1 for "l", +1 for "r");
    flips: per sample, true where the sample is mirrored (flip_sign -1), None = none.  This is
    Monodepth2's ``stereo_T[0, 3] = side_sign * baseline_sign * 0.1``.  The baseline is 0.1 and not
    KITTI's 0.54 m on purpose: depths then come out in units of 5.4 m, the ``scale=5.4`` that
    ``depth_errors(median_scaling=False, scale=5.4)`` multiplies back in."""
    sides = list(sides)
    flips = [False] * len(sides) if flips is None else [bool(f) for f in flips]
    if len(flips) != len(sides):
        raise ValueError("sides and flips differ in length")
    Rt = np.zeros((len(sides), 12), dtype=np.float32)
    Rt[:, 0] = Rt[:, 4] = Rt[:, 8] = 1.0
    for i, (s, f) in enumerate(zip(sides, flips)):
        if s not in ("l", "r"):
            raise ValueError(f"side must be 'l' or 'r', got {s!r}")
        Rt[i, 9] = np.float32((-1.0 if s == "l" else 1.0) * (-1.0 if f else 1.0) * baseline)
    return Rt


def check_stereo(x, x_stereo, stereo_Rt):
    """Shape / dtype / device checks of a stereo source against x [N,3,C,H,W] (the kernels read raw
    pointers): x_stereo [N,C,H,W] and stereo_Rt [N,12], float32, contiguous, on x's device."""
    import torch
    N, L, C_, H, W = x.shape
    if stereo_Rt is None:
        raise ValueError("x_stereo needs stereo_Rt ([N, 12]; md2hip.stereo_transforms)")
    for name, t, shape in (("x_stereo", x_stereo, (N, C_, H, W)), ("stereo_Rt", stereo_Rt, (N, 12))):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if t.device != x.device:
            raise ValueError(f"{name} is on {t.device}, x on {x.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if L != 3:
        raise ValueError("x must hold 3 frames")


def check_intrinsics(K, invK, N, device):
    """Per-sample intrinsics of a batch of N as the kernels read them: (K, invK), float32 [N, 9]
    contiguous tensors on ``device``, or (None, None) when neither is given.  K / invK: float32
    tensors on ``device``, [N,3,3] or [N,9].  K alone: invK is computed on the host in fp64 and
    rounded once.  ValueError for a wrong type, shape, dtype or device, or invK without K."""
    import torch
    if K is None:
        if invK is not None:
            raise ValueError("invK needs K")
        return None, None
    out = []
    for name, t in (("K", K), ("invK", invK)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if tuple(t.shape) not in ((N, 3, 3), (N, 9)):
            raise ValueError(f"{name} must have shape {(N, 3, 3)} or {(N, 9)}, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if t.device != torch.device(device):
            raise ValueError(f"{name} is on {t.device}, x on {device}")
        out.append(t.reshape(N, 9).contiguous())
    if invK is None:
        inv = np.linalg.inv(out[0].detach().cpu().numpy().astype(np.float64).reshape(N, 3, 3))
        out.append(torch.from_numpy(inv.reshape(N, 9).astype(np.float32)).to(device))
    return out[0], out[1]


def stereo_sources(x, x_stereo, stereo_Rt, cache: TrainCache, temporal=True):
    """The ``md2_loss_source`` array of MS (temporal: the two temporal sources of ``cache``, learned,
    then the stereo frame, fixed -- Monodepth2's [0, -1, 1, "s"]) or of S (the stereo frame alone).
    ``x_stereo`` None (with temporal): the two temporal sources alone, M in the sources form.
    Returns (array, nsrc, n_learned)."""
    N, L, C_, H, W = x.shape
    fs = C_ * H * W
    ids = list(cache.source_ids) if temporal else []
    if temporal:
        _check_ids(cache)
    arr = (_lib.LossSource * _lib.MAX_SOURCES)()
    for s, sid in enumerate(ids):
        arr[s].frames = x.data_ptr() + 4 * (sid - 1) * fs
        arr[s].sample_stride = L * fs
        arr[s].pose_block = s
        arr[s].invert = int(sid < cache.target_id)
        arr[s].Rt = None
    k = len(ids)
    if x_stereo is None:
        if not temporal:
            raise ValueError("temporal=False needs x_stereo")
        return arr, k, k
    arr[k].frames = x_stereo.data_ptr()
    arr[k].sample_stride = fs
    arr[k].pose_block = -1
    arr[k].invert = 0
    arr[k].Rt = stereo_Rt.data_ptr()
    return arr, k + 1, k


def _results(disparities, x, nsrc, n_learned, grads, visualize):
    """The result dict of a loss-tail call over ``nsrc`` sources, ``n_learned`` of them learned, and
    the ``md2_loss_out`` that points into it."""
    import torch
    N, L, C_, H, W = x.shape
    dev, ns = x.device, len(disparities)
    res = {"loss": torch.empty(1, dtype=torch.float32, device=dev),
           "terms": torch.empty(ns, 2, dtype=torch.float32, device=dev),
           "d_disp": [torch.empty_like(d) for d in disparities] if grads else [None] * ns,
           "d_pose": (torch.empty(n_learned * N, 6, dtype=torch.float32, device=dev)
                      if grads and n_learned > 0 else None)}
    if visualize:
        res["vis_loss"] = torch.empty(ns, N, H, W, dtype=torch.float32, device=dev)
        res["vis_sel"] = torch.empty(ns, N, H, W, dtype=torch.int8, device=dev)
        res["vis_warped"] = torch.empty(nsrc, N, C_, H, W, dtype=torch.float32, device=dev)
        # per-pixel bilinear cells / border states of every source (parity diagnostics)
        res["vis_cell"] = torch.empty(ns, nsrc, N, H, W, dtype=torch.int32, device=dev)
    out = _lib.LossOut()
    out.loss = res["loss"].data_ptr()
    out.terms = res["terms"].data_ptr()
    for i, d in enumerate(res["d_disp"]):
        out.d_disp[i] = None if d is None else d.data_ptr()
    out.d_pose = None if res["d_pose"] is None else res["d_pose"].data_ptr()
    out.vis_loss = res["vis_loss"].data_ptr() if visualize else None
    out.vis_sel = res["vis_sel"].data_ptr() if visualize else None
    out.vis_warped = res["vis_warped"].data_ptr() if visualize else None
    out.vis_cell = res["vis_cell"].data_ptr() if visualize else None
    return res, out


def loss_tail(disparities, poses, x, auto_loss, cache: TrainCache, params: Params, *,
              grads=True, smooth_weights=None, divisor=None, smooth_normalize=True,
              dloss=1.0, sigmoid_grad=False, visualize=False, keep_workspace=False,
              x_stereo=None, stereo_Rt=None, temporal=True, K=None, invK=None):
    """The body of ``train_loss`` after the model call (src/training.jl:25-77) and its pullback.

    disparities: list of [N,1,h,w] float32 CUDA tensors (one per scale); poses: list of
    (rvec [N,3], tvec [N,3]) per source; x: [N,L,C,H,W]; auto_loss: [N,1,H,W] or None.
    Returns a dict: loss [1], terms [nscales,2], d_disp (list), d_pose [2N,6] and, with
    ``visualize``, vis_loss / vis_sel [nscales,N,H,W] (training.jl:71-74 vis_loss) and
    vis_warped [2,N,C,H,W] (both sources warped by the last scale, training.jl:71-73).
    ``keep_workspace`` (diagnostics): also return the raw workspace as "workspace".

    Stereo supervision: with ``x_stereo`` [N,C,H,W] (the other camera's frame at the target's time)
    and ``stereo_Rt`` [N,12] (``stereo_transforms``) the loss runs over the sources
    (source_ids[0], source_ids[1], stereo) -- "MS", ``temporal=True`` -- or over the stereo frame
    alone -- "S", ``temporal=False``, where ``poses`` is not read and d_pose is None.  The stereo
    transform is data: it gets no gradient.  vis_sel then holds 0..S-1 (the stereo frame last) or
    -1, vis_warped is [S,N,C,H,W] and vis_cell [nscales,S,N,H,W]; an ``auto_loss`` of None is
    computed over the same sources.

    Per-sample intrinsics: ``K`` (and optionally ``invK``) float32 device tensors [N,3,3] or [N,9];
    sample i is warped by row i and cache.K / invK are not read (md2_loss_fwd_bwd_sources_k).  K
    alone: invK is computed on the host in fp64 and rounded once.  The call then runs on the
    kernel over sources whatever the number of sources; rows all equal to cache.K / invK give the
    bits of the call without them."""
    import torch
    K, invK = check_intrinsics(K, invK, x.shape[0], x.device)
    if x_stereo is not None or K is not None:
        if x_stereo is None and (stereo_Rt is not None or not temporal):
            raise ValueError("stereo_Rt / temporal=False need x_stereo")
        return _loss_tail_sources(disparities, poses, x, auto_loss, cache, params, x_stereo, stereo_Rt,
                                  temporal, K=K, invK=invK, grads=grads, smooth_weights=smooth_weights, divisor=divisor,
                                  smooth_normalize=smooth_normalize, dloss=dloss, sigmoid_grad=sigmoid_grad,
                                  visualize=visualize, keep_workspace=keep_workspace)
    if stereo_Rt is not None or not temporal:
        raise ValueError("stereo_Rt / temporal=False need x_stereo")
    N, L, C_, H, W = x.shape
    dev = x.device
    for d in disparities:
        assert d.dtype == torch.float32 and d.is_contiguous() and d.device == dev
    assert x.dtype == torch.float32 and x.is_contiguous()
    shapes = [(d.shape[-2], d.shape[-1]) for d in disparities]
    cfg = make_loss_cfg(N, C_, W, H, shapes, cache, params, smooth_weights=smooth_weights,
                        divisor=divisor, smooth_normalize=smooth_normalize, L=L,
                        sigmoid_grad=sigmoid_grad)
    pose = pack_poses(poses).to(dev, torch.float32)
    ws_bytes = lib().md2_loss_workspace_size(C.byref(cfg))
    ws = torch.empty(ws_bytes // 4 + 64, dtype=torch.float32, device=dev)
    res, out = _results(disparities, x, 2, 2, grads, visualize)
    if keep_workspace:
        res["workspace"] = ws
    am = None
    if params.automasking:
        if auto_loss is None:        # automasking_loss(ssim, x, target; source_ids), on the GPU
            from .primitives import automasking_loss
            auto_loss = automasking_loss(x, cache.target_id, cache.source_ids)
        am = auto_loss.contiguous()
    disp_arr = ptr_array(disparities)
    check(lib().md2_loss_fwd_bwd(C.byref(cfg), C.cast(disp_arr, _lib.FP), ptr(pose), ptr(x), ptr(am),
                                 C.c_float(dloss), C.byref(out), ptr(ws), stream_of(dev)),
          "md2_loss_fwd_bwd")
    return res


def _sources_cfg(N, C_, W, H, shapes, cache, params, **kw):
    """md2_loss_cfg of the sources form: the frame ids and strides of cfg are not read there."""
    two = TrainCache(K=cache.K, invK=cache.invK, target_id=cache.target_id, source_ids=(1, 3),
                     scales=cache.scales)
    return make_loss_cfg(N, C_, W, H, shapes, two, params, **kw)


def run_loss_sources(disparities, pose, x, target, target_stride, sources, nsrc, n_learned, auto_loss,
                     cache, params, *, grads=True, smooth_weights=None, divisor=None,
                     smooth_normalize=True, dloss=1.0, sigmoid_grad=False, visualize=False,
                     keep_workspace=False, K=None, invK=None):
    """md2_loss_fwd_bwd_sources on an ``md2_loss_source`` array (``stereo_sources``; the tests build
    their own).  x only gives the shape [N,L,C,H,W] and the device; target is a device address.
    ``K`` / ``invK`` (``check_intrinsics``): per-sample intrinsics, md2_loss_fwd_bwd_sources_k."""
    import torch
    N, L, C_, H, W = x.shape
    dev = x.device
    K, invK = check_intrinsics(K, invK, N, dev)
    for d in disparities:
        assert d.dtype == torch.float32 and d.is_contiguous() and d.device == dev
    shapes = [(d.shape[-2], d.shape[-1]) for d in disparities]
    cfg = _sources_cfg(N, C_, W, H, shapes, cache, params, smooth_weights=smooth_weights,
                       divisor=divisor, smooth_normalize=smooth_normalize, L=L, sigmoid_grad=sigmoid_grad)
    ws_bytes = lib().md2_loss_sources_workspace_size(C.byref(cfg), nsrc)
    ws = torch.empty(ws_bytes // 4 + 64, dtype=torch.float32, device=dev)
    res, out = _results(disparities, x, nsrc, n_learned, grads, visualize)
    if keep_workspace:
        res["workspace"] = ws
    am = None
    if params.automasking:
        if auto_loss is None:
            am = torch.empty(N, 1, H, W, dtype=torch.float32, device=dev)
            check(lib().md2_automasking_loss_sources(nsrc, sources, C.c_void_p(target), target_stride, N, C_,
                                                     H, W, ptr(am), stream_of(dev)),
                  "md2_automasking_loss_sources")
        else:
            am = auto_loss.contiguous()
            if tuple(am.shape) != (N, 1, H, W) or am.dtype != torch.float32 or am.device != dev:
                raise ValueError(f"auto_loss must be float32 [N,1,H,W] = {(N, 1, H, W)} on {dev}")
    disp_arr = ptr_array(disparities)
    if K is not None:
        check(lib().md2_loss_fwd_bwd_sources_k(C.byref(cfg), nsrc, sources, C.c_void_p(target), target_stride,
                                               ptr(K), ptr(invK), C.cast(disp_arr, _lib.FP), ptr(pose), ptr(am),
                                               C.c_float(dloss), C.byref(out), ptr(ws), stream_of(dev)),
              "md2_loss_fwd_bwd_sources_k")
        return res
    check(lib().md2_loss_fwd_bwd_sources(C.byref(cfg), nsrc, sources, C.c_void_p(target), target_stride,
                                         C.cast(disp_arr, _lib.FP), ptr(pose), ptr(am), C.c_float(dloss),
                                         C.byref(out), ptr(ws), stream_of(dev)),
          "md2_loss_fwd_bwd_sources")
    return res


def _loss_tail_sources(disparities, poses, x, auto_loss, cache, params, x_stereo, stereo_Rt, temporal, **kw):
    import torch
    assert x.dtype == torch.float32 and x.is_contiguous()
    if x_stereo is not None:
        check_stereo(x, x_stereo, stereo_Rt)
    N, L, C_, H, W = x.shape
    sources, nsrc, n_learned = stereo_sources(x, x_stereo, stereo_Rt, cache, temporal)
    pose = pack_poses(poses).to(x.device, torch.float32) if temporal else None
    if pose is not None and tuple(pose.shape) != (2 * N, 6):
        raise ValueError(f"poses must pack to [2N, 6] = {(2 * N, 6)}, got {tuple(pose.shape)}")
    target = x.data_ptr() + 4 * (cache.target_id - 1) * C_ * H * W
    return run_loss_sources(disparities, pose, x, target, L * C_ * H * W, sources, nsrc, n_learned,
                            auto_loss, cache, params, **kw)
