"""Depth evaluation on the device: the Monodepth2 / Eigen protocol (median scaling, Garg crop,
the seven error metrics) over the C-ABI (``md2_depth_eval``, include/md2.h).  No CPU fallback.

``depth_errors`` scores one batch of disparities against ground-truth depth in one batched call
and returns device tensors without a sync; ``evaluate_depth`` runs a model over a dataset's
batches, accumulates on the device and syncs once."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import DepthEvalCfg, check, lib, ptr, stream_of

METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "ratio", "med_gt", "med_pred")


def garg_crop(gt_h: int, gt_w: int):
    """The Garg et al. evaluation crop of a ``gt_h x gt_w`` depth map as ``(y0, y1, x0, x1)``,
    half-open, in pixels (Monodepth2's evaluate_depth.py)."""
    return (int(0.40810811 * gt_h), int(0.99189189 * gt_h), int(0.03594771 * gt_w), int(0.96405229 * gt_w))


def _check_f32_cuda(t, what):
    import torch
    if t.dtype != torch.float32 or t.device.type != "cuda" or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor")


def depth_errors(disp, gt, *, crop="garg", min_depth=0.1, max_depth=100.0, eval_min=1e-3, eval_max=80.0,
                 median_scaling=True, scale=1.0):
    """Per-image depth errors of sigmoid disparities ``disp`` ([N, 1, h, w] or [N, h, w], any
    level) against ground-truth depth ``gt`` ([N, Hg, Wg]; 0 or out-of-range = no measurement).

    The disparity is scaled to ``1/max_depth .. 1/min_depth``, resized to the ground truth's size
    (half-pixel-centre bilinear), inverted, masked by ``eval_min < gt < eval_max`` and ``crop``
    (``"garg"``, ``None`` for the whole image, or ``(y0, y1, x0, x1)``), scaled by the per-image
    ratio of medians (or by ``scale``) and clamped to the evaluation range; include/md2.h states
    every step.  Returns ``(metrics [N, 10] float32, counts [N, 2] int32)`` on the device, columns
    ``METRIC_NAMES`` and ``(count, n_bad)``; an image without a valid pixel gives NaNs and count 0.
    Bitwise reproducible; enqueues on the current stream and does not synchronise."""
    import torch
    if not isinstance(disp, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise ValueError("disp and gt must be torch tensors")
    if not (disp.dim() == 3 or (disp.dim() == 4 and disp.shape[1] == 1)):
        raise ValueError("disp must be [N, 1, h, w] or [N, h, w]")
    if gt.dim() != 3:
        raise ValueError("gt must be [N, Hg, Wg]")
    if disp.shape[0] != gt.shape[0]:
        raise ValueError(f"batch mismatch: disp has {disp.shape[0]} images, gt {gt.shape[0]}")
    _check_f32_cuda(disp, "disp")
    _check_f32_cuda(gt, "gt")
    if disp.device != gt.device:
        raise ValueError("disp and gt must be on the same device")
    if disp.dim() == 4:
        disp = disp[:, 0]
    N, h, w = (int(v) for v in disp.shape)
    Hg, Wg = int(gt.shape[1]), int(gt.shape[2])
    if isinstance(crop, str):
        if crop != "garg":
            raise ValueError('crop must be "garg", None or (y0, y1, x0, x1)')
        crop = garg_crop(Hg, Wg)
    elif crop is None:
        crop = (0, Hg, 0, Wg)
    y0, y1, x0, x1 = (int(v) for v in crop)
    cfg = DepthEvalCfg(N, h, w, Hg, Wg, y0, y1, x0, x1, min_depth, max_depth, eval_min, eval_max,
                       1 if median_scaling else 0, scale)
    nbytes = lib().md2_depth_eval_workspace_size(C.byref(cfg))
    with torch.cuda.device(disp.device):
        metrics = torch.empty(N, len(METRIC_NAMES), dtype=torch.float32, device=disp.device)
        counts = torch.empty(N, 2, dtype=torch.int32, device=disp.device)
        # an invalid cfg has size 0: the call below reports why
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=disp.device)
        check(lib().md2_depth_eval(C.byref(cfg), ptr(disp), ptr(gt), ptr(metrics), ptr(counts), ptr(ws),
                                   stream_of(disp.device)), "md2_depth_eval")
    return metrics, counts


def evaluate_depth(model, batches, *, allow_nonfinite=False, post_process=False, **depth_errors_kwargs):
    """Score ``model`` over ``batches``, an iterable of ``(x [n, C, H, W], gt [n, Hg, Wg])`` device
    pairs: ``md2hip.eval_disparity(model, x)`` in whatever mode the model is in -- call
    ``model.testmode()`` first, so that BatchNorm uses its running statistics and an image's score
    does not depend on its batch -- then ``depth_errors`` on the last (full-resolution) level.
    Everything accumulates on the device; the host syncs once at the end.  ``post_process=True``
    scores Monodepth's flip post-processing instead ("+pp"): each batch is also predicted mirrored,
    ``eval_disparity(model, x.flip(-1))``, and the two disparities are blended by
    ``post_process_disparity``.

    Returns a dict: the mean over the images with ``count > 0`` of ``abs_rel, sq_rel, rmse,
    rmse_log, a1, a2, a3``; ``ratio_median`` and ``ratio_std`` (the standard deviation of
    ``ratio / ratio_median``, as Monodepth2 prints them); ``images``, ``skipped`` (images with
    ``count == 0``), ``n_bad`` (masked pixels whose prediction was not finite and positive, in
    total) and ``nonfinite_inputs`` (elements of the frames ``x`` that are NaN or infinite).  The
    frames are checked as well as the predictions because the network hides them: its ReLUs are
    ``fmaxf(v, 0)``, which turns a NaN into 0, so a NaN pixel yields a finite, meaningless disparity.
    ``n_bad > 0`` or ``nonfinite_inputs > 0`` raises ``RuntimeError`` unless ``allow_nonfinite``."""
    import torch
    from .lidar import post_process_disparity
    from .model import eval_disparity
    ms, cs, bad_in = [], [], None
    for x, gt in batches:
        nf = (~torch.isfinite(x)).sum()                     # stays on the device
        bad_in = nf if bad_in is None else bad_in + nf
        disp = eval_disparity(model, x)[-1]
        if post_process:
            # eval_disparity returns views of executor-owned buffers that the next call overwrites:
            # the first result is cloned before the mirrored frame runs, and the blend lands in the clone
            disp = disp.clone()
            post_process_disparity(disp, eval_disparity(model, x.flip(-1))[-1], out=disp)
        m, c = depth_errors(disp, gt, **depth_errors_kwargs)
        ms.append(m)
        cs.append(c)
    if not ms:
        raise ValueError("evaluate_depth: no batches")
    m = torch.cat(ms).cpu().numpy().astype(np.float64)      # the one sync
    c = torch.cat(cs).cpu().numpy()
    bad_in = int(bad_in.cpu())
    n_bad = int(c[:, 1].sum())
    if (n_bad or bad_in) and not allow_nonfinite:
        raise RuntimeError(f"evaluate_depth: {n_bad} masked pixels have a prediction that is not finite and "
                           f"positive, {bad_in} input elements are not finite (pass allow_nonfinite=True to "
                           "score regardless)")
    ok = c[:, 0] > 0
    out = {}
    for k, name in enumerate(METRIC_NAMES[:7]):
        out[name] = float(m[ok, k].mean()) if ok.any() else float("nan")
    ratios = m[ok, 7]
    med = float(np.median(ratios)) if ok.any() else float("nan")
    out["ratio_median"] = med
    out["ratio_std"] = float(np.std(ratios / med)) if ok.any() else float("nan")
    out["images"] = int(len(c))
    out["skipped"] = int((~ok).sum())
    out["n_bad"] = n_bad
    out["nonfinite_inputs"] = bad_in
    return out
