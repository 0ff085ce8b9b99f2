"""Depth evaluation on the device: the Monodepth2 / Eigen protocol (median scaling, Garg crop,
the seven error metrics) over the C-ABI (``md2_depth_eval``, include/md2.h).  No CPU fallback.

``depth_errors`` scores one batch of disparities against ground-truth depth in one batched call
and returns device tensors without a sync; ``evaluate_depth`` runs a model over a dataset's
batches, accumulates on the device and syncs once.

Odometry evaluation (``md2_pose_eval``): ``pose_errors`` scores predicted pose steps against
ground-truth steps over 5-frame snippets (scale-aligned absolute trajectory error and a rotation
error) without a sync; ``evaluate_pose`` runs ``eval_pose`` over a sequence's windows and syncs
once."""
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


def _snippet_counts(offsets, track_length):
    return np.maximum(np.diff(offsets) - track_length + 2, 0)


def pose_errors(pred, gt_rel, offsets=None, track_length=5, invert=True, *, rt_out=None):
    """Monodepth2's odometry metric of predicted steps ``pred [M, 6]`` (raw ``(rvec, tvec)`` rows,
    e.g. ``eval_pose`` outputs concatenated) against ground-truth steps ``gt_rel [M, 12]``
    (``md2hip.data.relative_poses``), both float32 on the GPU (``md2_pose_eval``; include/md2.h
    states every operation).

    ``offsets`` (``nseq + 1`` host integers from 0 to M; default: one sequence) splits the steps
    into sequences.  Every run of ``track_length - 1`` consecutive steps of a sequence is a snippet
    of ``track_length`` frames: both trajectories are chained from the identity, the prediction is
    scaled onto the ground truth by least squares, and the snippet's ``ate`` is the root of the
    summed squared position error divided by the number of frames (Monodepth2's ``compute_ate``).
    ``invert=True`` inverts every predicted step first -- the network's pair output maps camera-k
    points into camera k+1, the chain wants the pose of camera k+1 in camera k's frame;
    ``invert=False`` chains the raw output as Monodepth2's evaluate_pose.py does.

    Returns ``(per_snippet [S, 3] = (ate, scale, rot_chord), summary [nseq, 4] = (mean_ate, std_ate,
    mean_scale, mean_rot_chord), counts [nseq, 2] int32 = (snippets, n_bad))`` on the device.
    ``rot_chord`` is the Frobenius distance of the final rotations, ``2 sqrt(2) sin(angle / 2)``
    (``chord_to_degrees``); a snippet with a non-finite value counts in ``n_bad`` and is left out of
    the summary, a sequence without a finite snippet gives NaNs.  ``rt_out`` (``[M, 12]`` float32,
    optional) receives the predicted step transforms.  Bitwise reproducible; enqueues on the current
    stream and does not synchronise.  More than 64 sequences go through in chunks of 64."""
    import torch
    from ._lib import POSE_EVAL_MAX_SEQ, POSE_EVAL_MAX_TRACK
    if not isinstance(pred, torch.Tensor) or not isinstance(gt_rel, torch.Tensor):
        raise ValueError("pred and gt_rel must be torch tensors")
    _check_f32_cuda(pred, "pred")
    _check_f32_cuda(gt_rel, "gt_rel")
    if pred.dim() != 2 or pred.shape[1] != 6:
        raise ValueError("pred must be [M, 6]")
    M = int(pred.shape[0])
    if tuple(gt_rel.shape) != (M, 12):
        raise ValueError(f"gt_rel must be [{M}, 12] for {M} predicted steps")
    if pred.device != gt_rel.device:
        raise ValueError("pred and gt_rel must be on the same device")
    L = int(track_length)
    if not 2 <= L <= POSE_EVAL_MAX_TRACK:
        raise ValueError(f"track_length must be in 2..{POSE_EVAL_MAX_TRACK}")
    if offsets is None:
        offsets = [0, M]
    offsets = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets)
    if offsets.ndim != 1 or offsets.size < 2 or offsets.dtype.kind not in "iu":
        raise ValueError("offsets must be a 1-D integer sequence of nseq + 1 entries")
    offsets = offsets.astype(np.int64)
    if offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != M:
        raise ValueError("offsets must start at 0, not decrease and end at the number of steps")
    if rt_out is not None:
        _check_f32_cuda(rt_out, "rt_out")
        if tuple(rt_out.shape) != (M, 12) or rt_out.device != pred.device:
            raise ValueError(f"rt_out must be [{M}, 12] on pred's device")
    nseq = int(offsets.size) - 1
    snips = _snippet_counts(offsets, L)
    soff = np.concatenate([[0], np.cumsum(snips)]).astype(np.int64)
    dev = pred.device

    def at(t, row):          # pointer to a row of a contiguous 2-D tensor (NULL for an empty one)
        return C.c_void_p(t.data_ptr() + row * t.stride(0) * t.element_size()) if t.numel() else None
    with torch.cuda.device(dev):
        out = torch.empty(int(soff[-1]), 3, dtype=torch.float32, device=dev)
        summary = torch.empty(nseq, 4, dtype=torch.float32, device=dev)
        counts = torch.empty(nseq, 2, dtype=torch.int32, device=dev)
        longest = max(int(offsets[min(nseq, a + POSE_EVAL_MAX_SEQ)] - offsets[a])
                      for a in range(0, nseq, POSE_EVAL_MAX_SEQ))
        ws = torch.empty(max(int(lib().md2_pose_eval_workspace_size(longest)), 256), dtype=torch.uint8, device=dev)
        for a in range(0, nseq, POSE_EVAL_MAX_SEQ):
            b = min(nseq, a + POSE_EVAL_MAX_SEQ)
            base = int(offsets[a])                  # the library wants offsets[0] == 0: rebase the chunk
            off = (C.c_longlong * (b - a + 1))(*(int(o) - base for o in offsets[a:b + 1]))
            check(lib().md2_pose_eval(at(pred, base), at(gt_rel, base), off, b - a, L, 1 if invert else 0,
                                      at(out, int(soff[a])), ptr(summary[a:b]), ptr(counts[a:b]),
                                      None if rt_out is None else at(rt_out, base), ptr(ws), stream_of(dev)),
                  "md2_pose_eval")
    return out, summary, counts


def chord_to_degrees(chord):
    """The rotation angle in degrees of a ``rot_chord`` (NumPy, host): ``chord = 2 sqrt(2)
    sin(angle / 2)``, clipped at the largest possible chord."""
    c = np.clip(np.asarray(chord, dtype=np.float64) / (2.0 * np.sqrt(2.0)), 0.0, 1.0)
    return np.degrees(2.0 * np.arcsin(c))


def pose_windows(x_seq, max_pairs):
    """The frames ``x_seq [F, C, H, W]`` of one sequence cut into windows of at most ``max_pairs + 1``
    frames that overlap by one frame, so that the windows' pairs are the sequence's F - 1 consecutive
    pairs, each once: what ``evaluate_pose`` takes as ``frames``.  ``max_pairs`` is twice the batch
    of the executor that will run them (``eval_pose`` accepts 2 * batch + 1 frames).  Views of
    ``x_seq``, made contiguous where they are not."""
    F = int(x_seq.shape[0])
    max_pairs = int(max_pairs)
    if max_pairs < 1:
        raise ValueError("max_pairs must be at least 1")
    if F < 2:
        raise ValueError("a sequence needs at least two frames")
    return [x_seq[a:min(F, a + max_pairs + 1)].contiguous() for a in range(0, F - 1, max_pairs)]


def evaluate_pose(model, frames, gt_rel, *, track_length=5, allow_nonfinite=False):
    """Score ``model``'s PoseDecoder over one sequence: ``frames`` is an iterable of ``[n, C, H, W]``
    device windows that overlap by one frame (the last frame of a window is the first of the next;
    the caller builds them, ``pose_windows(x_seq, max_pairs)`` does it for frames already on the
    device), ``gt_rel [M, 12]`` the ground-truth steps of the M pairs the windows cover together
    (``md2hip.data.relative_poses(load_kitti_poses(...))``; NumPy or a tensor).  Each window runs
    through ``eval_pose`` in whatever mode the model is in -- call ``model.testmode()`` first, so that
    BatchNorm uses its running statistics and a pair's pose does not depend on its window -- the
    outputs are concatenated on the device and scored by ``pose_errors(..., invert=True)``; the host
    syncs once at the end.

    Returns a dict: ``ate_mean``, ``ate_std`` (over the finite snippets), ``rot_deg_mean`` (the
    mean rotation chord as an angle, degrees), ``scale_mean``, ``snippets``, ``n_bad`` (snippets
    with a non-finite value) and ``nonfinite_inputs`` (elements of the frames that are NaN or
    infinite: checked because the network's ReLUs turn a NaN into 0).  ``n_bad > 0`` or
    ``nonfinite_inputs > 0`` raises ``RuntimeError`` unless ``allow_nonfinite``."""
    import torch
    from .model import eval_pose
    poses, bad_in = [], None
    for x in frames:
        nf = (~torch.isfinite(x)).sum()                     # stays on the device
        bad_in = nf if bad_in is None else bad_in + nf
        poses.append(eval_pose(model, x))
    if not poses:
        raise ValueError("evaluate_pose: no frames")
    pred = torch.cat(poses)
    gt = torch.as_tensor(gt_rel).to(device=pred.device, dtype=torch.float32).contiguous()
    if tuple(gt.shape) != (pred.shape[0], 12):
        raise ValueError(f"gt_rel must be [{pred.shape[0]}, 12] for the {pred.shape[0]} pairs of the windows, "
                         f"got {list(gt.shape)}")
    _, summary, counts = pose_errors(pred, gt, track_length=track_length, invert=True)
    s = summary.cpu().numpy().astype(np.float64)[0]         # the one sync
    c = counts.cpu().numpy()[0]
    bad_in = int(bad_in.cpu())
    n_bad = int(c[1])
    if (n_bad or bad_in) and not allow_nonfinite:
        raise RuntimeError(f"evaluate_pose: {n_bad} snippets have a non-finite error, {bad_in} input elements "
                           "are not finite (pass allow_nonfinite=True to score regardless)")
    return {"ate_mean": float(s[0]), "ate_std": float(s[1]), "rot_deg_mean": float(chord_to_degrees(s[3])),
            "scale_mean": float(s[2]), "snippets": int(c[0]), "n_bad": n_bad, "nonfinite_inputs": bad_in}


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
