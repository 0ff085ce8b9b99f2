"""Colour augmentation on the device (``md2_color_jitter``; include/md2.h states every operation).

Monodepth2 trains with torchvision's ``ColorJitter``: with probability 0.5 a sample's frames get a
random brightness, contrast, saturation and hue change, in random order, identically for every frame
of the sample.  The jittered frames feed the networks only -- pass them as ``x_net`` to
``train_loss`` / ``train_step`` / ``train_step_graph``; the loss, SSIM and the automask stay on x.

The per-sample numbers are drawn on the host (``ColorJitter.draw``) from a stream of their own,
``default_rng((seed, i, 1))``, so the FlipX coins of ``default_rng((seed, i))`` do not move."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import JITTER_MAX_SAMPLES, Jitter, check, lib, ptr, stream_of

# md2_jitter as a NumPy record: what ``draw`` returns and ``color_jitter`` takes
JITTER_DTYPE = np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue", "<f4"),
                         ("order", "u1", (4,)), ("apply", "<i4")])
assert JITTER_DTYPE.itemsize == C.sizeof(Jitter)

_workspaces = {}


def jitter_params(n: int) -> np.ndarray:
    """``n`` identity records (factors 1, hue 0, order 0123, apply 0) to fill in."""
    p = np.zeros(n, dtype=JITTER_DTYPE)
    p["brightness"] = p["contrast"] = p["saturation"] = 1.0
    p["order"] = np.arange(4, dtype=np.uint8)
    return p


def color_jitter(x, params, out=None, means=None, *, _cache=None):
    """``md2_color_jitter`` on x [n][frames][c][h][w] (float32, contiguous, on the GPU) with
    ``params`` (``JITTER_DTYPE`` records, one per sample).  ``out`` may be x (in place); ``means``
    [n][frames] receives each frame's contrast mean.  Enqueued on the current stream, no host
    synchronisation; batches above MD2_JITTER_MAX_SAMPLES go in chunks.  Returns ``out``."""
    import torch
    if x.dim() != 5 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be a contiguous float32 CUDA tensor [n][frames][c][h][w]")
    n, frames, c, h, w = x.shape
    params = np.ascontiguousarray(params, dtype=JITTER_DTYPE)
    if params.shape != (n,):
        raise ValueError(f"params must hold {n} records")
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != tuple(x.shape) or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor like x")
    if means is not None and (tuple(means.shape) != (n, frames) or means.dtype != torch.float32
                              or means.device != x.device or not means.is_contiguous()):
        raise ValueError("means must be a contiguous float32 tensor [n][frames] on x's device")
    st = stream_of(x.device)
    cache = _workspaces if _cache is None else _cache
    for a in range(0, n, JITTER_MAX_SAMPLES):
        b = min(n, a + JITTER_MAX_SAMPLES)
        key = (x.device, st.value, b - a, frames, h, w)
        ws = cache.get(key)
        if ws is None:
            size = lib().md2_color_jitter_workspace_size(b - a, frames, h, w)
            if size == 0:
                raise ValueError("color_jitter: sizes out of range (h * w <= 2^24, frames <= 65535)")
            ws = cache[key] = torch.empty(size // 8, dtype=torch.float64, device=x.device)
        check(lib().md2_color_jitter(ptr(x[a:b]), b - a, frames, c, h, w,
                                     C.cast(C.c_void_p(params[a:b].ctypes.data), C.POINTER(Jitter)), ptr(out[a:b]),
                                     None if means is None else ptr(means[a:b]), ptr(ws), st), "md2_color_jitter")
    return out


class ColorJitter:
    """``ColorJitter(brightness, contrast, saturation, hue, p)``: the ranges the factors are drawn
    from (Monodepth2's defaults) and the probability that a sample is changed at all."""

    def __init__(self, brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-0.1, 0.1),
                 p: float = 0.5):
        for name, (lo, hi) in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
            if not 0.0 <= lo <= hi:
                raise ValueError(f"{name} range must satisfy 0 <= lo <= hi")
        if not -0.5 <= hue[0] <= hue[1] <= 0.5:
            raise ValueError("hue range must lie in [-0.5, 0.5]")
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must be a probability")
        self.brightness, self.contrast, self.saturation, self.hue = (tuple(map(float, r)) for r in
                                                                     (brightness, contrast, saturation, hue))
        self.p = float(p)
        self._ws = {}                      # workspaces by (device, stream, sizes)

    def draw(self, indices, seed: int) -> np.ndarray:
        """The ``md2_jitter`` records of samples ``indices``: per sample, from
        ``default_rng((seed, i, 1))``, a coin, the four factors (uniform in their ranges) and the
        order (a permutation) -- all drawn whatever the coin shows."""
        out = jitter_params(len(indices))
        for k, i in enumerate(indices):
            rng = np.random.default_rng((int(seed), int(i), 1))
            out["apply"][k] = rng.random() < self.p
            for name in ("brightness", "contrast", "saturation", "hue"):
                lo, hi = getattr(self, name)
                # the float32 rounding of a draw can leave the range by an ulp: clip in float32
                out[name][k] = np.clip(np.float32(rng.uniform(lo, hi)), np.float32(lo), np.float32(hi))
            out["order"][k] = rng.permutation(4)
        return out

    def __call__(self, x, params, out=None, means=None):
        return color_jitter(x, params, out, means, _cache=self._ws)
