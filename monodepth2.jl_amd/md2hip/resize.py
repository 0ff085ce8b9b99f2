"""Frame resize on the device over the C-ABI (``md2_resize_frames``; include/md2.h states every
operation of both filters), and the decode -> upload -> resize route built on it.  No CPU fallback.

``resize_frames`` takes decoded images as they come out of a PNG decoder -- rows of interleaved
pixels, every image of its own size, packed at any byte offsets into one device buffer -- and
writes ``[n][C][H][W]`` float planes.  ``filter="imresize"`` with ``quantize=True`` gives the bytes
of the host path (``md2hip.data.imresize``, ``md2_load_kitti_u8``) followed by ``u / 255f``;
``filter="antialias"`` is the triangle filter widened by the reduction factor (Pillow's BILINEAR,
torch's ``interpolate(antialias=True)``).  ``load_frames`` is the loader for evaluation and
inference callers: files in, a resized batch on the device out."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import RESIZE_FILTERS, RESIZE_MAX_IMAGES, ResizeCfg, check, lib, ptr, stream_of

MAX_SIDE = 8192
MAX_REDUCTION = 16


def _filter_id(filter):
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
    return RESIZE_FILTERS[filter]


def resize_frames(src, offsets, sizes, height, width, *, channels, filter="imresize", quantize=True, flips=None,
                  out=None, return_u8=False):
    """``n`` decoded images resized to ``[n, channels, height, width]`` float32 on ``src``'s device.

    ``src`` is a 1-D contiguous uint8 CUDA tensor; image ``i`` is the ``sizes[i] = (h_i, w_i)``
    rows of interleaved ``channels``-byte pixels that start at byte ``offsets[i]`` (any offset;
    ``offsets`` and ``sizes`` are host sequences).  ``filter`` is ``"imresize"`` (bilinear, no
    antialiasing: the host path's bytes) or ``"antialias"``.  ``quantize`` rounds the result to
    N0f8, the element type imresize keeps, and returns ``q / 255f``; without it the fp64 result is
    rounded to float32 once.  ``flips`` (host, one truth value per image) mirrors an image left-right
    after the resize.  ``out`` may be a contiguous float32 tensor of the result's shape.
    ``return_u8`` (needs ``quantize``) adds the bytes ``q`` as a uint8 tensor of the same shape.
    A source side may be at most 16 times the target's.  Bitwise reproducible; enqueues on the
    current stream and does not synchronise.  More than 64 images go through in chunks of 64."""
    import torch
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.device.type != "cuda" \
            or src.dim() != 1 or not src.is_contiguous():
        raise ValueError("src must be a contiguous 1-D uint8 CUDA tensor")
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, got {channels!r}")
    fid = _filter_id(filter)
    H, W, c = int(height), int(width), int(channels)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"height and width must be in 1..{MAX_SIDE}")
    offsets = np.asarray(offsets)
    sizes = np.asarray(sizes)
    if offsets.ndim != 1 or offsets.size == 0 or offsets.dtype.kind not in "iu":
        raise ValueError("offsets must be a non-empty 1-D integer sequence")
    n = int(offsets.size)
    if sizes.shape != (n, 2) or sizes.dtype.kind not in "iu":
        raise ValueError(f"sizes must be {n} integer pairs (height, width)")
    offsets = offsets.astype(np.int64)
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    ws = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    if (hs < 1).any() or (ws < 1).any() or (hs > MAX_SIDE).any() or (ws > MAX_SIDE).any():
        raise ValueError(f"source sizes must be in 1..{MAX_SIDE}")
    if (hs > MAX_REDUCTION * H).any() or (ws > MAX_REDUCTION * W).any():
        raise ValueError(f"a source side may be at most {MAX_REDUCTION} times the target's")
    if (offsets < 0).any() or (offsets + hs.astype(np.int64) * ws * c > src.numel()).any():
        raise ValueError("every image must lie within src")
    if flips is None:
        fl = None
    else:
        fl = np.ascontiguousarray(np.asarray(flips).astype(bool), dtype=np.uint8)
        if fl.shape != (n,):
            raise ValueError(f"flips must hold one value per image ({n})")
    if return_u8 and not quantize:
        raise ValueError("return_u8 needs quantize")
    dev = src.device
    if out is None:
        out = torch.empty(n, c, H, W, dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev \
            or tuple(out.shape) != (n, c, H, W) or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError(f"out must be a contiguous, 16-byte aligned float32 tensor [{n}, {c}, {H}, {W}] on src's device")
    with torch.cuda.device(dev):
        u8 = torch.empty(n, c, H, W, dtype=torch.uint8, device=dev) if return_u8 else None
        plane = c * H * W
        for a in range(0, n, RESIZE_MAX_IMAGES):
            b = min(n, a + RESIZE_MAX_IMAGES)
            # a chunk starts a multiple of 64 images in: its part of out is 16-byte aligned as out is
            cfg = ResizeCfg(b - a, c, H, W, fid, 1 if quantize else 0)
            check(lib().md2_resize_frames(
                C.byref(cfg), ptr(src), offsets[a:b].ctypes.data_as(C.POINTER(C.c_longlong)),
                ws[a:b].ctypes.data_as(C.POINTER(C.c_int)), hs[a:b].ctypes.data_as(C.POINTER(C.c_int)),
                None if fl is None else fl[a:b].ctypes.data_as(C.c_void_p),
                C.c_void_p(out.data_ptr() + 4 * a * plane),
                None if u8 is None else C.c_void_p(u8.data_ptr() + a * plane), stream_of(dev)), "md2_resize_frames")
    return (out, u8) if return_u8 else out


def decode_frames(paths, *, channels, threads=8, slot_bytes=None, out=None):
    """PNG files decoded at their own sizes by the library's loader (``md2_load_frames_native_u8``)
    on ``threads`` host threads: returns ``(buf, offsets, sizes)`` -- ``buf`` a 1-D uint8 CPU tensor
    (pinned when CUDA is available) with image ``i`` at ``offsets[i] = i * slot_bytes`` as rows of
    interleaved pixels, ``sizes[i] = (h_i, w_i)``.  ``slot_bytes`` defaults to the first file's size
    with 4 % headroom (KITTI's frames differ by about 1.5 %); a file that does not fit is an error."""
    import torch
    paths = [p if isinstance(p, bytes) else str(p).encode() for p in paths]
    n = len(paths)
    if n == 0:
        raise ValueError("paths is empty")
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, got {channels!r}")
    if slot_bytes is None:
        slot_bytes = frame_slot_bytes(paths[0], channels)
    slot_bytes = int(slot_bytes)
    if out is None:
        out = torch.empty(n * slot_bytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    elif out.dtype != torch.uint8 or out.is_cuda or not out.is_contiguous() or out.numel() < n * slot_bytes:
        raise ValueError("out must be a contiguous uint8 CPU tensor of at least n * slot_bytes bytes")
    w = np.zeros(n, dtype=np.int32)
    h = np.zeros(n, dtype=np.int32)
    arr = (C.c_char_p * n)(*paths)
    check(lib().md2_load_frames_native_u8(arr, n, int(channels), C.c_void_p(out.data_ptr()), slot_bytes,
                                          w.ctypes.data_as(C.POINTER(C.c_int)), h.ctypes.data_as(C.POINTER(C.c_int)),
                                          int(threads)), "md2_load_frames_native_u8")
    return out, np.arange(n, dtype=np.int64) * slot_bytes, np.stack([h, w], 1)


def frame_slot_bytes(path, channels):
    """The staging slot for frames like ``path``: its decoded size with 4 % headroom, a multiple of
    16 bytes."""
    w, h, ch = C.c_int(), C.c_int(), C.c_int()
    path = path if isinstance(path, bytes) else str(path).encode()
    check(lib().md2_png_info(path, C.byref(w), C.byref(h), C.byref(ch)), "md2_png_info")
    need = w.value * h.value * int(channels)
    return (need + need // 25 + 15) // 16 * 16


def load_frames(paths, height, width, *, channels, filter="antialias", device=None, threads=8):
    """PNG files -> ``[n, channels, height, width]`` float32 on ``device`` (default: the current
    CUDA device): decoded at their own sizes on ``threads`` host threads, uploaded in one copy and
    resized by ``resize_frames`` with ``quantize=True``.  ``channels=1`` reads gray files, ``3`` RGB
    or RGBA (alpha dropped).  The frames may differ in size as long as each fits the first one's
    size with 4 % headroom."""
    import torch
    _filter_id(filter)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("load_frames resizes on the GPU: device must be a CUDA device")
    host, offsets, sizes = decode_frames(paths, channels=channels, threads=threads)
    src = host.to(dev, non_blocking=True)
    return resize_frames(src, offsets, sizes, height, width, channels=channels, filter=filter, quantize=True)
