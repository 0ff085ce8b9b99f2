"""NumPy float64 restatement of md2_resize_frames (include/md2.h), operation for operation: the
per-axis taps and weights by scalar loops, the sums by loops over the taps in the stated order
(each step one elementwise product and one elementwise add over the image: NumPy rounds each on its
own, there is no fused multiply-add, no einsum and no dot).  The device result must equal it bit
for bit."""
import math

import numpy as np

IMRESIZE, ANTIALIAS = "imresize", "antialias"


def imresize_axis(n_in, n_out):
    """Per output index the tap list [(source index, weight), (source index, weight)]."""
    sf = float(n_in) / float(n_out)
    taps = []
    for i in range(n_out):
        p = sf * ((i + 1) - 0.5) + 0.5
        if sf < 1:
            p = min(max(p, 1.0), float(n_in))
        p = p - 1.0
        i0 = min(int(math.floor(p)), n_in - 1)
        f = p - i0
        i1 = min(i0 + 1, n_in - 1)
        taps.append([(i0, 1.0 - f), (i1, f)])
    return taps


def antialias_axis(n_in, n_out):
    """Per output index the tap list [(k, w_k / ww) for k in lo .. hi-1]."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    taps = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int((center - fs) + 0.5), 0)          # int() truncates toward zero
        hi = min(int((center + fs) + 0.5), n_in)
        raw = [max(0.0, 1.0 - abs(((k - center) + 0.5) / fs)) for k in range(lo, hi)]
        ww = 0.0
        for w in raw:
            ww = ww + w
        taps.append([(k, w / ww) for k, w in zip(range(lo, hi), raw)])
    return taps


def axis_taps(filter, n_in, n_out):
    if filter == IMRESIZE:
        return imresize_axis(n_in, n_out)
    if filter == ANTIALIAS:
        return antialias_axis(n_in, n_out)
    raise ValueError(filter)


def resize_value(img, height, width, filter):
    """``img`` uint8 [h][w][c] (interleaved, as decoded) -> r, float64 [c][height][width]."""
    h, w, c = img.shape
    v = img.astype(np.float64) / 255.0
    if (h, w) == (height, width):
        return np.ascontiguousarray(v.transpose(2, 0, 1))
    tx, ty = axis_taps(filter, w, width), axis_taps(filter, h, height)
    # horizontal sums of every source row: H[yy][x][ch], taps ascending, from 0.0
    H = np.zeros((h, width, c), dtype=np.float64)
    for x in range(width):
        s = np.zeros((h, c), dtype=np.float64)
        for k, wk in tx[x]:
            s = s + wk * v[:, k, :]
        H[:, x, :] = s
    out = np.zeros((height, width, c), dtype=np.float64)
    for y in range(height):
        s = np.zeros((width, c), dtype=np.float64)
        for yy, wy in ty[y]:
            s = s + wy * H[yy]
        out[y] = s
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def resize_ref(img, height, width, filter, quantize=True, flip=False):
    """One image as md2_resize_frames writes it: ``(out float32 [c][H][W], out_u8 or None)``."""
    r = resize_value(img, height, width, filter)
    if flip:
        r = r[..., ::-1]
    if quantize:
        q = np.rint(r * 255.0)                          # ties to even
        return (q.astype(np.float32) / np.float32(255.0)), q.astype(np.uint8)
    return r.astype(np.float32), None


def resize_batch_ref(imgs, height, width, filter, quantize=True, flips=None):
    outs = [resize_ref(im, height, width, filter, quantize, bool(flips[i]) if flips is not None else False)
            for i, im in enumerate(imgs)]
    f = np.stack([o[0] for o in outs])
    return f, (np.stack([o[1] for o in outs]) if quantize else None)


def pack(imgs, first=1, gap=1):
    """The images' bytes in one buffer at odd byte offsets: ``(buf uint8, offsets, sizes (h, w))``."""
    offsets, pos = [], first
    for im in imgs:
        offsets.append(pos)
        pos += im.size + gap
        pos += (pos + 1) % 2                            # keep every offset odd
    buf = np.full(pos + 8, 0xA5, dtype=np.uint8)
    for o, im in zip(offsets, imgs):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, np.array(offsets, dtype=np.int64), np.array([im.shape[:2] for im in imgs], dtype=np.int64)


def random_images(seed, sizes, c):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in sizes]
