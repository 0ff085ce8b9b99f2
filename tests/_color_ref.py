"""NumPy restatement of md2_color_jitter (include/md2.h), operation by operation, in ``dtype``.

In float32 every product, sum and quotient is rounded on its own, as the kernel's (built without
contraction, divisions correctly rounded), so with the kernel's own frame means imposed (``means``)
the float32 restatement and the kernel agree bit for bit.  Without ``means`` the frame mean is
(dtype)(S / (h*w)) with S NumPy's float64 sum of the gray values (another order than the kernel's:
equal within one rounding of the float64 sum)."""
import itertools

import numpy as np

ORDERS = [tuple(p) for p in itertools.permutations(range(4))]      # all 24


def params(n):
    """``n`` identity md2_jitter records (md2hip.JITTER_DTYPE's layout, restated: no md2hip import)."""
    dt = np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue", "<f4"),
                   ("order", "u1", (4,)), ("apply", "<i4")])
    p = np.zeros(n, dtype=dt)
    p["brightness"] = p["contrast"] = p["saturation"] = 1.0
    p["order"] = np.arange(4, dtype=np.uint8)
    return p


def _clamp(v, T):
    return np.minimum(np.maximum(v, T(0)), T(1))


def _blend(a, b, t, T):
    return _clamp(t * a + (T(1) - t) * b, T)


def gray(v, T):
    if v.shape[0] == 1:
        return v[0]
    return (T(0.2989) * v[0] + T(0.587) * v[1]) + T(0.114) * v[2]


def _hue(v, hue, T):
    r, g, b = v[0], v[1], v[2]
    mx = np.maximum(np.maximum(r, g), b)
    mn = np.minimum(np.minimum(r, g), b)
    eq = mx == mn
    cr = mx - mn
    one = np.ones_like(mx)
    s = cr / np.where(eq, one, mx)
    d = np.where(eq, one, cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    hh = np.where(mx == r, bc - gc, np.where(mx == g, (T(2) + rc) - bc, (T(4) + gc) - rc))
    t = hh / T(6) + T(1)
    hh = t - np.floor(t)
    t = hh + hue
    hh = t - np.floor(t)
    h6 = hh * T(6)
    fi = np.floor(h6)
    f = h6 - fi
    i = fi.astype(np.int64) % 6
    p = _clamp(mx * (T(1) - s), T)
    q = _clamp(mx * (T(1) - s * f), T)
    tt = _clamp(mx * (T(1) - s * (T(1) - f)), T)
    table = [(mx, tt, p), (q, mx, p), (p, mx, tt), (p, q, mx), (tt, p, mx), (mx, p, q)]
    return np.stack([np.select([i == k for k in range(6)], [table[k][ch] for k in range(6)]) for ch in range(3)])


def jitter_frame(v, p, T, mean=None):
    """One frame v [c][h][w] (dtype T) under record p -> (frame, mean used by contrast, the float64
    mean of the gray values contrast saw, before its rounding to T)."""
    c = v.shape[0]
    used, exact = T(0), 0.0
    for op in p["order"]:
        if op == 0:
            v = _clamp(T(p["brightness"]) * v, T)
        elif op == 1:
            exact = np.sum(gray(v, T).astype(np.float64)) / float(v.shape[1] * v.shape[2])
            used = T(exact) if mean is None else T(mean)
            v = _blend(v, used, T(p["contrast"]), T)
        elif op == 2:
            if c == 3:
                v = _blend(v, gray(v, T)[None], T(p["saturation"]), T)
        elif c == 3:
            v = _hue(v, T(p["hue"]), T)
    return v, used, exact


def color_jitter(x, prm, dtype=np.float32, means=None, exact=False):
    """x [n][frames][c][h][w] -> (out, means [n][frames]) in ``dtype``; ``means``: imposed frame means.
    ``exact``: also the float64 means [n][frames] of the gray values contrast saw (0 where not applied)."""
    T = np.dtype(dtype).type
    x = np.asarray(x)
    out = x.astype(dtype).copy()
    got = np.zeros(x.shape[:2], dtype=dtype)
    ex = np.zeros(x.shape[:2], dtype=np.float64)
    for i in range(x.shape[0]):
        if not prm[i]["apply"]:
            continue
        for f in range(x.shape[1]):
            out[i, f], got[i, f], ex[i, f] = jitter_frame(out[i, f], prm[i], T,
                                                          None if means is None else means[i, f])
    return (out, got, ex) if exact else (out, got)


def test_images(n, frames, c, h, w, seed=0):
    """N0f8 / 255 images with rows of exact 0, exact 1 and grey (r == g == b) where they fit."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 256, (n, frames, c, h, w)).astype(np.float32) / np.float32(255.0))
    if h >= 4:
        x[..., 0, :] = 0.0
        x[..., 1, :] = 1.0
        x[..., 2, :] = x[:, :, :1, 2, :]          # grey: every channel the first one's value
    return np.ascontiguousarray(x)


test_images.__test__ = False
