"""NumPy restatement of the gradient guard as include/md2.h states it (md2_grad_norm,
md2_adam_guarded): the sum of squares in float64 in the header's exact order -- the element-to-thread
map as reshapes, the wave butterfly written out --, the finish (norm, coef, gscale) in float32, and the
guarded ADAM update in float32.  ``sumsq_plain`` is the plain answer, math.fsum of the squares."""
import math

import numpy as np

THREADS = 256
MAX_BLOCKS = 1024
STATE_DTYPE = np.dtype([("sumsq", "<f8"), ("nonfinite", "<i8"), ("skipped", "<i8"), ("norm", "<f4"),
                        ("coef", "<f4"), ("gscale", "<f4"), ("ok", "<i4")])
assert STATE_DTYPE.itemsize == 40


def blocks(n):
    return min((n + 4095) // 4096, MAX_BLOCKS)


def workspace_bytes(n):
    return 16 * blocks(n) if 1 <= n <= 2 ** 31 else 0


def _block_sum(v):
    """[..., 256] thread values -> [...]: per wave of 64 lanes the butterfly with partner lanes
    ^32, 16, 8, 4, 2, 1 (lane 0 holds the wave's sum), then (w0 + w1) + (w2 + w3)."""
    w = v.reshape(v.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def sumsq_ordered(g):
    """(S, c) of a flat float32 vector in the header's order.  Elements past n and non-finite entries
    enter as +0.0, which leaves a non-negative float64 accumulator unchanged bit for bit."""
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    n = g.size
    B = blocks(n)
    stride = B * THREADS * 4
    J = (n + stride - 1) // stride
    a = np.zeros(J * stride, np.float32)
    a[:n] = g
    a = a.reshape(J, B, THREADS, 4)          # element 4 (256 k + t) + j (1024 B) + e -> [j][k][t][e]
    fin = np.isfinite(a)
    d = np.where(fin, a, np.float32(0)).astype(np.float64)
    sq = d * d                               # exact: 24-bit significands
    acc = np.zeros((B, THREADS), np.float64)
    for j in range(J):
        for e in range(4):
            acc = acc + sq[j, :, :, e]
    part = _block_sum(acc)                                   # [B]
    cnt = (~fin).sum(axis=(0, 2, 3)).astype(np.float64)      # [B], exact integers
    R = (B + THREADS - 1) // THREADS
    pp = np.zeros(R * THREADS, np.float64)
    pp[:B] = part
    pp = pp.reshape(R, THREADS)              # thread t adds partials t, t + 256, ... ascending
    facc = np.zeros(THREADS, np.float64)
    for r in range(R):
        facc = facc + pp[r]
    return np.float64(_block_sum(facc)), int(cnt.sum())


def sumsq_plain(g):
    """The correctly rounded sum of the squares of the finite entries, and the non-finite count."""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    fin = np.isfinite(g)
    d = g[fin].astype(np.float64)
    return math.fsum((d * d).tolist()), int((~fin).sum())


def finish(S, c, grad_scale=1.0, max_norm=math.inf, skipped=0):
    """The state grad_guard_finish writes, as a STATE_DTYPE record."""
    gs = np.float32(grad_scale)
    mx = np.float32(max_norm)
    ok = c == 0
    norm = np.float32(np.sqrt(np.float64(S)) * np.float64(gs))
    with np.errstate(over="ignore"):
        coef = mx / norm if (ok and np.isfinite(mx) and norm > mx) else np.float32(1.0)
        gscale = np.float32(gs * np.float32(coef))
    st = np.zeros((), STATE_DTYPE)
    st["sumsq"], st["nonfinite"], st["skipped"] = S, c, skipped + (0 if ok else 1)
    st["norm"], st["coef"], st["gscale"], st["ok"] = norm, coef, gscale, int(ok)
    return st


def grad_norm(g, grad_scale=1.0, max_norm=math.inf, skipped=0):
    S, c = sumsq_ordered(g)
    return finish(S, c, grad_scale, max_norm, skipped)


def adam(p, g, m, v, lr, b1, b2, eps, step, gscale):
    """md2_adam in float32, every operation rounded on its own, in the kernel's order."""
    f = np.float32
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    lr, b1, b2, eps, gscale = f(lr), f(b1), f(b2), f(eps), f(gscale)
    bc1 = f(1.0 - float(b1) ** step)
    bc2 = f(1.0 - float(b2) ** step)
    gi = g * gscale
    mi = b1 * m + (f(1) - b1) * gi
    vi = b2 * v + (f(1) - b2) * gi * gi
    return p - lr * (mi / bc1) / (np.sqrt(vi / bc2) + eps), mi, vi


def adam_guarded(p, g, m, v, lr, b1, b2, eps, step, state):
    """md2_adam_guarded: nothing moves unless state.ok; otherwise adam with gscale = state.gscale."""
    if not int(state["ok"]):
        return (np.array(p, np.float32, copy=True), np.array(m, np.float32, copy=True),
                np.array(v, np.float32, copy=True))
    return adam(p, g, m, v, lr, b1, b2, eps, step, state["gscale"])
