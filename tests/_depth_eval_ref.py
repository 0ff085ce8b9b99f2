"""NumPy reference of md2_depth_eval (include/md2.h, steps 1-7) for the depth-evaluation tests.

``reference`` evaluates the formulas in fp64 on the fp32 inputs; with ``dtype=np.float32`` the same
formulas run in float32 (``fp32_floor`` uses that, in two summation orders, to measure how far a
float32 evaluation may sit from fp64).  Also the tests' input construction (``make_case``)."""
import numpy as np

NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "ratio", "med_gt", "med_pred")
CONTINUOUS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "ratio", "med_pred")
THRESH = (1.25, 1.5625, 1.953125)
BORDER_REL = 1e-5


def garg(H, W):
    return (int(0.40810811 * H), int(0.99189189 * H), int(0.03594771 * W), int(0.96405229 * W))


def _axis(n_out, n_in):
    """Half-pixel-centre source coordinates (fp64): lower neighbour, upper neighbour, weight."""
    s = np.clip((np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5, 0.0, n_in - 1.0)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0


def pred_depth(disp, Hg, Wg, min_depth=0.1, max_depth=100.0, dtype=np.float64):
    """Steps 1-2 for one image [h][w] -> pred [Hg][Wg] in ``dtype``."""
    h, w = disp.shape
    a = dtype(1.0 / np.float64(np.float32(min_depth)) - 1.0 / np.float64(np.float32(max_depth)))
    b = dtype(1.0 / np.float64(np.float32(max_depth)))
    with np.errstate(all="ignore"):
        sd = disp.astype(dtype) * a + b
        if (h, w) != (Hg, Wg):
            y0, y1, fy = _axis(Hg, h)
            x0, x1, fx = _axis(Wg, w)
            fy, fx = fy.astype(dtype)[:, None], fx.astype(dtype)[None, :]
            top = sd[y0][:, x0] * (1 - fx) + sd[y0][:, x1] * fx
            bot = sd[y1][:, x0] * (1 - fx) + sd[y1][:, x1] * fx
            sd = top * (1 - fy) + bot * fy
        return (dtype(1.0) / sd).astype(dtype)


def _sum(v, order):
    """Sum of a 1-D array in its own dtype: NumPy's pairwise sum, or strictly sequential."""
    if order == "pairwise":
        return v.sum(dtype=v.dtype)
    return np.cumsum(v, dtype=v.dtype)[-1] if len(v) else v.dtype.type(0)


def reference(disp, gt, crop, *, min_depth=0.1, max_depth=100.0, eval_min=1e-3, eval_max=80.0,
              median_scaling=True, scale=1.0, dtype=np.float64, order="pairwise"):
    """One image.  Returns a dict: the ten metrics by name, ``count``, ``n_bad``, ``a_counts``
    (pixels under each threshold) and ``borderline`` (pixels whose max(g/p, p/g) lies within
    relative 1e-5 of 1.25^k: they may fall either side in fp32)."""
    Hg, Wg = gt.shape
    y0, y1, x0, x1 = crop if crop is not None else (0, Hg, 0, Wg)
    emin, emax = np.float32(eval_min), np.float32(eval_max)     # the cfg fields are floats
    pred = pred_depth(disp, Hg, Wg, min_depth, max_depth, dtype)
    with np.errstate(all="ignore"):
        mask = (gt > emin) & (gt < emax)
        box = np.zeros_like(mask)
        box[y0:y1, x0:x1] = True
        mask &= box
        good = np.isfinite(pred) & (pred > 0)
    n_bad = int((mask & ~good).sum())
    mask &= good
    count = int(mask.sum())
    out = {"count": count, "n_bad": n_bad}
    if count == 0:
        out.update({k: float("nan") for k in NAMES})
        out["a_counts"], out["borderline"] = [0, 0, 0], [0, 0, 0]
        return out
    g, p0 = gt[mask].astype(dtype), pred[mask]
    med_g, med_p = np.median(g), np.median(p0)                  # exact; dtype's own for float32
    ratio = med_g / med_p if median_scaling else dtype(np.float32(scale))
    p = np.clip(p0 * ratio, dtype(emin), dtype(emax))
    d = g - p
    n = dtype(count)
    dl = np.log(g) - np.log(p)
    t = np.maximum(g / p, p / g)
    out["abs_rel"] = _sum(np.abs(d) / g, order) / n
    out["sq_rel"] = _sum(d * d / g, order) / n
    out["rmse"] = np.sqrt(_sum(d * d, order) / n)
    out["rmse_log"] = np.sqrt(_sum(dl * dl, order) / n)
    out["a_counts"] = [int((t < dtype(c)).sum()) for c in THRESH]
    for k in range(3):
        out[f"a{k + 1}"] = out["a_counts"][k] / count
    out["borderline"] = [int((np.abs(t.astype(np.float64) / c - 1.0) <= BORDER_REL).sum()) for c in THRESH]
    out["ratio"], out["med_gt"], out["med_pred"] = ratio, med_g, med_p
    for k in NAMES:
        out[k] = float(out[k])
    return out


def fp32_floor(disp, gt, crop, **kw):
    """Per continuous output: the largest relative deviation from the fp64 reference of the same
    formulas evaluated in float32 NumPy, over two summation orders."""
    r64 = reference(disp, gt, crop, **kw)
    floor = {k: 0.0 for k in CONTINUOUS}
    if r64["count"] == 0:
        return floor
    for order in ("pairwise", "sequential"):
        r32 = reference(disp, gt, crop, dtype=np.float32, order=order, **kw)
        for k in CONTINUOUS:
            if r64[k] != 0.0:
                floor[k] = max(floor[k], abs(r32[k] - r64[k]) / abs(r64[k]))
    return floor


def make_case(seed, N, h, w, Hg, Wg, zero_frac=0.3):
    """The tests' base inputs: disp ~ U(0.02, 0.9); gt = pred_resized * 30 * exp(0.25 * N(0, 1))
    rounded to fp32, ``zero_frac`` of the pixels zeroed (no measurement)."""
    rng = np.random.default_rng(seed)
    disp = rng.uniform(0.02, 0.9, size=(N, h, w)).astype(np.float32)
    gt = np.empty((N, Hg, Wg), np.float32)
    for i in range(N):
        pred = pred_depth(disp[i], Hg, Wg)
        gt[i] = (pred * 30.0 * np.exp(0.25 * rng.standard_normal((Hg, Wg)))).astype(np.float32)
    gt[rng.uniform(size=gt.shape) < zero_frac] = 0.0
    return disp, gt
