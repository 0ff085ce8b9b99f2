"""NumPy restatement of md2_pose_eval (include/md2.h): the step transforms, the snippet chain, the
scale-aligned ATE and rotation chord per snippet, and the per-sequence summary in the stated fp64
order.  ``dtype=np.float32`` follows the header operation by operation (every NumPy float32 op
rounds once, as the kernel built without contraction does); ``dtype=np.float64`` is the same
formulas in double precision, the reference the float32 floors are measured against.

sinf / cosf of the device are not bit-comparable with NumPy, so the bit-level GPU tests impose the
device's own step transforms (``rt_out``) on ``pose_eval_ref``; ``so3_compose_ref`` is held to them
by a closeness bound instead."""
import numpy as np

MAX_SEQ, MAX_TRACK = 64, 16


def so3_compose_ref(pose, invert, dtype=np.float64):
    """composeT(so3_exp_map(rvec), tvec, invert) of pose [M, 6] -> [M, 12] (R row-major, t) in
    ``dtype``: R = I + f1 S + f2 S^2, f1 = sin(th) / max(th, 1e-4), f2 = (1 - cos th) / max(th, 1e-4)^2."""
    p = np.asarray(pose).astype(dtype)
    r, t = p[:, :3], p[:, 3:]
    M = p.shape[0]
    S = np.zeros((M, 3, 3), dtype)
    S[:, 0, 1], S[:, 0, 2] = -r[:, 2], r[:, 1]
    S[:, 1, 0], S[:, 1, 2] = r[:, 2], -r[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -r[:, 1], r[:, 0]
    S2 = S @ S
    th = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
    thi = dtype(1) / np.maximum(th, dtype(1e-4))
    f1 = thi * np.sin(th)
    f2 = thi * thi * (dtype(1) - np.cos(th))
    R = f1[:, None, None] * S + f2[:, None, None] * S2 + np.eye(3, dtype=dtype)
    if invert:
        R = np.transpose(R, (0, 2, 1))
        t = -np.einsum("kij,kj->ki", R, t)
    return np.concatenate([R.reshape(M, 9), t], axis=1).astype(dtype)


def _compose(R, t, D):
    """(R, t) o (R', t') row by row, entries rounded in the header's order."""
    Rn, tn = np.empty_like(R), np.empty_like(t)
    for i in range(3):
        for j in range(3):
            Rn[:, 3 * i + j] = (R[:, 3 * i] * D[:, j] + R[:, 3 * i + 1] * D[:, 3 + j]) + R[:, 3 * i + 2] * D[:, 6 + j]
        tn[:, i] = ((R[:, 3 * i] * D[:, 9] + R[:, 3 * i + 1] * D[:, 10]) + R[:, 3 * i + 2] * D[:, 11]) + t[:, i]
    return Rn, tn


def _chain(rt, S, L, dtype):
    """Positions [L, S, 3] and final rotations [S, 9] of the S snippets of one sequence's steps rt."""
    R = np.tile(np.eye(3, dtype=dtype).reshape(1, 9), (S, 1))
    t = np.zeros((S, 3), dtype)
    pos = [t]
    for j in range(1, L):
        R, t = _compose(R, t, rt[j - 1:j - 1 + S])
        pos.append(t)
    return np.stack(pos), R


def snippets_ref(rt_pred, rt_gt, L, dtype=np.float32):
    """out [S, 3] = (ate, scale, rot_chord) of ONE sequence's step transforms [m, 12]."""
    m = rt_pred.shape[0]
    S = max(m - L + 2, 0)
    if S == 0:
        return np.zeros((0, 3), dtype)
    p, Rp = _chain(np.asarray(rt_pred).astype(dtype), S, L, dtype)
    q, Rq = _chain(np.asarray(rt_gt).astype(dtype), S, L, dtype)
    with np.errstate(all="ignore"):
        num, den = np.zeros(S, dtype), np.zeros(S, dtype)
        for j in range(1, L):
            for c in range(3):
                num = num + q[j, :, c] * p[j, :, c]
                den = den + p[j, :, c] * p[j, :, c]
        scale = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0)).astype(dtype)
        res = np.zeros(S, dtype)
        for j in range(1, L):
            for c in range(3):
                e = p[j, :, c] * scale - q[j, :, c]
                res = res + e * e
        chord = np.zeros(S, dtype)
        for k in range(9):
            d = Rp[:, k] - Rq[:, k]
            chord = chord + d * d
        ate = np.sqrt(res) / dtype(L)
        return np.stack([ate, scale, np.sqrt(chord)], axis=1).astype(dtype)


def _block_sum(v):
    """The header's order for one value per snippet (float64 [n], skipped snippets already 0):
    thread t adds snippets t, t + 256, ... ascending; wave butterfly; (w0 + w1) + (w2 + w3)."""
    n = v.shape[0]
    pad = np.zeros((n + 255) // 256 * 256 if n else 256, np.float64)
    pad[:n] = v
    acc = np.zeros(256, np.float64)
    for row in pad.reshape(-1, 256):
        acc = acc + row
    w = acc.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def summary_ref(out):
    """(summary [4] float32, counts [2] int32) of one sequence's per-snippet values [n, 3]."""
    o = np.asarray(out)
    ok = np.isfinite(o).all(axis=1) if o.shape[0] else np.zeros(0, bool)
    cnt = int(ok.sum())
    counts = np.array([o.shape[0], o.shape[0] - cnt], np.int32)
    if cnt == 0:
        return np.full(4, np.nan, np.float32), counts
    v = np.where(ok[:, None], o, 0).astype(np.float64)
    sums = [_block_sum(v[:, k]) for k in range(3)]
    mean = sums[0] / cnt
    dev = np.where(ok, v[:, 0] - mean, 0.0)
    std = np.sqrt(_block_sum(dev * dev) / cnt)
    return np.array([mean, std, sums[1] / cnt, sums[2] / cnt]).astype(np.float32), counts


def pose_eval_ref(rt_pred, gt_rel, offsets, L, dtype=np.float32):
    """(out [S_total, 3], summary [nseq, 4] float32, counts [nseq, 2] int32) from step transforms."""
    offsets = np.asarray(offsets, np.int64)
    outs, sums, cnts = [], [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        o = snippets_ref(rt_pred[a:b], gt_rel[a:b], L, dtype)
        s, c = summary_ref(o)
        outs.append(o)
        sums.append(s)
        cnts.append(c)
    return np.concatenate(outs) if outs else np.zeros((0, 3), dtype), np.stack(sums), np.stack(cnts)


def make_case(seed, M, *, invert, scale=None, noise_t=0.02, noise_r=0.002):
    """Random steps: ground truth with translations of 0.3 - 1.5 m and rotations up to 0.1 rad;
    the prediction is the ground truth times a random scale plus noise, expressed in the convention
    ``invert`` undoes.  Returns (pred [M, 6] float32, gt_rel [M, 12] float32)."""
    rng = np.random.default_rng(seed)

    def unit(n):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    rvec = unit(M) * rng.uniform(0.0, 0.1, (M, 1))
    tvec = unit(M) * rng.uniform(0.3, 1.5, (M, 1))
    gt = so3_compose_ref(np.concatenate([rvec, tvec], 1), False)
    s = rng.uniform(0.2, 5.0) if scale is None else scale
    want_r = rvec + rng.normal(size=(M, 3)) * noise_r
    want_t = s * tvec + rng.normal(size=(M, 3)) * noise_t
    if invert:   # the raw output whose inverse is (exp(want_r), want_t): (exp(-want_r), -exp(-want_r) want_t)
        Rinv = so3_compose_ref(np.concatenate([-want_r, np.zeros((M, 3))], 1), False)[:, :9].reshape(M, 3, 3)
        pred = np.concatenate([-want_r, -np.einsum("kij,kj->ki", Rinv, want_t)], 1)
    else:
        pred = np.concatenate([want_r, want_t], 1)
    return pred.astype(np.float32), gt.astype(np.float32)
