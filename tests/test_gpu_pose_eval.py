"""GPU: md2_pose_eval (snippet trajectories, scale-aligned ATE, rotation chord, per-sequence summary)
against the NumPy restatement of include/md2.h (tests/_pose_ref.py).

Bit level: the per-snippet output and the counts equal the float32 restatement with the device's own
step transforms (``rt_out``) imposed -- sinf / cosf are not bit-comparable with NumPy, everything
after them is.  The step transforms themselves are held to the float64 formula within
max(1e-6, 4 x the float32 NumPy floor on the same inputs); the summary means to 2^-22 of the fp64
mean of the device's own values, its deviation to 4 x the float32 floor of np.std.  Each test prints
what it measured (first MI355X run: step transforms 4.9e-8 against a float32 floor of 2.35e-7, so the
bound is 1e-6; std_ate 4.3e-8 against a floor of 4.75e-8, bound 1.9e-7; scaled prediction: scale off by
6.0e-8, ate 1.5e-7 m; known rotation: chord off by 8.7e-8)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _pose_ref as R

pytestmark = pytest.mark.gpu


def _run(pred, gt, offsets=None, L=5, invert=True):
    """(out, summary, counts, rt) as NumPy, through md2hip.pose_errors."""
    import md2hip
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    rt = torch.empty(pred.shape[0], 12, dtype=torch.float32, device="cuda")
    o, s, c = md2hip.pose_errors(p, g, offsets, track_length=L, invert=invert, rt_out=rt)
    torch.cuda.synchronize()
    return o.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy(), rt.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _lengths_70():
    rng = np.random.default_rng(70)
    n = rng.integers(0, 9, 70)
    n[[0, 63, 64, 69]] = [5, 0, 7, 1]          # around the chunk boundary: full, empty, full, too short
    return n


# name -> (sequence lengths in steps, L)
CASES = {
    "one_snippet_M_eq_L-1": ([4], 5),
    "M_eq_L": ([5], 5),
    "L2": ([9], 2),
    "L16": ([20], 16),
    "L16_one_snippet": ([15], 16),
    "M37_L5": ([37], 5),
    "M600_L5_three_rounds_per_thread": ([600], 5),
    "three_sequences_37_3_0": ([37, 3, 0], 5),
    "70_sequences_chunked": (_lengths_70(), 3),
}


@pytest.mark.parametrize("invert", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_for_bit(name, invert):
    lengths, L = CASES[name]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    M = int(offsets[-1])
    pred, gt = R.make_case(len(name) + 31 * L, M, invert=invert)
    out, summary, counts, rt = _run(pred, gt, offsets, L, invert)
    want_o, want_s, want_c = R.pose_eval_ref(rt, gt, offsets, L)
    snips = np.maximum(np.asarray(lengths) - L + 2, 0)
    assert out.shape == (snips.sum(), 3) and out.shape == want_o.shape
    assert np.isfinite(out).all()
    assert np.array_equal(_bits(out), _bits(want_o)), np.argwhere(_bits(out) != _bits(want_o))[:5]
    assert np.array_equal(counts, want_c) and np.array_equal(counts[:, 0], snips) and not counts[:, 1].any()
    # a sequence too short for a snippet: count 0, NaN summary; the others finite
    empty = snips == 0
    assert np.isnan(summary[empty]).all() and np.isfinite(summary[~empty]).all()
    # the stated fp64 order, restated: equal up to the final rounding of sqrt / the division
    assert np.allclose(summary[~empty], want_s[~empty], rtol=2.0 ** -22, atol=0)
    # snippets stop at sequence boundaries: each sequence alone gives its own rows
    if len(lengths) == 3:
        solo, _, _, _ = _run(pred[:37], gt[:37], None, L, invert)
        assert np.array_equal(_bits(solo), _bits(out[:34]))


def _so3_inputs():
    rng = np.random.default_rng(5)

    def with_angle(th):
        v = rng.normal(size=3)
        return v / np.linalg.norm(v) * th
    angles = [0.0, 1e-4 * (1 - 2.0 ** -10), 1e-4 * (1 + 2.0 ** -10), 0.5e-4, 1e-4, 1e-3, 0.1, 1.0,
              np.pi - 1e-3, np.pi - 1e-6, np.pi, 3.0]
    r = np.stack([with_angle(a) for a in angles] + [with_angle(a) for a in rng.uniform(0, 0.1, 52)])
    t = rng.uniform(-1.5, 1.5, r.shape)
    return np.concatenate([r, t], 1).astype(np.float32)


def _so3_err(a, want):
    return float((np.abs(a.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())


@pytest.mark.parametrize("invert", [False, True])
def test_step_transforms_against_float64(invert):
    pose = _so3_inputs()
    th = np.linalg.norm(pose[:, :3].astype(np.float64), axis=1)
    assert th[0] == 0 and th[1] < 1e-4 < th[2] and abs(th[9] - np.pi) < 2e-6      # the inputs reach the branches
    gt = np.zeros((pose.shape[0], 12), np.float32)
    _, _, _, rt = _run(pose, gt, None, 5, invert)
    want = R.so3_compose_ref(pose, invert)
    floor = _so3_err(R.so3_compose_ref(pose, invert, dtype=np.float32), want)
    err = _so3_err(rt, want)
    bound = max(1e-6, 4 * floor)
    print(f"\nstep transforms invert={invert}: err {err:.2e}, float32 floor {floor:.2e}, bound {bound:.2e}")
    assert err <= bound
    # orthonormal rotations, and invert really inverts: D(invert=1) o D(invert=0) = identity
    Rm = rt[:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max() < 1e-6
    _, _, _, other = _run(pose, gt, None, 5, not invert)
    Ro = other[:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(Rm @ Ro - np.eye(3)).max() < 1e-6
    assert np.abs(np.einsum("kij,kj->ki", Rm, other[:, 9:].astype(np.float64)) + rt[:, 9:]).max() < 1e-6


# ---- hand-built cases -------------------------------------------------------------------------------
def _gt_and_steps(seed, M):
    """Ground-truth (rvec, tvec) steps [M, 6] float32 and their transforms."""
    rng = np.random.default_rng(seed)
    steps = np.concatenate([rng.normal(size=(M, 3)) * 0.03, rng.normal(size=(M, 3)) * 0.2 + [0, 0, 0.9]], 1)
    steps = steps.astype(np.float32)
    return steps, R.so3_compose_ref(steps, False).astype(np.float32)


def test_scaled_prediction_gives_scale_and_no_error():
    """Prediction = ground truth x 2.5: scale 0.4 and ate 0 up to rounding.  Bounds: a position is the
    sum of <= L-1 = 4 rotated steps, each entry with <= 4 roundings (3 products summed, + t), so a
    component of p or q carries <= 16 x 2^-24 of the largest position, eps; scale = num / den then
    carries <= ~4 eps relative, and ate = sqrt(sum over 3 (L-1) components of e^2) / L with
    |e| <= |p scale - q| <= (2 + 4) eps |q|max -> ate <= 6 eps |q|max sqrt(3 (L-1)) / L."""
    L, M = 5, 12
    steps, gt = _gt_and_steps(3, M)
    pred = steps.copy()
    pred[:, 3:] *= np.float32(2.5)                              # exact in fp32 for most, 1 rounding else
    out, summary, counts, rt = _run(pred, gt, None, L, False)
    qmax = (L - 1) * np.abs(gt[:, 9:]).max() * np.sqrt(3)
    eps = 16 * 2.0 ** -24
    print(f"\nscaled: scale err {np.abs(out[:, 1] - 0.4).max():.2e}, ate max {out[:, 0].max():.2e}, "
          f"rot_chord max {out[:, 2].max():.2e}")
    assert np.abs(out[:, 1] - 0.4).max() <= 0.4 * 6 * eps
    assert out[:, 0].max() <= 6 * eps * qmax * np.sqrt(3 * (L - 1)) / L
    assert out[:, 2].max() <= 9 * eps                           # the same rotations, up to the last bit
    assert counts.tolist() == [[M - L + 2, 0]]


def test_motionless_prediction_is_finite():
    L, M = 5, 9
    _, gt = _gt_and_steps(4, M)
    pred = np.zeros((M, 6), np.float32)
    out, summary, counts, rt = _run(pred, gt, None, L, True)
    want_o, want_s, want_c = R.pose_eval_ref(rt, gt, [0, M], L)
    assert np.array_equal(rt[:, :9], np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (M, 1)))
    assert not rt[:, 9:].any()
    assert np.array_equal(out[:, 1], np.zeros(M - L + 2, np.float32))          # den = 0 -> scale 0
    assert np.isfinite(out).all() and (out[:, 0] > 0.5).all()                  # the zero trajectory's ATE
    assert np.array_equal(_bits(out), _bits(want_o))
    assert counts.tolist() == [[M - L + 2, 0]] and np.isfinite(summary).all()


def test_known_rotation_error():
    """All rotations about z; the last step of the prediction turns phi further: the final rotations
    differ by phi, rot_chord = 2 sqrt(2) sin(phi / 2).  Bound: each rotation entry carries
    <= (L-1) x 3 roundings of values <= 1, the chord sums nine squared differences ->
    |error| <= sqrt(9) x 3 (L-1) 2^-24 absolute, twice that allowed for the two chains."""
    L, phi = 5, 0.3
    ang = np.array([0.05, -0.02, 0.08, 0.03])
    steps = np.zeros((4, 6))
    steps[:, 2] = ang
    steps[:, 3:] = [[0.1, 0.0, 0.9]] * 4
    gt = R.so3_compose_ref(steps, False).astype(np.float32)
    pred = steps.copy()
    pred[3, 2] += phi
    out, _, counts, _ = _run(pred.astype(np.float32), gt, None, L, False)
    want = 2 * np.sqrt(2) * np.sin(phi / 2)
    print(f"\nrot_chord {out[0, 2]:.8f}, analytic {want:.8f}, diff {abs(out[0, 2] - want):.2e}")
    assert out.shape == (1, 3) and counts.tolist() == [[1, 0]]
    assert abs(out[0, 2] - want) <= 2 * 3 * 3 * (L - 1) * 2.0 ** -24
    assert abs(np.degrees(2 * np.arcsin(out[0, 2] / (2 * np.sqrt(2)))) - np.degrees(phi)) < 1e-3


def test_nan_step_is_counted_and_left_out():
    import md2hip
    L = 5
    offsets = np.array([0, 12, 24])
    pred, gt = R.make_case(9, 24, invert=True)
    pred[6, 4] = np.nan                       # mid-sequence: snippets 3..6 of sequence 0 hold step 6
    pred[23, 0] = np.nan                      # the last step of sequence 1: its last snippet only
    out, summary, counts, rt = _run(pred, gt, offsets, L, True)
    bad = ~np.isfinite(out).all(axis=1)
    assert np.flatnonzero(bad).tolist() == [3, 4, 5, 6, 9 + 8]
    assert counts.tolist() == [[9, L - 1], [9, 1]]
    for s, rows in enumerate((out[:9], out[9:])):
        keep = rows[np.isfinite(rows).all(axis=1)].astype(np.float64)
        want = [keep[:, 0].mean(), keep[:, 0].std(), keep[:, 1].mean(), keep[:, 2].mean()]
        assert np.allclose(summary[s, [0, 2, 3]], np.array(want)[[0, 2, 3]], rtol=2.0 ** -22, atol=0)
    want_o, want_s, want_c = R.pose_eval_ref(rt, gt, offsets, L)
    assert np.array_equal(counts, want_c)
    ok = ~bad
    assert np.array_equal(_bits(out[ok]), _bits(want_o[ok]))
    assert md2hip.chord_to_degrees(summary[0, 3]) > 0


# ---- summary ----------------------------------------------------------------------------------------
def test_summary_against_float64():
    L, M = 5, 600
    pred, gt = R.make_case(21, M, invert=True)
    out, summary, counts, _ = _run(pred, gt, None, L, True)
    o64 = out.astype(np.float64)
    for col, src in ((0, 0), (2, 1), (3, 2)):
        mean = o64[:, src].mean()
        assert abs(summary[0, col] - mean) <= 2.0 ** -22 * abs(mean), (col, summary[0, col], mean)
    std64 = o64[:, 0].std()
    floor = abs(float(np.std(out[:, 0])) - std64) / std64                      # NumPy's float32 evaluation
    err = abs(float(summary[0, 1]) - std64) / std64
    print(f"\nstd_ate {summary[0, 1]:.8e}: err {err:.2e}, float32 floor {floor:.2e}, bound {4 * floor:.2e}")
    assert err <= 4 * floor
    assert counts.tolist() == [[M - L + 2, 0]]


# ---- reproducibility --------------------------------------------------------------------------------
def test_reproducible_and_independent_of_buffer_contents():
    from md2hip._lib import lib, ptr, stream_of
    L = 5
    lengths = [37, 3, 0, 11]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    M, S = int(offsets[-1]), int(np.maximum(np.asarray(lengths) - L + 2, 0).sum())
    pred, gt = R.make_case(17, M, invert=True)
    a = _run(pred, gt, offsets, L, True)
    b = _run(pred, gt, offsets, L, True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # the C entry point on buffers pre-filled with 0xFF, without rt_out: the workspace holds the steps
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    out = torch.full((S, 3), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    summary = torch.full((len(lengths), 4), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    counts = torch.full((len(lengths), 2), -1, dtype=torch.int32, device="cuda")
    ws = torch.full((int(lib().md2_pose_eval_workspace_size(M)),), 0xFF, dtype=torch.uint8, device="cuda")
    off = (C.c_longlong * len(offsets))(*[int(o) for o in offsets])
    rc = lib().md2_pose_eval(ptr(p), ptr(g), off, len(lengths), L, 1, ptr(out), ptr(summary), ptr(counts), None,
                             ptr(ws), stream_of(p.device))
    assert rc == 0, lib().md2_last_error()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == a[0].tobytes()
    assert summary.cpu().numpy().tobytes() == a[1].tobytes()
    assert counts.cpu().numpy().tobytes() == a[2].tobytes()
