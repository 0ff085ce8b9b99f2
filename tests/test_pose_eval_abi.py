"""CPU checks of the odometry evaluation entry points (md2_model_eval_pose, md2_pose_eval,
include/md2.h): exports and signatures in the header, the ctypes table and the Julia shim, argument
validation (which comes before any HIP call, so it runs without a GPU), the pose-file helpers, and
the float32 NumPy restatement (tests/_pose_ref.py) against its float64 form.

Floors.  On random trajectories (steps of 0.3 - 1.5 m, rotations up to 0.1 rad, prediction = ground
truth x a random scale + noise of 2 cm / 2 mrad per step) the float32 restatement differs from
float64 by at most 1.95e-5 (ate), 4.1e-7 (scale) and 8.9e-6 (rot_chord) relative -- ate and the chord
are differences of nearly equal quantities (ate >= 2.3 mm of positions ~ 3 m, chord >= 1e-3 of entries
~ 1), so their relative error is the fp32 epsilon amplified by that ratio.  FLOOR below is asserted,
and is what tests/test_gpu_pose_eval.py builds its bounds from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _pose_ref as R
from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _jl_ccalls

MD2_EINVAL = 1
SYMBOLS = {"md2_model_eval_pose": 5, "md2_pose_eval_workspace_size": 1, "md2_pose_eval": 12}
# the largest relative float32-vs-float64 error of (ate, scale, rot_chord) over FLOOR_CASES, rounded up
FLOOR = {"ate": 2.0e-5, "scale": 4.2e-7, "rot_chord": 9.0e-6}
FLOOR_CASES = [(seed, M, L, inv) for seed, (M, L) in enumerate([(37, 5), (600, 5), (40, 2), (60, 16), (5, 5)])
               for inv in (False, True)]


# ---- exports, prototypes, bindings ------------------------------------------------------------------
def test_library_exports_and_header():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    hdr = open(HDR).read()
    protos = _c_prototypes(hdr)
    from md2hip import _lib
    for s, nargs in SYMBOLS.items():
        assert hasattr(lib, s), s
        assert protos.get(s) == nargs, (s, protos.get(s))
        assert len(_lib._SIGS[s][1]) == nargs, s
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2      # additive
    assert int(re.search(r"#define MD2_POSE_EVAL_MAX_SEQ (\d+)", hdr).group(1)) == _lib.POSE_EVAL_MAX_SEQ == R.MAX_SEQ
    assert int(re.search(r"#define MD2_POSE_EVAL_MAX_TRACK (\d+)", hdr).group(1)) == _lib.POSE_EVAL_MAX_TRACK \
        == R.MAX_TRACK
    lib.md2_pose_eval_workspace_size.restype = C.c_size_t
    lib.md2_pose_eval_workspace_size.argtypes = [C.c_longlong]
    assert lib.md2_pose_eval_workspace_size(1590) >= 1590 * 48
    assert lib.md2_pose_eval_workspace_size(0) > 0
    assert lib.md2_pose_eval_workspace_size(-1) == 0 and lib.md2_pose_eval_workspace_size((1 << 24) + 1) == 0


def test_python_api_is_exported():
    import md2hip
    for name in ("eval_pose", "pose_errors", "evaluate_pose", "pose_windows", "chord_to_degrees",
                 "load_kitti_poses", "relative_poses"):
        assert callable(getattr(md2hip, name)), name
    assert "executor" in md2hip.eval_pose.__doc__ and "overwrites" in md2hip.eval_pose.__doc__


def test_julia_ccalls_match_header():
    jl, hdr = open(JL).read(), open(HDR).read()
    protos = _c_prototypes(hdr)
    calls = dict(_jl_ccalls(jl))
    for name in SYMBOLS:
        assert name in calls, f"julia/MD2HIP.jl does not call {name}"
        assert calls[name] == protos[name]
    assert re.search(r"function eval_pose\(m::HIPModel, x::ROCArray\{Float32,4\}\)", jl)
    assert re.search(r"function pose_errors\(pred::ROCArray\{Float32,2\}, gt_rel::ROCArray\{Float32,2\};", jl)
    assert int(re.search(r"const POSE_EVAL_MAX_SEQ = (\d+)", jl).group(1)) == 64


# ---- md2_pose_eval refuses, before any HIP call -----------------------------------------------------
# (a valid call is never made here: it would launch)
@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    lib.md2_pose_eval.restype = C.c_int
    lib.md2_pose_eval.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.md2_model_eval_pose.restype = C.c_int
    lib.md2_model_eval_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.md2_last_error.restype = C.c_char_p
    return lib


INVALID = {
    "L_1": dict(L=1),
    "L_0": dict(L=0),
    "L_17": dict(L=17),
    "L_negative": dict(L=-5),
    "offsets_decrease": dict(offsets=[0, 9, 8]),
    "offsets_decrease_first": dict(offsets=[0, -1, 8]),
    "offset0_not_zero": dict(offsets=[2, 9, 12]),
    "nseq_65": dict(offsets=list(range(66))),
    "nseq_0": dict(offsets=[0], nseq=0),
    "invert_2": dict(invert=2),
    "steps_past_2_24": dict(offsets=[0, (1 << 24) + 1]),
}


def _call(L, *, offsets=(0, 9, 12), nseq=None, L_=5, invert=1, null=None):
    buf = (C.c_char * 256)()
    p = C.c_void_p(C.addressof(buf))                  # never dereferenced: validation comes first
    off = (C.c_longlong * len(offsets))(*offsets)
    a = dict(pred=p, gt_rel=p, out=p, summary=p, counts=p, rt_out=p, workspace=p)
    if null:
        a[null] = None
    return L.md2_pose_eval(a["pred"], a["gt_rel"], None if null == "offsets" else off,
                           len(offsets) - 1 if nseq is None else nseq, L_, invert, a["out"], a["summary"],
                           a["counts"], a["rt_out"], a["workspace"], None)


@pytest.mark.parametrize("name", sorted(INVALID))
def test_pose_eval_invalid_is_einval(L, name):
    kw = dict(INVALID[name])
    if "L" in kw:
        kw["L_"] = kw.pop("L")
    assert _call(L, **kw) == MD2_EINVAL, name
    msg = L.md2_last_error()
    assert msg and b"pose_eval" in msg, msg


@pytest.mark.parametrize("which", ["pred", "gt_rel", "offsets", "out", "summary", "counts", "workspace"])
def test_pose_eval_null_pointer_is_einval(L, which):
    assert _call(L, null=which) == MD2_EINVAL
    assert b"pose_eval" in L.md2_last_error()


def test_eval_pose_null_model_is_einval(L):
    assert L.md2_model_eval_pose(None, None, 3, None, None) == MD2_EINVAL


def _no_lib():
    raise AssertionError("the wrapper reached the library")


def test_pose_errors_rejects_bad_arguments(monkeypatch):
    import torch
    import md2hip
    from md2hip import evaluate
    monkeypatch.setattr(evaluate, "lib", _no_lib)
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.pose_errors(torch.zeros(8, 6), torch.zeros(8, 12))              # CPU tensors
    with pytest.raises(ValueError, match="torch tensors"):
        md2hip.pose_errors(np.zeros((8, 6), np.float32), np.zeros((8, 12), np.float32))
    # the shape / offsets / track_length checks follow the tensor checks: reached with those stubbed out
    monkeypatch.setattr(evaluate, "_check_f32_cuda", lambda t, what: None)
    with pytest.raises(ValueError, match=r"pred must be \[M, 6\]"):
        md2hip.pose_errors(torch.zeros(8, 5), torch.zeros(8, 12))
    with pytest.raises(ValueError, match=r"gt_rel must be \[8, 12\]"):
        md2hip.pose_errors(torch.zeros(8, 6), torch.zeros(7, 12))
    with pytest.raises(ValueError, match="track_length"):
        md2hip.pose_errors(torch.zeros(8, 6), torch.zeros(8, 12), track_length=17)
    with pytest.raises(ValueError, match="offsets must start at 0"):
        md2hip.pose_errors(torch.zeros(8, 6), torch.zeros(8, 12), offsets=[0, 5, 7])
    with pytest.raises(ValueError, match="offsets must start at 0"):
        md2hip.pose_errors(torch.zeros(8, 6), torch.zeros(8, 12), offsets=[0, 5, 4, 8])


def test_pose_windows():
    import torch
    import md2hip
    x = torch.arange(9.0).reshape(9, 1, 1, 1)
    w = md2hip.pose_windows(x, 4)
    assert [t.reshape(-1).tolist() for t in w] == [[0, 1, 2, 3, 4], [4, 5, 6, 7, 8]]
    w = md2hip.pose_windows(x, 3)
    assert [t.reshape(-1).tolist() for t in w] == [[0, 1, 2, 3], [3, 4, 5, 6], [6, 7, 8]]
    assert sum(t.shape[0] - 1 for t in w) == 8
    assert [t.shape[0] for t in md2hip.pose_windows(x[:2], 4)] == [2]
    with pytest.raises(ValueError):
        md2hip.pose_windows(x[:1], 4)
    with pytest.raises(ValueError):
        md2hip.pose_windows(x, 0)


def test_chord_to_degrees():
    import md2hip
    for deg in (0.0, 0.5, 17.0, 90.0, 180.0):
        chord = 2 * np.sqrt(2) * np.sin(np.radians(deg) / 2)
        assert abs(md2hip.chord_to_degrees(chord) - deg) < 1e-6


# ---- host helpers -----------------------------------------------------------------------------------
def _trajectory(rng, F):
    """Global camera-to-world poses [F, 3, 4] of a drive a few hundred metres long."""
    G = [np.eye(4)]
    for _ in range(F - 1):
        d = R.so3_compose_ref(np.concatenate([rng.normal(size=3) * 0.02, [0.05, -0.02, 9.0]])[None], False)[0]
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = d[:9].reshape(3, 3), d[9:]
        G.append(G[-1] @ step)
    return np.stack(G)[:, :3]


def test_load_kitti_poses_and_relative_poses(tmp_path):
    import md2hip
    G = _trajectory(np.random.default_rng(2), 40)
    assert np.abs(G[-1, :, 3]).max() > 300                      # hundreds of metres from the origin
    path = tmp_path / "09.txt"
    path.write_text("".join(" ".join(f"{v:.12e}" for v in g.ravel()) + "\n" for g in G) + "\n")
    got = md2hip.load_kitti_poses(str(path))
    assert got.dtype == np.float64 and got.shape == (40, 3, 4)
    written = np.array([[float(f"{v:.12e}") for v in g.ravel()] for g in G]).reshape(40, 3, 4)
    assert np.array_equal(got, written)
    rel = md2hip.relative_poses(got)
    assert rel.dtype == np.float32 and rel.shape == (39, 12)

    def h(g):
        return np.vstack([g, [0, 0, 0, 1]])
    want = np.stack([(np.linalg.inv(h(got[k])) @ h(got[k + 1]))[:3] for k in range(39)])
    want = np.concatenate([want[:, :, :3].reshape(39, 9), want[:, :, 3]], 1)
    # one float32 rounding of a float64 composition; the two float64 routes (a 4x4 inverse, a
    # transposed rotation applied to the difference) agree to ~1e-13 of |t| ~ 400 m
    assert np.abs(rel - want).max() <= 2.0 ** -23 * 9.5
    assert np.abs(rel[:, 11] - 9.0).max() < 0.01               # the steps, not the global positions
    # fp32 differencing of the global translations would not do: millimetres at this distance
    naive = (got[1:, :, 3].astype(np.float32) - got[:-1, :, 3].astype(np.float32))
    assert np.abs(np.linalg.norm(naive, axis=1) - np.linalg.norm(want[:, 9:], axis=1)).max() > 1e-5
    (tmp_path / "bad.txt").write_text("1 0 0 0 0 1 0 0 0 0 1\n")
    with pytest.raises(ValueError, match="12"):
        md2hip.load_kitti_poses(str(tmp_path / "bad.txt"))
    with pytest.raises(ValueError):
        md2hip.relative_poses(np.zeros((3, 4)))
    assert md2hip.relative_poses(got[:1]).shape == (0, 12)


# ---- the float32 restatement against float64 --------------------------------------------------------
def _floors(seed, M, L, invert):
    pred, gt = R.make_case(seed, M, invert=invert)
    rt = R.so3_compose_ref(pred, invert).astype(np.float32)     # what a device hands the chain: fp32 steps
    o32, s32, c32 = R.pose_eval_ref(rt, gt, [0, M], L)
    o64, s64, c64 = R.pose_eval_ref(rt, gt, [0, M], L, dtype=np.float64)
    assert o32.dtype == np.float32 and o64.dtype == np.float64
    assert o32.shape == (M - L + 2, 3) and np.array_equal(c32, c64) and c32.tolist() == [[M - L + 2, 0]]
    return o32, o64, s32, s64


@pytest.mark.parametrize("seed,M,L,invert", FLOOR_CASES)
def test_restatement_float32_against_float64(seed, M, L, invert):
    o32, o64, s32, s64 = _floors(seed, M, L, invert)
    # the inputs make a relative bound meaningful: no quantity is a rounding residue
    assert o64[:, 0].min() > 2e-3 and o64[:, 2].min() > 9e-4, (o64[:, 0].min(), o64[:, 2].min())
    assert 0.19 < o64[:, 1].min() and o64[:, 1].max() < 5.1
    rel = np.abs(o32.astype(np.float64) - o64) / np.abs(o64)
    worst = dict(zip(("ate", "scale", "rot_chord"), rel.max(axis=0)))
    print(f"M {M} L {L} invert {invert}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= FLOOR[k], (k, v)
    # the summary: fp64 sums of fp32 values, so the means inherit the per-snippet floors
    for col, k in ((0, "ate"), (2, "scale"), (3, "rot_chord")):
        assert abs(float(s32[0, col]) - s64[0, col].astype(np.float64)) <= FLOOR[k] * abs(s64[0, col]) + 1e-12


def test_summary_order_against_numpy():
    """The stated fp64 order against NumPy's own sums, and the n_bad bookkeeping."""
    rng = np.random.default_rng(11)
    o = rng.uniform(0.01, 0.05, (597, 3)).astype(np.float32)
    s, c = R.summary_ref(o)
    o64 = o.astype(np.float64)
    want = [o64[:, 0].mean(), o64[:, 0].std(), o64[:, 1].mean(), o64[:, 2].mean()]
    assert c.tolist() == [597, 0]
    assert np.abs(s.astype(np.float64) - want).max() <= 2.0 ** -23 * 0.05
    o[[3, 300, 596], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    s, c = R.summary_ref(o)
    keep = np.isfinite(o).all(axis=1)
    assert c.tolist() == [597, 3] and keep.sum() == 594
    want = [o64[keep, 0].mean(), o64[keep, 0].std(), o64[keep, 1].mean(), o64[keep, 2].mean()]
    assert np.abs(s.astype(np.float64) - want).max() <= 2.0 ** -23 * 0.05
    s, c = R.summary_ref(np.full((4, 3), np.nan, np.float32))
    assert np.isnan(s).all() and c.tolist() == [4, 4]
    s, c = R.summary_ref(np.zeros((0, 3), np.float32))
    assert np.isnan(s).all() and c.tolist() == [0, 0]


def test_restatement_meets_the_summary_bound_on_the_gpu_test_inputs():
    """tests/test_gpu_pose_eval.py::test_summary_against_float64 holds std_ate to 4 x the float32 floor of
    np.std; here the same bound on the restatement alone: the inputs give it room (a float32 np.std that
    happened to be exact would make 4 x floor an impossible bound for any fp32 result)."""
    L, M = 5, 600
    pred, gt = R.make_case(21, M, invert=True)
    rt = R.so3_compose_ref(pred, True).astype(np.float32)
    out, summary, _ = R.pose_eval_ref(rt, gt, [0, M], L)
    std64 = out[:, 0].astype(np.float64).std()
    floor = abs(float(np.std(out[:, 0])) - std64) / std64
    assert floor >= 2.0 ** -25 and abs(float(summary[0, 1]) - std64) / std64 <= 4 * floor
    assert out[:, 0].min() > 2e-3


def test_restatement_hand_cases():
    L = 5
    # pure translation along z, the prediction 2.5 x too long: scale 0.4, no residual, no rotation
    gt = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1.25], np.float32), (6, 1))
    pr = gt.copy()
    pr[:, 11] = 3.125
    o, s, c = R.pose_eval_ref(pr, gt, [0, 6], L)
    assert o.shape == (3, 3) and np.array_equal(o[:, 1], np.float32([0.4] * 3))
    assert np.array_equal(o[:, 0], np.zeros(3, np.float32)) and np.array_equal(o[:, 2], np.zeros(3, np.float32))
    # a motionless prediction: den = 0 -> scale 0, ate = |q| / L with q_j = 1.25 j along z
    pr[:, 9:] = 0
    o, s, c = R.pose_eval_ref(pr, gt, [0, 6], L)
    assert np.array_equal(o[:, 1], np.zeros(3, np.float32)) and c.tolist() == [[3, 0]]
    assert np.allclose(o[:, 0], 1.25 * np.sqrt(1 + 4 + 9 + 16) / L, rtol=1e-6)
    # sequences shorter than a snippet and boundaries
    o, s, c = R.pose_eval_ref(np.tile(gt, (7, 1))[:40], np.tile(gt, (7, 1))[:40], [0, 37, 40, 40], L)
    assert o.shape == (34, 3) and c.tolist() == [[34, 0], [0, 0], [0, 0]]
    assert np.isnan(s[1:]).all() and np.isfinite(s[0]).all()
