"""CPU checks of the LiDAR depth-map and flip post-processing entry points (md2_lidar_depth,
md2_disp_post_process, include/md2.h): exports, argument validation (which comes before any HIP
call, so it runs without a GPU), the Python wrappers' own checks, the calibration and scan readers,
the Julia struct / ccalls, and the float32 NumPy restatement of the tests against float64.

The restatement check.  float32 and float64 may round a point into different pixels only when its
u or v lies next to a half-integer; MARGIN_PX = 2e-3 px is 5 x the largest fp32 coordinate error
seen at 375 x 1242 (3.6e-4 px).  On the pixels no such point can reach ("clean") the two must have
identical support and values within 1e-6 relative: the fp32 dot-product bound 4 * 2^-24 *
sum|terms| / |z| ~ 2.6e-7 with a 4 x margin (2.0e-7 observed).  As a condition on the inputs the
dirty pixels are at most 3 % of the hit pixels at 375 x 1242 (1.4 - 1.7 % over five seeds) and at
most 10 % at the small sizes, which hit only ~75 - 450 pixels (0 - 8 % seen)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _lidar_ref as R
from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _c_struct, _jl_ccalls, _jl_struct, _layout

MD2_EINVAL = 1
SYMBOLS = ("md2_lidar_depth", "md2_disp_post_process")

IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
NAN, INF = float("nan"), float("inf")

# name -> (cfg overrides, offsets, P): every one must be refused
INVALID = {
    "n_zero": (dict(n=0), [0, 0, 0], None),
    "n_negative": (dict(n=-1), [0, 0, 0], None),
    "n_65": (dict(n=65), list(range(66)), IDENT * 65),
    "h_zero": (dict(h=0), None, None),
    "w_zero": (dict(w=0), None, None),
    "h_negative": (dict(h=-4), None, None),
    "hw_too_large": (dict(h=4097, w=4096), None, None),
    "offset0_negative": ({}, [-1, 3, 5], None),
    "offsets_decrease": ({}, [0, 5, 4], None),
    "offsets_decrease_first": ({}, [6, 5, 7], None),
    "offsets_past_2_27": ({}, [0, 5, (1 << 27) + 1], None),
    "P_nan": ({}, None, IDENT + IDENT[:7] + [NAN] + IDENT[8:]),
    "P_inf": ({}, None, [INF] + IDENT[1:] + IDENT),
    "P_minus_inf_last": ({}, None, IDENT + IDENT[:11] + [-INF]),
    "forward_only_2": (dict(forward_only=2), None, None),
    "forward_only_negative": (dict(forward_only=-1), None, None),
    "vel_depth_2": (dict(vel_depth=2), None, None),
}


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    from md2hip._lib import LidarCfg
    lib = C.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    lib.md2_lidar_depth.restype = C.c_int
    lib.md2_lidar_depth.argtypes = [C.POINTER(LidarCfg), C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_float),
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.md2_disp_post_process.restype = C.c_int
    lib.md2_disp_post_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.md2_last_error.restype = C.c_char_p
    return lib


def _dummy(k=0):
    """A non-null, 16-byte aligned pointer that is never dereferenced (validation comes first)."""
    buf = (C.c_char * 256)()
    a = C.addressof(buf)
    return buf, C.c_void_p((a + 15) // 16 * 16 + 16 * k)


def _args(over=None, offsets=None, P=None):
    from md2hip._lib import LidarCfg
    cfg = LidarCfg(**{**dict(n=2, h=8, w=16, forward_only=1, vel_depth=0), **(over or {})})
    offsets = [0, 3, 5] if offsets is None else offsets
    P = IDENT * 2 if P is None else P
    return cfg, (C.c_longlong * len(offsets))(*offsets), (C.c_float * len(P))(*P)


# ---- exports, prototypes, layouts -----------------------------------------------------------------
def test_library_exports_and_header():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    hdr = open(HDR).read()
    protos = _c_prototypes(hdr)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in protos, s
    assert protos["md2_lidar_depth"] == 7 and protos["md2_disp_post_process"] == 7
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2      # additive
    assert int(re.search(r"#define MD2_LIDAR_MAX_SCANS (\d+)", hdr).group(1)) == 64
    from md2hip import _lib
    assert _lib.LIDAR_MAX_SCANS == 64
    assert len(_lib._SIGS["md2_lidar_depth"][1]) == 7 and len(_lib._SIGS["md2_disp_post_process"][1]) == 7


def test_python_struct_matches_header():
    from md2hip._lib import LidarCfg
    cf = _c_struct(open(HDR).read(), "md2_lidar_cfg")
    assert [n for n, _, _ in cf] == [n for n, _ in LidarCfg._fields_]
    offs, size = _layout(cf)
    assert offs == [getattr(LidarCfg, n).offset for n, _ in LidarCfg._fields_]
    assert size == C.sizeof(LidarCfg) == 20


def test_julia_struct_matches_header():
    jl, hdr = open(JL).read(), open(HDR).read()
    cf, jf = _c_struct(hdr, "md2_lidar_cfg"), _jl_struct(jl, "LidarCfg")
    assert [n for n, _, _ in cf] == [n for n, _, _ in jf]
    assert [(s, n) for _, s, n in cf] == [(s, n) for _, s, n in jf], (cf, jf)
    assert _layout(cf) == _layout(jf)


def test_julia_ccalls_match_header():
    jl, hdr = open(JL).read(), open(HDR).read()
    protos = _c_prototypes(hdr)
    calls = dict(_jl_ccalls(jl))
    for name in SYMBOLS:
        assert name in calls, f"julia/MD2HIP.jl does not call {name}"
        assert calls[name] == protos[name]
    assert re.search(r"function lidar_depth\(points::ROCArray\{Float32,2\}, offsets::Vector\{Int64\}, "
                     r"P::Array\{Float32\}, h, w;", jl)
    assert re.search(r"function post_process_disparity\(disp::ROCArray\{Float32\}", jl)
    assert int(re.search(r"const LIDAR_MAX_SCANS = (\d+)", jl).group(1)) == 64


# ---- md2_lidar_depth refuses, before any HIP call --------------------------------------------------
# (a valid call is never made here: it would launch)
@pytest.mark.parametrize("name", sorted(INVALID))
def test_lidar_invalid_is_einval(L, name):
    over, offsets, P = INVALID[name]
    cfg, off, Pm = _args(over, offsets, P)
    keep, p = _dummy()
    rc = L.md2_lidar_depth(C.byref(cfg), p, off, Pm, p, p, None)
    assert rc == MD2_EINVAL, name
    msg = L.md2_last_error()
    assert msg and b"lidar_depth" in msg, msg


@pytest.mark.parametrize("which", ["cfg", "points", "offsets", "P", "depth"])
def test_lidar_null_pointer_is_einval(L, which):
    cfg, off, Pm = _args()
    keep, p = _dummy()
    args = dict(cfg=C.byref(cfg), points=p, offsets=off, P=Pm, depth=p)
    args[which] = None
    rc = L.md2_lidar_depth(args["cfg"], args["points"], args["offsets"], args["P"], args["depth"], p, None)
    assert rc == MD2_EINVAL
    assert b"lidar_depth" in L.md2_last_error()


def test_lidar_misaligned_points_is_einval(L):
    cfg, off, Pm = _args()
    keep, p = _dummy()
    rc = L.md2_lidar_depth(C.byref(cfg), C.c_void_p(p.value + 4), off, Pm, p, p, None)
    assert rc == MD2_EINVAL and b"lidar_depth" in L.md2_last_error()


# ---- md2_disp_post_process refuses -----------------------------------------------------------------
@pytest.mark.parametrize("name,n,h,w", [("n_zero", 0, 8, 16), ("h_zero", 2, 0, 16), ("w_zero", 2, 8, 0),
                                        ("n_negative", -2, 8, 16), ("w_negative", 2, 8, -16)])
def test_post_process_bad_size_is_einval(L, name, n, h, w):
    keep, a = _dummy(0)
    _, b = keep, C.c_void_p(a.value + 64)
    assert L.md2_disp_post_process(a, b, n, h, w, a, None) == MD2_EINVAL
    assert b"disp_post_process" in L.md2_last_error()


@pytest.mark.parametrize("which", range(3))
def test_post_process_null_pointer_is_einval(L, which):
    keep, a = _dummy(0)
    ptrs = [a, C.c_void_p(a.value + 64), C.c_void_p(a.value + 128)]
    ptrs[which] = None
    assert L.md2_disp_post_process(ptrs[0], ptrs[1], 2, 8, 16, ptrs[2], None) == MD2_EINVAL
    assert L.md2_last_error()


def test_post_process_out_aliasing_flipped_is_einval(L):
    keep, a = _dummy(0)
    b = C.c_void_p(a.value + 64)
    assert L.md2_disp_post_process(a, b, 2, 8, 16, b, None) == MD2_EINVAL
    assert b"alias" in L.md2_last_error()


# ---- the Python wrappers refuse bad tensors before the library -------------------------------------
def _no_lib():
    raise AssertionError("the wrapper reached the library")


def test_lidar_depth_rejects_bad_arguments(monkeypatch):
    import torch
    import md2hip
    from md2hip import lidar
    monkeypatch.setattr(lidar, "lib", _no_lib)
    P = np.eye(3, 4, dtype=np.float32)
    cpu = torch.zeros(5, 4)
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.lidar_depth([cpu], P, 8, 16)                                   # CPU scan
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.lidar_depth([cpu.double()], P, 8, 16)                          # float64
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.lidar_depth([torch.zeros(5, 3)], P, 8, 16)                     # three columns
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.lidar_depth([torch.zeros(20)], P, 8, 16)                       # rank 1
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.lidar_depth((cpu, [0, 2, 5]), P, 8, 16)                        # pair form, CPU points
    with pytest.raises(ValueError, match="non-empty"):
        md2hip.lidar_depth([], P, 8, 16)
    with pytest.raises(ValueError, match="non-empty"):
        md2hip.lidar_depth(cpu, P, 8, 16)                                     # a bare tensor


def test_lidar_depth_rejects_bad_P(monkeypatch):
    """The P checks follow the tensor checks: reached here with the tensor checks stubbed out."""
    import torch
    import md2hip
    from md2hip import lidar
    monkeypatch.setattr(lidar, "lib", _no_lib)
    pts = torch.zeros(5, 4)
    off = np.array([0, 2, 5])
    monkeypatch.setattr(lidar, "_points_and_offsets", lambda scans: (pts, off.astype(np.int64)))
    with pytest.raises(ValueError, match=r"P must be \[3, 4\] or \[2, 3, 4\]"):
        md2hip.lidar_depth((pts, off), np.zeros((3, 3, 4), np.float32), 8, 16)        # three matrices, two scans
    with pytest.raises(ValueError, match="P must be"):
        md2hip.lidar_depth((pts, off), np.zeros((4, 3), np.float32), 8, 16)
    with pytest.raises(ValueError, match="floating-point"):
        md2hip.lidar_depth((pts, off), np.zeros((3, 4), np.int32), 8, 16)


def test_post_process_rejects_bad_tensors(monkeypatch):
    import torch
    import md2hip
    from md2hip import lidar
    monkeypatch.setattr(lidar, "lib", _no_lib)
    d = torch.zeros(2, 1, 8, 16)
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.post_process_disparity(d, d.clone())                           # CPU tensors
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.post_process_disparity(d.double(), d.double())
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.post_process_disparity(d.numpy(), d.numpy())


# ---- host helpers ------------------------------------------------------------------------------------
def _fmt(v):
    return " ".join(f"{x:.12e}" for x in np.asarray(v).ravel())


def test_kitti_odometry_calibration(tmp_path):
    import md2hip
    rng = np.random.default_rng(3)
    Ps = [np.hstack([R.K, rng.uniform(-400, 50, (3, 1))]) for _ in range(4)]
    path = tmp_path / "calib.txt"
    path.write_text("".join(f"P{i}: {_fmt(P)}\n" for i, P in enumerate(Ps)) + f"Tr: {_fmt(R.TR)}\n")
    for cam in range(4):
        got = md2hip.kitti_odometry_velo_to_image(str(path), cam=cam)
        # the file holds 13 significant digits: compose what was written, in float64, round once
        P = np.array(_fmt(Ps[cam]).split(), dtype=np.float64).reshape(3, 4)
        Tr = np.array(_fmt(R.TR).split(), dtype=np.float64).reshape(3, 4)
        want = (P @ np.vstack([Tr, [0, 0, 0, 1]])).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (3, 4)
        assert np.array_equal(got, want), cam
    assert np.array_equal(md2hip.kitti_odometry_velo_to_image(str(path)),
                          md2hip.kitti_odometry_velo_to_image(str(path), cam=0))
    (tmp_path / "short.txt").write_text(f"P0: {_fmt(Ps[0])}\n")
    with pytest.raises(ValueError, match="Tr:"):
        md2hip.kitti_odometry_velo_to_image(str(tmp_path / "short.txt"))


def test_kitti_raw_calibration(tmp_path):
    import md2hip
    rng = np.random.default_rng(4)
    th = 0.01
    Rrect = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    Prect = {c: np.hstack([R.K, rng.uniform(-400, 50, (3, 1))]) for c in (0, 2, 3)}
    c2c = tmp_path / "calib_cam_to_cam.txt"
    c2c.write_text("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n"
                   f"S_00: 1.392000e+03 5.120000e+02\nR_rect_00: {_fmt(Rrect)}\n"
                   + "".join(f"P_rect_0{c}: {_fmt(P)}\n" for c, P in Prect.items()))
    v2c = tmp_path / "calib_velo_to_cam.txt"
    v2c.write_text(f"calib_time: 15-Mar-2012 11:37:16\nR: {_fmt(R.TR[:, :3])}\nT: {_fmt(R.TR[:, 3])}\n"
                   "delta_f: 0.000000e+00 0.000000e+00\n")

    def rd(v):
        return np.array(_fmt(v).split(), dtype=np.float64).reshape(np.asarray(v).shape)
    for cam in (2, 3, 0):
        got = md2hip.kitti_raw_velo_to_image(str(c2c), str(v2c), cam=cam)
        rect = np.eye(4)
        rect[:3, :3] = rd(Rrect)
        velo = np.vstack([np.hstack([rd(R.TR[:, :3]), rd(R.TR[:, 3]).reshape(3, 1)]), [0, 0, 0, 1]])
        want = (rd(Prect[cam]) @ rect @ velo).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (3, 4)
        assert np.array_equal(got, want), cam
    assert np.array_equal(md2hip.kitti_raw_velo_to_image(str(c2c), str(v2c)),
                          md2hip.kitti_raw_velo_to_image(str(c2c), str(v2c), cam=2))
    with pytest.raises(ValueError, match="P_rect_01"):
        md2hip.kitti_raw_velo_to_image(str(c2c), str(v2c), cam=1)


def test_load_velodyne(tmp_path):
    import md2hip
    pts = R.make_scan(np.random.default_rng(5), 321)
    path = tmp_path / "000000.bin"
    pts.tofile(path)
    got = md2hip.load_velodyne(str(path))
    assert got.dtype == np.float32 and got.shape == (321, 4) and np.array_equal(got, pts)
    with open(tmp_path / "cut.bin", "wb") as f:
        f.write(pts.tobytes()[:-4])
    with pytest.raises(ValueError, match="16-byte"):
        md2hip.load_velodyne(str(tmp_path / "cut.bin"))
    open(tmp_path / "empty.bin", "wb").close()
    assert md2hip.load_velodyne(str(tmp_path / "empty.bin")).shape == (0, 4)


# ---- the float32 restatement against float64 -------------------------------------------------------
@pytest.mark.parametrize("h,w,m,cap", [(375, 1242, 120000, 0.03), (24, 80, 4000, 0.10), (8, 16, 700, 0.10)])
@pytest.mark.parametrize("vel_depth", [False, True])
def test_restatement_float32_against_float64(h, w, m, cap, vel_depth):
    # the sizes and scan lengths of the device tests (tests/test_gpu_lidar.py)
    points, offsets = R.make_scans(100 + h, [m])
    P = R.calib(h, w)
    d32, c32 = R.lidar_depth_ref(points, offsets, P, h, w, vel_depth=vel_depth)
    d64, c64 = R.lidar_depth_ref(points, offsets, P, h, w, vel_depth=vel_depth, dtype=np.float64)
    assert d32.dtype == np.float32 and d64.dtype == np.float64
    dirty = R.dirty_pixels(points, offsets, P, h, w, vel_depth=vel_depth)
    hit = int((d64 != 0).sum())
    share = dirty.sum() / hit
    print(f"{h}x{w}: hit {hit}, stored {c64[0, 0]}, dirty {int(dirty.sum())} ({100 * share:.2f} %)")
    assert hit > 50 and c64[0, 1] == hit
    assert share <= cap, (share, cap)                       # condition on the inputs
    clean = ~dirty
    assert np.array_equal((d32 != 0) & clean, (d64 != 0) & clean)
    both = clean & (d64 != 0)
    rel = np.abs(d32[both].astype(np.float64) - d64[both]) / d64[both]
    print(f"  largest relative difference on clean pixels {rel.max():.3e}")
    # the stored x_velo is an input, not a computed value: exact
    assert rel.max() <= (0.0 if vel_depth else 1e-6)
    # counts differ by no more than the points next to a boundary can explain
    assert abs(int(c32[0, 1]) - int(c64[0, 1])) <= dirty.sum()


def test_generator_statistics():
    """The workload the issue describes: ~13 % of a scan lands in the 375 x 1242 image, ~15 k pixels
    are hit, a few hundred points lose a collision."""
    points, offsets = R.make_scans(0, [120000])
    d, c = R.lidar_depth_ref(points, offsets, R.calib(), R.CAM_H, R.CAM_W)
    stored, hit = int(c[0, 0]), int(c[0, 1])
    print(f"stored {stored} ({100 * stored / 120000:.1f} %), hit {hit}, collisions {stored - hit}")
    assert 0.10 * 120000 < stored < 0.16 * 120000
    assert 12000 < hit < 18000
    assert 100 < stored - hit < 1500
    assert (d >= 0).all() and np.isfinite(d).all()


def test_restatement_hand_cases():
    """Ties, the minus one, the edges and the drops, on exact coordinates (P = [I | 0], depth 2)."""
    P = np.eye(3, 4, dtype=np.float32)
    h, w = 4, 6

    def one(u, v, z=2.0, **kw):
        pts = np.array([[u * z, v * z, z, 0.5]], dtype=np.float32)
        return R.lidar_depth_ref(pts, np.array([0, 1]), P, h, w, forward_only=False, **kw)
    d, c = one(2.5, 1.0)
    assert d[0, 0, 1] == 2.0 and c.tolist() == [[1, 1]]        # 2.5 -> 2 -> ix 1
    assert one(3.5, 1.0)[0][0, 0, 3] == 2.0                    # 3.5 -> 4 -> ix 3
    assert one(0.5, 1.0)[1].tolist() == [[0, 0]]               # rint 0 -> ix -1
    assert one(1.0, 1.0)[0][0, 0, 0] == 2.0
    assert one(float(w), float(h))[0][0, h - 1, w - 1] == 2.0
    assert one(w + 0.5 + 2.0 ** -10, 1.0)[1].tolist() == [[0, 0]]
    assert one(1.0, h + 0.5 + 2.0 ** -10)[1].tolist() == [[0, 0]]
    assert one(1.0, 1.0, z=-2.0)[1].tolist() == [[0, 0]]
    assert one(1e30, 1.0)[1].tolist() == [[0, 0]]              # a huge u does not wrap


def test_post_process_restatement():
    rng = np.random.default_rng(8)
    for w in (1, 16, 21):
        a = rng.uniform(0.01, 1.0, (2, 8, w)).astype(np.float32)
        b = rng.uniform(0.01, 1.0, (2, 8, w)).astype(np.float32)
        o32, o64 = R.post_process_ref(a, b), R.post_process_ref(a, b, dtype=np.float64)
        assert o32.dtype == np.float32
        # a handful of fp32 roundings of values <= 1
        assert np.abs(o32 - o64).max() <= 8 * 2.0 ** -24
        sym = R.post_process_ref(a, a[..., ::-1])
        assert np.abs(sym - a).max() <= 4 * 2.0 ** -24
    # w = 21: t(10) = 0.5, both ramps are 0 in the middle column -> the plain mean
    a = rng.uniform(0.01, 1.0, (1, 3, 21)).astype(np.float32)
    b = rng.uniform(0.01, 1.0, (1, 3, 21)).astype(np.float32)
    o = R.post_process_ref(a, b)
    assert np.array_equal(o[..., 10], np.float32(0.5) * (a[..., 10] + b[..., 10]))
    # the left edge takes the mirrored prediction, the right edge the direct one
    assert np.array_equal(o[..., 0], b[..., 20]) and np.array_equal(o[..., 20], a[..., 20])
