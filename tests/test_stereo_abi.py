"""CPU checks of the sources (stereo) loss entry points (md2_loss_fwd_bwd_sources,
md2_loss_sources_workspace_size, md2_automasking_loss_sources, include/md2.h): exports, prototypes
and the md2_loss_source layout in the header, the Python binding and the Julia shim; the argument
errors, which are checked before any HIP call and so need no device; md2hip.stereo_transforms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _c_struct, _jl_ccalls, _jl_struct, _layout

MD2_EINVAL = 1
SYMBOLS = ("md2_loss_sources_workspace_size", "md2_loss_fwd_bwd_sources", "md2_automasking_loss_sources")
NARGS = {"md2_loss_sources_workspace_size": 2, "md2_loss_fwd_bwd_sources": 12, "md2_automasking_loss_sources": 10}


def _hdr():
    # _c_struct does not parse qualifiers
    return open(HDR).read().replace("const float*", "float*")


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    from md2hip._lib import _SIGS
    lib = C.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        getattr(lib, s).restype, getattr(lib, s).argtypes = _SIGS[s]
    lib.md2_last_error.restype = C.c_char_p
    return lib


def test_library_exports_and_header():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    hdr = open(HDR).read()
    protos = _c_prototypes(hdr)
    from md2hip import _lib
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert protos[s] == NARGS[s] == len(_lib._SIGS[s][1]), s
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2      # additive
    assert int(re.search(r"#define MD2_MAX_SOURCES (\d+)", hdr).group(1)) == 3 == _lib.MAX_SOURCES
    assert _lib.ABI_VERSION == 2
    lib.md2_abi_version.restype = C.c_int
    assert lib.md2_abi_version() == 2


def test_python_struct_matches_header():
    from md2hip._lib import LossSource
    cf = _c_struct(_hdr(), "md2_loss_source")
    assert [n for n, _, _ in cf] == [n for n, _ in LossSource._fields_]
    offs, size = _layout(cf)
    assert offs == [getattr(LossSource, n).offset for n, _ in LossSource._fields_] == [0, 8, 16, 20, 24]
    assert size == C.sizeof(LossSource) == 32


def test_julia_struct_and_ccalls_match_header():
    jl = open(JL).read()
    cf, jf = _c_struct(_hdr(), "md2_loss_source"), _jl_struct(jl, "LossSource")
    assert [(n, s, k) for n, s, k in cf] == [(n, s, k) for n, s, k in jf], (cf, jf)
    assert _layout(cf) == _layout(jf)
    protos = _c_prototypes(open(HDR).read())
    calls = dict(_jl_ccalls(jl))
    for s in SYMBOLS:
        assert calls.get(s) == protos[s], s
    assert int(re.search(r"const MAX_SOURCES = (\d+)", jl).group(1)) == 3
    assert re.search(r"function loss_tail_sources\(", jl)
    for s in ("md2_model_forward_loss_stereo", "md2_model_train_step_graph_stereo"):
        assert calls.get(s) == protos[s], s
    assert re.search(r"function train_loss_stereo\(m::HIPModel, x::ROCArray\{Float32,5\}, x_stereo::ROCArray\{Float32,4\}", jl)
    assert re.search(r"function train_step_graph_stereo!\(m::HIPModel", jl)
    assert re.search(r"function stereo_transforms\(sides, flips; baseline = 0\.1f0\)", jl)


# ---- argument errors: before any HIP call (a valid call is never made here: it would launch) -----
def _call(L, nsrc, sources, pose=True, target=True, cfg=True, out=True, ws=True, disp=True):
    from md2hip._lib import LossCfg, LossOut
    buf = (C.c_char * 256)()
    p = C.c_void_p(C.addressof(buf))      # non-null, never dereferenced
    c = LossCfg(n=2, c=3, width=64, height=32, nscales=1, divisor=1.0, min_depth=0.1, max_depth=100.0)
    c.scale_w[0], c.scale_h[0] = 64, 32
    o = LossOut()
    o.loss = p.value
    darr = (C.c_void_p * 5)(p.value)
    rc = L.md2_loss_fwd_bwd_sources(C.byref(c) if cfg else None, nsrc, sources, p if target else None, 3 * 3 * 32 * 64,
                                    C.cast(darr, C.POINTER(C.c_void_p)) if disp else None,
                                    p if pose else None, None, 1.0, C.byref(o) if out else None,
                                    p if ws else None, None)
    return rc, L.md2_last_error(), buf


def _sources(*specs):
    """specs: (pose_block, has_frames, has_Rt)"""
    from md2hip._lib import LossSource, MAX_SOURCES
    buf = (C.c_char * 64)()
    arr = (LossSource * max(MAX_SOURCES, len(specs)))()
    for s, (blk, fr, rt) in enumerate(specs):
        arr[s].frames = C.addressof(buf) if fr else None
        arr[s].sample_stride = 3 * 32 * 64
        arr[s].pose_block = blk
        arr[s].Rt = C.addressof(buf) if rt else None
    return arr, buf


LEARNED, FIXED = (0, True, False), (-1, True, True)


@pytest.mark.parametrize("nsrc", [0, 4, -1])
def test_nsrc_out_of_range_is_einval(L, nsrc):
    arr, keep = _sources(FIXED, FIXED, FIXED, FIXED)
    rc, msg, _ = _call(L, nsrc, arr)
    assert rc == MD2_EINVAL and b"nsrc" in msg, msg
    from md2hip._lib import LossCfg
    assert L.md2_loss_sources_workspace_size(C.byref(LossCfg(n=2, c=3, width=64, height=32, nscales=1)), nsrc) == 0
    out = (C.c_char * 64)()
    rc = L.md2_automasking_loss_sources(nsrc, arr, C.c_void_p(C.addressof(out)), 0, 2, 3, 32, 64,
                                        C.c_void_p(C.addressof(out)), None)
    assert rc == MD2_EINVAL and b"nsrc" in L.md2_last_error()


def test_learned_source_without_pose_is_einval(L):
    arr, keep = _sources(LEARNED, FIXED)
    rc, msg, _ = _call(L, 2, arr, pose=False)
    assert rc == MD2_EINVAL and b"learned source needs pose" in msg, msg


def test_fixed_source_without_Rt_is_einval(L):
    arr, keep = _sources((-1, True, False))
    rc, msg, _ = _call(L, 1, arr)
    assert rc == MD2_EINVAL and b"fixed source needs Rt" in msg, msg


@pytest.mark.parametrize("specs", [((1, True, False), FIXED),                 # block 1 with one learned source
                                   ((0, True, False), (0, True, False)),      # the same block twice
                                   ((-2, True, True),),                       # neither learned nor fixed
                                   ((3, True, False),)])
def test_bad_pose_blocks_are_einval(L, specs):
    arr, keep = _sources(*specs)
    rc, msg, _ = _call(L, len(specs), arr)
    assert rc == MD2_EINVAL and b"pose_block" in msg, msg


@pytest.mark.parametrize("which", ["cfg", "out", "target", "ws", "disp", "sources", "frames"])
def test_null_pointer_is_einval(L, which):
    arr, keep = _sources((-1, which != "frames", True))
    kw = {which: False} if which in ("cfg", "out", "target", "ws", "disp") else {}
    rc, msg, _ = _call(L, 1, None if which == "sources" else arr, **kw)
    assert rc == MD2_EINVAL, which
    assert msg


def test_workspace_size_grows_with_the_sources(L):
    from md2hip._lib import LossCfg
    c = LossCfg(n=2, c=3, width=64, height=32, nscales=1)
    c.scale_w[0], c.scale_h[0] = 64, 32
    s = [L.md2_loss_sources_workspace_size(C.byref(c), k) for k in (1, 2, 3)]
    assert 0 < s[0] <= s[1] <= s[2]
    assert L.md2_loss_sources_workspace_size(None, 2) == 0


# ---- md2hip.stereo_transforms -------------------------------------------------------------------
def test_stereo_transforms_signs():
    import md2hip
    Rt = md2hip.stereo_transforms(["l", "r", "l", "r"], [False, False, True, True])
    assert Rt.shape == (4, 12) and Rt.dtype == np.float32
    eye = np.eye(3, dtype=np.float32).reshape(-1)
    for i, tx in enumerate([-0.1, 0.1, 0.1, -0.1]):
        assert (Rt[i, :9] == eye).all()
        assert Rt[i, 9] == np.float32(tx) and Rt[i, 10] == 0 and Rt[i, 11] == 0
    assert (md2hip.stereo_transforms(["l", "r"]) == Rt[:2]).all()
    assert md2hip.stereo_transforms(["r"], [0], baseline=0.54)[0, 9] == np.float32(0.54)
    with pytest.raises(ValueError):
        md2hip.stereo_transforms(["x"])
    with pytest.raises(ValueError):
        md2hip.stereo_transforms(["l", "r"], [True])


def test_check_ids_points_to_x_stereo():
    import md2hip
    from md2hip.loss import _check_ids
    K, invK = md2hip.depth10k_intrinsics()
    with pytest.raises(ValueError, match="x_stereo"):
        _check_ids(md2hip.TrainCache(K=K, invK=invK, source_ids=(1, 3, 4)))
