"""CPU checks of the per-sample intrinsics entry points (md2_loss_fwd_bwd_sources_k,
md2_model_set_intrinsics, include/md2.h): exports, prototypes in the header, the Python binding and
the Julia shim; the ABI version, which they do not move; and the argument errors, which are checked
before any HIP call and so need no device."""
import ctypes as C
import os
import re

import pytest

from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _jl_ccalls
from tests.test_stereo_abi import FIXED, LEARNED, _sources

MD2_EINVAL = 1
NARGS = {"md2_loss_fwd_bwd_sources_k": 14, "md2_model_set_intrinsics": 4}


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    from md2hip._lib import _SIGS
    lib = C.CDLL(LIB)
    for s in NARGS:
        assert hasattr(lib, s), s
        getattr(lib, s).restype, getattr(lib, s).argtypes = _SIGS[s]
    lib.md2_last_error.restype = C.c_char_p
    return lib


def test_library_exports_header_and_bindings():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    hdr = open(HDR).read()
    protos = _c_prototypes(hdr)
    calls = dict(_jl_ccalls(open(JL).read()))
    from md2hip import _lib
    for s, n in NARGS.items():
        assert hasattr(lib, s), s
        assert protos[s] == n == len(_lib._SIGS[s][1]), s
        assert calls.get(s) == n, s
        assert s in _lib._INTRINSICS_SYMS          # an older library given for an A/B may lack them
    assert re.search(r"function set_intrinsics!\(m::HIPModel, K::ROCArray\{Float32,2\}, invK::ROCArray\{Float32,2\}\)",
                     open(JL).read())


def test_the_abi_version_does_not_move():
    from md2hip import _lib
    hdr = open(HDR).read()
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2
    assert _lib.ABI_VERSION == 2
    lib = C.CDLL(LIB)
    lib.md2_abi_version.restype = C.c_int
    assert lib.md2_abi_version() == 2


# ---- argument errors: before any HIP call (a valid call is never made here: it would launch) -----
def _call(L, nsrc, sources, K=True, invK=True, pose=True, target=True, cfg=True, out=True, ws=True, disp=True):
    from md2hip._lib import LossCfg, LossOut
    buf = (C.c_char * 256)()
    p = C.c_void_p(C.addressof(buf))      # non-null, never dereferenced
    c = LossCfg(n=2, c=3, width=64, height=32, nscales=1, divisor=1.0, min_depth=0.1, max_depth=100.0)
    c.scale_w[0], c.scale_h[0] = 64, 32
    o = LossOut()
    o.loss = p.value
    darr = (C.c_void_p * 5)(p.value)
    rc = L.md2_loss_fwd_bwd_sources_k(C.byref(c) if cfg else None, nsrc, sources, p if target else None,
                                      3 * 3 * 32 * 64, p if K else None, p if invK else None,
                                      C.cast(darr, C.POINTER(C.c_void_p)) if disp else None, p if pose else None,
                                      None, 1.0, C.byref(o) if out else None, p if ws else None, None)
    return rc, L.md2_last_error(), buf


@pytest.mark.parametrize("K,invK", [(False, True), (True, False), (False, False)])
def test_null_intrinsics_are_einval(L, K, invK):
    arr, keep = _sources(FIXED)
    rc, msg, _ = _call(L, 1, arr, K=K, invK=invK)
    assert rc == MD2_EINVAL and b"intrinsics" in msg, msg


@pytest.mark.parametrize("which", ["cfg", "out", "target", "ws", "disp", "sources", "frames"])
def test_the_uniform_forms_null_pointer_checks_hold(L, which):
    arr, keep = _sources((-1, which != "frames", True))
    kw = {which: False} if which in ("cfg", "out", "target", "ws", "disp") else {}
    rc, msg, _ = _call(L, 1, None if which == "sources" else arr, **kw)
    assert rc == MD2_EINVAL and msg, which


def test_the_uniform_forms_source_checks_hold(L):
    for nsrc in (0, 4, -1):
        arr, keep = _sources(FIXED, FIXED, FIXED, FIXED)
        rc, msg, _ = _call(L, nsrc, arr)
        assert rc == MD2_EINVAL and b"nsrc" in msg, msg
    arr, keep = _sources(LEARNED, FIXED)
    rc, msg, _ = _call(L, 2, arr, pose=False)
    assert rc == MD2_EINVAL and b"learned source needs pose" in msg, msg
    arr, keep = _sources((-1, True, False))
    rc, msg, _ = _call(L, 1, arr)
    assert rc == MD2_EINVAL and b"fixed source needs Rt" in msg, msg
    arr, keep = _sources((0, True, False), (0, True, False))
    rc, msg, _ = _call(L, 2, arr)
    assert rc == MD2_EINVAL and b"pose_block" in msg, msg


def test_set_intrinsics_argument_errors(L):
    buf = (C.c_char * 256)()
    p = C.c_void_p(C.addressof(buf))
    # exactly one of the two is null: refused before the model is looked at
    for K, invK in ((p, None), (None, p)):
        for m in (None, p):
            assert L.md2_model_set_intrinsics(m, K, invK, None) == MD2_EINVAL
            assert b"come together" in L.md2_last_error()
    # a null model
    assert L.md2_model_set_intrinsics(None, p, p, None) == MD2_EINVAL
    assert L.md2_model_set_intrinsics(None, None, None, None) == MD2_EINVAL


def test_check_intrinsics_shapes_and_the_host_inverse():
    import numpy as np
    import torch
    from md2hip.loss import check_intrinsics
    assert check_intrinsics(None, None, 2, "cpu") == (None, None)
    K = torch.tensor([[[100.0, 0, 31.5], [0, 103.0, 17.25], [0, 0, 1]], [[90.0, 0, 30.0], [0, 95.0, 16.0], [0, 0, 1]]])
    a, b = check_intrinsics(K, None, 2, "cpu")
    assert a.shape == (2, 9) and b.shape == (2, 9) and a.dtype == b.dtype == torch.float32
    want = np.linalg.inv(K.numpy().astype(np.float64)).astype(np.float32).reshape(2, 9)
    assert (b.numpy() == want).all()
    a2, b2 = check_intrinsics(K.reshape(2, 9), b.reshape(2, 3, 3), 2, "cpu")
    assert torch.equal(a, a2) and torch.equal(b, b2)
    for bad in (K[:1], K.double(), K.reshape(18), K.numpy()):
        with pytest.raises(ValueError):
            check_intrinsics(bad, None, 2, "cpu")
    with pytest.raises(ValueError):
        check_intrinsics(K, b[:1], 2, "cpu")
    with pytest.raises(ValueError):
        check_intrinsics(None, b, 2, "cpu")
