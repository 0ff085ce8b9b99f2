"""CPU checks of the BatchNorm entry points that carry the train step's operand forms
(md2_bn_forward_ex / md2_bn_backward_ex / md2_bn_ex_workspace_size / md2_bn_channel_fits and
md2_maxpool3s2_bwd_ex; include/md2.h): exports, prototypes, the struct layouts against their ctypes
mirrors, and the argument validation, which comes before any HIP call and so runs without a GPU.
A valid call is never made here: it would launch.  The kernels are checked in
tests/test_gpu_bn_ops.py."""
import ctypes as C
import os
import re

import pytest

from tests.test_julia_shim import HDR, LIB, _c_prototypes, _c_struct, _layout

MD2_EINVAL = 1
PROTOS = {"md2_bn_ex_workspace_size": 1, "md2_bn_channel_fits": 2, "md2_bn_forward_ex": 6,
          "md2_bn_backward_ex": 6, "md2_maxpool3s2_bwd_ex": 11}
WS_BYTES = 1 << 30      # claimed size of the never-dereferenced workspace
FWD_PTRS = ("y", "slab", "y_out", "part", "gamma", "beta", "mean", "invstd", "run_mean", "run_var", "y2", "gamma2",
            "beta2", "mean2", "invstd2", "res", "out", "pool_y", "pool_arg")
BWD_PTRS = ("dout", "slab", "dout_w", "mask", "y", "mean", "invstd", "gamma", "mbeta", "dgamma", "dbeta", "dy", "dres",
            "skip")


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    from md2hip import _lib
    lib = C.CDLL(LIB)
    for name in PROTOS:
        res, args = _lib._SIGS[name]
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    lib.md2_last_error.restype = C.c_char_p
    return lib


_BUF = (C.c_char * 1024)()
_BASE = (C.addressof(_BUF) + 15) // 16 * 16


def _p(k):
    """A non-null, 16-byte aligned pointer that is never dereferenced (validation comes first)."""
    return _BASE + 16 * k


def _desc(**over):
    from md2hip._lib import BNDesc
    f = dict(n=2, c=3, h=4, w=8, eps=1e-5, momentum=0.1, route=0, collapse=0)
    f.update(over)
    return BNDesc(**f)


def _fwd_ops(use=("y", "gamma", "beta", "mean", "invstd", "out"), **over):
    """Forward operands with the pointers named in `use` set (never dereferenced)."""
    from md2hip._lib import BNFwdOperands
    o = BNFwdOperands()
    for i, k in enumerate(FWD_PTRS):
        setattr(o, k, _p(i) if k in use else None)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _bwd_ops(use=("dout", "y", "mean", "invstd", "gamma", "dgamma", "dbeta", "dy"), **over):
    from md2hip._lib import BNBwdOperands
    o = BNBwdOperands()
    for i, k in enumerate(BWD_PTRS):
        setattr(o, k, _p(i) if k in use else None)
    for k, v in over.items():
        setattr(o, k, v)
    return o


FWD = ("y", "gamma", "beta", "mean", "invstd", "out")
BWD = ("dout", "y", "mean", "invstd", "gamma", "dgamma", "dbeta", "dy")


def _call(L, which, d, o, ws=True, ws_bytes=WS_BYTES, ws_shift=0):
    from md2hip._lib import BNInfo
    inf = BNInfo(family=-1)
    f = L.md2_bn_forward_ex if which == "fwd" else L.md2_bn_backward_ex
    rc = f(C.byref(d) if d is not None else None, C.byref(o) if o is not None else None, C.byref(inf),
           C.c_void_p(_p(40) + ws_shift) if ws else None, ws_bytes, None)
    assert inf.family == -1          # a refused call reports nothing
    return rc, L.md2_last_error()


def _refused(L, which, d, o, needle, **kw):
    rc, msg = _call(L, which, d, o, **kw)
    assert rc == MD2_EINVAL, (which, rc, msg)
    assert msg and needle in msg, msg


# ---- exports, prototypes, layouts -----------------------------------------------------------------
def test_library_exports_and_header():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    hdr = open(HDR).read()
    protos = _c_prototypes(hdr)
    from md2hip import _lib
    for s, nargs in PROTOS.items():
        assert hasattr(lib, s), s
        assert protos.get(s) == nargs, (s, protos.get(s))
        assert len(_lib._SIGS[s][1]) == nargs, s
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2      # additive


@pytest.mark.parametrize("c_name,py_name,size", [("md2_bn_desc", "BNDesc", 32), ("md2_bn_info", "BNInfo", 20),
                                                 ("md2_bn_fwd_operands", "BNFwdOperands", 168),
                                                 ("md2_bn_bwd_operands", "BNBwdOperands", 136)])
def test_python_struct_matches_header(c_name, py_name, size):
    from md2hip import _lib
    S = getattr(_lib, py_name)
    hdr = open(HDR).read().replace("const float*", "float*").replace("const double*", "float*")
    cf = _c_struct(hdr, c_name)
    assert [n for n, _, _ in cf] == [n for n, _ in S._fields_]
    assert [s for _, s, _ in cf] == [C.sizeof(t) for _, t in S._fields_]
    offs, total = _layout(cf)
    assert offs == [getattr(S, n).offset for n, _ in S._fields_]
    assert total == C.sizeof(S) == size


def test_channel_fits_is_host_arithmetic(L):
    # bn_channel_fits (csrc/bn_fwd.hip): hw % 4 == 0 and n * hw / 4 units <= 1024 threads x 2 units
    assert L.md2_bn_channel_fits(8, 32 * 32) == 1
    assert L.md2_bn_channel_fits(8, 4 * 260) == 0
    assert L.md2_bn_channel_fits(6, 2 * 3) == 0           # scalar units
    assert L.md2_bn_channel_fits(0, 16) == 0 and L.md2_bn_channel_fits(2, 0) == 0


def test_workspace_size(L):
    assert L.md2_bn_ex_workspace_size(None) == 0
    assert L.md2_bn_ex_workspace_size(C.byref(_desc(n=0))) == 0
    assert L.md2_bn_ex_workspace_size(C.byref(_desc(route=3))) == 0
    for d, parts in ((_desc(), 1), (_desc(n=80, c=3, h=32, w=64), 80)):
        # two partials slots [c][bn_parts][2] fp64 and one collapsed [c][2], each rounded up to 256 bytes
        need = L.md2_bn_ex_workspace_size(C.byref(d))
        up = lambda b: (b + 255) // 256 * 256
        assert need == 2 * up(16 * d.c * parts) + up(16 * d.c)


# ---- refused before any HIP call --------------------------------------------------------------------
@pytest.mark.parametrize("null", ["d", "o", "gamma", "beta", "mean", "invstd", "out", "ws"])
def test_forward_null_pointer_is_einval(L, null):
    d = None if null == "d" else _desc()
    o = None if null == "o" else _fwd_ops(tuple(k for k in FWD if k != null))
    _refused(L, "fwd", d, o, b"null pointer", ws=null != "ws")


@pytest.mark.parametrize("null", ["d", "o", "y", "mean", "invstd", "gamma", "dgamma", "dbeta", "dy", "ws"])
def test_backward_null_pointer_is_einval(L, null):
    d = None if null == "d" else _desc()
    o = None if null == "o" else _bwd_ops(tuple(k for k in BWD if k != null))
    _refused(L, "bwd", d, o, b"null pointer", ws=null != "ws")


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_input_is_exactly_one_of_tensor_and_slab(L, which):
    ops, base, t = (_fwd_ops, FWD, "y") if which == "fwd" else (_bwd_ops, BWD, "dout")
    _refused(L, which, _desc(), ops(tuple(k for k in base if k != t)), b"exactly one")
    _refused(L, which, _desc(), ops(base + ("slab", "y_out", "dout_w"), splits=2), b"exactly one")


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("bad", [dict(n=0), dict(c=0), dict(h=0), dict(w=-1), dict(route=3), dict(route=-1),
                                 dict(collapse=2), dict(n=1 << 10, c=1 << 10, h=1 << 6, w=1 << 6)])
def test_bad_descriptor_is_einval(L, which, bad):
    rc, msg = _call(L, which, _desc(**bad), _fwd_ops() if which == "fwd" else _bwd_ops())
    assert rc == MD2_EINVAL and msg, (which, bad)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("shape", [dict(n=8, c=3, h=4, w=260),        # 2080 float4 units: one more than a block holds
                                   dict(n=6, c=5, h=2, w=3)])         # scalar units
def test_one_kernel_route_where_the_channel_does_not_fit_is_einval(L, which, shape):
    _refused(L, which, _desc(route=2, **shape), _fwd_ops() if which == "fwd" else _bwd_ops(), b"route 2")
    assert L.md2_bn_ex_workspace_size(C.byref(_desc(route=2, **shape))) == 0


def test_forward_slab_forms(L):
    noy = tuple(k for k in FWD if k != "y")
    _refused(L, "fwd", _desc(), _fwd_ops(noy + ("slab", "y_out"), splits=0), b"splits")
    _refused(L, "fwd", _desc(), _fwd_ops(noy + ("slab",), splits=2), b"y_out")
    _refused(L, "fwd", _desc(), _fwd_ops(noy + ("slab", "y_out", "part"), splits=2, parts=4), b"slab with caller partials")


def test_forward_partials_forms(L):
    _refused(L, "fwd", _desc(), _fwd_ops(FWD + ("part",), parts=0), b"parts")
    _refused(L, "fwd", _desc(collapse=1), _fwd_ops(), b"collapse without caller partials")
    _refused(L, "fwd", _desc(route=2), _fwd_ops(FWD + ("part",), parts=3), b"route 2 with caller partials")


def test_forward_second_branch_and_running_statistics(L):
    for missing in ("gamma2", "beta2", "mean2", "invstd2"):
        use = FWD + tuple(k for k in ("y2", "gamma2", "beta2", "mean2", "invstd2") if k != missing)
        _refused(L, "fwd", _desc(), _fwd_ops(use), b"y2 needs")
    _refused(L, "fwd", _desc(), _fwd_ops(FWD + ("run_mean",)), b"run_mean and run_var")
    _refused(L, "fwd", _desc(), _fwd_ops(FWD + ("run_var",)), b"run_mean and run_var")
    _refused(L, "fwd", _desc(), _fwd_ops(relu=2), b"relu")


def test_forward_pool_outputs(L):
    pool = FWD + ("pool_y", "pool_arg")
    _refused(L, "fwd", _desc(h=5), _fwd_ops(pool, relu=1), b"even h and w")
    _refused(L, "fwd", _desc(w=7), _fwd_ops(pool, relu=1), b"even h and w")
    _refused(L, "fwd", _desc(), _fwd_ops(FWD + ("pool_y",), relu=1), b"pool_y and pool_arg")
    _refused(L, "fwd", _desc(), _fwd_ops(FWD + ("pool_arg",), relu=1), b"pool_y and pool_arg")
    _refused(L, "fwd", _desc(), _fwd_ops(pool, relu=0), b"pool outputs need relu")
    _refused(L, "fwd", _desc(), _fwd_ops(pool + ("res",), relu=1), b"pool outputs need relu")
    _refused(L, "fwd", _desc(), _fwd_ops(pool + ("y2", "gamma2", "beta2", "mean2", "invstd2"), relu=1),
             b"pool outputs need relu")
    _refused(L, "fwd", _desc(route=2), _fwd_ops(pool, relu=1), b"route 2 with pool outputs")


def test_backward_slab_forms(L):
    nod = tuple(k for k in BWD if k != "dout")
    _refused(L, "bwd", _desc(), _bwd_ops(nod + ("slab", "dout_w"), splits=0), b"splits")
    _refused(L, "bwd", _desc(), _bwd_ops(nod + ("slab", "dout_w", "mask"), splits=2), b"slab with a mask or a skip")
    _refused(L, "bwd", _desc(), _bwd_ops(nod + ("slab", "dout_w", "skip"), splits=2, skip_hi=64),
             b"slab with a mask or a skip")
    # two passes write the sum: dout_w is required there (route 1, or a channel that does not fit)
    _refused(L, "bwd", _desc(route=1), _bwd_ops(nod + ("slab",), splits=2), b"dout_w")
    _refused(L, "bwd", _desc(n=8, c=3, h=4, w=260), _bwd_ops(nod + ("slab",), splits=2), b"dout_w")


def test_backward_gate_and_dres(L):
    _refused(L, "bwd", _desc(), _bwd_ops(BWD + ("mask", "mbeta")), b"mask together with mbeta")
    _refused(L, "bwd", _desc(), _bwd_ops(BWD + ("dres",), dres_accumulate=2), b"dres_accumulate")


@pytest.mark.parametrize("route", [0, 1, 2])
def test_backward_skip_range(L, route):
    d = _desc(route=route)                 # 2 x 3 x 4 x 8 = 192 elements
    sk = BWD + ("skip",)
    _refused(L, "bwd", d, _bwd_ops(sk, skip_lo=-4, skip_hi=64), b"skip range")
    _refused(L, "bwd", d, _bwd_ops(sk, skip_lo=64, skip_hi=32), b"skip range")
    _refused(L, "bwd", d, _bwd_ops(sk, skip_lo=0, skip_hi=196), b"skip range")
    # the kernels read the addend in float4 units of the tensor: both ends on multiples of 4
    _refused(L, "bwd", d, _bwd_ops(sk, skip_lo=2, skip_hi=64), b"multiples of 4")
    _refused(L, "bwd", d, _bwd_ops(sk, skip_lo=0, skip_hi=62), b"multiples of 4")
    _refused(L, "bwd", d, _bwd_ops(sk, skip_lo=33, skip_hi=65), b"multiples of 4")


def test_backward_skip_needs_float4_planes(L):
    _refused(L, "bwd", _desc(n=6, c=5, h=2, w=3), _bwd_ops(BWD + ("skip",), skip_lo=0, skip_hi=60), b"h*w % 4")


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_misaligned_tensor_is_einval(L, which):
    o = _fwd_ops() if which == "fwd" else _bwd_ops()
    o.y = _p(0) + 4
    _refused(L, which, _desc(), o, b"aligned")
    # scalar units (h*w % 4 != 0) read single floats: no alignment demanded, the next check refuses
    _refused(L, which, _desc(h=1, w=3), o, b"workspace", ws_bytes=0)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_undersized_workspace_is_einval(L, which):
    o = _fwd_ops() if which == "fwd" else _bwd_ops()
    for d in (_desc(), _desc(n=80, c=3, h=32, w=64)):
        need = L.md2_bn_ex_workspace_size(C.byref(d))
        assert need > 0 and need % 256 == 0
        _refused(L, which, d, o, b"workspace", ws_bytes=need - 1)
        _refused(L, which, d, o, b"workspace", ws_bytes=0)
    _refused(L, which, _desc(), o, b"aligned", ws_shift=4)


# ---- md2_maxpool3s2_bwd_ex --------------------------------------------------------------------------
def _pool(L, null=None, n=3, c=4, h=6, w=8, skip=True, lo=0, hi=0, shift=0):
    a = dict(dy=_p(0), arg=_p(1), dx=_p(2))
    if null:
        a[null] = None
    rc = L.md2_maxpool3s2_bwd_ex(a["dy"], a["arg"], n, c, h, w, a["dx"], C.c_void_p(_p(3) + shift) if skip else None,
                                 lo, hi, None)
    return rc, L.md2_last_error()


@pytest.mark.parametrize("null", ["dy", "arg", "dx"])
def test_pool_null_pointer_is_einval(L, null):
    rc, msg = _pool(L, null=null)
    assert rc == MD2_EINVAL and b"null pointer" in msg


def test_pool_sizes_and_skip_range(L):
    for kw, needle in ((dict(n=0), b"positive"), (dict(h=0), b"positive"),
                       (dict(n=1 << 10, c=1 << 10, h=64, w=64, skip=False), b"2^31"),
                       (dict(w=7, hi=42), b"even w"),
                       (dict(lo=48, hi=48 * 4 + 8), b"skip range"),          # not a plane boundary
                       (dict(lo=24, hi=96), b"skip range"),
                       (dict(lo=96, hi=48), b"skip range"),
                       (dict(lo=-48, hi=48), b"skip range"),
                       (dict(lo=0, hi=3 * 4 * 48 + 48), b"skip range"),      # past the tensor
                       (dict(lo=0, hi=48, shift=4), b"aligned")):
        rc, msg = _pool(L, **kw)
        assert rc == MD2_EINVAL and needle in msg, (kw, rc, msg)
