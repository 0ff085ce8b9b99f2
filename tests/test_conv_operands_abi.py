"""CPU checks of the conv entry points that carry the train step's operand forms
(md2_conv2d_fwd_ex / dgrad_ex / wgrad_ex, md2_act_backward_bias, md2_conv_last_kernel;
include/md2.h): exports, prototypes, the struct layouts against their ctypes mirrors, and the
argument validation, which comes before any HIP call and so runs without a GPU.  A valid call is
never made here: it would launch.  The kernels are checked in tests/test_gpu_conv_operands.py."""
import ctypes as C
import os
import re

import pytest

from tests.test_julia_shim import HDR, LIB, _c_prototypes, _c_struct, _layout

MD2_EINVAL = 1
PROTOS = {"md2_conv2d_ex_workspace_size": 2, "md2_conv2d_fwd_ex": 11, "md2_conv2d_dgrad_ex": 9,
          "md2_conv2d_wgrad_ex": 11, "md2_act_bias_parts": 3, "md2_act_backward_bias": 9,
          "md2_conv_last_kernel": 0}
WS_BYTES = 1 << 30      # claimed size of the never-dereferenced workspace: large enough for every case


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


def _dummy(k=0):
    """A non-null, 16-byte aligned pointer that is never dereferenced (validation comes first)."""
    buf = (C.c_char * 512)()
    a = C.addressof(buf)
    return buf, C.c_void_p((a + 15) // 16 * 16 + 16 * k)


def _desc(**over):
    from md2hip._lib import ConvDesc
    f = dict(n=2, cin=64, h=6, w=10, cout=32, kh=3, kw=3, stride=1, pad=1, reflect=0, act=0)
    f.update(over)
    return ConvDesc(**f)


def _ops(**f):
    from md2hip._lib import ConvOperands
    return ConvOperands(**f)


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


@pytest.mark.parametrize("c_name,py_name,size", [("md2_conv_operands", "ConvOperands", 80),
                                                 ("md2_conv_defer", "ConvDefer", 24),
                                                 ("md2_conv_desc", "ConvDesc", 44)])
def test_python_struct_matches_header(c_name, py_name, size):
    from md2hip import _lib
    S = getattr(_lib, py_name)
    cf = _c_struct(open(HDR).read().replace("const float*", "float*"), c_name)
    assert [n for n, _, _ in cf] == [n for n, _ in S._fields_]
    assert [s for _, s, _ in cf] == [C.sizeof(t) for _, t in S._fields_]
    offs, total = _layout(cf)
    assert offs == [getattr(S, n).offset for n, _ in S._fields_]
    assert total == C.sizeof(S) == size


def test_last_kernel_is_a_string_and_refusals_leave_it(L):
    before = L.md2_conv_last_kernel()
    assert isinstance(before, bytes)          # "" until this thread launches a conv
    _refused(L, "fwd", _desc(), _ops(in_c0=32), b"in1")
    assert L.md2_conv_last_kernel() == before


def test_act_bias_parts_is_host_arithmetic(L):
    # act_bias_parts (csrc/conv.hip): min(max(1, 2048 / c), n*hw/4 / 1024 + 1), at least 1
    assert L.md2_act_bias_parts(20, 2, 48) == 1
    assert L.md2_act_bias_parts(64, 2, 64 * 208) == min(2048 // 64, 2 * 64 * 208 // 4 // 1024 + 1)
    assert L.md2_act_bias_parts(0, 2, 48) == 0 and L.md2_act_bias_parts(4, 0, 48) == 0


# ---- refused before any HIP call --------------------------------------------------------------------
def _call(L, which, d, o, null=None, db=True, db_part=False, db_parts=0, stats=False, defer=False, ws_bytes=WS_BYTES,
          ws_shift=0):
    from md2hip._lib import ConvDefer
    keep, p = _dummy()
    a = {k: C.c_void_p(p.value + 16 * i) for i, k in enumerate(("x", "w", "bias", "y", "dy", "dx", "dw", "db", "part",
                                                                "stats", "ws"))}
    a["ws"] = C.c_void_p(a["ws"].value + ws_shift)
    if null:
        a[null] = None
    dp = C.byref(d) if null != "d" else None
    op = C.byref(o) if o is not None else None
    df = ConvDefer()
    dfp = C.byref(df) if defer else None
    if which == "fwd":
        rc = L.md2_conv2d_fwd_ex(dp, op, a["x"], a["w"], a["bias"], a["y"], a["stats"] if stats else None, dfp,
                                 a["ws"], ws_bytes, None)
    elif which == "dgrad":
        rc = L.md2_conv2d_dgrad_ex(dp, op, a["dy"], a["w"], a["dx"], dfp, a["ws"], ws_bytes, None)
    else:
        rc = L.md2_conv2d_wgrad_ex(dp, op, a["x"], a["dy"], a["dw"], a["db"] if db else None,
                                   a["part"] if db_part else None, db_parts, a["ws"], ws_bytes, None)
    return rc, L.md2_last_error()


def _refused(L, which, d, o, needle, **kw):
    rc, msg = _call(L, which, d, o, **kw)
    assert rc == MD2_EINVAL, (which, rc, msg)
    assert msg and needle in msg, msg


@pytest.mark.parametrize("which,null", [("fwd", "d"), ("fwd", "x"), ("fwd", "w"), ("fwd", "y"), ("fwd", "ws"),
                                        ("dgrad", "d"), ("dgrad", "dy"), ("dgrad", "w"), ("dgrad", "dx"),
                                        ("dgrad", "ws"), ("wgrad", "d"), ("wgrad", "x"), ("wgrad", "dy"),
                                        ("wgrad", "dw"), ("wgrad", "ws")])
def test_null_pointer_is_einval(L, which, null):
    _refused(L, which, _desc(), None, b"null pointer", null=null)


@pytest.mark.parametrize("which", ["fwd", "wgrad"])
def test_in_c0_past_cin_is_einval(L, which):
    keep, p = _dummy(20)
    _refused(L, which, _desc(), _ops(in_c0=80, in1=p.value), b"in_c0")
    _refused(L, which, _desc(), _ops(in_c0=-16, in1=p.value), b"in_c0")


@pytest.mark.parametrize("which", ["fwd", "wgrad"])
def test_missing_second_input_is_einval(L, which):
    _refused(L, which, _desc(), _ops(in_c0=32), b"in1")


def test_out_c0_past_rows_and_missing_second_output_are_einval(L):
    keep, p = _dummy(20)
    _refused(L, "dgrad", _desc(), _ops(out_c0=65, out1=p.value), b"out_c0")      # dgrad rows = cin = 64
    _refused(L, "fwd", _desc(), _ops(out_c0=33, out1=p.value), b"out_c0")        # forward rows = cout = 32
    _refused(L, "dgrad", _desc(), _ops(out_c0=32), b"out1")
    _refused(L, "fwd", _desc(), _ops(out_c0=16), b"out1")


def test_concat_split_inside_a_16_channel_chunk_is_einval(L):
    keep, p = _dummy(20)
    _refused(L, "fwd", _desc(), _ops(in_c0=24, in1=p.value), b"multiple of 16")


def test_output_stride_smaller_than_its_rows_is_einval(L):
    keep, p = _dummy(20)
    _refused(L, "dgrad", _desc(), _ops(out_bs0=64 * 60 - 1), b"out_bs0")
    _refused(L, "dgrad", _desc(), _ops(out_c0=32, out1=p.value, out_bs1=32 * 60 - 4), b"out_bs1")
    _refused(L, "fwd", _desc(), _ops(accumulate=2), b"accumulate")
    _refused(L, "wgrad", _desc(), _ops(accumulate=-1), b"accumulate")


@pytest.mark.parametrize("which", ["fwd", "dgrad", "wgrad"])
def test_cin_w_is_checked(L, which):
    _refused(L, which, _desc(), _ops(cin_w=65), b"cin_w")                         # more weight channels than cin
    _refused(L, which, _desc(cout=1), _ops(cin_w=53), b"cin_w")                   # a padded head conv
    _refused(L, which, _desc(cin=24), _ops(cin_w=20), b"cin % 16")
    _refused(L, which, _desc(), _ops(cin_w=-1), b"cin_w")


def test_db_part_without_db_is_einval(L):
    _refused(L, "wgrad", _desc(), None, b"db_part without db", db=False, db_part=True, db_parts=2)
    _refused(L, "wgrad", _desc(), None, b"db_parts", db=True, db_part=True, db_parts=0)


def test_stats_without_defer_is_einval(L):
    _refused(L, "fwd", _desc(), None, b"stats", stats=True)


@pytest.mark.parametrize("which", ["fwd", "dgrad", "wgrad"])
def test_undersized_workspace_is_einval(L, which):
    for d, o in ((_desc(), None), (_desc(n=2, cin=512, h=2, w=4, cout=256), _ops(cin_w=501))):
        need = L.md2_conv2d_ex_workspace_size(C.byref(d), C.byref(o) if o is not None else None)
        assert need > 0 and need % 256 == 0
        _refused(L, which, d, o, b"workspace", ws_bytes=need - 1)
        _refused(L, which, d, o, b"workspace", ws_bytes=0)
    _refused(L, which, _desc(), None, b"aligned", ws_shift=4)


def test_workspace_size_matches_the_plain_entry(L):
    """No operand form changes the sizing functions' shape except cin_w: with ops == NULL the
    extended size is the plain one (both are packed operand + the largest conv_*_workspace)."""
    from md2hip._lib import ConvDesc
    L.md2_conv2d_workspace_size.restype = C.c_size_t
    L.md2_conv2d_workspace_size.argtypes = [C.POINTER(ConvDesc)]
    for d in (_desc(), _desc(n=6, cin=256, h=4, w=8, cout=512, stride=2), _desc(cin=3, h=32, w=64, cout=64, kh=7, kw=7,
                                                                                 stride=2, pad=3)):
        assert L.md2_conv2d_ex_workspace_size(C.byref(d), None) == L.md2_conv2d_workspace_size(C.byref(d))
    assert L.md2_conv2d_ex_workspace_size(None, None) == 0
    assert L.md2_conv2d_ex_workspace_size(C.byref(_desc(stride=3)), None) == 0


@pytest.mark.parametrize("bad", [dict(stride=0), dict(stride=3), dict(kh=5, kw=5), dict(n=0), dict(reflect=1, stride=2)])
def test_bad_shape_is_einval(L, bad):
    for which in ("fwd", "dgrad", "wgrad"):
        rc, msg = _call(L, which, _desc(**bad), None)
        assert rc == MD2_EINVAL and msg, (which, bad)


@pytest.mark.parametrize("null", ["out", "dout", "dpre", "part"])
def test_act_backward_bias_null_pointer_is_einval(L, null):
    keep, p = _dummy()
    a = dict(out=p, dout=C.c_void_p(p.value + 64), dpre=C.c_void_p(p.value + 128), part=C.c_void_p(p.value + 192))
    a[null] = None
    assert L.md2_act_backward_bias(a["out"], a["dout"], a["dpre"], 2, 20, 48, 2, a["part"], None) == MD2_EINVAL
    assert b"act_backward_bias" in L.md2_last_error()


@pytest.mark.parametrize("n,c,hw,act", [(0, 20, 48, 2), (2, 0, 48, 2), (2, 20, 0, 2), (2, 20, 46, 2), (2, 20, 48, 4),
                                        (2, 20, 48, -1), (1 << 10, 1 << 10, 1 << 12, 1)])
def test_act_backward_bias_bad_size_is_einval(L, n, c, hw, act):
    keep, p = _dummy()
    q = C.c_void_p(p.value + 64)
    assert L.md2_act_backward_bias(p, q, q, n, c, hw, act, C.c_void_p(p.value + 128), None) == MD2_EINVAL
    assert b"act_backward_bias" in L.md2_last_error()


def test_act_backward_bias_misaligned_is_einval(L):
    keep, p = _dummy()
    q = C.c_void_p(p.value + 64)
    assert L.md2_act_backward_bias(C.c_void_p(p.value + 4), q, q, 2, 20, 48, 2, q, None) == MD2_EINVAL
    assert b"aligned" in L.md2_last_error()
