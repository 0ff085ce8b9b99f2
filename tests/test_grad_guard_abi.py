"""CPU checks of the gradient guard (md2_grad_norm, md2_adam_guarded, md2_model_set_grad_guard,
md2_model_grad_guard_state; include/md2.h): exports and signatures in the header, the ctypes table
and the Julia shim, argument validation (which comes before any HIP call, so it runs without a GPU),
and the NumPy restatement (tests/_grad_guard_ref.py) against the plain answer.

Bound.  The restated order is a tree over at most 2^31 non-negative float64 terms: every partial sum
is at most the total, so each of the at most ~8200 additions on an element's path (8192 per thread,
6 + 2 in the block, 4 + 6 + 2 in the finish) errs by at most 2^-53 of the total -- a relative error
below 8210 x 2^-53 < 2^-40 in the worst case and, on the sizes here (at most 16 additions per thread,
34 on a path), below 34 x 2^-53 < 2^-47.  BOUND = 2^-45 is asserted; a restatement that misses it is
wrong."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import _grad_guard_ref as R
from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _jl_ccalls

MD2_EINVAL = 1
SYMBOLS = {"md2_grad_norm_workspace_size": 1, "md2_grad_norm": 7, "md2_adam_guarded": 12,
           "md2_model_set_grad_guard": 3, "md2_model_grad_guard_state": 2}
BOUND = 2.0 ** -45
SIZES = [1, 255, 4097, 2 ** 20 + 5]


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
    # the state block: the header's field order is the ctypes structure's and the restatement's
    body = re.search(r"typedef struct md2_guard_state \{(.*?)\} md2_guard_state;", hdr, re.S).group(1)
    fields = re.findall(r"(double|long long|float|int)\s+(\w+);", body)
    ctype = {"double": C.c_double, "long long": C.c_longlong, "float": C.c_float, "int": C.c_int}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.GuardState._fields_)
    assert C.sizeof(_lib.GuardState) == R.STATE_DTYPE.itemsize == 40
    assert [n for _, n in fields] == list(R.STATE_DTYPE.names)
    for n in R.STATE_DTYPE.names:
        assert getattr(_lib.GuardState, n).offset == R.STATE_DTYPE.fields[n][1], n


def test_workspace_size():
    lib = C.CDLL(LIB)
    f = lib.md2_grad_norm_workspace_size
    f.restype, f.argtypes = C.c_size_t, [C.c_longlong]
    for n in (0, -1, -2 ** 40, 2 ** 31 + 1, 2 ** 62):
        assert f(n) == 0, n
    for n in (1, 255, 4096, 4097, 2 ** 20 + 5, 4 * 2 ** 20 + 3, 2 ** 31):
        assert f(n) == R.workspace_bytes(n) > 0, n
    assert f(2 ** 31) == f(4 * 2 ** 20) == 16 * 1024       # the grid stops growing at 1024 blocks


def test_python_api_is_exported():
    import inspect
    import md2hip
    for name in ("grad_norm", "decode_guard_state"):
        assert callable(getattr(md2hip, name)), name
    sig = inspect.signature(md2hip.ADAM.__init__).parameters
    assert sig["max_grad_norm"].default is None and sig["skip_nonfinite"].default is False
    assert not md2hip.ADAM(1e-3).guarded
    assert md2hip.ADAM(1e-3, skip_nonfinite=True).guarded and md2hip.ADAM(1e-3, max_grad_norm=2.0).guarded
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            md2hip.ADAM(1e-3, max_grad_norm=bad)
    for name in ("guard_state", "guard_tensor"):
        assert callable(getattr(md2hip.ADAM, name)), name
    assert "SYNCHRONISES" in md2hip.ADAM.guard_state.__doc__


def test_julia_ccalls_match_header():
    jl, hdr = open(JL).read(), open(HDR).read()
    protos = _c_prototypes(hdr)
    calls = dict(_jl_ccalls(jl))
    for name in ("md2_model_set_grad_guard", "md2_model_grad_guard_state"):
        assert name in calls, f"julia/MD2HIP.jl does not call {name}"
        assert calls[name] == protos[name]
    assert re.search(r"function set_grad_guard\(m::HIPModel", jl)
    assert re.search(r"function grad_guard_state\(m::HIPModel", jl)


# ---- md2_grad_norm refuses, before any HIP call -----------------------------------------------------
# (a valid call is never made here: it would launch)
@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    lib.md2_grad_norm.restype = C.c_int
    lib.md2_grad_norm.argtypes = [C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                  C.c_void_p]
    lib.md2_adam_guarded.restype = C.c_int
    lib.md2_adam_guarded.argtypes = [C.c_void_p] * 4 + [C.c_longlong] + [C.c_float] * 4 + [C.c_int, C.c_void_p,
                                                                                         C.c_void_p]
    lib.md2_model_set_grad_guard.restype = C.c_int
    lib.md2_model_set_grad_guard.argtypes = [C.c_void_p, C.c_int, C.c_float]
    lib.md2_model_grad_guard_state.restype = C.c_int
    lib.md2_model_grad_guard_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.md2_last_error.restype = C.c_char_p
    return lib


INVALID = {
    "null_g": dict(null="g"),
    "null_state": dict(null="state"),
    "null_workspace": dict(null="workspace"),
    "n_0": dict(n=0),
    "n_negative": dict(n=-7),
    "n_past_2_31": dict(n=2 ** 31 + 1),
    "max_norm_nan": dict(max_norm=float("nan")),
    "max_norm_0": dict(max_norm=0.0),
    "max_norm_negative": dict(max_norm=-1.0),
    "max_norm_minus_inf": dict(max_norm=-math.inf),
    "grad_scale_0": dict(grad_scale=0.0),
    "grad_scale_negative": dict(grad_scale=-0.5),
    "grad_scale_inf": dict(grad_scale=math.inf),
    "grad_scale_nan": dict(grad_scale=float("nan")),
    "workspace_misaligned_4": dict(ws_off=4),
    "workspace_misaligned_1": dict(ws_off=1),
}


def _call(L, *, n=1000, grad_scale=1.0, max_norm=math.inf, null=None, ws_off=0):
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) & ~15              # never dereferenced: validation comes first
    a = dict(g=base, state=base + 64, workspace=base + 128 + ws_off)
    if null:
        a[null] = None
    return L.md2_grad_norm(a["g"], n, grad_scale, max_norm, a["state"], a["workspace"], None)


@pytest.mark.parametrize("name", sorted(INVALID))
def test_grad_norm_invalid_is_einval(L, name):
    assert _call(L, **INVALID[name]) == MD2_EINVAL, name
    msg = L.md2_last_error()
    assert msg.startswith(b"invalid argument: grad_norm"), msg


def test_other_entries_refuse_null(L):
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert L.md2_adam_guarded(*args, 10, 1e-3, 0.9, 0.999, 1e-8, 1, p, None) == MD2_EINVAL
    assert L.md2_adam_guarded(p, p, p, p, 10, 1e-3, 0.9, 0.999, 1e-8, 1, None, None) == MD2_EINVAL
    assert L.md2_adam_guarded(p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 1, p, None) == MD2_EINVAL
    assert L.md2_adam_guarded(p, p, p, p, 10, 1e-3, 0.9, 0.999, 1e-8, 0, p, None) == MD2_EINVAL
    assert L.md2_model_set_grad_guard(None, 1, 1.0) == MD2_EINVAL
    assert L.md2_model_grad_guard_state(None, p) == MD2_EINVAL


# ---- the restatement ----------------------------------------------------------------------------------
def _vector(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_restated_order_against_fsum(n):
    g = _vector(n, n)
    S, c = R.sumsq_ordered(g)
    T, c0 = R.sumsq_plain(g)
    assert c == c0 == 0 and T > 0
    rel = abs(float(S) - T) / T
    print(f"n = {n}: ordered {float(S)!r}, fsum {T!r}, relative error {rel:.3e}")
    assert rel <= BOUND, (n, rel)


def test_restated_nonfinite_entries_add_nothing():
    g = _vector(4097, 7)
    clean = R.sumsq_ordered(g)
    for k, bad in ((0, np.nan), (255, np.inf), (4096, -np.inf)):
        g[k] = bad
    h = g.copy()
    h[[0, 255, 4096]] = 0.0
    S, c = R.sumsq_ordered(g)
    assert c == 3 and S == R.sumsq_ordered(h)[0] and S < clean[0]
    st = R.finish(S, c, 1.0, 1.0, skipped=4)
    assert int(st["ok"]) == 0 and int(st["skipped"]) == 5 and float(st["coef"]) == 1.0 and int(st["nonfinite"]) == 3


def test_restated_finish():
    st = R.finish(np.float64(16.0), 0, 0.5, math.inf)
    assert float(st["norm"]) == 2.0 and float(st["coef"]) == 1.0 and float(st["gscale"]) == 0.5 and int(st["ok"]) == 1
    st = R.finish(np.float64(16.0), 0, 1.0, 4.0)             # exactly the norm: `>` takes no clip
    assert float(st["coef"]) == 1.0
    st = R.finish(np.float64(16.0), 0, 1.0, 2.0)
    assert float(st["coef"]) == 0.5 and float(st["gscale"]) == 0.5
    st = R.finish(np.float64(0.0), 0, 1.0, 1.0)              # all zeros
    assert float(st["norm"]) == 0.0 and float(st["coef"]) == 1.0 and int(st["ok"]) == 1
    # not torch's max_norm / (norm + 1e-6)
    st = R.finish(np.float64(9.0), 0, 1.0, 1.5)
    assert st["coef"] == np.float32(1.5) / np.float32(3.0) != np.float32(1.5 / (3.0 + 1e-6))


@pytest.mark.parametrize("n", [1, 1000])
def test_guarded_update_equals_plain_update_without_clipping(n):
    rng = np.random.default_rng(n)
    p, g, m, v = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    for gs in (1.0, 0.25, 1.0 / 3.0):
        st = R.grad_norm(g, gs, math.inf)
        assert int(st["ok"]) == 1 and st["gscale"].tobytes() == np.float32(gs).tobytes()
        a = R.adam_guarded(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 3, st)
        b = R.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 3, gs)
        for x, y in zip(a, b):
            assert x.dtype == np.float32 and x.tobytes() == y.tobytes()
    g2 = g.copy()
    g2[n // 2] = np.inf
    a = R.adam_guarded(p, g2, m, v, 1e-3, 0.9, 0.999, 1e-8, 3, R.grad_norm(g2))
    for x, y in zip(a, (p, m, v)):
        assert x.tobytes() == y.tobytes()
