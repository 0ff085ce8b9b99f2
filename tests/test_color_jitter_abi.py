"""CPU checks of the colour-jitter entry points (md2_color_jitter, md2_model_*_aug; include/md2.h):
exports, argument validation (which comes before any HIP call, so it runs without a GPU), the Julia
struct / ccalls, the host draws of md2hip.ColorJitter, the x_net plumbing of the Python layer, and the
float32 NumPy restatement of the GPU tests against float64.

The restatement check.  Over all 24 orders at 16 x 24, for c = 3 and 1, including black, white and
grey pixels, float32 differs from float64 by at most 8.7e-7 (seen when the formulas were written
down; 1.2e-6 with the wider factor ranges drawn here); the test allows 4e-6, about 4 x the former."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _color_ref as R
from tests import test_julia_shim as J
from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _c_struct, _jl_ccalls, _jl_struct, _layout

MD2_EINVAL = 1
SYMBOLS = {"md2_color_jitter_workspace_size": 4, "md2_color_jitter": 11, "md2_model_forward_loss_aug": 7,
           "md2_model_train_step_graph_aug": 10}
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    from md2hip._lib import Jitter
    lib = C.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    lib.md2_color_jitter.restype = C.c_int
    lib.md2_color_jitter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Jitter),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.md2_color_jitter_workspace_size.restype = C.c_size_t
    lib.md2_color_jitter_workspace_size.argtypes = [C.c_int] * 4
    lib.md2_last_error.restype = C.c_char_p
    return lib


@pytest.fixture()
def char_sizes(monkeypatch):
    """the shim test's parsers know no one-byte field yet"""
    monkeypatch.setitem(J.C_SIZES, "char", 1)
    monkeypatch.setitem(J.JL_SIZES, "Cuchar", 1)


# ---- exports, prototypes, layouts -----------------------------------------------------------------
def test_library_exports_and_header():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    hdr = open(HDR).read()
    protos = _c_prototypes(hdr)
    from md2hip import _lib
    for s, nargs in SYMBOLS.items():
        assert hasattr(lib, s), s
        assert protos[s] == nargs, s
        assert len(_lib._SIGS[s][1]) == nargs, s
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2      # additive
    assert int(re.search(r"#define MD2_JITTER_MAX_SAMPLES (\d+)", hdr).group(1)) == _lib.JITTER_MAX_SAMPLES == 64


def test_python_struct_matches_header(char_sizes):
    from md2hip import JITTER_DTYPE
    from md2hip._lib import Jitter
    cf = _c_struct(open(HDR).read(), "md2_jitter")
    assert [n for n, _, _ in cf] == [n for n, _ in Jitter._fields_] == list(JITTER_DTYPE.names)
    offs, size = _layout(cf)
    assert offs == [getattr(Jitter, n).offset for n, _ in Jitter._fields_] == [JITTER_DTYPE.fields[n][1] for n in
                                                                             JITTER_DTYPE.names]
    assert size == C.sizeof(Jitter) == JITTER_DTYPE.itemsize == 24


def test_julia_struct_and_ccalls_match_header(char_sizes):
    jl, hdr = open(JL).read(), open(HDR).read()
    cf, jf = _c_struct(hdr, "md2_jitter"), _jl_struct(jl, "Jitter")
    assert [n for n, _, _ in cf] == [n for n, _, _ in jf]
    assert [(s, n) for _, s, n in cf] == [(s, n) for _, s, n in jf], (cf, jf)
    assert _layout(cf) == _layout(jf)
    protos, calls = _c_prototypes(hdr), dict(_jl_ccalls(jl))
    for name in SYMBOLS:
        assert name in calls, f"julia/MD2HIP.jl does not call {name}"
        assert calls[name] == protos[name]
    assert re.search(r"function color_jitter\(x::ROCArray\{Float32,5\}, params::Vector\{Jitter\}", jl)
    assert re.search(r"function train_loss\(m::HIPModel, [^)]*; x_net=nothing\)", jl, re.S)
    assert int(re.search(r"const JITTER_MAX_SAMPLES = (\d+)", jl).group(1)) == 64


# ---- md2_color_jitter refuses, before any HIP call -------------------------------------------------
# (a valid call is never made here: it would launch)
def _dummy(nbytes=4096):
    buf = (C.c_char * (nbytes + 64))()
    return buf, (C.addressof(buf) + 63) // 64 * 64


def _call(L, *, n=2, frames=3, c=3, h=4, w=8, x="x", out="out", params=True, ws="ws", edit=None):
    """One call with everything valid but the overrides; pointers are never dereferenced."""
    from md2hip._lib import Jitter
    keep = {k: _dummy() for k in ("x", "out", "ws")}

    def addr(v):
        return v if v is None or isinstance(v, int) else keep[v][1]
    p = R.params(max(n, 2))
    p["apply"] = 1
    if edit:
        edit(p)
    pp = C.cast(C.c_void_p(p.ctypes.data), C.POINTER(Jitter)) if params else None
    rc = L.md2_color_jitter(addr(x), n, frames, c, h, w, pp, addr(out), None, addr(ws), None)
    return rc, L.md2_last_error().decode()


def _set(field, value, k=1):
    def edit(p):
        p[field][k] = value
    return edit


INVALID = {
    "null_x": dict(x=None), "null_out": dict(out=None), "null_params": dict(params=False), "null_workspace": dict(ws=None),
    "n_zero": dict(n=0), "n_negative": dict(n=-1), "n_65": dict(n=65),
    "frames_zero": dict(frames=0), "h_zero": dict(h=0), "w_zero": dict(w=0), "w_negative": dict(w=-8),
    "c_2": dict(c=2), "c_4": dict(c=4), "c_zero": dict(c=0),
    "hw_too_large": dict(h=4097, w=4096),
    "order_repeats": dict(edit=_set("order", [0, 1, 1, 3])),
    "order_out_of_range": dict(edit=_set("order", [0, 1, 2, 4])),
    "order_255": dict(edit=_set("order", [255, 1, 2, 3], 0)),
    "brightness_nan": dict(edit=_set("brightness", NAN)), "contrast_inf": dict(edit=_set("contrast", INF)),
    "saturation_nan": dict(edit=_set("saturation", NAN, 0)), "hue_nan": dict(edit=_set("hue", NAN)),
    "hue_minus_inf": dict(edit=_set("hue", -INF)),
    "brightness_negative": dict(edit=_set("brightness", -0.1)), "contrast_negative": dict(edit=_set("contrast", -1e-6)),
    "saturation_negative": dict(edit=_set("saturation", -2.0, 0)),
    "hue_above_half": dict(edit=_set("hue", 0.5001)), "hue_below_minus_half": dict(edit=_set("hue", -0.51)),
    "apply_2": dict(edit=_set("apply", 2)), "apply_negative": dict(edit=_set("apply", -1, 0)),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_color_jitter_refuses(L, case):
    rc, msg = _call(L, **INVALID[case])
    assert rc == MD2_EINVAL, (case, rc, msg)
    assert msg.startswith("invalid argument: color_jitter"), msg


def test_color_jitter_refuses_an_invalid_record_even_when_not_applied(L):
    def edit(p):
        p["apply"][1] = 0
        p["hue"][1] = 0.75
    assert _call(L, edit=edit)[0] == MD2_EINVAL


@pytest.mark.parametrize("shift", [4, 2 * 3 * 3 * 4 * 8 * 4 - 4, -4])
def test_color_jitter_refuses_partial_aliasing(L, shift):
    """out overlapping x without being x (the batch is 2*3*3*4*8 floats)"""
    buf, base = _dummy(8192)
    rc, msg = _call(L, x=base + 2048, out=base + 2048 + shift)
    assert rc == MD2_EINVAL and "overlaps" in msg, (rc, msg)


def test_workspace_size(L):
    ws = L.md2_color_jitter_workspace_size
    assert ws(12, 3, 128, 416) == 8 * 12 * 3 * 52          # one fp64 partial per block of 1024 pixels
    assert ws(1, 1, 7, 13) == 8 and ws(3, 3, 64, 128) == 8 * 9 * 8
    assert ws(2, 1, 4096, 4096) == 8 * 2 * 64              # at most 64 blocks per frame
    for bad in ((0, 3, 8, 8), (65, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (1, 3, 4097, 4096)):
        assert ws(*bad) == 0, bad


# ---- ColorJitter.draw ------------------------------------------------------------------------------
def test_draw_is_reproducible_and_per_sample():
    import md2hip
    cj = md2hip.ColorJitter()
    a, b = cj.draw(list(range(40)), 7), cj.draw(list(range(40)), 7)
    assert a.dtype == md2hip.JITTER_DTYPE and a.tobytes() == b.tobytes()
    # a sample's draw depends on (seed, index) alone, not on its place in the batch
    c = cj.draw([31, 5], 7)
    assert c[0].tobytes() == a[31].tobytes() and c[1].tobytes() == a[5].tobytes()
    assert cj.draw(list(range(40)), 8).tobytes() != a.tobytes()


def test_draw_ranges_and_apply_rate():
    import md2hip
    cj = md2hip.ColorJitter()
    p = cj.draw(list(range(10000)), 3)
    for name, (lo, hi) in (("brightness", (0.8, 1.2)), ("contrast", (0.8, 1.2)), ("saturation", (0.8, 1.2)),
                           ("hue", (-0.1, 0.1))):
        v = p[name]
        assert np.float32(lo) <= v.min() and v.max() <= np.float32(hi), name
        assert v.min() < lo + 0.01 * (hi - lo) and v.max() > hi - 0.01 * (hi - lo), name     # the range is used
        assert abs(v.mean() - 0.5 * (lo + hi)) < 0.02 * (hi - lo), name    # 5.8 sigma of a uniform mean at 10^4
    assert set(map(tuple, p["order"].tolist())) == set(R.ORDERS)          # every order occurs, all are permutations
    assert set(np.unique(p["apply"]).tolist()) == {0, 1}
    assert abs(p["apply"].mean() - 0.5) < 0.025                            # 5 sigma of a fair coin at 10^4
    assert md2hip.ColorJitter(p=0.0).draw(range(50), 1)["apply"].sum() == 0
    assert md2hip.ColorJitter(p=1.0).draw(range(50), 1)["apply"].sum() == 50
    q = md2hip.ColorJitter(brightness=(0.5, 0.5), hue=(0.5, 0.5)).draw(range(5), 1)
    assert (q["brightness"] == 0.5).all() and (q["hue"] == 0.5).all()
    with pytest.raises(ValueError):
        md2hip.ColorJitter(hue=(-0.6, 0.1))
    with pytest.raises(ValueError):
        md2hip.ColorJitter(contrast=(-0.1, 1.0))


def test_draw_leaves_the_flip_coins_alone():
    import md2hip
    from md2hip.data import _Dataset
    ds = _Dataset()
    ds.augmentations = md2hip.FlipX(0.5)
    idx = list(range(200))
    before = ds._native_flips(idx, 11)
    cj = md2hip.ColorJitter()
    drawn = cj.draw(idx, 11)
    after = ds._native_flips(idx, 11)
    assert before.tobytes() == after.tobytes() and 60 < before.sum() < 140
    # and they are the coins of default_rng((seed, i)), which the jitter's stream (seed, i, 1) is not
    assert before.tolist() == [int(np.random.default_rng((11, i)).random() < 0.5) for i in idx]
    assert drawn["apply"].tolist() != before.tolist()


# ---- the Python layer: x_net=None calls the old symbols ------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def _executor(monkeypatch):
    import md2hip.model as M
    fake = _FakeLib()
    monkeypatch.setattr(M, "lib", lambda: fake)
    monkeypatch.setattr(M, "stream_of", lambda device=None: "stream")
    monkeypatch.setattr(M, "ptr", lambda t: None if t is None else ("ptr", id(t)))

    class _M:
        version = 0
        device = "cpu"

        def _require_train(self, what):
            pass

        def touch(self):
            pass

    ex = object.__new__(M._Executor)
    ex.model, ex.handle, ex.automask, ex.forwarded, ex.pending, ex.version = _M(), None, True, False, False, 0
    ex.sync = lambda: None
    ex._trained = lambda: None
    return ex, fake


def test_forward_loss_plumbs_x_net(monkeypatch):
    import torch
    ex, fake = _executor(monkeypatch)
    x, xn, am = torch.zeros(1, 3, 3, 4, 8), torch.ones(1, 3, 3, 4, 8), torch.zeros(1, 4, 8)
    loss = torch.zeros(1)
    ex.forward_loss(x, am, loss)
    ex.forward_loss(x, am, loss, x_net=xn)
    (n0, a0), (n1, a1) = fake.calls
    assert n0 == "md2_model_forward_loss" and len(a0) == 6 and a0[1] == ("ptr", id(x))
    assert n1 == "md2_model_forward_loss_aug" and len(a1) == 7
    assert a1[1] == ("ptr", id(x)) and a1[2] == ("ptr", id(xn)) and a1[4] == ("ptr", id(loss)) and a1[6] == "stream"
    with pytest.raises(ValueError):
        ex.forward_loss(x, am, loss, x_net=torch.ones(1, 3, 3, 4, 4))
    with pytest.raises(ValueError):
        ex.forward_loss(x, am, loss, x_net=xn.double())


def test_train_step_graph_plumbs_x_net(monkeypatch):
    import torch
    import md2hip
    ex, fake = _executor(monkeypatch)
    x, xn = torch.zeros(1, 3, 3, 4, 8), torch.ones(1, 3, 3, 4, 8)
    opt = md2hip.ADAM(1e-4)
    opt.m, opt.v = torch.zeros(4), torch.zeros(4)
    ex.train_step_graph(x, opt)
    ex.train_step_graph(x, opt, x_net=xn)
    (n0, a0), (n1, a1) = fake.calls
    assert n0 == "md2_model_train_step_graph" and len(a0) == 9 and a0[6] == 1
    assert n1 == "md2_model_train_step_graph_aug" and len(a1) == 10
    assert a1[1] == ("ptr", id(x)) and a1[2] == ("ptr", id(xn)) and a1[3] is None and a1[7] == 2


def test_train_loss_and_train_step_take_x_net():
    import inspect
    import md2hip
    for fn in (md2hip.train_loss, md2hip.train_step, md2hip.model._Executor.forward_loss,
               md2hip.model._Executor.train_step_graph):
        assert inspect.signature(fn).parameters["x_net"].default is None, fn
    assert inspect.signature(md2hip.DataLoader.__init__).parameters["color_jitter"].default is None
    assert callable(md2hip.color_jitter) and md2hip.ColorJitter().p == 0.5


# ---- the float32 restatement against float64 -------------------------------------------------------
@pytest.fixture(scope="module")
def all_orders():
    """24 samples, one per order, two frames, at 16 x 24: (c, x, params, out32, means32, out64, means64)"""
    res = {}
    for c in (3, 1):
        x = R.test_images(24, 2, c, 16, 24, seed=c)
        p = R.params(24)
        rng = np.random.default_rng(5)
        p["apply"] = 1
        p["order"] = np.array(R.ORDERS, dtype=np.uint8)
        p["brightness"], p["contrast"], p["saturation"] = (rng.uniform(0.6, 1.4, 24) for _ in range(3))
        p["hue"] = rng.uniform(-0.5, 0.5, 24)
        res[c] = (x, p) + R.color_jitter(x, p, np.float32) + R.color_jitter(x, p, np.float64)
    return res


@pytest.mark.parametrize("c", [3, 1])
def test_restatement_float32_against_float64(all_orders, c):
    x, p, o32, m32, o64, m64 = all_orders[c]
    assert o32.dtype == np.float32 and o64.dtype == np.float64
    assert np.isfinite(o32).all() and o32.min() >= 0.0 and o32.max() <= 1.0
    err = np.abs(o32.astype(np.float64) - o64).max()
    print(f"c={c}: max |float32 - float64| = {err:.3g}, means {np.abs(m32 - m64).max():.3g}")
    assert err <= 4e-6
    assert np.abs(m32.astype(np.float64) - m64).max() <= 4e-6
    assert not np.array_equal(o32, x)


def test_restatement_apply_zero_is_the_identity():
    x = R.test_images(3, 2, 3, 8, 12)
    p = R.params(3)
    p["brightness"], p["hue"], p["order"] = 0.3, 0.4, [3, 2, 1, 0]
    out, means = R.color_jitter(x, p)
    assert out.tobytes() == x.tobytes() and not means.any()


def test_restatement_one_channel_ignores_saturation_and_hue():
    x = R.test_images(2, 2, 1, 8, 12)
    a, b = R.params(2), R.params(2)
    for q in (a, b):
        q["apply"], q["brightness"], q["contrast"], q["order"] = 1, 1.1, 0.7, [[2, 0, 3, 1], [3, 1, 2, 0]]
    b["saturation"], b["hue"] = 0.2, -0.45
    oa, ma = R.color_jitter(x, a)
    ob, mb = R.color_jitter(x, b)
    assert oa.tobytes() == ob.tobytes() and ma.tobytes() == mb.tobytes() and not np.array_equal(oa, x)


def test_restatement_imposed_mean_is_used():
    x = R.test_images(1, 1, 3, 8, 12)
    p = R.params(1)
    p["apply"], p["contrast"] = 1, 0.5
    own, m = R.color_jitter(x, p)
    same, _ = R.color_jitter(x, p, means=m)
    other, m2 = R.color_jitter(x, p, means=np.full((1, 1), 0.9, np.float32))
    assert own.tobytes() == same.tobytes() and not np.array_equal(own, other) and m2[0, 0] == np.float32(0.9)
