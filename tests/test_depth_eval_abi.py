"""CPU checks of the depth-evaluation entry points (md2_depth_eval, include/md2.h): exports,
argument validation (which comes before any HIP call, so it runs without a GPU), the Python
wrappers' own checks and the Julia struct / ccall."""
import ctypes as C
import os
import re

import pytest

from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _c_struct, _jl_ccalls, _jl_struct, _layout

MD2_EINVAL = 1

VALID = dict(n=2, h=32, w=104, gt_h=93, gt_w=310, y0=37, y1=92, x0=11, x1=298, min_depth=0.1, max_depth=100.0,
             eval_min=1e-3, eval_max=80.0, median_scaling=1, scale=1.0)

INVALID = {
    "n_zero": dict(n=0),
    "n_negative": dict(n=-3),
    "h_zero": dict(h=0),
    "w_zero": dict(w=0),
    "gt_h_zero": dict(gt_h=0, y0=0, y1=0),
    "gt_w_zero": dict(gt_w=0, x0=0, x1=0),
    "gt_too_large": dict(gt_h=4097, gt_w=4096, y0=0, y1=4097, x0=0, x1=4096),
    "crop_empty_rows": dict(y0=50, y1=50),
    "crop_empty_cols": dict(x0=120, x1=100),
    "crop_negative": dict(y0=-1),
    "crop_past_bottom": dict(y1=94),
    "crop_past_right": dict(x1=311),
    "depth_range_equal": dict(min_depth=1.0, max_depth=1.0),
    "depth_range_reversed": dict(min_depth=100.0, max_depth=0.1),
    "min_depth_zero": dict(min_depth=0.0),
    "eval_range_equal": dict(eval_min=80.0, eval_max=80.0),
    "eval_range_reversed": dict(eval_min=80.0, eval_max=1e-3),
    "eval_min_zero": dict(eval_min=0.0),
    "eval_min_negative": dict(eval_min=-1.0),
    "scale_zero": dict(median_scaling=0, scale=0.0),
    "scale_negative": dict(median_scaling=0, scale=-2.0),
    "scale_inf": dict(median_scaling=0, scale=float("inf")),
    "scale_nan": dict(median_scaling=0, scale=float("nan")),
}


@pytest.fixture(scope="module")
def L():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    from md2hip._lib import DepthEvalCfg
    lib = C.CDLL(LIB)
    assert hasattr(lib, "md2_depth_eval") and hasattr(lib, "md2_depth_eval_workspace_size")
    lib.md2_depth_eval_workspace_size.restype = C.c_size_t
    lib.md2_depth_eval_workspace_size.argtypes = [C.POINTER(DepthEvalCfg)]
    lib.md2_depth_eval.restype = C.c_int
    lib.md2_depth_eval.argtypes = [C.POINTER(DepthEvalCfg)] + [C.c_void_p] * 6
    lib.md2_last_error.restype = C.c_char_p
    return lib


def _cfg(**over):
    from md2hip._lib import DepthEvalCfg
    return DepthEvalCfg(**{**VALID, **over})


def test_library_exports_depth_eval():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    assert hasattr(lib, "md2_depth_eval")
    assert hasattr(lib, "md2_depth_eval_workspace_size")
    hdr = open(HDR).read()
    assert "md2_depth_eval" in _c_prototypes(hdr) and "md2_depth_eval_workspace_size" in _c_prototypes(hdr)
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2      # additive


def test_python_struct_matches_header():
    from md2hip._lib import DepthEvalCfg
    cf = _c_struct(open(HDR).read(), "md2_depth_eval_cfg")
    assert [n for n, _, _ in cf] == [n for n, _ in DepthEvalCfg._fields_]
    offs, size = _layout(cf)
    assert offs == [getattr(DepthEvalCfg, n).offset for n, _ in DepthEvalCfg._fields_]
    assert size == C.sizeof(DepthEvalCfg)


def test_workspace_size(L):
    small = L.md2_depth_eval_workspace_size(C.byref(_cfg()))
    assert small > 0
    kitti = L.md2_depth_eval_workspace_size(C.byref(_cfg(n=12, h=128, w=416, gt_h=375, gt_w=1242, y0=153,
                                                         y1=371, x0=44, x1=1197)))
    assert small < kitti < 8 << 20
    assert L.md2_depth_eval_workspace_size(None) == 0
    for name, over in INVALID.items():
        assert L.md2_depth_eval_workspace_size(C.byref(_cfg(**over))) == 0, name


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_cfg_is_einval(L, name):
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)           # dummy non-null pointers: validation must come first
    # a valid call is never made here (it would launch); an invalid one must not reach HIP
    rc = L.md2_depth_eval(C.byref(_cfg(**INVALID[name])), p, p, p, p, p, None)
    assert rc == MD2_EINVAL
    msg = L.md2_last_error()
    assert msg and b"depth_eval" in msg, msg


@pytest.mark.parametrize("which", range(6))
def test_null_pointer_is_einval(L, which):
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    args = [C.byref(_cfg()), p, p, p, p, p]
    args[which] = None
    assert L.md2_depth_eval(*args, None) == MD2_EINVAL
    assert L.md2_last_error()


def test_garg_crop_known_answers():
    import md2hip
    assert md2hip.garg_crop(375, 1242) == (153, 371, 44, 1197)
    assert md2hip.garg_crop(93, 310) == (37, 92, 11, 298)
    assert md2hip.evaluate.METRIC_NAMES == ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "ratio",
                                            "med_gt", "med_pred")
    assert len(md2hip.METRIC_NAMES) == 10


def test_depth_errors_rejects_bad_tensors(monkeypatch):
    """ValueError before any library call: the library is made unreachable for the test."""
    import torch
    import md2hip
    from md2hip import evaluate

    def no_lib():
        raise AssertionError("depth_errors reached the library")
    monkeypatch.setattr(evaluate, "lib", no_lib)
    d, g = torch.zeros(2, 1, 8, 16), torch.zeros(2, 8, 16)
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.depth_errors(d, g)                                   # CPU tensors
    with pytest.raises(ValueError, match="float32 CUDA"):
        md2hip.depth_errors(d.double(), g.double())                 # float64
    with pytest.raises(ValueError, match="gt must be"):
        md2hip.depth_errors(d, g[0])                                # rank-2 gt
    with pytest.raises(ValueError, match="batch mismatch"):
        md2hip.depth_errors(d, torch.zeros(3, 8, 16))               # batch mismatch
    with pytest.raises(ValueError, match="disp must be"):
        md2hip.depth_errors(torch.zeros(2, 3, 8, 16), g)            # disp with 3 channels


def test_julia_struct_matches_header():
    jl, hdr = open(JL).read(), open(HDR).read()
    cf, jf = _c_struct(hdr, "md2_depth_eval_cfg"), _jl_struct(jl, "DepthEvalCfg")
    assert [n for n, _, _ in cf] == [n for n, _, _ in jf]
    assert [(s, n) for _, s, n in cf] == [(s, n) for _, s, n in jf], (cf, jf)
    assert _layout(cf) == _layout(jf)


def test_julia_ccall_names_declared_symbols():
    jl, hdr = open(JL).read(), open(HDR).read()
    protos = _c_prototypes(hdr)
    calls = dict(_jl_ccalls(jl))
    lib = C.CDLL(LIB) if os.path.exists(LIB) else None
    for name in ("md2_depth_eval", "md2_depth_eval_workspace_size"):
        assert name in calls, f"julia/MD2HIP.jl does not call {name}"
        assert calls[name] == protos[name]
        if lib is not None:
            assert hasattr(lib, name)
    assert re.search(r"function depth_errors\(disp::ROCArray\{Float32", jl)
