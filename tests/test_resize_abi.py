"""CPU checks of the frame-resize entry points (md2_resize_frames, md2_load_frames_native_u8,
include/md2.h): exports, prototypes and the struct layout in the header, the Python binding and the
Julia shim; every refusal of md2_resize_frames (validation comes before any HIP call, so it runs
without a GPU); the Python wrapper's own checks; and the native-size PNG decoder against PIL."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_julia_shim import HDR, JL, LIB, _c_prototypes, _c_struct, _jl_ccalls, _jl_struct, _layout

MD2_EINVAL = 1
SYMBOLS = ("md2_resize_frames", "md2_load_frames_native_u8")

# name -> (cfg overrides, offsets, src_w, src_h): every one must be refused
INVALID = {
    "m_zero": (dict(m=0), None, None, None),
    "m_negative": (dict(m=-1), None, None, None),
    "m_65": (dict(m=65), [0] * 65, [8] * 65, [8] * 65),
    "c_2": (dict(c=2), None, None, None),
    "c_4": (dict(c=4), None, None, None),
    "c_zero": (dict(c=0), None, None, None),
    "out_h_zero": (dict(out_h=0), None, None, None),
    "out_w_zero": (dict(out_w=0), None, None, None),
    "out_h_8193": (dict(out_h=8193), None, None, None),
    "out_w_8193": (dict(out_w=8193), None, None, None),
    "src_w_zero": ({}, None, [8, 0], None),
    "src_h_zero": ({}, None, None, [0, 8]),
    "src_w_8193": (dict(out_w=8192), None, [8, 8193], None),
    "src_h_8193": (dict(out_h=8192), None, None, [8193, 8]),
    "filter_2": (dict(filter=2), None, None, None),
    "filter_negative": (dict(filter=-1), None, None, None),
    "quantize_2": (dict(quantize=2), None, None, None),
    "offset_negative": ({}, [0, -1], None, None),
    "offset0_negative": ({}, [-5, 100], None, None),
    "reduction_w": (dict(out_w=4), None, [64, 65], None),          # 65 > 16 * 4
    "reduction_h": (dict(out_h=2), None, None, [33, 8]),           # 33 > 16 * 2
    "reduction_w_imresize": (dict(out_w=4, filter=0), None, [65, 8], None),
}


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


def _dummy():
    """A non-null, 16-byte aligned pointer that is never dereferenced (validation comes first)."""
    buf = (C.c_char * 256)()
    a = C.addressof(buf)
    return buf, C.c_void_p((a + 15) // 16 * 16)


def _args(over=None, offsets=None, src_w=None, src_h=None):
    from md2hip._lib import ResizeCfg
    cfg = ResizeCfg(**{**dict(m=2, c=3, out_h=8, out_w=12, filter=1, quantize=1), **(over or {})})
    offsets = [1, 4001] if offsets is None else offsets
    src_w = [53, 52] if src_w is None else src_w
    src_h = [37, 36] if src_h is None else src_h
    return (cfg, (C.c_longlong * len(offsets))(*offsets), (C.c_int * len(src_w))(*src_w),
            (C.c_int * len(src_h))(*src_h))


# ---- exports, prototypes, layouts -----------------------------------------------------------------
def test_library_exports_and_header():
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = C.CDLL(LIB)
    hdr = open(HDR).read()
    protos = _c_prototypes(hdr)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in protos, s
    assert protos["md2_resize_frames"] == 9 and protos["md2_load_frames_native_u8"] == 8
    assert int(re.search(r"#define MD2_ABI_VERSION (\d+)", hdr).group(1)) == 2      # additive
    assert int(re.search(r"#define MD2_RESIZE_MAX_IMAGES (\d+)", hdr).group(1)) == 64
    assert re.search(r"enum \{ MD2_RESIZE_IMRESIZE = 0, MD2_RESIZE_ANTIALIAS = 1 \};", hdr)
    from md2hip import _lib
    assert _lib.ABI_VERSION == 2
    assert _lib.RESIZE_MAX_IMAGES == 64
    assert _lib.RESIZE_FILTERS == {"imresize": 0, "antialias": 1}
    assert len(_lib._SIGS["md2_resize_frames"][1]) == 9
    assert len(_lib._SIGS["md2_load_frames_native_u8"][1]) == 8
    lib.md2_abi_version.restype = C.c_int
    assert lib.md2_abi_version() == 2


def test_python_struct_matches_header():
    from md2hip._lib import ResizeCfg
    cf = _c_struct(open(HDR).read(), "md2_resize_cfg")
    assert [n for n, _, _ in cf] == [n for n, _ in ResizeCfg._fields_]
    offs, size = _layout(cf)
    assert offs == [getattr(ResizeCfg, n).offset for n, _ in ResizeCfg._fields_]
    assert size == C.sizeof(ResizeCfg) == 24


def test_julia_struct_matches_header():
    jl, hdr = open(JL).read(), open(HDR).read()
    cf, jf = _c_struct(hdr, "md2_resize_cfg"), _jl_struct(jl, "ResizeCfg")
    assert [n for n, _, _ in cf] == [n for n, _, _ in jf]
    assert [(s, n) for _, s, n in cf] == [(s, n) for _, s, n in jf], (cf, jf)
    assert _layout(cf) == _layout(jf)


def test_julia_ccalls_match_header():
    jl, hdr = open(JL).read(), open(HDR).read()
    protos = _c_prototypes(hdr)
    calls = dict(_jl_ccalls(jl))
    assert "md2_resize_frames" in calls, "julia/MD2HIP.jl does not call md2_resize_frames"
    assert calls["md2_resize_frames"] == protos["md2_resize_frames"]
    assert re.search(r"function resize_frames\(src::ROCVector\{UInt8\}, offsets::Vector\{Int64\}, "
                     r"src_w::Vector\{Int32\}, src_h::Vector\{Int32\}, h, w;", jl)
    assert int(re.search(r"const RESIZE_MAX_IMAGES = (\d+)", jl).group(1)) == 64
    assert re.search(r"const RESIZE_IMRESIZE = 0", jl) and re.search(r"const RESIZE_ANTIALIAS = 1", jl)


# ---- md2_resize_frames refuses, before any HIP call -------------------------------------------------
# (a valid call is never made here: it would launch)
@pytest.mark.parametrize("name", sorted(INVALID))
def test_resize_invalid_is_einval(L, name):
    cfg, off, sw, sh = _args(*INVALID[name])
    keep, p = _dummy()
    rc = L.md2_resize_frames(C.byref(cfg), p, off, sw, sh, None, p, p, None)
    assert rc == MD2_EINVAL, name
    msg = L.md2_last_error()
    assert msg and b"resize_frames" in msg, msg


@pytest.mark.parametrize("which", ["cfg", "src", "offsets", "src_w", "src_h", "out"])
def test_resize_null_pointer_is_einval(L, which):
    cfg, off, sw, sh = _args()
    keep, p = _dummy()
    a = dict(cfg=C.byref(cfg), src=p, offsets=off, src_w=sw, src_h=sh, out=p)
    a[which] = None
    rc = L.md2_resize_frames(a["cfg"], a["src"], a["offsets"], a["src_w"], a["src_h"], None, a["out"], None, None)
    assert rc == MD2_EINVAL
    assert b"resize_frames" in L.md2_last_error()


def test_resize_out_u8_without_quantize_is_einval(L):
    cfg, off, sw, sh = _args(dict(quantize=0))
    keep, p = _dummy()
    assert L.md2_resize_frames(C.byref(cfg), p, off, sw, sh, None, p, p, None) == MD2_EINVAL
    msg = L.md2_last_error()
    assert b"resize_frames" in msg and b"quantize" in msg


@pytest.mark.parametrize("shift", [4, 8, 1])
def test_resize_misaligned_out_is_einval(L, shift):
    cfg, off, sw, sh = _args()
    keep, p = _dummy()
    rc = L.md2_resize_frames(C.byref(cfg), p, off, sw, sh, None, C.c_void_p(p.value + shift), None, None)
    assert rc == MD2_EINVAL
    msg = L.md2_last_error()
    assert b"resize_frames" in msg and b"aligned" in msg


# ---- the Python wrapper refuses bad arguments before the library ------------------------------------
def _no_lib():
    raise AssertionError("the wrapper reached the library")


def test_resize_frames_rejects_bad_arguments(monkeypatch):
    import torch
    import md2hip
    from md2hip import resize
    monkeypatch.setattr(resize, "lib", _no_lib)
    cpu = torch.zeros(4000, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 CUDA"):
        md2hip.resize_frames(cpu, [0], [(8, 8)], 4, 4, channels=1)                     # CPU tensor
    with pytest.raises(ValueError, match="uint8 CUDA"):
        md2hip.resize_frames(cpu.float(), [0], [(8, 8)], 4, 4, channels=1)
    with pytest.raises(ValueError, match="uint8 CUDA"):
        md2hip.resize_frames(cpu.numpy(), [0], [(8, 8)], 4, 4, channels=1)


def test_resize_frames_rejects_bad_host_arguments(monkeypatch):
    """The host-argument checks follow the tensor check: reached here through a stand-in tensor."""
    import torch
    import md2hip
    from md2hip import resize
    monkeypatch.setattr(resize, "lib", _no_lib)

    class Fake(torch.Tensor):                     # passes the tensor check without a GPU
        device = torch.device("cuda", 0)
    src = torch.zeros(4000, dtype=torch.uint8).as_subclass(Fake)
    with pytest.raises(ValueError, match="channels"):
        md2hip.resize_frames(src, [0], [(8, 8)], 4, 4, channels=2)
    with pytest.raises(ValueError, match="filter"):
        md2hip.resize_frames(src, [0], [(8, 8)], 4, 4, channels=1, filter="lanczos")
    with pytest.raises(ValueError, match="sizes must be 2 integer pairs"):
        md2hip.resize_frames(src, [0, 100], [(8, 8)], 4, 4, channels=1)
    with pytest.raises(ValueError, match="within src"):
        md2hip.resize_frames(src, [3990], [(8, 8)], 4, 4, channels=1)
    with pytest.raises(ValueError, match="within src"):
        md2hip.resize_frames(src, [-1], [(8, 8)], 4, 4, channels=1)
    with pytest.raises(ValueError, match="16 times"):
        md2hip.resize_frames(src, [0], [(33, 8)], 2, 4, channels=1)
    with pytest.raises(ValueError, match="one value per image"):
        md2hip.resize_frames(src, [0], [(8, 8)], 4, 4, channels=1, flips=[1, 0])
    with pytest.raises(ValueError, match="return_u8 needs quantize"):
        md2hip.resize_frames(src, [0], [(8, 8)], 4, 4, channels=1, quantize=False, return_u8=True)
    with pytest.raises(ValueError, match="height and width"):
        md2hip.resize_frames(src, [0], [(8, 8)], 0, 4, channels=1)


def test_kitty_dataset_options(tmp_path):
    import md2hip
    root = _kitti_tree(tmp_path, "image_0", "L", 3)
    with pytest.raises(ValueError, match="antialias"):
        md2hip.KittyDataset(root, "00", target_size=(8, 24), filter="antialias")      # the host path has none
    with pytest.raises(ValueError, match="resize"):
        md2hip.KittyDataset(root, "00", target_size=(8, 24), resize="gpu")
    with pytest.raises(ValueError, match="camera"):
        md2hip.KittyDataset(root, "00", target_size=(8, 24), camera="image_9")
    host = md2hip.KittyDataset(root, "00", target_size=(8, 24))
    dev = md2hip.KittyDataset(root, "00", target_size=(8, 24), resize="device", filter="antialias")
    assert host.channels == dev.channels == 1 and np.array_equal(host.K, dev.K)
    assert host.resize == "host" and dev.resize == "device" and dev.filter == "antialias"
    with pytest.raises(TypeError, match="device"):
        host.batch_native([0])
    with pytest.raises(ValueError, match="host and device"):
        md2hip.DChain([host, dev])
    with pytest.raises(ValueError, match="colour camera"):
        md2hip.KittyDataset(root, "00", target_size=(8, 24), camera="image_2")
    # the native-size batch: three frames in slots sized from the first, FlipX coins per frame
    buf, offsets, sizes, flips = dev.batch_native([0], threads=2)
    assert sizes.tolist() == [[31, 94], [30, 93], [31, 94]] and flips.tolist() == [0, 0, 0]
    assert offsets.tolist() == [0, dev.slot_bytes, 2 * dev.slot_bytes] and dev.slot_bytes % 16 == 0
    assert 31 * 94 < dev.slot_bytes <= 31 * 94 * 1.05 + 16
    chain = md2hip.DChain([dev, dev])
    assert chain.resize == "device" and len(chain) == 2
    _, o2, s2, _ = chain.batch_native([1, 0], threads=2)
    assert s2.tolist() == sizes.tolist() * 2 and len(set(o2.tolist())) == 6
    root2 = _kitti_tree(tmp_path / "colour", "image_2", "RGB", 3)
    col = md2hip.KittyDataset(root2, "00", target_size=(8, 24), camera="image_2", resize="device")
    assert col.channels == 3 and len(col) == 1


# ---- md2_load_frames_native_u8 against PIL ----------------------------------------------------------
def _write_png(path, mode, h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    nch = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
    a = rng.integers(0, 256, (h, w, nch), dtype=np.uint8)
    Image.fromarray(a[..., 0] if nch == 1 else a).save(path)      # L / RGB / RGBA by the shape
    return a


def _kitti_tree(root, camera, mode, n_frames, sizes=((31, 94), (30, 93))):
    d = root / "sequences" / "00" / camera
    d.mkdir(parents=True)
    (root / "sequences" / "00" / "calib.txt").write_text(
        "P0: 7.188560000000e+02 0 6.071928000000e+02 0 0 7.188560000000e+02 1.852157000000e+02 0 0 0 1 0\n")
    for k in range(n_frames):
        h, w = sizes[k % len(sizes)]
        _write_png(str(d / ("%06d.png" % k)), mode, h, w, 100 + k)
    return str(root)


def _decode(paths, c, slot):
    from md2hip._lib import check, lib
    n = len(paths)
    out = np.full(n * slot, 0xEE, dtype=np.uint8)
    w, h = np.zeros(n, np.int32), np.zeros(n, np.int32)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    check(lib().md2_load_frames_native_u8(arr, n, c, out.ctypes.data_as(C.c_void_p), slot,
                                          w.ctypes.data_as(C.POINTER(C.c_int)), h.ctypes.data_as(C.POINTER(C.c_int)), 3),
          "md2_load_frames_native_u8")
    return out, w, h


@pytest.mark.parametrize("mode,c", [("L", 1), ("RGB", 3), ("RGBA", 3)])
def test_native_decode_equals_pil_mixed_sizes(tmp_path, mode, c):
    from PIL import Image
    sizes = [(31, 94), (30, 93), (31, 92), (5, 7), (30, 92)]
    paths = []
    for k, (h, w) in enumerate(sizes):
        paths.append(str(tmp_path / f"{k}.png"))
        _write_png(paths[-1], mode, h, w, k)
    slot = 31 * 94 * c + 5
    out, w, h = _decode(paths, c, slot)
    assert list(zip(h.tolist(), w.tolist())) == sizes
    for k, (hh, ww) in enumerate(sizes):
        with Image.open(paths[k]) as im:
            want = np.asarray(im.convert("RGB") if c == 3 else im, dtype=np.uint8).reshape(hh, ww, c)
        got = out[k * slot:k * slot + hh * ww * c].reshape(hh, ww, c)
        assert np.array_equal(got, want), k
        assert (out[k * slot + hh * ww * c:(k + 1) * slot] == 0xEE).all()      # nothing past the image


def test_native_decode_errors_name_the_file(tmp_path):
    from md2hip import MD2Error
    gray, rgb = str(tmp_path / "gray.png"), str(tmp_path / "rgb.png")
    _write_png(gray, "L", 8, 9, 1)
    _write_png(rgb, "RGB", 8, 9, 2)
    with pytest.raises(MD2Error, match="gray.png"):
        _decode([rgb, gray], 3, 8 * 9 * 3)                  # a gray file under c = 3
    with pytest.raises(MD2Error, match="rgb.png"):
        _decode([gray, rgb], 1, 8 * 9)                      # a colour file under c = 1
    with pytest.raises(MD2Error, match="rgb.png.*slot"):
        _decode([rgb], 3, 8 * 9 * 3 - 1)                    # one byte short
    with pytest.raises(MD2Error, match="c must be 1 or 3"):
        _decode([rgb], 2, 8 * 9 * 3)
    out, w, h = _decode([rgb], 3, 8 * 9 * 3)                # exactly fitting
    assert (w[0], h[0]) == (9, 8)


def test_decode_frames_wrapper(tmp_path):
    import md2hip
    paths = []
    want = []
    for k, (h, w) in enumerate([(31, 94), (30, 93), (31, 92)]):
        paths.append(str(tmp_path / f"{k}.png"))
        want.append(_write_png(paths[-1], "RGB", h, w, k))
    buf, offsets, sizes = md2hip.decode_frames(paths, channels=3, threads=2)
    assert sizes.tolist() == [[31, 94], [30, 93], [31, 92]]
    assert offsets[0] == 0 and offsets[1] % 16 == 0 and offsets[1] >= 31 * 94 * 3
    for o, im in zip(offsets, want):
        assert np.array_equal(buf.numpy()[o:o + im.size].reshape(im.shape), im)
