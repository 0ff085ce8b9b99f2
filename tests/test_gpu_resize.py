"""md2_resize_frames on the GPU against its float64 NumPy restatement (tests/_resize_ref.py:
include/md2.h operation by operation) and against the host path it replaces.  The kernel is fp64
without contraction in the stated order, so every comparison here is BIT FOR BIT: the float planes
with and without the N0f8 rounding, and the bytes.

The reduction cap.  The interface refuses n_in > 16 * n_out, so the largest reduction of a 2-row
target is 32 rows; 33 x 1 -> 2 x 1 must be refused (tests/test_resize_abi.py holds the library to
that without a GPU, test_beyond_the_cap_is_refused here the wrapper).  The cap case below is
therefore 32 x 1 -> 2 x 1, with 48 x 1 -> 3 x 1 for an interior window at the full 16x."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _resize_ref as R

pytestmark = pytest.mark.gpu

FILTERS = [R.IMRESIZE, R.ANTIALIAS]
R_FILTER_ID = {R.IMRESIZE: 0, R.ANTIALIAS: 1}      # MD2_RESIZE_IMRESIZE, MD2_RESIZE_ANTIALIAS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu_resize(imgs, height, width, filter, *, quantize=True, flips=None, return_u8=None):
    import md2hip
    c = imgs[0].shape[2]
    buf, offsets, sizes = R.pack(imgs)
    src = torch.from_numpy(buf).cuda()
    if return_u8 is None:
        return_u8 = quantize
    res = md2hip.resize_frames(src, offsets, sizes, height, width, channels=c, filter=filter, quantize=quantize,
                               flips=flips, return_u8=return_u8)
    out, u8 = res if return_u8 else (res, None)
    return out.cpu().numpy(), None if u8 is None else u8.cpu().numpy()


def check(imgs, height, width, filter, flips=None):
    """All three outputs of the device held to the restatement: out and out_u8 with quantize, out
    without."""
    out, u8 = gpu_resize(imgs, height, width, filter, quantize=True, flips=flips)
    rf, ru = R.resize_batch_ref(imgs, height, width, filter, True, flips)
    assert out.dtype == np.float32 and out.shape == rf.shape and u8.dtype == np.uint8
    bad = u8 != ru
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], u8[bad][:5], ru[bad][:5])
    assert np.array_equal(bits(out), bits(rf))
    raw, none = gpu_resize(imgs, height, width, filter, quantize=False, flips=flips)
    rr, _ = R.resize_batch_ref(imgs, height, width, filter, False, flips)
    bad = bits(raw) != bits(rr)
    assert none is None and not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], raw[bad][:5], rr[bad][:5])
    return out, u8


# ---- bit-equality with the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("src,dst", [((37, 53), (8, 12)),     # odd row lengths, 3-byte pixels
                                     ((5, 7), (8, 12)),       # upsampling (imresize clamps)
                                     ((16, 24), (8, 12)),     # the exact 2x: weights in eighths, many ties
                                     ((1, 1), (4, 4)),
                                     ((32, 1), (2, 1)),       # the 16x cap (module docstring)
                                     ((48, 1), (3, 1)),
                                     ((8, 12), (8, 12))])     # identity: a copy
def test_equals_restatement(src, dst, filter, c):
    imgs = R.random_images(21, [src, src], c)
    check(imgs, dst[0], dst[1], filter, flips=[0, 1])


@pytest.mark.parametrize("filter", FILTERS)
def test_exact_two_to_one_has_ties(filter):
    """Bytes that are multiples of 8 through the 1/8, 3/8 weights: r * 255 is often exactly k + 1/2."""
    rng = np.random.default_rng(22)
    imgs = [(rng.integers(0, 32, (16, 24, 3)) * 8).astype(np.uint8)]
    r = R.resize_value(imgs[0], 8, 12, filter) * 255.0
    if filter == R.ANTIALIAS:
        assert (np.abs(r - np.floor(r) - 0.5) == 0).sum() > 0        # the case is what it claims to be
    check(imgs, 8, 12, filter)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("filter", FILTERS)
def test_five_sizes_in_one_call(filter, c):
    # KITTI's spread scaled down, flips on some
    sizes = [(31, 94), (30, 93), (31, 92), (30, 92), (31, 93)]
    check(R.random_images(23, sizes, c), 8, 24, filter, flips=[0, 1, 1, 0, 1])


@pytest.mark.parametrize("filter", FILTERS)
def test_more_than_one_block_each_way(filter):
    # 150 columns (two column tiles, the second partly filled), 19 rows (three row bands), two staging
    # passes for the colour rows
    check(R.random_images(24, [(97, 301), (60, 450)], 3), 19, 150, filter, flips=[1, 0])


def test_beyond_the_cap_is_refused():
    import md2hip
    src = torch.zeros(64, dtype=torch.uint8).cuda()
    with pytest.raises(ValueError, match="16 times"):
        md2hip.resize_frames(src, [1], [(33, 1)], 2, 1, channels=1, filter="antialias")


# ---- the same bytes as the host path -------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("src,dst", [((37, 53), (8, 12)), ((5, 7), (8, 12)), ((61, 187), (16, 48))])
def test_imresize_equals_host_path(src, dst, flip):
    from md2hip.data import imresize
    for c in (1, 3):
        imgs = R.random_images(25, [src], c)
        out, u8 = gpu_resize(imgs, dst[0], dst[1], R.IMRESIZE, quantize=True, flips=[flip])
        want = imresize(np.ascontiguousarray(imgs[0].transpose(2, 0, 1)), *dst)
        if flip:
            want = want[..., ::-1]
        assert np.array_equal(u8[0], want)
        assert np.array_equal(bits(out[0]), bits(want.astype(np.float32) / np.float32(255.0)))


# ---- only its own output, and the same bits twice --------------------------------------------------------
@pytest.mark.parametrize("filter", FILTERS)
def test_writes_only_its_output_and_repeats(filter):
    from md2hip._lib import ResizeCfg, check as md2_check, lib, ptr, stream_of
    imgs = R.random_images(26, [(37, 53), (36, 52), (37, 51)], 3)
    buf, offsets, sizes = R.pack(imgs)
    src = torch.from_numpy(buf).cuda()
    m, c, H, W = 3, 3, 8, 12
    n = m * c * H * W
    sw = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    sh = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    runs = []
    for _ in range(2):
        out = torch.full((n + W,), float("nan"), dtype=torch.float32, device="cuda")
        out.view(torch.uint8).fill_(0xFF)
        u8 = torch.full((n + W,), 0xFF, dtype=torch.uint8, device="cuda")
        cfg = ResizeCfg(m, c, H, W, R_FILTER_ID[filter], 1)
        md2_check(lib().md2_resize_frames(C.byref(cfg), ptr(src), offsets.ctypes.data_as(C.POINTER(C.c_longlong)),
                                          sw.ctypes.data_as(C.POINTER(C.c_int)), sh.ctypes.data_as(C.POINTER(C.c_int)),
                                          None, ptr(out), ptr(u8), stream_of(out.device)), "md2_resize_frames")
        torch.cuda.synchronize()
        runs.append((out.view(torch.int32).cpu().numpy(), u8.cpu().numpy()))
    (o1, b1), (o2, b2) = runs
    assert (o1[n:] == -1).all() and (b1[n:] == 0xFF).all()           # the guard rows stay untouched
    assert np.array_equal(o1, o2) and np.array_equal(b1, b2)         # the same bits twice
    rf, ru = R.resize_batch_ref(imgs, H, W, filter, True, None)      # flip = NULL: none
    assert np.array_equal(o1[:n].view(np.uint32), bits(rf).reshape(-1))
    assert np.array_equal(b1[:n], ru.reshape(-1))


# ---- wrapper chunking ----------------------------------------------------------------------------------
def test_wrapper_chunks_at_64_images():
    import md2hip
    imgs = R.random_images(27, [(9 + k % 3, 11 + k % 4) for k in range(65)], 3)
    flips = [k % 3 == 0 for k in range(65)]
    buf, offsets, sizes = R.pack(imgs)
    src = torch.from_numpy(buf).cuda()
    kw = dict(channels=3, filter="antialias", quantize=True)
    whole, whole8 = md2hip.resize_frames(src, offsets, sizes, 4, 6, flips=flips, return_u8=True, **kw)
    a = md2hip.resize_frames(src, offsets[:64], sizes[:64], 4, 6, flips=flips[:64], **kw)
    b = md2hip.resize_frames(src, offsets[64:], sizes[64:], 4, 6, flips=flips[64:], **kw)
    assert whole.shape == (65, 3, 4, 6)
    assert torch.equal(whole, torch.cat([a, b]))
    rf, ru = R.resize_batch_ref(imgs, 4, 6, R.ANTIALIAS, True, flips)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(rf)) and np.array_equal(whole8.cpu().numpy(), ru)


# ---- the loader, end to end ------------------------------------------------------------------------------
def _kitti_tree(root, camera, n_frames, seed):
    from PIL import Image
    d = root / "sequences" / "00" / camera
    d.mkdir(parents=True)
    (root / "sequences" / "00" / "calib.txt").write_text(
        "P0: 7.188560000000e+02 0 6.071928000000e+02 0 0 7.188560000000e+02 1.852157000000e+02 0 0 0 1 0\n")
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(n_frames):
        h, w = ((61, 187), (60, 186))[(k // 2) % 2]
        a = rng.integers(0, 256, (h, w, 3 if camera == "image_2" else 1), dtype=np.uint8)
        Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).save(str(d / ("%06d.png" % k)))
        frames.append(a)
    return str(root), frames


def test_loader_gray_equals_host_loader(tmp_path):
    import md2hip
    root, _ = _kitti_tree(tmp_path, "image_0", 12, 31)
    kw = dict(target_size=(16, 48), augmentations=md2hip.FlipX(0.5))
    host = md2hip.KittyDataset(root, "00", **kw)
    dev = md2hip.KittyDataset(root, "00", resize="device", **kw)
    lk = dict(shuffle=True, seed=5, workers=4, device="cuda")
    coins = host._native_flips(list(range(4)), 5)
    assert 0 < coins.sum() < 4                                       # the seed flips some samples, not all
    want = [x.cpu() for x in md2hip.DataLoader(host, 2, **lk)]
    got = [x.cpu() for x in md2hip.DataLoader(dev, 2, **lk)]
    assert len(got) == len(want) == 2
    for x, y in zip(got, want):
        assert x.shape == (2, 3, 1, 16, 48) and x.dtype == torch.float32
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_loader_colour_equals_restatement_and_trains(tmp_path):
    import md2hip
    """16 x 48 as for the gray frames, with both filters; the train step takes the same frames at
    64 x 128, the smallest size the five-level network of smoke() is run at."""
    root, frames = _kitti_tree(tmp_path, "image_2", 12, 32)
    batches = {}
    for (H, W), filter in (((16, 48), "antialias"), ((16, 48), "imresize"), ((64, 128), "antialias")):
        ds = md2hip.KittyDataset(root, "00", target_size=(H, W), camera="image_2", resize="device",
                                 filter=filter, augmentations=md2hip.FlipX(0.5))
        assert ds.channels == 3 and len(ds) == 4
        coins = ds._native_flips(list(range(4)), 5)
        assert 0 < coins.sum() < 4
        batches[H, filter] = list(md2hip.DataLoader(ds, 2, shuffle=False, seed=5, workers=4, device="cuda"))
        assert len(batches[H, filter]) == 2
        for b, x in enumerate(batches[H, filter]):
            assert x.shape == (2, 3, 3, H, W)
            rf, _ = R.resize_batch_ref(frames[6 * b:6 * b + 6], H, W, filter, True, np.repeat(coins[2 * b:2 * b + 2], 3))
            assert np.array_equal(bits(x.cpu().numpy().reshape(6, 3, H, W)), bits(rf)), (H, W, filter, b)
    # one train step on the colour batch
    enc = md2hip.ResNet(18, in_channels=3)
    model = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0), md2hip.PoseDecoder(512), seed=42)
    cache = md2hip.TrainCache(K=ds.K, invK=ds.invK)
    params = md2hip.Params(target_size=(128, 64), batch_size=2, automasking=False)
    loss = md2hip.train_step(model, batches[64, "antialias"][0].contiguous(), None, cache, params, md2hip.ADAM(1e-4))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def test_load_frames(tmp_path):
    import md2hip
    root, frames = _kitti_tree(tmp_path, "image_2", 3, 33)
    paths = [str(tmp_path / "sequences" / "00" / "image_2" / ("%06d.png" % k)) for k in range(3)]
    x = md2hip.load_frames(paths, 16, 48, channels=3, filter="antialias", threads=2)
    rf, _ = R.resize_batch_ref(frames, 16, 48, R.ANTIALIAS, True, None)
    assert x.shape == (3, 3, 16, 48) and np.array_equal(bits(x.cpu().numpy()), bits(rf))
