"""The NumPy restatement of md2_resize_frames (tests/_resize_ref.py) against what it restates, on the
CPU: the imresize filter against md2hip.data.imresize byte for byte, the antialias filter against
known answers and against torch's float64 interpolate(antialias=True).

The torch bound.  Both sides form the same weights and the same products in float64; torch is free
to sum in another order.  A sum of at most 33 x 33 non-negative terms bounded by 1 differs between
two orders by far less than 1e-12 (a few units of 2^-53 ~ 1.1e-16 per add; 5.6e-16 observed)."""
import numpy as np
import pytest

from tests import _resize_ref as R

SIZES = [((37, 53), (8, 12)), ((5, 7), (8, 12)), ((8, 12), (8, 12))]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("src,dst", SIZES)
def test_imresize_filter_equals_data_imresize(src, dst, c):
    from md2hip.data import imresize
    img = R.random_images(11, [src], c)[0]
    want = imresize(np.ascontiguousarray(img.transpose(2, 0, 1)), *dst)
    assert want.dtype == np.uint8
    f, u8 = R.resize_ref(img, dst[0], dst[1], R.IMRESIZE, quantize=True)
    assert u8.dtype == np.uint8 and np.array_equal(u8, want)
    assert np.array_equal(f.view(np.uint32), (want.astype(np.float32) / np.float32(255.0)).view(np.uint32))
    ff, _ = R.resize_ref(img, dst[0], dst[1], R.IMRESIZE, quantize=True, flip=True)
    assert np.array_equal(ff, f[..., ::-1])


def test_imresize_upsampling_clamps():
    taps = R.imresize_axis(5, 8)
    assert taps[0][0] == (0, 1.0) and taps[-1][0][0] == 4 and taps[-1][1] == (4, 0.0)


@pytest.mark.parametrize("value", [0, 1, 77, 128, 254, 255])
@pytest.mark.parametrize("src,dst", [((37, 53), (8, 12)), ((5, 7), (8, 12)), ((16, 24), (8, 12))])
def test_antialias_constant_stays_constant(src, dst, value):
    img = np.full(src + (3,), value, dtype=np.uint8)
    f, u8 = R.resize_ref(img, dst[0], dst[1], R.ANTIALIAS, quantize=True)
    assert (u8 == value).all()
    assert (f.view(np.uint32) == (np.float32(value) / np.float32(255.0)).view(np.uint32)).all()


def test_antialias_two_to_one_weights():
    taps = R.antialias_axis(8, 4)
    assert taps[1] == [(1, 0.125), (2, 0.375), (3, 0.375), (4, 0.125)]
    assert taps[2] == [(3, 0.125), (4, 0.375), (5, 0.375), (6, 0.125)]
    # the edge windows are truncated and renormalised: 3/8, 3/8, 1/8 over 7/8
    assert [k for k, _ in taps[0]] == [0, 1, 2]
    assert [w for _, w in taps[0]] == [0.375 / 0.875, 0.375 / 0.875, 0.125 / 0.875]
    assert [k for k, _ in taps[3]] == [5, 6, 7]
    assert [w for _, w in taps[3]] == [0.125 / 0.875, 0.375 / 0.875, 0.375 / 0.875]
    # an image through it: the interior pixel is the 2-D product of the 1-D weights
    img = np.zeros((8, 8, 1), dtype=np.uint8)
    img[3, 3, 0] = 255
    r = R.resize_value(img, 4, 4, R.ANTIALIAS)
    assert r[0, 1, 1] == 0.375 * 0.375 and r[0, 2, 2] == 0.125 * 0.125 and r[0, 1, 2] == 0.375 * 0.125


def test_antialias_tap_count_is_bounded():
    # the interface's cap: n_in <= 16 * n_out, at most 33 taps
    for n_in, n_out in [(32, 2), (48, 3), (16 * 7, 7), (127, 8), (8192, 512), (33, 3)]:
        assert max(len(t) for t in R.antialias_axis(n_in, n_out)) <= 33, (n_in, n_out)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("src,dst", [((37, 53), (8, 12)), ((31, 94), (8, 24)), ((16, 24), (8, 12)),
                                     ((5, 7), (8, 12))])
def test_antialias_against_torch_float64(src, dst, c):
    import torch
    import torch.nn.functional as F
    img = R.random_images(12, [src], c)[0]
    r = R.resize_value(img, dst[0], dst[1], R.ANTIALIAS)
    x = torch.from_numpy(img.astype(np.float64) / 255.0).permute(2, 0, 1)[None]
    want = F.interpolate(x, size=dst, mode="bilinear", antialias=True, align_corners=False)[0].numpy()
    err = np.abs(r - want).max()
    print(f"{src} -> {dst}, c = {c}: largest difference to torch float64 {err:.3e}")
    assert err <= 1e-12


def test_unquantised_is_the_rounded_value():
    img = R.random_images(13, [(16, 24)], 3)[0]
    f, u8 = R.resize_ref(img, 8, 12, R.ANTIALIAS, quantize=False)
    assert u8 is None and f.dtype == np.float32
    assert np.array_equal(f, R.resize_value(img, 8, 12, R.ANTIALIAS).astype(np.float32))


def test_pack_places_images_at_odd_offsets():
    imgs = R.random_images(14, [(3, 5), (4, 4), (2, 7)], 3)
    buf, offsets, sizes = R.pack(imgs)
    assert (offsets % 2 == 1).all() and sizes.tolist() == [[3, 5], [4, 4], [2, 7]]
    for o, im in zip(offsets, imgs):
        assert np.array_equal(buf[o:o + im.size].reshape(im.shape), im)
