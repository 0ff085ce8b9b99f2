"""The stereo partner frame in the KITTI loader (KittyDataset(stereo=True), DataLoader(stereo=True))
on a synthetic KITTI tree: partner paths and side for all four cameras, the [4][C][H][W] host
restatement and its FlipX, the refusals, and (GPU) the device-route loader against the restatement,
bit for bit."""
import os

import numpy as np
import pytest
import torch

from PIL import Image

CALIB = ("P0: 7.215377e+02 0.000000e+00 6.095593e+02 0.000000e+00 0.000000e+00 7.215377e+02 "
         "1.728540e+02 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00\n")
CHANNELS = {"image_0": 1, "image_1": 1, "image_2": 3, "image_3": 3}
PARTNER = {"image_0": "image_1", "image_1": "image_0", "image_2": "image_3", "image_3": "image_2"}
SIDE = {"image_0": "l", "image_1": "r", "image_2": "l", "image_3": "r"}
NFRAMES, SH, SW, TH, TW = 7, 37, 123, 16, 48          # 7 frames -> 2 triplets; odd source size


@pytest.fixture(scope="module")
def kitti(tmp_path_factory):
    """sequences/03 with all four cameras, as tests/test_data.py builds image_0."""
    root = tmp_path_factory.mktemp("kitti")
    seq = root / "sequences" / "03"
    seq.mkdir(parents=True)
    (seq / "calib.txt").write_text(CALIB)
    rng = np.random.default_rng(1)
    for cam, c in CHANNELS.items():
        (seq / cam).mkdir()
        for k in range(NFRAMES):
            a = (rng.random((SH, SW) if c == 1 else (SH, SW, 3)) * 255).round().astype(np.uint8)
            Image.fromarray(a, mode="L" if c == 1 else "RGB").save(str(seq / cam / ("%06d.png" % k)))
    return str(root)


def _ds(kitti, cam, **kw):
    import md2hip
    return md2hip.KittyDataset(kitti, "03", target_size=(TH, TW), camera=cam, resize="device", stereo=True, **kw)


def _resized(path, c):
    from md2hip.data import imresize
    a = np.asarray(Image.open(path))
    a = a[None] if c == 1 else a.transpose(2, 0, 1)
    return imresize(np.ascontiguousarray(a), TH, TW)


@pytest.mark.parametrize("cam", sorted(CHANNELS))
def test_partner_paths_and_side(kitti, cam):
    ds = _ds(kitti, cam)
    assert ds.side == SIDE[cam] and ds.stereo and ds.frames_per_sample == 4 and len(ds) == 2
    for i in range(2):
        want = os.path.join(kitti, "sequences", "03", PARTNER[cam], "%06d.png" % (3 * i + 1))
        assert ds.partner_path(i) == want
        paths = [p.decode() for p in ds._paths([i])]
        assert paths == [os.path.join(kitti, "sequences", "03", cam, "%06d.png" % (3 * i + j)) for j in range(3)] + [want]


@pytest.mark.parametrize("cam", sorted(CHANNELS))
def test_getobs_u8_fourth_frame_is_the_resized_partner(kitti, cam):
    c = CHANNELS[cam]
    ds = _ds(kitti, cam)
    s = ds.getobs_u8(1)
    assert s.shape == (4, c, TH, TW) and s.dtype == np.uint8
    assert (s[3] == _resized(ds.partner_path(1), c)).all()
    for j in range(3):
        assert (s[j] == _resized(os.path.join(kitti, "sequences", "03", cam, "%06d.png" % (3 + j)), c)).all()
    # without stereo the sample is the first three frames
    import md2hip
    plain = md2hip.KittyDataset(kitti, "03", target_size=(TH, TW), camera=cam, resize="device")
    assert not plain.stereo and (plain.getobs_u8(1) == s[:3]).all()


def test_flipx_mirrors_the_partner_with_its_sample(kitti):
    import md2hip
    ds = _ds(kitti, "image_2", augmentations=md2hip.FlipX(0.5))
    plain = _ds(kitti, "image_2")
    seen = set()
    for seed in range(8):
        for i in range(2):
            coin = bool(ds._native_flips([i], seed)[0])
            seen.add(coin)
            want = plain.getobs_u8(i)
            got = ds.getobs_u8(i, seed)
            assert (got == (want[..., ::-1] if coin else want)).all()
    assert seen == {True, False}


def test_stereo_transforms_follow_side_and_flip():
    import md2hip
    for side, flip, tx in (("l", False, -0.1), ("l", True, 0.1), ("r", False, 0.1), ("r", True, -0.1)):
        Rt = md2hip.stereo_transforms([side], [flip])
        assert Rt[0, 9] == np.float32(tx) and (Rt[0, [0, 4, 8]] == 1).all() and Rt[0].sum() == np.float32(3) + Rt[0, 9]


def test_host_resize_with_stereo_is_refused(kitti):
    import md2hip
    with pytest.raises(ValueError, match='resize="device"'):
        md2hip.KittyDataset(kitti, "03", target_size=(TH, TW), camera="image_0", resize="host", stereo=True)
    host = md2hip.KittyDataset(kitti, "03", target_size=(TH, TW), camera="image_0", resize="host")
    with pytest.raises(ValueError, match='resize="device"'):
        md2hip.DataLoader(host, 2, stereo=True)
    with pytest.raises(ValueError, match="agree"):
        md2hip.DataLoader(_ds(kitti, "image_0"), 2)
    with pytest.raises(ValueError, match="stereo"):
        md2hip.DChain([_ds(kitti, "image_0")])


@pytest.mark.gpu
@pytest.mark.parametrize("cam", ["image_1", "image_2"])
def test_loader_yields_the_partner_frame_and_its_transform(kitti, cam):
    import md2hip
    c = CHANNELS[cam]
    ds = _ds(kitti, cam, filter="imresize", augmentations=md2hip.FlipX(0.5))
    seed = 3
    dl = md2hip.DataLoader(ds, 2, shuffle=False, seed=seed, device="cuda", stereo=True)
    batches = list(dl)
    assert len(batches) == 1
    x, x_stereo, Rt = batches[0]
    torch.cuda.synchronize()
    assert x.shape == (2, 3, c, TH, TW) and x_stereo.shape == (2, c, TH, TW) and Rt.shape == (2, 12)
    assert x.is_contiguous() and x_stereo.is_contiguous() and Rt.dtype == torch.float32
    want = np.stack([ds.getobs_u8(i, seed) for i in range(2)]).astype(np.float32) / np.float32(255)
    assert (x.cpu().numpy() == want[:, :3]).all()
    assert (x_stereo.cpu().numpy() == want[:, 3]).all()
    coins = ds._native_flips([0, 1], seed)
    assert (Rt.cpu().numpy() == md2hip.stereo_transforms([SIDE[cam]] * 2, coins)).all()


@pytest.mark.gpu
def test_loader_with_colour_jitter_leaves_the_partner_alone(kitti):
    import md2hip
    ds = _ds(kitti, "image_2", filter="imresize")
    jit = md2hip.ColorJitter()
    x, x_net, x_stereo, Rt = next(iter(md2hip.DataLoader(ds, 2, shuffle=False, device="cuda", stereo=True,
                                                         color_jitter=jit)))
    torch.cuda.synchronize()
    want = np.stack([ds.getobs_u8(i) for i in range(2)]).astype(np.float32) / np.float32(255)
    assert (x.cpu().numpy() == want[:, :3]).all() and (x_stereo.cpu().numpy() == want[:, 3]).all()
    assert x_net.shape == x.shape and Rt.shape == (2, 12)
