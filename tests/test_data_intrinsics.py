"""CPU: per-sample intrinsics in the data pipeline (DChain.intrinsics, DataLoader(intrinsics=True))
and the mirror formula they rest on.

K is in the 1-based pixel coordinates of Backproject, whose image centre is (W + 1) / 2, so a sample
mirrored left-right (FlipX) keeps its geometry with cx' = W + 1 - cx.  The last test states that on
the fp64 oracle: mirroring frames, disparities and poses with cx' reproduces the loss to 1e-7
relative.  On this test's inputs (3 x 32 x 64, cx = W/2 + W/16) the oracle alone gives 3.6e-9, 2.2e-9
with the automask; the nearest wrong formula, W - cx, is off by 2.7e-4 (3.9e-4), and leaving cx
alone by 3.4e-3 (1.6e-3): the bound sits 25x above the one and 2700x below the other."""
import numpy as np
import pytest
import torch

from oracle import md2_oracle as O
from tests import _data as D
from PIL import Image


def _depth10k(tmp_path, name, n, seed, augmentations=None):
    import md2hip
    d = tmp_path / name
    d.mkdir()
    rng = np.random.default_rng(seed)
    files = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (128, 3 * 416, 3), dtype=np.uint8), mode="RGB").save(str(d / f"{i:03d}.png"))
        files.append(f"{i:03d}.png")
    return md2hip.Depth10k(str(d), files, augmentations=augmentations)


def _chain(tmp_path, augmentations=None):
    """Two Depth10k members with different cameras (the second's K is replaced)."""
    import md2hip
    a = _depth10k(tmp_path, "a", 3, 1, augmentations)
    b = _depth10k(tmp_path, "b", 4, 2, augmentations)
    b.K = md2hip.data.intrinsics(501.5, 517.25, 230.75, 55.5)
    b.invK = np.linalg.inv(b.K)
    return md2hip.DChain([a, b]), a, b


def test_dataset_and_dchain_intrinsics_follow_the_members(tmp_path):
    ch, a, b = _chain(tmp_path)
    k = a.intrinsics([0, 2])
    assert k.shape == (2, 3, 3) and k.dtype == np.float64 and (k == a.K).all()
    idx = [2, 3, 0, 6, 1, 4]                      # bin edge at 3: 0..2 -> a, 3..6 -> b
    k = ch.intrinsics(idx)
    assert k.shape == (6, 3, 3) and k.dtype == np.float64
    for row, i in zip(k, idx):
        assert (row == (a.K if i < 3 else b.K)).all(), i
    assert not (a.K == b.K).all()
    with pytest.raises(IndexError):
        ch.intrinsics([7])


def test_dchain_still_refuses_stereo_members(tmp_path):
    import md2hip
    a = _depth10k(tmp_path, "a", 2, 1)
    a.stereo = True
    with pytest.raises(ValueError, match="stereo"):
        md2hip.DChain([a])


def test_loader_intrinsics_mirror_cx_and_leave_the_rest(tmp_path):
    import md2hip
    ch, a, b = _chain(tmp_path, augmentations=md2hip.FlipX(0.5))
    W = ch.resolution[0]
    seed = 5
    dl = md2hip.DataLoader(ch, 7, shuffle=False, seed=seed, workers=2, intrinsics=True)
    plain = md2hip.DataLoader(ch, 7, shuffle=False, seed=seed, workers=2)
    out = list(dl)
    ref = list(plain)
    assert len(out) == 1 and isinstance(out[0], tuple) and len(out[0]) == 3
    x, K, invK = out[0]
    # without intrinsics=True the loader yields what it yielded: the bare batch, the same samples
    assert isinstance(ref[0], torch.Tensor) and torch.equal(ref[0], x)
    assert K.shape == (7, 9) and invK.shape == (7, 9) and K.dtype == invK.dtype == torch.float32
    coins = ch.flip_coins(list(range(7)), seed)          # epoch 0
    assert 0 < coins.sum() < 7, coins                    # both kinds of sample are present
    for i in range(7):
        ds, li = (a, i) if i < 3 else (b, i - 3)
        # the coin is the sample's own: the frames of a mirrored sample are the mirrored frames
        raw = md2hip.Depth10k(ds.dir, ds.files).getobs(li)
        want_x = raw[..., ::-1] if coins[i] else raw
        assert (x[i].numpy() == want_x).all(), i
        Ki = np.array(ds.K, dtype=np.float64)
        if coins[i]:
            Ki[0, 2] = W + 1.0 - Ki[0, 2]
        assert (K[i].numpy() == Ki.reshape(9).astype(np.float32)).all(), i
        assert (invK[i].numpy() == np.linalg.inv(Ki).reshape(9).astype(np.float32)).all(), i
        if not coins[i]:
            assert (K[i].numpy().reshape(3, 3) == ds.K.astype(np.float32)).all()


def test_loader_intrinsics_need_known_augmentations(tmp_path):
    import md2hip
    ds = _depth10k(tmp_path, "a", 2, 1, augmentations=lambda frames, rng: frames)
    with pytest.raises(ValueError, match="FlipX"):
        list(md2hip.DataLoader(ds, 2, shuffle=False, workers=1, native=False, intrinsics=True))


# ---- the mirror formula on the oracle -------------------------------------------------------------
def _loss(x, disps, poses, K, automask):
    N, L, C, H, W = x.shape
    cache = O.TrainCache(K=K, invK=torch.linalg.inv(K), scales=(0.125, 0.25, 0.5, 1.0), source_ids=(1, 3))
    p = O.Params(target_size=(W, H), batch_size=N, automasking=automask, disparity_smoothness=1e-3)
    am = O.automasking_loss(x, x[:, 1], (1, 3)) if automask else None
    return O.loss_from_outputs(disps, poses, x, am, cache, p).item()


@pytest.mark.parametrize("automask", [False, True], ids=["plain", "automask"])
def test_mirror_invariance_on_the_oracle(automask):
    from tests.test_gpu_loss_intrinsics import sample_intrinsics
    N, C, H, W = 1, 3, 32, 64
    x = D.triplets(N, C, H, W, seed=7)
    disps = D.disparities(N, H, W, seed=11)
    poses = D.poses(N, seed=13)
    K = sample_intrinsics(1, W, H)[0][0]
    base = _loss(x, disps, poses, K, automask)
    sr = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64)
    st = torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64)
    xm, dm = x.flip(-1), [d.flip(-1) for d in disps]
    pm = [(r * sr, t * st) for r, t in poses]

    def mirrored(cx):
        Km = K.clone()
        Km[0, 2] = cx
        return _loss(xm, dm, pm, Km, automask)

    cx = K[0, 2].item()
    good = abs(mirrored(W + 1 - cx) - base) / abs(base)
    print(f"cx' = W + 1 - cx: {good:.3e}; cx: {abs(mirrored(cx) - base) / abs(base):.3e}; "
          f"W - cx: {abs(mirrored(W - cx) - base) / abs(base):.3e}")
    assert good <= 1e-7, good
    # the formulas this one replaces are wrong by orders of magnitude more
    assert abs(mirrored(W - cx) - base) / abs(base) > 1e-5
    assert abs(mirrored(cx) - base) / abs(base) > 1e-5


# ---- the GPU branch of the loader: K, invK ride behind whatever it yields -------------------------
from tests.test_data_stereo import TW, _ds, kitti  # noqa: E402,F401  (kitti: the synthetic KITTI tree fixture)


def _expected(dl, ds, n, seed):
    K, invK = dl.batch_intrinsics(list(range(n)), 0)
    coins = ds.flip_coins(list(range(n)), seed)
    return K, invK, coins


@pytest.mark.gpu
def test_gpu_loader_appends_intrinsics_plain_and_with_colour_jitter(tmp_path):
    import md2hip
    ch, a, b = _chain(tmp_path, augmentations=md2hip.FlipX(0.5))
    seed = 5
    dl = md2hip.DataLoader(ch, 7, shuffle=False, seed=seed, workers=2, device="cuda", intrinsics=True)
    (out,) = list(dl)
    torch.cuda.synchronize()
    assert isinstance(out, tuple) and len(out) == 3
    x, K, invK = out
    wK, wiK, coins = _expected(dl, ch, 7, seed)
    assert 0 < coins.sum() < 7
    assert x.shape == (7, 3, 3, 128, 416) and x.is_cuda
    for t, w in ((K, wK), (invK, wiK)):
        assert t.is_cuda and t.dtype == torch.float32 and t.shape == (7, 9) and t.is_contiguous()
        assert (t.cpu().numpy() == w).all()
    W = ch.resolution[0]
    for i in range(7):
        cx = (a if i < 3 else b).K[0, 2]
        assert K[i, 2].item() == np.float32(W + 1.0 - cx if coins[i] else cx)
    # the same batch without the option: the bare tensor
    (bare,) = list(md2hip.DataLoader(ch, 7, shuffle=False, seed=seed, workers=2, device="cuda"))
    assert isinstance(bare, torch.Tensor) and torch.equal(bare, x)
    # with colour jitter: (x, x_net, K, invK)
    jl = md2hip.DataLoader(ch, 7, shuffle=False, seed=seed, workers=2, device="cuda", intrinsics=True,
                           color_jitter=md2hip.ColorJitter())
    (out,) = list(jl)
    torch.cuda.synchronize()
    assert len(out) == 4
    assert torch.equal(out[0], x) and out[1].shape == x.shape
    assert torch.equal(out[2], K) and torch.equal(out[3], invK)


@pytest.mark.gpu
def test_gpu_loader_appends_intrinsics_to_the_stereo_tuple(kitti):
    import md2hip
    ds = _ds(kitti, "image_2", filter="imresize", augmentations=md2hip.FlipX(0.5))
    seed = 3
    plain = next(iter(md2hip.DataLoader(ds, 2, shuffle=False, seed=seed, device="cuda", stereo=True)))
    dl = md2hip.DataLoader(ds, 2, shuffle=False, seed=seed, device="cuda", stereo=True, intrinsics=True)
    out = next(iter(dl))
    torch.cuda.synchronize()
    assert len(plain) == 3 and len(out) == 5
    for u, v in zip(plain, out[:3]):            # (x, x_stereo, stereo_Rt) as without the option
        assert torch.equal(u, v)
    wK, wiK, coins = _expected(dl, ds, 2, seed)
    assert (out[3].cpu().numpy() == wK).all() and (out[4].cpu().numpy() == wiK).all()
    for i in range(2):
        assert out[3][i, 2].item() == np.float32(TW + 1.0 - ds.K[0, 2] if coins[i] else ds.K[0, 2])
    jl = md2hip.DataLoader(ds, 2, shuffle=False, seed=seed, device="cuda", stereo=True, intrinsics=True,
                           color_jitter=md2hip.ColorJitter())
    out = next(iter(jl))
    torch.cuda.synchronize()
    assert len(out) == 6 and out[1].shape == out[0].shape and out[2].shape == plain[1].shape
    assert (out[4].cpu().numpy() == wK).all() and (out[5].cpu().numpy() == wiK).all()
