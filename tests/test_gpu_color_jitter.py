"""md2_color_jitter on the GPU against its float32 NumPy restatement (tests/_color_ref.py) -- bit for
bit with the kernel's own frame means imposed -- and the means themselves, reproducibility, the
in-place call and the DataLoader's ``color_jitter`` keyword.

Sizes: 7 x 13 (less than a wave), 16 x 24, 64 x 128 (8 blocks per frame: the partials path); three
samples of three frames, one of them with apply = 0; c = 3 and 1.  Every one of the 24 orders runs at
every size: 12 launches per case, two orders each.

The means: the kernel's is (float)(S / (h*w)) with S its own fp64 sum, the restatement's the same
with NumPy's fp64 sum.  Two fp64 sums of <= 2^13 non-negative values differ by far less than an fp32
ulp, so the two agree within one fp32 rounding, 2^-23 relative; the bound is 2^-22."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _color_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(7, 13), (16, 24), (64, 128)]


def _run(x, p, out=None, means=None, ws=None):
    """md2_color_jitter through the C-ABI with caller-owned buffers"""
    from md2hip._lib import Jitter, check, lib, ptr, stream_of
    n, frames, c, h, w = x.shape
    out = torch.empty_like(x) if out is None else out
    means = torch.empty(n, frames, device="cuda") if means is None else means
    if ws is None:
        ws = torch.empty(lib().md2_color_jitter_workspace_size(n, frames, h, w) // 8, dtype=torch.float64,
                         device="cuda")
    check(lib().md2_color_jitter(ptr(x), n, frames, c, h, w, C.cast(C.c_void_p(p.ctypes.data), C.POINTER(Jitter)),
                                 ptr(out), ptr(means), ptr(ws), stream_of("cuda")), "md2_color_jitter")
    return out, means


def _params(k, rng, skip):
    """three records: orders 2k and 2k+1 on the two applied samples, sample ``skip`` copied"""
    p = R.params(3)
    p["brightness"], p["contrast"], p["saturation"] = (rng.uniform(0.6, 1.4, 3) for _ in range(3))
    p["hue"] = rng.uniform(-0.5, 0.5, 3)
    p["apply"] = 1
    p["apply"][skip] = 0
    rest = [i for i in range(3) if i != skip]
    p["order"][skip] = R.ORDERS[(5 * k) % 24]
    p["order"][rest[0]], p["order"][rest[1]] = R.ORDERS[2 * k], R.ORDERS[2 * k + 1]
    return p


@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("h,w", SIZES)
def test_bit_identical_to_the_restatement(h, w, c):
    x = R.test_images(3, 3, c, h, w, seed=h + c)
    xg = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(w)
    seen = set()
    for k in range(12):
        skip = k % 3
        p = _params(k, rng, skip)
        out, means = _run(xg, p)
        out, means = out.cpu().numpy(), means.cpu().numpy()
        ref, used, exact = R.color_jitter(x, p, np.float32, means=means, exact=True)
        assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
        bad = (out.view(np.uint32) != ref.view(np.uint32))
        assert not bad.any(), (f"orders {p['order'].tolist()}: {bad.sum()} of {bad.size} values differ, "
                               f"max {np.abs(out - ref).max():.3g}")
        assert out[skip].tobytes() == x[skip].tobytes()
        # the means: one fp32 rounding of an fp64 sum away from the restatement's, 0 where not applied
        assert (means[skip] == 0).all()
        rel = np.abs(means.astype(np.float64) - exact)[exact > 0] / exact[exact > 0]
        assert (exact > 0).sum() == 6 and rel.max() <= 2.0 ** -22, (rel.max(), means, exact)
        seen.update(tuple(o) for i, o in enumerate(p["order"].tolist()) if i != skip)
    assert seen == set(R.ORDERS)


def test_changes_the_image_and_one_channel_ignores_saturation_and_hue():
    x = R.test_images(3, 3, 1, 16, 24)
    xg = torch.from_numpy(x).cuda()
    a = _params(3, np.random.default_rng(0), 1)
    b = a.copy()
    b["saturation"], b["hue"] = 0.2, -0.45
    oa, ma = _run(xg, a)
    ob, mb = _run(xg, b)
    assert torch.equal(oa, ob) and torch.equal(ma, mb)
    assert not torch.equal(oa[0], xg[0]) and torch.equal(oa[1], xg[1])


@pytest.mark.parametrize("c", [3, 1])
def test_reproducible_and_in_place(c):
    """two calls, a call on 0xFF-filled workspace / out / means, and the in-place call: equal bytes"""
    from md2hip._lib import lib
    h, w = 64, 128
    x = torch.from_numpy(R.test_images(3, 3, c, h, w, seed=9)).cuda()
    p = _params(7, np.random.default_rng(1), 2)       # contrast mid-order on one sample, last on the other
    o1, m1 = _run(x, p)
    o2, m2 = _run(x, p)
    assert torch.equal(o1, o2) and torch.equal(m1, m2)
    nws = lib().md2_color_jitter_workspace_size(3, 3, h, w) // 8
    assert nws == 3 * 3 * 8
    ws = torch.full((nws * 8,), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float64)
    out = torch.full((x.numel() * 4,), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32).view(x.shape)
    means = torch.full((3 * 3 * 4,), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32).view(3, 3)
    o3, m3 = _run(x, p, out, means, ws)
    assert torch.equal(o1.view(torch.int32), o3.view(torch.int32)) and torch.equal(m1.view(torch.int32),
                                                                                   m3.view(torch.int32))
    xi = x.clone()
    o4, m4 = _run(xi, p, out=xi)
    assert o4.data_ptr() == xi.data_ptr() and torch.equal(o4, o1) and torch.equal(m4, m1)
    assert not torch.equal(o1, x)


def test_python_wrapper_chunks_and_matches_the_abi():
    """md2hip.color_jitter on 70 samples (two chunks of at most 64) equals per-sample calls; means too"""
    import md2hip
    cj = md2hip.ColorJitter(p=0.8)
    x = torch.from_numpy(R.test_images(70, 2, 3, 7, 13, seed=2)).cuda()
    p = cj.draw(list(range(70)), 4)
    means = torch.empty(70, 2, device="cuda")
    out = cj(x, p, means=means)
    assert out.shape == x.shape and out.data_ptr() != x.data_ptr()
    for i in (0, 63, 64, 69):
        oi, mi = _run(x[i:i + 1].contiguous(), p[i:i + 1])
        assert torch.equal(out[i:i + 1], oi) and torch.equal(means[i:i + 1], mi), i
    assert torch.equal(md2hip.color_jitter(x, p), out)
    assert md2hip.color_jitter(x, p, out=x) is x and torch.equal(x, out)
    with pytest.raises(ValueError):
        md2hip.color_jitter(out, p[:3])


def test_loader_yields_the_batch_and_its_jittered_copy(tmp_path):
    import md2hip
    from PIL import Image
    rng = np.random.default_rng(0)
    files = []
    for i in range(6):
        a = (rng.random((128, 3 * 416, 3)) * 255).round().astype(np.uint8)
        Image.fromarray(a, mode="RGB").save(str(tmp_path / f"{i}.png"))
        files.append(f"{i}.png")
    ds = md2hip.Depth10k(str(tmp_path), files, augmentations=md2hip.FlipX(0.5))
    cj = md2hip.ColorJitter(p=0.7)
    kw = dict(shuffle=True, seed=3, workers=2, device="cuda")
    plain = md2hip.DataLoader(ds, 2, **kw)
    aug = md2hip.DataLoader(ds, 2, color_jitter=cj, **kw)
    changed = 0
    for epoch in range(2):
        idx = aug.batch_indices(epoch)
        assert idx == plain.batch_indices(epoch)
        nb = 0
        for b, (x0, pair) in enumerate(zip(plain, aug)):
            assert isinstance(pair, tuple) and len(pair) == 2
            x, x_net = pair
            assert x.is_cuda and x_net.is_cuda and x.shape == x_net.shape == (2, 3, 3, 128, 416)
            assert torch.equal(x, x0)
            p = cj.draw(idx[b], 3 + epoch)
            assert torch.equal(x_net, md2hip.color_jitter(x, p))
            for k in range(2):
                assert torch.equal(x_net[k], x[k]) == (p["apply"][k] == 0)
            changed += int(p["apply"].sum())
            nb += 1
        assert nb == 3
    assert 0 < changed < 12
    with pytest.raises(ValueError):
        next(iter(md2hip.DataLoader(ds, 2, color_jitter=cj, device=None)))
