"""GPU: the loss tail over S = 1, 2 or 3 sources, learned or fixed (md2_loss_fwd_bwd_sources,
photo_sources.hip) -- stereo supervision.

1. S = 2 with two learned sources pointing at frames 0 and 2 of x gives the bits of the packed
   two-source kernel behind md2hip.loss_tail: every output, torch.equal, no tolerance.
2. S = 3 ("MS": both temporal sources and a stereo frame with a fixed transform) and S = 1 ("S")
   against the fp64 oracle, by the method of tests/test_gpu_loss.py::_check generalised to S
   candidates: the argmin map equals the oracle's first argmin except at near ties, then loss,
   d_disp and d_pose against the oracle with the GPU's argmin and bilinear cells imposed (loss rel
   2e-5, gradients relative Frobenius 2e-4 -- that file's bounds at the same pixel counts).
3. d_pose is [2N, 6] in MS and absent in S; the fixed transform is read, not differentiated.
4. md2_automasking_loss_sources: two sources give md2_automasking_loss's bits, three the oracle's
   values."""
import ctypes as C

import pytest
import torch

from oracle import md2_oracle as O
from tests import _data as D
from tests.golden import make_photo_bits as M

pytestmark = pytest.mark.gpu

SCALES = M.SCALES
DEV = "cuda"


def _cache_params(K, invK, W, H, N, nscales, automask):
    import md2hip
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy(), scales=SCALES[-nscales:])
    params = md2hip.Params(target_size=(W, H), batch_size=N, automasking=automask,
                           disparity_smoothness=1e-3)
    return cache, params


def _two_learned(x, cache, frame2=None):
    """md2_loss_source[2]: frames 0 and 2 of x, learned, invert as invert_mask gives it; with
    ``frame2`` the second source is that separate [N,C,H,W] tensor."""
    from md2hip import _lib
    N, L, Cc, H, W = x.shape
    fs = Cc * H * W
    arr = (_lib.LossSource * _lib.MAX_SOURCES)()
    for s, sid in enumerate(cache.source_ids):
        arr[s].frames = x.data_ptr() + 4 * (sid - 1) * fs
        arr[s].sample_stride = L * fs
        arr[s].pose_block = s
        arr[s].invert = int(sid < cache.target_id)
    if frame2 is not None:
        arr[1].frames = frame2.data_ptr()
        arr[1].sample_stride = fs
    return arr


def _bits_inputs(N, Cc, H, W, nscales, sources, automask, near):
    """The inputs of tests/golden/make_photo_bits.py::run_tail_case for such a case."""
    if sources == "uniform":
        x = torch.rand(N, 3, Cc, H, W, generator=torch.Generator().manual_seed(3), dtype=torch.float32)
    else:
        x = D.triplets(N, Cc, H, W, seed=7, ramp_sources=sources == "ramp").float()
    x = x.to(DEV).contiguous()
    K, invK = D.intrinsics(W, H)
    disps = [d.float().to(DEV).contiguous() for d in D.disparities(N, H, W, nscales=nscales, seed=11)]
    kw = dict(forward=0.05, jitter=0.2) if near else {}
    poses = [(a.float().to(DEV), b.float().to(DEV)) for a, b in D.poses(N, seed=13, **kw)]
    am = None
    if automask:
        am = (0.2 * torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(5))).to(DEV).contiguous()
    return x, K, invK, disps, poses, am


KEYS = ("loss", "terms", "d_disp", "d_pose", "vis_loss", "vis_sel", "vis_cell", "vis_warped")

S2_CASES = {
    "small": (2, 3, 32, 64, 4, "texture", False, False),
    "gray-96wide": M.TAIL_CASES["gray-96wide"],
    "ragged": (3, 3, 40, 72, 4, "texture", False, False),
    "near-field-automask": M.TAIL_CASES["near-field-automask"],
}


def _assert_same_bits(a, b):
    for k in KEYS:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k])
            for i, (u, v) in enumerate(zip(a[k], b[k])):
                assert torch.equal(u, v), f"{k}[{i}]"
        else:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def _s2_pair(case, separate):
    import md2hip
    from md2hip import loss as L
    N, Cc, H, W, nscales, sources, automask, near = case
    x, K, invK, disps, poses, am = _bits_inputs(N, Cc, H, W, nscales, sources, automask, near)
    cache, params = _cache_params(K, invK, W, H, N, nscales, automask)
    want = md2hip.loss_tail(disps, poses, x, am, cache, params, visualize=True)
    f2 = x[:, 2].contiguous().clone() if separate else None
    fs = Cc * H * W
    got = L.run_loss_sources(disps, md2hip.pack_poses(poses), x, x.data_ptr() + 4 * fs, 3 * fs,
                             _two_learned(x, cache, f2), 2, 2, am, cache, params, visualize=True)
    torch.cuda.synchronize()
    return want, got


@pytest.mark.parametrize("name", list(S2_CASES))
def test_two_learned_sources_give_the_packed_kernels_bits(name):
    want, got = _s2_pair(S2_CASES[name], separate=False)
    _assert_same_bits(want, got)


def test_a_source_addressed_by_its_own_pointer_gives_the_same_bits():
    """Frame 2 copied into a separate [N,C,H,W] tensor (sample stride C*H*W)."""
    want, got = _s2_pair(S2_CASES["ragged"], separate=True)
    _assert_same_bits(want, got)


# ---- S = 3 (MS) and S = 1 (S) against the fp64 oracle -----------------------------------------
def _stereo_inputs(N, Cc, H, W, strict):
    x3 = D.triplets(N, Cc, H, W, seed=7, ramp_sources=strict)
    xs = D.triplets(N, Cc, H, W, seed=29, ramp_sources=strict)[:, 0]
    K, invK = D.intrinsics(W, H)
    disps = D.disparities(N, H, W, seed=11)
    poses = D.poses(N, seed=13)
    tx = D.fp32_grid(torch.tensor([0.1 * (-1) ** i for i in range(N)], dtype=torch.float64))
    return x3, xs, K, invK, disps, poses, tx


def _stereo_Rt(tx):
    Rt = torch.zeros(len(tx), 12, dtype=torch.float32)
    Rt[:, 0] = Rt[:, 4] = Rt[:, 8] = 1
    Rt[:, 9] = tx.float()
    return Rt.to(DEV)


def _gpu_stereo(disps, poses, x3, xs, tx, K, invK, am, temporal, visualize=True):
    import md2hip
    N, _, Cc, H, W = x3.shape
    cache, params = _cache_params(K, invK, W, H, N, len(disps), am is not None)
    r = md2hip.loss_tail([d.float().to(DEV).contiguous() for d in disps],
                         [(a.float().to(DEV), b.float().to(DEV)) for a, b in poses],
                         x3.float().to(DEV).contiguous(),
                         None if am is None else am.float().to(DEV).contiguous(), cache, params,
                         visualize=visualize, x_stereo=xs.float().to(DEV).contiguous(),
                         stereo_Rt=_stereo_Rt(tx), temporal=temporal)
    torch.cuda.synchronize()
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else (None if v is None else v.cpu()))
            for k, v in r.items()}


def _oracle(disps, poses, x, K, invK, am, ids, forced_sel=None, forced_cells=None):
    """poses: the learned ones first, the stereo pose (zeros, (t_x, 0, 0)) last -- data, no grad."""
    disps = [d.clone().requires_grad_(True) for d in disps]
    poses = [(r.clone().requires_grad_(True), t.clone().requires_grad_(True)) for r, t in poses[:-1]] + [poses[-1]]
    N, L, Cc, H, W = x.shape
    cache = O.TrainCache(K=K, invK=invK, scales=SCALES, source_ids=ids)
    p = O.Params(target_size=(W, H), batch_size=N, automasking=am is not None, disparity_smoothness=1e-3)
    per_source = []
    loss = O.loss_from_outputs(disps, poses, x, am, cache, p, forced_sel=forced_sel,
                               per_source=per_source, forced_cells=forced_cells)
    loss.backward()
    return loss.detach(), [d.grad for d in disps], poses, per_source


def _check_stereo(N, Cc, H, W, strict, temporal, automask=False):
    x3, xs, K, invK, disps, poses, tx = _stereo_inputs(N, Cc, H, W, strict)
    x4 = torch.cat([x3, xs.unsqueeze(1)], 1)
    ids = (1, 3, 4) if temporal else (4,)
    S = len(ids)
    t_st = torch.zeros(N, 3, dtype=torch.float64)
    t_st[:, 0] = tx
    oposes = (list(poses) if temporal else []) + [(torch.zeros(N, 3, dtype=torch.float64), t_st)]
    am = O.automasking_loss(x4, x4[:, 1], ids).detach() if automask else None
    g = _gpu_stereo(disps, poses, x3, xs, tx, K, invK, am, temporal)
    _, _, _, per_src = _oracle(disps, oposes, x4, K, invK, am, ids)
    forced = []
    npix = N * H * W
    for s in range(len(SCALES)):
        ls = per_src[s]
        sel = g["vis_sel"][s].unsqueeze(1).long()              # [N,1,H,W], -1 = automask
        lmin, ref = ls[0], torch.zeros_like(sel)
        for j in range(1, S):
            ref = torch.where(ls[j] < lmin, torch.full_like(ref, j), ref)
            lmin = torch.where(ls[j] < lmin, ls[j], lmin)
        if am is not None:
            ref = torch.where(~(lmin < am), torch.full_like(ref, -1), ref)
        tie = torch.zeros_like(sel, dtype=torch.bool)
        for i in range(S):
            for j in range(i + 1, S):
                tie |= (ls[i] - ls[j]).abs() <= 1e-4 * torch.maximum(ls[i], ls[j])
        if am is not None:
            tie |= (lmin - am).abs() <= 1e-4 * am.abs().clamp_min(1e-12)
        ntie = tie.sum().item()
        shares = {j: (sel == j).sum().item() / npix for j in (list(range(S)) + ([-1] if am is not None else []))}
        print(f"scale {s}: near ties {ntie / npix:.4%}, shares {shares}")
        # conditions under which the comparison below cannot hide a failure
        assert ntie <= 0.01 * npix, (s, ntie)
        if S > 1 or am is not None:
            for j, sh in shares.items():
                assert sh >= 0.10, (s, j, sh)
        mism = (sel != ref) & ~tie
        assert mism.sum().item() == 0, (s, mism.sum().item())
        forced.append(sel + (1 if am is not None else 0))
    lo, dd_o, op, _ = _oracle(disps, oposes, x4, K, invK, am, ids, forced_sel=forced,
                              forced_cells=g["vis_cell"])
    rel = abs(g["loss"].item() - lo.item()) / abs(lo.item())
    errs = [D.rel_err(g["d_disp"][s], dd_o[s]) for s in range(len(SCALES))]
    print(f"loss rel {rel:.3e}, d_disp rel {['%.3e' % e for e in errs]}")
    assert rel <= 2e-5, (g["loss"].item(), lo.item())
    for s, e in enumerate(errs):
        assert e < 2e-4, (s, e)
    if temporal:
        dp_o = torch.cat([torch.cat([r.grad, t.grad], 1) for r, t in op[:2]], 0)
        assert g["d_pose"].shape == (2 * N, 6)
        e = D.rel_err(g["d_pose"], dp_o)
        print(f"d_pose rel {e:.3e}")
        assert e < 2e-4, e
    else:
        assert g["d_pose"] is None
    assert g["vis_warped"].shape == (S, N, Cc, H, W)
    assert g["vis_cell"].shape == (len(SCALES), S, N, H, W)


STEREO_CASES = [(2, 3, 32, 64, True, False), (2, 3, 32, 64, False, False), (2, 1, 32, 64, False, False),
                (3, 3, 40, 72, False, True)]


@pytest.mark.parametrize("N,C,H,W,strict,automask", STEREO_CASES)
def test_ms_three_sources_against_the_oracle(N, C, H, W, strict, automask):
    _check_stereo(N, C, H, W, strict, temporal=True, automask=automask)


@pytest.mark.parametrize("N,C,H,W,strict,automask", STEREO_CASES)
def test_s_stereo_source_alone_against_the_oracle(N, C, H, W, strict, automask):
    _check_stereo(N, C, H, W, strict, temporal=False, automask=automask)


def test_d_pose_shape_and_the_fixed_transform_is_read():
    N, Cc, H, W = 2, 3, 32, 64
    x3, xs, K, invK, disps, poses, tx = _stereo_inputs(N, Cc, H, W, False)
    ms = _gpu_stereo(disps, poses, x3, xs, tx, K, invK, None, True, visualize=False)
    ms_neg = _gpu_stereo(disps, poses, x3, xs, -tx, K, invK, None, True, visualize=False)
    assert ms["d_pose"].shape == (2 * N, 6) and torch.isfinite(ms["d_pose"]).all()
    assert ms["d_pose"].abs().max().item() > 0
    assert ms["loss"].item() != ms_neg["loss"].item()
    s = _gpu_stereo(disps, poses, x3, xs, tx, K, invK, None, False, visualize=False)
    s_neg = _gpu_stereo(disps, poses, x3, xs, -tx, K, invK, None, False, visualize=False)
    assert s["d_pose"] is None
    assert s["loss"].item() != s_neg["loss"].item()
    # S mode does not read the poses at all
    other = [(a + 1.0, b - 1.0) for a, b in poses]
    s_other = _gpu_stereo(disps, other, x3, xs, tx, K, invK, None, False, visualize=False)
    assert torch.equal(s["loss"], s_other["loss"])
    for u, v in zip(s["d_disp"], s_other["d_disp"]):
        assert torch.equal(u, v)


def test_ms_with_the_stereo_source_first_gives_the_same_values():
    """The same three sources in the order (stereo, src0 block 0, src1 block 1): not learned-first, so
    the learned Rt / dRt rows are staged through copies.  The depth cotangent sums its sources in
    the order given, so values, not bits: this file's bounds.  d_pose is in pose-block order."""
    import md2hip
    from md2hip import _lib
    from md2hip import loss as L
    N, Cc, H, W = 2, 3, 32, 64
    x3, xs, K, invK, disps, poses, tx = _stereo_inputs(N, Cc, H, W, False)
    cache, params = _cache_params(K, invK, W, H, N, len(disps), False)
    dd = [d.float().to(DEV).contiguous() for d in disps]
    pp = [(a.float().to(DEV), b.float().to(DEV)) for a, b in poses]
    x, xst, Rt = x3.float().to(DEV).contiguous(), xs.float().to(DEV).contiguous(), _stereo_Rt(tx)
    want = md2hip.loss_tail(dd, pp, x, None, cache, params, x_stereo=xst, stereo_Rt=Rt)
    fs = Cc * H * W
    arr = (_lib.LossSource * _lib.MAX_SOURCES)()
    arr[0].frames, arr[0].sample_stride, arr[0].pose_block, arr[0].Rt = xst.data_ptr(), fs, -1, Rt.data_ptr()
    for s, sid in enumerate(cache.source_ids):
        arr[1 + s].frames, arr[1 + s].sample_stride = x.data_ptr() + 4 * (sid - 1) * fs, 3 * fs
        arr[1 + s].pose_block, arr[1 + s].invert = s, int(sid < cache.target_id)
    got = L.run_loss_sources(dd, md2hip.pack_poses(pp), x, x.data_ptr() + 4 * fs, 3 * fs, arr, 3, 2, None,
                             cache, params)
    torch.cuda.synchronize()
    rel = abs(got["loss"].item() - want["loss"].item()) / abs(want["loss"].item())
    errs = [D.rel_err(u.cpu(), v.cpu()) for u, v in zip(got["d_disp"], want["d_disp"])]
    ep = D.rel_err(got["d_pose"].cpu(), want["d_pose"].cpu())
    print(f"loss rel {rel:.3e}, d_disp rel {['%.3e' % e for e in errs]}, d_pose rel {ep:.3e}")
    assert rel <= 2e-5, (got["loss"].item(), want["loss"].item())
    for s, e in enumerate(errs):
        assert e < 2e-4, (s, e)
    assert got["d_pose"].shape == (2 * N, 6) and ep < 2e-4, ep


def test_loss_tail_refuses_a_malformed_stereo_source():
    import md2hip
    N, Cc, H, W = 2, 3, 32, 64
    x3, xs, K, invK, disps, poses, tx = _stereo_inputs(N, Cc, H, W, False)
    cache, params = _cache_params(K, invK, W, H, N, 4, False)
    dd = [d.float().to(DEV).contiguous() for d in disps]
    pp = [(a.float().to(DEV), b.float().to(DEV)) for a, b in poses]
    x = x3.float().to(DEV).contiguous()
    good, Rt = xs.float().to(DEV).contiguous(), _stereo_Rt(tx)
    for bad_x, bad_Rt in ((good[:, :, :-1].contiguous(), Rt), (good.double(), Rt), (good.cpu(), Rt),
                          (good, Rt[:, :9].contiguous()), (good, Rt.double()), (good, None),
                          (good.transpose(2, 3), Rt)):
        with pytest.raises(ValueError):
            md2hip.loss_tail(dd, pp, x, None, cache, params, x_stereo=bad_x, stereo_Rt=bad_Rt)
    with pytest.raises(ValueError):
        md2hip.loss_tail(dd, pp, x, None, cache, params, stereo_Rt=Rt)
    with pytest.raises(ValueError):
        md2hip.loss_tail(dd, pp, x, None, cache, params, temporal=False)


# ---- md2_automasking_loss_sources ---------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 64), (3, 1, 40, 72)])
def test_automask_two_sources_give_md2_automasking_loss_bits(N, C, H, W):
    from md2hip import _lib
    from md2hip import primitives as Pm
    from md2hip._lib import check, lib, ptr, stream_of
    x = D.triplets(N, C, H, W, seed=7).float().to(DEV).contiguous()
    want = Pm.automasking_loss(x, 2, (1, 3))
    fs = C * H * W
    arr = (_lib.LossSource * _lib.MAX_SOURCES)()
    for s, f in enumerate((0, 2)):
        arr[s].frames, arr[s].sample_stride, arr[s].pose_block = x.data_ptr() + 4 * f * fs, 3 * fs, -1
    got = torch.empty_like(want)
    check(lib().md2_automasking_loss_sources(2, arr, C_void(x.data_ptr() + 4 * fs), 3 * fs, N, C, H, W,
                                             ptr(got), stream_of(x.device)))
    torch.cuda.synchronize()
    assert torch.equal(want, got)


def C_void(addr):
    return C.c_void_p(addr)


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 64), (3, 1, 40, 72)])
def test_automask_three_sources_against_the_oracle(N, C, H, W):
    """The tolerance of the existing automask test (tests/test_gpu_ops.py): relative Frobenius 1e-5."""
    from md2hip import primitives as Pm
    x3 = D.triplets(N, C, H, W, seed=7).float().double()
    xs = D.triplets(N, C, H, W, seed=29)[:, 0].float().double()
    x4 = torch.cat([x3, xs.unsqueeze(1)], 1)
    ref = O.automasking_loss(x4, x4[:, 1], (1, 3, 4))
    got = Pm.automasking_loss(x3.float().to(DEV).contiguous(), 2, (1, 3),
                              x_stereo=xs.float().to(DEV).contiguous())
    torch.cuda.synchronize()
    assert got.shape == (N, 1, H, W)
    assert D.rel_err(got.cpu(), ref) < 1e-5
    one = Pm.automasking_loss(x3.float().to(DEV).contiguous(), 2, (), x_stereo=xs.float().to(DEV).contiguous())
    torch.cuda.synchronize()
    assert D.rel_err(one.cpu(), O.automasking_loss(x4, x4[:, 1], (4,))) < 1e-5
