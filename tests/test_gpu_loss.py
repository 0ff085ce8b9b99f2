"""GPU parity of the fused loss tail (md2_loss_fwd_bwd) against the CPU oracle.

Two kinds of branch decision make the exact gradient piecewise smooth, so fp32 and fp64 may
legitimately decide differently at isolated pixels:
  * the per-pixel ``minimum`` over sources (src/training.jl:13-15) at near-ties, and
  * ``grid_sample``'s bilinear cell and border clamp (src/training.jl:56): a sample coordinate
    within fp32 rounding of an integer (or of the border) switches the gradient between cells.
The test therefore checks
  1. the GPU argmin map equals the oracle's except at near-ties (|l0-l1| <= 1e-4 max(l0,l1); fp32
     E[x^2]-E[x]^2 cancellation),
  2. loss / d_disparity / d_pose against the oracle evaluated with the GPU's argmin AND its
     bilinear cells / border states imposed (md2_loss_out.vis_cell, O.grid_sample_border_forced):
     loss rel 2e-5, gradients relative Frobenius error 2e-4 (fp32 accumulation over up to 53k
     pixels) -- for affine-ramp sources, textured sources and the near-field regime alike.
     (Without the imposed cells the textured gradients sit at the fp64 oracle's own conditioning
     floor, up to 2.9e-2: tools/oracle_sensitivity.py.)
"""
import pytest
import torch

from oracle import md2_oracle as O
from tests import _data as D

pytestmark = pytest.mark.gpu

SCALES = (0.125, 0.25, 0.5, 1.0)


def _gpu(disps, poses, x, K, invK, automask, smoothness=1e-3):
    import md2hip
    dev = torch.device("cuda")
    N, L, C, H, W = x.shape
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy(), scales=SCALES)
    params = md2hip.Params(target_size=(W, H), batch_size=N, automasking=automask is not None,
                           disparity_smoothness=smoothness)
    r = md2hip.loss_tail(
        [d.float().to(dev).contiguous() for d in disps],
        [(a.float().to(dev), b.float().to(dev)) for a, b in poses],
        x.float().to(dev).contiguous(),
        None if automask is None else automask.float().to(dev).contiguous(),
        cache, params, visualize=True)
    torch.cuda.synchronize()
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in r.items()}


def _oracle(disps, poses, x, K, invK, automask, forced_sel=None, smoothness=1e-3, forced_cells=None):
    disps = [d.clone().requires_grad_(True) for d in disps]
    poses = [(r.clone().requires_grad_(True), t.clone().requires_grad_(True)) for r, t in poses]
    N, L, C, H, W = x.shape
    cache = O.TrainCache(K=K, invK=invK, scales=SCALES)
    p = O.Params(target_size=(W, H), batch_size=N, automasking=automask is not None,
                 disparity_smoothness=smoothness)
    per_source = []
    loss = O.loss_from_outputs(disps, poses, x, automask, cache, p, forced_sel=forced_sel,
                               per_source=per_source, forced_cells=forced_cells)
    loss.backward()
    dpose = torch.cat([torch.cat([r.grad, t.grad], 1) for r, t in poses], 0)
    return loss.detach(), [d.grad for d in disps], dpose, per_source


def _check(N, C, H, W, automask=False, seed=7, strict=True, near=False):
    """near=False: depth 1-9 m, forward/backward motion 0.3 m.  near=True: the untrained-network
    regime (sigmoid disparities ~0.1-0.9 => depth 0.1-1 m) with 2 cm motion."""
    x = D.triplets(N, C, H, W, seed=seed, ramp_sources=strict)
    K, invK = D.intrinsics(W, H)
    if near:
        disps = D.disparities(N, H, W, seed=seed + 4, lo=0.1, hi=0.9)
        poses = D.poses(N, seed=seed + 6, forward=0.02, jitter=0.005)
    else:
        disps = D.disparities(N, H, W, seed=seed + 4)
        poses = D.poses(N, seed=seed + 6)
    am = O.automasking_loss(x, x[:, 1], (1, 3)).detach() if automask else None
    _check_inputs(disps, poses, x, K, invK, am)


def _check_inputs(disps, poses, x, K, invK, am, smoothness=1e-3):
    """The procedure of the module docstring on given inputs (tests/test_gpu_loss_smooth.py runs it
    at a smoothness weight that makes both gradient passes comparable)."""
    g = _gpu(disps, poses, x, K, invK, am, smoothness=smoothness)
    _, _, _, per_src = _oracle(disps, poses, x, K, invK, am, smoothness=smoothness)
    forced = []
    for s in range(len(SCALES)):
        l0, l1 = per_src[s][0], per_src[s][1]
        sel = g["vis_sel"][s].unsqueeze(1).long()              # [N,1,H,W], -1 = automask
        ref = (l1 < l0).long()
        if am is not None:
            lmin = torch.minimum(l0, l1)
            ref = torch.where(~(lmin < am), torch.full_like(ref, -1), ref)
        tie = (l0 - l1).abs() <= 1e-4 * torch.maximum(l0, l1)
        if am is not None:
            tie |= (torch.minimum(l0, l1) - am).abs() <= 1e-4 * am.abs().clamp_min(1e-12)
        mism = (sel != ref) & ~tie
        assert mism.sum().item() == 0, (s, mism.sum().item())
        forced.append(sel + (1 if am is not None else 0))
    lo, dd_o, dp_o, _ = _oracle(disps, poses, x, K, invK, am, forced_sel=forced, smoothness=smoothness,
                                forced_cells=g["vis_cell"])
    assert abs(g["loss"].item() - lo.item()) <= 2e-5 * abs(lo.item()), (g["loss"].item(), lo.item())
    tol_d, tol_p = 2e-4, 2e-4
    for s in range(len(SCALES)):
        e = D.rel_err(g["d_disp"][s], dd_o[s])
        assert e < tol_d, (s, e)
    e = D.rel_err(g["d_pose"], dp_o)
    assert e < tol_p, e


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 64), (2, 1, 32, 64), (1, 3, 128, 416), (2, 3, 128, 416)])
def test_loss_tail_parity_strict(N, C, H, W):
    _check(N, C, H, W, strict=True)


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 64), (1, 3, 128, 416), (4, 3, 128, 416), (2, 1, 128, 416)])
def test_loss_tail_parity_texture(N, C, H, W):
    _check(N, C, H, W, strict=False)


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 128, 416)])
def test_loss_tail_parity_texture_near(N, C, H, W):
    _check(N, C, H, W, strict=False, near=True)


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 64), (1, 3, 128, 416)])
def test_loss_tail_parity_near(N, C, H, W):
    _check(N, C, H, W, strict=True, near=True)


def test_loss_tail_automask():
    _check(2, 3, 32, 64, automask=True)
    _check(2, 3, 32, 64, automask=True, strict=False)


def test_loss_tail_ragged_tiles():
    """Sizes that are not multiples of the 32x8 / 64x4 tiles (partial edge tiles)."""
    _check(3, 3, 40, 72, seed=21)


def test_so3_compose_roundtrip():
    """so3_exp_map / composeT forward against the oracle (test/runtests.jl:14-50 semantics)."""
    import md2hip
    from md2hip._lib import check, lib, ptr, stream_of
    N = 5
    poses = D.poses(N, seed=3)
    pose = md2hip.pack_poses([(r.float(), t.float()) for r, t in poses]).cuda()
    Rt = torch.empty(2 * N, 12, dtype=torch.float32, device="cuda")
    check(lib().md2_so3_compose_fwd(ptr(pose), N, 1, ptr(Rt), stream_of()))
    torch.cuda.synchronize()
    for s, (r, t) in enumerate(poses):
        R, tt = O.composeT(r, t, s == 0)
        got = Rt[s * N:(s + 1) * N].cpu().double()
        assert torch.allclose(got[:, :9].view(N, 3, 3), R, atol=1e-6)
        assert torch.allclose(got[:, 9:], tt, atol=1e-6)


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 64), (2, 1, 32, 64), (1, 3, 128, 416)])
def test_loss_tail_vis_outputs(N, C, H, W):
    """train_loss visualisation outputs (src/training.jl:71-74): both sources warped by the last
    scale against the oracle's ``warp`` (fp32 vs fp64 on kink-free ramp sources: rel 1e-5), and
    the last scale's per-pixel warp-loss map whose mean is that scale's warp term."""
    x = D.triplets(N, C, H, W, seed=5, ramp_sources=True)
    K, invK = D.intrinsics(W, H)
    disps = D.disparities(N, H, W, seed=9)
    poses = D.poses(N, seed=15)
    g = _gpu(disps, poses, x, K, invK, None)
    assert g["vis_warped"].shape == (2, N, C, H, W)
    d = disps[-1]
    if d.shape[-2:] != (H, W):
        d = O.upsample_bilinear_size(d, (H, W))
    Ps = O.poses_to_transforms(poses, (1, 3), 2)
    ref = O.warp(d, x, Ps, K, invK, (1, 3), 0.1, 100.0)
    for s in range(2):
        assert D.rel_err(g["vis_warped"][s], ref[s]) < 1e-5, s
    vl = g["vis_loss"][-1]
    assert abs(vl.double().mean().item() - g["terms"][-1, 0].item()) <= 1e-5 * abs(g["terms"][-1, 0].item())
