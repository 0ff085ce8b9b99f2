"""The smoothness path of the fused loss tail (disp_sum_kernel, smooth_kernel, up_adjoint_kernel,
loss_finalize_kernel behind md2_loss_fwd_bwd / md2_loss_fwd_bwd_sources) at full weight against the
fp64 reference of tests/_smooth_ref.py.

tests/test_gpu_loss.py sees this path multiplied by disparity_smoothness * scale = 1.25e-4 .. 1e-3,
where it is 2e-4 of the loss and 7e-5 .. 3e-2 of d_disp.  Here the two source frames are constant,
so the photometric d_disp and d_pose are exactly zero and d_disp IS the smoothness gradient; the
disparities (families A and B of tests/_smooth_ref.py) keep every sign decision identical in fp32
and fp64, so nothing is masked.  tests/test_smooth_ref.py proves on the CPU that these inputs catch
seven wrong forms of the term by 100 x the bounds used here.

Cases (N, C, H, W; scales): _smooth_ref.CASES.  A1 two 62-column seams with a one-column third
tile, a one-row second row block, dw == W with dh != H; A2 smooth_kernel<1>, one block, a one-row
last band; A3 five scales (MAX_SCALES) and one scale; A4 the in == 1 paths of the upsample and its
adjoint that exist, dh == 1 (with dw < W and dw == W) -- a one-column map is refused by the host
entry, which is tested instead; B the model's non-dyadic ratios.

Bounds.  terms[:,1] and d_disp (relative Frobenius) per scale: max(1e-5, 4 x fp32 floor), the floor
being the reference evaluated by torch in fp32 against itself in fp64 on the same inputs and
options, computed here per case.  terms[:,0] 1e-5 and loss 2e-5 against the oracle, as in
tests/test_gpu_loss.py.  A quantity whose reference is exactly zero (a zero weight, A4's constant
scale) must be exactly zero.

Measured on an MI355X, default options, per scale (every floor is below 2.5e-6, so every bound is
1e-5; "0" is an exact zero):
  case  d_disp: fp32 floor                     d_disp: GPU error
  A1    1.8e-7 1.1e-7 7.8e-8 9.2e-8            8.4e-8 1.3e-7 9.5e-8 1.4e-7
  A2    1.1e-7 8.0e-8 5.8e-8 5.0e-8            8.3e-8 1.0e-7 7.8e-8 9.2e-8
  A3    3.3e-7 2.2e-7 1.3e-7 1.0e-7 8.7e-8     1.2e-7 1.1e-7 1.1e-7 9.6e-8 1.1e-7
  A4    0      6.7e-8 1.7e-7                   0      7.1e-8 1.6e-7
  B     2.3e-7 2.7e-7 8.8e-7 2.4e-7            1.3e-7 6.7e-8 1.9e-7 2.6e-7
  case  terms[:,1]: fp32 floor                 terms[:,1]: GPU error
  A1    1.0e-7 5.1e-8 2.5e-8 1.3e-7            1.0e-8 5.1e-8 2.1e-7 6.6e-8
  A2    5.9e-8 2.2e-9 1.5e-7 2.7e-8            5.9e-8 1.2e-7 4.6e-8 4.7e-8
  A3    1.0e-7 8.2e-8 5.6e-8 7.1e-8 2.2e-8     6.1e-9 1.2e-7 5.6e-8 1.2e-8 2.2e-8
  A4    0      1.5e-7 7.2e-8                   0      3.3e-8 1.3e-7
  B     1.3e-7 4.2e-8 2.6e-8 3.8e-8            1.3e-7 4.2e-8 2.6e-8 3.8e-8
terms[:,0] 4.6e-8 .. 2.7e-7 (A4, a 9 x 63 frame: 2.4e-6), loss 6.5e-8 .. 2.4e-6; d_disp and d_pose
of the isolation runs and d_pose of every run exactly 0.  With the options (dloss / divisor, a zero
weight, no normalisation, sigmoid_grad, grads=False, the sources form, one scale) the errors stay
below 2.6e-7 for d_disp and 2.1e-7 for terms[:,1].  Combined case: smoothness share of d_disp 0.50,
0.61, 0.70, 0.69 at disparity_smoothness = 8; it meets the 2e-4 / 2e-5 bounds of tests/test_gpu_loss.py.
"""
import functools

import pytest
import torch

from oracle import md2_oracle as O
from tests import _data as D
from tests import _smooth_ref as S

pytestmark = pytest.mark.gpu

NEAR = dict(forward=0.02, jitter=0.005)      # depth 0.1-1 m at these disparities: 2 cm motion
COMBINED_SMOOTHNESS = 8.0


def _cpu(r):
    return {k: ([None if t is None else t.cpu() for t in v] if isinstance(v, list)
                else (None if v is None else v.cpu())) for k, v in r.items()}


def _gpu(name, disps, x, *, stereo=None, **opts):
    import md2hip
    dev = torch.device("cuda")
    N, L, C, H, W = x.shape
    K, invK = D.intrinsics(W, H)
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy(), scales=S.DEFAULT_SCALES)
    params = md2hip.Params(target_size=(W, H), batch_size=N, automasking=False,
                           disparity_smoothness=S.SMOOTHNESS)
    if len(disps) != len(S.DEFAULT_SCALES) and "smooth_weights" not in opts:
        opts["smooth_weights"] = S.default_weights(name)
    poses = [(a.float().to(dev), b.float().to(dev)) for a, b in D.poses(N, **NEAR)]
    if stereo is not None:
        Rt = torch.from_numpy(md2hip.stereo_transforms(["l"] * N)).to(dev)
        opts.update(x_stereo=stereo.float().to(dev).contiguous(), stereo_Rt=Rt, temporal=False)
    r = md2hip.loss_tail([d.float().to(dev).contiguous() for d in disps], poses,
                         x.float().to(dev).contiguous(), None, cache, params, **opts)
    torch.cuda.synchronize()
    return _cpu(r)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    disps, x, w = S.case_inputs(name)
    N, L, C, H, W = x.shape
    K, invK = D.intrinsics(W, H)
    cache = O.TrainCache(K=K, invK=invK, scales=tuple(w))
    p = O.Params(target_size=(W, H), batch_size=N, automasking=False, disparity_smoothness=0.0)
    with torch.no_grad():
        _, parts = O.loss_from_outputs(disps, D.poses(N, **NEAR), x, None, cache, p, return_parts=True)
    photo = torch.stack([pw for pw, _ in parts])
    return disps, x, w, photo


@functools.lru_cache(maxsize=None)
def _reference(name, weights=None, keep=None, **opts):
    """(terms, loss, grads, floor_d, floor_t) of a case: lru-cached, shared and never modified."""
    disps, x, w, _ = _inputs(name)
    w = w if weights is None else weights
    if keep is not None:
        disps, w = [disps[s] for s in keep], [w[s] for s in keep]
    terms, loss, grads = S.reference(disps, x, w, **opts)
    fd, ft = S.fp32_floor(disps, x, w, **opts)
    return terms, loss, grads, fd, ft


def _err(got, want):
    """Relative (Frobenius) error; a reference that is exactly zero asks for exactly zero."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    if want.norm().item() == 0.0:
        return 0.0 if got.norm().item() == 0.0 else float("inf")
    return D.rel_err(got, want)


def _compare(tag, g, ref, photo, divisor=None, grads=True):
    """Checks 3-5 of a run against (terms, loss, grads, floors); prints every figure, then asserts."""
    terms, _, rgrads, fd, ft = ref
    ns = len(terms)
    divisor = float(ns if divisor is None else divisor)
    bad = []
    for s in range(ns):
        et = _err(g["terms"][s, 1], terms[s])
        ep = _err(g["terms"][s, 0], photo[s])
        line = f"{tag} scale {s}: term floor {ft[s]:.1e} bound {S.bound(ft[s]):.1e} err {et:.1e} | photo err {ep:.1e}"
        if et > S.bound(ft[s]):
            bad.append(("term", s, et))
        if ep > 1e-5:
            bad.append(("photo", s, ep))
        if grads:
            ed = _err(g["d_disp"][s], rgrads[s])
            line += f" | d_disp floor {fd[s]:.1e} bound {S.bound(fd[s]):.1e} err {ed:.1e}"
            if ed > S.bound(fd[s]):
                bad.append(("d_disp", s, ed))
        print(line)
    want = (photo.sum().item() + terms.sum().item()) / divisor
    el = abs(g["loss"].item() - want) / abs(want)
    print(f"{tag} loss err {el:.1e}")
    if el > 2e-5:
        bad.append(("loss", el))
    if grads and g["d_pose"] is not None:
        bad += _pose_is_zero(tag, g, rgrads)
    assert not bad, (tag, bad)


def _pose_is_zero(tag, g, rgrads):
    """Check 2: d_pose is photometric only, so zero: <= 1e-6 x the smallest non-zero smoothness
    gradient norm of the run (exact zero expected)."""
    norms = [r.norm().item() for r in rgrads if r.norm().item() > 0]
    n = g["d_pose"].double().norm().item()
    print(f"{tag} |d_pose| {n:.1e}")
    return [] if n <= 1e-6 * min(norms) else [("d_pose", n)]


@pytest.mark.parametrize("name", list(S.CASES))
def test_smoothness_default_options(name):
    disps, x, w, photo = _inputs(name)
    ref = _reference(name)
    # 1. isolation: without the smoothness term nothing reaches the disparities or the poses
    g0 = _gpu(name, disps, x, smooth_weights=(0.0,) * len(disps))
    bad = _pose_is_zero(name + " iso", g0, ref[2])
    for s in range(len(disps)):
        n, rn = g0["d_disp"][s].double().norm().item(), ref[2][s].norm().item()
        print(f"{name} iso scale {s}: |d_disp| {n:.1e} (smoothness gradient {rn:.1e})")
        if n > 1e-6 * rn:
            bad.append(("iso", s, n))
        assert g0["terms"][s, 1].item() == 0.0
    assert not bad, bad
    # 2.-5.
    g = _gpu(name, disps, x)
    _compare(name, g, ref, photo)
    if name == "A4":
        # 6. known answers: the first scale is constant after the upsample; the others have
        # identical rows, so their terms are the horizontal sums alone (the reference's, asserted
        # vertical-free in tests/test_smooth_ref.py) -- both already held above; exactness here
        assert g["terms"][0, 1].item() == 0.0 and (g["d_disp"][0] == 0).all()


@pytest.mark.parametrize("shapes", S.A4_REJECTED)
def test_one_column_scales_are_refused(shapes):
    """in == 1 along x is unsupported by design (the photometric pass loads column pairs): the tail
    refuses the scale list with an argument error (before any launch: tests/test_smooth_ref.py)."""
    import md2hip
    N, C, H, W, _ = S.CASES["A4"]
    x = S.frames(N, C, H, W)
    disps = S.family_a(N, shapes)
    with pytest.raises(md2hip._lib.MD2Error, match="scale dims"):
        _gpu("A4", disps, x, smooth_weights=(1e-3,) * len(shapes))


OPTIONS = {
    "dloss_divisor": dict(dloss=2.5, divisor=3),
    "zero_weight": dict(smooth_weights=(3e-4, 0.0, 1e-3, 2e-4)),
    "no_normalize": dict(smooth_normalize=False),
    "sigmoid_grad": dict(sigmoid_grad=True),
    "no_grads": dict(grads=False),
}


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("name", ["A1", "B"])
def test_smoothness_options(name, option):
    disps, x, w, photo = _inputs(name)
    opts = dict(OPTIONS[option])
    ropts = {k: v for k, v in opts.items() if k not in ("grads", "smooth_weights")}
    if "smooth_normalize" in ropts:
        ropts["normalize"] = ropts.pop("smooth_normalize")
    ref = _reference(name, weights=opts.get("smooth_weights"), **ropts)
    g = _gpu(name, disps, x, **opts)
    tag = f"{name} {option}"
    _compare(tag, g, ref, photo, divisor=opts.get("divisor"), grads=opts.get("grads", True))
    if option == "dloss_divisor":
        base, bref = _gpu(name, disps, x), _reference(name)
        assert torch.equal(g["terms"], base["terms"])
        assert torch.equal(ref[0], bref[0])
        for s in range(len(disps)):     # the reference's own scaling: 2.5 / 3 against 1 / 4
            assert D.rel_err(ref[2][s], bref[2][s] * (2.5 / 3.0 * len(disps))) <= 1e-14
    if option == "zero_weight":
        assert g["terms"][1, 1].item() == 0.0 and (g["d_disp"][1] == 0).all()
    if option == "no_grads":
        assert all(d is None for d in g["d_disp"]) and g["d_pose"] is None


def test_smoothness_through_the_sources_form():
    """A1 through md2_loss_fwd_bwd_sources, the "S" tail: one fixed (stereo) source, a constant
    frame, no learned pose.  The smoothness result is that of the plain run."""
    disps, x, w, _ = _inputs("A1")
    N, L, C, H, W = x.shape
    xs = D.fp32_grid(torch.full((N, C, H, W), 0.45, dtype=torch.float64))
    photo = O.photometric_loss(xs, x[:, 1]).mean().expand(len(disps))
    g = _gpu("A1", disps, x, stereo=xs)
    assert g["d_pose"] is None
    _compare("A1 sources", g, _reference("A1"), photo)


def test_smoothness_one_scale():
    """A3's full-resolution scale alone: the direct (dw == W, dh == H) path with the mean
    normalisation, nscales = 1."""
    disps, x, w, photo = _inputs("A3")
    g = _gpu("A3", disps[4:], x, smooth_weights=w[4:])
    _compare("A3 one scale", g, _reference("A3", keep=(4,)), photo[4:])


def test_smoothness_and_photometric_gradients_together():
    """Family-B disparities, textured sources, near-field poses and disparity_smoothness = 8 through
    the procedure of tests/test_gpu_loss.py (GPU argmin and cells imposed on the oracle, loss 2e-5,
    gradients 2e-4): the one place where the photometric and the smoothness pass write comparable
    magnitudes into the same full-resolution gradient.  The oracle's smoothness share of each
    scale's d_disp, |g_smooth| / (|g_smooth| + |g_photo|), must lie in 10 % .. 90 % (fp64: 0.50,
    0.61, 0.70, 0.69)."""
    from tests.test_gpu_loss import _check_inputs, _oracle
    N, C, H, W, shapes = S.CASES["B"]
    disps = S.family_b(N, shapes)
    x = D.triplets(N, C, H, W, seed=7)
    K, invK = D.intrinsics(W, H)
    poses = D.poses(N, **NEAR)
    _, g_photo, _, _ = _oracle(disps, poses, x, K, invK, None, smoothness=0.0)
    _, g_all, _, _ = _oracle(disps, poses, x, K, invK, None, smoothness=COMBINED_SMOOTHNESS)
    for s in range(len(disps)):
        ns, npz = (g_all[s] - g_photo[s]).norm().item(), g_photo[s].norm().item()
        share = ns / (ns + npz)
        print(f"combined scale {s}: smoothness share of d_disp {share:.3f}")
        assert 0.1 <= share <= 0.9, (s, share)
    _check_inputs(disps, poses, x, K, invK, None, smoothness=COMBINED_SMOOTHNESS)
