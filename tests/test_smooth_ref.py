"""The inputs and the fp64 reference of tests/test_gpu_loss_smooth.py, checked on the CPU: the
preconditions that make the smoothness term of the loss tail testable at full weight, the
reference against the oracle, and the proof that the inputs have teeth.

Teeth.  Each deliberately wrong variant of the reference (tests/_smooth_ref.py VARIANTS) must move
at least one scale's d_disp or term by at least 100 x the bound the GPU test applies to that scale
(max(1e-5, 4 x fp32 floor)), on every case to which it applies:
  * abs0_plus (abs'(0) = +1) needs exact-zero differences whose gradient survives the upsample
    adjoint: A1-A3 (the planted flat patch).  Family B has no zero difference by construction; in
    A4 the zeros are whole constant columns / maps, whose +1/-1 pairs telescope to zero in the
    adjoint.
  * drop_row_seams needs vertical differences: not A4, whose scales are one row high (a one-column
    scale, which would have them, is refused by the host entry: test_one_column_scales_are_refused).
  * every other variant applies to all five cases.
Measured worst-scale factors over the bound (fp64, this file's ``-s`` output): const_mean 1.2e4 to
3.8e4, swap_norm 1.4e3 to 1.1e4, abs0_plus 1.4e4 to 3.1e4, edge_left 5.5e2 to 2.4e4, drop_col_seams
6.4e3 to 6.5e4, drop_row_seams 1.2e4 to 1.7e5, prev_weight 1e5 to 7e5.
"""
import functools

import pytest
import torch

from oracle import md2_oracle as O
from tests import _data as D
from tests import _smooth_ref as S

NAMES = tuple(S.CASES)
TEETH_FACTOR = 100.0
APPLIES = {v: NAMES for v in S.VARIANTS}
APPLIES["abs0_plus"] = ("A1", "A2", "A3")
APPLIES["drop_row_seams"] = ("A1", "A2", "A3", "B")


@functools.lru_cache(maxsize=None)
def _case(name):
    disps, x, w = S.case_inputs(name)
    terms, loss, grads = S.reference(disps, x, w)
    fd, ft = S.fp32_floor(disps, x, w)
    return disps, x, w, terms, loss, grads, fd, ft


@pytest.mark.parametrize("name", ["A1", "A2", "A3", "A4"])
def test_family_a_is_exact(name):
    N, C, H, W, shapes = S.CASES[name]
    disps = _case(name)[0]
    for s, d in enumerate(disps):
        k = d * 1024.0
        assert torch.equal(k, k.round()) and d.min() >= 0.1 and d.max() <= 0.9, s
        assert torch.equal(d.float().double(), d), s
        up32, up64 = S.upsampled(d.float(), H, W), S.upsampled(d, H, W)
        assert torch.equal(up32.double(), up64), (name, s)
        dx, dy = S.full_res_differences(d, H, W)
        if S.has_patch(*shapes[s]):
            assert (dx == 0).sum().item() > 0 and (dy == 0).sum().item() > 0, (name, s)
            # the smallest non-zero difference is far above fp32 resolution at these magnitudes
            assert min(dx[dx != 0].abs().min().item(), dy[dy != 0].abs().min().item()) >= 2.0 ** -16


def test_family_b_keeps_its_signs():
    N, C, H, W, shapes = S.CASES["B"]
    disps = _case("B")[0]
    worst = float("inf")
    for s, d in enumerate(disps):
        assert torch.equal(d.float().double(), d), s
        dx, dy = S.full_res_differences(d, H, W)
        mean = S.upsampled(d, H, W).mean().item()
        worst = min(worst, dx.abs().min().item() / mean, dy.abs().min().item() / mean)
        for n in range(N):
            sx, sy = torch.sign(dx[n]), torch.sign(dy[n])
            assert (sx == sx.flatten()[0]).all() and (sy == sy.flatten()[0]).all(), (s, n)
            assert sx.flatten()[0] == -sy.flatten()[0], (s, n)
        assert torch.sign(dx[0]).flatten()[0] == -torch.sign(dx[1]).flatten()[0], s
    print(f"family B: min |delta| / mean = {worst:.2e}")
    assert worst >= 1e-4


@pytest.mark.parametrize("name", NAMES)
def test_sources_isolate_the_smoothness_gradient(name):
    """With constant sources the oracle's d_disp and d_pose are exactly zero at smoothness 0, in
    fp64 and fp32, and its photometric term is not."""
    N, C, H, W, shapes = S.CASES[name]
    disps, x, w = _case(name)[:3]
    K, invK = D.intrinsics(W, H)
    for dt in (torch.float64, torch.float32):
        dd = [d.to(dt).clone().requires_grad_(True) for d in disps]
        poses = [(r.to(dt).requires_grad_(True), t.to(dt).requires_grad_(True)) for r, t in D.poses(N)]
        cache = O.TrainCache(K=K.to(dt), invK=invK.to(dt), scales=tuple(w))
        p = O.Params(target_size=(W, H), batch_size=N, automasking=False, disparity_smoothness=0.0)
        loss = O.loss_from_outputs(dd, poses, x.to(dt), None, cache, p)
        loss.backward()
        assert loss.item() > 1e-2
        for d in dd:
            assert d.grad is None or (d.grad == 0).all()
        for r, t in poses:
            assert (r.grad is None or (r.grad == 0).all()) and (t.grad is None or (t.grad == 0).all())


@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_oracle(name):
    N, C, H, W, shapes = S.CASES[name]
    disps, x, w, terms, loss, grads = _case(name)[:6]
    K, invK = D.intrinsics(W, H)
    dd = [d.clone().requires_grad_(True) for d in disps]
    # weights through the oracle's own product disparity_smoothness * scale
    cache = O.TrainCache(K=K, invK=invK, scales=tuple(wi / S.SMOOTHNESS for wi in w))
    p = O.Params(target_size=(W, H), batch_size=N, automasking=False, disparity_smoothness=S.SMOOTHNESS)
    lo, parts = O.loss_from_outputs(dd, D.poses(N), x, None, cache, p, return_parts=True)
    lo.backward()
    photo = sum(pw for pw, _ in parts)
    assert abs((lo - photo / len(w)).item() - loss.item()) <= 1e-12 * abs(lo.item())
    for s in range(len(w)):
        assert abs(parts[s][1].item() - terms[s].item()) <= 1e-12 * max(abs(terms[s].item()), 1e-300), s
        if grads[s].norm().item() == 0.0:
            assert (dd[s].grad == 0).all(), s
        else:
            assert D.rel_err(dd[s].grad, grads[s]) <= 1e-12, s


def test_restated_smooth_loss_is_the_oracles():
    """The breakable restatement the wrong variants are built on equals O.smooth_loss."""
    disps, x, w = _case("A1")[:3]
    H, W = x.shape[-2:]
    for d in disps:
        full = S.upsampled(d, H, W)[:, 0]
        a, b = S._smooth(full, x[:, 1]), O.smooth_loss(full, x[:, 1])
        assert abs(a.item() - b.item()) <= 1e-14 * abs(b.item())


def test_reference_options():
    """divisor / dloss scale the gradient and leave the terms; sigmoid_grad multiplies by d (1 - d);
    a zero weight empties its scale."""
    disps, x, w, terms, loss, grads = _case("A1")[:6]
    t2, l2, g2 = S.reference(disps, x, w, divisor=3, dloss=2.5)
    assert torch.equal(t2, terms) and abs(l2.item() - terms.sum().item() / 3) <= 1e-15
    for a, b in zip(g2, grads):
        assert D.rel_err(a, b * (2.5 / 3) * len(w)) <= 1e-14
    _, _, g3 = S.reference(disps, x, w, sigmoid_grad=True)
    for a, b, d in zip(g3, grads, disps):
        assert torch.equal(a, b * d * (1 - d))
    w0 = (w[0], 0.0, w[2], w[3])
    t4, _, g4 = S.reference(disps, x, w0)
    assert t4[1].item() == 0.0 and (g4[1] == 0).all() and g4[0].norm() > 0


def test_a4_known_answers():
    """The constant first scale is constant after the upsample: term and gradient exactly zero.  The
    other one-row scales have identical rows: no vertical contribution."""
    N, C, H, W, shapes = S.CASES["A4"]
    disps, x, w, terms, loss, grads = _case("A4")[:6]
    assert terms[0].item() == 0.0 and (grads[0] == 0).all()
    for s in (1, 2):
        dx, dy = S.full_res_differences(disps[s], H, W)
        assert (dy == 0).all() and (dx != 0).any()
        assert terms[s].item() > 0 and grads[s].norm().item() > 0


@pytest.mark.parametrize("form", ["plain", "sources"])
@pytest.mark.parametrize("shapes", S.A4_REJECTED)
def test_one_column_scales_are_refused(shapes, form):
    """A one-column disparity map is unsupported by design (the photometric pass loads column
    pairs): both host entries refuse it with an argument error before anything is launched, so no
    device is needed and the (never dereferenced) pointers may be host addresses."""
    import ctypes as C
    from md2hip._lib import LossCfg, LossOut, LossSource, MAX_SOURCES, lib
    N, Cc, H, W, _ = S.CASES["A4"]
    buf = (C.c_char * 256)()
    p = C.c_void_p(C.addressof(buf))
    c = LossCfg(n=N, c=Cc, width=W, height=H, nscales=len(shapes), divisor=float(len(shapes)),
                min_depth=0.1, max_depth=100.0, smooth_normalize=1)
    for s, (h, w) in enumerate(shapes):
        c.scale_w[s], c.scale_h[s] = w, h
    o = LossOut()
    o.loss = p.value
    darr = C.cast((C.c_void_p * 5)(*([p.value] * 5)), C.POINTER(C.c_void_p))
    if form == "plain":
        rc = lib().md2_loss_fwd_bwd(C.byref(c), darr, p, p, None, C.c_float(1.0), C.byref(o), p, None)
    else:
        arr = (LossSource * MAX_SOURCES)()
        arr[0].frames, arr[0].sample_stride, arr[0].pose_block, arr[0].Rt = p.value, Cc * H * W, -1, p.value
        rc = lib().md2_loss_fwd_bwd_sources(C.byref(c), 1, arr, p, 3 * Cc * H * W, darr, None, None,
                                            C.c_float(1.0), C.byref(o), p, None)
    assert rc == 1 and b"scale dims" in lib().md2_last_error(), lib().md2_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor(name):
    """The floor the GPU bounds are built on; it leaves the 1e-5 of md2_smooth_loss_* in force."""
    fd, ft = _case(name)[6:]
    print(f"{name}: fp32 floor d_disp " + ", ".join(f"{v:.1e}" for v in fd)
          + " | terms " + ", ".join(f"{v:.1e}" for v in ft))
    assert max(fd + ft) < 2.5e-6


@pytest.mark.parametrize("name,variant", [(n, v) for v in S.VARIANTS for n in APPLIES[v]])
def test_wrong_variants_are_caught(name, variant):
    disps, x, w, terms, loss, grads, fd, ft = _case(name)
    tv, _, gv = S.reference(disps, x, w, variant=variant)
    factors = []
    for s in range(len(w)):
        if grads[s].norm().item() == 0.0:       # A4's constant scale: any change at all counts
            factors.append(float("inf") if gv[s].norm().item() > 0 or tv[s].item() != 0 else 0.0)
            continue
        factors.append(max(D.rel_err(gv[s], grads[s]) / S.bound(fd[s]),
                           S.rel(tv[s], terms[s]) / S.bound(ft[s])))
    print(f"{name} {variant}: x bound per scale " + ", ".join(f"{f:.0f}" for f in factors))
    assert max(factors) >= TEETH_FACTOR, (name, variant, factors)
