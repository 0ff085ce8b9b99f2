"""The gradient guard on the device (md2_grad_norm, md2_adam_guarded, md2_model_set_grad_guard;
include/md2.h) against its NumPy restatement (tests/_grad_guard_ref.py) and against the plain step.

Every comparison here is of bytes: the sum of squares has a stated order, the finish is a handful of
correctly rounded operations, and a guarded step that clips nothing and skips nothing is the plain
step.  Model cases: ResNet-18, N = 2, 64 x 128."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import _data as D
from tests import _grad_guard_ref as R

pytestmark = pytest.mark.gpu

MD2_ENOTSUP, MD2_ESTATE = 3, 5
N, H, W = 2, 64, 128
SIZES = [1, 255, 256, 257, 4096, 4097, 1024 * 1024 + 5, 4 * 1024 * 1024 + 3]


def _state(t):
    """a 40-byte uint8 state tensor -> a STATE_DTYPE record (synchronises)"""
    return np.frombuffer(t.cpu().numpy().tobytes(), R.STATE_DTYPE)[0]


def _same_state(a, b, what=""):
    for f in R.STATE_DTYPE.names:
        assert a[f].tobytes() == b[f].tobytes(), (what, f, a[f], b[f])


def _vector(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32)


# ---- the primitive ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_equals_the_restatement(n):
    import md2hip
    from md2hip._lib import lib
    g = _vector(n, n)
    S, c = R.sumsq_ordered(g)
    half = float(np.float32(R.finish(S, c)["norm"]) / np.float32(2))
    gd = torch.from_numpy(g).cuda()
    for gs, mx in ((1.0, math.inf), (0.25, math.inf), (1.0, half), (1.0 / 3.0, 0.01)):
        want = R.finish(S, c, gs, mx)
        got = _state(md2hip.grad_norm(gd, gs, mx))
        _same_state(got, want, (n, gs, mx))
        assert int(got["ok"]) == 1 and int(got["skipped"]) == 0
    # twice, and on a workspace and a state that held 0xFF (skipped zeroed): the same bytes
    want = R.finish(S, c, 1.0, half)
    a = _state(md2hip.grad_norm(gd, 1.0, half))
    b = _state(md2hip.grad_norm(gd, 1.0, half))
    ws = torch.full((lib().md2_grad_norm_workspace_size(n),), 0xFF, dtype=torch.uint8, device="cuda")
    st = torch.full((40,), 0xFF, dtype=torch.uint8, device="cuda")
    st[16:24] = 0
    d = _state(md2hip.grad_norm(gd, 1.0, half, state=st, workspace=ws))
    assert a.tobytes() == b.tobytes() == d.tobytes() == want.tobytes()
    # a pointer that is 4-byte aligned only: the bytes of the aligned copy
    buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    off = buf[1:n + 1]
    off.copy_(gd)
    assert off.data_ptr() % 16 == 4 and gd.data_ptr() % 16 == 0
    assert _state(md2hip.grad_norm(off, 1.0, half)).tobytes() == want.tobytes()


def test_grad_norm_hand_built_cases():
    import md2hip
    z = _state(md2hip.grad_norm(torch.zeros(5000, device="cuda"), 1.0, 1.0))
    assert float(z["norm"]) == 0.0 and float(z["coef"]) == 1.0 and int(z["ok"]) == 1 and float(z["sumsq"]) == 0.0

    big = torch.full((1000,), 1e30, device="cuda")         # squares overflow fp32, not fp64
    b = _state(md2hip.grad_norm(big))
    assert np.isfinite(b["norm"]) and int(b["ok"]) == 1 and int(b["nonfinite"]) == 0
    _same_state(b, R.grad_norm(big.cpu().numpy()))
    assert abs(float(b["norm"]) / (1e30 * math.sqrt(1000.0)) - 1.0) < 1e-6

    g = _vector(4097, 3)
    g[[0, 255, 4096]] = [np.nan, np.inf, -np.inf]
    gd = torch.from_numpy(g).cuda()
    st = None
    for k in (1, 2, 3):                                    # skipped: exactly one more per call
        st = md2hip.grad_norm(gd, 1.0, 1.0, state=st)
        s = _state(st)
        _same_state(s, R.grad_norm(g, 1.0, 1.0, skipped=k - 1))
        assert int(s["nonfinite"]) == 3 and int(s["ok"]) == 0 and int(s["skipped"]) == k and float(s["coef"]) == 1.0
    s = _state(md2hip.grad_norm(torch.from_numpy(_vector(4097, 3)).cuda(), state=st))
    assert int(s["ok"]) == 1 and int(s["skipped"]) == 3    # a clean call leaves the count alone

    g = _vector(3001, 5)
    gd = torch.from_numpy(g).cuda()
    norm = np.float32(_state(md2hip.grad_norm(gd))["norm"])
    s = _state(md2hip.grad_norm(gd, 1.0, float(norm)))     # exactly the norm: `>` takes no clip
    assert float(s["coef"]) == 1.0 and float(s["gscale"]) == 1.0
    s = _state(md2hip.grad_norm(gd, 1.0, float(norm / np.float32(2))))
    assert abs(float(s["coef"]) - 0.5) <= 2.0 ** -25 and s["coef"] == (norm / np.float32(2)) / norm
    s = _state(md2hip.grad_norm(gd, 1.0, float(np.nextafter(norm, np.float32(0)))))
    assert float(s["coef"]) < 1.0


# ---- md2_adam_guarded ---------------------------------------------------------------------------------
def test_adam_guarded_against_adam():
    import md2hip
    from md2hip._lib import check, lib, ptr, stream_of
    n = 1000
    rng = np.random.default_rng(11)
    p0, g, m0, v0 = (torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda() for _ in range(4))
    v0 = v0.abs()
    st = stream_of(p0.device)
    half = float(np.float32(_state(md2hip.grad_norm(g, 0.37))["norm"]) / np.float32(2))
    state = md2hip.grad_norm(g, 0.37, half)
    s = _state(state)
    assert int(s["ok"]) == 1 and float(s["coef"]) < 1.0
    pa, ma, va = p0.clone(), m0.clone(), v0.clone()
    pb, mb, vb = p0.clone(), m0.clone(), v0.clone()
    check(lib().md2_adam_guarded(ptr(pa), ptr(g), ptr(ma), ptr(va), n, 1e-3, 0.9, 0.999, 1e-8, 3, ptr(state), st),
          "md2_adam_guarded")
    check(lib().md2_adam(ptr(pb), ptr(g), ptr(mb), ptr(vb), n, 1e-3, 0.9, 0.999, 1e-8, 3, float(s["gscale"]), st),
          "md2_adam")
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa, p0)
    # not ok: nothing moves
    gbad = g.clone()
    gbad[500] = float("inf")
    state = md2hip.grad_norm(gbad, 0.37, half)
    assert int(_state(state)["ok"]) == 0
    pa, ma, va = p0.clone(), m0.clone(), v0.clone()
    check(lib().md2_adam_guarded(ptr(pa), ptr(gbad), ptr(ma), ptr(va), n, 1e-3, 0.9, 0.999, 1e-8, 3, ptr(state), st),
          "md2_adam_guarded")
    torch.cuda.synchronize()
    assert torch.equal(pa, p0) and torch.equal(ma, m0) and torch.equal(va, v0)


# ---- the model ----------------------------------------------------------------------------------------
def _setup():
    import md2hip
    enc = md2hip.ResNet(18, in_channels=3)
    m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                              embedding_levels=0), md2hip.PoseDecoder(512), seed=42)
    K, invK = D.intrinsics(W, H)
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy())
    params = md2hip.Params(target_size=(W, H), batch_size=N, automasking=False)
    return m, cache, params


def _xs():
    return [D.triplets(N, 3, H, W, seed=s).float().cuda().contiguous() for s in (1, 2, 3)]


def _snap(m, opt, loss):
    torch.cuda.synchronize()
    return dict(loss=loss.clone(), flat=m.flat.clone(), m=opt.m.clone(), v=opt.v.clone(), grad=m.grad.clone())


def _eager(m, cache, params, opt, x):
    import md2hip
    return _snap(m, opt, md2hip.train_step(m, x, None, cache, params, opt))


def _equal(a, b, what, grad=True):
    for k in ("loss", "flat", "m", "v") + (("grad",) if grad else ()):
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module")
def plain3():
    """three plain eager steps from the seed-42 start: the snapshots the guarded paths must equal"""
    import md2hip
    m, cache, params = _setup()
    opt = md2hip.ADAM(1e-3)
    return [_eager(m, cache, params, opt, x) for x in _xs()]


def test_guarded_without_clipping_is_the_plain_step(plain3):
    """Fails without the feature: ADAM takes no guard options there."""
    import md2hip
    xs = _xs()
    me, cache, params = _setup()
    mg, _, _ = _setup()
    oe = md2hip.ADAM(1e-3, max_grad_norm=math.inf)
    og = md2hip.ADAM(1e-3, skip_nonfinite=True)
    ex_g = mg.executor(tuple(xs[0].shape), cache, params)
    for i, x in enumerate(xs):
        e = _eager(me, cache, params, oe, x)
        g = _snap(mg, og, ex_g.train_step_graph(x, og))
        _equal(e, plain3[i], ("eager", i))
        _equal(g, plain3[i], ("graph", i))
        se, sg = _state(oe.guard_tensor()), _state(og.guard_tensor())
        _same_state(se, sg, i)
        assert int(se["ok"]) == 1 and float(se["coef"]) == 1.0 and float(se["gscale"]) == 1.0
    # the norm is the restatement's, on the downloaded gradient
    _same_state(se, R.grad_norm(plain3[-1]["grad"].cpu().numpy()), "norm")
    d = oe.guard_state()
    assert set(d) == {"norm", "coef", "ok", "skipped", "nonfinite"}
    assert d["ok"] is True and d["skipped"] == 0 and d["nonfinite"] == 0 and d["norm"] == float(se["norm"]) > 0


def test_clipping_equals_adam_with_the_coefficient(plain3):
    import md2hip
    from md2hip._lib import check, lib, ptr, stream_of
    x = _xs()[0]
    norm = np.float32(R.grad_norm(plain3[0]["grad"].cpu().numpy())["norm"])
    half = float(norm / np.float32(2))
    m, cache, params = _setup()
    opt = md2hip.ADAM(1e-3, max_grad_norm=half)
    a = _eager(m, cache, params, opt, x)
    s = _state(opt.guard_tensor())
    assert s["norm"] == norm and float(s["coef"]) == 0.5 and int(s["ok"]) == 1
    # forward_loss + segments + the plain md2_model_adam with grad_scale = the coefficient read back
    mr, _, _ = _setup()
    ex = mr.executor(tuple(x.shape), cache, params)
    loss = ex.forward_loss(x).clone()
    ex.backward()
    am, av = torch.zeros_like(mr.flat), torch.zeros_like(mr.flat)
    check(lib().md2_model_adam(ex.handle, ptr(am), ptr(av), 1e-3, 0.9, 0.999, 1e-8, 1, float(s["coef"]),
                               stream_of(mr.device)), "md2_model_adam")
    torch.cuda.synchronize()
    assert torch.equal(loss, a["loss"]) and torch.equal(mr.grad, a["grad"])
    assert torch.equal(mr.flat, a["flat"]) and torch.equal(am, a["m"]) and torch.equal(av, a["v"])
    assert not torch.equal(a["flat"], plain3[0]["flat"])
    # the captured step clips alike
    mg, _, _ = _setup()
    og = md2hip.ADAM(1e-3, max_grad_norm=half)
    g = _snap(mg, og, mg.executor(tuple(x.shape), cache, params).train_step_graph(x, og))
    _equal(g, a, "graph")
    _same_state(_state(og.guard_tensor()), s, "graph")


def test_a_non_finite_gradient_skips_the_update(plain3):
    import md2hip
    from md2hip._lib import check, lib, ptr, stream_of
    xs = _xs()
    m, cache, params = _setup()
    opt = md2hip.ADAM(1e-3, skip_nonfinite=True)
    _equal(_eager(m, cache, params, opt, xs[0]), plain3[0], "clean step 1")
    ex = m._last
    xe = xs[1][:, 1].contiguous()
    e0 = [d.clone() for d in md2hip.eval_disparity(m, xe)]
    before = dict(flat=m.flat.clone(), m=opt.m.clone(), v=opt.v.clone())

    # a forward, a backward from a cotangent with one Inf, the guarded update
    ex.forward(xs[1])
    disps, _ = ex.outputs()
    cot = [torch.zeros_like(d) for d in disps]
    cot[-1].view(-1)[::7] = 1e-3
    cot[-1].view(-1)[1234] = float("inf")                  # the full-resolution level: 2 x 64 x 128
    arr = (C.c_void_p * 5)(*[c.data_ptr() for c in cot])
    check(lib().md2_model_backward_from(ex.handle, arr, None, stream_of(m.device)), "md2_model_backward_from")
    ex.pending = False
    m._last = ex
    opt.update(m)
    torch.cuda.synchronize()
    s = opt.guard_state()
    assert s["ok"] is False and s["skipped"] == 1 and s["nonfinite"] >= 1 and s["coef"] == 1.0
    assert not torch.isfinite(m.grad).all()
    assert torch.equal(m.flat, before["flat"]) and torch.equal(opt.m, before["m"]) and torch.equal(opt.v, before["v"])
    e1 = md2hip.eval_disparity(m, xe)
    for a, b in zip(e0, e1):
        assert torch.isfinite(b).all() and torch.equal(a, b)           # the packed weights too
    assert opt.t == 2                                                  # the skipped step took its number

    # the next clean step: that of a plain run whose second step number went unused
    after = _eager(m, cache, params, opt, xs[2])
    mr, _, _ = _setup()
    orf = md2hip.ADAM(1e-3)
    _eager(mr, cache, params, orf, xs[0])
    orf.t = 2
    _equal(after, _eager(mr, cache, params, orf, xs[2]), "clean step after the skip")
    assert opt.guard_state()["skipped"] == 1 and opt.guard_state()["ok"] is True


def test_a_nan_pixel_skips_the_captured_step(plain3):
    import md2hip
    xs = _xs()
    m, cache, params = _setup()
    opt = md2hip.ADAM(1e-3, skip_nonfinite=True)
    ex = m.executor(tuple(xs[0].shape), cache, params)
    start = m.flat.clone()
    bad = xs[0].clone()
    bad[1, 1, 0, 17, 40] = float("nan")       # the networks' ReLUs swallow it, the loss tail does not
    loss = ex.train_step_graph(bad, opt).clone()
    torch.cuda.synchronize()
    s = opt.guard_state()
    assert torch.isnan(loss).all() and s["ok"] is False and s["skipped"] == 1 and s["nonfinite"] >= 1
    assert torch.equal(m.flat, start) and not opt.m.any() and not opt.v.any()
    # the next captured step on clean frames works and is the eager path's second step
    g = _snap(m, opt, ex.train_step_graph(xs[0], opt))
    assert torch.isfinite(g["loss"]).all() and torch.isfinite(g["flat"]).all()
    mr, _, _ = _setup()
    orf = md2hip.ADAM(1e-3)
    orf.t = 1
    _equal(g, _eager(mr, cache, params, orf, xs[0]), "captured step after the skip")
    s = opt.guard_state()
    assert s["ok"] is True and s["skipped"] == 1 and s["nonfinite"] == 0


def test_switches_and_refusals(plain3):
    import md2hip
    from md2hip import comm as MC  # noqa: F401  (declares md2_model_train_step_dp)
    from md2hip._lib import check, lib, ptr, stream_of
    x = _xs()[0]
    m, cache, params = _setup()
    ex = m.executor(tuple(x.shape), cache, params)
    st = stream_of(m.device)
    p = C.c_void_p()
    assert lib().md2_model_grad_guard_state(ex.handle, C.byref(p)) == MD2_ESTATE     # never switched on
    for bad in (0.0, -1.0, float("nan")):
        assert lib().md2_model_set_grad_guard(ex.handle, 1, bad) == 1
    assert lib().md2_model_grad_guard_state(ex.handle, C.byref(p)) == MD2_ESTATE

    # the DP step without a communicator, guarded with max_norm = inf: the plain step
    bytes0 = ex.device_bytes()
    ex.set_grad_guard(True, math.inf)
    # state and workspace are executor-owned and counted from the first switch-on
    assert ex.device_bytes() == bytes0 + 40 + R.workspace_bytes(m.flat.numel())
    am, av = torch.zeros_like(m.flat), torch.zeros_like(m.flat)
    loss = torch.zeros(1, device="cuda")
    ex.sync()
    check(lib().md2_model_train_step_dp(ex.handle, None, ptr(x), None, ptr(am), ptr(av), 1e-3, 0.9, 0.999, 1e-8, 1,
                                        ptr(loss), st), "md2_model_train_step_dp")
    torch.cuda.synchronize()
    assert torch.equal(loss, plain3[0]["loss"]) and torch.equal(m.flat, plain3[0]["flat"])
    assert torch.equal(am, plain3[0]["m"]) and torch.equal(av, plain3[0]["v"])
    s = _state(ex.guard_tensor())
    assert int(s["ok"]) == 1 and float(s["norm"]) > 0

    # a segment's update cannot know the global norm
    rc = lib().md2_model_adam_segment(ex.handle, 0, ptr(am), ptr(av), 1e-3, 0.9, 0.999, 1e-8, 2, 1.0, st)
    assert rc == MD2_ENOTSUP and b"guard" in lib().md2_last_error()

    # test mode refuses, like the other training entries
    m.testmode(True)
    try:
        ex.sync()
        assert lib().md2_model_set_grad_guard(ex.handle, 1, 1.0) == MD2_ESTATE
        assert b"test mode" in lib().md2_last_error()
    finally:
        m.testmode(False)
    ex.sync()

    # off again: the plain bytes, and the segment update is back
    ex.set_grad_guard(False)
    m.touch()
    m._last = ex
    opt = md2hip.ADAM(1e-3)
    opt.m, opt.v, opt.t = am, av, 1
    _equal(_eager(m, cache, params, opt, _xs()[1]), plain3[1], "guard off")
    rc = lib().md2_model_forward_loss(ex.handle, ptr(x), None, ptr(loss), None, st)
    assert rc == 0
    assert lib().md2_model_backward_segment(ex.handle, 0, None, None, st) == 0
    assert lib().md2_model_adam_segment(ex.handle, 0, ptr(am), ptr(av), 1e-3, 0.9, 0.999, 1e-8, 3, 1.0, st) == 0
    assert lib().md2_model_adam_join(ex.handle, st) == 0
    torch.cuda.synchronize()


def test_mpi_mode_refuses():
    import md2hip
    from md2hip._lib import lib
    enc = md2hip.ResNet(18, in_channels=3)
    m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                              embedding_levels=21), md2hip.PoseDecoder(512), seed=42)
    K, invK = D.intrinsics(W, H)
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy())
    params = md2hip.Params(target_size=(W, H), batch_size=1, automasking=False)
    ex = m.executor((1, 3, 3, H, W), cache, params, num_bins=4)
    assert lib().md2_model_set_grad_guard(ex.handle, 1, 1.0) == MD2_ENOTSUP
    assert b"MPI mode" in lib().md2_last_error()
