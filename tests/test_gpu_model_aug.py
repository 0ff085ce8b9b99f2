"""A separate network input (md2_model_forward_loss_aug / md2_model_train_step_graph_aug): the
encoder, both decoders and the stem's filter gradient read ``x_net``; the automask and the loss tail
read ``x``.  ResNet-18, N = 2, 64 x 128, automask off and on.

  * x_net = x (a null pointer, the same pointer, a clone) is the plain call, bit for bit;
  * x_net = color_jitter(x): the fused path equals md2_model_forward(x_net) + loss_tail on x +
    pullback, bit for bit -- which fails if the loss reads x_net or the stem gradient reads x -- and
    differs from the un-augmented gradient;
  * the captured-graph step equals eager steps and re-captures when x_net comes and goes;
  * test mode and MPI mode refuse."""
import numpy as np
import pytest
import torch

from tests import _data as D

pytestmark = pytest.mark.gpu

MD2_ENOTSUP, MD2_ESTATE = 3, 5
N, H, W = 2, 64, 128


def _setup(automasking, emb=0, n=N):
    import md2hip
    enc = md2hip.ResNet(18, in_channels=3)
    m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                              embedding_levels=emb), md2hip.PoseDecoder(512), seed=42)
    K, invK = D.intrinsics(W, H)
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy())
    params = md2hip.Params(target_size=(W, H), batch_size=n, automasking=automasking)
    return m, cache, params


def _jitter(x, seed=0):
    """every sample changed, each in its own order"""
    import md2hip
    p = md2hip.ColorJitter(p=1.0).draw(list(range(x.shape[0])), seed)
    assert p["apply"].all()
    return md2hip.color_jitter(x, p)


def _fused(m, ex, x, x_net, how="tensor"):
    """forward_loss (+ backward) -> (loss, disparities, poses, gradient), all cloned"""
    from md2hip._lib import check, lib, ptr, stream_of
    m.grad.fill_(float("nan"))
    if how == "tensor":
        loss = ex.forward_loss(x, x_net=x_net).clone()
    else:               # straight through the C-ABI: a null pointer / the same pointer as x
        loss = torch.empty(1, device="cuda")
        ex.sync()
        check(lib().md2_model_forward_loss_aug(ex.handle, ptr(x), None if how == "null" else ptr(x), None, ptr(loss),
                                               None, stream_of(x.device)), "md2_model_forward_loss_aug")
        ex.forwarded = ex.pending = True
        ex._trained()
    disps, pose = ex.outputs()
    disps, pose = [d.clone() for d in disps], pose.clone()
    ex.backward()
    torch.cuda.synchronize()
    return loss, disps, pose, m.grad.clone()


def _same(a, b):
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    for da, db in zip(a[1], b[1]):
        assert torch.equal(da, db)
    assert torch.equal(a[2], b[2])
    assert torch.isfinite(a[3]).all()
    diff = (a[3] != b[3]).sum().item()
    assert diff == 0, f"{diff} of {a[3].numel()} gradient entries differ"


@pytest.mark.parametrize("automasking", [False, True], ids=["plain", "automask"])
def test_x_net_equal_to_x_is_the_plain_call(automasking):
    m, cache, params = _setup(automasking)
    x = D.triplets(N, 3, H, W).float().cuda().contiguous()
    ex = m.executor(tuple(x.shape), cache, params)
    ref = _fused(m, ex, x, None)
    _same(_fused(m, ex, x, None, how="null"), ref)
    _same(_fused(m, ex, x, None, how="same"), ref)
    _same(_fused(m, ex, x, x), ref)
    _same(_fused(m, ex, x, x.clone()), ref)


@pytest.mark.parametrize("automasking", [False, True], ids=["plain", "automask"])
def test_fused_equals_forward_on_x_net_and_loss_tail_on_x(automasking):
    import md2hip
    from md2hip.primitives import automasking_loss
    m, cache, params = _setup(automasking)
    x = D.triplets(N, 3, H, W).float().cuda().contiguous()
    x_net = _jitter(x)
    assert not torch.equal(x_net, x)
    ex = m.executor(tuple(x.shape), cache, params)
    plain = _fused(m, ex, x, None)
    aug = _fused(m, ex, x, x_net)

    # the composition the library already guarantees (tests/test_gpu_forward_boundary.py)
    m.grad.fill_(float("nan"))
    disps, poses = m(x_net, cache=cache, params=params)               # md2_model_forward
    for a, b in zip(aug[1], disps):
        assert torch.equal(a, b)
    auto = automasking_loss(x) if automasking else None
    tail = md2hip.loss_tail([d.contiguous() for d in disps], [(p.rvec, p.tvec) for p in poses], x, auto,
                            cache, params, sigmoid_grad=False)
    assert torch.equal(tail["loss"], aug[0]), (tail["loss"], aug[0])
    g = md2hip.pullback(m, tail["d_disp"], tail["d_pose"]).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(g).all()
    diff = (g != aug[3]).sum().item()
    assert diff == 0, f"{diff} of {g.numel()} gradient entries differ from forward(x_net) + loss_tail(x)"

    # not vacuous: the augmented step is another step, and not the one that jitters the loss too
    assert not torch.equal(aug[0], plain[0])
    assert (aug[3] != plain[3]).float().mean().item() > 0.5
    both = _fused(m, ex, x_net, None)
    assert not torch.equal(both[0], aug[0]) and not torch.equal(both[3], aug[3])
    # the stem's filter gradient in particular
    name, shape, off = m.table[0]
    n = int(np.prod(shape))
    assert not torch.equal(aug[3][off:off + n], plain[3][off:off + n]), name


@pytest.mark.parametrize("automasking", [False, True], ids=["plain", "automask"])
def test_graph_step_equals_eager_steps(automasking):
    import md2hip
    xs = [D.triplets(N, 3, H, W, seed=s).float().cuda().contiguous() for s in (1, 2, 3)]
    nets = [_jitter(x, seed=s) for s, x in enumerate(xs)]
    me, cache, params = _setup(automasking)
    mg, _, _ = _setup(automasking)
    oe, og = md2hip.ADAM(1e-3), md2hip.ADAM(1e-3)
    ex_e = me.executor(tuple(xs[0].shape), cache, params)
    ex_g = mg.executor(tuple(xs[0].shape), cache, params)

    def eager(x, x_net):
        loss = ex_e.forward_loss(x, x_net=x_net).clone()
        ex_e.backward()
        me._last = ex_e
        oe.update(me)
        return loss

    for i, (x, xn) in enumerate(zip(xs, nets)):
        le, lg = eager(x, xn), ex_g.train_step_graph(x, og, x_net=xn).clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (i, le, lg)
        assert torch.equal(me.flat, mg.flat), i
        assert torch.equal(oe.m, og.m) and torch.equal(oe.v, og.v), i
        assert torch.equal(me.grad, mg.grad) and (mg.grad != 0).any(), i
    # x_net goes and comes back: the step is captured again each time and still matches
    for i, xn in enumerate([None, nets[0], None, nets[1]]):
        x = xs[i % 3]
        le, lg = eager(x, xn), ex_g.train_step_graph(x, og, x_net=xn).clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (i, le, lg)
        assert torch.equal(me.flat, mg.flat), i
    assert torch.isfinite(mg.flat).all() and torch.isfinite(mg.grad).all()


def test_refused_in_test_mode():
    from md2hip._lib import lib, ptr, stream_of
    m, cache, params = _setup(False)
    x = D.triplets(N, 3, H, W).float().cuda().contiguous()
    x_net = _jitter(x)
    ex = m.executor(tuple(x.shape), cache, params)
    ex.forward_loss(x)                   # one train-mode forward: running statistics to fold
    ex.backward()
    st = stream_of(m.device)
    loss = torch.zeros(1, device="cuda")
    am, av = torch.zeros_like(m.flat), torch.zeros_like(m.flat)
    m.testmode(True)
    try:
        ex.sync()
        rc = lib().md2_model_forward_loss_aug(ex.handle, ptr(x), ptr(x_net), None, ptr(loss), None, st)
        assert rc == MD2_ESTATE and b"test mode" in lib().md2_last_error()
        rc = lib().md2_model_train_step_graph_aug(ex.handle, ptr(x), ptr(x_net), None, ptr(am), ptr(av), 1e-4, 1,
                                                  ptr(loss), st)
        assert rc == MD2_ESTATE and b"test mode" in lib().md2_last_error()
    finally:
        m.testmode(False)
    ex.sync()
    torch.cuda.synchronize()


def test_refused_in_mpi_mode():
    import md2hip
    from md2hip._lib import lib, ptr, stream_of
    m, cache, params = _setup(False, emb=21, n=1)
    x = D.triplets(1, 3, H, W).float().cuda().contiguous()
    x_net = _jitter(x)
    ex = m.executor(tuple(x.shape), cache, params, num_bins=4)
    ex.set_bins(md2hip.disparity_bins(1, 4, u=torch.rand(1, 4, dtype=torch.float64,
                                                        generator=torch.Generator().manual_seed(3))))
    st = stream_of(m.device)
    loss = torch.zeros(1, device="cuda")
    am, av = torch.zeros_like(m.flat), torch.zeros_like(m.flat)
    rc = lib().md2_model_forward_loss_aug(ex.handle, ptr(x), ptr(x_net), None, ptr(loss), None, st)
    assert rc == MD2_ENOTSUP and b"MPI mode" in lib().md2_last_error()
    rc = lib().md2_model_train_step_graph_aug(ex.handle, ptr(x), ptr(x_net), None, ptr(am), ptr(av), 1e-4, 1,
                                              ptr(loss), st)
    assert rc == MD2_ENOTSUP and b"MPI mode" in lib().md2_last_error()
    with pytest.raises(md2hip.MD2Error, match="MPI mode"):
        md2hip.train_loss(m, x, None, cache, params, num_bins=4, x_net=x_net)
    # without x_net the aug entry is the plain call, MPI mode included
    rc = lib().md2_model_forward_loss_aug(ex.handle, ptr(x), None, None, ptr(loss), None, st)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(loss).all()
