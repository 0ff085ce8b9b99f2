"""Stereo supervision through the model (md2_model_forward_loss_stereo /
md2_model_train_step_graph_stereo): ResNet-18, N = 2, 3 x 64 x 96, "MS" (both temporal sources and
the stereo frame) and "S" (the stereo frame alone).

  * train_loss(..., x_stereo, stereo_Rt) equals model(x) + loss_tail(..., x_stereo, stereo_Rt) +
    pullback, bit for bit, on the loss and the flat gradient;
  * S mode: the pose decoder's gradient is exactly zero, the encoder's and depth decoder's are not;
  * the captured step equals eager steps, and a live executor switched between M, MS and S gives
    what fresh executors give;
  * with x_net the networks read x_net and the loss reads x and x_stereo;
  * without x_stereo nothing moves; MPI mode refuses."""
import pytest
import torch

from tests import _data as D

pytestmark = pytest.mark.gpu

MD2_ENOTSUP = 3
N, H, W = 2, 64, 96


def _setup(automasking, emb=0, n=N):
    import md2hip
    enc = md2hip.ResNet(18, in_channels=3)
    m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                              embedding_levels=emb), md2hip.PoseDecoder(512), seed=42)
    K, invK = D.intrinsics(W, H)
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy())
    params = md2hip.Params(target_size=(W, H), batch_size=n, automasking=automasking)
    return m, cache, params


def _inputs(seed=7, n=N):
    import md2hip
    x = D.triplets(n, 3, H, W, seed=seed).float().cuda().contiguous()
    xs = D.triplets(n, 3, H, W, seed=seed + 22)[:, 0].float().cuda().contiguous()
    Rt = torch.from_numpy(md2hip.stereo_transforms(["l", "r"][:n], [False, True][:n])).cuda()
    return x, xs, Rt


def _jitter(x, seed=0):
    import md2hip
    return md2hip.color_jitter(x, md2hip.ColorJitter(p=1.0).draw(list(range(x.shape[0])), seed))


def _fused(m, cache, params, x, xs, Rt, temporal, x_net=None):
    import md2hip
    m.grad.fill_(float("nan"))
    loss, *_ = md2hip.train_loss(m, x, None, cache, params, x_net=x_net, x_stereo=xs, stereo_Rt=Rt,
                                 temporal=temporal)
    loss = loss.clone()
    g = md2hip.gradient(m)
    torch.cuda.synchronize()
    return loss, m.grad.clone()


def _composed(m, cache, params, x, xs, Rt, temporal, x_net=None):
    import md2hip
    m.grad.fill_(float("nan"))
    disps, poses = m(x if x_net is None else x_net, cache=cache, params=params)
    tail = md2hip.loss_tail([d.contiguous() for d in disps], [(p.rvec, p.tvec) for p in poses], x, None,
                            cache, params, sigmoid_grad=False, x_stereo=xs, stereo_Rt=Rt, temporal=temporal)
    g = md2hip.pullback(m, tail["d_disp"], tail["d_pose"]).clone()
    torch.cuda.synchronize()
    return tail["loss"].clone(), g


@pytest.mark.parametrize("automasking", [False, True], ids=["plain", "automask"])
@pytest.mark.parametrize("temporal", [True, False], ids=["MS", "S"])
def test_train_loss_equals_model_then_loss_tail_then_pullback(temporal, automasking):
    m, cache, params = _setup(automasking)
    x, xs, Rt = _inputs()
    a = _fused(m, cache, params, x, xs, Rt, temporal)
    b = _composed(m, cache, params, x, xs, Rt, temporal)
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert torch.isfinite(a[1]).all()
    diff = (a[1] != b[1]).sum().item()
    assert diff == 0, f"{diff} of {a[1].numel()} gradient entries differ"
    # the stereo source matters: another frame, or the other sign of t_x, is another step
    c = _fused(m, cache, params, x, xs, Rt * torch.tensor([1.0] * 9 + [-1.0] * 3, device="cuda"), temporal)
    assert not torch.equal(a[0], c[0])


def test_s_mode_gives_the_pose_decoder_a_zero_gradient():
    import numpy as np
    m, cache, params = _setup(False)
    x, xs, Rt = _inputs()
    _, g = _fused(m, cache, params, x, xs, Rt, temporal=False)
    pose = torch.zeros_like(g, dtype=torch.bool)
    groups = {}
    for name, shape, off in m.table:
        n = int(np.prod(shape))
        if "pose" in name.lower():
            pose[off:off + n] = True
        else:
            groups.setdefault(name.split(".")[0], []).append((off, off + n))
    assert pose.any() and len(groups) >= 2, [name for name, _, _ in m.table][:8]
    assert torch.isfinite(g).all()
    assert (g[pose] == 0).all()
    for key, ranges in groups.items():       # the encoder and the depth decoder do learn
        assert any((g[a:b] != 0).any().item() for a, b in ranges), key
    # MS: the pose decoder learns too
    _, g = _fused(m, cache, params, x, xs, Rt, temporal=True)
    assert (g[pose] != 0).any()


@pytest.mark.parametrize("temporal", [True, False], ids=["MS", "S"])
def test_graph_step_equals_eager_steps(temporal):
    import md2hip
    ins = [_inputs(seed=s) for s in (1, 2, 3)]
    me, cache, params = _setup(True)
    mg, _, _ = _setup(True)
    oe, og = md2hip.ADAM(1e-3), md2hip.ADAM(1e-3)
    ex_g = mg.executor(tuple(ins[0][0].shape), cache, params)
    for i, (x, xs, Rt) in enumerate(ins):
        le = md2hip.train_step(me, x, None, cache, params, oe, x_stereo=xs, stereo_Rt=Rt, temporal=temporal).clone()
        lg = ex_g.train_step_graph(x, og, x_stereo=xs, stereo_Rt=Rt, temporal=temporal).clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (i, le, lg)
        assert torch.equal(me.flat, mg.flat), i
        assert torch.equal(oe.m, og.m) and torch.equal(oe.v, og.v), i
    assert torch.isfinite(mg.flat).all()


def test_switching_a_live_executor_between_m_ms_and_s_recaptures():
    """One executor stepped through M, MS, S, M, MS (a new capture at every switch) against a twin
    model that gets a fresh executor -- a first capture -- for every step."""
    import md2hip
    x, xs, Rt = _inputs()
    modes = [dict(), dict(x_stereo=xs, stereo_Rt=Rt, temporal=True), dict(x_stereo=xs, stereo_Rt=Rt, temporal=False),
             dict(), dict(x_stereo=xs, stereo_Rt=Rt, temporal=True)]
    live, cache, params = _setup(False)
    twin, _, _ = _setup(False)
    ol, ot = md2hip.ADAM(1e-3), md2hip.ADAM(1e-3)
    ex = live.executor(tuple(x.shape), cache, params)
    losses = []
    for i, kw in enumerate(modes):
        ll = ex.train_step_graph(x, ol, **kw).clone()
        twin.evict()
        lt = twin.executor(tuple(x.shape), cache, params).train_step_graph(x, ot, **kw).clone()
        torch.cuda.synchronize()
        assert torch.equal(ll, lt), (i, ll, lt)
        assert torch.equal(live.flat, twin.flat), i
        losses.append(ll.item())
    assert len(set(losses[:3])) == 3, losses          # the three regimes are three different losses
    assert torch.isfinite(live.flat).all()


def test_x_net_feeds_the_networks_and_the_loss_reads_x_and_x_stereo():
    m, cache, params = _setup(True)
    x, xs, Rt = _inputs()
    x_net = _jitter(x)
    a = _fused(m, cache, params, x, xs, Rt, True, x_net=x_net)
    b = _composed(m, cache, params, x, xs, Rt, True, x_net=x_net)
    assert torch.equal(a[0], b[0]) and (a[1] != b[1]).sum().item() == 0
    plain = _fused(m, cache, params, x, xs, Rt, True)
    assert not torch.equal(a[0], plain[0])


@pytest.mark.parametrize("automasking", [False, True], ids=["plain", "automask"])
def test_without_x_stereo_nothing_moves(automasking):
    """train_loss and the captured step without x_stereo give the bits of the untouched entry points."""
    import md2hip
    from md2hip._lib import check, lib, ptr, stream_of
    m, cache, params = _setup(automasking)
    x, _, _ = _inputs()
    m.grad.fill_(float("nan"))
    loss, *_ = md2hip.train_loss(m, x, None, cache, params)
    loss = loss.clone()
    md2hip.gradient(m)
    torch.cuda.synchronize()
    g = m.grad.clone()
    ex = m.executor(tuple(x.shape), cache, params)
    raw = torch.empty(1, device="cuda")
    m.grad.fill_(float("nan"))
    ex.sync()
    check(lib().md2_model_forward_loss(ex.handle, ptr(x), None, ptr(raw), None, stream_of(x.device)))
    ex.forwarded = ex.pending = True
    ex._trained()
    ex.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, raw) and torch.equal(g, m.grad)
    # the captured step: the python entry against the C entry on a twin model
    m1, _, _ = _setup(automasking)
    m2, _, _ = _setup(automasking)
    o1, o2 = md2hip.ADAM(1e-3), md2hip.ADAM(1e-3)
    e1, e2 = m1.executor(tuple(x.shape), cache, params), m2.executor(tuple(x.shape), cache, params)
    o2.m, o2.v = torch.zeros_like(m2.flat), torch.zeros_like(m2.flat)
    l2 = torch.empty(1, device="cuda")
    for step in (1, 2):
        l1 = e1.train_step_graph(x, o1).clone()
        e2.sync()
        check(lib().md2_model_train_step_graph(e2.handle, ptr(x), None, ptr(o2.m), ptr(o2.v), 1e-3, step, ptr(l2),
                                               stream_of(x.device)))
        torch.cuda.synchronize()
        assert torch.equal(l1, l2) and torch.equal(m1.flat, m2.flat), step


def test_refused_in_mpi_mode():
    import md2hip
    from md2hip._lib import lib, ptr, stream_of
    m, cache, params = _setup(False, emb=21, n=1)
    x, xs, Rt = _inputs(n=1)
    ex = m.executor(tuple(x.shape), cache, params, num_bins=4)
    ex.set_bins(md2hip.disparity_bins(1, 4, u=torch.rand(1, 4, dtype=torch.float64,
                                                        generator=torch.Generator().manual_seed(3))))
    st = stream_of(m.device)
    loss = torch.zeros(1, device="cuda")
    am, av = torch.zeros_like(m.flat), torch.zeros_like(m.flat)
    rc = lib().md2_model_forward_loss_stereo(ex.handle, ptr(x), None, ptr(xs), ptr(Rt), 1, None, ptr(loss), None, st)
    assert rc == MD2_ENOTSUP and b"MPI mode" in lib().md2_last_error()
    rc = lib().md2_model_train_step_graph_stereo(ex.handle, ptr(x), None, ptr(xs), ptr(Rt), 0, None, ptr(am), ptr(av),
                                                 1e-4, 1, ptr(loss), st)
    assert rc == MD2_ENOTSUP and b"MPI mode" in lib().md2_last_error()
    with pytest.raises(md2hip.MD2Error, match="MPI mode"):
        md2hip.train_loss(m, x, None, cache, params, num_bins=4, x_stereo=xs, stereo_Rt=Rt)
    torch.cuda.synchronize()
