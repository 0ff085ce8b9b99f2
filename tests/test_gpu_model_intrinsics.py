"""Per-sample intrinsics through the model (md2_model_set_intrinsics): ResNet-18, N = 2, 3 x 64 x 96.

  * rows all equal to TrainCache.K: loss, flat gradient and the parameters after one step equal the
    plain step's bit for bit, eager and captured;
  * distinct rows: train_loss(K=, invK=) equals model(x) + loss_tail(K=, invK=) + pullback bit for
    bit, in M and in MS, with the library's own automask and without;
  * the captured step reads the executor's copies: new values between two replays take effect and
    equal the eager step, and a call without them is the plain step again;
  * MPI mode refuses; a malformed K is a ValueError."""
import pytest
import torch

from tests import _data as D
from tests.test_gpu_loss_intrinsics import rows, sample_intrinsics
from tests.test_gpu_model_stereo import H, MD2_ENOTSUP, N, W, _inputs, _setup

pytestmark = pytest.mark.gpu


def _distinct(scale=1.0):
    Ks = sample_intrinsics(N, W, H)
    if scale != 1.0:
        out = []
        for K, _ in Ks:
            K = K.clone()
            K[0, 0] *= scale
            K[1, 1] *= scale
            out.append((D.fp32_grid(K), D.fp32_grid(torch.linalg.inv(K))))
        Ks = out
    return rows(Ks)


def _equal():
    return rows([D.intrinsics(W, H)] * N)


def _stereo_kw(mode, xs, Rt):
    return {} if mode == "M" else dict(x_stereo=xs, stereo_Rt=Rt, temporal=True)


def _fused(m, cache, params, x, kw):
    import md2hip
    m.grad.fill_(float("nan"))
    loss, *_ = md2hip.train_loss(m, x, None, cache, params, **kw)
    loss = loss.clone()
    md2hip.gradient(m)
    torch.cuda.synchronize()
    return loss, m.grad.clone()


def _composed(m, cache, params, x, kw):
    import md2hip
    m.grad.fill_(float("nan"))
    disps, poses = m(x, cache=cache, params=params)
    tail = md2hip.loss_tail([d.contiguous() for d in disps], [(p.rvec, p.tvec) for p in poses], x, None, cache,
                            params, sigmoid_grad=False, **kw)
    g = md2hip.pullback(m, tail["d_disp"], tail["d_pose"]).clone()
    torch.cuda.synchronize()
    return tail["loss"].clone(), g


@pytest.mark.parametrize("automasking", [False, True], ids=["plain", "automask"])
def test_equal_rows_are_the_plain_step_eager_and_captured(automasking):
    import md2hip
    x, _, _ = _inputs()
    K, invK = _equal()
    ms = [_setup(automasking) for _ in range(4)]
    cache, params = ms[0][1], ms[0][2]
    plain, withk, gplain, gwithk = (m for m, _, _ in ms)
    before = plain.flat.clone()
    a = _fused(plain, cache, params, x, {})
    b = _fused(withk, cache, params, x, dict(K=K, invK=invK))
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert torch.isfinite(a[1]).all() and (a[1] != b[1]).sum().item() == 0
    opts = [md2hip.ADAM(1e-3) for _ in range(4)]
    la = md2hip.train_step(plain, x, None, cache, params, opts[0]).clone()
    lb = md2hip.train_step(withk, x, None, cache, params, opts[1], K=K, invK=invK).clone()
    lc = gplain.executor(tuple(x.shape), cache, params).train_step_graph(x, opts[2]).clone()
    ld = gwithk.executor(tuple(x.shape), cache, params).train_step_graph(x, opts[3], K=K, invK=invK).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(la, lc) and torch.equal(la, ld), (la, lb, lc, ld)
    for m in (withk, gplain, gwithk):
        assert torch.equal(plain.flat, m.flat)
    assert not torch.equal(plain.flat, before)      # the step moved the parameters


@pytest.mark.parametrize("automasking", [False, True], ids=["plain", "automask"])
@pytest.mark.parametrize("mode", ["M", "MS"])
def test_train_loss_equals_model_then_loss_tail_then_pullback(mode, automasking):
    m, cache, params = _setup(automasking)
    x, xs, Rt = _inputs()
    K, invK = _distinct()
    kw = dict(K=K, invK=invK, **_stereo_kw(mode, xs, Rt))
    a = _fused(m, cache, params, x, kw)
    b = _composed(m, cache, params, x, kw)
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert torch.isfinite(a[1]).all()
    diff = (a[1] != b[1]).sum().item()
    assert diff == 0, f"{diff} of {a[1].numel()} gradient entries differ"
    # the matrices matter: TrainCache.K for every sample is another step
    c = _fused(m, cache, params, x, _stereo_kw(mode, xs, Rt))
    assert not torch.equal(a[0], c[0])
    # K alone: invK is the fp64 host inverse of the fp32 K, rounded once
    import numpy as np
    inv = np.linalg.inv(K.cpu().numpy().astype(np.float64).reshape(N, 3, 3)).astype(np.float32)
    d = _fused(m, cache, params, x, dict(K=K.reshape(N, 3, 3), **_stereo_kw(mode, xs, Rt)))
    e = _fused(m, cache, params, x, dict(K=K, invK=torch.from_numpy(inv).cuda(), **_stereo_kw(mode, xs, Rt)))
    assert torch.equal(d[0], e[0]) and (d[1] != e[1]).sum().item() == 0


@pytest.mark.parametrize("mode", ["M", "MS"])
def test_the_captured_step_reads_new_values_and_clears(mode):
    """Graph executor against an eager twin: K1, K2 (new values, the same capture), none (the plain
    step again), K1 (captured again)."""
    import md2hip
    ins = [_inputs(seed=s) for s in (1, 2, 3, 4)]
    k1, k2 = _distinct(), _distinct(0.95)
    ks = [dict(K=k1[0], invK=k1[1]), dict(K=k2[0], invK=k2[1]), {}, dict(K=k1[0], invK=k1[1])]
    me, cache, params = _setup(True)
    mg, _, _ = _setup(True)
    mp, _, _ = _setup(True)          # never sees intrinsics: the plain captured step
    oe, og, op = md2hip.ADAM(1e-3), md2hip.ADAM(1e-3), md2hip.ADAM(1e-3)
    ex_g = mg.executor(tuple(ins[0][0].shape), cache, params)
    losses = []
    for i, ((x, xs, Rt), k) in enumerate(zip(ins, ks)):
        kw = dict(k, **_stereo_kw(mode, xs, Rt))
        le = md2hip.train_step(me, x, None, cache, params, oe, **kw).clone()
        lg = ex_g.train_step_graph(x, og, **kw).clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (i, le, lg)
        assert torch.equal(me.flat, mg.flat), i
        losses.append(lg.item())
        if i == 2:
            # the step without K on the executor that had them: the plain step's bits from the same state
            mp.load_flat(flat_before)
            op.m, op.v, op.t = m_before.clone(), v_before.clone(), 2
            lp = mp.executor(tuple(x.shape), cache, params).train_step_graph(
                x, op, **_stereo_kw(mode, xs, Rt)).clone()
            torch.cuda.synchronize()
            assert torch.equal(lp, lg) and torch.equal(mp.flat, mg.flat)
        flat_before, m_before, v_before = mg.flat.clone(), og.m.clone(), og.v.clone()
    assert torch.isfinite(mg.flat).all()
    # same batch, other matrices: another loss (values are read at replay, not baked into the capture)
    x, xs, Rt = ins[0]
    kw = _stereo_kw(mode, xs, Rt)
    a = ex_g.train_step_graph(x, og, **dict(ks[0], **kw)).clone()
    mg.load_flat(me.flat)
    og.m.copy_(oe.m)              # in place: the capture holds these addresses
    og.v.copy_(oe.v)
    og.t = oe.t
    b = ex_g.train_step_graph(x, og, **dict(ks[1], **kw)).clone()
    le = md2hip.train_step(me, x, None, cache, params, oe, **dict(ks[1], **kw)).clone()
    torch.cuda.synchronize()
    assert not torch.equal(a, b) and torch.equal(b, le)


def test_refused_in_mpi_mode_and_clearing_is_not():
    import md2hip
    from md2hip._lib import lib, ptr, stream_of
    m, cache, params = _setup(False, emb=21, n=1)
    x, _, _ = _inputs(n=1)
    ex = m.executor(tuple(x.shape), cache, params, num_bins=4)
    K, invK = rows(sample_intrinsics(1, W, H))
    st = stream_of(m.device)
    assert lib().md2_model_set_intrinsics(ex.handle, ptr(K), ptr(invK), st) == MD2_ENOTSUP
    assert b"MPI mode" in lib().md2_last_error()
    assert lib().md2_model_set_intrinsics(ex.handle, None, None, st) == 0
    with pytest.raises(md2hip.MD2Error, match="MPI mode"):
        md2hip.train_loss(m, x, None, cache, params, num_bins=4, K=K, invK=invK)
    torch.cuda.synchronize()


def test_a_malformed_K_is_a_value_error():
    import md2hip
    m, cache, params = _setup(False)
    x, _, _ = _inputs()
    K, invK = _distinct()
    for bad_K, bad_invK in ((K[:1], None), (K.double(), None), (K.cpu(), None), (K.reshape(-1), None),
                            (K, invK[:, :8].contiguous()), (None, invK), (K.cpu().numpy(), None)):
        with pytest.raises(ValueError):
            md2hip.train_loss(m, x, None, cache, params, K=bad_K, invK=bad_invK)
        with pytest.raises(ValueError):
            md2hip.train_step(m, x, None, cache, params, md2hip.ADAM(1e-3), K=bad_K, invK=bad_invK)
