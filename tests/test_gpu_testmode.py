"""GPU: BatchNorm running statistics as model state and test mode (Flux testmode!).

ResNet-18 at N=2, 64x128 (layer 4 is 2x4 there; every block kind is present) and one ResNet-50 case
at N=1.  References and bounds: tests/_testmode.py (fp64 oracle with batchnorm_train patched;
max(1e-6, 2 x the fp32 floor over four realisations)).  Every parity record goes to the parity
record directory (tests/_model_parity.parity_record_path) as testmode_*.json (first MI355X run: worst error / bound 0.37, the level-5
disparity of the synthetic set at 3.66e-7 against 1e-6; the running update 0.038 of its bound)."""
import pytest
import torch

from tests import _data as D
from tests import _testmode as T

pytestmark = pytest.mark.gpu

N, H, W = 2, 64, 128
MD2_EINVAL, MD2_ESTATE = 1, 5


def _model(arch=18, seed=42):
    import md2hip
    enc = md2hip.ResNet(arch, in_channels=3)
    return md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                 embedding_levels=0),
                        md2hip.PoseDecoder(enc.stages[-1]), seed=seed)


def _cfg(n, h, w):
    import md2hip
    K, invK = D.intrinsics(w, h)
    return (md2hip.TrainCache(K=K.numpy(), invK=invK.numpy()),
            md2hip.Params(target_size=(w, h), batch_size=n, automasking=False))


def _x(n, h, w, seed):
    return D.triplets(n, 3, h, w, seed=seed)


def _pose(poses):
    return torch.cat([torch.cat([p.rvec, p.tvec], 1) for p in poses], 0)


def _initial(model):
    return torch.cat([torch.cat([torch.zeros(c), torch.ones(c)]) for c in model.bn_channels])


@pytest.fixture(scope="module")
def mp():
    with pytest.MonkeyPatch.context() as m:
        yield m


@pytest.fixture(scope="module")
def trained():
    """A ResNet-18 model after three train-mode forwards on three different batches: the statistics
    after the first (stats1) and after the third (stats_a, set (a) of the parity cases)."""
    import md2hip
    model = _model()
    cache, params = _cfg(N, H, W)
    xs = [_x(N, H, W, s) for s in (7, 8, 9)]
    ex = model.executor((N, 3, 3, H, W), cache, params)
    bytes0 = ex.device_bytes()
    fresh = ex.get_bn_stats().cpu()
    md2hip.train_loss(model, xs[0].float().cuda().contiguous(), None, cache, params)
    stats1 = model.bn_stats().cpu()
    for x in xs[1:]:
        md2hip.train_loss(model, x.float().cuda().contiguous(), None, cache, params)
    stats_a = model.bn_stats().cpu()
    md2hip.gradient(model)          # no forward left pending: eval_disparity may reuse this executor
    torch.cuda.synchronize()
    return {"model": model, "ex": ex, "cache": cache, "params": params, "x": xs[0],
            "xg": xs[0].float().cuda().contiguous(), "flat": model.flat.detach().double().cpu(),
            "fresh": fresh, "stats1": stats1, "stats_a": stats_a, "bytes0": bytes0,
            "bytes_trained": ex.device_bytes()}


@pytest.fixture(scope="module")
def batch_stats(trained, mp):
    """fp64 and fp32 (CPU) oracle batch statistics of the first batch, per BatchNorm."""
    out = {}
    for dt in (torch.float64, torch.float32):
        rec = []
        T.oracle_forward(mp, trained["flat"], trained["x"], 18, dt, record=rec)
        out[dt] = rec
    return out


@pytest.fixture(scope="module")
def stats_b(batch_stats):
    """Set (b): synthetic statistics far from the batch's own -- mean ~ U(-0.3, 0.3) x the channel's
    batch std, variance ~ U(0.6, 1.6) x the batch variance (on the fp32 grid: the GPU gets these)."""
    g = torch.Generator().manual_seed(5)
    st = []
    for mean, var in batch_stats[torch.float64]:
        u = torch.rand(mean.shape, generator=g, dtype=torch.float64) * 0.6 - 0.3
        k = torch.rand(mean.shape, generator=g, dtype=torch.float64) * 1.0 + 0.6
        st.append((u * var.sqrt(), k * var))
    return T.join_stats(st).float()


@pytest.fixture(scope="module")
def refs(trained, stats_b, mp):
    return {k: T.reference(mp, trained["flat"], trained["x"], T.split_stats(s.double(), 18), 18)
            for k, s in (("a", trained["stats_a"]), ("b", stats_b))}


# ---- 1. state round trip ------------------------------------------------------------------------
def test_state_round_trip(trained):
    from md2hip._lib import lib, ptr, stream_of
    model = _model()
    cache, params = _cfg(N, H, W)
    ex = model.executor((N, 3, 3, H, W), cache, params)
    assert torch.equal(ex.get_bn_stats().cpu(), _initial(model))
    assert torch.equal(trained["fresh"], _initial(model))
    assert torch.equal(model.bn_stats().cpu(), _initial(model))
    g = torch.Generator().manual_seed(3)
    v = torch.randn(model.bn_numel, generator=g)
    off = 0
    for c in model.bn_channels:
        v[off + c:off + 2 * c] = v[off + c:off + 2 * c].abs()
        off += 2 * c
    vg = v.cuda()
    st = stream_of(model.device)
    assert lib().md2_model_set_bn_stats(ex.handle, ptr(vg), st) == 0
    assert torch.equal(ex.get_bn_stats().cpu(), v)
    c0 = model.bn_channels[0]
    for bad in (-1.0, float("nan"), float("inf")):
        w = v.clone()
        w[c0 + 3] = bad                         # a variance of the stem
        wg = w.cuda()
        assert lib().md2_model_set_bn_stats(ex.handle, ptr(wg), st) == MD2_EINVAL
        assert torch.equal(ex.get_bn_stats().cpu(), v)
    w = v.clone()
    w[-1] = -0.5                                # the last variance of the last BatchNorm
    wg = w.cuda()
    assert lib().md2_model_set_bn_stats(ex.handle, ptr(wg), st) == MD2_EINVAL
    assert torch.equal(ex.get_bn_stats().cpu(), v)
    with pytest.raises(ValueError):
        model.load_bn_stats(w)
    with pytest.raises(ValueError):
        model.load_bn_stats(v[:-1])


# ---- 2. the running update ----------------------------------------------------------------------
def test_running_update_is_flux_rule(trained, batch_stats):
    """After one train-mode forward_loss: 0.9 * init + 0.1 * (batch mean, unbiased batch variance),
    per BatchNorm within max(1e-6, 4 x the fp32 CPU oracle's error of the same quantity)."""
    init = T.split_stats(_initial(trained["model"]).double(), 18)
    got = T.split_stats(trained["stats1"].double(), 18)
    worst = 0.0
    for k, (name, _) in enumerate(T.bn_names(18)):
        want, o32 = [torch.cat([0.9 * init[k][j] + 0.1 * batch_stats[dt][k][j].double() for j in (0, 1)])
                     for dt in (torch.float64, torch.float32)]
        err, floor = D.rel_err(torch.cat(got[k]), want), D.rel_err(o32, want)
        bound = max(1e-6, 4 * floor)
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, floor, bound)
    print(f"\nrunning update: worst err / bound {worst:.3f}")


# ---- 3. test-mode parity ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "b"])
def test_testmode_parity(trained, stats_b, refs, mp, kind):
    import md2hip
    model, ref = trained["model"], refs[kind]
    # the inputs make the comparison meaningful: the sigmoid is not saturated ...
    d5 = ref["disps"][-1]
    assert ((d5 > 0.05) & (d5 < 0.95)).double().mean().item() >= 0.9
    if kind == "b":   # ... and batch statistics would give a clearly different answer
        dtrain, _ = T.oracle_forward(mp, trained["flat"], trained["x"], 18, torch.float64)
        for i, (a, b) in enumerate(zip(dtrain, ref["disps"])):
            assert D.rel_err(a, b) > 100 * ref["bound"][f"disp{i}"], (i, D.rel_err(a, b))
    model.load_bn_stats(trained["stats_a"] if kind == "a" else stats_b)
    model.testmode(True)
    try:
        d = md2hip.eval_disparity(model, trained["xg"][:, 1].contiguous())
        T.check(ref, d, None, f"r18_{kind}_eval")
        disps, poses = model(trained["xg"], cache=trained["cache"], params=trained["params"])
        T.check(ref, disps, _pose(poses), f"r18_{kind}_call")
    finally:
        model.testmode(False)


# ---- 4. batch independence ----------------------------------------------------------------------
def test_batch_independence(trained, refs):
    import md2hip
    model, bound = trained["model"], refs["a"]["bound"]
    xt = trained["xg"][:, 1].contiguous()
    model.load_bn_stats(trained["stats_a"])
    model.testmode(True)
    try:
        d2 = md2hip.eval_disparity(model, xt)
        d1 = md2hip.eval_disparity(model, xt[0:1].contiguous())
    finally:
        model.testmode(False)
    for i, (a, b) in enumerate(zip(d1, d2)):
        assert D.rel_err(a, b[0:1]) <= bound[f"disp{i}"], (i, D.rel_err(a, b[0:1]))
    t2 = md2hip.eval_disparity(model, xt)                # train mode: batch statistics
    t1 = md2hip.eval_disparity(model, xt[0:1].contiguous())
    for i, (a, b) in enumerate(zip(t1, t2)):
        assert D.rel_err(a, b[0:1]) > 100 * bound[f"disp{i}"], (i, D.rel_err(a, b[0:1]))
    model.load_bn_stats(trained["stats_a"])


# ---- 5. ResNet-50 -------------------------------------------------------------------------------
def test_resnet50_parity(mp):
    import md2hip
    model = _model(50)
    cache, params = _cfg(1, H, W)
    xs = [_x(1, H, W, s) for s in (7, 8, 9)]
    for x in xs:
        md2hip.train_loss(model, x.float().cuda().contiguous(), None, cache, params)
    stats = model.bn_stats().cpu()
    md2hip.gradient(model)          # no forward left pending: eval_disparity reuses this executor
    ref = T.reference(mp, model.flat.detach().double().cpu(), xs[0], T.split_stats(stats.double(), 50), 50)
    xg = xs[0].float().cuda().contiguous()
    model.testmode(True)
    d = md2hip.eval_disparity(model, xg[:, 1].contiguous())
    T.check(ref, d, None, "r50_a_eval")
    disps, poses = model(xg, cache=cache, params=params)
    T.check(ref, disps, _pose(poses), "r50_a_call")


# ---- 6. mode hygiene ----------------------------------------------------------------------------
def test_training_is_refused_in_test_mode(trained):
    import md2hip
    from md2hip._lib import lib, ptr, stream_of
    model, ex, xg = trained["model"], trained["ex"], trained["xg"]
    st = stream_of(model.device)
    loss = torch.zeros(1, device="cuda")
    am, av = torch.zeros_like(model.flat), torch.zeros_like(model.flat)
    model.testmode(True)
    try:
        ex.sync()
        assert lib().md2_model_testmode(ex.handle) == 1
        calls = {
            "forward_loss": lambda: lib().md2_model_forward_loss(ex.handle, ptr(xg), None, ptr(loss), None, st),
            "backward_from": lambda: lib().md2_model_backward_from(ex.handle, None, None, st),
            "adam": lambda: lib().md2_model_adam(ex.handle, ptr(am), ptr(av), 1e-4, 0.9, 0.999, 1e-8, 1, 1.0, st),
            "train_step": lambda: lib().md2_model_train_step(ex.handle, ptr(xg), None, ptr(am), ptr(av), 1e-4, 1,
                                                             ptr(loss), st),
        }
        for name, call in calls.items():
            assert call() == MD2_ESTATE, name
            assert b"test mode" in lib().md2_last_error(), name
        opt = md2hip.ADAM(1e-4)
        for call in (lambda: md2hip.train_loss(model, xg, None, trained["cache"], trained["params"]),
                     lambda: md2hip.gradient(model), lambda: md2hip.pullback(model),
                     lambda: opt.update(model),
                     lambda: md2hip.train_step(model, xg, None, trained["cache"], trained["params"], opt)):
            with pytest.raises(RuntimeError, match=r"testmode\(False\)"):
                call()
    finally:
        model.testmode(False)
    ex.sync()
    assert lib().md2_model_testmode(ex.handle) == 0
    torch.cuda.synchronize()


def test_statistics_frozen_in_test_mode(trained):
    import md2hip
    model, ex = trained["model"], trained["ex"]
    xt = trained["xg"][:, 1].contiguous()
    model.load_bn_stats(trained["stats_a"])
    model.testmode(True)
    try:
        for _ in range(5):
            md2hip.eval_disparity(model, xt)
            model(trained["xg"], cache=trained["cache"], params=trained["params"])
        assert torch.equal(ex.get_bn_stats().cpu(), trained["stats_a"])
    finally:
        model.testmode(False)
    md2hip.eval_disparity(model, xt)                     # train mode moves them (today's path)
    assert not torch.equal(model.bn_stats().cpu(), trained["stats_a"])
    model.load_bn_stats(trained["stats_a"])


def test_train_path_bit_identical_after_test_mode(trained):
    """Model A: two train steps.  Model B: test mode, eval_disparity, back, the same two steps."""
    import md2hip
    cache, params = trained["cache"], trained["params"]
    xs = [_x(N, H, W, s).float().cuda().contiguous() for s in (7, 8)]
    out = []
    for detour in (False, True):
        model = _model()
        opt = md2hip.ADAM(1e-4)
        if detour:
            model.testmode(True)
            md2hip.eval_disparity(model, xs[0][:, 1].contiguous())
            model(xs[0], cache=cache, params=params)
            model.testmode(False)
        for x in xs:
            md2hip.train_step(model, x, None, cache, params, opt)
        torch.cuda.synchronize()
        out.append((model.flat.cpu(), model.grad.cpu(), model.bn_stats().cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][2], _initial(model))


def test_set_params_refolds(trained, mp):
    """New weights while test mode is on: md2_model_set_params re-folds; parity holds again."""
    import md2hip
    model = _model()
    cache, params = trained["cache"], trained["params"]
    model.executor((N, 3, 3, H, W), cache, params)
    model.load_bn_stats(trained["stats_a"])
    model.testmode(True)
    xt = trained["xg"][:, 1].contiguous()
    before = md2hip.eval_disparity(model, xt)
    g = torch.Generator().manual_seed(11)
    new = md2hip.flux_params(model).cpu() * (1 + 0.2 * torch.randn(model.numel, generator=g))
    md2hip.set_flux_params(model, new)
    d = md2hip.eval_disparity(model, xt)
    assert D.rel_err(d[-1], before[-1]) > 1e-3
    ref = T.reference(mp, model.flat.detach().double().cpu(), trained["x"],
                      T.split_stats(trained["stats_a"].double(), 18), 18)
    T.check(ref, d, None, "r18_set_params_eval")


def test_device_bytes_grow_at_first_switch_only(trained):
    model, ex = trained["model"], trained["ex"]
    assert trained["bytes_trained"] == trained["bytes0"]
    model.testmode(True)
    ex.sync()
    b1 = ex.device_bytes()
    model.testmode(False)
    ex.sync()
    model.testmode(True)
    ex.sync()
    b2 = ex.device_bytes()
    model.testmode(False)
    ex.sync()
    assert b1 > trained["bytes0"] and b2 == b1


# ---- 7. Python state across executors -----------------------------------------------------------
def test_statistics_follow_the_model_across_executors(mp):
    import md2hip
    model = _model()
    cache, params = _cfg(N, H, W)
    md2hip.train_loss(model, _x(N, H, W, 7).float().cuda().contiguous(), None, cache, params)
    first = model._last
    stats = model.bn_stats().cpu()
    assert not torch.equal(stats, _initial(model))
    H2, W2 = 96, 160
    x2 = _x(N, H2, W2, 8)
    xt = x2[:, 1].float().cuda().contiguous()
    model.testmode(True)
    d = md2hip.eval_disparity(model, xt)                 # a new executor: first gets the statistics
    ref = T.reference(mp, model.flat.detach().double().cpu(), x2, T.split_stats(stats.double(), 18), 18)
    T.check(ref, d, None, "r18_cross_executor_eval")
    second = [e for e in model._ex.values() if e is not first]
    assert len(second) == 1 and torch.equal(second[0].get_bn_stats().cpu(), stats)
    # load_bn_stats reaches the executors that already exist
    new = stats.clone()
    new[:64] += 0.25
    model.load_bn_stats(new)
    d2 = md2hip.eval_disparity(model, xt)
    assert torch.equal(second[0].get_bn_stats().cpu(), new)
    assert D.rel_err(d2[-1], d[-1]) > 1e-4
    model.testmode(False)
    first.sync()
    assert torch.equal(first.get_bn_stats().cpu(), new)
