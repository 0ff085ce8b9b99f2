"""GPU: md2_model_eval_pose -- the PoseDecoder on consecutive frames without the DepthDecoder -- and
the evaluate_pose driver.  ResNet-18, N = 2, 64x128 (the configuration of tests/test_gpu_testmode.py);
references and the pose bound are those of tests/_testmode.py: the fp64 oracle with the BatchNorms on
the running statistics, max(1e-6, 2 x the fp32 floor over four realisations).  A batch of another
shape may take another conv route, so eval_pose is held to that bound against the forward's poses,
not to bit equality (as test_batch_independence treats disparities)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _data as D
from tests import _pose_ref as R
from tests import _testmode as T

pytestmark = pytest.mark.gpu

N, H, W = 2, 64, 128
MD2_EINVAL, MD2_ENOTSUP, MD2_ESTATE = 1, 3, 5


def _model(emb=0, seed=42):
    import md2hip
    enc = md2hip.ResNet(18, in_channels=3)
    return md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                 embedding_levels=emb),
                        md2hip.PoseDecoder(enc.stages[-1]), seed=seed)


def _cfg(n):
    import md2hip
    K, invK = D.intrinsics(W, H)
    return (md2hip.TrainCache(K=K.numpy(), invK=invK.numpy()),
            md2hip.Params(target_size=(W, H), batch_size=n, automasking=False))


def _x(n, seed):
    return D.triplets(n, 3, H, W, seed=seed)


def _pose(poses):
    return torch.cat([torch.cat([p.rvec, p.tvec], 1) for p in poses], 0)


def _eval_pose_raw(ex, x, n):
    """(rc, poses or None) of md2_model_eval_pose on the executor itself."""
    from md2hip._lib import lib, ptr, stream_of
    from md2hip.model import _wrap
    pp = C.c_void_p()
    rc = lib().md2_model_eval_pose(ex.handle, ptr(x), n, C.byref(pp), stream_of(x.device))
    return rc, (_wrap(pp.value, (n - 1, 6), x.device) if rc == 0 else None)


@pytest.fixture(scope="module")
def mp():
    with pytest.MonkeyPatch.context() as m:
        yield m


@pytest.fixture(scope="module")
def trained(mp):
    """A ResNet-18 model whose running statistics come from three train-mode forwards, the fp64
    test-mode oracle of the first batch, and the model's own forward of it in test mode."""
    import md2hip
    model = _model()
    cache, params = _cfg(N)
    xs = [_x(N, s) for s in (7, 8, 9)]
    ex = model.executor((N, 3, 3, H, W), cache, params)
    for x in xs:
        md2hip.train_loss(model, x.float().cuda().contiguous(), None, cache, params)
    stats = model.bn_stats().cpu()
    md2hip.gradient(model)          # no forward left pending: the eval calls may reuse this executor
    torch.cuda.synchronize()
    ref = T.reference(mp, model.flat.detach().double().cpu(), xs[0], T.split_stats(stats.double(), 18), 18)
    xg = xs[0].float().cuda().contiguous()
    model.load_bn_stats(stats)
    model.testmode(True)
    disps, poses = model(xg, cache=cache, params=params)
    fwd_pose = _pose(poses).clone()
    T.check(ref, disps, fwd_pose, "r18_eval_pose_forward")
    return {"model": model, "ex": ex, "cache": cache, "params": params, "xg": xg, "ref": ref,
            "fwd_pose": fwd_pose, "stats": stats}


# ---- parity -----------------------------------------------------------------------------------------
def test_parity_with_forward_and_oracle(trained):
    """The three frames of sample i as one eval_pose call: row 0 = pair (frame 0, frame 1) = row i of
    the forward's poses, row 1 = pair (frame 1, frame 2) = row N + i."""
    import md2hip
    model, ref, fwd = trained["model"], trained["ref"], trained["fwd_pose"]
    bound = ref["bound"]["pose"]
    got = torch.empty(2 * N, 6, device="cuda")
    for i in range(N):
        p = md2hip.eval_pose(model, trained["xg"][i].contiguous())
        assert p.shape == (2, 6)
        got[i], got[N + i] = p[0], p[1]
    for row in (0, N):                                   # sample 0, as the forward wrote them
        e = D.rel_err(got[row], fwd[row])
        print(f"\neval_pose row {row}: {e:.2e} from the forward's (bound {bound:.2e})")
        assert e <= bound, (row, e, bound)
    assert D.rel_err(got, fwd) <= bound
    sub = {"disps": [], "pose": ref["pose"], "floor": ref["floor"], "bound": ref["bound"],
           "realisations": ref["realisations"]}
    T.check(sub, [], got, "r18_eval_pose")
    # the poses are not degenerate: the two pairs of a sample differ by far more than the bound
    assert D.rel_err(got[0], got[N]) > 100 * bound


def test_shape_limits(trained):
    from md2hip._lib import lib
    model, ex = trained["model"], trained["ex"]
    ex.sync()
    assert lib().md2_model_testmode(ex.handle) == 1
    x6 = trained["xg"].reshape(3 * N, 3, H, W)
    for n in (2, 2 * N + 1):
        rc, p = _eval_pose_raw(ex, x6, n)
        assert rc == 0 and p.shape == (n - 1, 6) and torch.isfinite(p).all(), (n, rc)
    for n in (1, 0, -3, 2 * N + 2):
        rc, _ = _eval_pose_raw(ex, x6, n)
        assert rc == MD2_EINVAL, (n, rc)
        assert b"eval_pose" in lib().md2_last_error()
    torch.cuda.synchronize()


def test_window_consistency(trained):
    """Row i of a 5-frame call = the 2-frame call on frames (i, i+1): test mode makes a pair's pose
    independent of its window."""
    import md2hip
    model, bound = trained["model"], trained["ref"]["bound"]["pose"]
    x5 = trained["xg"].reshape(3 * N, 3, H, W)[:5].contiguous()
    p5 = md2hip.eval_pose(model, x5).clone()
    assert p5.shape == (4, 6)
    for i in range(4):
        p2 = md2hip.eval_pose(model, x5[i:i + 2].contiguous())
        e = D.rel_err(p2[0], p5[i])
        assert p2.shape == (1, 6) and e <= bound, (i, e, bound)
    # the running statistics did not move
    assert torch.equal(trained["ex"].get_bn_stats().cpu(), trained["stats"])


# ---- state ------------------------------------------------------------------------------------------
def test_backward_is_refused_after_eval_pose():
    import md2hip
    from md2hip._lib import lib, stream_of
    model = _model()
    cache, params = _cfg(N)
    xg = _x(N, 7).float().cuda().contiguous()
    md2hip.train_loss(model, xg, None, cache, params)
    ex = model._last
    rc, p = _eval_pose_raw(ex, xg.reshape(3 * N, 3, H, W), 3)
    assert rc == 0
    st = stream_of(model.device)
    off, ln = C.c_longlong(), C.c_longlong()
    assert lib().md2_model_backward_segment(ex.handle, 0, C.byref(off), C.byref(ln), st) == MD2_ESTATE
    md2hip.train_loss(model, xg, None, cache, params)            # the next forward_loss: backward again
    assert lib().md2_model_backward_segment(ex.handle, 0, C.byref(off), C.byref(ln), st) == 0
    torch.cuda.synchronize()


def test_train_step_unchanged_by_an_eval_pose_before_it():
    import md2hip
    cache, params = _cfg(N)
    xg = _x(N, 7).float().cuda().contiguous()
    out = []
    for detour in (False, True):
        model = _model()
        ex = model.executor((N, 3, 3, H, W), cache, params)
        if detour:                                        # on the executor the step then runs on
            p = md2hip.eval_pose(model, _x(N, 8).float().cuda().reshape(3 * N, 3, H, W)[:5].contiguous())
            assert torch.isfinite(p).all() and len(model._ex) == 1
        loss, *_ = md2hip.train_loss(model, xg, None, cache, params)
        md2hip.gradient(model)
        torch.cuda.synchronize()
        out.append((loss.cpu(), model.grad.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][1].abs().max() > 0


def test_mpi_mode_is_not_supported():
    import md2hip
    from md2hip._lib import lib
    model = _model(emb=21)
    cache, params = _cfg(1)
    ex = model.executor((1, 3, 3, H, W), cache, params, num_bins=4)
    x = _x(1, 7).float().cuda().reshape(3, 3, H, W).contiguous()
    rc, _ = _eval_pose_raw(ex, x, 2)
    assert rc == MD2_ENOTSUP and b"MPI" in lib().md2_last_error()
    with pytest.raises(NotImplementedError):
        md2hip.eval_pose(model, x)


# ---- driver -----------------------------------------------------------------------------------------
def test_evaluate_pose_driver(trained):
    import md2hip
    model = trained["model"]
    x_seq = _x(3, 12).float().cuda().reshape(9, 3, H, W).contiguous()
    _, gt = R.make_case(4, 8, invert=True)
    windows = md2hip.pose_windows(x_seq, 2 * N)
    assert [int(w.shape[0]) for w in windows] == [5, 5]
    res = md2hip.evaluate_pose(model, windows, gt, track_length=5)
    pred = torch.cat([md2hip.eval_pose(model, w) for w in windows])
    assert pred.shape == (8, 6)
    o, s, c = md2hip.pose_errors(pred, torch.from_numpy(gt).cuda(), track_length=5, invert=True)
    s, c = s.cpu().numpy(), c.cpu().numpy()
    assert res["ate_mean"] == float(s[0, 0]) and res["ate_std"] == float(s[0, 1])
    assert res["snippets"] == 5 == int(c[0, 0]) and res["n_bad"] == 0 and res["nonfinite_inputs"] == 0
    assert np.isfinite(res["ate_mean"]) and res["ate_mean"] > 0 and 0 <= res["rot_deg_mean"] <= 180
    # a NaN pixel: the ReLUs hide it from the poses, the input check does not
    bad = x_seq.clone()
    bad[6, 1, 10, 20] = float("nan")
    with pytest.raises(RuntimeError, match="not finite"):
        md2hip.evaluate_pose(model, md2hip.pose_windows(bad, 2 * N), gt)
    res = md2hip.evaluate_pose(model, md2hip.pose_windows(bad, 2 * N), gt, allow_nonfinite=True)
    assert res["nonfinite_inputs"] == 1 and res["snippets"] == 5
    with pytest.raises(ValueError, match="gt_rel must be"):
        md2hip.evaluate_pose(model, windows, gt[:7])
