"""GPU: the one-kernel BatchNorm forward (bn_fwd_channel in bn_fwd.hip: a channel that fits in one
block is summed and applied from registers, MD2_FUSE_BN_FWD) against the two passes it replaces
(bn_stats_partial[_slabs] + bn_apply_fused, MD2_FUSE_BN_FWD=0).  Both take the same fp64 sums of
the same values, in another order, and finalise them with the same device code, so mean / invstd
agree to an ulp and not bitwise by construction -- the situation of MD2_FUSE_BNSTATS and
MD2_FUSE_BN_BWD, judged by the same bounds (test_fused_bnstats_close, test_fused_bn_bwd_close).

The switch is read when the executor is built, so each arm runs in a child process of its own;
an arm is run once per shape and shared by the tests that read it."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 2                     # 6 images
LR = 1e-4

# argv: root, out, B, H, W, lr, steps.  After the first step: the running statistics, and the
# test-mode disparities of that step's target frames (test mode reads, never writes, the state).
_CHILD = r"""
import os, sys
root, out = sys.argv[1], sys.argv[2]
B, H, W, lr, steps = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]), int(sys.argv[7])
sys.path[:0] = [root, os.path.join(root, "monodepth2.jl_amd")]
import numpy as np, torch, md2hip, md2hip.dist
from tests import _data as D
enc = md2hip.ResNet(18, in_channels=3)
m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                          embedding_levels=0), md2hip.PoseDecoder(512), seed=42)
K, invK = D.intrinsics(W, H)
ex = m.executor((B, 3, 3, H, W), md2hip.TrainCache(K=K.numpy(), invK=invK.numpy()),
                md2hip.Params(target_size=(W, H), batch_size=B, automasking=True))
opt = md2hip.ADAM(lr)
comm = md2hip.dist.GradAllReduce(force=False)
losses, flats, extra = [], [], {}
for i, s in enumerate((5, 6, 7)[:steps]):
    x = D.triplets(B, 3, H, W, seed=s).float().cuda().contiguous()
    losses.append(float(md2hip.dist.train_step(ex, m, opt, x, comm)))
    torch.cuda.synchronize()
    flats.append(m.flat.cpu().numpy().copy())
    if i == 0:
        extra["bn_stats"] = m.bn_stats().cpu().numpy().copy()
        m.testmode(True)
        try:
            disps = md2hip.eval_disparity(m, x[:, 1].contiguous())
            torch.cuda.synchronize()
        finally:
            m.testmode(False)
        for k, d in enumerate(disps):
            extra[f"disp{k}"] = d.cpu().numpy().copy()
        extra["ndisp"] = np.array(len(disps))
np.savez(out, loss=np.array(losses, dtype=np.float64), flat=np.stack(flats), **extra)
"""


def _arm(tmp, H, W, steps, value, **more):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MD2_")}
    env["MD2_FUSE_BN_FWD"] = value
    env.update(more)
    out = str(tmp / f"bn_fwd_{H}x{W}_{value}.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, out, str(B), str(H), str(W), str(LR), str(steps)],
                       env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, (H, W, value, r.stderr[-3000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def arms_128(tmp_path_factory):
    """B=2 64x128, three steps: every BatchNorm of layers 1-4 fits in a block (<= 6*16*32 values),
    so the `on` arm runs all three forms of the kernel, from slabs and from y."""
    tmp = tmp_path_factory.mktemp("bn_fwd_128")
    return _arm(tmp, 64, 128, 3, "1"), _arm(tmp, 64, 128, 3, "0")


@pytest.fixture(scope="module")
def arms_96(tmp_path_factory):
    """B=2 64x96, one step: layer 4 is 2x3, HW % 4 != 0 -- two passes there in both arms, the
    one kernel on layers 1-3 of the `on` arm."""
    tmp = tmp_path_factory.mktemp("bn_fwd_96")
    return _arm(tmp, 64, 96, 1, "1"), _arm(tmp, 64, 96, 1, "0")


def _close(on, off, steps):
    bitwise = True
    for i in range(steps):
        lf, lu = float(on["loss"][i]), float(off["loss"][i])
        dp = float(np.abs(on["flat"][i] - off["flat"][i]).max())
        bitwise = bitwise and lf == lu and dp == 0.0
        print(f"step {i}: loss on {lf!r} off {lu!r}; max |dparam| {dp:.3e}")
        assert abs(lf - lu) <= 1e-6 * abs(lu), (i, lf, lu)
        assert dp <= 2.0 * LR * (i + 1) + 1e-7, (i, dp)
    print("arms bitwise equal (losses, parameters):", bitwise)


@pytest.mark.timeout(420)
def test_fused_bn_fwd_close(arms_128):
    """Three train steps (seeds 5, 6, 7, automasking) with MD2_FUSE_BN_FWD=1 against =0: losses
    within 1e-6 relative at every step, parameters within ADAM's per-step bound
    2*lr*(i+1) + 1e-7 (test_fused_bn_bwd_close's bounds, for the same reason: reordered fp64 sums).
    After the first step the running statistics of the arms agree within rtol 1e-6, atol 1e-10: a
    few fp32 ulps on values that come from fp64 sums rounded once (later steps inherit parameter
    differences and are not compared this tightly).  The stem's 6*32*64 values per channel do not
    fit: two passes in both arms.  Measured on an MI355X: both arms bit-identical over the three
    steps, running statistics included (an fp64 sum rounded to float hides its order almost
    always), which the bounds allow and do not require."""
    on, off = arms_128
    _close(on, off, 3)
    a, b = on["bn_stats"], off["bn_stats"]
    d = np.abs(a - b)
    rel = float((d / np.maximum(np.abs(b), 1e-30)).max())
    print(f"bn_stats after step 0: max |d| {float(d.max()):.3e}, max rel {rel:.3e}, "
          f"bitwise equal: {bool(np.array_equal(a, b))}")
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-10)


@pytest.mark.timeout(420)
def test_fused_bn_fwd_fallback(arms_96):
    """One step at 64x96: the predicate's edge (layer 4 has HW = 6) and the mixed path, same bounds."""
    on, off = arms_96
    _close(on, off, 1)


@pytest.mark.timeout(420)
def test_fused_bn_fwd_plain_y(tmp_path):
    """One step at 64x128 with the convs reducing their own split-K slabs and no statistics in a
    conv epilogue (MD2_FUSE_SPLITK=0, MD2_FUSE_BNSTATS=0 in both arms): every BatchNorm of layers
    1-4 reaches the kernel with a finished y -- its form without slabs, whatever the conv planner
    decides at the other shapes.  Same bounds."""
    plain = {"MD2_FUSE_SPLITK": "0", "MD2_FUSE_BNSTATS": "0"}
    on = _arm(tmp_path, 64, 128, 1, "1", **plain)
    off = _arm(tmp_path, 64, 128, 1, "0", **plain)
    _close(on, off, 1)
    np.testing.assert_allclose(on["bn_stats"], off["bn_stats"], rtol=1e-6, atol=1e-10)


@pytest.mark.timeout(420)
def test_fused_bn_fwd_inference(arms_128):
    """After one train step in each arm: testmode(True) + eval_disparity on that step's target
    frames.  The running statistics and the stored mean / invstd feed the folded inference as
    before: disparities within 1e-6 absolute."""
    on, off = arms_128
    n = int(on["ndisp"])
    assert n == int(off["ndisp"]) and n >= 1
    for k in range(n):
        a, b = on[f"disp{k}"], off[f"disp{k}"]
        assert a.shape == b.shape and np.isfinite(a).all()
        d = float(np.abs(a - b).max())
        print(f"disp{k} {a.shape}: max |on - off| {d:.3e}, bitwise equal: {bool(np.array_equal(a, b))}")
        assert d <= 1e-6, (k, d)
