"""GPU: the one-kernel BatchNorm backward (bn_bwd_channel in bn_bwd.hip: a channel that fits in one
block is summed and applied from registers, MD2_FUSE_BN_BWD) against the two-pass path it replaces
(bn_bwd_partial + bn_bwd_apply_fused, MD2_FUSE_BN_BWD=0).  Both take the same fp64 sums of the same
values, in another order, so dgamma / dbeta / dy agree to the last bits and not bitwise -- the
situation of MD2_FUSE_BNSTATS in the forward, judged by test_fused_bnstats_close's bounds.

The switch is read when the executor is built, so each arm runs in a child process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 128      # 6 images: a channel of layers 1-4 (<= 6*16*32 values) fits in a block
LR = 1e-4

_CHILD = r"""
import os, sys
root, out = sys.argv[1], sys.argv[2]
B, H, W, lr = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6])
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
losses, flats = [], []
for s in (5, 6, 7):
    x = D.triplets(B, 3, H, W, seed=s).float().cuda().contiguous()
    losses.append(float(md2hip.dist.train_step(ex, m, opt, x, comm)))
    torch.cuda.synchronize()
    flats.append(m.flat.cpu().numpy().copy())
np.savez(out, loss=np.array(losses, dtype=np.float64), flat=np.stack(flats))
"""


def _arm(tmp_path, name, value):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MD2_")}
    env["MD2_FUSE_BN_BWD"] = value
    out = str(tmp_path / f"{name}.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, out, str(B), str(H), str(W), str(LR)],
                       env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, (name, r.stderr[-3000:])
    return np.load(out)


@pytest.mark.timeout(420)
def test_fused_bn_bwd_close(tmp_path):
    """Three train steps at B=2 64x128 with MD2_FUSE_BN_BWD=1 against =0: losses within 1e-6
    relative at every step, parameters within ADAM's per-step bound 2*lr*(i+1) + 1e-7 (an update
    can flip where a gradient component sits at the rounding level) -- test_fused_bnstats_close's
    bounds, for the same reason (reordered fp64 sums).  At this shape every BN of
    layers 1-4 fits in a block and takes the one-kernel path in the `on` arm (the stem's 6*32*64
    values per channel do not: two passes in both arms).  Measured on an MI355X: both arms
    bit-identical over the three steps (an fp64 sum rounded to float hides its order almost always),
    which the bounds allow and do not require."""
    on = _arm(tmp_path, "on", "1")
    off = _arm(tmp_path, "off", "0")
    for i in range(3):
        lf, lu = float(on["loss"][i]), float(off["loss"][i])
        dp = float(np.abs(on["flat"][i] - off["flat"][i]).max())
        print(f"step {i}: loss on {lf!r} off {lu!r}; max |dparam| {dp:.3e}")
        assert abs(lf - lu) <= 1e-6 * abs(lu), (i, lf, lu)
        assert dp <= 2.0 * LR * (i + 1) + 1e-7, (i, dp)
