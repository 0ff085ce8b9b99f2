"""GPU: the eager train step with HIP-event profiling on (bench.py --full, tools/layer_table.py, the
roofline).  Profiling runs every launch on the model stream with an event bracket around it and
must change no bit of the step: losses, parameters and ADAM moments equal those of the plain step.
The records cover the three conv passes, one batched launch each for the heads' forward and
backward, and one photometric launch; reading them clears them."""
import math

import pytest
import torch

from tests import _data as D
from tests.test_gpu_fusion import _setup

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 128


def test_profiled_step_bitwise_and_records():
    import md2hip.dist
    xs = [D.triplets(B, 3, H, W, seed=s).float().cuda().contiguous() for s in (5, 6)]
    mp, exp, op = _setup(True, H, W, B)
    mu, exu, ou = _setup(True, H, W, B)
    exp.set_profiling(True)
    comm = md2hip.dist.GradAllReduce(force=False)
    for i, x in enumerate(xs):
        lp = md2hip.dist.train_step(exp, mp, op, x, comm).clone()
        lu = md2hip.dist.train_step(exu, mu, ou, x, comm).clone()
        torch.cuda.synchronize()
        assert torch.equal(lp, lu), (i, lp, lu)
        assert torch.equal(mp.flat, mu.flat), i
        assert torch.equal(op.m, ou.m) and torch.equal(op.v, ou.v), i
        recs = exp.profile_records()
        assert recs, i
        assert all(math.isfinite(ms) and ms >= 0 for _, _, ms, _ in recs), i
        tags = [tag for tag, _, _, _ in recs]
        for pass_ in ("fwd ", "dgrad ", "wgrad "):
            assert any(t.startswith(pass_) for t in tags), (i, pass_)
        for once in ("heads fwd", "heads bwd", "photometric (all scales)"):
            assert tags.count(once) == 1, (i, once, tags.count(once))
        assert exp.profile_records() == [], i
