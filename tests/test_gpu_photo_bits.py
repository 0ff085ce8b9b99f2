"""GPU: the photometric kernel (photo.hip) reproduces, bit for bit, the outputs recorded from the
scalar kernel whose arithmetic order it took over (tests/golden/photo_bits.json; the recorder,
the case table and the digest are tests/golden/make_photo_bits.py): every output of the fused loss
tail (loss, per-scale terms, d disparity per scale, d pose, the per-pixel loss / argmin / bilinear
cell maps of the parity diagnostics) and of the op-level warp_photometric fwd / bwd with a
per-pixel cotangent map, at the bench shape (B=12, 416x128, 4 scales) and at odd shapes (one
channel, a 96-wide frame whose level-1 disparity is 6 columns, automasking, near-field poses).
Equality is digest equality: NaNs equal NaNs and -0.0 equals +0.0, nothing else is tolerated.
The inputs are checked first, so a change of the input generators is reported as such."""
import json

import pytest

from tests.golden import make_photo_bits as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(M.FIXTURE) as f:
        return json.load(f)["cases"]


def _check(case, want, ins, outs):
    for name, hexd in want["inputs"].items():
        assert ins.get(name) == hexd, (f"{case}: INPUT {name} is not the recorded one (the input generation "
                                       "changed; the kernel is not at fault)")
    assert set(ins) == set(want["inputs"]), f"{case}: inputs {sorted(set(ins) ^ set(want['inputs']))}"
    for key, hexd in want["outputs"].items():
        assert outs.get(key) == hexd, f"{case}: output {key} differs from the recorded bits"
    assert set(outs) == set(want["outputs"]), f"{case}: outputs {sorted(set(outs) ^ set(want['outputs']))}"


@pytest.mark.parametrize("name", list(M.TAIL_CASES))
@pytest.mark.parametrize("vis", list(M.VISUALIZE))
def test_photo_bits_loss_tail_equals_recorded_scalar_kernel(name, vis, recorded):
    case = M.tail_id(name, vis)
    ins, outs = M.run_tail_case(name, M.VISUALIZE[vis])
    _check(case, recorded[case], ins, outs)


@pytest.mark.parametrize("scale", M.OP_SCALES)
def test_photo_bits_warp_op_with_cotangent_map_equals_recorded(scale, recorded):
    """md2_warp_photometric_fwd / _bwd (one scale, per-pixel cotangent map = the kernel's gmap
    path) through the op-level API."""
    case = M.op_id(scale)
    ins, outs = M.run_op_case(scale)
    _check(case, recorded[case], ins, outs)
