"""The conv tile kernels are built for the tiles the planners can choose and for no others
(csrc/conv_plan.h: MD2_PX_TILES, MD2_W_TILES; the enums, the BM / BN lookups and the launchers'
dispatch are generated from those two lists).

CPU: the knobs that reached the tiles and the conv_px16 width no longer built are not in the
library.  GPU: no default route ends in the launchers' "tile without a launcher" error."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import md2_oracle as O
from tests import _data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "monodepth2.jl_amd", "lib", "libmd2hip.so")


def test_removed_tile_knobs_not_in_the_library():
    """MD2_PX_TILE selected a fwd / dgrad tile by number and MD2_PX16_BN the 256-pixel conv_px16
    block; both went with the kernels they reached."""
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    blob = open(LIB, "rb").read()
    for knob in (b"MD2_PX_TILE", b"MD2_PX16_BN"):
        assert knob not in blob, knob
    assert b"MD2_W_TILE" in blob      # the wgrad knob stays (the numbers of the built tiles)


# (x_shape, cout, stride, reflect): 3x3, pad 1.  The stride-1 shapes in both paddings: the padding
# decides the route (zero padding: the LDS-halo kernels; reflect: tiles where no halo form exists).
TILE_CASES = [
    ((2, 64, 8, 16), 64, 1, False),
    ((2, 64, 8, 16), 64, 1, True),
    ((2, 32, 8, 16), 32, 1, False),
    ((2, 32, 8, 16), 32, 1, True),
    ((2, 64, 8, 16), 128, 2, False),
]


@pytest.mark.gpu
def test_default_routes_reach_a_launcher():
    """fwd, dgrad and wgrad of (2, 64, 8, 16) -> 64 and (2, 32, 8, 16) -> 32 (3x3 stride 1) and
    (2, 64, 8, 16) -> 128 (3x3 stride 2) on the default routes: every call succeeds (a plan whose
    tile had no launcher case would raise: MD2_EINVAL) and is within 1e-5 of fp64, the bound of
    tests/test_gpu_conv.py.  The kernel each call ran is printed.

    Tiles these shapes reach through the generated dispatch by default: T64x64 (the stride-2
    forward, conv_px3), T32x128 (the 32 -> 32 data gradients, conv_px) and W64x192 (the reflect
    64 -> 64 and the stride-2 filter gradients); the other calls run kernels of their own (halo,
    halo2d, halo_rfl_dgrad, halo_s2, whalo, wgrad16).  W64x128, W64x64 and W32x128 are reached by
    cases of tests/test_gpu_conv.py (and W64x64 by MD2_W_TILE=2 in tests/test_gpu_fusion.py)."""
    from md2hip import ops
    dev = torch.device("cuda")
    for xs, cout, stride, reflect in TILE_CASES:
        g = torch.Generator().manual_seed(5)
        x = torch.randn(*xs, generator=g, dtype=torch.float64).float().double()
        w = (torch.randn(cout, xs[1], 3, 3, generator=g, dtype=torch.float64) / (xs[1] * 9) ** 0.5).float().double()
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        pre = (F.conv2d(O.pad_reflect(xr, 1), wr, stride=stride) if reflect
               else F.conv2d(xr, wr, stride=stride, padding=1))
        dy = torch.randn(pre.shape, generator=g, dtype=torch.float64).float().double()
        pre.backward(dy)
        xg, wg, dyg = x.float().to(dev), w.float().to(dev), dy.float().to(dev)
        ran = []
        y = ops.conv2d(xg, wg, None, stride=stride, pad=1, reflect=reflect)
        ran.append(ops.conv_last_kernel())
        dx = ops.conv2d_dgrad(dyg, wg, xs, stride=stride, pad=1, reflect=reflect)
        ran.append(ops.conv_last_kernel())
        dw, _ = ops.conv2d_wgrad(xg, dyg, tuple(w.shape), stride=stride, pad=1, reflect=reflect, bias=False)
        ran.append(ops.conv_last_kernel())
        torch.cuda.synchronize()
        errs = [D.rel_err(y, pre.detach()), D.rel_err(dx, xr.grad), D.rel_err(dw, wr.grad)]
        print(xs, cout, f"s{stride}", "reflect" if reflect else "zero", ran, ["%.2e" % e for e in errs])
        assert max(errs) < 1e-5, (xs, cout, stride, reflect, ran, errs)
