"""md2_conv2d_ex_workspace_size against tests/golden/conv_workspace_sizes.json, recorded from the
commit before the conv passes took their kernel from one route (csrc/conv_route.hip) by
tests/golden/make_conv_workspace_sizes.py: the sizes a caller allocates did not change.

Equality is required for every row, except where the earlier sizing reserved slabs for a kernel
the shape can never run; there the size may only shrink.  Those shape classes are listed in
SMALLER with their reason; a row outside them must be equal.  Host arithmetic: needs the built
library and no GPU."""
import json
import os

import pytest

from tests.golden import make_conv_workspace_sizes as G
from tests.test_julia_shim import LIB

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_workspace_sizes.json")

def _stem_s2d_shape(cin, h, w):
    return cin == 3 and h % 2 == 0 and w % 2 == 0 and (w // 2) % 16 == 0


# (name, predicate over a row, reason): the only rows that may be smaller than recorded.
# Row: n, cin, cout, k, stride, pad, reflect, h, w, cin_w, bytes
SMALLER = [
    ("forward on conv_px16",
     lambda r: r[3] == 3 and r[4] == 1 and r[1] % 16 == 0 and 1 < r[2] <= 16,
     "3x3 stride-1 forwards with Cin % 16 == 0 and Cout <= 16 run the 16-row kernel, which has no split-K; the "
     "earlier sizing also reserved the tile kernel's split-K slabs, and no operand form sends such a shape there"),
    ("reflect data gradient on the halo kernel",
     lambda r: r[6] == 1 and r[9] == 0 and r[1] % 32 == 0 and r[1] > 32 and r[2] % 16 == 0,
     "the reflect-padded 3x3 data gradient with Cin % 32 == 0, Cin > 32, Cout % 16 == 0 runs on the padded grid "
     "(slabs + the padded image); the earlier sizing also took the maximum with conv_px3's tile slabs, and the data "
     "gradient has no operand form that falls back to the tile"),
    ("stem filter gradient off the space-to-depth kernel",
     lambda r: r[3] == 7 and r[1] <= 4 and r[2] == 64 and not _stem_s2d_shape(r[1], r[7], r[8]),
     "7x7/2 stems (Cin <= 4, Cout 64) whose shape the space-to-depth kernel refuses (Cin != 3, odd H or W, "
     "Wo % 16 != 0) run conv_wgrad_stem_kernel's own splits; the earlier sizing reserved one slab per "
     "space-to-depth block regardless"),
]


@pytest.fixture(scope="module")
def rows():
    with open(FIXTURE) as f:
        return [tuple(r) for r in json.load(f)]


def test_fixture_covers_the_model_and_the_grid(rows):
    assert 0 < len(rows) <= G.MAX_ROWS
    have = {r[:-1] for r in rows}
    assert len(have) == len(rows), "duplicate rows"
    for m in G.model_rows():
        assert m in have, m
    grid = set(G.grid_rows()) | set(G.model_rows())
    assert have <= grid
    # every kernel / stride / padding form and every map of the grid is present
    assert {r[3:7] for r in rows} >= set(G.KERNELS)
    assert {r[7:9] for r in rows} >= set(G.MAPS)
    assert any(r[9] for r in rows), "no cin_w row"


def test_workspace_sizes_are_the_recorded_ones(rows):
    assert os.path.exists(LIB), "build libmd2hip.so first (make -C monodepth2.jl_amd/csrc)"
    lib = G.load()
    bad = []
    for r in rows:
        got, want = G.workspace_size(lib, r[:-1]), r[-1]
        if got == want:
            continue
        if 0 < got < want and any(pred(r) for _, pred, _ in SMALLER):
            continue
        bad.append((r[:-1], got, want))
    assert not bad, (len(bad), bad[:10])
