"""Writes tests/golden/conv_workspace_sizes.json: md2_conv2d_ex_workspace_size over a grid of conv
shapes, one list per row  [n, cin, cout, k, stride, pad, reflect, h, w, cin_w, bytes].

The fixture characterises the library it is run against, so it is recorded from the commit BEFORE
a change to the conv dispatch and then held fixed (tests/test_conv_route_sizes.py):

    MD2HIP_LIB=/path/to/parent/libmd2hip.so python tests/golden/make_conv_workspace_sizes.py

(MD2HIP_LIB selects the library, as for tools/step_digest.py; default: the in-tree build.)

Rows: every conv of the flagship model (ResNet-18 encoder at 416 x 128, B = 12 -- encoder batch
36 --, the depth decoder with its heads, the pose decoder), then a seeded sample of the cross
product of N x CH x CH x KERNELS x MAPS x {cin_w = 0, cin - 16}, up to 1500 rows in all; a row the
library refuses (check_shape / ex_check_shape: size 0) is left out."""
import ctypes as C
import itertools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "monodepth2.jl_amd")]

MAX_ROWS = 1500
N = (1, 2, 6, 12, 36)
CH = (1, 3, 16, 32, 48, 64, 96, 128, 256, 512)
KERNELS = ((1, 1, 0, 0), (1, 2, 0, 0), (3, 1, 1, 0), (3, 1, 1, 1), (3, 2, 1, 0), (7, 2, 3, 0))   # k, stride, pad, reflect
MAPS = ((2, 4), (4, 13), (6, 10), (6, 12), (7, 9), (8, 24), (8, 200), (16, 52), (32, 104), (64, 208), (128, 416))


def model_rows():
    """(n, cin, cout, k, stride, pad, reflect, h, w, cin_w) of every conv of the flagship model."""
    rows = [(36, 3, 64, 7, 2, 3, 0, 128, 416, 0)]                        # stem
    h, w, cin = 32, 104, 64
    for cout in (64, 128, 256, 512):                                      # layer1..4, two basic blocks each
        s = 1 if cout == 64 else 2
        rows.append((36, cin, cout, 3, s, 1, 0, h, w, 0))                 # block 1 conv1
        if s == 2:
            rows.append((36, cin, cout, 1, 2, 0, 0, h, w, 0))             # its downsample
            h, w = h // 2, w // 2
        rows.append((36, cout, cout, 3, 1, 1, 0, h, w, 0))                # conv2 and block 2
        cin = cout
    dec, skip = (256, 128, 64, 32, 16), (256, 128, 64, 64, 0)
    h, w, cin = 4, 13, 512
    for b in range(5):                                                    # depth decoder branches
        rows.append((12, cin, dec[b], 3, 1, 1, 1, h, w, 0))               # c1
        h, w = 2 * h, 2 * w
        rows.append((12, dec[b] + skip[b], dec[b], 3, 1, 1, 1, h, w, 0))  # c2 on (up || skip)
        if b >= 1:
            rows.append((12, dec[b], 1, 3, 1, 1, 1, h, w, 0))             # disparity head
        cin = dec[b]
    rows.append((36, 512, 256, 1, 1, 0, 0, 4, 13, 0))                     # pose squeezer
    for n in (12, 24):                                                    # pose decoder (per source pair / both)
        rows += [(n, 512, 256, 3, 1, 1, 0, 4, 13, 0), (n, 256, 256, 3, 1, 1, 0, 4, 13, 0),
                 (n, 256, 6, 1, 1, 0, 0, 4, 13, 0)]
    return rows


def grid_rows():
    out = []
    for n, cin, cout, (k, s, p, r), (h, w) in itertools.product(N, CH, CH, KERNELS, MAPS):
        out.append((n, cin, cout, k, s, p, r, h, w, 0))
        if cin > 16 and cin % 16 == 0 and cout > 1:
            out.append((n, cin, cout, k, s, p, r, h, w, cin - 16))
    return out


def workspace_size(lib, row):
    from md2hip._lib import ConvDesc, ConvOperands
    n, cin, cout, k, s, p, r, h, w, cin_w = row
    d = ConvDesc(n=n, cin=cin, h=h, w=w, cout=cout, kh=k, kw=k, stride=s, pad=p, reflect=r, act=0)
    o = ConvOperands(cin_w=cin_w)
    return lib.md2_conv2d_ex_workspace_size(C.byref(d), C.byref(o) if cin_w else None)


def load():
    from md2hip import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    res, args = _lib._SIGS["md2_conv2d_ex_workspace_size"]
    lib.md2_conv2d_ex_workspace_size.restype, lib.md2_conv2d_ex_workspace_size.argtypes = res, args
    return lib


def main():
    lib = load()
    rows, seen = [], set()
    pool = grid_rows()
    random.Random(20).shuffle(pool)
    for row in model_rows() + pool:
        if len(rows) == MAX_ROWS:
            break
        if row in seen:
            continue
        seen.add(row)
        b = workspace_size(lib, row)
        if b:
            rows.append(list(row) + [b])
    with open(os.path.join(HERE, "conv_workspace_sizes.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows")


if __name__ == "__main__":
    main()
