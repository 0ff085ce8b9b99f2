"""The conv kernels in the operand forms the train step feeds them (md2_conv2d_*_ex, csrc/conv.h
TensorIn / TensorOut / ConvShape.cin_w / SplitKDefer), each against F.conv2d in fp64 on
fp32-representable inputs (as tests/test_gpu_conv.py, whose shapes all use the plainest operands).

Every case asserts
  * the route: md2_conv_last_kernel() names the kernel family the case is listed under;
  * the values: D.rel_err < 1e-5 per destination part (the p0 rows and the p1 rows separately);
    accumulating calls ||got - (init + ref)|| / ||ref|| < 1e-5 with init = seeded randn scaled to
    ref's rms (the one fp32 add contributes ~1e-7: 2^-24 * ||init + ref|| / ||ref||);
  * nothing else is written: destinations are channel windows of wider tensors with 64 guard
    floats either side, prefilled with a finite sentinel that must be bit-identical afterwards;
  * determinism: a second call on fresh copies of the same inputs gives the same bits.

form x family -> case id (test function[case])
  a concat input     fwd   px3             test_concat[32+64-32], [16+32-20 ragged]
                           px16            test_concat[16+16-16]
                           px3             test_concat[256+256-256@2x4]
                           halo            test_concat[64+64-64], [128+128-128], [256+256-256@4x13],
                                           [16+32-64], [32+64-64]
                           halo2d          test_concat[32+64-32 wide]
                           halo (overlap)  test_concat[pose 256+256 shift N], [pose 256+256 shift 1]
                     wgrad wgrad16         test_concat[32+64-32], [16+16-16], [16+32-20 ragged], [32+64-32 wide]
                           wgrad_tile c16  test_concat[16+32-64]
                           wgrad_px3 c32   test_concat[32+64-64]
                           wgrad_px3 c64   test_concat[64+64-64]            (64x192 tiles)
                           wgrad_px3 c128  test_concat[128+128-128], [256+256-256@*], [pose 256+256 *]
                           whalo           test_concat[pose 512 one tensor]  (the same shape, no split)
  b split / strided / accumulating output
                     dgrad px3             test_split_dgrad[32+64-32], [256+256-256@2x4]
                           halo_rfl_dgrad  test_split_dgrad[64+64-64], [128+128-128], [256+256-256@4x13],
                                           [64+64-64 mpi stride]
                     dgrad accumulate      test_accumulate_dgrad[512-256@2x4 split-K] (px3),
                                           [512-256@4x13 split-K] (halo_rfl_dgrad),
                                           [64-32] (halo_rfl_dgrad, one split), [64-128/2] (halo_s2),
                                           [16-16] (px), [head 64-1@4x13] (head_fallback),
                                           test_head_then_c1_dgrad (head_batched, then halo_rfl_dgrad
                                           accumulating into the head's dx)
                     dgrad stride 2  px3   test_stride2_dgrad[1x1/2 64-128@8x12], [3x3/2 48-96@8x12] (the four
                                           output-parity classes merged into one launch; taps 1 resp. 1/2/2/4
                                           per class), [3x3/2 64-128@7x9] (odd H and W: four class launches
                                           with unequal extents), test_accumulate_dgrad[64-128/2@7x9] (the same, +=)
                                     px    test_stride2_dgrad[3x3/2 32-64@8x12] (Cin <= 32: the 32-row tile,
                                           four class launches)
                     head shape, concat / split  test_head_shape_with_concat_or_split_runs_the_generic_kernels
                                           (px, wgrad16, px: the head kernels take one tensor only)
                     wgrad accumulate      test_accumulate_wgrad[64+64-64] (wgrad_px3 tile, one split),
                                           [64+64-64@16x16 split-K] (wgrad_px3 tile, split-K),
                                           [pose 512 one tensor] (whalo, split-K)
  c cin_w            fwd/dgrad/wgrad       test_cin_w[3x3 concat], [3x3], [1x1]  (px3, px3, wgrad_px3 c32)
  d frame-major stem fwd   stem_s2d        test_stem_frame_major[3x32x64], [3x4x96]
                           px              test_stem_frame_major[3x18x44]
                     wgrad stem_wgrad_s2d  test_stem_frame_major[3x32x64], [3x4x96]
                           stem_wgrad      test_stem_frame_major[3x18x44]
  e deferred split-K fwd   px3             test_deferred_splitk[fwd 256-512/2@4x8], [fwd 512-512@2x4]
                           halo            test_deferred_splitk[fwd 512-512@4x13]
                     dgrad px3, halo       test_deferred_splitk[dgrad 512-512@2x4], [dgrad 512-512@4x13]
                     declined              test_deferral_declined[bias], [act], [accumulate], [split output]
    statistics       fwd   halo            test_epilogue_statistics[ragged], [small images], [M=128]
  f bias partials    act_backward_bias     test_act_backward_bias[*]; wgrad16 test_bias_partials_into_wgrad

The statistics epilogue (conv_halo.inc) sums, per channel and 256-pixel tile, the fp32 values it
stores (acc0 + acc1 rounded to fp32, widened to fp64): test_epilogue_statistics compares with the
fp64 sums of the call's own stored y, bound 1e-10 * sum|y| resp. 1e-10 * sum y^2 (fp64 summation
error over at most 2^20 terms, 2^20 * 2^-53 ~ 1.2e-10; derived, not measured)."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import md2_oracle as O
from tests import _data as D

pytestmark = pytest.mark.gpu

SENT = 7168.5      # finite sentinel, exactly representable
G = 64             # guard floats either side of every destination
TOL = 1e-5

Spec = collections.namedtuple("Spec", "n c0 c1 h w cout k stride pad reflect act bias cin_w shift")


def S(n, c0, c1, h, w, cout, k=3, stride=1, pad=1, reflect=True, act="elu", bias=True, cin_w=0, shift=0):
    return Spec(n, c0, c1, h, w, cout, k, stride, pad, reflect, act, bias, cin_w, shift)


def _plain(n, cin, h, w, cout, **kw):
    """Zero padding, no bias, no activation (the encoder's convs)."""
    return S(n, cin, 0, h, w, cout, **{**dict(reflect=False, act=None, bias=False), **kw})


def _r(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()


def _act(y, act):
    return {None: y, "relu": F.relu(y), "elu": F.elu(y), "sigmoid": torch.sigmoid(y)}[act]


def _conv(x, w, b, sp):
    if sp.reflect:
        return F.conv2d(O.pad_reflect(x, sp.pad), w, b, stride=sp.stride)
    return F.conv2d(x, w, b, stride=sp.stride, padding=sp.pad)


@functools.lru_cache(maxsize=None)
def _ref(sp):
    """The fp64 reference of one spec, computed once and shared (never modified): x [n][cin] (its
    padded channels zero; with `shift` the concat of two overlapping windows of `buf`), w, b, dy,
    y = act(conv), dx (padded rows zero), dw [cout][cin_w], db."""
    g = torch.Generator().manual_seed(11)
    cin = sp.c0 + sp.c1
    cw = sp.cin_w or cin
    buf = None
    if sp.shift:
        assert sp.c0 == sp.c1
        buf = _r(g, sp.n + sp.shift, sp.c0, sp.h, sp.w)
        x = torch.cat([buf[:sp.n], buf[sp.shift:sp.shift + sp.n]], 1)
    else:
        x = _r(g, sp.n, cin, sp.h, sp.w)
        x[:, cw:] = 0
    w = (torch.randn(sp.cout, cw, sp.k, sp.k, generator=g, dtype=torch.float64) / (cw * sp.k * sp.k) ** 0.5).float().double()
    b = _r(g, sp.cout) if sp.bias else None
    xr = x[:, :cw].clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if sp.bias else None
    pre = _conv(xr, wr, br, sp)
    dy = _r(g, *pre.shape)
    pre.backward(dy)
    dx = torch.zeros_like(x)
    dx[:, :cw] = xr.grad
    return dict(x=x, buf=buf, w=w, b=b, dy=dy, y=_act(pre, sp.act).detach(), dx=dx, dw=wr.grad,
                db=br.grad if sp.bias else None)


def _desc(sp):
    from md2hip._lib import ConvDesc
    from md2hip.ops import ACT
    return ConvDesc(n=sp.n, cin=sp.c0 + sp.c1, h=sp.h, w=sp.w, cout=sp.cout, kh=sp.k, kw=sp.k, stride=sp.stride,
                    pad=sp.pad, reflect=int(sp.reflect), act=ACT[sp.act])


def _out_hw(sp):
    return (sp.h + 2 * sp.pad - sp.k) // sp.stride + 1, (sp.w + 2 * sp.pad - sp.k) // sp.stride + 1


def _gpu(t):
    return None if t is None else t.float().cuda().contiguous()


def _inputs(sp, r):
    """Device input tensors and the input fields of md2_conv_operands."""
    if sp.shift:
        buf = _gpu(r["buf"])
        return buf, dict(in1=buf[sp.shift], in_c0=sp.c0)        # contiguous images: default strides
    if sp.c1 == 0:
        return _gpu(r["x"]), {}
    x1 = _gpu(r["x"][:, sp.c0:])
    return _gpu(r["x"][:, :sp.c0]), dict(in1=x1, in_c0=sp.c0)


class Dest:
    """`c` channels per image as the window [off, off + c) of a wider tensor [n][c + extra][hw],
    64 guard floats either side, everything prefilled with the sentinel (then `init` in the window)."""

    def __init__(self, n, c, hw, extra=0, off=0, init=None, dtype=torch.float32):
        cw = c + extra
        self.flat = torch.full((G + n * cw * hw + G,), SENT, dtype=dtype, device="cuda")
        body = self.flat[G:G + n * cw * hw].view(n, cw, hw)
        self.win = body[:, off:off + c]
        self.bs = cw * hw
        if init is not None:
            self.win.copy_(init.reshape(n, c, hw).to(dtype))
        self.mask = torch.ones(self.flat.shape, dtype=torch.bool, device="cuda")
        self.mask[G:G + n * cw * hw].view(n, cw, hw)[:, off:off + c] = False
        self.before = self.flat.clone()

    def untouched(self):
        it = torch.int32 if self.flat.dtype == torch.float32 else torch.int64
        return torch.equal(self.flat.view(it)[self.mask], self.before.view(it)[self.mask])

    def unwritten(self):
        it = torch.int32 if self.flat.dtype == torch.float32 else torch.int64
        return torch.equal(self.flat.view(it), self.before.view(it))

    def get(self):
        torch.cuda.synchronize()
        return self.win.clone()


def _err(got, want, scale=None):
    got, want = got.double().cpu().reshape(-1), want.double().reshape(-1)
    return ((got - want).norm() / max((want if scale is None else scale.double()).norm().item(), 1e-30)).item()


def _init_like(ref, seed):
    """Seeded randn scaled to ref's rms, fp32-representable."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(ref.shape, generator=g, dtype=torch.float64) * (ref.norm() / ref.numel() ** 0.5)).float().double()


WORST = collections.defaultdict(float)


def _check(form, what, e, tol=TOL):
    WORST[form] = max(WORST[form], e)
    print(f"[operands] form {form} {what}: {e:.3e} (worst of form so far {WORST[form]:.3e})")
    assert e < tol, (what, e)


def _twice(fn):
    """fn() -> list of result tensors: run twice on fresh buffers, require the same bits."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "not deterministic"
    return a


# ---- the three passes on sentinel-guarded destinations ----------------------------------------------
def _forward(sp, route, y_extra=4, accumulate=False, seed=0, **fwd_kw):
    from md2hip import ops
    r = _ref(sp)
    ho, wo = _out_hw(sp)
    init = _init_like(r["y"], 100 + seed) if accumulate else None

    def run():
        x0, ikw = _inputs(sp, r)
        dst = Dest(sp.n, sp.cout, ho * wo, extra=y_extra, init=init)
        o = ops.conv_operands(out_bs0=dst.bs, accumulate=accumulate, cin_w=sp.cin_w, **ikw)
        info = ops.conv2d_fwd_ex(_desc(sp), o, x0, _gpu(r["w"]), _gpu(r["b"]), dst.win, **fwd_kw)
        y = dst.get()
        assert info["kernel"] == route, (info["kernel"], route)
        assert dst.untouched(), "forward wrote outside y"
        return [y]
    y, = _twice(run)
    want = r["y"] if init is None else init + r["y"]
    return _err(y, want.reshape(sp.n, sp.cout, -1), r["y"])


def _dgrad(sp, route, split=True, p0_extra=4, p1_extra=16, p1_off=4, accumulate=False, seed=0):
    """dX of the spec's conv; split: rows [0, c0) to p0, the rest into a window of a wider tensor."""
    from md2hip import ops
    r = _ref(sp)
    cin, hw = sp.c0 + sp.c1, sp.h * sp.w
    c0 = sp.c0 if split and sp.c1 else cin
    ref0, ref1 = r["dx"][:, :c0], r["dx"][:, c0:]
    i0 = _init_like(ref0, 200 + seed) if accumulate else None
    i1 = _init_like(ref1, 300 + seed) if accumulate and c0 < cin else None

    def run():
        d0 = Dest(sp.n, c0, hw, extra=p0_extra, init=i0)
        kw = dict(out_bs0=d0.bs, accumulate=accumulate, cin_w=sp.cin_w)
        d1 = None
        if c0 < cin:
            d1 = Dest(sp.n, cin - c0, hw, extra=p1_extra, off=p1_off, init=i1)
            kw.update(out1=d1.win, out_c0=c0, out_bs1=d1.bs)
        info = ops.conv2d_dgrad_ex(_desc(sp), ops.conv_operands(**kw), _gpu(r["dy"]), _gpu(r["w"]), d0.win)
        out = [d0.get()] + ([d1.get()] if d1 else [])
        assert info["kernel"] == route, (info["kernel"], route)
        assert d0.untouched() and (d1 is None or d1.untouched()), "dgrad wrote outside dx"
        return out
    got = _twice(run)
    errs = [_err(got[0], ref0 if i0 is None else i0 + ref0, ref0)]
    if c0 < cin:
        errs.append(_err(got[1], ref1 if i1 is None else i1 + ref1, ref1))
    return errs, got


def _wgrad(sp, route, accumulate=False, seed=0, db_part=None):
    from md2hip import ops
    r = _ref(sp)
    idw = _init_like(r["dw"], 400 + seed) if accumulate else None
    idb = _init_like(r["db"], 500 + seed) if accumulate and sp.bias else None

    def run():
        x0, ikw = _inputs(sp, r)
        dw = Dest(1, r["dw"].numel(), 1, init=idw)
        db = Dest(1, sp.cout, 1, init=idb) if sp.bias else None
        o = ops.conv_operands(accumulate=accumulate, cin_w=sp.cin_w, **ikw)
        info = ops.conv2d_wgrad_ex(_desc(sp), o, x0, _gpu(r["dy"]), dw.win, db.win if db else None, db_part=db_part)
        out = [dw.get()] + ([db.get()] if db else [])
        assert info["kernel"] == route, (info["kernel"], route)
        assert dw.untouched() and (db is None or db.untouched()), "wgrad wrote outside dw / db"
        return out
    got = _twice(run)
    errs = [_err(got[0], r["dw"] if idw is None else idw + r["dw"], r["dw"])]
    if sp.bias:
        errs.append(_err(got[1], r["db"] if idb is None else idb + r["db"], r["db"]))
    return errs, got


# ---- a. concat input: forward and filter gradient ---------------------------------------------------
POSE = dict(reflect=False, act="relu")
CONCAT = {
    # the decoder's four (up || skip) pairs on small maps, reflect + ELU + bias
    "32+64-32": (S(2, 32, 64, 6, 10, 32), "px3", "wgrad16"),
    # (the flattened halo image holds 256 pixels of rows W + 16 wide: it takes W >= 11, so 6 x 12
    # maps, and the 2 x 4 maps of the 64 x 128 parity geometry run conv_px3)
    "64+64-64": (S(2, 64, 64, 6, 12, 64), "halo", "wgrad_px3:64x192c64"),
    "128+128-128": (S(2, 128, 128, 6, 12, 128), "halo", "wgrad_px3:64x128c128"),
    "256+256-256@2x4": (S(2, 256, 256, 2, 4, 256), "px3", "wgrad_px3:64x128c128"),
    "256+256-256@4x13": (S(2, 256, 256, 4, 13, 256), "halo", "wgrad_px3:64x128c128"),
    # a split that is a multiple of 16 but not of 32 (16-channel tap blocks), and of 32 but not 64
    "16+32-64": (S(2, 16, 32, 6, 12, 64), "halo", "wgrad_tile:64x128c16"),
    "32+64-64": (S(2, 32, 64, 6, 12, 64), "halo", "wgrad_px3:64x128c32"),
    "16+16-16": (S(2, 16, 16, 6, 10, 16), "px16", "wgrad16"),
    # 32-row tiles of the 2D halo kernel (tiles at least half full: 8 x 200 in 8 x 32 tiles)
    "32+64-32 wide": (S(1, 32, 64, 8, 200, 32), "halo2d", "wgrad16"),
    # ragged: Cout 20, odd H and W
    "16+32-20 ragged": (S(2, 16, 32, 5, 7, 20), "px3", "wgrad16"),
    # pose conv1: two overlapping windows of the squeezer output, the second N images (resp. one
    # image) further into the same buffer; zero padding, so only the split keeps it off conv_whalo
    "pose 256+256 shift N": (S(4, 256, 256, 4, 13, 256, shift=2, **POSE), "halo", "wgrad_px3:64x128c128"),
    "pose 256+256 shift 1": (S(4, 256, 256, 4, 13, 256, shift=1, **POSE), "halo", "wgrad_px3:64x128c128"),
    "pose 512 one tensor": (S(4, 512, 0, 4, 13, 256, **POSE), "halo", "whalo"),
}


@pytest.mark.parametrize("name", list(CONCAT))
def test_concat(name):
    sp, fwd_route, wgrad_route = CONCAT[name]
    _check("a", f"{name} fwd y", _forward(sp, fwd_route))
    errs, _ = _wgrad(sp, wgrad_route)
    for what, e in zip(("dw", "db"), errs):
        _check("a", f"{name} wgrad {what}", e)


# ---- b. split / strided / accumulating output -------------------------------------------------------
SPLIT_DGRAD = {
    "32+64-32": (S(2, 32, 64, 6, 10, 32), "px3", {}),
    "64+64-64": (S(2, 64, 64, 6, 10, 64), "halo_rfl_dgrad", {}),
    "128+128-128": (S(2, 128, 128, 6, 10, 128), "halo_rfl_dgrad", {}),
    "256+256-256@2x4": (S(2, 256, 256, 2, 4, 256), "px3", {}),     # padded grid 4 x 6: too narrow for the halo
    "256+256-256@4x13": (S(2, 256, 256, 4, 13, 256), "halo_rfl_dgrad", {}),
    # the MPI d_emb layout: p1 at channel 0 of a buffer whose image stride carries 16 more channels
    "64+64-64 mpi stride": (S(2, 64, 64, 6, 10, 64), "halo_rfl_dgrad", dict(p0_extra=0, p1_extra=16, p1_off=0)),
}


@pytest.mark.parametrize("name", list(SPLIT_DGRAD))
def test_split_dgrad(name):
    sp, route, kw = SPLIT_DGRAD[name]
    errs, _ = _dgrad(sp, route, **kw)
    for part, e in zip(("p0 rows", "p1 rows"), errs):
        _check("b", f"{name} dgrad {part}", e)


ACC_DGRAD = {
    "512-256@2x4 split-K": (S(2, 512, 0, 2, 4, 256), "px3"),                  # 8 K splits, reduced into dx +=
    "512-256@4x13 split-K": (S(2, 512, 0, 4, 13, 256), "halo_rfl_dgrad"),     # channel splits summed by the fold
    "64-32": (S(2, 64, 0, 6, 10, 32), "halo_rfl_dgrad"),                      # 2 chunks: no split
    "64-128/2": (_plain(2, 64, 8, 24, 128, stride=2), "halo_s2"),             # dY rows of 12 (>= 12: its halo image)
    "16-16": (S(2, 16, 0, 6, 10, 16), "px"),                                  # Cin 16: the 32-row tile
    "64+64-64 split": (S(2, 64, 64, 6, 10, 64), "halo_rfl_dgrad"),            # both parts accumulate
    "head 64-1@4x13": (S(2, 64, 0, 4, 13, 1, act="sigmoid"), "head_fallback"),  # odd W (head2), strided dx +=
    "64-128/2@7x9": (_plain(2, 64, 7, 9, 128, stride=2), "px3"),              # four class launches, each dx +=
}


@pytest.mark.parametrize("name", list(ACC_DGRAD))
def test_accumulate_dgrad(name):
    sp, route = ACC_DGRAD[name]
    errs, _ = _dgrad(sp, route, accumulate=True)
    for part, e in zip(("p0 rows", "p1 rows"), errs):
        _check("b", f"{name} dgrad += {part}", e)


# the stride-2 data gradient off the stride-2 halo kernel: one dense GEMM per output-parity class
S2_DGRAD = {
    "1x1/2 64-128@8x12": (_plain(2, 64, 8, 12, 128, k=1, stride=2, pad=0), "px3"),   # merged classes, one tap
    "3x3/2 48-96@8x12": (_plain(2, 48, 8, 12, 96, stride=2), "px3"),     # Cin % 64 != 0; merged, taps 1/2/2/4
    "3x3/2 64-128@7x9": (_plain(2, 64, 7, 9, 128, stride=2), "px3"),     # odd H, W: four launches, unequal extents
    "3x3/2 32-64@8x12": (_plain(2, 32, 8, 12, 64, stride=2), "px"),      # Cin <= 32: the 32-row tile
}


@pytest.mark.parametrize("name", list(S2_DGRAD))
def test_stride2_dgrad(name):
    sp, route = S2_DGRAD[name]
    errs, _ = _dgrad(sp, route)
    _check("b", f"{name} dgrad", errs[0])


def test_head_then_c1_dgrad():
    """The model's order: a head's data gradient stores d_o2, the next branch's c1 data gradient
    adds to it in the same (strided) buffer."""
    from md2hip import ops
    head = S(2, 64, 0, 8, 16, 1, act="sigmoid")
    c1 = S(2, 64, 0, 8, 16, 32)
    rh, rc = _ref(head), _ref(c1)
    hw = 8 * 16

    def run():
        d = Dest(2, 64, hw, extra=4)
        o = ops.conv_operands(out_bs0=d.bs)
        k1 = ops.conv2d_dgrad_ex(_desc(head), o, _gpu(rh["dy"]), _gpu(rh["w"]), d.win)["kernel"]
        first = d.get()
        o = ops.conv_operands(out_bs0=d.bs, accumulate=True)
        k2 = ops.conv2d_dgrad_ex(_desc(c1), o, _gpu(rc["dy"]), _gpu(rc["w"]), d.win)["kernel"]
        both = d.get()
        assert (k1, k2) == ("head_batched", "halo_rfl_dgrad"), (k1, k2)
        assert d.untouched()
        return [first, both]
    first, both = _twice(run)
    _check("b", "head dgrad", _err(first, rh["dx"].reshape(2, 64, -1)))
    want = first.double().cpu() + rc["dx"].reshape(2, 64, -1)        # the stored head gradient is the init
    _check("b", "head dgrad then c1 dgrad +=", _err(both, want, rc["dx"]))


ACC_WGRAD = {
    "64+64-64": (S(2, 64, 64, 6, 10, 64), "wgrad_px3:64x192c64"),             # one split
    "pose 512 one tensor": (S(4, 512, 0, 4, 13, 256, **POSE), "whalo"),       # split-K over row chunks
    "64+64-64@16x16 split-K": (S(2, 64, 64, 16, 16, 64), "wgrad_px3:64x192c64"),
}


@pytest.mark.parametrize("name", list(ACC_WGRAD))
def test_accumulate_wgrad(name):
    sp, route = ACC_WGRAD[name]
    errs, _ = _wgrad(sp, route, accumulate=True)
    for what, e in zip(("dw", "db"), errs):
        _check("b", f"{name} wgrad += {what}", e)


# ---- c. zero-padded input channels (MPI mode: E = 21 embedding channels in Ep = 32) -----------------
CIN_W = {
    # Cin = co + featC + 32 = 96 with cin_w = Cin - 11; the LDS-halo kernels refuse cin_w
    "3x3 concat": (S(2, 32, 64, 6, 10, 64, cin_w=85), "px3", "px3", "wgrad_px3:64x128c32"),
    "3x3": (S(2, 96, 0, 6, 10, 64, cin_w=85), "px3", "px3", "wgrad_px3:64x128c32"),
    "1x1": (S(2, 96, 0, 6, 10, 64, k=1, pad=0, reflect=False, cin_w=85), "px3", "px3", "wgrad_px3:64x128c32"),
}


@pytest.mark.parametrize("name", list(CIN_W))
def test_cin_w(name):
    sp, fr, dr, wr = CIN_W[name]
    _check("c", f"{name} fwd y", _forward(sp, fr))
    errs, got = _dgrad(sp, dr, p1_extra=16, p1_off=0)
    for part, e in zip(("p0 rows", "p1 rows"), errs):
        _check("c", f"{name} dgrad {part}", e)
    dx = torch.cat(got, 1)
    assert dx.shape[1] == 96 and (dx[:, sp.cin_w:] == 0).all(), "padded rows of dx must be exactly zero"
    errs, got = _wgrad(sp, wr)                   # dw holds cout * cin_w * k * k floats between its guards
    assert got[0].numel() == sp.cout * sp.cin_w * sp.k * sp.k
    for what, e in zip(("dw", "db"), errs):
        _check("c", f"{name} wgrad {what}", e)


# ---- d. frame-major stem input ----------------------------------------------------------------------
STEM = {
    "3x32x64": ((2, 32, 64), "stem_s2d", "stem_wgrad_s2d"),
    "3x4x96": ((2, 4, 96), "stem_s2d", "stem_wgrad_s2d"),
    "3x18x44": ((2, 18, 44), "px", "stem_wgrad"),              # Wo % 16 != 0: the generic kernels
}


@pytest.mark.parametrize("name", list(STEM))
def test_stem_frame_major(name):
    """x[n][3 frames][c][h][w] read as 3n images in frame-major order (image b = l * n + i is
    x[i][l]: in_bdiv = n, in_bs0 = the sample stride, in_bhi = the frame stride)."""
    from md2hip import ops
    (n, h, w), fwd_route, wgrad_route = STEM[name]
    g = torch.Generator().manual_seed(13)
    x = _r(g, n, 3, 3, h, w)
    sp = _plain(3 * n, 3, h, w, 64, k=7, stride=2, pad=3)
    wt = (torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64) / 147 ** 0.5).float().double().requires_grad_(True)
    pre = F.conv2d(x.transpose(0, 1).reshape(3 * n, 3, h, w), wt, stride=2, padding=3)
    dy = _r(g, *pre.shape)
    pre.backward(dy)
    ho, wo = pre.shape[2:]
    fs = 3 * h * w
    ikw = dict(in_bdiv=n, in_bs0=3 * fs, in_bhi=fs)

    def run():
        xg = _gpu(x)
        y = Dest(3 * n, 64, ho * wo, extra=4)
        kf = ops.conv2d_fwd_ex(_desc(sp), ops.conv_operands(out_bs0=y.bs, **ikw), xg, _gpu(wt.detach()), None,
                               y.win)["kernel"]
        dw = Dest(1, 64 * 147, 1)
        kw = ops.conv2d_wgrad_ex(_desc(sp), ops.conv_operands(**ikw), xg, _gpu(dy), dw.win)["kernel"]
        out = [y.get(), dw.get()]
        assert (kf, kw) == (fwd_route, wgrad_route), (kf, kw)
        assert y.untouched() and dw.untouched()
        return out
    y, dw = _twice(run)
    _check("d", f"{name} fwd y", _err(y, pre.detach().reshape(3 * n, 64, -1)))
    _check("d", f"{name} wgrad dw", _err(dw, wt.grad))


# ---- e. deferred split-K, statistics from the halo epilogue -----------------------------------------
DEFER = {
    "fwd 256-512/2@4x8": ("fwd", _plain(6, 256, 4, 8, 512, stride=2), "px3"),
    "fwd 512-512@2x4": ("fwd", _plain(6, 512, 2, 4, 512), "px3"),
    "dgrad 512-512@2x4": ("dgrad", _plain(6, 512, 2, 4, 512), "px3"),
    "fwd 512-512@4x13": ("fwd", _plain(2, 512, 4, 13, 512), "halo"),
    "dgrad 512-512@4x13": ("dgrad", _plain(2, 512, 4, 13, 512), "halo"),
}


def _call_plain(kind, sp, r, dst, **kw):
    from md2hip import ops
    o = ops.conv_operands(out_bs0=dst.bs)
    if kind == "fwd":
        return ops.conv2d_fwd_ex(_desc(sp), o, _gpu(r["x"]), _gpu(r["w"]), _gpu(r["b"]), dst.win, **kw)
    return ops.conv2d_dgrad_ex(_desc(sp), o, _gpu(r["dy"]), _gpu(r["w"]), dst.win, **kw)


@pytest.mark.parametrize("name", list(DEFER))
def test_deferred_splitk(name):
    """A deferred launch leaves [splits][rows][n * pixels] slabs and does not write the output;
    their fp32 sum in split order is bit-equal to what the same call stores when it reduces."""
    kind, sp, route = DEFER[name]
    r = _ref(sp)
    ho, wo = _out_hw(sp)
    rows, pix = (sp.cout, ho * wo) if kind == "fwd" else (sp.c0, sp.h * sp.w)
    ref = (r["y"] if kind == "fwd" else r["dx"]).reshape(sp.n, rows, pix)

    def run():
        dst = Dest(sp.n, rows, pix)                       # contiguous: the deferral needs a plain output
        info = _call_plain(kind, sp, r, dst, defer=True)
        torch.cuda.synchronize()
        assert info["kernel"] == route, info["kernel"]
        assert info["splits"] > 1, "the shape no longer splits: pick another"
        assert dst.unwritten(), "a deferred launch must not write the output"
        acc = torch.zeros(rows, sp.n * pix, device="cuda")
        for k in range(info["splits"]):
            acc = acc + info["slab"][k]
        return [acc.view(rows, sp.n, pix).transpose(0, 1).contiguous()]
    summed, = _twice(run)
    dst = Dest(sp.n, rows, pix)
    info = _call_plain(kind, sp, r, dst)
    y = dst.get()
    assert info["kernel"] == route and info["splits"] == 0 and dst.untouched()
    assert torch.equal(summed.view(torch.int32), y.view(torch.int32)), "slab sum != reduced output"
    _check("e", f"{name} slab sum", _err(summed, ref))


@pytest.mark.parametrize("why", ["bias", "act", "accumulate", "split output"])
def test_deferral_declined(why):
    """A request on an output the caller could not rebuild from the slabs alone is declined:
    splits == 0 and the output is complete."""
    from md2hip import ops
    base = dict(reflect=False, act=None, bias=False)
    base.update({"bias": dict(bias=True), "act": dict(act="relu")}.get(why, {}))
    sp = S(2, 512, 0, 4, 13, 512, **base)
    r = _ref(sp)
    acc = why == "accumulate"
    init = _init_like(r["y"], 7) if acc else None
    c0 = 256 if why == "split output" else 512
    d0 = Dest(2, c0, 52, init=None if init is None else init[:, :c0])
    kw = dict(out_bs0=d0.bs, accumulate=acc)
    d1 = None
    if c0 < 512:
        d1 = Dest(2, 512 - c0, 52, extra=16, off=4)
        kw.update(out1=d1.win, out_c0=c0, out_bs1=d1.bs)
    info = ops.conv2d_fwd_ex(_desc(sp), ops.conv_operands(**kw), _gpu(r["x"]), _gpu(r["w"]), _gpu(r["b"]), d0.win,
                             defer=True)
    y = torch.cat([d0.get()] + ([d1.get()] if d1 else []), 1)
    assert info["kernel"] == "halo" and info["splits"] == 0 and info["slab"] is None
    assert d0.untouched() and (d1 is None or d1.untouched())
    want = r["y"] if init is None else init + r["y"]
    for part, sl in (("p0 rows", slice(0, c0)), ("p1 rows", slice(c0, 512))):
        if sl.start < sl.stop:
            _check("e", f"declined ({why}) {part}", _err(y[:, sl], want[:, sl].reshape(2, sl.stop - sl.start, -1),
                                                         r["y"][:, sl]))


STATS = {
    # (W >= 11 for the flattened halo image: the narrowest maps that reach the kernel)
    "ragged": _plain(3, 32, 5, 11, 64),       # 165 pixels: one ragged tile
    "small images": _plain(14, 32, 2, 11, 64),    # 308 pixels: a full tile over 11.6 two-row images + a ragged one
    "M=128": _plain(2, 32, 13, 20, 128),      # two 64-row tiles, 3 pixel tiles
}


@pytest.mark.parametrize("name", list(STATS))
def test_epilogue_statistics(name):
    """[cout][parts][2] fp64 partials of the stored fp32 y (see the module docstring), reduced over
    parts, against the fp64 sums of the call's own y."""
    from md2hip import ops
    sp = STATS[name]
    r = _ref(sp)
    pix = sp.h * sp.w
    parts = -(-sp.n * pix // 256)

    def run():
        y = Dest(sp.n, sp.cout, pix)
        st = Dest(1, sp.cout * parts * 2, 1, dtype=torch.float64)
        info = ops.conv2d_fwd_ex(_desc(sp), ops.conv_operands(), _gpu(r["x"]), _gpu(r["w"]), None, y.win, stats=st.win)
        out = [y.get(), st.get()]
        assert info["kernel"] == "halo" and info["splits"] == 0
        assert info["stats_parts"] == parts, (info["stats_parts"], parts)
        assert y.untouched() and st.untouched()
        return out
    a, b = run(), run()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int64),
                                                                                    b[1].view(torch.int64))
    y, st = a[0].double().cpu(), a[1].cpu().view(sp.cout, parts, 2).sum(1)
    _check("e", f"stats {name} y", _err(y, r["y"].reshape(sp.n, sp.cout, -1)))
    s1, s2, sa = y.sum((0, 2)), (y * y).sum((0, 2)), y.abs().sum((0, 2))
    d1, d2 = ((st[:, 0] - s1).abs() / sa).max().item(), ((st[:, 1] - s2).abs() / s2).max().item()
    print(f"[operands] form e stats {name}: sum {d1:.3e}, sum of squares {d2:.3e} (bound 1e-10)")
    assert d1 <= 1e-10 and d2 <= 1e-10, (d1, d2)


# ---- f. bias partials -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _act_ref(act, n, c, h, w):
    g = torch.Generator().manual_seed(17)
    pre = _r(g, n, c, h, w).requires_grad_(True)
    out = _act(pre, act)
    out32 = out.detach().float().double()       # the stored activation the kernels see
    dout = _r(g, n, c, h, w)
    # the gradient as the kernels define it, from the stored post-activation output, in fp64
    dpre = {"relu": torch.where(out32 > 0, dout, torch.zeros_like(dout)),
            "elu": torch.where(out32 > 0, dout, dout * (out32 + 1)),
            "sigmoid": dout * out32 * (1 - out32)}[act]
    return out32, dout, dpre


@pytest.mark.parametrize("shape", [(2, 20, 6, 10), (2, 20, 32, 64)], ids=["1 part", "2 parts"])
@pytest.mark.parametrize("act", ["elu", "relu", "sigmoid"])
def test_act_backward_bias(act, shape):
    from md2hip import ops
    out, dout, dpre = _act_ref(act, *shape)
    og, dg = _gpu(out), _gpu(dout)
    got, part = ops.act_backward_bias(og, dg, act)
    again, part2 = ops.act_backward_bias(og, dg, act)
    plain = ops.act_backward(og, dg, act)
    torch.cuda.synchronize()
    assert part.shape[1] == (1 if shape[2] == 6 else 2), part.shape
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), "dpre differs from act_backward"
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(part.view(torch.int32),
                                                                                       part2.view(torch.int32))
    _check("f", f"{act} {shape} dpre", _err(got, dpre))
    _check("f", f"{act} {shape} sum of parts", _err(part.double().sum(1), dpre.sum((0, 2, 3))))


def test_bias_partials_into_wgrad():
    """db from act_backward_bias partials (db_part) = db from the pass over dy, both within 1e-5 of fp64."""
    from md2hip import ops
    sp = S(2, 16, 32, 6, 10, 20)
    r = _ref(sp)
    # the partials of this conv's own dy (act none: dpre = dy, bit for bit)
    dy = _gpu(r["dy"])
    dpre, part = ops.act_backward_bias(dy, dy, None)
    torch.cuda.synchronize()
    assert torch.equal(dpre.view(torch.int32), dy.view(torch.int32))
    errs_p, got_p = _wgrad(sp, "wgrad16", db_part=part)
    errs, got = _wgrad(sp, "wgrad16")
    _check("f", "db from db_part", errs_p[1])
    _check("f", "db from dy", errs[1])
    _check("f", "db_part vs plain", _err(got_p[1], got[1].double().cpu()))
    assert torch.equal(got_p[0].view(torch.int32), got[0].view(torch.int32)), "dw must not depend on db_part"


# ---- forms the head kernels do not implement go to the generic kernels ------------------------------
def test_head_shape_with_concat_or_split_runs_the_generic_kernels():
    """The Cout = 1 head kernels read and write p0 only (conv_head_in): a head shape with a concat
    input or a split dX must leave the head path, not drop the second tensor."""
    sp = S(2, 16, 16, 6, 10, 1, act="sigmoid")
    _check("a", "head shape, concat input: fwd y", _forward(sp, "px"))
    errs, _ = _wgrad(sp, "wgrad16")
    for what, e in zip(("dw", "db"), errs):
        _check("a", f"head shape, concat input: wgrad {what}", e)
    errs, _ = _dgrad(sp, "px")
    for part, e in zip(("p0 rows", "p1 rows"), errs):
        _check("b", f"head shape, split dx: dgrad {part}", e)
