"""The BatchNorm kernels (csrc/bn_fwd.hip, csrc/bn_bwd.hip) in the operand forms the train step
feeds them (md2_bn_forward_ex / md2_bn_backward_ex), each against the fp64 reference of
tests/_bn_ref.py, in-process: the route is an argument of the calls.

Every case asserts
  (a) the values, per channel (one wrong plane, owner store or LDS slot cannot dilute into a tensor
      norm): out / dy / dres as max|got-ref| / max|ref| over the channel, dgamma as |err| / sum|g*xhat|,
      dbeta as |err| / sum|g|, mean / invstd / running statistics as relative errors.  The backward
      reference takes its statistics from y in fp64, never the kernel's mean / invstd; its ReLU gate
      is data (the kernel forward's out > 0), so no near-zero pre-activation is excluded.
      Bound: max(1e-6, 8 * floor), floor = the worst channel of the same quantity evaluated on the
      CPU in fp32 with fp64 sums (_bn_ref.*_f32) against fp64; channels with |mean|/std <= 4 must
      also stay under 1e-5.  Floor and measured error are printed per case and quantity;
  (b) sentinels: every output sits between 64 guard elements that must be bit-identical afterwards,
      and outputs a form must not write (dout_w of the one-kernel slab backward) stay untouched;
  (c) determinism: a second call on fresh buffers gives the same bits;
  (d) the info record: family, partials and units per thread the case is listed for (SHAPES).

Bitwise claims of the kernels' comments, each within one route: slab forms == the call on the
host's fp32 presum (split order from 0.0f) and y_out / dout_w == that sum; the skip addend == dout
with the range pre-added; the mbeta re-derivation == the forward's out as mask (gamma < 0 and
gamma = 0 included); bn_relu_maxpool == bn_apply_fused + md2_maxpool3s2_fwd (ties included);
collapsed == uncollapsed caller partials.  One kernel against two passes: mean / invstd within one
fp32 ulp, the rest under the bound of (a).

The floor functions use the kernels' algebraic form (scale / shift: y*sc + sh with sc = gamma*invstd,
sh = beta - mean*sc; xhat = (y - mean)*invstd) without fused multiply-adds, so the floor carries the
same conditioning as any correct fp32 kernel: the rounding of mean and of sh, times invstd.

Worst per-channel error measured on an MI355X, with the floor of that case in brackets (the bound
is max(1e-6, 8 * floor)); the file's 176 tests take about 6 s:
  forward, all forms        out 1.7e-6 [1.6e-6] (7x259x1x3 relu: 21 values per channel), mean 5.8e-8 [5.8e-8],
                            invstd 5.6e-8 [5.6e-8], run_mean 8.1e-7 [8.1e-7], run_var 1.2e-7 [1.2e-7]
  forward, variance 0       out 1.2e-5 [3.9e-6] plain, 3.2e-5 [5.9e-5] y2_relu (1x2x1x1: y*sc and sh cancel to beta)
  forward, |mean|/std 500   out 6.0e-6 [1.3e-5] plain / relu, 5.5e-6 [1.1e-5] res_relu, 1.2e-5 [2.1e-5] y2_relu
  caller partials           out 9.8e-8 [9.8e-8], run_mean 9.1e-8 [9.1e-8]; collapsed == uncollapsed bitwise
  backward, all forms       dy 5.3e-7 [5.3e-7] (mbeta), dgamma 5.4e-7 [5.4e-7], dbeta 5.5e-8 [5.5e-8],
                            dres 5.9e-8 [5.9e-8]
  backward, |mean|/std 500  dy 5.7e-7 [5.7e-7], dgamma 1.2e-6 [1.2e-6], dbeta 3.3e-9 [3.3e-9]
  UPT 2 / 4 / 8 shapes      out 2.2e-7 [2.9e-7], dy 2.0e-7 [2.0e-7], dgamma 2.4e-8, dbeta 4.9e-9, dres 5.9e-8
  stem tail with the pool   out 5.7e-6 [5.7e-6] (1x2x2x2 quantised: 4 values per channel), else <= 1.4e-7
"""
import collections
import functools

import numpy as np
import pytest
import torch

from tests import _bn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7168.5      # finite sentinel, exactly representable
G = 64             # guard elements either side of every output
EPS = float(np.float32(1e-5))
MOM = 0.1

E = collections.namedtuple("E", "vec fits parts upt what")
# shape -> what the info record must report: float4 units, one-kernel eligible, bn_parts, and the
# units per thread of the two-pass apply (forward and backward pick it with the same bn_upt)
SHAPES = {
    (1, 2, 1, 1): E(0, 0, 1, 1, "one value per channel: variance 0, max(total-1, 1), scalar units"),
    (2, 3, 1, 4): E(1, 1, 1, 1, "smallest float4 case, U = 1"),
    (6, 5, 2, 3): E(0, 0, 1, 1, "scalar units; layer 4 at 64x96"),
    (7, 259, 1, 3): E(0, 0, 1, 1, "scalar units, planes straddle blocks, c wraps mid-block"),
    (3, 300, 2, 2): E(1, 1, 1, 1, "U = 1: 256 planes per block (full LDS tables), C does not divide 256"),
    (5, 4, 6, 10): E(1, 1, 1, 1, "fits with 75 units: most waves idle"),
    (3, 2, 40, 48): E(1, 1, 3, 1, "1440 units: the second register unit partly live"),
    (8, 3, 32, 32): E(1, 1, 5, 1, "exactly 2048 units: the last shape that fits"),
    (8, 3, 4, 260): E(1, 0, 5, 1, "2080 units: must not fit"),
    (6, 64, 16, 32): E(1, 1, 2, 1, "the model's layer 1 at 64x128"),
    (80, 3, 32, 64): E(1, 0, 80, 1, "80 partials: the 64-lane partial loop takes a second trip"),
    (6, 5, 24, 40): E(1, 1, 3, 1, "caller partials per 256-value tile, 23 tiles"),
    (4, 3, 96, 100): E(1, 0, 4, 1, "caller partials per 256-value tile, 150 tiles"),
    (3, 37, 100, 190): E(1, 0, 3, 2, "UPT 2; U = 4750: planes straddle blocks"),
    (3, 37, 200, 190): E(1, 0, 3, 4, "UPT 4"),
    (3, 37, 200, 380): E(1, 0, 3, 8, "UPT 8; 8.4M floats"),
    (64, 2051, 4, 4): E(1, 1, 1, 2, "U = 4, large: UPT 2 (here the block-count rule already stops at 2)"),
    # twice the images let UPT 4 pass the block-count rule, so that only the LDS-table clamp
    # (256*4/U + 2 > 256) brings it to 2
    (128, 2051, 4, 4): E(1, 1, 1, 2, "U = 4, large: bn_upt clamps UPT to 2 to keep a block's planes in the tables"),
}
BIG = [(3, 37, 100, 190), (3, 37, 200, 190), (3, 37, 200, 380), (64, 2051, 4, 4), (128, 2051, 4, 4)]
SMALL = [s for s in SHAPES if s not in BIG]
ILL = (5, 4, 6, 10)          # the deliberately ill-conditioned case runs at this shape: mean 50, std 0.1

FWD_FORMS = {          # form -> (relu, res, y2, running statistics)
    "plain": (0, 0, 0, 1),
    "relu": (1, 0, 0, 0),
    "res_relu": (1, 1, 0, 1),
    "y2_relu": (1, 0, 1, 0),
}
# backward form -> the forward form whose out / mean / invstd it follows
BWD_FORMS = {"plain": "plain", "mbeta": "relu", "mbeta_slabs": "relu", "mask_dres_skip": "res_relu",
             "mask_dres_acc": "res_relu"}


def _ops():
    from md2hip import ops
    return ops


def _routes(shape):
    """(route argument, family the info record must name): 0 = the executor's choice."""
    e = SHAPES[shape]
    r = [(1, "two_pass"), (0, "one_kernel" if e.fits else "two_pass")]
    if e.fits:
        r.append((2, "one_kernel"))
    return r


def _families(shape):
    return ["two_pass", "one_kernel"] if SHAPES[shape].fits else ["two_pass"]


ROUTE_OF = {"two_pass": 1, "one_kernel": 2}


# ---- inputs (CPU, fp32), shared and never modified ---------------------------------------------------
@functools.lru_cache(maxsize=6)
def _case(shape, ill=False):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 + n * 7 + c * 13 + h * 17 + w)
    ch = torch.arange(c)
    if ill:
        std = torch.full((c,), 0.1)
        mean = torch.where(ch % 2 == 0, 50.0, -50.0)
    else:                # std from 0.1 to 30, mean up to +-4 std: a channel-indexing error is large
        std = 0.1 * 300.0 ** ((ch % 7).double() / 6.0)
        mean = std * ((ch % 5).double() - 2.0) * 2.0
    std, mean = std.float(), mean.float()

    def rn(*s):
        return torch.randn(*s, generator=g)

    def bc(v):
        return v.view(1, c, 1, 1)

    d = {"shape": shape, "ill": ill}
    d["y"] = bc(mean) + bc(std) * rn(*shape)
    d["y2"] = bc(mean.flip(0)) + bc(std.flip(0)) * rn(*shape)
    d["res"] = rn(*shape) * 0.7
    sign = torch.where(ch % 3 == 1, -1.0, 1.0)
    d["gamma"] = (sign * (0.5 + rn(c).abs())).float()
    d["beta"] = (0.3 * rn(c)).float()
    d["gamma2"] = (0.5 + rn(c).abs()).float()
    d["beta2"] = (0.3 * rn(c)).float()
    d["rm0"] = 0.7 * mean + 0.05
    d["rv0"] = 1.3 * std * std
    d["dout"] = rn(*shape) * bc(0.5 + (ch % 4).float())
    d["skip"] = rn(*shape)
    d["dres0"] = rn(*shape)
    return d


def _fwd_operands(d, form):
    relu, res, y2, run = FWD_FORMS[form]
    kw = dict(gamma=d["gamma"], beta=d["beta"], relu=bool(relu))
    if res:
        kw["res"] = d["res"]
    if y2:
        kw.update(y2=d["y2"], gamma2=d["gamma2"], beta2=d["beta2"])
    return kw, bool(run)


# ---- guarded device buffers --------------------------------------------------------------------------
class Guarded:
    """An output tensor between G guard elements either side, all prefilled with the sentinel."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        numel = int(np.prod(shape))
        fill = SENT if dtype == torch.float32 else 0xA5
        self.buf = torch.full((numel + 2 * G,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[G:G + numel].view(*shape)
        if init is not None:
            self.t.copy_(init)
        self.fill = fill

    def intact(self):
        return bool((self.buf[:G] == self.fill).all()) and bool((self.buf[-G:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())

    def cpu(self):
        return self.t.cpu()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _assert_same(ra, rb, keys, what):
    for k in keys:
        assert _same_bits(ra[k], rb[k]), (what, k)


def run_forward(shape, route, gamma, beta, y=None, slab=None, part=None, collapse=False, y2=None, gamma2=None,
                beta2=None, res=None, relu=False, run=None, pool=False):
    """One md2_bn_forward_ex call on fresh guarded outputs; returns CPU copies, the info record and
    checks the guards.  `run`: (run_mean0, run_var0) or None."""
    ops = _ops()
    n, c, h, w = shape
    d = ops.bn_desc(shape, eps=EPS, momentum=MOM, route=route, collapse=collapse)
    o = {"out": Guarded(shape), "mean": Guarded((c,)), "invstd": Guarded((c,))}
    kw = {}
    if slab is not None:
        o["y_out"] = Guarded(shape)
        kw.update(slab=_dev(slab), y_out=o["y_out"].t)
    else:
        kw["y"] = _dev(y)
    if y2 is not None:
        o["mean2"], o["invstd2"] = Guarded((c,)), Guarded((c,))
        kw.update(y2=_dev(y2), gamma2=_dev(gamma2), beta2=_dev(beta2), mean2=o["mean2"].t, invstd2=o["invstd2"].t)
    if run is not None:
        o["run_mean"], o["run_var"] = Guarded((c,), init=run[0]), Guarded((c,), init=run[1])
        kw.update(run_mean=o["run_mean"].t, run_var=o["run_var"].t)
    if pool:
        o["pool_y"] = Guarded((n, c, h // 2, w // 2))
        o["pool_arg"] = Guarded((n, c, h // 2, w // 2), dtype=torch.uint8)
        kw.update(pool_y=o["pool_y"].t, pool_arg=o["pool_arg"].t)
    info = ops.bn_forward_ex(d, o["out"].t, _dev(gamma), _dev(beta), o["mean"].t, o["invstd"].t, part=_dev(part),
                             res=_dev(res), relu=relu, **kw)
    torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact(), ("guard elements of %s were written" % k, shape, route)
    r = {k: b.cpu() for k, b in o.items()}
    r["info"] = info
    r["dev"] = o
    return r


def run_backward(shape, route, y, mean, invstd, gamma, dout=None, slab=None, mask=None, mbeta=None, dres=None,
                 dres_acc=False, skip=None, skip_lo=0, skip_hi=0):
    """One md2_bn_backward_ex call on fresh guarded outputs.  dres: None, True (stored) or the initial
    tensor (with dres_acc).  skip: the addend of the flat range [skip_lo, skip_hi)."""
    ops = _ops()
    n, c, h, w = shape
    d = ops.bn_desc(shape, eps=EPS, momentum=MOM, route=route)
    o = {"dgamma": Guarded((c,)), "dbeta": Guarded((c,)), "dy": Guarded(shape)}
    kw = {}
    if slab is not None:
        o["dout_w"] = Guarded(shape)
        kw.update(slab=_dev(slab), dout_w=o["dout_w"].t)
    else:
        kw["dout"] = _dev(dout)
    if dres is not None:
        o["dres"] = Guarded(shape, init=None if dres is True else dres)
        kw.update(dres=o["dres"].t, dres_accumulate=dres_acc)
    if skip is not None:
        kw.update(skip=_dev(skip), skip_lo=skip_lo, skip_hi=skip_hi)
    info = ops.bn_backward_ex(d, _dev(y), _dev(mean), _dev(invstd), _dev(gamma), o["dgamma"].t, o["dbeta"].t,
                              o["dy"].t, mask=_dev(mask), mbeta=_dev(mbeta), **kw)
    torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact(), ("guard elements of %s were written" % k, shape, route)
    r = {k: b.cpu() for k, b in o.items()}
    r["info"] = info
    r["dev"] = o
    return r


# ---- the bound ---------------------------------------------------------------------------------------
def _check(tag, quantity, err, floor, well):
    """err / floor: per-channel measures of the kernel and of the fp32 evaluation against fp64."""
    e, f = float(err.max()), float(floor.max())
    bound = max(1e-6, 8.0 * f)
    print("BNERR %-46s %-9s floor %.3e err %.3e bound %.3e" % (tag, quantity, f, e, bound))
    assert e <= bound, (tag, quantity, "channel", int(err.argmax()), e, "floor", f, "bound", bound)
    if well is not None and bool(well.any()):      # channels with |mean|/std <= 4: the project's 1e-5 as well
        assert float(err[well].max()) < 1e-5, (tag, quantity, float(err[well].max()))


def _well(y, y2=None):
    """Per channel: |mean| <= 4 std of the data itself (of both branches), in fp64."""
    ok = None
    for t in (y, y2):
        if t is None:
            continue
        m, v = R.channel_stats(t)
        k = m.abs() <= 4.0 * torch.sqrt(v + EPS)
        ok = k if ok is None else ok & k
    return ok


def _check_info(info, shape, family, parts=None, fin_parts=None):
    e = SHAPES[shape]
    assert info["family"] == family, (shape, info)
    assert info["vec"] == bool(e.vec), (shape, info)
    if family == "one_kernel":
        assert (info["parts"], info["fin_parts"], info["upt"]) == (0, 0, 0), (shape, info)
    else:
        p = e.parts if parts is None else parts
        assert info["parts"] == p and info["fin_parts"] == (p if fin_parts is None else fin_parts), (shape, info)
        assert info["upt"] == (1 if family == "stem_pool" else e.upt), (shape, info)


def _check_forward(tag, got, ref, f32, well, run_ref=None, run_f32=None):
    _check(tag, "out", R.ch_max_rel(got["out"], ref["out"]), R.ch_max_rel(f32["out"], ref["out"]), well)
    for k in ("mean", "invstd", "mean2", "invstd2"):
        if k in ref:
            _check(tag, k, R.ch_rel(got[k], ref[k]), R.ch_rel(f32[k], ref[k]), well)
    if run_ref is not None:
        for k, a, b in (("run_mean", run_ref[0], run_f32[0]), ("run_var", run_ref[1], run_f32[1])):
            _check(tag, k, R.ch_rel(got[k], a), R.ch_rel(b, a), well)


def _check_backward(tag, got, ref, f32, well, dres_ref=None, dres_f32=None):
    _check(tag, "dy", R.ch_max_rel(got["dy"], ref["dy"]), R.ch_max_rel(f32["dy"], ref["dy"]), well)
    _check(tag, "dgamma", R.ch_scaled(got["dgamma"], ref["dgamma"], ref["sum_abs_gx"]),
           R.ch_scaled(f32["dgamma"], ref["dgamma"], ref["sum_abs_gx"]), well)
    _check(tag, "dbeta", R.ch_scaled(got["dbeta"], ref["dbeta"], ref["sum_abs_g"]),
           R.ch_scaled(f32["dbeta"], ref["dbeta"], ref["sum_abs_g"]), well)
    if dres_ref is not None:
        _check(tag, "dres", R.ch_max_rel(got["dres"], dres_ref), R.ch_max_rel(dres_f32, dres_ref), well)


def _ulps(a, b):
    """distance in fp32 steps (same-sign finite values)."""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max().item()


def _mid_images(shape):
    """flat range of the middle image(s): image 1 .. N-2 (N >= 3), else the last image."""
    n, c, h, w = shape
    chw = c * h * w
    i0 = min(1, n - 1)
    i1 = max(i0 + 1, n - 1)
    return i0 * chw, i1 * chw


def _skip_full(d, lo, hi):
    """The addend as a whole-tensor fp32 term: skip[e - lo] on [lo, hi), 0 elsewhere."""
    full = torch.zeros(d["dout"].numel())
    full[lo:hi] = d["skip"].reshape(-1)[:hi - lo]
    return full.view(d["dout"].shape)


def _slabs_of(x, splits, seed):
    """Split-K slabs [splits][C][N*HW] with channel-dependent scale, and their fp32 sum in split
    order from 0.0f as an [N][C][H][W] tensor (the conv's own reduction, done on the host)."""
    n, c, h, w = x.shape
    g = torch.Generator().manual_seed(seed)
    base = x.permute(1, 0, 2, 3).reshape(c, n * h * w)
    slab = torch.stack([base / splits + base.abs().mean(dim=1, keepdim=True) * 0.3 * torch.randn(base.shape, generator=g)
                        for _ in range(splits)])
    acc = torch.zeros_like(base)
    for q in range(splits):
        acc = acc + slab[q]
    return slab.contiguous(), acc.view(c, n, h, w).permute(1, 0, 2, 3).contiguous()


# ---- forward: operand forms x shapes x routes ----------------------------------------------------------
def _forward_case(shape, form, ill=False):
    d = _case(shape, ill)
    kw, run = _fwd_operands(d, form)
    n, c, h, w = shape
    total = float(n * h * w)
    ref = R.forward(d["y"], eps=EPS, **kw)
    f32 = R.forward_f32(d["y"], eps=EPS, **kw)
    well = _well(d["y"], kw.get("y2"))
    assert not (ill and bool(well.any()))
    run_ref = run_f32 = None
    if run:
        run_ref = R.running(d["rm0"], d["rv0"], ref["mean"], ref["var"], total, MOM)
        run_f32 = R.running_f32(d["rm0"], d["rv0"], f32["mean"], f32["var"], total, MOM)
    res = {}
    for route, family in _routes(shape):
        tag = "fwd %s%s %s r%d" % ("x".join(map(str, shape)), " ill" if ill else "", form, route)
        a = run_forward(shape, route, y=d["y"], run=(d["rm0"], d["rv0"]) if run else None, **kw)
        _check_info(a["info"], shape, family)
        _check_forward(tag, a, ref, f32, well, run_ref, run_f32)
        b = run_forward(shape, route, y=d["y"], run=(d["rm0"], d["rv0"]) if run else None, **kw)
        _assert_same(a, b, [k for k in a if k not in ("info", "dev")], tag + ": a repeat differs")
        if family in res:        # route 0 chose a family that also ran by argument: the same kernels
            _assert_same(a, res[family], [k for k in a if k not in ("info", "dev")], tag + ": route 0 differs")
        res[family] = a
    if len(res) == 2:            # "mean and invstd within an ulp of the two passes, not bitwise" (nn.h)
        for k in ("mean", "invstd"):
            assert _ulps(res["two_pass"][k], res["one_kernel"][k]) <= 1, (shape, form, k)


@pytest.mark.parametrize("form", list(FWD_FORMS))
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_forward_forms(shape, form):
    _forward_case(shape, form)


@pytest.mark.parametrize("form", list(FWD_FORMS))
def test_forward_ill_conditioned(form):
    _forward_case(ILL, form, ill=True)


# ---- backward: operand forms x shapes x routes ---------------------------------------------------------
def _backward_case(shape, form, ill=False, families=None):
    d = _case(shape, ill)
    n, c, h, w = shape
    vec = (h * w) % 4 == 0
    fkw, _ = _fwd_operands(d, BWD_FORMS[form])
    dout, slab = d["dout"], None
    if form == "mbeta_slabs":
        slab, dout = _slabs_of(d["dout"], 2, 5)
    lo = hi = 0
    skip_full = None
    if form == "mask_dres_skip" and vec:
        lo, hi = _mid_images(shape)
        skip_full = _skip_full(d, lo, hi)
    well = _well(d["y"])
    res = {}
    for family in families or _families(shape):
        route = ROUTE_OF[family]
        tag = "bwd %s%s %s r%d" % ("x".join(map(str, shape)), " ill" if ill else "", form, route)
        f = run_forward(shape, route, y=d["y"], **fkw)
        gate = (f["out"] > 0) if fkw["relu"] else None      # data: the kernel forward's own sign pattern
        ref = R.backward(dout, d["y"], d["gamma"], EPS, gate=gate, skip=skip_full)
        f32 = R.backward_f32(dout, d["y"], d["gamma"], EPS, gate=gate, skip=skip_full)
        kw = dict(y=d["y"], mean=f["mean"], invstd=f["invstd"], gamma=d["gamma"])
        dres_ref = dres_f32 = None
        if form in ("plain", "mbeta"):
            kw.update(dout=dout, mbeta=d["beta"] if form == "mbeta" else None)
        elif form == "mbeta_slabs":
            kw.update(slab=slab, mbeta=d["beta"])
        elif form == "mask_dres_skip":
            kw.update(dout=dout, mask=f["out"], dres=True)
            if vec:
                kw.update(skip=d["skip"].reshape(-1)[:hi - lo], skip_lo=lo, skip_hi=hi)
            dres_ref, dres_f32 = ref["g"], f32["g"]
        else:
            kw.update(dout=dout, mask=f["out"], dres=d["dres0"], dres_acc=True)
            dres_ref, dres_f32 = d["dres0"].double() + ref["g"], d["dres0"] + f32["g"]
        a = run_backward(shape, route, **kw)
        _check_info(a["info"], shape, family)
        _check_backward(tag, a, ref, f32, well, dres_ref, dres_f32)
        if form == "mbeta_slabs":
            if family == "one_kernel":      # "nothing but dy and dgamma/dbeta is written" (nn.h)
                assert a["dev"]["dout_w"].untouched(), tag
            else:
                assert _same_bits(a["dout_w"], dout), tag
        b = run_backward(shape, route, **kw)
        _assert_same(a, b, [k for k in a if k not in ("info", "dev")], tag + ": a repeat differs")
        if SHAPES[shape].fits == (family == "one_kernel"):       # the executor's choice is this family
            z = run_backward(shape, 0, **kw)
            _check_info(z["info"], shape, family)
            _assert_same(a, z, [k for k in a if k not in ("info", "dev")], tag + ": route 0 differs")
        res[family] = a


@pytest.mark.parametrize("form", list(BWD_FORMS))
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_backward_forms(shape, form):
    _backward_case(shape, form)


@pytest.mark.parametrize("form", list(BWD_FORMS))
def test_backward_ill_conditioned(form):
    _backward_case(ILL, form, ill=True)


# ---- the large shapes: units per thread 2, 4, 8 and the LDS-table clamp, reduced forms ----------------
@pytest.mark.parametrize("shape", BIG, ids=lambda s: "x".join(map(str, s)))
def test_units_per_thread(shape):
    assert SHAPES[shape].upt > 1
    d = _case(shape)
    fkw, _ = _fwd_operands(d, "res_relu")
    tag = "upt%d %s" % (SHAPES[shape].upt, "x".join(map(str, shape)))
    f = run_forward(shape, 1, y=d["y"], **fkw)
    _check_info(f["info"], shape, "two_pass")
    well = _well(d["y"])
    _check_forward(tag + " fwd res_relu", f, R.forward(d["y"], eps=EPS, **fkw), R.forward_f32(d["y"], eps=EPS, **fkw),
                   well)
    n, c, h, w = shape
    lo, hi = c * h * w, 2 * c * h * w                            # image 1
    skip_full = _skip_full(d, lo, hi)
    gate = f["out"] > 0
    ref = R.backward(d["dout"], d["y"], d["gamma"], EPS, gate=gate, skip=skip_full)
    f32 = R.backward_f32(d["dout"], d["y"], d["gamma"], EPS, gate=gate, skip=skip_full)
    kw = dict(y=d["y"], mean=f["mean"], invstd=f["invstd"], gamma=d["gamma"], dout=d["dout"], mask=f["out"], dres=True,
              skip=d["skip"].reshape(-1)[:hi - lo], skip_lo=lo, skip_hi=hi)
    a = run_backward(shape, 1, **kw)
    _check_info(a["info"], shape, "two_pass")
    _check_backward(tag + " bwd mask_dres_skip", a, ref, f32, well, ref["g"], f32["g"])
    b = run_backward(shape, 1, **kw)
    _assert_same(a, b, ("dy", "dgamma", "dbeta", "dres"), tag + ": a repeat differs")


# ---- caller partials: a conv epilogue's per-tile form, with and without the collapse -------------------
def _tile_partials(y):
    """[c][ceil(n*hw/256)][2] fp64 sum / sum of squares per 256-value tile of each channel's [n*hw] run."""
    n, c, h, w = y.shape
    v = y.permute(1, 0, 2, 3).reshape(c, -1).double()
    tiles = (v.shape[1] + 255) // 256
    v = torch.nn.functional.pad(v, (0, tiles * 256 - v.shape[1])).view(c, tiles, 256)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], dim=-1).contiguous()


@pytest.mark.parametrize("shape,tiles", [((6, 5, 24, 40), 23), ((4, 3, 96, 100), 150)])
def test_caller_partials(shape, tiles):
    d = _case(shape)
    kw, _ = _fwd_operands(d, "res_relu")
    part = _tile_partials(d["y"])
    assert part.shape == (shape[1], tiles, 2)
    ref = R.forward(d["y"], eps=EPS, **kw)
    f32 = R.forward_f32(d["y"], eps=EPS, **kw)
    total = float(shape[0] * shape[2] * shape[3])
    run_ref = R.running(d["rm0"], d["rv0"], ref["mean"], ref["var"], total, MOM)
    run_f32 = R.running_f32(d["rm0"], d["rv0"], f32["mean"], f32["var"], total, MOM)
    res = {}
    for collapse in (False, True):
        tag = "fwd %s parts%d collapse%d" % ("x".join(map(str, shape)), tiles, collapse)
        a = run_forward(shape, 0, y=d["y"], part=part, collapse=collapse, run=(d["rm0"], d["rv0"]), **kw)
        _check_info(a["info"], shape, "two_pass", parts=tiles, fin_parts=1 if collapse else tiles)
        _check_forward(tag, a, ref, f32, _well(d["y"]), run_ref, run_f32)
        b = run_forward(shape, 1, y=d["y"], part=part, collapse=collapse, run=(d["rm0"], d["rv0"]), **kw)
        _assert_same(a, b, ("out", "mean", "invstd", "run_mean", "run_var"), tag + ": a repeat differs")
        res[collapse] = a
    _assert_same(res[False], res[True], ("out", "mean", "invstd", "run_mean", "run_var"), "collapsed partials")


# ---- slab forms: bit-equal to the call on the host's presum --------------------------------------------
@pytest.mark.parametrize("splits", [1, 2, 5])
@pytest.mark.parametrize("shape", [(6, 5, 2, 3), (2, 3, 1, 4), (5, 4, 6, 10), (3, 2, 40, 48), (8, 3, 4, 260)],
                         ids=lambda s: "x".join(map(str, s)))
def test_slab_forms_equal_the_presummed_tensor(shape, splits):
    d = _case(shape)
    yslab, ysum = _slabs_of(d["y"], splits, 21)
    dslab, dsum = _slabs_of(d["dout"], splits, 22)
    kw, _ = _fwd_operands(d, "relu")
    run = (d["rm0"], d["rv0"])
    for family in _families(shape):
        route = ROUTE_OF[family]
        what = (shape, splits, family)
        a = run_forward(shape, route, slab=yslab, run=run, **kw)
        b = run_forward(shape, route, y=ysum, run=run, **kw)
        _check_info(a["info"], shape, family)
        assert _same_bits(a["y_out"], ysum), what
        _assert_same(a, b, ("out", "mean", "invstd", "run_mean", "run_var"), what)
        bw = dict(y=ysum, mean=a["mean"], invstd=a["invstd"], gamma=d["gamma"], mbeta=d["beta"])
        s = run_backward(shape, route, slab=dslab, **bw)
        t = run_backward(shape, route, dout=dsum, **bw)
        _check_info(s["info"], shape, family)
        _assert_same(s, t, ("dy", "dgamma", "dbeta"), what)
        if family == "one_kernel":          # "nothing but dy and dgamma/dbeta is written" (nn.h)
            assert s["dev"]["dout_w"].untouched(), what
        else:
            assert _same_bits(s["dout_w"], dsum), what


# ---- skip addend: bit-equal to dout with the range pre-added -------------------------------------------
def _skip_ranges(shape):
    n, c, h, w = shape
    chw, hw = c * h * w, h * w
    return {"empty": (chw, chw), "whole": (0, n * chw), "middle": _mid_images(shape),
            "mid_plane": ((chw + hw // 2) // 4 * 4, (2 * chw - hw // 3) // 4 * 4)}


@pytest.mark.parametrize("rng", ["empty", "whole", "middle", "mid_plane"])
@pytest.mark.parametrize("shape", [(5, 4, 6, 10), (3, 2, 40, 48), (8, 3, 4, 260), (3, 300, 2, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_skip_equals_preadded_dout(shape, rng):
    d = _case(shape)
    lo, hi = _skip_ranges(shape)[rng]
    assert 0 <= lo <= hi <= d["dout"].numel() and lo % 4 == 0 and hi % 4 == 0
    pre = d["dout"] + _skip_full(d, lo, hi)          # one fp32 add per element of the range
    fkw, _ = _fwd_operands(d, "res_relu")
    for family in _families(shape):
        route = ROUTE_OF[family]
        f = run_forward(shape, route, y=d["y"], **fkw)
        kw = dict(y=d["y"], mean=f["mean"], invstd=f["invstd"], gamma=d["gamma"], mask=f["out"], dres=True)
        skip = d["skip"].reshape(-1)[:max(hi - lo, 4)]           # (an empty range still passes a pointer)
        a = run_backward(shape, route, dout=d["dout"], skip=skip, skip_lo=lo, skip_hi=hi, **kw)
        b = run_backward(shape, route, dout=pre, **kw)
        _assert_same(a, b, ("dy", "dgamma", "dbeta", "dres"), (shape, rng, family))


# ---- ReLU gate re-derived from y: bit-equal to the forward's out as mask -------------------------------
@pytest.mark.parametrize("shape", [(5, 4, 6, 10), (9, 4, 4, 260), (6, 4, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_mbeta_equals_the_forward_output_as_mask(shape):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(77)
    y = 1.5 + 2.0 * torch.randn(*shape, generator=g)
    y = torch.round(y * 4) / 4                       # quantised
    dout = torch.randn(*shape, generator=g)
    gamma = torch.tensor([1.25, -0.75, 0.0, 0.0])     # gamma < 0, and gamma = 0 with beta = 0 and beta > 0
    beta = torch.tensor([0.25, -0.5, 0.0, 0.5])
    fits = bool(_ops().lib().md2_bn_channel_fits(n, h * w))
    for family in ["two_pass"] + (["one_kernel"] if fits else []):
        route = ROUTE_OF[family]
        f = run_forward(shape, route, gamma, beta, y=y, relu=True)
        assert f["info"]["family"] == family
        assert bool((f["out"][:, 2] == 0).all()) and bool((f["out"][:, 3] == 0.5).all())
        kw = dict(y=y, mean=f["mean"], invstd=f["invstd"], gamma=gamma, dout=dout)
        a = run_backward(shape, route, mbeta=beta, **kw)
        b = run_backward(shape, route, mask=f["out"], **kw)
        _assert_same(a, b, ("dy", "dgamma", "dbeta"), (shape, family))
        # the gate itself: relu'(0) = 0, so the all-zero channel passes no gradient, the beta > 0 one all of it
        assert float(a["dbeta"][2]) == 0.0 and float(a["dgamma"][2]) == 0.0
        ref = dout[:, 3].double().sum()
        assert abs(float(a["dbeta"][3]) - float(ref)) <= 1e-6 * float(dout[:, 3].abs().sum())


# ---- stem tail: BN + ReLU + max pool in one pass == bn_apply_fused then md2_maxpool3s2_fwd -------------
@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("shape", [(1, 2, 2, 2), (3, 4, 6, 8), (2, 5, 10, 12), (2, 64, 8, 16)],
                         ids=lambda s: "x".join(map(str, s)))
def test_stem_pool_equals_apply_then_pool(shape, quantised):
    ops = _ops()
    n, c, h, w = shape
    g = torch.Generator().manual_seed(31)
    ch = torch.arange(c)
    y = (0.5 * ((ch % 5) - 2.0)).view(1, c, 1, 1) + (0.5 + (ch % 3).float()).view(1, c, 1, 1) * torch.randn(*shape, generator=g)
    if quantised:
        y = torch.round(y)                           # ties: equal inputs give equal activations
    gamma = torch.where(ch % 3 == 1, -1.0, 1.0) * (0.5 + torch.randn(c, generator=g).abs())
    beta = 0.3 * torch.randn(c, generator=g)
    run = (0.1 * torch.randn(c, generator=g), 1.0 + torch.rand(c, generator=g))
    a = run_forward(shape, 1, gamma, beta, y=y, relu=True, run=run)
    py, parg = ops.maxpool3s2(a["dev"]["out"].t)
    b = run_forward(shape, 0, gamma, beta, y=y, relu=True, run=run, pool=True)
    assert b["info"]["family"] == "stem_pool" and b["info"]["upt"] == 1
    _assert_same(a, b, ("out", "mean", "invstd", "run_mean", "run_var"), shape)
    assert _same_bits(b["pool_y"], py.cpu()) and torch.equal(b["pool_arg"], parg.cpu()), shape
    if quantised and h * w >= 48:
        win = torch.nn.functional.pad(a["out"], (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2)
        flat = win.reshape(n, c, h // 2, w // 2, 9)
        assert int(((flat == flat.amax(-1, keepdim=True)).sum(-1) > 1).sum()) > 0      # the case has ties
        assert torch.equal(b["pool_arg"].long(), flat.argmax(-1))                      # first maximum
    ref = R.forward(y, gamma, beta, EPS, relu=True)
    f32 = R.forward_f32(y, gamma, beta, EPS, relu=True)
    _check("pool %s q%d" % ("x".join(map(str, shape)), quantised), "out", R.ch_max_rel(b["out"], ref["out"]),
           R.ch_max_rel(f32["out"], ref["out"]), _well(y))
    c2 = run_forward(shape, 0, gamma, beta, y=y, relu=True, run=run, pool=True)
    _assert_same(b, c2, ("out", "pool_y", "pool_arg", "mean", "invstd"), "a repeat differs")


def test_every_shape_of_the_table_reports_its_route():
    """The info record of a plain forward and backward per table row: family by route argument,
    partials and units per thread (the rows' mechanisms are exercised by the tests above)."""
    lib = _ops().lib()
    for shape, e in SHAPES.items():
        n, c, h, w = shape
        assert bool(lib.md2_bn_channel_fits(n, h * w)) == bool(e.fits), shape
        assert ((h * w) % 4 == 0) == bool(e.vec), shape
        if shape in BIG[:3]:
            continue                       # asserted by test_units_per_thread on the same calls
        d = _case(shape)
        for route, family in _routes(shape):
            f = run_forward(shape, route, d["gamma"], d["beta"], y=d["y"])
            _check_info(f["info"], shape, family)
            b = run_backward(shape, route, y=d["y"], mean=f["mean"], invstd=f["invstd"], gamma=d["gamma"],
                             dout=d["dout"])
            _check_info(b["info"], shape, family)
