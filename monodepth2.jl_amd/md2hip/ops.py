"""Op-level host mirror: Flux ``Conv`` forward and its NNlib pullbacks (∇conv_data,
∇conv_filter) over the C-ABI.  Weights are cross-correlation [Cout, Cin, KH, KW]."""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import ConvDesc, ConvOperands, check, lib, ptr, stream_of

ACT = {None: 0, "identity": 0, "relu": 1, "elu": 2, "sigmoid": 3}


def conv_desc(x_shape, w_shape, stride=1, pad=0, reflect=False, act=None) -> ConvDesc:
    n, cin, h, w = x_shape
    cout, cin2, kh, kw = w_shape
    if cin != cin2:
        raise ValueError(f"channel mismatch {cin} vs {cin2}")
    d = ConvDesc()
    d.n, d.cin, d.h, d.w, d.cout, d.kh, d.kw = n, cin, h, w, cout, kh, kw
    d.stride, d.pad, d.reflect, d.act = stride, pad, int(reflect), ACT[act]
    return d


def _ws(d, dev):
    import torch
    nbytes = lib().md2_conv2d_workspace_size(C.byref(d))
    return torch.empty(max(nbytes // 4, 1) + 64, dtype=torch.float32, device=dev)


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv2d(x, weight, bias=None, stride=1, pad=0, reflect=False, act=None):
    """y = act(conv(x, w) + b) -- Flux ``Conv((k,k), cin=>cout, act; stride, pad)`` (cross-corr.)
    with ``reflect`` = ``DecoderBlock`` semantics (pad_reflect then valid conv)."""
    import torch
    d = conv_desc(tuple(x.shape), tuple(weight.shape), stride, pad, reflect, act)
    ho, wo = out_hw(d.h, d.w, d.kh, stride, pad)
    y = torch.empty(d.n, d.cout, ho, wo, dtype=torch.float32, device=x.device)
    check(lib().md2_conv2d_fwd(C.byref(d), ptr(x), ptr(weight), ptr(bias), ptr(y),
                               ptr(_ws(d, x.device)), stream_of(x.device)), "md2_conv2d_fwd")
    return y


def conv2d_dgrad(dy, weight, x_shape, stride=1, pad=0, reflect=False):
    """NNlib ``∇conv_data``: dx from the pre-activation output gradient."""
    import torch
    d = conv_desc(tuple(x_shape), tuple(weight.shape), stride, pad, reflect)
    dx = torch.empty(*x_shape, dtype=torch.float32, device=dy.device)
    check(lib().md2_conv2d_dgrad(C.byref(d), ptr(dy), ptr(weight), ptr(dx), ptr(_ws(d, dy.device)),
                                 stream_of(dy.device)), "md2_conv2d_dgrad")
    return dx


def conv2d_wgrad(x, dy, w_shape, stride=1, pad=0, reflect=False, bias=True):
    """NNlib ``∇conv_filter`` (+ the bias gradient)."""
    import torch
    d = conv_desc(tuple(x.shape), tuple(w_shape), stride, pad, reflect)
    dw = torch.empty(*w_shape, dtype=torch.float32, device=x.device)
    db = torch.empty(w_shape[0], dtype=torch.float32, device=x.device) if bias else None
    check(lib().md2_conv2d_wgrad(C.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(db), ptr(_ws(d, x.device)),
                                 stream_of(x.device)), "md2_conv2d_wgrad")
    return dw, db


def conv_operands(in1=None, in_c0=0, in_bs0=0, in_bs1=0, in_bdiv=0, in_bhi=0, out1=None, out_c0=0,
                  out_bs0=0, out_bs1=0, accumulate=False, cin_w=0) -> ConvOperands:
    """``md2_conv_operands``: the operand forms of the train step (include/md2.h).  ``in1`` /
    ``out1`` are tensors (or views) whose first element is the second base pointer; strides count
    floats, 0 = contiguous."""
    o = ConvOperands()
    o.in1 = None if in1 is None else in1.data_ptr()
    o.out1 = None if out1 is None else out1.data_ptr()
    o.in_bs0, o.in_bs1, o.in_bhi, o.out_bs0, o.out_bs1 = in_bs0, in_bs1, in_bhi, out_bs0, out_bs1
    o.in_c0, o.in_bdiv, o.out_c0, o.accumulate, o.cin_w = in_c0, in_bdiv, out_c0, int(accumulate), cin_w
    o._keep = (in1, out1)
    return o


def conv_last_kernel() -> str:
    """Kernel family of the calling thread's last conv launch (``md2_conv_last_kernel``)."""
    return lib().md2_conv_last_kernel().decode()


def conv2d_ex_workspace(d, o, dev):
    import torch
    nbytes = lib().md2_conv2d_ex_workspace_size(C.byref(d), C.byref(o) if o is not None else None)
    if nbytes == 0:
        raise ValueError("md2_conv2d_ex_workspace_size: invalid conv description")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev)


def _ex_result(defer, ws, rows, cols):
    info = {"kernel": conv_last_kernel(), "splits": 0, "slab": None, "stats_parts": 0}
    if defer is not None:
        info["splits"], info["stats_parts"] = defer.splits, defer.stats_parts
        if defer.splits > 0:
            off = (defer.slab - ws.data_ptr()) // 4
            info["slab"] = ws[off:off + defer.splits * rows * cols].view(defer.splits, rows, cols)
    return info


def conv2d_fwd_ex(d, o, x, weight, bias, y, defer=False, stats=None, ws=None):
    """``md2_conv2d_fwd_ex`` on caller-owned buffers: ``x`` / ``y`` (tensors or views) give the
    first base pointers, ``o`` (:func:`conv_operands`) the rest.  ``defer``: ask for the split-K
    deferral; ``stats``: a float64 tensor [cout, ceil(n*ho*wo/256), 2] offered to the epilogue.
    Returns {kernel, splits, slab ([splits, cout, n*ho*wo] view of the workspace, or None),
    stats_parts}; keep the result alive while ``slab`` is read."""
    ws = conv2d_ex_workspace(d, o, x.device) if ws is None else ws
    df = None
    if defer or stats is not None:
        df = _lib.ConvDefer()
        df.defer_reduce = int(bool(defer))
    ho, wo = out_hw(d.h, d.w, d.kh, d.stride, d.pad)
    check(lib().md2_conv2d_fwd_ex(C.byref(d), C.byref(o) if o is not None else None, ptr(x), ptr(weight),
                                  ptr(bias), ptr(y), ptr(stats), C.byref(df) if df is not None else None,
                                  ptr(ws), ws.numel() * 4, stream_of(x.device)), "md2_conv2d_fwd_ex")
    return _ex_result(df, ws, d.cout, d.n * ho * wo)


def conv2d_dgrad_ex(d, o, dy, weight, dx, defer=False, ws=None):
    """``md2_conv2d_dgrad_ex``: dx (split / strided / accumulated as ``o`` says) from dy."""
    ws = conv2d_ex_workspace(d, o, dy.device) if ws is None else ws
    df = None
    if defer:
        df = _lib.ConvDefer()
        df.defer_reduce = 1
    check(lib().md2_conv2d_dgrad_ex(C.byref(d), C.byref(o) if o is not None else None, ptr(dy), ptr(weight),
                                    ptr(dx), C.byref(df) if df is not None else None, ptr(ws), ws.numel() * 4,
                                    stream_of(dy.device)), "md2_conv2d_dgrad_ex")
    return _ex_result(df, ws, d.cin, d.n * d.h * d.w)


def conv2d_wgrad_ex(d, o, x, dy, dw, db=None, db_part=None, ws=None):
    """``md2_conv2d_wgrad_ex``: dw [cout, cin_w or cin, k, k] and db (stored, or accumulated with
    ``o.accumulate``); ``db_part`` [cout, parts] from :func:`act_backward_bias`."""
    ws = conv2d_ex_workspace(d, o, x.device) if ws is None else ws
    check(lib().md2_conv2d_wgrad_ex(C.byref(d), C.byref(o) if o is not None else None, ptr(x), ptr(dy), ptr(dw),
                                    ptr(db), ptr(db_part), 0 if db_part is None else db_part.shape[1], ptr(ws),
                                    ws.numel() * 4, stream_of(x.device)), "md2_conv2d_wgrad_ex")
    return _ex_result(None, ws, 0, 0)


def bn_desc(shape, eps=1e-5, momentum=0.1, route=0, collapse=False) -> "_lib.BNDesc":
    """``md2_bn_desc`` of an [n, c, h, w] BatchNorm; route 0 = the executor's choice, 1 = two
    passes, 2 = one kernel."""
    n, c, h, w = shape
    return _lib.BNDesc(n=n, c=c, h=h, w=w, eps=eps, momentum=momentum, route=route, collapse=int(bool(collapse)))


def bn_ex_workspace(d, dev):
    import torch
    nbytes = lib().md2_bn_ex_workspace_size(C.byref(d))
    if nbytes == 0:
        raise ValueError("md2_bn_ex_workspace_size: invalid BatchNorm description")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev)


def _bn_operands(S, tensors, ints):
    o = S()
    for k, t in tensors.items():
        setattr(o, k, None if t is None else t.data_ptr())
    for k, v in ints.items():
        setattr(o, k, int(v))
    o._keep = tuple(tensors.values())
    return o


def _bn_info(inf):
    return {"family": {1: "two_pass", 2: "one_kernel", 3: "stem_pool"}.get(inf.family, inf.family),
            "parts": inf.parts, "fin_parts": inf.fin_parts, "upt": inf.upt, "vec": bool(inf.vec)}


def bn_forward_ex(d, out, gamma, beta, mean, invstd, y=None, slab=None, y_out=None, part=None, run_mean=None,
                  run_var=None, y2=None, gamma2=None, beta2=None, mean2=None, invstd2=None, res=None, relu=False,
                  pool_y=None, pool_arg=None, ws=None):
    """``md2_bn_forward_ex`` on caller-owned buffers (tensors or views give the base pointers).
    ``slab`` [splits, c, n*h*w] is summed into ``y_out``; ``part`` [c, parts, 2] float64 are
    caller statistics partials.  Returns {family, parts, fin_parts, upt, vec}."""
    dev = out.device
    ws = bn_ex_workspace(d, dev) if ws is None else ws
    o = _bn_operands(_lib.BNFwdOperands,
                     dict(y=y, slab=slab, y_out=y_out, part=part, gamma=gamma, beta=beta, mean=mean, invstd=invstd,
                          run_mean=run_mean, run_var=run_var, y2=y2, gamma2=gamma2, beta2=beta2, mean2=mean2,
                          invstd2=invstd2, res=res, out=out, pool_y=pool_y, pool_arg=pool_arg),
                     dict(splits=0 if slab is None else slab.shape[0], parts=0 if part is None else part.shape[1],
                          relu=bool(relu)))
    inf = _lib.BNInfo()
    check(lib().md2_bn_forward_ex(C.byref(d), C.byref(o), C.byref(inf), ptr(ws), ws.numel() * ws.element_size(),
                                  stream_of(dev)), "md2_bn_forward_ex")
    return _bn_info(inf)


def bn_backward_ex(d, y, mean, invstd, gamma, dgamma, dbeta, dy, dout=None, slab=None, dout_w=None, mask=None,
                   mbeta=None, dres=None, dres_accumulate=False, skip=None, skip_lo=0, skip_hi=0, ws=None):
    """``md2_bn_backward_ex``: ``dout`` or ``slab`` [splits, c, n*h*w] (two passes write the sum
    to ``dout_w``), gated by ``mask`` > 0 or by the ReLU re-derived from ``y`` with ``mbeta``;
    ``skip`` is added over the flat elements [skip_lo, skip_hi).  Returns the info record."""
    dev = dy.device
    ws = bn_ex_workspace(d, dev) if ws is None else ws
    o = _bn_operands(_lib.BNBwdOperands,
                     dict(dout=dout, slab=slab, dout_w=dout_w, mask=mask, y=y, mean=mean, invstd=invstd, gamma=gamma,
                          mbeta=mbeta, dgamma=dgamma, dbeta=dbeta, dy=dy, dres=dres, skip=skip),
                     dict(skip_lo=skip_lo, skip_hi=skip_hi, splits=0 if slab is None else slab.shape[0],
                          dres_accumulate=bool(dres_accumulate)))
    inf = _lib.BNInfo()
    check(lib().md2_bn_backward_ex(C.byref(d), C.byref(o), C.byref(inf), ptr(ws), ws.numel() * ws.element_size(),
                                   stream_of(dev)), "md2_bn_backward_ex")
    return _bn_info(inf)


def maxpool3s2_backward_ex(dy, arg, dx, skip=None, skip_lo=0, skip_hi=0):
    """``md2_maxpool3s2_bwd_ex`` into the caller's ``dx`` [n, c, h, w]: the pool's pullback plus
    ``skip`` over the flat elements [skip_lo, skip_hi) (whole planes)."""
    n, c, h, w = dx.shape
    check(lib().md2_maxpool3s2_bwd_ex(ptr(dy), ptr(arg), n, c, h, w, ptr(dx), ptr(skip), skip_lo, skip_hi,
                                      stream_of(dy.device)), "md2_maxpool3s2_bwd_ex")
    return dx


def act_backward_bias(out, dout, act):
    """:func:`act_backward` over [n, c, h, w] fused with the per-channel partial sums of dpre:
    returns (dpre, part [c, parts])."""
    import torch
    n, c = out.shape[0], out.shape[1]
    hw = out[0, 0].numel()
    parts = lib().md2_act_bias_parts(c, n, hw)
    dpre = torch.empty_like(dout)
    part = torch.empty(c, max(parts, 1), dtype=torch.float32, device=out.device)
    check(lib().md2_act_backward_bias(ptr(out), ptr(dout), ptr(dpre), n, c, hw, ACT[act], ptr(part),
                                      stream_of(out.device)), "md2_act_backward_bias")
    return dpre, part


def act_backward(out, dout, act):
    import torch
    dpre = torch.empty_like(dout)
    check(lib().md2_act_backward(ptr(out), ptr(dout), ptr(dpre), dout.numel(), ACT[act],
                                 stream_of(out.device)), "md2_act_backward")
    return dpre


def maxpool3s2(x):
    """ResNet stem ``MaxPool((3,3), pad=1, stride=2)``: (y, arg) with arg the uint8 window index
    of the first maximum, kept for :func:`maxpool3s2_backward`."""
    import torch
    n, c, h, w = x.shape
    y = torch.empty(n, c, (h + 1) // 2, (w + 1) // 2, dtype=torch.float32, device=x.device)
    arg = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
    check(lib().md2_maxpool3s2_fwd(ptr(x), n, c, h, w, ptr(y), ptr(arg), stream_of(x.device)),
          "md2_maxpool3s2_fwd")
    return y, arg


def maxpool3s2_backward(dy, arg, x_shape):
    import torch
    n, c, h, w = x_shape
    dx = torch.empty(n, c, h, w, dtype=torch.float32, device=dy.device)
    check(lib().md2_maxpool3s2_bwd(ptr(dy), ptr(arg), n, c, h, w, ptr(dx), stream_of(dy.device)),
          "md2_maxpool3s2_bwd")
    return dx


def upsample2(x):
    """``upsample_bilinear(x, (2,2))`` with align_corners (src/depth_decoder.jl:18-19)."""
    import torch
    n, c, h, w = x.shape
    y = torch.empty(n, c, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
    check(lib().md2_upsample2_fwd(ptr(x), n, c, h, w, ptr(y), stream_of(x.device)),
          "md2_upsample2_fwd")
    return y


def upsample2_backward(dy):
    import torch
    n, c, h2, w2 = dy.shape
    dx = torch.empty(n, c, h2 // 2, w2 // 2, dtype=torch.float32, device=dy.device)
    check(lib().md2_upsample2_bwd(ptr(dy), n, c, h2 // 2, w2 // 2, ptr(dx), stream_of(dy.device)),
          "md2_upsample2_bwd")
    return dx
