"""Plain references of the BatchNorm forward and backward on the CPU (tests/test_gpu_bn_ops.py).

`forward` / `backward` / `running` are the operation in fp64, every statistic taken from y itself
(two-pass mean and biased variance).  `forward_f32` / `backward_f32` / `running_f32` evaluate the
same operation in fp32 the way a correct fp32 kernel has to -- fp64 sums, mean / invstd rounded to
fp32, every elementwise step rounded to fp32, no fused multiply-add -- so their error against the
fp64 functions is the rounding floor of a case: it grows with |mean| / std, because the rounding of
mean is multiplied by invstd.  Nothing here reads a kernel's output except the ReLU gate, which is
data (`gate`: a boolean tensor).

The per-channel error measures of the tests live here too."""
import torch

DIMS = (0, 2, 3)


def _b(v):
    return v.view(1, -1, 1, 1)


def channel_stats(y):
    """fp64 mean and biased variance over N*H*W per channel (two passes)."""
    y = y.double()
    m = y.mean(dim=DIMS)
    return m, ((y - _b(m)) ** 2).mean(dim=DIMS)


def forward(y, gamma, beta, eps, y2=None, gamma2=None, beta2=None, res=None, relu=False):
    """out = act(gamma*(y-mean)*invstd + beta [+ gamma2*(y2-mean2)*invstd2 + beta2] [+ res])."""
    r = {}
    m, v = channel_stats(y)
    r["mean"], r["var"], r["invstd"] = m, v, 1.0 / torch.sqrt(v + eps)
    out = _b(gamma.double()) * (y.double() - _b(m)) * _b(r["invstd"]) + _b(beta.double())
    if y2 is not None:
        m2, v2 = channel_stats(y2)
        r["mean2"], r["invstd2"] = m2, 1.0 / torch.sqrt(v2 + eps)
        out = out + _b(gamma2.double()) * (y2.double() - _b(m2)) * _b(r["invstd2"]) + _b(beta2.double())
    if res is not None:
        out = out + res.double()
    r["out"] = out.clamp_min(0.0) if relu else out
    return r


def running(old_mean, old_var, mean, var, total, momentum):
    """(1-m)*old + m*new, the variance unbiased by total / max(total-1, 1)."""
    m = float(momentum)
    unb = var * (total / max(total - 1.0, 1.0))
    return (1.0 - m) * old_mean.double() + m * mean, (1.0 - m) * old_var.double() + m * unb


def backward(dout, y, gamma, eps, gate=None, skip=None):
    """g = (dout [+ skip]) * gate; dbeta = sum g; dgamma = sum g*xhat;
    dy = gamma*invstd*(g - dbeta/L - xhat*dgamma/L).  Also sum|g| and sum|g*xhat| (the scales
    dbeta and dgamma are measured against)."""
    L = y.shape[0] * y.shape[2] * y.shape[3]
    m, v = channel_stats(y)
    invstd = 1.0 / torch.sqrt(v + eps)
    g = dout.double()
    if skip is not None:
        g = g + skip.double()
    if gate is not None:
        g = g * gate.double()
    xhat = (y.double() - _b(m)) * _b(invstd)
    gx = g * xhat
    dbeta, dgamma = g.sum(dim=DIMS), gx.sum(dim=DIMS)
    dy = _b(gamma.double() * invstd) * (g - _b(dbeta) / L - xhat * _b(dgamma) / L)
    return {"g": g, "dbeta": dbeta, "dgamma": dgamma, "dy": dy, "sum_abs_g": g.abs().sum(dim=DIMS),
            "sum_abs_gx": gx.abs().sum(dim=DIMS)}


# ---- the same operation in fp32 (fp64 sums): the rounding floor -------------------------------------
def _stats_f32(y, eps):
    """One-pass fp64 sums of the fp32 data; mean and invstd rounded to fp32; var kept in fp64."""
    yd = y.double()
    total = float(y.shape[0] * y.shape[2] * y.shape[3])
    mu = yd.sum(dim=DIMS) / total
    var = ((yd * yd).sum(dim=DIMS) / total - mu * mu).clamp_min(0.0)
    return mu.float(), (1.0 / torch.sqrt(var + eps)).float(), var


def _affine_f32(y, gamma, beta, meanf, isf):
    sc = gamma.float() * isf
    sh = beta.float() - meanf * sc
    return y.float() * _b(sc) + _b(sh)


def forward_f32(y, gamma, beta, eps, y2=None, gamma2=None, beta2=None, res=None, relu=False):
    r = {}
    r["mean"], r["invstd"], r["var"] = _stats_f32(y, eps)
    out = _affine_f32(y, gamma, beta, r["mean"], r["invstd"])
    if y2 is not None:
        r["mean2"], r["invstd2"], _ = _stats_f32(y2, eps)
        out = out + _affine_f32(y2, gamma2, beta2, r["mean2"], r["invstd2"])
    if res is not None:
        out = out + res.float()
    r["out"] = out.clamp_min(0.0) if relu else out
    return r


def running_f32(old_mean, old_var, meanf, var, total, momentum):
    m = torch.tensor(momentum, dtype=torch.float32)
    one = torch.tensor(1.0, dtype=torch.float32)
    unb = (var * (total / max(total - 1.0, 1.0))).float()
    return (one - m) * old_mean.float() + m * meanf, (one - m) * old_var.float() + m * unb


def backward_f32(dout, y, gamma, eps, gate=None, skip=None):
    L = y.shape[0] * y.shape[2] * y.shape[3]
    meanf, isf, _ = _stats_f32(y, eps)
    g = dout.float()
    if skip is not None:
        g = g + skip.float()
    if gate is not None:
        g = g * gate.float()
    xhat = (y.float() - _b(meanf)) * _b(isf)
    dbeta = g.double().sum(dim=DIMS).float()
    dgamma = (g.double() * xhat.double()).sum(dim=DIMS).float()
    invL = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(L), dtype=torch.float32)
    dy = _b(gamma.float() * isf) * (g - _b(dbeta * invL) - xhat * _b(dgamma * invL))
    return {"g": g, "dbeta": dbeta, "dgamma": dgamma, "dy": dy}


# ---- per-channel error measures -----------------------------------------------------------------------
def ratio(err, den):
    """err / den per channel; a zero scale demands a zero error (0, else inf)."""
    r = err / den.clamp_min(torch.finfo(torch.float64).tiny)
    r = torch.where(den > 0, r, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return r


def ch_max_rel(got, ref):
    """max|got - ref| / max|ref| over each channel of [N][C][H][W]."""
    return ratio((got.double() - ref).abs().amax(dim=DIMS), ref.abs().amax(dim=DIMS))


def ch_rel(got, ref):
    """|got - ref| / |ref| of a per-channel vector."""
    return ratio((got.double() - ref).abs(), ref.abs())


def ch_scaled(got, ref, scale):
    """|got - ref| / scale of a per-channel vector (dgamma against sum|g*xhat|, dbeta against sum|g|)."""
    return ratio((got.double() - ref).abs(), scale)
