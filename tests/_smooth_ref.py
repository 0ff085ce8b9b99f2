"""Inputs and the fp64 reference for the smoothness path of the fused loss tail at full weight
(tests/test_smooth_ref.py on the CPU, tests/test_gpu_loss_smooth.py on the device).

Isolation.  The photometric gradient reaches the disparity and the poses only through the spatial
differences of the SOURCE frames.  ``frames`` keeps the textured target of tests/_data.py and makes
the two sources constant (0.3 and 0.7, so the argmin is no global tie): the photometric term stays
non-zero, its d_disp and d_pose are exactly zero, and the edge weights of the smoothness term --
taken from the target -- keep their structure.  What the tail returns in d_disp is then the
smoothness gradient alone, at its real weight.

Two disparity families keep every sign(d_q - d_r) decision identical in fp32 and fp64:
  A  low-res values on the 2^-10 grid in [0.1, 0.9] and sizes whose align-corners ratios
     (in-1)/(out-1) are dyadic: the upsampled disparity is bit-identical in fp32 and fp64, and a
     planted flat patch (top-left max(2, h//2) x max(2, w//3), where the scale has two rows and two
     columns) gives exact-zero differences in both directions (abs'(0) = 0).
  B  the model's halvings of 40 x 136, d = 0.5 +- (0.25 x - 0.12 y) + (0.1/max(h,w)) U[0,1): every
     horizontal difference keeps one sign, every vertical one the other, the samples alternate.

``reference`` restates src/training.jl:64-67 from the oracle's pieces; ``variant`` selects one of
seven deliberately wrong forms that only prove the inputs can tell them apart."""
import torch

from oracle import md2_oracle as O
from tests import _data as D

DEFAULT_SCALES = (0.125, 0.25, 0.5, 1.0)
SMOOTHNESS = 1e-3

# name -> (N, C, H, W, ((h, w) per scale))
CASES = {
    "A1": (2, 3, 33, 125, ((5, 32), (9, 63), (17, 125), (33, 125))),
    "A2": (1, 1, 9, 63, ((2, 32), (3, 32), (5, 63), (9, 63))),
    "A3": (3, 3, 33, 65, ((3, 5), (5, 9), (9, 17), (17, 33), (33, 65))),
    "A4": (1, 3, 9, 63, ((1, 32), (1, 32), (1, 63))),
    "B": (2, 3, 40, 136, ((5, 17), (10, 34), (20, 68), (40, 136))),
}
# A3 runs five scales through explicit weights (non-uniform, so a scale reading its neighbour's
# weight shows) and A4 three; the others use disparity_smoothness * scale
A3_WEIGHTS = (2e-4, 7e-4, 3e-4, 1e-3, 5e-4)
A4_WEIGHTS = (1e-3, 5e-4, 2.5e-4)
# One-column disparity maps are rejected by the host entry (the photometric pass loads the two
# column taps of the upsample as one pair), so of the in == 1 paths only dh == 1 exists.  A4 keeps
# the one-row scale (1, 32), adds (1, 63) (dw == W) and, for the known answer "a constant map has
# term 0 and gradient 0", a (1, 32) scale holding one value (63 columns allow no other dyadic
# ratio); these are the scale lists that must be refused:
A4_REJECTED = (((1, 1), (1, 32), (2, 1)), ((1, 1),), ((2, 1),))

VARIANTS = ("const_mean", "swap_norm", "abs0_plus", "edge_left", "drop_col_seams", "drop_row_seams",
            "prev_weight")
SEAM_COLS, SEAM_ROWS = 62, 8        # a wave's columns and a band's rows in smooth_kernel


def default_weights(name):
    if name == "A3":
        return A3_WEIGHTS
    if name == "A4":
        return A4_WEIGHTS
    return tuple(SMOOTHNESS * s for s in DEFAULT_SCALES)


def frames(N, C, H, W, seed=7, sources=(0.3, 0.7)):
    """[N,3,C,H,W] float64 on the fp32 grid: the textured target of D.triplets, constant sources."""
    x = D.triplets(N, C, H, W, seed=seed).clone()
    x[:, 0] = sources[0]
    x[:, 2] = sources[1]
    return D.fp32_grid(x).contiguous()


def has_patch(h, w):
    return h >= 2 and w >= 2


def family_a(N, shapes, seed=3):
    """Per scale [N,1,h,w] float64, integer multiples of 2^-10 in [0.1, 0.9], with the flat patch."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        k = torch.randint(103, 922, (N, 1, h, w), generator=g)
        if has_patch(h, w):
            k[:, :, :max(2, h // 2), :max(2, w // 3)] = k[:, :, :1, :1].clone()
        out.append((k.double() / 1024.0).contiguous())
    return out


def family_b(N, shapes, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        xx = torch.linspace(0, 1, w, dtype=torch.float64).view(1, 1, 1, w)
        yy = torch.linspace(0, 1, h, dtype=torch.float64).view(1, 1, h, 1)
        sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(N)], dtype=torch.float64)
        noise = (0.1 / max(h, w)) * torch.rand(N, 1, h, w, generator=g, dtype=torch.float64)
        d = 0.5 + sign.view(N, 1, 1, 1) * (0.25 * xx - 0.12 * yy) + noise
        out.append(D.fp32_grid(d).contiguous())
    return out


def case_inputs(name):
    """(disps, x, weights) of a named case."""
    N, C, H, W, shapes = CASES[name]
    disps = family_b(N, shapes) if name == "B" else family_a(N, shapes)
    if name == "A4":
        disps[0] = disps[0][..., :1].expand_as(disps[0]).contiguous()
    return disps, frames(N, C, H, W), default_weights(name)


def upsampled(d, H, W):
    return d if d.shape[-2:] == (H, W) else O.upsample_bilinear_size(d, (H, W))


class _AbsPlusAtZero(torch.autograd.Function):
    """|v| with the wrong subgradient +1 at 0."""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return v.abs()

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return g * torch.where(v < 0, -torch.ones_like(v), torch.ones_like(v))


def _smooth(dn, image, variant=None):
    """O.smooth_loss restated so that single pieces can be broken.  dn [N,H,W], image [N,C,H,W]."""
    N, H, W = dn.shape
    absf = _AbsPlusAtZero.apply if variant == "abs0_plus" else torch.abs
    ddx = absf(dn[:, :, :-1] - dn[:, :, 1:])
    ddy = absf(dn[:, :-1, :] - dn[:, 1:, :])
    ex = torch.exp(-torch.abs(image[:, :, :, :-1] - image[:, :, :, 1:]).mean(dim=1))
    ey = torch.exp(-torch.abs(image[:, :, :-1, :] - image[:, :, 1:, :]).mean(dim=1))
    if variant == "edge_left":
        ex = torch.cat([ex[:, :, :1], ex[:, :, :-1]], 2)
    if variant == "drop_col_seams":
        keep = (torch.arange(W - 1) % SEAM_COLS) != SEAM_COLS - 1
        ex = ex * keep.to(ex.dtype).view(1, 1, -1)
    if variant == "drop_row_seams":
        keep = (torch.arange(H - 1) % SEAM_ROWS) != SEAM_ROWS - 1
        ey = ey * keep.to(ey.dtype).view(1, -1, 1)
    nx, ny = N * H * (W - 1), N * (H - 1) * W
    if variant == "swap_norm":
        nx, ny = ny, nx
    return (ddx * ex).sum() / nx + (ddy * ey).sum() / ny


def reference(disps, x, weights, *, normalize=True, divisor=None, dloss=1.0, sigmoid_grad=False,
              dtype=torch.float64, variant=None):
    """The smoothness part of the loss tail.  disps: per scale [N,1,h,w]; x [N,3,C,H,W] (frame 1 is
    the target); weights: per scale, disparity_smoothness * scale.
    -> (terms [S] = weight * smooth, NOT divided by the divisor; loss = sum(terms) / divisor;
        d_disp per scale = d(dloss * loss)/d disp, times d (1 - d) with ``sigmoid_grad``)."""
    assert variant is None or variant in VARIANTS, variant
    target = x[:, 1].to(dtype)
    H, W = target.shape[-2:]
    leaves = [d.detach().to(dtype).clone().requires_grad_(True) for d in disps]
    divisor = float(len(disps) if divisor is None else divisor)
    weights = [float(w) for w in weights]
    if variant == "prev_weight":
        weights = weights[-1:] + weights[:-1]
    terms = []
    for d, w in zip(leaves, weights):
        full = upsampled(d, H, W)
        if normalize:
            mean = full.mean(dim=(2, 3), keepdim=True)
            if variant == "const_mean":
                mean = mean.detach()
            full = full / (mean + 1e-7)
        s = O.smooth_loss(full[:, 0], target) if variant is None else _smooth(full[:, 0], target, variant)
        terms.append(s * w)
    terms = torch.stack(terms)
    loss = terms.sum() / divisor
    (loss * dloss).backward()
    grads = []
    for d in leaves:
        g = d.grad if d.grad is not None else torch.zeros_like(d)
        grads.append((g * d * (1 - d) if sigmoid_grad else g).detach())
    return terms.detach(), loss.detach(), grads


def rel(a, b):
    """|a - b| / |b| of two scalars."""
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


def fp32_floor(disps, x, weights, **kw):
    """Per scale, the error of the reference evaluated by torch in fp32 against itself in fp64 on
    the same inputs: (d_disp rel Frobenius, term rel).  A scale whose fp64 result is exactly zero
    has floor 0 (its fp32 result must be zero too)."""
    t64, _, g64 = reference(disps, x, weights, dtype=torch.float64, **kw)
    t32, _, g32 = reference(disps, x, weights, dtype=torch.float32, **kw)
    fd, ft = [], []
    for s in range(len(disps)):
        if g64[s].norm().item() == 0.0:
            assert g32[s].norm().item() == 0.0, s
            fd.append(0.0)
        else:
            fd.append(D.rel_err(g32[s], g64[s]))
        if t64[s].item() == 0.0:
            assert t32[s].item() == 0.0, s
            ft.append(0.0)
        else:
            ft.append(rel(t32[s], t64[s]))
    return fd, ft


def bound(floor):
    """max(1e-5, 4 x floor): 1e-5 is what md2_smooth_loss_* is held to (tests/test_gpu_ops.py), 4 x
    the margin tests/_model_parity.py gives over an fp32 floor (one fp32 realisation is a single
    sample of the rounding error)."""
    return max(1e-5, 4.0 * floor)


def full_res_differences(d, H, W):
    """Horizontal and vertical neighbour differences of the upsampled disparity."""
    f = upsampled(d, H, W)[:, 0]
    return f[:, :, :-1] - f[:, :, 1:], f[:, :-1, :] - f[:, 1:, :]
