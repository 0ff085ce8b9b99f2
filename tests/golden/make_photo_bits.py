"""Recorded bits of the photometric kernel: tests/golden/photo_bits.json.

This fixture's authority is the SCALAR photometric kernel at the commit the fixture names
("commit"): the packed kernel that runs today took its arithmetic order from that scalar kernel
and was held bit-identical to it while both existed.  The digests were recorded from the scalar
kernel, and the packed kernel gave the same digests in the same run; then the scalar kernel was
deleted.  From here on this script can only re-record from the surviving kernel, which proves
nothing by itself.  A re-record is legitimate only for a toolchain change (another hipcc than the
fixture's "hipcc" line), and only with the oracle parity tests green on that toolchain
(tests/test_gpu_loss.py, tests/test_gpu_bench_parity.py).

The case table (TAIL_CASES x VISUALIZE, OP_SCALES), the input builders and the digest function
live here and tests/test_gpu_photo_bits.py imports them: there is no second copy.

    python tests/golden/make_photo_bits.py --commit HASH    # rewrites tests/golden/photo_bits.json
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import _data as D  # noqa: E402

FIXTURE = os.path.join(HERE, "photo_bits.json")
SCALES = (0.125, 0.25, 0.5, 1.0)

# id: N, C, H, W, nscales, sources, automask, near -- the bench shape (B=12, 416x128, 4 scales)
# and odd shapes (one channel, a 96-wide frame whose level-1 disparity is 6 columns, automasking,
# near-field poses)
TAIL_CASES = {
    "bench-uniform": (12, 3, 128, 416, 4, "uniform", False, False),
    "bench-texture-automask": (12, 3, 128, 416, 4, "texture", True, False),
    "gray-96wide": (2, 1, 64, 96, 4, "texture", False, False),
    "near-field-automask": (3, 3, 64, 128, 2, "ramp", True, True),
}
VISUALIZE = {"plain": False, "cells": True}
OP_SCALES = (1, 4)


def digest(t):
    """SHA-256 over dtype, shape and the contiguous host bytes of a tensor, after the
    canonicalisation under which two tensors have equal digests exactly when no element differs
    by ``!=`` and NaNs sit in the same places: every NaN becomes one canonical NaN, -0.0 becomes
    +0.0."""
    a = np.array(t.detach().cpu().contiguous().numpy())     # an owned host copy
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
        a[a == 0] = 0
    h = hashlib.sha256()
    h.update(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def digests(named):
    """{name: tensor | list of tensors | None} -> {name or name[i]: hex | "none"}"""
    out = {}
    for k, v in named.items():
        if isinstance(v, (list, tuple)):
            for i, u in enumerate(v):
                out.update(digests({f"{k}[{i}]": u}))
        else:
            out[k] = "none" if v is None else digest(v)
    return out


def run_tail_case(name, visualize):
    """One loss_tail case -> (input digests, output digests); every key of the result except
    the workspace."""
    import md2hip
    N, C, H, W, nscales, sources, automask, near = TAIL_CASES[name]
    dev = torch.device("cuda")
    if sources == "uniform":
        g = torch.Generator().manual_seed(3)
        x = torch.rand(N, 3, C, H, W, generator=g, dtype=torch.float32)
    else:
        x = D.triplets(N, C, H, W, seed=7, ramp_sources=sources == "ramp").float()
    x = x.to(dev).contiguous()
    K, invK = D.intrinsics(W, H)
    disps = [d.float().to(dev).contiguous() for d in D.disparities(N, H, W, nscales=nscales, seed=11)]
    kw = dict(forward=0.05, jitter=0.2) if near else {}
    poses = [(a.float().to(dev), b.float().to(dev)) for a, b in D.poses(N, seed=13, **kw)]
    am = None
    if automask:
        am = (0.2 * torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(5))).to(dev).contiguous()
    cache = md2hip.TrainCache(K=K.numpy(), invK=invK.numpy(), scales=SCALES[-len(disps):])
    params = md2hip.Params(target_size=(W, H), batch_size=N, automasking=am is not None,
                           disparity_smoothness=1e-3)
    r = md2hip.loss_tail(disps, poses, x, am, cache, params, visualize=visualize)
    torch.cuda.synchronize()
    keys = sorted(set(r) - {"workspace"})
    assert {"loss", "terms", "d_disp", "d_pose"} <= set(keys)
    ins = digests({"x": x, "disp": disps, "poses": [t for pr in poses for t in pr], "automask": am})
    return ins, digests({k: r[k] for k in keys})


def run_op_case(scale):
    """md2_warp_photometric_fwd / _bwd (one scale, per-pixel cotangent map = the kernel's gmap
    path) through the op-level API -> (input digests, output digests)."""
    from md2hip import primitives as Pm
    dev = torch.device("cuda")
    N, C, H, W = 4, 3, 128, 416
    x = D.triplets(N, C, H, W, seed=7).float().to(dev).contiguous()
    K, invK = D.intrinsics(W, H)
    d = D.disparities(N, H, W, nscales=4, seed=11)[-1 if scale == 1 else 0].float().to(dev).contiguous()
    rt = torch.randn(2 * N, 12, generator=torch.Generator().manual_seed(2)) * 0.01
    rt[:, 0] += 1
    rt[:, 4] += 1
    rt[:, 8] += 1
    rt = rt.to(dev)
    dl = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(9)).to(dev)
    dd = d.clone().requires_grad_(True)
    rr = rt.clone().requires_grad_(True)
    out, sel = Pm.warp_photometric(dd, rr, x, K.numpy(), invK.numpy(), return_sel=True)
    out.backward(dl)
    torch.cuda.synchronize()
    ins = digests({"x": x, "disp": d, "rt": rt, "dl": dl})
    return ins, digests({"loss_map": out.detach(), "sel": sel, "d_disp": dd.grad, "d_Rt": rr.grad})


def tail_id(name, vis):
    return f"tail-{name}-{vis}"


def op_id(scale):
    return f"op-scale{scale}"


def record():
    """Every case -> {case id: {"inputs": {...}, "outputs": {...}}}"""
    cases = {}
    for vis, flag in VISUALIZE.items():
        for name in TAIL_CASES:
            ins, outs = run_tail_case(name, flag)
            cases[tail_id(name, vis)] = {"inputs": ins, "outputs": outs}
    for scale in OP_SCALES:
        ins, outs = run_op_case(scale)
        cases[op_id(scale)] = {"inputs": ins, "outputs": outs}
    return cases


def hipcc_version():
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, check=True).stdout
    return next(ln.strip() for ln in out.splitlines() if "version" in ln.lower())


def write_fixture(cases, commit, kernel, path=FIXTURE):
    with open(path, "w") as f:
        json.dump({"authority": "the scalar photometric kernel at `commit`; see make_photo_bits.py",
                   "commit": commit, "recorded_from": kernel, "hipcc": hipcc_version(),
                   "digest": "sha256(dtype.str + shape + bytes), NaN -> one NaN, -0.0 -> +0.0",
                   "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit whose library is loaded")
    args = ap.parse_args()
    write_fixture(record(), args.commit, "photo_stream_kernel (re-recorded from the surviving kernel)")
    print(FIXTURE)
