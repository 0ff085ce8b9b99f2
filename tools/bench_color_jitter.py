"""Colour-jitter timing: one md2hip.color_jitter call on a batch against (a) the torch composition a
user would otherwise write on the device -- the same formulas as tensor ops, one sample at a time
because each sample has its own order -- and (b) the traffic floor: the call must move one read of x
for the reduction pass and one read and one write for the second, 3 * 4 * numel(x) bytes.  Then the
captured train step (train_step_graph) with and without x_net, at the bench configuration
(ResNet-18, N = 12, 128x416, no automask).

Workload: N = 12, 3 frames, 3x128x416, every sample applied, contrast in the middle of the order.

Each repeat is a window of `--calls` back-to-back calls between two device events; the paths
alternate, and the reported time per call is the median over `--repeats` windows after warm-up.  The
same for the steps (`--steps` per window).  The step windows also give the run-to-run spread (min and
max over the windows) the difference is to be read against.  Prints ONE JSON line:

    python tools/bench_color_jitter.py [--repeats 20] [--calls 20] [--steps 10] [--cold]
           [--bench-line parent=FILE --bench-line this=FILE] > profiles/<tag>_color_jitter.json

The batch (23 MB) and its jittered copy stay far below the 256 MiB Infinity Cache, so in a loop that
re-reads the same batch the achieved bytes per second is a cache-resident figure, not an HBM one;
`--cold` interleaves a 512 MiB fill between calls (timed separately and subtracted) to show the
other end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, FRAMES, C, H, W = 12, 3, 3, 128, 416
HBM_ACHIEVABLE = 6.3e12      # bytes/s a streaming copy reaches on an MI355X (8.0e12 is the specification)


def _blend(a, b, t):
    return (t * a + (1.0 - t) * b).clamp(0.0, 1.0)


def _gray(v):
    return (0.2989 * v[:, 0] + 0.587 * v[:, 1] + 0.114 * v[:, 2]).unsqueeze(1)


def _hue(v, hue):
    import torch
    r, g, b = v.unbind(1)
    mx, mn = v.max(1).values, v.min(1).values
    eq = mx == mn
    cr = mx - mn
    one = torch.ones_like(mx)
    s = cr / torch.where(eq, one, mx)
    d = torch.where(eq, one, cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    hh = torch.where(mx == r, bc - gc, torch.where(mx == g, 2.0 + rc - bc, 4.0 + gc - rc))
    hh = torch.frac(hh / 6.0 + 1.0)
    t = hh + hue
    hh = t - torch.floor(t)
    h6 = hh * 6.0
    i = torch.floor(h6)
    f = h6 - i
    i = i.to(torch.int64) % 6
    p = (mx * (1.0 - s)).clamp(0.0, 1.0)
    q = (mx * (1.0 - s * f)).clamp(0.0, 1.0)
    tt = (mx * (1.0 - s * (1.0 - f))).clamp(0.0, 1.0)
    sel = torch.stack([torch.stack(c, 1) for c in ((mx, tt, p), (q, mx, p), (p, mx, tt), (p, q, mx), (tt, p, mx),
                                                   (mx, p, q))], 0)                 # [6][F][3][H][W]
    return torch.gather(sel, 0, i[None, :, None].expand(1, *v.shape))[0]


def torch_color_jitter(x, params):
    """torchvision's float-tensor ColorJitter as tensor ops; a sample's frames go together"""
    import torch
    out = torch.empty_like(x)
    for k in range(x.shape[0]):
        v = x[k]                                                  # [frames][3][H][W]
        if not params["apply"][k]:
            out[k] = v
            continue
        for op in params["order"][k]:
            if op == 0:
                v = (float(params["brightness"][k]) * v).clamp(0.0, 1.0)
            elif op == 1:
                v = _blend(v, _gray(v).mean((1, 2, 3), keepdim=True), float(params["contrast"][k]))
            elif op == 2:
                v = _blend(v, _gray(v), float(params["saturation"][k]))
            else:
                v = _hue(v, float(params["hue"][k]))
        out[k] = v
    return out


def _windows(paths, repeats, per_window, warmup):
    """{name: [ms per call of each window]}: the paths alternate window by window"""
    import torch
    for f in paths.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(repeats):
        for k, f in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_window):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / per_window)
    return ms


def _summary(ms):
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--bench-line", action="append", default=[], metavar="NAME=FILE",
                    help="embed ms_per_step / value of the bench.py JSON lines in FILE under NAME (e.g. the "
                         "parent's and this build's lines from the same job)")
    args = ap.parse_args()

    import numpy as np
    import torch
    import md2hip
    from md2hip.dist import synthetic_triplets

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x = synthetic_triplets(N, H, W, 0, dev)
    assert tuple(x.shape) == (N, FRAMES, C, H, W)
    cj = md2hip.ColorJitter(p=1.0)
    params = cj.draw(list(range(N)), 0)
    orders = [(0, 1, 2, 3), (3, 1, 0, 2), (2, 0, 1, 3), (0, 3, 1, 2), (3, 2, 1, 0), (2, 1, 3, 0)]   # contrast 2nd / 3rd
    params["order"] = np.array([orders[k % len(orders)] for k in range(N)], dtype=np.uint8)
    out = torch.empty_like(x)

    ours, theirs = cj(x, params, out=out).clone(), torch_color_jitter(x, params)
    torch.cuda.synchronize()
    agree = float((ours - theirs).abs().max())

    kernel_paths = {"md2hip_color_jitter": lambda: cj(x, params, out=out),
                    "torch_composition": lambda: torch_color_jitter(x, params)}
    kms = _windows(kernel_paths, args.repeats, args.calls, args.warmup)
    ksum = _summary(kms)
    floor_bytes = 3 * x.numel() * 4
    t_ours = ksum["md2hip_color_jitter"]["median_ms"] * 1e-3
    result = {
        "tool": "bench_color_jitter", "device": torch.cuda.get_device_name(0), "batch": [N, FRAMES, C, H, W],
        "repeats": args.repeats, "calls_per_window": args.calls, "steps_per_window": args.steps,
        "max_abs_diff_between_paths": agree,
        "call": ksum,
        "torch_over_md2hip": round(ksum["torch_composition"]["median_ms"] / ksum["md2hip_color_jitter"]["median_ms"], 2),
        "traffic_floor_bytes": floor_bytes,
        "achieved_bytes_per_s_cache_resident": round(floor_bytes / t_ours, 0),
        "share_of_hbm_achievable_6.3e12_cache_resident": round(floor_bytes / t_ours / HBM_ACHIEVABLE, 3),
        "batch_sits_in_infinity_cache": True,
    }

    if args.cold:
        # evict: a 512 MiB fill between calls, timed alone and subtracted
        big = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        cold = {"fill_then_jitter": lambda: (big.fill_(1), cj(x, params, out=out)), "fill_alone": lambda: big.fill_(1)}
        cms = _summary(_windows(cold, args.repeats, args.calls, args.warmup))
        t_cold = (cms["fill_then_jitter"]["median_ms"] - cms["fill_alone"]["median_ms"]) * 1e-3
        result["cold"] = cms
        result["cold_call_ms"] = round(t_cold * 1e3, 4)
        result["achieved_bytes_per_s_after_eviction"] = round(floor_bytes / t_cold, 0) if t_cold > 0 else None
        result["share_of_hbm_achievable_6.3e12_after_eviction"] = (round(floor_bytes / t_cold / HBM_ACHIEVABLE, 3)
                                                                   if t_cold > 0 else None)

    # the captured step at the bench configuration, with and without x_net, and the 23 MB copy alone
    enc = md2hip.ResNet(18, in_channels=3)
    K, invK = md2hip.depth10k_intrinsics(W, H)
    cache = md2hip.TrainCache(K=K, invK=invK, scales=(0.125, 0.25, 0.5, 1.0))
    prm = md2hip.Params(target_size=(W, H), batch_size=N, automasking=False, disparity_smoothness=1e-3)
    steps = {}
    keep = []
    for name in ("step_plain", "step_x_net", "step_x_net_with_jitter"):
        model = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                      embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]),
                             device=dev, seed=42)
        ex, opt, loss = model.executor(tuple(x.shape), cache, prm), md2hip.ADAM(1e-4), torch.empty(1, device=dev)
        keep.append((model, ex, opt, loss))
        if name == "step_plain":
            steps[name] = lambda ex=ex, opt=opt, loss=loss: ex.train_step_graph(x, opt, loss=loss)
        elif name == "step_x_net":
            steps[name] = lambda ex=ex, opt=opt, loss=loss: ex.train_step_graph(x, opt, loss=loss, x_net=ours)
        else:
            steps[name] = lambda ex=ex, opt=opt, loss=loss: ex.train_step_graph(x, opt, loss=loss,
                                                                               x_net=cj(x, params, out=out))
    copy_dst = torch.empty_like(x)
    steps["copy_23MB"] = lambda: copy_dst.copy_(ours)
    sms = _summary(_windows(steps, args.repeats, args.steps, args.warmup))
    result["step"] = sms
    plain, aug, full = (sms[k]["median_ms"] for k in ("step_plain", "step_x_net", "step_x_net_with_jitter"))
    result["step_x_net_minus_plain_ms"] = round(aug - plain, 4)
    result["step_x_net_with_jitter_minus_plain_ms"] = round(full - plain, 4)
    result["expected_extra_ms_jitter_plus_copy"] = round(ksum["md2hip_color_jitter"]["median_ms"]
                                                         + sms["copy_23MB"]["median_ms"], 4)
    result["plain_step_spread_ms"] = round(sms["step_plain"]["max_ms"] - sms["step_plain"]["min_ms"], 4)
    result["plain_steps_per_s"] = round(1e3 / plain, 2)
    for item in args.bench_line:
        name, path = item.split("=", 1)
        with open(path) as f:
            lines = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
        result.setdefault("bench_py", {})[name] = {"ms_per_step": [ln["ms_per_step"] for ln in lines],
                                                   "images_per_s": [ln["value"] for ln in lines]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
