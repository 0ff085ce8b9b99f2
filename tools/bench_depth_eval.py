"""Depth evaluation timing: one batched md2hip.depth_errors call against the torch composition a
user would write without it (F.interpolate(align_corners=False), boolean indexing, torch.median per
image and the seven reductions), on the same device and the same inputs.  N = 12, 128x416 ->
375x1242, Garg crop, median scaling.  The parent of this feature has no such path, so the torch
composition is the yardstick.

Each repeat is a window of `--calls` back-to-back evaluations between two device events (the torch
composition syncs inside itself, at every boolean index); the two paths alternate, and the reported
time per evaluation is the median over `--repeats` windows after warm-up.  Prints ONE JSON line:

    python tools/bench_depth_eval.py [--repeats 20] [--calls 10] [--warmup 5] > profiles/<tag>_depth_eval.json

The outputs of the two paths are compared first and the largest relative difference is reported
(fp32 rounding, and torch.median's lower-middle element for an even count)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, H, W, HG, WG = 12, 128, 416, 375, 1242


def torch_depth_errors(disp, gt, crop, min_depth=0.1, max_depth=100.0, eval_min=1e-3, eval_max=80.0):
    """The straightforward per-image torch pipeline; returns [N, 8] (seven metrics and the ratio)."""
    import torch
    import torch.nn.functional as F
    y0, y1, x0, x1 = crop
    sd = disp * (1.0 / min_depth - 1.0 / max_depth) + 1.0 / max_depth
    pred = 1.0 / F.interpolate(sd[:, None], size=gt.shape[1:], mode="bilinear", align_corners=False)[:, 0]
    box = torch.zeros_like(gt[0], dtype=torch.bool)
    box[y0:y1, x0:x1] = True
    rows = []
    for i in range(disp.shape[0]):
        mask = (gt[i] > eval_min) & (gt[i] < eval_max) & box
        g, p = gt[i][mask], pred[i][mask]
        # torch.median returns the LOWER middle element of an even count (NumPy and the library
        # average the two): the cheapest form, and the paths then agree to ~1e-5 only
        ratio = g.median() / p.median()
        p = (p * ratio).clamp(eval_min, eval_max)
        t = torch.maximum(g / p, p / g)
        d = g - p
        rows.append(torch.stack([(d.abs() / g).mean(), (d * d / g).mean(), (d * d).mean().sqrt(),
                                 ((g.log() - p.log()) ** 2).mean().sqrt(), (t < 1.25).float().mean(),
                                 (t < 1.25 ** 2).float().mean(), (t < 1.25 ** 3).float().mean(), ratio]))
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    import md2hip
    from tests import _depth_eval_ref as R

    torch.cuda.set_device(0)
    disp_h, gt_h = R.make_case(0, N, H, W, HG, WG)
    disp, gt = torch.from_numpy(disp_h).cuda(), torch.from_numpy(gt_h).cuda()
    crop = md2hip.garg_crop(HG, WG)

    paths = {"md2hip_depth_errors": lambda: md2hip.depth_errors(disp, gt)[0],
             "torch_composition": lambda: torch_depth_errors(disp, gt, crop)}
    ours, theirs = (f()[:, :8] for f in paths.values())
    torch.cuda.synchronize()
    agree = float(((ours - theirs).abs() / theirs.abs().clamp_min(1e-30)).max())

    for f in paths.values():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):                      # alternating: ours, torch, ours, torch, ...
        for k, f in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / args.calls)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "tool": "bench_depth_eval", "device": torch.cuda.get_device_name(0), "images": N,
        "disp": [H, W], "gt": [HG, WG], "crop": list(crop), "repeats": args.repeats, "calls_per_repeat": args.calls,
        "ms_per_call": {k: round(v, 4) for k, v in med.items()},
        "ms_per_call_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "torch_over_md2hip": round(med["torch_composition"] / med["md2hip_depth_errors"], 2),
        "max_rel_diff_between_paths": agree}))


if __name__ == "__main__":
    main()
