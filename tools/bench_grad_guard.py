"""Gradient-guard timing at the bench configuration (ResNet-18, N = 12, 128x416, no automask).

(a) The primitive: md2hip.grad_norm (md2_grad_norm: the sum-of-squares pass and its finishing launch)
    on the model's flat gradient, against what a user would otherwise write on the device --
    torch.linalg.vector_norm(g) and torch.isfinite(g).all().  The pass must read the gradient once:
    4 * numel(g) bytes, the figure the GB/s is over.
(b) The captured train step (train_step_graph): plain, guarded with max_norm = inf, guarded with
    clipping.  The overhead is to be read against the plain step's own window spread and against the
    primitive's time from (a).

Each repeat is a window of `--calls` back-to-back calls (`--steps` steps) between two device events;
the variants alternate window by window, and the reported time is the median over `--repeats` windows
after warm-up, with the minimum and maximum beside it.  Prints ONE JSON line:

    python tools/bench_grad_guard.py [--repeats 20] [--calls 20] [--steps 10] [--cold]
           [--bench-line parent=FILE --bench-line this=FILE] > profiles/<tag>_grad_guard.json

The gradient (about 60 MB) stays below the 256 MiB Infinity Cache, so in a loop that re-reads it the
achieved bytes per second is a cache-resident figure, not an HBM one -- as it is in the step, where
the backward has just written it; `--cold` interleaves a 512 MiB fill between calls (timed separately
and subtracted) to show the other end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, H, W = 12, 128, 416


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

    import torch
    import md2hip
    from md2hip.dist import synthetic_triplets
    from md2hip._lib import lib

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x = synthetic_triplets(N, H, W, 0, dev)
    enc = md2hip.ResNet(18, in_channels=3)
    K, invK = md2hip.depth10k_intrinsics(W, H)
    cache = md2hip.TrainCache(K=K, invK=invK, scales=(0.125, 0.25, 0.5, 1.0))
    prm = md2hip.Params(target_size=(W, H), batch_size=N, automasking=False, disparity_smoothness=1e-3)

    def new_model():
        return md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                     embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]),
                            device=dev, seed=42)

    # (a) the primitive on the gradient of one step
    model = new_model()
    md2hip.train_step(model, x, None, cache, prm, md2hip.ADAM(1e-4))
    g = model.grad
    n = g.numel()
    state = torch.zeros(40, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib().md2_grad_norm_workspace_size(n), dtype=torch.uint8, device=dev)
    ours = md2hip.decode_guard_state(md2hip.grad_norm(g, state=state, workspace=ws))
    theirs = float(torch.linalg.vector_norm(g))
    finite = bool(torch.isfinite(g).all())

    def torch_pair():
        return torch.linalg.vector_norm(g), torch.isfinite(g).all()

    kernel_paths = {"md2hip_grad_norm": lambda: md2hip.grad_norm(g, state=state, workspace=ws),
                    "torch_vector_norm_and_isfinite": torch_pair}
    ksum = _summary(_windows(kernel_paths, args.repeats, args.calls, args.warmup))
    nbytes = 4 * n
    t_ours = ksum["md2hip_grad_norm"]["median_ms"] * 1e-3
    result = {
        "tool": "bench_grad_guard", "device": torch.cuda.get_device_name(0), "batch": [N, 3, 3, H, W],
        "gradient_elements": n, "bytes_read": nbytes,
        "repeats": args.repeats, "calls_per_window": args.calls, "steps_per_window": args.steps,
        "norm_md2hip": ours["norm"], "norm_torch": theirs, "all_finite": [ours["ok"], finite],
        "call": ksum,
        "torch_over_md2hip": round(ksum["torch_vector_norm_and_isfinite"]["median_ms"]
                                   / ksum["md2hip_grad_norm"]["median_ms"], 2),
        "achieved_GB_per_s_cache_resident": round(nbytes / t_ours / 1e9, 1),
        "gradient_sits_in_infinity_cache": True,
    }

    if args.cold:
        big = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        cold = {"fill_then_grad_norm": lambda: (big.fill_(1), md2hip.grad_norm(g, state=state, workspace=ws)),
                "fill_alone": lambda: big.fill_(1)}
        cms = _summary(_windows(cold, args.repeats, args.calls, args.warmup))
        t_cold = (cms["fill_then_grad_norm"]["median_ms"] - cms["fill_alone"]["median_ms"]) * 1e-3
        result["cold"] = cms
        result["cold_call_ms"] = round(t_cold * 1e3, 4)
        result["achieved_GB_per_s_after_eviction"] = round(nbytes / t_cold / 1e9, 1) if t_cold > 0 else None

    # (b) the captured step: plain, guarded without clipping, guarded with clipping
    half = 0.5 * ours["norm"]
    steps, keep = {}, []
    for name, kw in (("step_plain", {}), ("step_guard_inf", {"skip_nonfinite": True}),
                     ("step_guard_clip", {"max_grad_norm": half})):
        m = new_model()
        ex, opt, loss = m.executor(tuple(x.shape), cache, prm), md2hip.ADAM(1e-4, **kw), torch.empty(1, device=dev)
        keep.append((m, ex, opt, loss))
        steps[name] = lambda ex=ex, opt=opt, loss=loss: ex.train_step_graph(x, opt, loss=loss)
    sms = _summary(_windows(steps, args.repeats, args.steps, args.warmup))
    result["step"] = sms
    result["guard_state_after"] = {k[5:]: o.guard_state() for k, (_, _, o, _) in zip(steps, keep) if o.guarded}
    plain = sms["step_plain"]["median_ms"]
    result["step_guard_inf_minus_plain_ms"] = round(sms["step_guard_inf"]["median_ms"] - plain, 4)
    result["step_guard_clip_minus_plain_ms"] = round(sms["step_guard_clip"]["median_ms"] - plain, 4)
    result["expected_extra_ms_grad_norm"] = ksum["md2hip_grad_norm"]["median_ms"]
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
