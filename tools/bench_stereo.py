"""Stereo-supervision timing at the bench configuration (ResNet-18, N = 12, 3 x 128 x 416, 4 scales).

(a) The loss tail alone (disparity sums, photometric pass, smoothness, upsample adjoint, reductions,
    so3) on fixed model-sized inputs: md2hip.loss_tail over the packed two-source kernel (the
    baseline), then over photo_sources_kernel with S = 2 (two learned sources: the same work as the
    baseline), S = 3 (MS) and S = 1 (S).  The photometric pass dominates the tail; the difference
    between the first two rows is the price of the scalar per-source form.
(b) The captured train step (train_step_graph) in M (the untouched path), MS and S.

Each repeat is a window of `--calls` back-to-back calls (`--steps` steps) between two device events;
the variants alternate window by window, and the reported time is the median over `--repeats` windows
after warm-up, with the minimum and maximum beside it.  Prints ONE JSON line:

    python tools/bench_stereo.py [--repeats 20] [--calls 20] [--steps 10] [--automask] > profiles/<tag>_stereo.json

--automask: Params(automasking=True) -- the tail rows and the step rows then also compute the
identity-reprojection mask over their sources.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, C, H, W = 12, 3, 128, 416
SCALES = (0.125, 0.25, 0.5, 1.0)


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
    ap.add_argument("--automask", action="store_true")
    args = ap.parse_args()

    import torch
    import md2hip
    from md2hip import _lib
    from md2hip import loss as L
    from md2hip.dist import synthetic_triplets

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x = synthetic_triplets(N, H, W, 0, dev)
    xs = synthetic_triplets(N, H, W, 1, dev)[:, 0].contiguous()
    Rt = torch.from_numpy(md2hip.stereo_transforms(["l", "r"] * (N // 2), [False, False, True, True] * (N // 4))).to(dev)
    K, invK = md2hip.depth10k_intrinsics(W, H)
    cache = md2hip.TrainCache(K=K, invK=invK, scales=SCALES)
    prm = md2hip.Params(target_size=(W, H), batch_size=N, automasking=args.automask, disparity_smoothness=1e-3)

    # (a) the loss tail on fixed inputs
    g = torch.Generator().manual_seed(11)
    disps = [(0.01 + 0.09 * torch.rand(N, 1, H >> s, W >> s, generator=g)).to(dev).contiguous() for s in (3, 2, 1, 0)]
    poses = [((0.01 * torch.randn(N, 3, generator=g)).to(dev),
              (torch.tensor([0.0, 0.0, sgn * 0.3]) + 0.05 * torch.randn(N, 3, generator=g)).to(dev)) for sgn in (-1, 1)]
    pose = md2hip.pack_poses(poses)
    fs = C * H * W
    two = (_lib.LossSource * _lib.MAX_SOURCES)()
    for s, sid in enumerate(cache.source_ids):
        two[s].frames, two[s].sample_stride = x.data_ptr() + 4 * (sid - 1) * fs, 3 * fs
        two[s].pose_block, two[s].invert = s, int(sid < cache.target_id)
    tail = {
        "packed_S2": lambda: md2hip.loss_tail(disps, poses, x, None, cache, prm),
        "sources_S2": lambda: L.run_loss_sources(disps, pose, x, x.data_ptr() + 4 * fs, 3 * fs, two, 2, 2, None,
                                                 cache, prm),
        "sources_S3_MS": lambda: md2hip.loss_tail(disps, poses, x, None, cache, prm, x_stereo=xs, stereo_Rt=Rt),
        "sources_S1_S": lambda: md2hip.loss_tail(disps, poses, x, None, cache, prm, x_stereo=xs, stereo_Rt=Rt,
                                                 temporal=False),
    }
    a, b = tail["packed_S2"](), tail["sources_S2"]()
    torch.cuda.synchronize()
    same = bool(torch.equal(a["loss"], b["loss"]) and torch.equal(a["d_pose"], b["d_pose"])
                and all(torch.equal(u, v) for u, v in zip(a["d_disp"], b["d_disp"])))
    tsum = _summary(_windows(tail, args.repeats, args.calls, args.warmup))
    result = {"tool": "bench_stereo", "device": torch.cuda.get_device_name(0), "batch": [N, 3, C, H, W],
              "scales": len(SCALES), "repeats": args.repeats, "calls_per_window": args.calls,
              "steps_per_window": args.steps, "loss_tail": tsum, "sources_S2_equals_packed_bits": same}
    if args.automask:
        result["automask"] = True
    base = tsum["packed_S2"]["median_ms"]
    result["loss_tail_over_packed"] = {k: round(v["median_ms"] / base, 3) for k, v in tsum.items()}

    # (b) the captured step: M (the untouched path), MS, S
    enc = md2hip.ResNet(18, in_channels=3)
    steps, keep = {}, []
    for name, kw in (("step_M", {}), ("step_MS", dict(x_stereo=xs, stereo_Rt=Rt)),
                     ("step_S", dict(x_stereo=xs, stereo_Rt=Rt, temporal=False))):
        m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]),
                         device=dev, seed=42)
        ex, opt, loss = m.executor(tuple(x.shape), cache, prm), md2hip.ADAM(1e-4), torch.empty(1, device=dev)
        keep.append((m, ex, opt, loss))
        steps[name] = lambda ex=ex, opt=opt, loss=loss, kw=kw: ex.train_step_graph(x, opt, loss=loss, **kw)
    sms = _summary(_windows(steps, args.repeats, args.steps, args.warmup))
    result["step"] = sms
    plain = sms["step_M"]["median_ms"]
    result["step_M_spread_ms"] = round(sms["step_M"]["max_ms"] - sms["step_M"]["min_ms"], 4)
    result["step_minus_M_ms"] = {k: round(v["median_ms"] - plain, 4) for k, v in sms.items()}
    result["final_losses"] = {k: float(l[3]) for k, l in zip(steps, keep)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
