"""Odometry-evaluation timing, two measurements.  The parent of this feature has neither path, so each
is set against what a user would write without it.

(a) md2hip.pose_errors on M = 1590 synthetic steps in one sequence (the size of KITTI odometry
    sequence 09), track_length 5, against
      torch_composition    the same arithmetic as batched torch ops on the device (so3 in fp32, the
                           chains by bmm over all snippets at once, no synchronisation);
      host_numpy_download  the poses downloaded (a synchronise), then the float32 NumPy restatement
                           of tests/_pose_ref.py.
    1590 steps are 1587 threads of work: expect the device figures to be launch / enqueue latency,
    not throughput.

(b) pairs per second of md2hip.eval_pose (25 consecutive frames per call = 24 pairs, each frame
    encoded once, no DepthDecoder) against the same 24 poses from the model's forward on 12 triplets
    that advance by two frames (frames 2i, 2i+1, 2i+2: every pair once, every second frame encoded
    twice, plus a DepthDecoder nobody reads) -- the cheapest way md2_model_forward gives them; triplets
    that advance by one frame cost twice that.  ResNet-18, batch 12, 128x416, test mode.

Each repeat is a window of back-to-back calls between two device events (the host route: the host
clock around work that ends synchronised); the paths alternate, and the reported time per call is
the median over `--repeats` windows after warm-up.  Prints ONE JSON line:

    python tools/bench_pose_eval.py [--repeats 10] [--calls 200] [--model-calls 20] > profiles/<tag>_pose_eval.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

M, L = 1590, 5
N, H, W = 12, 128, 416


def torch_pose_errors(pred, gt_rel, L, invert=True):
    """(per_snippet [S, 3], summary [4]) with batched torch ops, fp32, on pred's device."""
    import torch
    r, t = pred[:, :3], pred[:, 3:]
    m = pred.shape[0]
    z = torch.zeros(m, device=pred.device)
    S = torch.stack([z, -r[:, 2], r[:, 1], r[:, 2], z, -r[:, 0], -r[:, 1], r[:, 0], z], 1).view(m, 3, 3)
    th = r.norm(dim=1)
    thi = 1.0 / th.clamp_min(1e-4)
    R = torch.eye(3, device=pred.device) + (thi * th.sin())[:, None, None] * S \
        + (thi * thi * (1 - th.cos()))[:, None, None] * (S @ S)
    if invert:
        R = R.transpose(1, 2)
        t = -(R @ t[:, :, None])[:, :, 0]
    Rg, tg = gt_rel[:, :9].view(m, 3, 3), gt_rel[:, 9:]
    n = m - L + 2

    def chain(R, t):
        C, p, pos = R[0:n], t[0:n], [t[0:n]]
        for j in range(1, L - 1):
            p = (C @ t[j:j + n, :, None])[:, :, 0] + p
            C = C @ R[j:j + n]
            pos.append(p)
        return torch.stack(pos, 1), C                     # [n, L-1, 3] (p_0 = 0 left out)
    p, Cp = chain(R, t)
    q, Cq = chain(Rg, tg)
    num, den = (q * p).sum((1, 2)), (p * p).sum((1, 2))
    scale = torch.where(den > 0, num / den, torch.zeros_like(den))
    ate = ((p * scale[:, None, None] - q) ** 2).sum((1, 2)).sqrt() / L
    chord = ((Cp - Cq) ** 2).sum((1, 2)).sqrt()
    out = torch.stack([ate, scale, chord], 1)
    ok = torch.isfinite(out).all(1)
    o = out[ok].double()
    return out, torch.stack([o[:, 0].mean(), o[:, 0].std(unbiased=False), o[:, 1].mean(), o[:, 2].mean()]).float()


def windows(paths, repeats, warmup):
    """{name: [ms per call]} over `repeats` alternating windows; a path is (fn, calls, host_timed)."""
    import torch
    for f, calls, _ in paths.values():
        for _ in range(warmup if calls > 1 else 1):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(repeats):
        for k, (f, calls, host) in paths.items():
            if host:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    f()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return ms


def stats(ms):
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--model-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    import md2hip
    from tests import _data as D
    from tests import _pose_ref as R

    torch.cuda.set_device(0)
    # ---- (a) the metric
    pred_h, gt_h = R.make_case(0, M, invert=True)
    pred, gt = torch.from_numpy(pred_h).cuda(), torch.from_numpy(gt_h).cuda()

    def host_route():
        ph = pred.cpu().numpy()                             # the download is the synchronise
        rt = R.so3_compose_ref(ph, True, dtype=np.float32)
        return R.pose_eval_ref(rt, gt_h, [0, M], L)
    paths = {"md2hip_pose_errors": (lambda: md2hip.pose_errors(pred, gt, track_length=L), args.calls, False),
             "torch_composition": (lambda: torch_pose_errors(pred, gt, L), max(1, args.calls // 10), False),
             "host_numpy_download": (host_route, 1, True)}
    ours = md2hip.pose_errors(pred, gt, track_length=L)
    theirs = torch_pose_errors(pred, gt, L)
    host = host_route()
    torch.cuda.synchronize()
    o = ours[0].cpu().numpy()
    agree = {"torch_composition_max_rel_diff": float(np.abs(theirs[0].cpu().numpy() / o - 1).max()),
             "host_numpy_max_rel_diff": float(np.abs(host[0] / o - 1).max()),
             "summary": [float(v) for v in ours[1].cpu().numpy()[0]]}
    ms_a = windows(paths, args.repeats, args.warmup)
    med_a = {k: statistics.median(v) for k, v in ms_a.items()}

    # ---- (b) the poses
    enc = md2hip.ResNet(18, in_channels=3)
    model = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]), seed=42)
    K, invK = md2hip.depth10k_intrinsics(W, H)
    cache = md2hip.TrainCache(K=K, invK=invK)
    params = md2hip.Params(target_size=(W, H), batch_size=N, automasking=False)
    seq = D.triplets(9, 3, H, W, seed=5).float().reshape(27, 3, H, W)[:2 * N + 1].cuda().contiguous()
    trip = torch.stack([seq[2 * i:2 * i + 3] for i in range(N)]).contiguous()       # [N, 3, C, H, W]
    ex = model.executor(tuple(trip.shape), cache, params)
    md2hip.train_loss(model, trip, None, cache, params)     # one train forward: statistics worth folding
    md2hip.gradient(model)
    model.testmode(True)
    pairs = 2 * N

    def triplet_route():
        ex.forward(trip)
        return ex.outputs()[1]
    pose_t = triplet_route().clone()                       # rows i: pair (2i, 2i+1); rows N + i: (2i+1, 2i+2)
    pose_e = md2hip.eval_pose(model, seq)
    torch.cuda.synchronize()
    order = torch.stack([pose_t[:N], pose_t[N:]], 1).reshape(pairs, 6)
    paths = {"md2hip_eval_pose": (lambda: md2hip.eval_pose(model, seq), args.model_calls, False),
             "forward_on_triplets": (triplet_route, args.model_calls, False)}
    ms_b = windows(paths, args.repeats, args.warmup)
    med_b = {k: statistics.median(v) for k, v in ms_b.items()}

    print(json.dumps({
        "tool": "bench_pose_eval", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
        "metric": {"steps": M, "track_length": L, "snippets": M - L + 2,
                   "calls_per_repeat": {"md2hip_pose_errors": args.calls,
                                        "torch_composition": max(1, args.calls // 10), "host_numpy_download": 1},
                   "ms_per_call": stats(ms_a),
                   "torch_over_md2hip": round(med_a["torch_composition"] / med_a["md2hip_pose_errors"], 2),
                   "host_over_md2hip": round(med_a["host_numpy_download"] / med_a["md2hip_pose_errors"], 2),
                   "agreement": agree},
        "poses": {"arch": 18, "batch": N, "size": [H, W], "testmode": True, "pairs_per_call": pairs,
                  "frames_encoded_per_call": {"md2hip_eval_pose": pairs + 1, "forward_on_triplets": 3 * N},
                  "calls_per_repeat": args.model_calls, "ms_per_call": stats(ms_b),
                  "pairs_per_s": {k: round(pairs / v * 1e3, 1) for k, v in med_b.items()},
                  "eval_pose_over_triplets": round(med_b["forward_on_triplets"] / med_b["md2hip_eval_pose"], 3),
                  "max_rel_diff_of_the_poses": float(((pose_e - order).norm() / order.norm()).item())}}))


if __name__ == "__main__":
    main()
