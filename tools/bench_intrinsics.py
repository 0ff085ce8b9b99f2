"""Per-sample-intrinsics timing at the bench configuration (ResNet-18, N = 12, 3 x 128 x 416, 4 scales).

(a) The loss tail alone on fixed model-sized inputs: photo_sources_kernel with one K for the batch
    (md2_loss_fwd_bwd_sources) against its per-sample instances (md2_loss_fwd_bwd_sources_k) at
    S = 1 (S), 2 (M in the sources form) and 3 (MS), and the packed two-source kernel behind
    md2hip.loss_tail, which the plain step keeps.
(b) The captured train step (train_step_graph) in M, MS and S, without and with intrinsics.  M with
    intrinsics leaves the packed kernel for the S = 2 sources kernel; MS and S stay on their kernel.

Windows, alternation and medians as tools/bench_stereo.py.  With MD2HIP_LIB pointing at a library
from before this entry point existed, only the rows that library can run are measured -- run the
tool once per library, alternating, for an A/B of the untouched paths.  Prints ONE JSON line:

    python tools/bench_intrinsics.py [--repeats 20] [--calls 20] [--steps 10] > profiles/<tag>_intrinsics.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_stereo import C, H, N, SCALES, W, _summary, _windows  # noqa: E402


def sample_rows(K, dev):
    """(K, invK) float32 [N, 9]: the bench K with a per-sample focal scale and principal-point shift."""
    import numpy as np
    import torch
    Ks = np.repeat(np.asarray(K, dtype=np.float64)[None], N, 0)
    for i in range(N):
        s, d = (1.10, 0.92, 1.04, 1.0)[i % 4], (1.0, -1.0, 0.5, 0.0)[i % 4]
        Ks[i, 0, 0] *= s
        Ks[i, 1, 1] *= s * 1.03
        Ks[i, 0, 2] += d * W / 16.0
        Ks[i, 1, 2] -= d * H / 16.0
    return (torch.from_numpy(Ks.reshape(N, 9).astype(np.float32)).to(dev),
            torch.from_numpy(np.linalg.inv(Ks).reshape(N, 9).astype(np.float32)).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    import md2hip
    from md2hip import _lib
    from md2hip import loss as L
    from md2hip.dist import synthetic_triplets

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    have_k = hasattr(_lib.lib(), "md2_loss_fwd_bwd_sources_k")
    x = synthetic_triplets(N, H, W, 0, dev)
    xs = synthetic_triplets(N, H, W, 1, dev)[:, 0].contiguous()
    Rt = torch.from_numpy(md2hip.stereo_transforms(["l", "r"] * (N // 2), [False, False, True, True] * (N // 4))).to(dev)
    K, invK = md2hip.depth10k_intrinsics(W, H)
    cache = md2hip.TrainCache(K=K, invK=invK, scales=SCALES)
    prm = md2hip.Params(target_size=(W, H), batch_size=N, automasking=False, disparity_smoothness=1e-3)
    Kn, iKn = sample_rows(K, dev)

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
    ms_src, _, _ = L.stereo_sources(x, xs, Rt, cache, True)
    s_src, _, _ = L.stereo_sources(x, xs, Rt, cache, False)

    def run(src, nsrc, nl, **kw):
        return lambda: L.run_loss_sources(disps, pose if nl else None, x, x.data_ptr() + 4 * fs, 3 * fs, src, nsrc, nl,
                                          None, cache, prm, **kw)
    tail = {"packed_S2": lambda: md2hip.loss_tail(disps, poses, x, None, cache, prm),
            "uniform_S1": run(s_src, 1, 0), "uniform_S2": run(two, 2, 2), "uniform_S3": run(ms_src, 3, 2)}
    if have_k:
        kk = dict(K=Kn, invK=iKn)
        tail.update({"per_sample_S1": run(s_src, 1, 0, **kk), "per_sample_S2": run(two, 2, 2, **kk),
                     "per_sample_S3": run(ms_src, 3, 2, **kk)})
    tsum = _summary(_windows(tail, args.repeats, args.calls, args.warmup))
    result = {"tool": "bench_intrinsics", "lib": os.environ.get("MD2HIP_LIB", "default"),
              "device": torch.cuda.get_device_name(0), "batch": [N, 3, C, H, W], "scales": len(SCALES),
              "repeats": args.repeats, "calls_per_window": args.calls, "steps_per_window": args.steps,
              "loss_tail": tsum}
    if have_k:
        result["per_sample_over_uniform"] = {f"S{s}": round(tsum[f"per_sample_S{s}"]["median_ms"]
                                                            / tsum[f"uniform_S{s}"]["median_ms"], 3) for s in (1, 2, 3)}
        result["per_sample_S2_over_packed"] = round(tsum["per_sample_S2"]["median_ms"] / tsum["packed_S2"]["median_ms"], 3)

    enc = md2hip.ResNet(18, in_channels=3)
    steps, keep = {}, []
    modes = (("M", {}), ("MS", dict(x_stereo=xs, stereo_Rt=Rt)), ("S", dict(x_stereo=xs, stereo_Rt=Rt, temporal=False)))
    for name, kw in modes:
        for tag, extra in (("", {}), ("_K", dict(K=Kn, invK=iKn))):
            if tag and not have_k:
                continue
            m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                      embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]),
                             device=dev, seed=42)
            ex, opt, loss = m.executor(tuple(x.shape), cache, prm), md2hip.ADAM(1e-4), torch.empty(1, device=dev)
            keep.append((m, ex, opt, loss))
            kw2 = dict(kw, **extra)
            steps[f"step_{name}{tag}"] = lambda ex=ex, opt=opt, loss=loss, kw2=kw2: ex.train_step_graph(
                x, opt, loss=loss, **kw2)
    sms = _summary(_windows(steps, args.repeats, args.steps, args.warmup))
    result["step"] = sms
    if have_k:
        result["step_K_minus_plain_ms"] = {n: round(sms[f"step_{n}_K"]["median_ms"] - sms[f"step_{n}"]["median_ms"], 4)
                                           for n, _ in modes}
    result["final_losses"] = {k: float(l[3]) for k, l in zip(steps, keep)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
