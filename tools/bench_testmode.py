"""Inference A/B: eval_disparity with BatchNorm in train mode (batch statistics; the only path
before test mode existed) against test mode (running statistics folded into the convs), interleaved
on one GPU.  ResNet-18, 416x128, B = 12 and B = 1; 3 x 60 calls of each after warm-up, as DESIGN's
A/Bs.  Prints ONE JSON line: images/s of both paths at both batch sizes and the per-kernel-family
HIP-event split (md2_model_set_profiling) of one call of each.

    python tools/bench_testmode.py [--rounds 3] [--calls 60] [--warmup 10] > profiles/<tag>_testmode.json

The event split brackets the convs, the disparity heads and test mode's two new passes; the
train-mode BatchNorm passes carry no bracket of their own (a statistics pass fused behind a conv is
inside that conv's bracket), so `unbracketed_ms` = wall time of an unprofiled call minus the
bracketed sum holds them, the decoder's upsampling and the launch gaps."""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W = 128, 416


def family(tag):
    m = re.match(r"fwd (\d)x\d/(\d)(r?) ", tag)
    if m:
        k, stride, reflect = m.groups()
        if k == "7":
            return "conv 7x7 stem"
        if reflect:
            return "conv 3x3 decoder (reflect)"
        return f"conv {k}x{k} encoder" + ("" if stride == "1" else " stride 2")
    return tag or "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()

    import torch
    import md2hip
    from md2hip._lib import check, lib, ptr, stream_of
    from md2hip.dist import synthetic_triplets

    torch.cuda.set_device(0)

    def make(testmode):
        enc = md2hip.ResNet(18, in_channels=3)
        m = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0), md2hip.PoseDecoder(512), seed=42)
        m.testmode(testmode)
        return m

    models = {"train_mode": make(False), "test_mode": make(True)}
    dptr = (C.c_void_p * 5)()
    result = {"tool": "bench_testmode", "arch": 18, "height": H, "width": W, "rounds": args.rounds,
              "calls": args.calls, "device": torch.cuda.get_device_name(0), "batch": {}}
    for B in (12, 1):
        x = synthetic_triplets(B, H, W, 0, "cuda")[:, 1].contiguous()
        exs = {k: m.eval_executor(B, H, W) for k, m in models.items()}
        st = stream_of(x.device)

        def call(k):
            check(lib().md2_model_eval_disparity(exs[k].handle, ptr(x), B, dptr, st), "md2_model_eval_disparity")

        for k in exs:
            for _ in range(args.warmup):
                call(k)
        torch.cuda.synchronize()
        ips = {k: [] for k in exs}
        for _ in range(args.rounds):               # interleaved: train, test, train, test, ...
            for k in exs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    call(k)
                b.record()
                b.synchronize()
                ips[k].append(args.calls * B / (a.elapsed_time(b) * 1e-3))
        rec = {}
        for k, ex in exs.items():
            best = max(ips[k])
            ex.set_profiling(True)
            call(k)
            torch.cuda.synchronize()
            fam = {}
            for tag, _cat, ms, _work in ex.profile_records():
                f = fam.setdefault(family(tag), {"ms": 0.0, "launches": 0})
                f["ms"] += ms
                f["launches"] += 1
            ex.set_profiling(False)
            wall = 1e3 * B / best
            bracketed = sum(f["ms"] for f in fam.values())
            rec[k] = {"images_per_s": [round(v, 1) for v in ips[k]], "images_per_s_best": round(best, 1),
                      "ms_per_call": round(wall, 4), "bracketed_ms": round(bracketed, 4),
                      "unbracketed_ms": round(wall - bracketed, 4),
                      "families": {n: {"ms": round(f["ms"], 4), "launches": f["launches"]}
                                   for n, f in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])}}
        rec["test_over_train"] = round(rec["test_mode"]["images_per_s_best"] /
                                       rec["train_mode"]["images_per_s_best"], 4)
        rec["test_mode_not_slower"] = rec["test_over_train"] >= 1.0
        result["batch"][str(B)] = rec
    print(json.dumps(result))


if __name__ == "__main__":
    main()
