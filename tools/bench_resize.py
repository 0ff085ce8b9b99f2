"""Frame-resize timing (md2_resize_frames), three measurements in one JSON:

1. The kernel alone.  36 gray frames 1241x376 and 36 RGB frames 1242x375 to 128x416 and to 192x640,
   both filters, against the composition a user would write on the device without it: per size
   group x.float().div(255), F.interpolate(bilinear, antialias=...), mul(255).round().div(255), a
   flip and a stack.  (The library had no device path before; torch's interpolate runs in float32
   and maps imresize's positions only when antialias=False, so the two agree to rounding, not bit
   for bit: the largest difference is reported.)  Windows of --calls calls between device events,
   the arms alternating, median and range over --repeats windows.  GB/s is over the bytes the call
   must move: the source bytes once and the output floats once.
2. The loader.  Triplets/s into HBM of DataLoader(KittyDataset) on synthetic PNGs of the real sizes
   (tools/loader_bench.py's content): gray resize="host" (md2_load_kitti_u8, the previous route),
   gray resize="device", colour image_2 resize="device" with both filters, and the decode alone
   (md2_load_frames_native_u8 into pinned memory), arms interleaved, --loader-rounds rounds.
3. The training step.  The captured step at B=12, 128x416 colour, alone and with the device loader
   producing its batches on the side stream.

    python tools/bench_resize.py [--repeats 15] [--calls 20] [--workers 16] > profiles/<tag>_resize.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monodepth2.jl_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

M = 36                                                                 # frames of a 12-triplet batch
KITTI_SIZES = [(376, 1241), (375, 1242), (370, 1226), (370, 1224), (374, 1238)]


def _windows(paths, repeats, calls, warmup):
    import torch
    for f in paths.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(repeats):                                           # alternating arms
        for k, f in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return ms


def _summary(ms):
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}


def torch_resize(frames, flips, H, W, antialias):
    """The device composition without the library: `frames` a list of uint8 [h][w][c] CUDA tensors."""
    import torch
    import torch.nn.functional as F
    out = [None] * len(frames)
    groups = {}
    for i, f in enumerate(frames):
        groups.setdefault(tuple(f.shape), []).append(i)
    for idx in groups.values():
        x = torch.stack([frames[i] for i in idx]).permute(0, 3, 1, 2).float().div(255.0)
        y = F.interpolate(x, size=(H, W), mode="bilinear", antialias=antialias, align_corners=False)
        y = y.mul(255.0).round().div(255.0)
        for j, i in enumerate(idx):
            out[i] = y[j].flip(-1) if flips[i] else y[j]
    return torch.stack(out)


def kernel_cases(args, result):
    import numpy as np
    import torch
    import md2hip
    rng = np.random.default_rng(0)
    flips = [(i // 3) % 2 for i in range(M)]
    rows = []
    for name, c, (h, w) in (("gray_1241x376", 1, (376, 1241)), ("rgb_1242x375", 3, (375, 1242))):
        imgs = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for _ in range(M)]
        slot = (h * w * c + 15) // 16 * 16 + 1                         # odd: the rows start at any byte
        buf = np.zeros(M * slot, dtype=np.uint8)
        offsets = np.arange(M, dtype=np.int64) * slot
        for o, im in zip(offsets, imgs):
            buf[o:o + im.size] = im.reshape(-1)
        src = torch.from_numpy(buf).cuda()
        frames = [torch.from_numpy(im).cuda() for im in imgs]
        sizes = np.array([(h, w)] * M)
        for H, W in ((128, 416), (192, 640)):
            out = torch.empty(M, c, H, W, dtype=torch.float32, device="cuda")
            for filter in ("imresize", "antialias"):
                ours = lambda: md2hip.resize_frames(src, offsets, sizes, H, W, channels=c, filter=filter,   # noqa: E731
                                                    quantize=True, flips=flips, out=out)
                theirs = lambda: torch_resize(frames, flips, H, W, filter == "antialias")                    # noqa: E731
                a, b = ours().clone(), theirs()
                torch.cuda.synchronize()
                diff = (a - b).abs()
                ms = _summary(_windows({"md2hip_resize_frames": ours, "torch_composition": theirs},
                                       args.repeats, args.calls, args.warmup))
                moved = M * h * w * c + out.numel() * 4
                t = ms["md2hip_resize_frames"]["median_ms"] * 1e-3
                rows.append({"case": name, "target": [H, W], "filter": filter, "call": ms,
                             "bytes_moved": moved, "GB_per_s": round(moved / t / 1e9, 1),
                             "torch_over_md2hip": round(ms["torch_composition"]["median_ms"]
                                                        / ms["md2hip_resize_frames"]["median_ms"], 2),
                             "max_abs_diff_to_torch": float(diff.max()),
                             "share_of_values_differing_from_torch": float((diff > 0).float().mean())})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    result["kernel"] = rows


def write_sequences(root, n_frames):
    import numpy as np
    from PIL import Image
    from loader_bench import natural
    rng = np.random.default_rng(0)
    seq = os.path.join(root, "sequences", "00")
    for cam in ("image_0", "image_2"):
        os.makedirs(os.path.join(seq, cam))
    with open(os.path.join(seq, "calib.txt"), "w") as f:
        f.write("P0: 7.188560e+02 0 6.071928e+02 0 0 7.188560e+02 1.852157e+02 0 0 0 1 0\n")
    distinct = 3 * len(KITTI_SIZES) * 3                                # 45 images per camera, then hard links
    for i in range(n_frames):
        h, w = KITTI_SIZES[(i // 3) % len(KITTI_SIZES)]
        for cam, c in (("image_0", 1), ("image_2", 3)):
            path = os.path.join(seq, cam, "%06d.png" % i)
            if i < distinct:
                Image.fromarray(natural(rng, h, w, c)).save(path)
            else:
                os.link(os.path.join(seq, cam, "%06d.png" % (i % distinct)), path)


def loader_rate(loader, batches):
    import torch
    it = iter(loader)
    next(it)                                                           # warm-up batch (thread pool start)
    torch.cuda.synchronize()
    t, n = time.perf_counter(), 0
    for x in it:
        n += x.shape[0]
        if n >= batches * x.shape[0]:
            break
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t)


def loader_cases(args, result, root):
    import torch
    import md2hip
    B, w = 12, args.workers
    kw = dict(target_size=(128, 416), augmentations=md2hip.FlipX(0.5))
    sets = {"gray_host": md2hip.KittyDataset(root, "00", **kw),
            "gray_device_imresize": md2hip.KittyDataset(root, "00", resize="device", **kw),
            "gray_device_antialias": md2hip.KittyDataset(root, "00", resize="device", filter="antialias", **kw),
            "colour_device_imresize": md2hip.KittyDataset(root, "00", camera="image_2", resize="device", **kw),
            "colour_device_antialias": md2hip.KittyDataset(root, "00", camera="image_2", resize="device",
                                                           filter="antialias", **kw)}
    nb = len(sets["gray_host"]) // B - 1
    rates = {k: [] for k in sets}
    decode = {"gray_decode_only": [], "colour_decode_only": []}
    pinned = {}
    for _ in range(args.loader_rounds):                                # arms interleaved
        for k, ds in sets.items():
            rates[k].append(loader_rate(md2hip.DataLoader(ds, B, workers=w, seed=1, device="cuda"), nb))
        for k, ds in (("gray_decode_only", sets["gray_device_imresize"]),
                      ("colour_decode_only", sets["colour_device_imresize"])):
            buf = pinned.setdefault(k, torch.empty(B * 3 * ds.slot_bytes, dtype=torch.uint8, pin_memory=True))
            t = time.perf_counter()
            for b in range(nb):
                ds.batch_native(list(range(b * B, (b + 1) * B)), seed=1, threads=w, out=buf)
            decode[k].append(nb * B / (time.perf_counter() - t))
    result["loader"] = {"batch": B, "workers": w, "batches_per_rate": nb, "cpu_quota": os.environ.get("OMP_NUM_THREADS"),
                        "triplets_per_s": {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                                               "max": round(max(v), 1)} for k, v in {**rates, **decode}.items()}}
    return sets["colour_device_antialias"]


def step_cases(args, result, ds):
    import torch
    import md2hip
    dev = torch.device("cuda", 0)
    N, H, W = 12, 128, 416
    enc = md2hip.ResNet(18, in_channels=3)
    model = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]),
                         device=dev, seed=42)
    cache = md2hip.TrainCache(K=ds.K, invK=ds.invK, scales=(0.125, 0.25, 0.5, 1.0))
    prm = md2hip.Params(target_size=(W, H), batch_size=N, automasking=False, disparity_smoothness=1e-3)
    ex, opt, loss = model.executor((N, 3, 3, H, W), cache, prm), md2hip.ADAM(1e-4), torch.empty(1, device=dev)
    x0 = next(iter(md2hip.DataLoader(ds, N, workers=args.workers, seed=1, device="cuda"))).contiguous()
    for _ in range(args.warmup):
        ex.train_step_graph(x0, opt, loss=loss)
    torch.cuda.synchronize()
    plain, fed = [], []
    for _ in range(args.step_rounds):                                  # alternating: plain, fed
        t = time.perf_counter()
        for _ in range(args.steps):
            ex.train_step_graph(x0, opt, loss=loss)
        torch.cuda.synchronize()
        plain.append((time.perf_counter() - t) / args.steps * 1e3)
        it = iter(md2hip.DataLoader(ds, N, workers=args.workers, seed=1, device="cuda"))
        next(it)                                                       # the prefetch queue fills
        torch.cuda.synchronize()
        t, n = time.perf_counter(), 0
        for x in it:
            ex.train_step_graph(x, opt, loss=loss)
            n += 1
            if n >= args.steps:
                break
        torch.cuda.synchronize()
        fed.append((time.perf_counter() - t) / n * 1e3)
        it.close()
    result["step"] = {"steps_per_window": args.steps, "loss_finite": bool(torch.isfinite(loss).all()),
                      "plain_ms": {"median": round(statistics.median(plain), 4), "min": round(min(plain), 4),
                                   "max": round(max(plain), 4)},
                      "fed_by_device_loader_ms": {"median": round(statistics.median(fed), 4), "min": round(min(fed), 4),
                                                  "max": round(max(fed), 4)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--loader-rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1080, help="synthetic frames per camera (45 distinct files)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma list of kernel,loader,step")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))

    import torch
    torch.cuda.set_device(0)
    result = {"tool": "bench_resize", "device": torch.cuda.get_device_name(0), "images_per_call": M,
              "repeats": args.repeats, "calls_per_window": args.calls}
    if "kernel" not in skip:
        kernel_cases(args, result)
    if "loader" not in skip or "step" not in skip:
        with tempfile.TemporaryDirectory() as d:
            write_sequences(d, args.frames)
            import md2hip
            ds = None
            if "loader" not in skip:
                ds = loader_cases(args, result, d)
            if "step" not in skip:
                ds = ds or md2hip.KittyDataset(d, "00", target_size=(128, 416), camera="image_2", resize="device",
                                               filter="antialias", augmentations=md2hip.FlipX(0.5))
                step_cases(args, result, ds)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
