"""LiDAR depth-map timing: one batched md2hip.lidar_depth call against the two routes a user has
without it, on the same 12 synthetic scans of 120 k points rasterised into 375x1242
(tests/_lidar_ref.py's generator and calibration).  The parent of this feature has no such path, so
there are two yardsticks:

  host_numpy_upload   the float32 NumPy restatement on the host (project, round, np.minimum.at per
                      scan) plus the upload of the 12 maps -- the route a user takes today;
  torch_composition   the same arithmetic in torch on the device, one scan at a time, the minimum by
                      scatter_reduce_(..., "amin"); dropped points go to a spare slot, so it never
                      synchronises.

The device paths start from points already in device memory, the host route from points in host
memory (where np.fromfile leaves them); `points_upload_ms` is what the device paths add when the
scans come from disk (23 MB against the 22 MB of maps the host route uploads).

Each repeat is a window of back-to-back calls: `--calls` for md2hip, a twentieth of that for the
torch composition (between two device events), one for the host route (host clock around work that
ends in a device synchronise).  The three paths alternate, and the reported time per call is the
median over `--repeats` windows after warm-up.  Prints ONE JSON line:

    python tools/bench_lidar_depth.py [--repeats 10] [--calls 200] [--warmup 3] > profiles/<tag>_lidar_depth.json

The outputs of the three paths are compared first: the number of pixels whose bits differ and the
largest absolute difference are reported."""
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

N, M, H, W = 12, 120000, 375, 1242


def torch_lidar_depth(scans, Pd, h, w):
    """The per-scan torch pipeline: [N, h, w], the operations of include/md2.h in their order."""
    import torch
    out = []
    inf = torch.tensor(float("inf"), device=scans[0].device)
    for pts, p in zip(scans, Pd):
        X, Y, Z = pts[:, 0], pts[:, 1], pts[:, 2]
        x = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3]
        y = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7]
        zc = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11]
        ru, rv = torch.round(x / zc), torch.round(y / zc)            # ties to even, as rintf
        keep = (X >= 0) & torch.isfinite(zc) & (zc > 0) & (ru >= 1) & (ru <= w) & (rv >= 1) & (rv <= h)
        idx = torch.where(keep, (rv - 1) * w + (ru - 1), float(h * w)).long()      # spare slot h*w
        flat = torch.full((h * w + 1,), float("inf"), device=pts.device)
        flat.scatter_reduce_(0, idx, torch.where(keep, zc, inf), "amin", include_self=True)
        flat = flat[:h * w]
        out.append(torch.where(torch.isinf(flat), 0.0, flat).view(h, w))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import md2hip
    from tests import _lidar_ref as R

    torch.cuda.set_device(0)
    points_h, offsets = R.make_scans(0, [M] * N)
    P = R.calib(H, W)
    points = torch.from_numpy(points_h).cuda()
    scans = [points[offsets[i]:offsets[i + 1]] for i in range(N)]
    Pd = [torch.from_numpy(P.reshape(12)).cuda() for _ in range(N)]

    def host_route():
        d, _ = R.lidar_depth_ref(points_h, offsets, P, H, W)
        return torch.from_numpy(d).cuda()

    paths = {"md2hip_lidar_depth": (lambda: md2hip.lidar_depth((points, offsets), P, H, W), args.calls),
             "torch_composition": (lambda: torch_lidar_depth(scans, Pd, H, W), max(1, args.calls // 20)),
             "host_numpy_upload": (host_route, 1)}
    outs = {k: f().view(torch.int32) for k, (f, _) in paths.items()}
    torch.cuda.synchronize()
    ours = outs["md2hip_lidar_depth"]
    agree = {}
    for k in ("torch_composition", "host_numpy_upload"):
        diff = ours != outs[k]
        agree[k] = {"pixels_differing": int(diff.sum()),
                    "max_abs_diff": float((ours.view(torch.float32) - outs[k].view(torch.float32)).abs().max())}
    hit = int((ours != 0).sum())

    for f, calls in paths.values():
        for _ in range(args.warmup if calls > 1 else 1):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.repeats):                      # alternating: ours, torch, host, ours, ...
        for k, (f, calls) in paths.items():
            if k == "host_numpy_upload":
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    up = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.from_numpy(points_h).cuda()
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "tool": "bench_lidar_depth", "device": torch.cuda.get_device_name(0), "scans": N, "points_per_scan": M,
        "depth": [H, W], "pixels_hit": hit, "repeats": args.repeats,
        "calls_per_repeat": {k: c for k, (_, c) in paths.items()},
        "ms_per_call": {k: round(v, 4) for k, v in med.items()},
        "ms_per_call_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "torch_over_md2hip": round(med["torch_composition"] / med["md2hip_lidar_depth"], 2),
        "host_over_md2hip": round(med["host_numpy_upload"] / med["md2hip_lidar_depth"], 2),
        "points_upload_ms": round(statistics.median(up), 4),
        "difference_from_md2hip": agree}))


if __name__ == "__main__":
    main()
