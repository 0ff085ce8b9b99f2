"""Bit-identity digest of the bench train step: `steps` full steps (forward + loss + backward +
ADAM) at B, 416x128 on the bench's synthetic batch, then SHA-256 of the loss, the flat
parameters, the flat gradient and the BatchNorm running statistics.  Run it once per library
(MD2HIP_LIB=...) to show that a kernel change only regroups work (same digest) or to see that it
re-rounds (different digest).

    python tools/step_digest.py [B] [steps] [--height H] [--width W] [--graph] [--guard MAXNORM]
                                [--automask] [--stereo MS|S]

--graph runs the captured step (train_step_graph) instead of the eager one; --guard MAXNORM uses a
guarded optimiser (ADAM(max_grad_norm=MAXNORM)) and also prints its guard_state() after the last
step; --automask sets Params(automasking=True), so the model computes the identity-reprojection
mask itself; --stereo MS|S adds a seeded stereo frame with stereo_transforms (as
tools/bench_stereo.py builds them), beside the temporal sources (MS) or alone (S)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "monodepth2.jl_amd")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("B", nargs="?", type=int, default=12)
    ap.add_argument("steps", nargs="?", type=int, default=3)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--guard", type=float, default=None, metavar="MAXNORM")
    ap.add_argument("--automask", action="store_true")
    ap.add_argument("--stereo", choices=("MS", "S"), default=None)
    a = ap.parse_args()
    B, steps, H, W = a.B, a.steps, a.height, a.width
    import torch
    import md2hip
    import md2hip.dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    enc = md2hip.ResNet(18, in_channels=3)
    model = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0),
                         md2hip.PoseDecoder(512), device=dev, seed=42)
    K, invK = md2hip.depth10k_intrinsics(W, H)
    cache = md2hip.TrainCache(K=K, invK=invK, scales=(0.125, 0.25, 0.5, 1.0))
    params = md2hip.Params(target_size=(W, H), batch_size=B, automasking=a.automask, disparity_smoothness=1e-3)
    opt = md2hip.ADAM(1e-4) if a.guard is None else md2hip.ADAM(1e-4, max_grad_norm=a.guard)
    x = md2hip.dist.synthetic_triplets(B, H, W, 0, dev)
    stereo = {}
    if a.stereo:
        sides, flips = ["l", "r"] * B, [False, False, True, True] * B
        stereo = dict(x_stereo=md2hip.dist.synthetic_triplets(B, H, W, 1, dev)[:, 0].contiguous(),
                      stereo_Rt=torch.from_numpy(md2hip.stereo_transforms(sides[:B], flips[:B])).to(dev),
                      temporal=a.stereo == "MS")
    ex = model.executor(tuple(x.shape), cache, params)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    losses = []
    for _ in range(steps):
        if a.graph:
            ex.train_step_graph(x, opt, loss=loss, **stereo)
        else:
            md2hip.dist.train_step(ex, model, opt, x, loss=loss, **stereo)
        torch.cuda.synchronize()
        losses.append(loss.item())

    def h(t):
        return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]
    out = {"lib": os.environ.get("MD2HIP_LIB", "default"), "B": B, "steps": steps,
           "losses": losses, "params": h(model.flat), "grad": h(model.grad), "bn_stats": h(model.bn_stats())}
    if (H, W) != (128, 416):
        out["height"], out["width"] = H, W
    if a.graph:
        out["graph"] = True
    if a.automask:
        out["automask"] = True
    if a.stereo:
        out["stereo"] = a.stereo
    if a.guard is not None:
        out["guard"] = a.guard
        out["guard_state"] = opt.guard_state()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
