"""Test-mode (BatchNorm on running statistics) references for tests/test_gpu_testmode.py.

The oracle enters through ``oracle.md2_oracle.batchnorm_train``, which ``resnet_stages`` looks up as
a module global: the tests patch that name (``pytest.MonkeyPatch``), oracle/ itself is untouched.
The oracle calls BatchNorm in the order stem, then per block bn1, bn2, (bn3,) down_bn -- the order
of the gamma entries of ``param_spec`` / ``md2_arch_param_info``, which is the layout of the flat
statistics vector (per BatchNorm C means, then C variances).

Bound (tests/_model_parity.py): every disparity level and the poses within
max(1e-6, 2 x floor) of the fp64 oracle, floor = the largest error against fp64 of four fp32
evaluations of the same test-mode function: the oracle in float32 on the CPU, the same with the
BatchNorms folded into the conv weights (w*s, bias t -- folding rounds s into every weight, which an
unfolded fp32 run does not), and both again through torch on the GPU with TF32 off."""
import json

import torch
import torch.nn.functional as F

from oracle import md2_oracle as O
from tests import _data as D
from tests._model_parity import FWD_ABS, FWD_FLOOR, parity_record_path

EPS = 1e-5


def bn_names(arch, C=3, levels=(2, 3, 4, 5)):
    """BatchNorm layer names in flat-statistics order, with their channel counts."""
    return [(n[:-len(".gamma")], s[0]) for n, s in O.param_spec(arch, C, tuple(levels)) if n.endswith(".gamma")]


def conv_of(bn):
    """The conv a BatchNorm follows: '<block>.bn<k>' -> '<block>.conv<k>', 'down_bn' -> 'down'."""
    if bn.endswith(".down_bn"):
        return bn[:-len("_bn")]
    head, tail = bn.rsplit(".", 1)
    return head + "." + tail.replace("bn", "conv")


def split_stats(flat, arch):
    """flat statistics vector -> [(mean [C], var [C])] per BatchNorm."""
    out, off = [], 0
    for _, c in bn_names(arch):
        out.append((flat[off:off + c], flat[off + c:off + 2 * c]))
        off += 2 * c
    assert off == flat.numel()
    return out


def join_stats(stats):
    return torch.cat([torch.cat([m.reshape(-1), v.reshape(-1)]) for m, v in stats])


def recording_bn(rec):
    """batchnorm_train that also records each call's batch mean and UNBIASED batch variance."""
    def bn(x, gamma, beta, eps=EPS):
        rec.append((x.mean((0, 2, 3)).detach(), x.var((0, 2, 3), unbiased=True).detach()))
        return F.batch_norm(x, None, None, gamma, beta, training=True, momentum=0.1, eps=eps)
    return bn


def queue_bn(stats, calls):
    """Test-mode BatchNorm: call k normalises with stats[k] = (mean, var)."""
    def bn(x, gamma, beta, eps=EPS):
        mu, var = stats[len(calls)]
        calls.append(tuple(x.shape))
        return F.batch_norm(x, mu.to(x), var.to(x), gamma, beta, training=False, eps=eps)
    return bn


def folded_bn(st, calls):
    """The folded realisation's 'BatchNorm': call k adds the shift t (the conv weights already
    carry s), except where s is kept (the stem, whose conv is not folded): x*s + t."""
    def bn(x, gamma, beta, eps=EPS):
        s, t = st[len(calls)]
        calls.append(tuple(x.shape))
        y = x if s is None else x * s.view(1, -1, 1, 1)
        return y + t.view(1, -1, 1, 1)
    return bn


def fold_params(P, stats, arch):
    """(P', [(s or None, t)]) in P's dtype: w' = w*s for every encoder conv but the stem."""
    P2, st = dict(P), []
    for (name, _), (mu, var) in zip(bn_names(arch), stats):
        g, b = P[name + ".gamma"], P[name + ".beta"]
        s = g / torch.sqrt(var.to(g) + EPS)
        t = b - mu.to(g) * s
        if name == "encoder.stem.bn":
            st.append((s, t))
        else:
            w = conv_of(name) + ".weight"
            P2[w] = P[w] * s.view(-1, 1, 1, 1)
            st.append((None, t))
    return P2, st


def oracle_forward(mp, flat, x, arch, dt, device="cpu", stats=None, folded=False, record=None):
    """O.model_forward (disparities, poses [2N, 6]) in dtype ``dt`` on ``device`` with
    batchnorm_train patched through ``mp`` (a pytest.MonkeyPatch): train mode (stats None;
    ``record`` collects the batch statistics), else test mode on ``stats`` -- unfolded or folded."""
    spec = O.param_spec(arch, x.shape[2])
    P = O.unflatten(flat.to(device=device, dtype=dt), spec)
    calls = []
    if stats is None:
        mp.setattr(O, "batchnorm_train", recording_bn(record if record is not None else []))
    elif folded:
        P, st = fold_params(P, [(m.to(device), v.to(device)) for m, v in stats], arch)
        mp.setattr(O, "batchnorm_train", folded_bn(st, calls))
    else:
        mp.setattr(O, "batchnorm_train", queue_bn(stats, calls))
    with torch.no_grad(), torch.device(device):
        disps, poses = O.model_forward(P, x.to(device=device, dtype=dt), arch=arch)
    if stats is not None:
        assert len(calls) == len(bn_names(arch)), (len(calls), len(bn_names(arch)))
    pose = torch.cat([torch.cat([r, t], 1) for r, t in poses], 0)
    return [d.double().cpu() for d in disps], pose.double().cpu()


def reference(mp, flat, x, stats, arch):
    """fp64 test-mode oracle outputs and the per-tensor floors / bounds."""
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    d64, p64 = oracle_forward(mp, flat, x, arch, torch.float64, stats=stats)
    names = [f"disp{i}" for i in range(len(d64))] + ["pose"]
    floor = dict.fromkeys(names, 0.0)
    per = {}
    for dev in ("cpu", "cuda"):
        for fold in (False, True):
            d32, p32 = oracle_forward(mp, flat, x, arch, torch.float32, dev, stats=stats, folded=fold)
            e = {f"disp{i}": D.rel_err(a, b) for i, (a, b) in enumerate(zip(d32, d64))}
            e["pose"] = D.rel_err(p32, p64)
            per[f"{dev}32{'_folded' if fold else ''}"] = e
            floor = {k: max(floor[k], e[k]) for k in names}
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    bound = {k: max(FWD_ABS, FWD_FLOOR * floor[k]) for k in names}
    return {"disps": d64, "pose": p64, "floor": floor, "bound": bound, "realisations": per}


def check(ref, disps, pose, label):
    """Record every tensor's (error, floor, bound) in parity_record_path("testmode_<label>"),
    print it, then assert error <= bound.  ``pose`` None: disparities only (eval_disparity)."""
    rec = {}
    for i, (a, b) in enumerate(zip(disps, ref["disps"])):
        rec[f"disp{i}"] = D.rel_err(a, b)
    if pose is not None:
        rec["pose"] = D.rel_err(pose, ref["pose"])
    out = {k: {"err": e, "floor": ref["floor"][k], "bound": ref["bound"][k]} for k, e in rec.items()}
    worst = max(v["err"] / v["bound"] for v in out.values())
    with open(parity_record_path("testmode_" + label), "w") as f:
        json.dump({"label": label, "tensors": out, "worst_err_over_bound": worst,
                   "realisations": ref["realisations"]}, f, indent=1)
    print(f"\ntestmode {label}: " + ", ".join(f"{k} {v['err']:.2e}/{v['bound']:.2e} (floor {v['floor']:.2e})"
                                              for k, v in out.items()))
    bad = {k: v for k, v in out.items() if v["err"] > v["bound"]}
    assert not bad, bad
    return out
