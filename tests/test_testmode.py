"""CPU: the BatchNorm running statistics as model state -- layout queries, the oracle's BatchNorm
call order against the parameter table, and the checkpoint round trip on device="cpu" models."""
import ctypes as C
import json

import pytest
import torch

from oracle import md2_oracle as O
from tests import _testmode as T


def _model(arch=18, levels=(2, 3, 4, 5), seed=42):
    import md2hip
    enc = md2hip.ResNet(arch, in_channels=3)
    return md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=list(levels),
                                                 embedding_levels=0),
                        md2hip.PoseDecoder(enc.stages[-1]), device="cpu", seed=seed)


def _random_stats(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(model.bn_numel, generator=g)
    off = 0
    for c in model.bn_channels:
        v[off + c:off + 2 * c] = v[off + c:off + 2 * c].abs()
        off += 2 * c
    return v


@pytest.mark.parametrize("arch", [18, 34, 50])
def test_bn_stat_count_matches_param_spec(arch):
    from md2hip._lib import lib
    from md2hip.model import _cfg
    cfg = _cfg(arch, 3, (2, 3, 4, 5))
    nb, ne = C.c_longlong(), C.c_longlong()
    assert lib().md2_arch_bn_stat_count(C.byref(cfg), C.byref(nb), C.byref(ne)) == 0
    chans = [s[0] for n, s in O.param_spec(arch, 3) if n.endswith(".gamma")]
    assert (nb.value, ne.value) == (len(chans), 2 * sum(chans))
    model = _model(arch)
    assert model.bn_channels == chans and model.bn_numel == ne.value


@pytest.mark.parametrize("arch", [18, 50])
def test_oracle_bn_call_order_is_the_gamma_order(arch, monkeypatch):
    """The oracle calls BatchNorm stem, then per block bn1, bn2, (bn3,) down_bn: the order of the
    gamma entries of md2_arch_param_info, i.e. of the flat statistics vector."""
    import md2hip
    table, _ = md2hip.param_table(arch, 3, (2, 3, 4, 5))
    want = [n[:-len(".gamma")] for n, _, _ in table if n.endswith(".gamma")]
    assert want == [n for n, _ in T.bn_names(arch)]
    spec = O.param_spec(arch, 3)
    flat = O.init_params(spec, dtype=torch.float32)
    P = O.unflatten(flat, spec)
    by_ptr = {v.data_ptr(): k[:-len(".gamma")] for k, v in P.items() if k.endswith(".gamma")}
    seen = []

    def bn(x, gamma, beta, eps=1e-5):
        seen.append(by_ptr[gamma.data_ptr()])
        return O.F.batch_norm(x, None, None, gamma, beta, training=True, eps=eps)

    monkeypatch.setattr(O, "batchnorm_train", bn)
    with torch.no_grad():
        O.resnet_stages(P, torch.rand(1, 3, 64, 64), arch)
    assert seen == want


def test_initial_state_and_load_on_cpu_model():
    m = _model()
    init = m.bn_stats()
    assert init.numel() == m.bn_numel and set(init.tolist()) == {0.0, 1.0}
    assert torch.equal(init[:64], torch.zeros(64)) and torch.equal(init[64:128], torch.ones(64))
    v = _random_stats(m)
    m.load_bn_stats(v)
    assert torch.equal(m.bn_stats(), v)
    with pytest.raises(ValueError):
        m.load_bn_stats(v[:-2])
    bad = v.clone()
    bad[64] = -1.0
    with pytest.raises(ValueError):
        m.load_bn_stats(bad)
    assert torch.equal(m.bn_stats(), v)


def test_checkpoint_roundtrip_of_bn_stats(tmp_path):
    import md2hip
    a = _model(seed=42)
    v = _random_stats(a, 1)
    a.load_bn_stats(v)
    path = str(tmp_path / "ck.safetensors")
    md2hip.save_checkpoint(path, a)
    b = _model(seed=7)
    md2hip.load_checkpoint(path, b)
    assert torch.equal(a.flat, b.flat)
    assert torch.equal(b.bn_stats(), v)


def _write_old_style(path, model, extra_tensors=None):
    """A checkpoint as written before the statistics were stored (no bn_stats tensor)."""
    from safetensors.torch import save_file
    from md2hip import checkpoint as ck
    tensors = {"params": model.flat.detach().float().cpu().contiguous()}
    tensors.update(extra_tensors or {})
    meta = {"format": ck._FORMAT, "model": ck._model_meta(model), "extra": {}}
    save_file(tensors, path, metadata={"md2hip": json.dumps(meta)})


def test_checkpoint_without_bn_stats_leaves_them(tmp_path):
    import md2hip
    path = str(tmp_path / "old.safetensors")
    _write_old_style(path, _model(seed=42))
    b = _model(seed=7)
    v = _random_stats(b, 2)
    b.load_bn_stats(v)
    md2hip.load_checkpoint(path, b)
    assert torch.equal(b.bn_stats(), v)


def test_checkpoint_refuses_wrong_bn_stats_length(tmp_path):
    import md2hip
    a = _model(seed=42)
    path = str(tmp_path / "bad.safetensors")
    _write_old_style(path, a, {"bn_stats": torch.ones(a.bn_numel - 2)})
    b = _model(seed=7)
    before = b.flat.clone()
    with pytest.raises(ValueError):
        md2hip.load_checkpoint(path, b)
    assert torch.equal(b.flat, before)
