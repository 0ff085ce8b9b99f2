"""GPU: per-sample camera intrinsics in the loss tail (md2_loss_fwd_bwd_sources_k, the per-sample
instances of photo_sources.hip).  Inputs are those of tests/test_gpu_photo_sources.py.

1. Rows all equal to cfg.K / cfg.invK give md2_loss_fwd_bwd_sources' bits on every output: S = 1, 2,
   3, C = 1, 3, with and without the automask and the visualisation outputs (vis_cell among them).
2. Distinct rows against the fp64 oracle.  The oracle takes one K, so it runs per sample (N = 1, that
   sample's K) and the results are combined: loss = mean over samples, gradients = per-sample / N.
   Method and bounds of test_gpu_photo_sources.py::_check_stereo (the GPU's argmin map and bilinear
   cells imposed; loss rel <= 2e-5, d_disp and d_pose relative Frobenius < 2e-4; near ties <= 1 % of
   the pixels per scale, every candidate's share >= 10 %).  The same case with one K for all samples,
   through the uniform entry point, is printed beside it.
3. Rows are indexed by sample: changing row j alone leaves every other sample's bits alone.

Per-sample matrices: from K0 = D.intrinsics(W, H, grid32=False), sample i has fx = K0.fx s_i,
fy = K0.fy s_i 1.03, cx = W/2 + d_i W/16, cy = H/2 - d_i H/16, s = (1.10, 0.92, 1.04),
d = (1, -1, 0.5); K and inv(K) each rounded to the fp32 grid."""
import pytest
import torch

from oracle import md2_oracle as O
from tests import _data as D
from tests import test_gpu_photo_sources as PS

pytestmark = pytest.mark.gpu

SCALES = PS.SCALES
DEV = "cuda"
S_I = (1.10, 0.92, 1.04)
D_I = (1.0, -1.0, 0.5)


def sample_intrinsics(N, W, H):
    """[(K_i, invK_i)] fp64 tensors on the fp32 grid, one pair per sample."""
    K0, _ = D.intrinsics(W, H, grid32=False)
    out = []
    for i in range(N):
        K = torch.zeros(3, 3, dtype=torch.float64)
        K[0, 0] = K0[0, 0] * S_I[i]
        K[1, 1] = K0[1, 1] * S_I[i] * 1.03
        K[0, 2] = W / 2.0 + D_I[i] * W / 16.0
        K[1, 2] = H / 2.0 - D_I[i] * H / 16.0
        K[2, 2] = 1.0
        out.append((D.fp32_grid(K), D.fp32_grid(torch.linalg.inv(K))))
    return out


def rows(Ks):
    """(K, invK) float32 [N, 9] device tensors of a list of per-sample pairs."""
    K = torch.stack([k.reshape(9) for k, _ in Ks]).float().to(DEV).contiguous()
    iK = torch.stack([ik.reshape(9) for _, ik in Ks]).float().to(DEV).contiguous()
    return K, iK


def _sources(mode, x, xs, Rt, cache):
    from md2hip import loss as L
    if mode == "M":
        return PS._two_learned(x, cache), 2, 2
    return L.stereo_sources(x, xs, Rt, cache, temporal=mode == "MS")


def _run(mode, disps, poses, x3, xs, tx, K, invK, am, Kn=None, visualize=True):
    """md2_loss_fwd_bwd_sources (Kn None) or _k on device copies of fp64 inputs; results on the host."""
    import md2hip
    from md2hip import loss as L
    N, _, Cc, H, W = x3.shape
    cache, params = PS._cache_params(K, invK, W, H, N, len(disps), am is not None)
    x = x3.float().to(DEV).contiguous()
    xst = xs.float().to(DEV).contiguous()
    Rt = PS._stereo_Rt(tx)
    src, nsrc, nl = _sources(mode, x, xst, Rt, cache)
    pose = md2hip.pack_poses([(a.float().to(DEV), b.float().to(DEV)) for a, b in poses]) if nl else None
    fs = Cc * H * W
    kw = {} if Kn is None else dict(K=Kn[0], invK=Kn[1])
    r = L.run_loss_sources([d.float().to(DEV).contiguous() for d in disps], pose, x, x.data_ptr() + 4 * fs,
                           3 * fs, src, nsrc, nl, None if am is None else am.float().to(DEV).contiguous(),
                           cache, params, visualize=visualize, **kw)
    torch.cuda.synchronize()
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else (None if v is None else v.cpu()))
            for k, v in r.items()}


# ---- 1. equal rows are the uniform kernel ---------------------------------------------------------
@pytest.mark.parametrize("visualize", [True, False], ids=["vis", "novis"])
@pytest.mark.parametrize("automask", [False, True], ids=["plain", "automask"])
@pytest.mark.parametrize("mode", ["S", "M", "MS"], ids=["S1", "S2", "S3"])
@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 64), (3, 3, 40, 72), (2, 1, 32, 64)])
def test_equal_rows_give_the_uniform_kernels_bits(N, C, H, W, mode, automask, visualize):
    x3, xs, K, invK, disps, poses, tx = PS._stereo_inputs(N, C, H, W, False)
    am = None
    if automask:
        am = 0.2 * torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    want = _run(mode, disps, poses, x3, xs, tx, K, invK, am, visualize=visualize)
    got = _run(mode, disps, poses, x3, xs, tx, K, invK, am, Kn=rows([(K, invK)] * N), visualize=visualize)
    assert set(want) == set(got) and set(want) == set(PS.KEYS if visualize else PS.KEYS[:4])
    for k in want:
        a, b = want[k], got[k]
        if a is None:
            assert k == "d_pose" and mode == "S" and b is None
            continue
        if isinstance(a, list):
            assert len(a) == len(b)
            for i, (u, v) in enumerate(zip(a, b)):
                assert torch.equal(u, v), f"{k}[{i}]"
        else:
            assert a.shape == b.shape and torch.equal(a, b), k


# ---- 2. distinct rows against the fp64 oracle, sample by sample -----------------------------------
def _oracle(disps, poses, n_learned, x, K, invK, am, ids, forced_sel=None, forced_cells=None):
    disps = [d.clone().requires_grad_(True) for d in disps]
    poses = ([(r.clone().requires_grad_(True), t.clone().requires_grad_(True)) for r, t in poses[:n_learned]]
             + list(poses[n_learned:]))
    N, L, Cc, H, W = x.shape
    cache = O.TrainCache(K=K, invK=invK, scales=SCALES, source_ids=ids)
    p = O.Params(target_size=(W, H), batch_size=N, automasking=am is not None, disparity_smoothness=1e-3)
    per_source = []
    loss = O.loss_from_outputs(disps, poses, x, am, cache, p, forced_sel=forced_sel, per_source=per_source,
                               forced_cells=forced_cells)
    loss.backward()
    return loss.detach(), [d.grad for d in disps], poses, per_source


def _against_oracle(mode, N, Cc, H, W, strict, automask, Ks, per_sample, check):
    """Errors of the GPU loss tail against the per-sample oracle; with ``check`` the conditions and
    the bounds are asserted.  Ks: one (K, invK) per sample; per_sample: through the _k entry point."""
    x3, xs, K0, invK0, disps, poses, tx = PS._stereo_inputs(N, Cc, H, W, strict)
    x4 = torch.cat([x3, xs.unsqueeze(1)], 1)
    ids = {"M": (1, 3), "MS": (1, 3, 4), "S": (4,)}[mode]
    S, nl = len(ids), 0 if mode == "S" else 2
    t_st = torch.zeros(N, 3, dtype=torch.float64)
    t_st[:, 0] = tx
    oposes = (list(poses) if nl else []) + ([(torch.zeros(N, 3, dtype=torch.float64), t_st)] if mode != "M" else [])
    am = O.automasking_loss(x4, x4[:, 1], ids).detach() if automask else None
    if per_sample:
        g = _run(mode, disps, poses, x3, xs, tx, K0, invK0, am, Kn=rows(Ks))
    else:
        g = _run(mode, disps, poses, x3, xs, tx, Ks[0][0], Ks[0][1], am)
    one = lambda t, i: None if t is None else t[i:i + 1]
    sample = lambda i, **kw: _oracle([d[i:i + 1] for d in disps], [(r[i:i + 1], t[i:i + 1]) for r, t in oposes], nl,
                                     x4[i:i + 1], Ks[i][0], Ks[i][1], one(am, i), ids, **kw)
    per_src = [sample(i)[3] for i in range(N)]
    forced, npix, worst_tie, least = [], N * H * W, 0.0, 1.0
    for s in range(len(SCALES)):
        ls = [torch.cat([per_src[i][s][j] for i in range(N)], 0) for j in range(S)]
        sel = g["vis_sel"][s].unsqueeze(1).long()
        lmin, ref = ls[0], torch.zeros_like(sel)
        for j in range(1, S):
            ref = torch.where(ls[j] < lmin, torch.full_like(ref, j), ref)
            lmin = torch.where(ls[j] < lmin, ls[j], lmin)
        if am is not None:
            ref = torch.where(~(lmin < am), torch.full_like(ref, -1), ref)
        tie = torch.zeros_like(sel, dtype=torch.bool)
        for i in range(S):
            for j in range(i + 1, S):
                tie |= (ls[i] - ls[j]).abs() <= 1e-4 * torch.maximum(ls[i], ls[j])
        if am is not None:
            tie |= (lmin - am).abs() <= 1e-4 * am.abs().clamp_min(1e-12)
        ntie = tie.sum().item()
        shares = {j: (sel == j).sum().item() / npix for j in (list(range(S)) + ([-1] if am is not None else []))}
        worst_tie = max(worst_tie, ntie / npix)
        if S > 1 or am is not None:
            least = min(least, min(shares.values()))
        mism = ((sel != ref) & ~tie).sum().item()
        if check:
            print(f"scale {s}: near ties {ntie / npix:.4%}, shares {shares}")
            assert ntie <= 0.01 * npix, (s, ntie)
            if S > 1 or am is not None:
                for j, sh in shares.items():
                    assert sh >= 0.10, (s, j, sh)
            assert mism == 0, (s, mism)
        forced.append(sel + (1 if am is not None else 0))
    res = [sample(i, forced_sel=[f[i:i + 1] for f in forced],
                  forced_cells=[c[:, i:i + 1] for c in g["vis_cell"]]) for i in range(N)]
    lo = sum(r[0] for r in res) / N
    dd_o = [torch.cat([res[i][1][s] for i in range(N)], 0) / N for s in range(len(SCALES))]
    out = {"loss": abs(g["loss"].item() - lo.item()) / abs(lo.item()),
           "d_disp": [D.rel_err(g["d_disp"][s], dd_o[s]) for s in range(len(SCALES))], "ties": worst_tie,
           "share": least}
    if nl:
        dp_o = torch.cat([torch.cat([torch.cat([res[i][2][j][0].grad, res[i][2][j][1].grad], 1) for i in range(N)], 0)
                          for j in range(2)], 0) / N
        assert g["d_pose"].shape == (2 * N, 6)
        out["d_pose"] = D.rel_err(g["d_pose"], dp_o)
    else:
        assert g["d_pose"] is None
    return out


def _fmt(e):
    return (f"loss rel {e['loss']:.3e}, d_disp rel {['%.3e' % v for v in e['d_disp']]}"
            + (f", d_pose rel {e['d_pose']:.3e}" if "d_pose" in e else "")
            + f", ties {e['ties']:.3%}, least share {e['share']:.1%}")


def _check_k(mode, N, Cc, H, W, strict, automask):
    Ks = sample_intrinsics(N, W, H)
    e = _against_oracle(mode, N, Cc, H, W, strict, automask, Ks, per_sample=True, check=True)
    print("per-sample K:", _fmt(e))
    twin = _against_oracle(mode, N, Cc, H, W, strict, automask, [D.intrinsics(W, H)] * N, per_sample=False,
                           check=False)
    print("uniform K   :", _fmt(twin))
    assert e["loss"] <= 2e-5, e["loss"]
    for s, v in enumerate(e["d_disp"]):
        assert v < 2e-4, (s, v)
    if "d_pose" in e:
        assert e["d_pose"] < 2e-4, e["d_pose"]


@pytest.mark.parametrize("N,C,H,W,strict,automask", [(2, 3, 32, 64, True, False), (2, 1, 32, 64, False, False),
                                                     (3, 3, 40, 72, False, True)])
def test_m_two_sources_distinct_rows_against_the_oracle(N, C, H, W, strict, automask):
    _check_k("M", N, C, H, W, strict, automask)


@pytest.mark.parametrize("N,C,H,W,strict,automask", PS.STEREO_CASES)
def test_ms_three_sources_distinct_rows_against_the_oracle(N, C, H, W, strict, automask):
    _check_k("MS", N, C, H, W, strict, automask)


def test_s_stereo_source_alone_distinct_rows_against_the_oracle():
    _check_k("S", 3, 3, 40, 72, False, True)


# ---- 3. rows are indexed by sample ----------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 2])
def test_a_row_moves_its_own_sample_only(j):
    N, Cc, H, W = 3, 3, 40, 72
    x3, xs, K0, invK0, disps, poses, tx = PS._stereo_inputs(N, Cc, H, W, False)
    Ks = sample_intrinsics(N, W, H)
    base = _run("M", disps, poses, x3, xs, tx, K0, invK0, None, Kn=rows(Ks))
    K = Ks[j][0].clone()
    K[0, 0] *= 1.05
    K[0, 2] += 1.5
    K[1, 2] -= 0.75
    moved = list(Ks)
    moved[j] = (D.fp32_grid(K), D.fp32_grid(torch.linalg.inv(K)))
    got = _run("M", disps, poses, x3, xs, tx, K0, invK0, None, Kn=rows(moved))
    views = {"vis_loss": lambda r, i: r["vis_loss"][:, i], "vis_sel": lambda r, i: r["vis_sel"][:, i],
             "vis_warped": lambda r, i: r["vis_warped"][:, i]}
    for s in range(len(SCALES)):
        views[f"d_disp[{s}]"] = lambda r, i, s=s: r["d_disp"][s][i]
    for name, view in views.items():
        for i in range(N):
            same = torch.equal(view(base, i), view(got, i))
            assert same == (i != j), (name, i, j)
