"""md2_depth_eval on the GPU against the fp64 NumPy reference (tests/_depth_eval_ref.py: the
formulas of include/md2.h applied to the same fp32 inputs).

Bounds.  Continuous outputs (abs_rel, sq_rel, rmse, rmse_log, ratio, med_pred): relative error
within max(1e-5, 4 x floor), the floor being the largest deviation from fp64 of the same formulas in
float32 NumPy over two summation orders (``fp32_floor``).  count and n_bad are exact; med_gt equals
``np.median(gt[mask])`` evaluated in float32 bit for bit (no arithmetic happens to gt before the
selection).  Threshold fractions a_k: a pixel whose max(g/p, p/g) lies within relative 1e-5 of
1.25^k in the reference may fall either side in fp32, so |a_k - a_k_ref| * count <= borderline_k,
where a_k * count is rounded to the nearest integer first (a_k is stored in fp32, which moves the
product by < 0.02 at the counts used here), and borderline_k <= 0.001 * count is asserted as a
condition on the inputs.  The hand-built cases have no borderline pixel and compare a_k exactly.
A single valid pixel under median scaling has p == g in exact arithmetic, so its four error metrics
are rounding alone and have no relative error: they are held to 1e-6 (abs_rel, rmse_log), 1e-6 * g
(rmse, sq_rel) absolutely -- a few fp32 roundings of g -- and its a_k must be exactly 1.
Every case's floor, bound and observed error go to the parity record ``depth_eval``."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import _depth_eval_ref as R
from tests._model_parity import parity_record_path

pytestmark = pytest.mark.gpu

RTOL = 1e-5
_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    worst = {}
    for rec in _RECORD.values():
        for k, v in rec["outputs"].items():
            worst[k] = max(worst.get(k, 0.0), v["err"])
    with open(parity_record_path("depth_eval"), "w") as f:
        json.dump({"worst_err": worst, "cases": _RECORD}, f, indent=1)


def gpu_eval(disp, gt, **kw):
    import md2hip
    m, c = md2hip.depth_errors(torch.from_numpy(disp).cuda().contiguous(), torch.from_numpy(gt).cuda().contiguous(),
                               **kw)
    return m.cpu().numpy(), c.cpu().numpy()


def _crop_of(crop, Hg, Wg):
    return R.garg(Hg, Wg) if isinstance(crop, str) else crop


def check(label, disp, gt, crop="garg", exact_a=False, **kw):
    """Run the batch on the GPU and hold every image to the reference.  Returns (metrics, counts,
    [reference per image])."""
    m, c = gpu_eval(disp, gt, crop=crop, **kw)
    refs = []
    for i in range(disp.shape[0]):
        box = _crop_of(crop, *gt.shape[1:])
        ref = R.reference(disp[i], gt[i], box, **kw)
        refs.append(ref)
        tag = f"{label}[{i}]"
        assert int(c[i, 0]) == ref["count"], (tag, c[i], ref["count"])
        assert int(c[i, 1]) == ref["n_bad"], (tag, c[i], ref["n_bad"])
        if ref["count"] == 0:
            assert np.isnan(m[i]).all(), (tag, m[i])
            continue
        floor = R.fp32_floor(disp[i], gt[i], box, **kw)
        rec = {"count": ref["count"], "borderline": ref["borderline"], "outputs": {}}
        single = ref["count"] == 1 and kw.get("median_scaling", True)
        if single:
            g1 = float(m[i, 8])
            for k, lim in (("abs_rel", 1e-6), ("sq_rel", 1e-6 * g1), ("rmse", 1e-6 * g1), ("rmse_log", 1e-6)):
                assert 0.0 <= m[i, R.NAMES.index(k)] <= lim, (tag, k, m[i])
            assert (m[i, 4:7] == 1.0).all(), (tag, m[i])
        for k in (("ratio", "med_pred") if single else R.CONTINUOUS):
            got = float(m[i, R.NAMES.index(k)])
            err = abs(got - ref[k]) / abs(ref[k])
            rec["outputs"][k] = {"err": err, "floor": floor[k], "bound": max(RTOL, 4 * floor[k])}
        _RECORD[tag] = rec
        print(f"\n{tag} count {ref['count']} " + ", ".join(
            f"{k} {v['err']:.1e}/{v['bound']:.1e}" for k, v in rec["outputs"].items()))
        # med_gt: the float32 median, bit for bit
        mask = _mask(disp[i], gt[i], box, **kw)
        want = np.median(gt[i][mask])
        assert want.dtype == np.float32
        assert m[i, 8].tobytes() == want.tobytes(), (tag, m[i, 8], want)
        for k, v in rec["outputs"].items():
            assert v["err"] <= v["bound"], (tag, k, v)
        for k in range(3):
            bl = ref["borderline"][k]
            assert bl <= 0.001 * ref["count"], (tag, k, bl)          # a condition on the inputs
            got = m[i, 4 + k]
            if exact_a:
                assert bl == 0, (tag, k, bl)
                assert got == np.float32(ref["a_counts"][k] / ref["count"]), (tag, k, got, ref["a_counts"][k])
            else:
                assert abs(round(float(got) * ref["count"]) - ref["a_counts"][k]) <= bl, \
                    (tag, k, got, ref["a_counts"][k], bl)
    return m, c, refs


def _mask(disp, gt, box, eval_min=1e-3, eval_max=80.0, min_depth=0.1, max_depth=100.0, **_):
    y0, y1, x0, x1 = box if box is not None else (0, gt.shape[0], 0, gt.shape[1])
    with np.errstate(all="ignore"):
        pred = R.pred_depth(disp, *gt.shape, min_depth, max_depth)
        m = (gt > np.float32(eval_min)) & (gt < np.float32(eval_max)) & np.isfinite(pred) & (pred > 0)
    inside = np.zeros_like(m)
    inside[y0:y1, x0:x1] = True
    return m & inside


@pytest.fixture(scope="module")
def real_size():
    """Case 3's inputs (N=2, 128x416 -> 375x1242), shared with the reproducibility test."""
    return R.make_case(3, 2, 128, 416, 375, 1242)


# ---- 1. identity size, odd and even count -----------------------------------------------------
def test_identity_size_odd_and_even_count():
    disp, gt = R.make_case(1, 3, 8, 16, 8, 16)
    box = R.garg(8, 16)
    want_parity = [1, 0, None]
    for i, par in enumerate(want_parity):
        if par is None:
            continue
        mask = _mask(disp[i], gt[i], box)
        if mask.sum() % 2 != par:                  # remove one more valid pixel
            y, x = np.argwhere(mask)[0]
            gt[i, y, x] = 0.0
    m, c, refs = check("identity_8x16", disp, gt)
    assert c[0, 0] % 2 == 1 and c[1, 0] % 2 == 0 and c[0, 0] > 20 and c[1, 0] > 20


# ---- 2. non-integer upsample ------------------------------------------------------------------
def test_non_integer_upsample():
    disp, gt = R.make_case(2, 2, 32, 104, 93, 310)
    _, c, _ = check("up_32x104_93x310", disp, gt)
    assert (c[:, 0] > 10000).all()


# ---- 3. real size -----------------------------------------------------------------------------
def test_real_size(real_size):
    disp, gt = real_size
    _, c, _ = check("kitti_128x416_375x1242", disp, gt)
    assert (c[:, 0] > 170000).all()


# ---- 4. downsample, no crop -------------------------------------------------------------------
def test_downsample_whole_image():
    disp, gt = R.make_case(4, 1, 24, 40, 10, 17)
    check("down_24x40_10x17", disp, gt, crop=None)


# ---- 5. crop and range edges ------------------------------------------------------------------
@pytest.mark.parametrize("crop", [(5, 6, 0, 64), (0, 16, 40, 41)], ids=["row", "column"])
def test_custom_crop(crop):
    disp, gt = R.make_case(5, 2, 16, 64, 16, 64, zero_frac=0.1)
    check(f"crop_{crop}", disp, gt, crop=crop, exact_a=True)


def test_range_edges_are_excluded():
    disp, gt = R.make_case(6, 1, 16, 64, 16, 64)
    plain = R.reference(disp[0], gt[0], None)
    gt2 = gt.copy()
    zeros = np.argwhere(gt2[0] == 0)
    for (y, x), v in zip(zeros[:6], [1e-3, 80.0, np.nan, np.inf, -5.0, np.float32(1e-3)]):
        gt2[0, y, x] = v                       # bounds are strict, NaN compares false
    _, c, refs = check("range_edges", disp, gt2, crop=None, exact_a=True)
    assert refs[0]["count"] == plain["count"] and refs[0]["n_bad"] == 0
    # the neighbours of the bounds on the inside are counted
    gt3 = gt2.copy()
    (y0, x0), (y1, x1) = zeros[0], zeros[1]
    gt3[0, y0, x0] = np.nextafter(np.float32(1e-3), np.float32(1))
    gt3[0, y1, x1] = np.nextafter(np.float32(80), np.float32(0))
    _, c3, _ = check("range_edges_inside", disp, gt3, crop=None, exact_a=True)
    assert c3[0, 0] == plain["count"] + 2


# ---- 6. selection stress ----------------------------------------------------------------------
def _stress_gt(kind, rng, H, W):
    n = H * W
    gt = np.zeros(n, np.float32)
    if kind == "four_values":
        gt[:] = rng.choice(np.array([2.5, 7.0, 7.5, 31.0], np.float32), size=n)
        gt[rng.uniform(size=n) < 0.3] = 0
    elif kind == "all_equal":
        gt[rng.uniform(size=n) < 0.7] = 12.5
    elif kind.startswith("count"):
        k = int(kind[5:])
        gt[rng.choice(n, size=k, replace=False)] = np.array([4.0, 9.0, 23.0], np.float32)[:k]
    elif kind == "exponent_boundary":
        two = np.float32(2)
        vals = np.concatenate([np.full(200, 1.0), np.full(100, np.nextafter(two, np.float32(0))), np.full(50, two),
                               np.full(50, np.nextafter(two, np.float32(3))), np.full(200, 3.0)]).astype(np.float32)
        gt[rng.choice(n, size=len(vals), replace=False)] = vals
    elif kind == "wide_range":
        gt[:] = np.exp(rng.uniform(np.log(1e-2), np.log(79.9), size=n)).astype(np.float32)
        gt[rng.uniform(size=n) < 0.2] = 0
    else:
        raise KeyError(kind)
    return gt.reshape(1, H, W)


STRESS = ["four_values", "all_equal", "count1", "count2", "count3", "exponent_boundary", "wide_range"]


@pytest.mark.parametrize("kind,H,W", [(k, 16, 64) for k in STRESS] + [("four_values", 64, 512)],
                         ids=STRESS + ["four_values_64x512"])
def test_selection_stress(kind, H, W):
    rng = np.random.default_rng(60 + STRESS.index(kind))
    disp = rng.uniform(0.02, 0.9, size=(1, H, W)).astype(np.float32)
    gt = _stress_gt(kind, rng, H, W)
    # the 64x512 run has tens of thousands of pixels: the borderline rule, not exact a_k
    m, c, refs = check(f"stress_{kind}_{H}x{W}", disp, gt, crop=None, exact_a=(H * W <= 1024))
    if kind == "exponent_boundary":       # the two middle ranks sit in different top-level bins
        two = np.float32(2)
        assert c[0, 0] == 600 and m[0, 8] == np.float32(0.5) * (np.nextafter(two, np.float32(0)) + two)
    if kind.startswith("count"):
        assert c[0, 0] == int(kind[5:])


# ---- 7. empty mask ----------------------------------------------------------------------------
def test_empty_mask_beside_a_normal_image():
    disp, gt = R.make_case(7, 2, 16, 64, 16, 64)
    alone, c_alone = gpu_eval(disp[1:], gt[1:], crop=None)
    gt[0] = 0.0
    m, c, _ = check("empty_mask", disp, gt, crop=None, exact_a=True)      # returns MD2_OK (no exception)
    assert c[0, 0] == 0 and c[0, 1] == 0 and np.isnan(m[0]).all()
    assert m[1].tobytes() == alone[0].tobytes() and (c[1] == c_alone[0]).all()


# ---- 8. bad pixels ----------------------------------------------------------------------------
def test_bad_pixels_are_counted_and_excluded():
    disp, gt = R.make_case(8, 1, 16, 64, 16, 64)
    valid = np.argwhere(_mask(disp[0], gt[0], None))
    (ya, xa), (yb, xb) = valid[3], valid[40]
    clean = R.reference(disp[0], gt[0], None)
    disp[0, ya, xa] = np.nan
    disp[0, yb, xb] = np.inf
    m, c, refs = check("bad_pixels", disp, gt, crop=None, exact_a=True)
    assert c[0, 1] == 2 and c[0, 0] == clean["count"] - 2
    assert np.isfinite(m[0]).all()
    # the reference without those pixels: the same as the reference that saw and excluded them
    gt2 = gt.copy()
    gt2[0, ya, xa] = gt2[0, yb, xb] = 0.0
    without = R.reference(disp[0], gt2[0], None)
    for k in R.NAMES:
        assert without[k] == refs[0][k], k


# ---- 9. fixed scale ---------------------------------------------------------------------------
def test_fixed_scale():
    disp, gt = R.make_case(9, 2, 32, 104, 93, 310)
    s = 27.3
    m, c, _ = check("fixed_scale", disp, gt, median_scaling=False, scale=s)
    assert (m[:, 7] == np.float32(s)).all()


# ---- 10. reproducibility ----------------------------------------------------------------------
def test_bitwise_reproducible(real_size):
    import md2hip
    from md2hip._lib import DepthEvalCfg, check as rc_check, lib, ptr, stream_of
    disp, gt = (torch.from_numpy(a).cuda().contiguous() for a in real_size)
    m1, c1 = md2hip.depth_errors(disp, gt)
    m2, c2 = md2hip.depth_errors(disp, gt)
    assert torch.equal(m1.view(torch.int32), m2.view(torch.int32)) and torch.equal(c1, c2)
    # a workspace full of 0xFF bytes: the call clears what it needs itself
    N, h, w = disp.shape
    Hg, Wg = gt.shape[1:]
    cfg = DepthEvalCfg(N, h, w, Hg, Wg, *md2hip.garg_crop(Hg, Wg), 0.1, 100.0, 1e-3, 80.0, 1, 1.0)
    nbytes = lib().md2_depth_eval_workspace_size(C.byref(cfg))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    m3 = torch.empty_like(m1)
    c3 = torch.empty_like(c1)
    rc_check(lib().md2_depth_eval(C.byref(cfg), ptr(disp), ptr(gt), ptr(m3), ptr(c3), ptr(ws), stream_of("cuda")),
             "md2_depth_eval")
    torch.cuda.synchronize()
    assert torch.equal(m1.view(torch.int32), m3.view(torch.int32)) and torch.equal(c1, c3)
    assert torch.isfinite(m1).all()


# ---- 11. dataset driver -----------------------------------------------------------------------
def test_evaluate_depth_driver():
    import md2hip
    from tests import _data as D
    N, H, W, Hg, Wg = 2, 64, 128, 48, 100
    enc = md2hip.ResNet(18, in_channels=3)
    model = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]), seed=42)
    model.testmode()
    rng = np.random.default_rng(11)
    batches = []
    for s in (21, 22):
        x = D.triplets(N, 3, H, W, seed=s)[:, 1].float().cuda().contiguous()
        gt = rng.uniform(0.5, 60.0, size=(N, Hg, Wg)).astype(np.float32)
        gt[rng.uniform(size=gt.shape) < 0.3] = 0
        batches.append((x, torch.from_numpy(gt).cuda()))
    res = md2hip.evaluate_depth(model, batches)
    rows, counts = [], []
    for x, gt in batches:
        disp = md2hip.eval_disparity(model, x)[-1]
        assert disp.shape == (N, 1, H, W)
        m, c = md2hip.depth_errors(disp, gt)
        rows.append(m.cpu().numpy().astype(np.float64))
        counts.append(c.cpu().numpy())
    rows, counts = np.concatenate(rows), np.concatenate(counts)
    assert res["images"] == 4 and res["skipped"] == 0 and res["n_bad"] == 0 and res["nonfinite_inputs"] == 0
    assert (counts[:, 0] > 0).all()
    for k, name in enumerate(md2hip.METRIC_NAMES[:7]):
        want = rows[:, k].mean()
        assert abs(res[name] - want) <= 1e-6 * abs(want), (name, res[name], want)
    med = np.median(rows[:, 7])
    assert abs(res["ratio_median"] - med) <= 1e-6 * med
    assert abs(res["ratio_std"] - np.std(rows[:, 7] / med)) <= 1e-6
    # a NaN in one input frame is an error unless allowed (the network's fmaxf ReLUs turn it into 0,
    # so the driver counts non-finite input elements beside the non-finite predictions)
    x_bad = batches[1][0].clone()
    x_bad[0, 0, 5, 5] = float("nan")
    poisoned = [batches[0], (x_bad, batches[1][1])]
    with pytest.raises(RuntimeError, match="not finite"):
        md2hip.evaluate_depth(model, poisoned)
    res2 = md2hip.evaluate_depth(model, poisoned, allow_nonfinite=True)
    assert res2["images"] == 4 and res2["n_bad"] + res2["nonfinite_inputs"] > 0
