"""md2_lidar_depth and md2_disp_post_process on the GPU against their float32 NumPy restatements
(tests/_lidar_ref.py: include/md2.h operation by operation).  Both are stated in fp32 without
contraction and use integer atomics only, so every comparison here is BIT FOR BIT: the whole depth
batch, the counts and the blended disparities.  (The restatement itself is held to float64 on the
CPU, tests/test_lidar_abi.py.)"""
import numpy as np
import pytest
import torch

from tests import _lidar_ref as R

pytestmark = pytest.mark.gpu

IDENT = np.eye(3, 4, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu_depth(points, offsets, P, h, w, **kw):
    import md2hip
    d, c = md2hip.lidar_depth((torch.from_numpy(points).cuda(), offsets), P, h, w, return_counts=True, **kw)
    return d.cpu().numpy(), c.cpu().numpy()


def check(points, offsets, P, h, w, **kw):
    """The device result, after holding all of it to the restatement."""
    d, c = gpu_depth(points, offsets, P, h, w, **kw)
    rd, rc = R.lidar_depth_ref(points, offsets, P, h, w, **kw)
    assert d.dtype == np.float32 and d.shape == rd.shape and c.dtype == np.int32
    assert np.array_equal(c, rc), (c, rc)
    diff = bits(d) != bits(rd)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], d[diff][:5], rd[diff][:5])
    return d, c


def exact_points(uvz):
    """Points that [I | 0] projects to exactly (u, v) at depth z: z a power of two, u and v with few
    bits, so u * z, v * z and the quotients are exact."""
    pts = np.array([[u * z, v * z, z, 0.25] for u, v, z in uvz], dtype=np.float32)
    return pts


# ---- generator cases ------------------------------------------------------------------------------
def test_one_small_scan():
    points, offsets = R.make_scans(1, [700])
    d, c = check(points, offsets, R.calib(8, 16), 8, 16)
    assert c[0, 1] > 20


def test_three_scans_own_matrices_empty_middle():
    h, w = 24, 80
    points, offsets = R.make_scans(2, [4000, 0, 1237])
    P = np.stack([R.calib(h, w), R.calib(h, w, shift_px=5.0), R.calib(h, w, shift_px=5.0)])
    d, c = check(points, offsets, P, h, w)
    assert c[1].tolist() == [0, 0] and not d[1].any()            # the empty scan: all zero, no bleed
    assert c[0, 1] > 200 and c[2, 1] > 50
    # the 5 px shift is visible: scan 2 under scan 0's matrix gives another map
    other, _ = R.lidar_depth_ref(points[offsets[2]:], np.array([0, 1237]), P[0], h, w)
    assert not np.array_equal(other[0], d[2])
    # one matrix for all scans broadcasts
    d1, c1 = check(points, offsets, P[0], h, w)
    assert np.array_equal(d1[0], d[0])


@pytest.fixture(scope="module")
def full_size():
    points, offsets = R.make_scans(3, [120000, 120000])
    P = R.calib()
    return points, offsets, P, R.lidar_depth_ref(points, offsets, P, R.CAM_H, R.CAM_W)


def test_two_full_scans(full_size):
    points, offsets, P, (rd, rc) = full_size
    d, c = gpu_depth(points, offsets, P, R.CAM_H, R.CAM_W)
    assert np.array_equal(c, rc), (c, rc)
    assert np.array_equal(bits(d), bits(rd))
    assert (rc[:, 0] - rc[:, 1] > 100).all()                     # collisions were decided


def test_list_of_scans_equals_pair(full_size):
    import md2hip
    points, offsets, P, (rd, rc) = full_size
    scans = [torch.from_numpy(points[offsets[i]:offsets[i + 1]]).cuda() for i in range(2)]
    d = md2hip.lidar_depth(scans, torch.from_numpy(P), R.CAM_H, R.CAM_W)
    assert isinstance(d, torch.Tensor) and d.is_cuda and d.shape == (2, R.CAM_H, R.CAM_W)
    assert np.array_equal(bits(d.cpu().numpy()), bits(rd))


# ---- hand-built scans: P = [I | 0], power-of-two depths, exact coordinates ---------------------------
H0, W0 = 5, 7


def hand(uvz, **kw):
    pts = exact_points(uvz)
    kw.setdefault("forward_only", False)          # X = u * z here, not a forward axis
    return check(pts, np.array([0, len(pts)]), IDENT, H0, W0, **kw)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (1, 0, 2), (1, 2, 0)])
def test_nearest_of_three_wins_wherever_it_stands(order):
    three = [(3.0, 2.0, 8.0), (3.25, 2.25, 2.0), (2.75, 1.75, 4.0)]      # all round to (3, 2)
    d, c = hand([three[k] for k in order])
    assert c.tolist() == [[3, 1]]
    assert d[0, 1, 2] == 2.0 and np.count_nonzero(d) == 1


def test_ties_go_to_even():
    d, c = hand([(2.5, 1.0, 2.0), (3.5, 2.0, 2.0), (1.0, 2.5, 4.0), (2.0, 3.5, 4.0)])
    assert c.tolist() == [[4, 4]]
    assert d[0, 0, 1] == 2.0            # u 2.5 -> 2 -> ix 1
    assert d[0, 1, 3] == 2.0            # u 3.5 -> 4 -> ix 3
    assert d[0, 1, 0] == 4.0            # v 2.5 -> 2 -> iy 1
    assert d[0, 3, 1] == 4.0            # v 3.5 -> 4 -> iy 3


def test_edges():
    eps = 2.0 ** -10
    d, c = hand([(0.5, 1.0, 2.0),                 # rint 0 -> ix -1: dropped
                 (1.0, 0.5, 2.0),                 # iy -1: dropped
                 (W0 + 0.5 + eps, 1.0, 2.0),      # rint W0 + 1: out
                 (1.0, H0 + 0.5 + eps, 2.0),      # out
                 (-3.0, 2.0, 2.0), (2.0, -3.0, 2.0)])
    assert c.tolist() == [[0, 0]] and not d.any()
    d, c = hand([(1.0, 1.0, 2.0), (float(W0), float(H0), 4.0), (float(W0), 1.0, 8.0), (1.0, float(H0), 16.0),
                 (W0 + 0.5, 2.0, 32.0),           # tie at W0 + 0.5 (7.5) -> 8 -> out; kept out of the image
                 (1.5, 3.0, 64.0)])               # 1.5 -> 2 -> ix 1
    assert d[0, 0, 0] == 2.0 and d[0, H0 - 1, W0 - 1] == 4.0 and d[0, 0, W0 - 1] == 8.0 and d[0, H0 - 1, 0] == 16.0
    assert d[0, 2, 1] == 64.0
    assert c.tolist() == [[5, 5]]


def test_huge_coordinates_do_not_wrap():
    # u = 2^32 would be pixel -1 or 0 after an int conversion that wraps; 3e38 / 2^-100 is inf
    pts = np.array([[2.0 ** 33, 2.0, 2.0, 0], [2.0, 2.0 ** 33, 2.0, 0], [-(2.0 ** 33), 2.0, 2.0, 0],
                    [3e38, 2.0, 2.0 ** -100, 0]], dtype=np.float32)
    d, c = check(pts, np.array([0, 4]), IDENT, H0, W0, forward_only=False)
    assert c.tolist() == [[0, 0]] and not d.any()


def test_forward_only():
    # velodyne-like matrix: camera z = X (forward), u = 2 - Y / X, v = 2 - Z / X
    P = np.array([[2, -1, 0, 0], [2, 0, -1, 0], [1, 0, 0, 0]], dtype=np.float32)
    pts = np.array([[4.0, 0.0, 0.0, 0], [-4.0, 4.0, 0.0, 0], [-0.0, 1.0, 1.0, 0]], dtype=np.float32)
    off = np.array([0, 3])
    d, c = check(pts, off, P, H0, W0, forward_only=True)
    assert c.tolist() == [[1, 1]] and d[0, 1, 1] == 4.0
    # without the filter the point behind still has zc = X < 0 and is dropped by the zc test
    d, c = check(pts, off, P, H0, W0, forward_only=False)
    assert c.tolist() == [[1, 1]]
    # a matrix that sees backwards (zc = -X): the point behind lands only when the filter is off
    Pb = np.array([[-2, -1, 0, 0], [-2, 0, -1, 0], [-1, 0, 0, 0]], dtype=np.float32)
    d, c = check(pts, off, Pb, H0, W0, forward_only=False)
    assert c.tolist() == [[1, 1]] and d[0, 1, 0] == 4.0          # u = (8 - 4) / 4 = 1, v = 8 / 4 = 2
    d, c = check(pts, off, Pb, H0, W0, forward_only=True)
    assert c.tolist() == [[0, 0]]


def test_nonpositive_and_nonfinite():
    nan, inf = np.nan, np.inf
    pts = np.array([[2.0, 2.0, 0.0, 0],            # zc = 0: u = inf
                    [2.0, 2.0, -1.0, 0],           # zc < 0, u and v inside the image by sign only
                    [-4.0, -4.0, -2.0, 0],         # zc < 0 with u = v = 2: must not land
                    [nan, 2.0, 1.0, 0], [2.0, nan, 1.0, 0], [2.0, 2.0, nan, 0],
                    [inf, 2.0, 1.0, 0], [2.0, -inf, 1.0, 0], [2.0, 2.0, inf, 0],
                    [inf, inf, inf, 0], [0.0, 0.0, 0.0, 0],
                    [4.0, 4.0, 2.0, nan]],         # reflectance is ignored: this one lands at (2, 2)
                   dtype=np.float32)
    d, c = check(pts, np.array([0, len(pts)]), IDENT, H0, W0, forward_only=False)
    assert c.tolist() == [[1, 1]] and d[0, 1, 1] == 2.0
    d, c = check(pts, np.array([0, len(pts)]), IDENT, H0, W0, forward_only=True)
    assert c.tolist() == [[1, 1]]


def test_vel_depth_stores_and_selects_by_x():
    # zc = Z orders the two points one way, X the other; both land in pixel (ix 1, iy 1)
    P = np.array([[0, 2, 0, 0], [0, 0, 2, 0], [0, 0, 1, 0]], dtype=np.float32)    # u = 2Y/Z, v = 2, zc = Z
    pts = np.array([[16.0, 2.0, 2.0, 0], [8.0, 4.0, 4.0, 0], [-1.0, 8.0, 8.0, 0], [0.0, 16.0, 16.0, 0]],
                   dtype=np.float32)
    off = np.array([0, 4])
    d, c = check(pts, off, P, H0, W0, forward_only=False, vel_depth=False)
    assert d[0, 1, 1] == 2.0 and c.tolist() == [[4, 1]]
    d, c = check(pts, off, P, H0, W0, forward_only=False, vel_depth=True)
    assert d[0, 1, 1] == 8.0 and c.tolist() == [[2, 1]]          # X <= 0 never competes
    d, c = check(pts, off, P, H0, W0, forward_only=True, vel_depth=True)
    assert d[0, 1, 1] == 8.0 and c.tolist() == [[2, 1]]


# ---- other checks -----------------------------------------------------------------------------------
def test_bitwise_reproducible_and_counts_null(full_size):
    import ctypes as C
    import md2hip
    from md2hip._lib import LidarCfg, check as rc_check, lib, ptr, stream_of
    points, offsets, P, (rd, rc) = full_size
    pts = torch.from_numpy(points).cuda()
    h, w = R.CAM_H, R.CAM_W
    d1, c1 = md2hip.lidar_depth((pts, offsets), P, h, w, return_counts=True)
    d2, c2 = md2hip.lidar_depth((pts, offsets), P, h, w, return_counts=True)
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32)) and torch.equal(c1, c2)
    # an output buffer full of 0x5A bytes, and no counts: the call clears what it needs itself
    d3 = torch.full((2, h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cfg = LidarCfg(2, h, w, 1, 0)
    off = (C.c_longlong * 3)(*offsets.tolist())
    Pm = np.ascontiguousarray(np.broadcast_to(P, (2, 3, 4)), dtype=np.float32)
    rc_check(lib().md2_lidar_depth(C.byref(cfg), ptr(pts), off, Pm.ctypes.data_as(C.POINTER(C.c_float)), ptr(d3),
                                   None, stream_of("cuda")), "md2_lidar_depth")
    torch.cuda.synchronize()
    assert torch.equal(d1.view(torch.int32), d3)
    # without return_counts the wrapper passes NULL too
    d4 = md2hip.lidar_depth((pts, offsets), P, h, w)
    assert torch.equal(d1.view(torch.int32), d4.view(torch.int32))


def test_seventy_scans_go_through_in_chunks():
    import md2hip
    h, w = 8, 16
    sizes = [(37 * k) % 90 for k in range(70)]                   # includes empty scans
    points, offsets = R.make_scans(4, sizes)
    P = np.stack([R.calib(h, w, shift_px=float(k % 7)) for k in range(70)])
    d, c = check(points, offsets, P, h, w)
    assert c[64:, 1].sum() > 0                                   # the second chunk holds measurements
    scans = [torch.from_numpy(points[offsets[i]:offsets[i + 1]]).cuda() for i in range(70)]
    dl = md2hip.lidar_depth(scans, P, h, w)
    assert np.array_equal(bits(dl.cpu().numpy()), bits(d))


def test_wrapper_rejects_mismatches_on_device_tensors():
    import md2hip
    pts = torch.zeros(5, 4, device="cuda")
    P = np.eye(3, 4, dtype=np.float32)
    with pytest.raises(ValueError, match="P must be"):
        md2hip.lidar_depth([pts, pts], np.stack([P, P, P]), 8, 16)
    for bad in ([0], [[0, 2, 5]], [0.0, 2.0, 5.0], [-1, 2, 5], [0, 3, 2], [0, 2, 6]):
        with pytest.raises(ValueError, match="offsets"):
            md2hip.lidar_depth((pts, bad), P, 8, 16)
    with pytest.raises(ValueError, match="alias"):
        d = torch.zeros(1, 4, 4, device="cuda")
        f = torch.zeros(1, 4, 4, device="cuda")
        md2hip.post_process_disparity(d, f, out=f)
    with pytest.raises(ValueError, match="shape"):
        md2hip.post_process_disparity(torch.zeros(1, 4, 4, device="cuda"), torch.zeros(1, 4, 5, device="cuda"))


# ---- post_process_disparity -----------------------------------------------------------------------------
def _pp(a, b, **kw):
    import md2hip
    return md2hip.post_process_disparity(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), **kw).cpu().numpy()


@pytest.mark.parametrize("shape", [(2, 8, 16), (2, 1, 8, 16), (3, 5, 1), (2, 3, 21), (1, 2, 300)])
def test_post_process_bit_equal(shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.uniform(0.01, 1.0, shape).astype(np.float32)
    b = rng.uniform(0.01, 1.0, shape).astype(np.float32)
    got, want = _pp(a, b), R.post_process_ref(a, b)
    assert got.shape == a.shape and np.array_equal(bits(got), bits(want))
    if shape[-1] == 21:                                          # the middle column: both ramps 0
        assert np.array_equal(got[..., 10], np.float32(0.5) * (a[..., 10] + b[..., 10]))
    if shape[-1] == 1:                                           # t = 0: ml = mr = 1 -> (l + r) - the mean
        assert np.array_equal(bits(got), bits((a + b) + np.float32(-1) * (np.float32(0.5) * (a + b))))


def test_post_process_out_aliases_disp():
    import md2hip
    rng = np.random.default_rng(12)
    a = rng.uniform(0.01, 1.0, (2, 1, 8, 16)).astype(np.float32)
    b = rng.uniform(0.01, 1.0, (2, 1, 8, 16)).astype(np.float32)
    d, f = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = md2hip.post_process_disparity(d, f, out=d)
    assert out.data_ptr() == d.data_ptr()
    assert np.array_equal(bits(d.cpu().numpy()), bits(R.post_process_ref(a, b)))
    assert np.array_equal(f.cpu().numpy(), b)


def test_post_process_symmetric_input_returns_disp():
    rng = np.random.default_rng(13)
    a = rng.uniform(0.01, 1.0, (2, 6, 41)).astype(np.float32)
    got = _pp(a, np.ascontiguousarray(a[..., ::-1]))
    assert np.array_equal(bits(got), bits(R.post_process_ref(a, a[..., ::-1])))
    # t in [0.1, 0.9] (x = 4 .. 36 of 0 .. 40): both ramps are 0, out = 0.5 * (l + l) = l exactly
    assert np.array_equal(got[..., 5:36], a[..., 5:36])


# ---- end to end --------------------------------------------------------------------------------------
def test_depth_errors_on_device_map_equals_uploaded_restatement(full_size):
    import md2hip
    points, offsets, P, (rd, rc) = full_size
    h, w = R.CAM_H, R.CAM_W
    gt = md2hip.lidar_depth((torch.from_numpy(points).cuda(), offsets), P, h, w)
    disp = torch.from_numpy(np.random.default_rng(14).uniform(0.02, 0.9, (2, 1, 96, 320)).astype(np.float32)).cuda()
    m1, c1 = md2hip.depth_errors(disp, gt)
    m2, c2 = md2hip.depth_errors(disp, torch.from_numpy(rd).cuda())
    assert (c1[:, 0] > 1000).all().item()
    assert torch.equal(m1.view(torch.int32), m2.view(torch.int32)) and torch.equal(c1, c2)


def _aggregate(rows, counts):
    """evaluate_depth's reduction of per-image rows, as it stood before post_process existed."""
    import md2hip
    m = torch.cat(rows).cpu().numpy().astype(np.float64)
    c = torch.cat(counts).cpu().numpy()
    ok = c[:, 0] > 0
    out = {name: float(m[ok, k].mean()) for k, name in enumerate(md2hip.METRIC_NAMES[:7])}
    med = float(np.median(m[ok, 7]))
    out.update(ratio_median=med, ratio_std=float(np.std(m[ok, 7] / med)), images=int(len(c)),
               skipped=int((~ok).sum()), n_bad=int(c[:, 1].sum()), nonfinite_inputs=0)
    return out


def test_evaluate_depth_post_process():
    import md2hip
    from tests import _data as D
    N, H, W, Hg, Wg = 2, 64, 128, 48, 100
    enc = md2hip.ResNet(18, in_channels=3)
    model = md2hip.Model(enc, md2hip.DepthDecoder(encoder_channels=enc.stages, scale_levels=[2, 3, 4, 5],
                                                  embedding_levels=0), md2hip.PoseDecoder(enc.stages[-1]), seed=42)
    model.testmode()
    rng = np.random.default_rng(15)
    batches = []
    for s in (31, 32):
        x = D.triplets(N, 3, H, W, seed=s)[:, 1].float().cuda().contiguous()
        gt = rng.uniform(0.5, 60.0, size=(N, Hg, Wg)).astype(np.float32)
        gt[rng.uniform(size=gt.shape) < 0.3] = 0
        batches.append((x, torch.from_numpy(gt).cuda()))

    plain_rows, plain_counts, pp_rows, pp_counts = [], [], [], []
    for x, gt in batches:
        disp = md2hip.eval_disparity(model, x)[-1].clone()       # the next call overwrites the buffer
        flipped = md2hip.eval_disparity(model, x.flip(-1))[-1]
        blend = md2hip.post_process_disparity(disp, flipped)
        assert not torch.equal(blend, disp)
        for rows, counts, d in ((plain_rows, plain_counts, disp), (pp_rows, pp_counts, blend)):
            m, c = md2hip.depth_errors(d, gt)
            rows.append(m)
            counts.append(c)
    want_plain, want_pp = _aggregate(plain_rows, plain_counts), _aggregate(pp_rows, pp_counts)
    assert md2hip.evaluate_depth(model, batches, post_process=True) == want_pp
    # the default path is what it was
    assert md2hip.evaluate_depth(model, batches) == want_plain
    assert md2hip.evaluate_depth(model, batches, post_process=False) == want_plain
    assert want_pp["abs_rel"] != want_plain["abs_rel"]
