"""NumPy restatements of md2_lidar_depth and md2_disp_post_process (include/md2.h) and a synthetic
scan generator, for the LiDAR tests and tools/bench_lidar_depth.py.

``lidar_depth_ref`` / ``post_process_ref`` follow the header operation by operation in the dtype
they are given: in float32 they are what the device must reproduce bit for bit (NumPy rounds every
product, sum and quotient on its own, ``np.rint`` rounds ties to even, ``np.minimum.at`` is the
order-independent minimum); in float64 they are the yardstick the float32 restatement is itself
checked against (tests/test_lidar_abi.py).

The generator imitates a Velodyne HDL-64E over a flat road: azimuth uniform on the full circle,
elevation uniform in -24.8 .. 2 degrees, range the smaller of the ground plane 1.73 m below the
sensor and a uniform 4 .. 80 m "wall".  The calibration is KITTI-like: focal length 721.5377,
principal point (609.56, 172.85) at 375 x 1242, and the usual velodyne -> camera rotation (camera
z = velodyne x, camera x = -velodyne y, camera y = -velodyne z) with its small misalignment."""
import numpy as np

CAM_H, CAM_W = 375, 1242
K = np.array([[721.5377, 0.0, 609.56],
              [0.0, 721.5377, 172.85],
              [0.0, 0.0, 1.0]])
TR = np.array([[4.2768e-04, -9.999672e-01, -8.0845e-03, -1.19846e-02],
               [-7.2106e-03, 8.0812e-03, -9.999413e-01, -5.40398e-02],
               [9.999739e-01, 4.8595e-04, -7.2069e-03, -2.921969e-01]])
SENSOR_HEIGHT = 1.73
MARGIN_PX = 2e-3        # 5 x the largest fp32 coordinate error seen at 375 x 1242 (3.6e-4 px)


def calib(h=CAM_H, w=CAM_W, shift_px=0.0):
    """float32 [3, 4] velodyne -> image matrix for an ``h x w`` raster of the camera's view (rows 0
    and 1 of the camera's matrix scaled), the principal point moved right by ``shift_px`` pixels."""
    k = K.copy()
    k[0, 2] += shift_px * CAM_W / w
    p = k @ TR
    p[0] *= w / CAM_W
    p[1] *= h / CAM_H
    return p.astype(np.float32)


def make_scan(rng, m):
    """[m, 4] float32 points of one synthetic scan."""
    az = rng.uniform(0.0, 2.0 * np.pi, m)
    el = np.deg2rad(rng.uniform(-24.8, 2.0, m))
    wall = rng.uniform(4.0, 80.0, m)
    with np.errstate(divide="ignore"):
        ground = np.where(el < 0.0, SENSOR_HEIGHT / np.sin(-el), np.inf)
    r = np.minimum(wall, ground)
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el),
                    rng.uniform(0.0, 1.0, m)], axis=1)
    return pts.astype(np.float32)


def make_scans(seed, sizes):
    """(points [sum(sizes), 4] float32, offsets [len(sizes) + 1] int64) of seeded scans."""
    rng = np.random.default_rng(seed)
    scans = [make_scan(rng, m) for m in sizes]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return (np.concatenate(scans) if scans else np.zeros((0, 4), np.float32)), offsets


def _project(pts, p, dt):
    """x, y, zc, u, v of md2.h steps 1-2 in dtype ``dt``."""
    X, Y, Z = (pts[:, k].astype(dt) for k in range(3))
    p = p.reshape(12).astype(dt)
    with np.errstate(all="ignore"):             # NaN, inf and zc = 0 are inputs the tests feed on purpose
        x = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3]
        y = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7]
        zc = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11]
        return X, zc, x / zc, y / zc


def _kept_before_pixel_test(X, zc, s, forward_only):
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(s) & (s > 0) & np.isfinite(zc) & (zc > 0)
        if forward_only:
            keep &= ~(X < 0)
    return keep


def lidar_depth_ref(points, offsets, P, h, w, forward_only=True, vel_depth=False, dtype=np.float32):
    """(depth [n, h, w] ``dtype``, counts [n, 2] int32) as include/md2.h defines them."""
    dt = np.dtype(dtype).type
    n = len(offsets) - 1
    P = np.broadcast_to(np.asarray(P, dtype=np.float32), (n, 3, 4))
    depth = np.zeros((n, h, w), dtype=dt)
    counts = np.zeros((n, 2), dtype=np.int32)
    for i in range(n):
        pts = points[offsets[i]:offsets[i + 1]]
        X, zc, u, v = _project(pts, P[i], dt)
        s = X if vel_depth else zc
        with np.errstate(invalid="ignore"):
            ru, rv = np.rint(u), np.rint(v)
            # the pixel test on the rounded floats (false for NaN), before any conversion to int
            keep = _kept_before_pixel_test(X, zc, s, forward_only) & (ru >= 1) & (ru <= w) & (rv >= 1) & (rv <= h)
        ix, iy = ru[keep].astype(np.int64) - 1, rv[keep].astype(np.int64) - 1
        flat = np.full(h * w, np.inf, dtype=dt)
        np.minimum.at(flat, iy * w + ix, s[keep])
        flat[np.isinf(flat)] = 0
        depth[i] = flat.reshape(h, w)
        counts[i] = (int(keep.sum()), int((flat != 0).sum()))
    return depth, counts


def dirty_pixels(points, offsets, P, h, w, forward_only=True, vel_depth=False, margin=MARGIN_PX):
    """bool [n, h, w]: the pixels a point within ``margin`` px of a rounding boundary (a half-integer
    u or v, in float64) could reach -- where float32 and float64 may legitimately disagree."""
    n = len(offsets) - 1
    P = np.broadcast_to(np.asarray(P, dtype=np.float32), (n, 3, 4))
    dirty = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        pts = points[offsets[i]:offsets[i + 1]]
        X, zc, u, v = _project(pts, P[i], np.float64)
        keep = _kept_before_pixel_test(X, zc, X if vel_depth else zc, forward_only) & np.isfinite(u) & np.isfinite(v)
        u, v = u[keep], v[keep]
        near = (np.abs(u - np.floor(u) - 0.5) < margin) | (np.abs(v - np.floor(v) - 0.5) < margin)
        u, v = u[near], v[near]
        for du in (-margin, margin):
            for dv in (-margin, margin):
                ru, rv = np.rint(u + du), np.rint(v + dv)
                ok = (ru >= 1) & (ru <= w) & (rv >= 1) & (rv <= h)
                dirty[i, rv[ok].astype(np.int64) - 1, ru[ok].astype(np.int64) - 1] = True
    return dirty


def post_process_ref(disp, disp_flipped, dtype=np.float32):
    """md2_disp_post_process on [..., h, w] arrays, in ``dtype``."""
    dt = np.dtype(dtype).type
    w = disp.shape[-1]
    x = np.arange(w).astype(dt)
    t = x / dt(w - 1) if w > 1 else np.zeros(w, dtype=dt)
    ml = dt(1) - np.minimum(np.maximum(dt(20) * (t - dt(np.float32(0.05))), dt(0)), dt(1))
    mr = ml[::-1]
    l, r = disp.astype(dt), disp_flipped.astype(dt)[..., ::-1]
    return (mr * l + ml * r) + ((dt(1) - ml) - mr) * (dt(0.5) * (l + r))
