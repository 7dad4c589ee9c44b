"""numpy reference of the occupancy grid ("Occupancy grid"): the definition the device build must reproduce byte
for byte.  `build` steps all rays together (one numpy pass per step index k), so a few thousand rays of a few hundred cells take
well under a second; `build_clipped` takes per ray only the steps inside the box's major range, for rays of up to 2^29 cells,
boxes of thousands of tiles and millions of rays."""
import numpy as np

CELL_LIMIT = 2.0 ** 28      # a beam whose origin or end cell is not inside (-2^28, 2^28) is skipped


def floor64(v):
    return (np.asarray(v, np.int64) // 64) * 64


def beam_table(n, angle_min, increment):
    """(n, 2) float64: cos a, sin a of a = angle_min + i * increment (in double, as the host computes it)"""
    a = np.float64(angle_min) + np.arange(n, dtype=np.float64) * np.float64(increment)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def ray_records(cos_sin, ranges, rmin, rmax, rthr, origin, fwd, left, inv_res):
    """per beam: gx0, gy0, gx1, gy1 (int64), counted (bool), hit (bool)"""
    r = np.asarray(ranges, np.float32).astype(np.float64)
    rmin, rmax, rthr = (np.float64(np.float32(v)) for v in (rmin, rmax, rthr))
    ox, oy = np.float64(origin[0]), np.float64(origin[1])
    fx, fy = np.float64(fwd[0]), np.float64(fwd[1])
    lx, ly = np.float64(left[0]), np.float64(left[1])
    oxc, oyc = ox * inv_res, oy * inv_res
    origin_ok = abs(oxc) < CELL_LIMIT and abs(oyc) < CELL_LIMIT
    gx0 = int(np.floor(oxc)) if origin_ok else 0
    gy0 = int(np.floor(oyc)) if origin_ok else 0
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(r) & ~(r < rmin) & origin_ok
        hit = (r < rthr) & (r <= rmax)
        L = np.where(hit, r, rthr if rthr < rmax else rmax)
        c, s = cos_sin[:, 0], cos_sin[:, 1]
        ex = ox + L * (c * fx + s * lx)
        ey = oy + L * (c * fy + s * ly)
        exc, eyc = ex * inv_res, ey * inv_res
        ok &= (np.abs(exc) < CELL_LIMIT) & (np.abs(eyc) < CELL_LIMIT)
        gx1 = np.where(ok, np.floor(np.where(ok, exc, 0)), gx0).astype(np.int64)
        gy1 = np.where(ok, np.floor(np.where(ok, eyc, 0)), gy0).astype(np.int64)
    n = len(r)
    return np.full(n, gx0, np.int64), np.full(n, gy0, np.int64), gx1, gy1, ok, hit & ok


def build(scans, poses, res, max_side, with_counts=False):
    """scans: {key: (cos_sin, ranges, range_min, range_max, range_threshold)}; poses: sequence of (key, origin, fwd, left).
    Returns (grid int8 (height, width), info dict as lpslam_hip_grid_info); with_counts: also the hit and miss counts."""
    out = _build(scans, poses, res, max_side)
    return out if with_counts else out[:2]


def _rays_and_box(scans, poses, res, max_side):
    """the contract's FP64 part, shared by both traversals: the counted rays (gx0, gy0, gx1, gy1, hit) and the box (lo, hi);
    None when no beam is counted"""
    inv_res = 1.0 / np.float64(res)
    parts = []
    for key, origin, fwd, left in poses:
        cs, ranges, rmin, rmax, rthr = scans[key]
        parts.append(ray_records(cs, ranges, rmin, rmax, rthr, origin, fwd, left, inv_res))
    if not parts:
        return None
    gx0, gy0, gx1, gy1, ok, hit = (np.concatenate([p[i] for p in parts]) for i in range(6))
    gx0, gy0, gx1, gy1, hit = gx0[ok], gy0[ok], gx1[ok], gy1[ok], hit[ok]
    if len(gx0) == 0:
        return None
    lo = [int(floor64(min(gx0.min(), gx1.min()))), int(floor64(min(gy0.min(), gy1.min())))]
    hi = [int(floor64(max(gx0.max(), gx1.max()))) + 64, int(floor64(max(gy0.max(), gy1.max()))) + 64]
    last = poses[-1][1]
    for a in range(2):
        if hi[a] - lo[a] > max_side:
            v = np.float64(last[a]) * inv_res
            c = int(np.floor(np.clip(v, -CELL_LIMIT, CELL_LIMIT))) if np.isfinite(v) else 0
            lo[a] = int(floor64(c - max_side // 2))
            hi[a] = lo[a] + max_side
    return gx0, gy0, gx1, gy1, hit, lo, hi


def _empty():
    info = {"x0": 0, "y0": 0, "width": 0, "height": 0, "rays": 0, "cell_visits": 0}
    return np.zeros((0, 0), np.int8), info, None, None


def _finish(hits, misses, lo, W, H, n_rays):
    tot = hits + misses
    grid = np.where(tot == 0, -1, (100 * hits + tot // 2) // np.maximum(tot, 1)).astype(np.int8)
    info = {"x0": lo[0], "y0": lo[1], "width": W, "height": H, "rays": int(n_rays), "cell_visits": int(tot.sum())}
    return grid.reshape(H, W), info, hits.reshape(H, W), misses.reshape(H, W)


def _build(scans, poses, res, max_side):
    rb = _rays_and_box(scans, poses, res, max_side)
    if rb is None:
        return _empty()
    gx0, gy0, gx1, gy1, hit, lo, hi = rb
    W, H = hi[0] - lo[0], hi[1] - lo[1]
    hits = np.zeros(W * H, np.int64)
    misses = np.zeros(W * H, np.int64)
    dx, dy = np.abs(gx1 - gx0), np.abs(gy1 - gy0)
    sx, sy = np.sign(gx1 - gx0), np.sign(gy1 - gy0)
    xmaj = dx >= dy
    da = np.where(xmaj, dx, dy)
    db = np.where(xmaj, dy, dx)
    n = da
    order = np.argsort(-n, kind="stable")
    gx0, gy0, sx, sy, xmaj, da, db, n, hit = (v[order] for v in (gx0, gy0, sx, sy, xmaj, da, db, n, hit))
    den = np.maximum(2 * da, 1)
    neg_n = -n
    for k in range(int(n[0]) + 1):
        m = int(np.searchsorted(neg_n, -k, side="right"))      # rays with n >= k (a prefix: sorted by n descending)
        q = (2 * k * db[:m] + da[:m]) // den[:m]
        x = np.where(xmaj[:m], gx0[:m] + sx[:m] * k, gx0[:m] + sx[:m] * q)
        y = np.where(xmaj[:m], gy0[:m] + sy[:m] * q, gy0[:m] + sy[:m] * k)
        inb = (x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1])
        idx = (y - lo[1]) * W + (x - lo[0])
        is_hit = hit[:m] & (n[:m] == k)
        hits += np.bincount(idx[inb & is_hit], minlength=W * H)
        misses += np.bincount(idx[inb & ~is_hit], minlength=W * H)
    return _finish(hits, misses, lo, W, H, len(gx0))


def build_clipped(scans, poses, res, max_side, with_counts=False):
    """`build` with another traversal, for rays far longer than the box: per ray only the steps whose *major* coordinate lies in
    the box are taken (at most one box side of them), q(k) is evaluated forward for each and the minor coordinate tested.  Nothing
    here inverts q.  Same inputs and outputs as `build`."""
    out = _build_clipped(scans, poses, res, max_side)
    return out if with_counts else out[:2]


_CHUNK_STEPS = 1 << 22      # steps expanded at a time


def _build_clipped(scans, poses, res, max_side):
    rb = _rays_and_box(scans, poses, res, max_side)
    if rb is None:
        return _empty()
    gx0, gy0, gx1, gy1, hit, lo, hi = rb
    W, H = hi[0] - lo[0], hi[1] - lo[1]
    dx, dy = np.abs(gx1 - gx0), np.abs(gy1 - gy0)
    sx, sy = np.sign(gx1 - gx0), np.sign(gy1 - gy0)
    xmaj = dx >= dy
    da, db = np.where(xmaj, dx, dy), np.where(xmaj, dy, dx)
    a0, b0 = np.where(xmaj, gx0, gy0), np.where(xmaj, gy0, gx0)
    sa, sb = np.where(xmaj, sx, sy), np.where(xmaj, sy, sx)
    alo, ahi = np.where(xmaj, lo[0], lo[1]), np.where(xmaj, hi[0], hi[1])
    blo, bhi = np.where(xmaj, lo[1], lo[0]), np.where(xmaj, hi[1], hi[0])
    # every product below stays under 2^60 for admitted cells: -2^28 <= cell < 2^28, so da, db, k < 2^29 and 2 k db + da < 2^59 + 2^29
    assert max(int(np.abs(gx0).max()), int(np.abs(gy0).max()), int(np.abs(gx1).max()), int(np.abs(gy1).max())) <= 2 ** 28
    assert 2 * int(da.max()) * int(db.max()) + int(da.max()) < 2 ** 60
    # steps with the major coordinate a0 + sa k in [alo, ahi): sa = 0 only when da = 0 (the origin cell alone, k = 0)
    kfirst = np.where(sa > 0, alo - a0, np.where(sa < 0, a0 - (ahi - 1), np.where((a0 >= alo) & (a0 < ahi), 0, 1)))
    klast = np.where(sa > 0, ahi - 1 - a0, np.where(sa < 0, a0 - alo, 0))
    kfirst, klast = np.maximum(kfirst, 0), np.minimum(klast, da)
    cnt = np.maximum(klast - kfirst + 1, 0)
    assert int(cnt.max()) <= max(W, H)
    hits = np.zeros(W * H, np.int64)
    misses = np.zeros(W * H, np.int64)
    ends = np.cumsum(cnt)
    r0 = 0
    while r0 < len(cnt):
        done = int(ends[r0 - 1]) if r0 else 0
        r1 = max(int(np.searchsorted(ends, done + _CHUNK_STEPS, side="right")), r0 + 1)
        c = cnt[r0:r1]
        total = int(c.sum())
        if total:
            ray = np.repeat(np.arange(r0, r1), c)
            k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(c) - c, c) + kfirst[ray]
            q = (2 * k * db[ray] + da[ray]) // np.maximum(2 * da[ray], 1)
            a = a0[ray] + sa[ray] * k
            b = b0[ray] + sb[ray] * q
            assert ((a >= alo[ray]) & (a < ahi[ray])).all()
            inb = (b >= blo[ray]) & (b < bhi[ray])
            x, y = np.where(xmaj[ray], a, b), np.where(xmaj[ray], b, a)
            idx = (y - lo[1]) * W + (x - lo[0])
            is_hit = hit[ray] & (k == da[ray])
            hits += np.bincount(idx[inb & is_hit], minlength=W * H)
            misses += np.bincount(idx[inb & ~is_hit], minlength=W * H)
        r0 = r1
    return _finish(hits, misses, lo, W, H, len(gx0))
