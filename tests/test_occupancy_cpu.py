"""CPU checks of the occupancy grid: the host's scan-pose computation (axis conventions) against numpy, and the numpy reference of
INTEGRATION.md on cases small enough to write down by hand."""
import numpy as np
import pytest

import occupancy_cases as C
import occupancy_ref as R

A = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)      # optical (x right, y down, z fwd) -> lpslam (x up, y right, z fwd)


def rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.fixture(scope="module")
def mgr():
    from lpslam_amd import _build, manager
    _build.host_library()
    return manager


def test_scan_pose_matches_numpy(mgr):
    rng = np.random.default_rng(5)
    for _ in range(50):
        Rcw, tcw = rot(rng), rng.normal(size=3) * 3
        Rcl, tcl = rot(rng), rng.normal(size=3) * 0.3
        T = np.eye(4); T[:3, :3] = Rcw; T[:3, 3] = tcw
        origin, fwd, left = mgr.scan_pose(T, mgr.laser_state(Rcl, tcl))
        Rwc = Rcw.T; C = -Rcw.T @ tcw
        Rwl = (A @ Rwc @ A.T) @ Rcl
        twl = (A @ Rwc @ A.T) @ tcl + A @ C
        assert np.allclose(origin, twl[1:], atol=1e-12)
        assert np.allclose(fwd, (Rwl @ [0, 0, 1])[1:], atol=1e-12)
        assert np.allclose(left, (Rwl @ [0, -1, 0])[1:], atol=1e-12)


def test_scan_pose_axes(mgr):
    """identity camera and laser: the laser looks along world z (map +y), its left is world -y (map -x); a camera moved 2 m to its
    right (optical +x) puts the laser at map x = 2; an invalid laser transform is the identity"""
    s = mgr.laser_state(np.eye(3), [0, 0, 0])
    o, f, l = mgr.scan_pose(np.eye(4), s)
    assert np.allclose(o, 0) and np.allclose(f, [0, 1]) and np.allclose(l, [-1, 0])
    T = np.eye(4); T[0, 3] = -2.0                          # T_cw: camera centre at optical x = +2
    o, f, l = mgr.scan_pose(T, s)
    assert np.allclose(o, [2, 0])
    bad = mgr.laser_state(np.eye(3), [5, 5, 5]); bad.valid = False
    o, _, _ = mgr.scan_pose(np.eye(4), bad)
    assert np.allclose(o, 0)
    # a laser mounted 0.5 m forward and yawed 90 degrees to the right (about lpslam x, up): it looks along world +y (map +x), its
    # left is world +z (map +y)
    c = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], np.float64)      # R_cl: laser z -> camera +y
    o, f, l = mgr.scan_pose(np.eye(4), mgr.laser_state(c, [0, 0, 0.5]))
    assert np.allclose(o, [0, 0.5]) and np.allclose(f, [1, 0]) and np.allclose(l, [0, 1])


def one_beam(ang, rng_m, origin=(0.0, 0.0), rmax=10.0, thr=9.0, res=0.05, max_side=4096):
    cs = np.array([[np.cos(ang), np.sin(ang)]])
    scans = {0: (cs, np.array([rng_m], np.float32), 0.0, rmax, thr)}
    return R.build(scans, [(0, origin, (0.0, 1.0), (-1.0, 0.0))], res, max_side, with_counts=True)


def test_reference_single_horizontal_ray():
    # beam 0 along fwd = map +y; 0.52 m at 5 cm: cells y = 0 .. 10, hit in cell 10
    g, info, hits, misses = one_beam(0.0, 0.52, origin=(0.01, 0.01))
    assert info["x0"] == 0 and info["y0"] == 0 and info["width"] == 64 and info["height"] == 64
    assert info["rays"] == 1 and info["cell_visits"] == 11
    assert (misses[0:10, 0] == 1).all() and hits[10, 0] == 1 and hits.sum() == 1 and misses.sum() == 10
    assert g[10, 0] == 100 and (g[0:10, 0] == 0).all() and (g == -1).sum() == 64 * 64 - 11


def test_reference_45_degree_ray_and_ties():
    # beam at +90 degrees = left = map -x; 45 degrees: dx == dy, x is the major axis, minor steps every cell
    c = np.sqrt(0.5)
    scans = {0: (np.array([[c, c]]), np.array([0.3 * np.sqrt(2)], np.float32), 0.0, 10.0, 9.0)}
    g, info, hits, misses = R.build(scans, [(0, (0.025, 0.025), (0.0, 1.0), (-1.0, 0.0))], 0.05, 4096, with_counts=True)
    # end point (0.025 - 0.3, 0.025 + 0.3) -> cell (-6, 6): visits (0,0), (-1,1), ..., (-6,6)
    assert info["x0"] == -64 and info["y0"] == 0 and info["cell_visits"] == 7
    for k in range(7):
        assert hits[k, 64 - k] + misses[k, 64 - k] == 1
    assert hits[6, 58] == 1
    # a shallow ray with a rounding tie: dx = 4, dy = 1 -> q(k) = (2k + 4) div 8 = 0, 0, 1, 1, 1
    scans = {0: (np.array([[1.0, 0.0]]), np.array([0.21], np.float32), 0.0, 10.0, 9.0)}
    _, _, h2, m2 = R.build(scans, [(0, (0.01, 0.01), (4 / np.sqrt(17), 1 / np.sqrt(17)), (-1 / np.sqrt(17), 4 / np.sqrt(17)))], 0.05, 4096, with_counts=True)
    visited = sorted(zip(*np.nonzero(h2 + m2)))
    assert visited == [(0, 0), (0, 1), (1, 2), (1, 3), (1, 4)]


def test_reference_snapping_and_free_beams():
    # a free beam (range above the threshold) stops at min(threshold, range_max) and counts misses only
    g, info, hits, misses = one_beam(0.0, 50.0, origin=(-0.01, -0.01), rmax=10.0, thr=3.0)
    assert hits.sum() == 0 and info["cell_visits"] == 61          # cells y = -1 .. 59
    assert info["x0"] == -64 and info["y0"] == -64 and info["width"] == 64 and info["height"] == 128
    # a side longer than max_side: re-centred on the last pose's origin cell, snapped down to 64
    g, info, _, _ = one_beam(0.0, 9.0, origin=(0.0, 0.0), rmax=10.0, thr=9.5, max_side=64)
    assert info["height"] == 64 and info["y0"] == -64 and info["width"] == 64 and info["x0"] == 0
    # skipped beams: NaN, below range_min; an origin cell beyond 2^28 cells
    cs = np.array([[1.0, 0.0]] * 3)
    scans = {0: (cs, np.array([np.nan, 0.01, 1.0], np.float32), 0.1, 10.0, 9.0)}
    _, info = R.build(scans, [(0, (0.0, 0.0), (0.0, 1.0), (-1.0, 0.0))], 0.05, 4096)
    assert info["rays"] == 1
    _, info = R.build(scans, [(0, (2.0 ** 29 * 0.05, 0.0), (0.0, 1.0), (-1.0, 0.0))], 0.05, 4096)
    assert info["rays"] == 0 and info["width"] == 0


# ---- the second reference: build_clipped against build, against shifted inputs and against a plain integer loop -----------------
def same(a, b):
    assert a[1] == b[1], (a[1], b[1])
    assert a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes()
    for u, v in zip(a[2:], b[2:]):                   # (with_counts: hits and misses)
        assert (u is None and v is None) or np.array_equal(u, v)


def both(puts, poses, res, max_side):
    scans = C.as_scans(puts)
    a = R.build(scans, poses, res, max_side, with_counts=True)
    same(R.build_clipped(scans, poses, res, max_side, with_counts=True), a)
    return a


def test_clipped_equals_build_on_hand_cases():
    c = np.sqrt(0.5)
    up, lf = (0.0, 1.0), (-1.0, 0.0)
    one = lambda cs, r, rmax=10.0, thr=9.0, rmin=0.0: [(0, np.array(cs, np.float64), np.array(r, np.float32), rmin, rmax, thr)]
    both(one([[1.0, 0.0]], [0.52]), [(0, (0.01, 0.01), up, lf)], 0.05, 4096)
    both(one([[c, c]], [0.3 * np.sqrt(2)]), [(0, (0.025, 0.025), up, lf)], 0.05, 4096)
    both(one([[1.0, 0.0]], [0.21]), [(0, (0.01, 0.01), (4 / np.sqrt(17), 1 / np.sqrt(17)), (-1 / np.sqrt(17), 4 / np.sqrt(17)))], 0.05, 4096)
    both(one([[1.0, 0.0]], [50.0], thr=3.0), [(0, (-0.01, -0.01), up, lf)], 0.05, 4096)
    both(one([[1.0, 0.0]], [9.0], thr=9.5), [(0, (0.0, 0.0), up, lf)], 0.05, 64)
    skipped = one([[1.0, 0.0]] * 3, [np.nan, 0.01, 1.0], rmin=0.1)
    assert both(skipped, [(0, (0.0, 0.0), up, lf)], 0.05, 4096)[1]["rays"] == 1
    assert both(skipped, [(0, (2.0 ** 29 * 0.05, 0.0), up, lf)], 0.05, 4096)[1]["width"] == 0
    assert both(skipped, [], 0.05, 4096)[1]["width"] == 0


def test_clipped_equals_build_on_shared_cases():
    puts, poses = C.edge_beam_case()
    both(puts, poses[:3], C.RES, 4096)
    both(puts, poses, C.RES, 4096)
    both(puts, poses, C.RES, 64)
    puts, poses = C.window_case()
    assert both(puts, poses, C.RES, 256)[1]["width"] == 256
    both(puts, poses, C.RES, 4096)


def test_clipped_equals_build_on_lattice():
    puts, poses = C.lattice_case()
    _, info, hits, misses = both(puts, poses, 1.0, 4096)
    assert info["rays"] == 99405 and (info["width"], info["height"]) == (512, 448)
    both(puts, poses, 1.0, 128)


def test_clipped_equals_build_on_long_rays_in_a_small_window():
    puts = [C.planted_put(1, C.fan_rows(300, np.random.default_rng(21), 30))]
    poses = [C.planted_pose(1, c) for c in [(0, 0), (-37, 90), (150, -20), (20, 17)]]
    _, info, _, _ = both(puts, poses, 1.0, 128)
    assert info["width"] == 128 and info["height"] == 128 and info["cell_visits"] > 0
    both(puts, poses[::-1], 1.0, 128)
    both(puts, poses, 1.0, 64)
    for side in (64, 128):
        both(*C.window_case_planted(side, C.window_rays(side)), 1.0, side)
        both(*C.window_case_planted(side, C.missing_rays(side)), 1.0, side)


def test_window_cases_are_what_they_say():
    for side in (64, 128):
        puts, poses = C.window_case_planted(side, C.missing_rays(side))
        g, info = R.build_clipped(C.as_scans(puts), poses, 1.0, side)
        assert (info["x0"], info["y0"], info["width"], info["height"]) == (0, 0, side, side)
        assert info["rays"] == len(C.missing_rays(side)) and info["cell_visits"] == 0 and (g == -1).all()
        S = side
        for cx, cy, ox, oy in [(0, 0, -1, -1), (S - 1, 0, 1, -1), (0, S - 1, -1, 1), (S - 1, S - 1, 1, 1)]:
            ray = (cx + 3 * ox, cy - 3 * oy, cx - 3 * ox, cy + 3 * oy, 0)
            assert ray in C.window_rays(side)
            far = [(-200, -200, -200, -200, 0), (S + 200, S + 200, S + 200, S + 200, 0)]      # (the box must be wider than the window)
            puts, poses = C.window_case_planted(side, [ray] + far)
            g, info, hits, misses = R.build_clipped(C.as_scans(puts), poses, 1.0, side, with_counts=True)
            assert info["cell_visits"] == 1 and misses[cy, cx] == 1 and (info["x0"], info["width"]) == (0, side)


@pytest.mark.parametrize("m", [(1, 0), (0, -1), (-3, 7), (4000000, -4000000), (-4194290, 4194290), (4194290, 1)])
def test_translation_invariance(m):
    """origins shifted by whole tiles: the same bytes, x0 / y0 shifted; against `build` run near zero"""
    puts, poses = C.lattice_case()
    puts = [(k, cs[::7], r[::7]) + tuple(rest) for k, cs, r, *rest in puts]
    near = R.build(C.as_scans(puts), poses, 1.0, 4096, with_counts=True)
    sx, sy = 64 * m[0], 64 * m[1]
    assert max(abs(sx), abs(sy)) + 64 + 140 < 2 ** 28      # (the lattice reaches 140 cells from origin cells within +-64)
    far_poses = [(k, (o[0] + sx, o[1] + sy), f, l) for k, o, f, l in poses]
    far = R.build_clipped(C.as_scans(puts), far_poses, 1.0, 4096, with_counts=True)
    info = dict(far[1]); info["x0"] -= sx; info["y0"] -= sy
    same((far[0], info) + far[2:], near)
    # and in a window that cuts rays
    near = R.build(C.as_scans(puts), poses, 1.0, 128)
    far = R.build_clipped(C.as_scans(puts), far_poses, 1.0, 128)
    info = dict(far[1]); info["x0"] -= sx; info["y0"] -= sy
    same((far[0], info), near)


def int_loop(recs, lo, hi):
    """the traversal over the box's major range per ray in Python integers (arbitrary precision, no numpy)"""
    W, H = hi[0] - lo[0], hi[1] - lo[1]
    hits, misses = [0] * (W * H), [0] * (W * H)
    for gx0, gy0, gx1, gy1, hit in recs:
        dx, dy = abs(gx1 - gx0), abs(gy1 - gy0)
        sx, sy = (gx1 > gx0) - (gx1 < gx0), (gy1 > gy0) - (gy1 < gy0)
        xmaj = dx >= dy
        a0, b0, sa, sb, da, db = (gx0, gy0, sx, sy, dx, dy) if xmaj else (gy0, gx0, sy, sx, dy, dx)
        alo, ahi = (lo[0], hi[0]) if xmaj else (lo[1], hi[1])
        for a in range(alo, ahi):
            k = (a - a0) * sa if sa else (0 if a == a0 else -1)
            if k < 0 or k > da:
                continue
            b = b0 + sb * ((2 * k * db + da) // (2 * da)) if da else b0
            x, y = (a, b) if xmaj else (b, a)
            if lo[0] <= x < hi[0] and lo[1] <= y < hi[1]:
                (hits if hit and k == da else misses)[(y - lo[1]) * W + (x - lo[0])] += 1
    return hits, misses


@pytest.mark.parametrize("cell", C.FAR_WINDOWS)
def test_far_rays_against_integer_loop(cell):
    puts, poses = C.far_puts(), C.far_poses(cell)
    g, info, hits, misses = R.build_clipped(C.as_scans(puts), poses, 1.0, 256, with_counts=True)
    lo = [int(R.floor64(cell[0] - 128)), int(R.floor64(cell[1] - 128))]
    assert (info["x0"], info["y0"], info["width"], info["height"]) == (lo[0], lo[1], 256, 256)
    gx0, gy0, gx1, gy1, ok, hit = C.expected_records(puts, poses)
    recs = [tuple(int(v) for v in r) for r in zip(gx0[ok], gy0[ok], gx1[ok], gy1[ok], hit[ok])]
    assert info["rays"] == len(recs) == 7 + 7 + 2 + 2 + 4 + 1
    h, m = int_loop(recs, lo, [lo[0] + 256, lo[1] + 256])
    assert hits.reshape(-1).tolist() == h and misses.reshape(-1).tolist() == m
    assert info["cell_visits"] == sum(h) + sum(m) > 256


def test_planting_is_exact():
    """ray_records returns exactly the intended integer cells for every planted case"""
    cases = [C.lattice_case(), C.fan_case([(1024, 1024), (1088, 1024)]), (C.split_puts(), C.two_hot_poses()), C.stride_case(),
             C.window_case_planted(128, C.window_rays(128) + C.missing_rays(128))] + [(C.far_puts(), C.far_poses(c)) for c in C.FAR_WINDOWS]
    for puts, poses in cases:
        scans = C.as_scans(puts)
        want = C.expected_records(puts, poses)
        got = [R.ray_records(*scans[key], origin, fwd, left, 1.0) for key, origin, fwd, left in poses]
        for i in range(6):
            assert np.array_equal(np.concatenate([g[i] for g in got]), want[i])


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("axis", [0, 1])
def test_skip_rule_at_the_limit(sign, axis):
    """a pre-floor end coordinate of 2^28 - 0.5 is counted, 2^28 and 2^28 + 0.5 are skipped; the same at -2^28"""
    ends = [2.0 ** 28 - 0.5, 2.0 ** 28, 2.0 ** 28 + 0.5]
    o = 1000.5
    rows = np.zeros((3, 2))
    rows[:, axis] = [sign * e - o for e in ends]
    rows[:, 1 - axis] = 4
    k, cs, r, rmin, rmax, rthr = C.planted_put(1, rows)
    gx0, gy0, gx1, gy1, ok, hit = R.ray_records(cs, r, rmin, rmax, rthr, (o, o), (1.0, 0.0), (0.0, 1.0), 1.0)
    assert ok.tolist() == [True, False, False] and hit.tolist() == [True, False, False]
    end = (gx1, gy1)[axis][0]
    assert end == (2 ** 28 - 1 if sign > 0 else -2 ** 28) and (gx1, gy1)[1 - axis][0] == 1004
    # the origin's coordinate under the same rule
    for e, counted in zip(ends, [True, False, False]):
        origin = [o, o]; origin[axis] = sign * e
        ok = R.ray_records(np.zeros((1, 2)), np.array([1.0], np.float32), 0.0, 2.0, 2.0, origin, (1.0, 0.0), (0.0, 1.0), 1.0)[4]
        assert bool(ok[0]) == counted
