"""CPU checks of the occupancy grid: the host's scan-pose computation (axis conventions) against numpy, and the numpy reference of
INTEGRATION.md on cases small enough to write down by hand."""
import numpy as np
import pytest

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
