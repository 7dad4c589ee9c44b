"""The occupancy-grid build of the C ABI (lpslam_hip_scan_* / lpslam_hip_occupancy_build) against the numpy reference of
INTEGRATION.md, byte for byte."""
import numpy as np
import pytest

import occupancy_ref as R
from occupancy_cases import RES, Session, edge_beam_case, pose_array, pose_rec, window_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(320, 240, 500, 1.2, 3, max_images=2)
    yield c
    c.close()


def room_ranges(origin, yaw, cs, walls):
    """ray-cast against a polygon (list of vertices, map plane); beams in the laser frame from cs"""
    o = np.asarray(origin, np.float64)
    fwd = np.array([np.sin(yaw), np.cos(yaw)]); left = np.array([-fwd[1], fwd[0]])
    d = cs[:, :1] * fwd + cs[:, 1:] * left
    best = np.full(len(cs), np.inf)
    for a, b in zip(walls, walls[1:] + walls[:1]):
        a = np.asarray(a, np.float64); e = np.asarray(b, np.float64) - a
        den = d[:, 0] * e[1] - d[:, 1] * e[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((a[0] - o[0]) * e[1] - (a[1] - o[1]) * e[0]) / den
            u = ((a[0] - o[0]) * d[:, 1] - (a[1] - o[1]) * d[:, 0]) / den
        ok = (np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1)
        best = np.where(ok & (t < best), t, best)
    return best.astype(np.float32)


def test_room_scans(hiplib, ctx):
    rng = np.random.default_rng(1)
    s = Session(hiplib, ctx)
    room = [(-3.0, -2.0), (4.0, -2.5), (5.0, 3.0), (1.0, 4.5), (-2.5, 3.5)]
    cs = R.beam_table(720, -np.pi, 2 * np.pi / 720)
    poses = []
    for key in range(64):
        o = rng.uniform([-1.5, -1.0], [3.0, 2.5]); yaw = rng.uniform(-np.pi, np.pi)
        r = room_ranges(o, yaw, cs, room) + rng.normal(0, 0.01, len(cs)).astype(np.float32)
        s.put(key, cs, r, 0.1, 8.0, 7.5)
        poses.append(pose_rec(hiplib, key, o, yaw))
    grid, info = s.check(np.concatenate(poses))
    assert info["rays"] > 40000 and (grid >= 50).sum() > 200 and (grid == 0).sum() > 2000


def test_edge_beams(hiplib, ctx):
    s = Session(hiplib, ctx)
    puts, poses = edge_beam_case()
    poses = pose_array(hiplib, poses)
    s.load(puts[:2])
    s.check(poses[:3])
    # range_threshold above range_max, and a beam length of exactly zero
    s.load(puts[2:])
    s.check(poses)


def test_max_side_window_cuts_rays(hiplib, ctx):
    s = Session(hiplib, ctx)
    puts, poses = window_case()
    s.load(puts)
    grid, info = s.check(pose_array(hiplib, poses), max_side=256)
    assert info["width"] == 256 and info["height"] == 256


def test_one_origin_counts_above_16_bits(hiplib, ctx):
    s = Session(hiplib, ctx)
    cs = R.beam_table(181, -np.pi / 2, np.pi / 180)
    rng = np.random.default_rng(3)
    poses = []
    for key in range(500):
        s.put(1000 + key, cs, rng.uniform(0.3, 1.5, 181).astype(np.float32), 0.1, 2.0, 1.9)
        poses.append(pose_rec(hiplib, 1000 + key, (0.51, 0.49), key * 0.013))
    poses = np.concatenate(poses)
    scans = s.scans
    _, _, hits, misses = R.build(scans, [(int(p["key"]), p["origin"], p["fwd"], p["left"]) for p in poses], RES, 4096, with_counts=True)
    assert (hits + misses).max() > 65535
    s.check(poses)


def test_drop_and_replace(hiplib, ctx):
    s = Session(hiplib, ctx)
    cs = R.beam_table(90, -np.pi / 4, np.pi / 180)
    s.put(500, cs, np.full(90, 2.0, np.float32), 0.1, 10.0, 9.0)
    s.put(501, cs, np.full(90, 3.0, np.float32), 0.1, 10.0, 9.0)
    both = np.concatenate([pose_rec(hiplib, 500, (0, 0), 0.0), pose_rec(hiplib, 501, (1, 1), 1.0)])
    g_both, _ = s.check(both)
    s.drop(501)
    with pytest.raises(hiplib.LpslamHipError):
        ctx.occupancy_build(both, RES, 4096)
    s.check(both[:1])
    s.put(500, cs, np.full(90, 1.0, np.float32), 0.1, 10.0, 9.0)      # replaced
    g_new, _ = s.check(both[:1])
    assert g_new.shape != g_both.shape or not np.array_equal(g_new, g_both[: g_new.shape[0], : g_new.shape[1]])


def test_sizing_repeat_and_errors(hiplib, ctx):
    s = Session(hiplib, ctx)
    cs = R.beam_table(270, -np.pi * 0.75, np.pi / 180 * 1.5 / 1.5)
    rng = np.random.default_rng(4)
    poses = []
    for key in range(20):
        s.put(2000 + key, cs, rng.uniform(0.5, 6.0, 270).astype(np.float32), 0.1, 8.0, 7.0)
        poses.append(pose_rec(hiplib, 2000 + key, rng.uniform(-2, 2, 2), rng.uniform(-3, 3)))
    poses = np.concatenate(poses)
    _, sized = ctx.occupancy_build(poses, RES, 4096, sizing=True)
    g1, i1 = s.check(poses)
    assert sized == i1
    g2, i2 = ctx.occupancy_build(poses, RES, 4096)
    assert i2 == i1 and g1.tobytes() == g2.tobytes()
    cells = i1["width"] * i1["height"]
    # too small a buffer: error, nothing written
    buf = np.full(cells - 1, 77, np.int8)
    with pytest.raises(hiplib.LpslamHipError):
        ctx.occupancy_build(poses, RES, 4096, out=buf)
    assert (buf == 77).all()
    # an unknown key: error, nothing written
    bad = poses.copy(); bad[3]["key"] = 99999
    buf = np.full(cells, 77, np.int8)
    with pytest.raises(hiplib.LpslamHipError):
        ctx.occupancy_build(bad, RES, 4096, out=buf)
    assert (buf == 77).all()
    # no poses: an empty grid
    g0, i0 = ctx.occupancy_build(poses[:0], RES, 4096)
    assert g0.size == 0 and i0["width"] == 0 and i0["rays"] == 0
