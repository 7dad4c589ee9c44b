"""The occupancy-grid build on planted integer rays: every slope and tile residue, boxes of more than 1024 tiles, a hot tile split
at its exact boundaries, cells next to +-2^28, windows that rays miss, graze or cross, more rays than one pass of the binning
kernel takes, and small builds after large ones.  Every check is `info ==` and every grid byte against the numpy reference.

The rays are planted as `occupancy_cases` describes: with res = 1 and an axis-aligned pose, an integer geometry row is the offset of
the end cell.  The tests rely on the geometry table not being validated as unit vectors."""
import numpy as np
import pytest

import occupancy_cases as C
from occupancy_cases import Session, pose_array

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(320, 240, 500, 1.2, 3, max_images=2)
    yield c
    c.close()


@pytest.fixture
def session(hiplib, ctx):
    s = Session(hiplib, ctx)
    yield s
    s.drop_all()


def tiles(info):
    return info["width"] // 64, info["height"] // 64


def test_lattice_every_slope_and_tile_residue(hiplib, session):
    """A: against both references, and cut by a 128-cell window"""
    puts, poses = C.lattice_case()
    session.load(puts)
    poses = pose_array(hiplib, poses)
    _, info = session.check(poses, res=1.0)
    assert info["rays"] == 99405 and (info["width"], info["height"]) == (512, 448)
    session.check(poses, res=1.0, clipped=True)
    session.check(poses, res=1.0, max_side=128)


@pytest.mark.parametrize("origins, max_side, want_tiles", [
    ([(1024, 1024), (1088, 1024)], 4096, (33, 32)),      # 1056 tiles: two per scan thread, the tail threads idle
    ([(1024, 1024), (1040, 1010)], 4096, (32, 32)),      # exactly one tile per scan thread
    ([(1024, 1024), (1040, 1010)], 64, (1, 1)),          # one tile, every ray cut to it
])
def test_more_than_1024_tiles(hiplib, session, origins, max_side, want_tiles):
    """B: a fan of 1000-cell rays at integer slopes.  (1000 and not more: a full fan spans 2 da + 1 cells and has to fit the 32
    tiles of the smaller side.)"""
    puts, poses = C.fan_case(origins)
    session.load(puts)
    _, info = session.check(pose_array(hiplib, poses), res=1.0, max_side=max_side, clipped=True)
    assert tiles(info) == want_tiles and info["rays"] == 2 * len(puts[0][1]) and info["cell_visits"] > 0


def test_1100_cell_fan_cut_to_1024_tiles(hiplib, session):
    """B: the fan at da = 1100 is wider than 32 tiles; a 2048-cell window cuts it to 32 x 32"""
    puts, poses = C.fan_case([(1024, 1024), (1088, 1030)], da=1100)
    session.load(puts)
    _, info = session.check(pose_array(hiplib, poses), res=1.0, max_side=2048, clipped=True)
    assert tiles(info) == (32, 32)


def test_split_tile_boundaries_and_reuse(hiplib, session):
    """C: a tile of exactly 16384, 16385, 32768 and 32769 segments (SPLIT_BEAMS mirrors kChunkSegs: one, two, two and three
    chunks); two split tiles with a lightly hit tile between them; then the small build after the large one and the large one
    again, over the buffers the large one left"""
    session.load(C.split_puts())
    for n in (C.SPLIT_BEAMS, C.SPLIT_BEAMS + 1, 2 * C.SPLIT_BEAMS, 2 * C.SPLIT_BEAMS + 1):
        _, info = session.check(pose_array(hiplib, C.split_poses(n)), res=1.0)
        assert info["rays"] == n and tiles(info) == (1, 1)      # (every ray is one segment of the one tile)
    large = pose_array(hiplib, C.two_hot_poses())
    ref_large = session.reference(large, res=1.0)
    _, info = session.compare(large, ref_large, res=1.0)
    assert tiles(info)[0] >= 5 and info["rays"] == 3 * C.SPLIT_BEAMS + 11000
    session.check(pose_array(hiplib, C.split_poses(C.SPLIT_BEAMS)), res=1.0)
    session.compare(large, ref_large, res=1.0)


@pytest.mark.parametrize("cell", C.FAR_WINDOWS)
def test_far_cells(hiplib, session, cell):
    """D: rays of 2^29 - 4 cells between the corners of the admitted range, and a beam on either side of the +-2^28 limit, seen
    through a 256-cell window in the middle and at the far corners"""
    session.load(C.far_puts())
    _, info = session.check(pose_array(hiplib, C.far_poses(cell)), res=1.0, max_side=256, clipped=True)
    assert tiles(info) == (4, 4) and info["rays"] == 7 + 7 + 2 + 2 + 4 + 1 and info["cell_visits"] > 256


@pytest.mark.parametrize("side", [64, 128])
def test_windows(hiplib, session, side):
    """E: rays that all miss the window; rays on its corner cells, across it and of zero length"""
    puts, poses = C.window_case_planted(side, C.missing_rays(side))
    session.load(puts)
    grid, info = session.check(pose_array(hiplib, poses), res=1.0, max_side=side, clipped=True)
    assert info["rays"] == len(C.missing_rays(side)) > 0 and info["cell_visits"] == 0 and (grid == -1).all()
    assert (info["x0"], info["y0"], info["width"], info["height"]) == (0, 0, side, side)
    session.drop_all()
    puts, poses = C.window_case_planted(side, C.window_rays(side))
    session.load(puts)
    grid, info = session.check(pose_array(hiplib, poses), res=1.0, max_side=side)
    assert (info["x0"], info["y0"], info["width"], info["height"]) == (0, 0, side, side)
    assert all(grid[y, x] >= 0 for x in (0, side - 1) for y in (0, side - 1))
    session.check(pose_array(hiplib, poses), res=1.0, max_side=side, clipped=True)


def test_more_rays_than_one_pass_of_the_binning(hiplib, session):
    """F: 66 poses of one stored scan of 65536 beams"""
    puts, poses = C.stride_case()
    session.load(puts)
    _, info = session.check(pose_array(hiplib, poses), res=1.0, clipped=True)
    assert info["rays"] == C.STRIDE_BEAMS * C.STRIDE_POSES > 16384 * 256
