"""Inputs of the occupancy-grid tests, shared by the CPU checks of the two numpy references and the device tests, and the device
tests' mirror of the scan store.

A case is `(puts, poses)`: `puts` a list of `(key, cos_sin, ranges, range_min, range_max, range_threshold)` as handed to the scan
store, `poses` a list of `(key, origin, fwd, left)` as `occupancy_ref.build` takes them.

Planted rays.  With `res = 1`, `fwd = (1, 0)`, `left = (0, 1)`, the origin at `(gx0 + 0.5, gy0 + 0.5)` and the limits
`(range_min, range_max, range_threshold) = (0, 2, 2)`, a geometry row `(u, v)` and range 1.0 give a hit whose end point is
`(gx0 + 0.5 + u, gy0 + 0.5 + v)`; range 3.0 gives a free beam of length 2 ending at `(gx0 + 0.5 + 2 u, gy0 + 0.5 + 2 v)`.  For
integer (or, for free beams, half-integer) rows every operation of the contract's end-point formula is exact in FP64, so the ray
record is exactly the intended pair of cells.  This relies on the geometry table not being validated as unit vectors."""
import numpy as np

import occupancy_ref as R

RES = 0.05
PLANT_LIMITS = (0.0, 2.0, 2.0)      # range_min, range_max, range_threshold of planted scans
HIT, FREE = np.float32(1.0), np.float32(3.0)
F = 2 ** 28 - 2                     # the far cell of case D


# ---- the device tests' mirror of the store ----------------------------------------------------------------------------------------
def pose_tuple(key, origin, yaw):
    fwd = np.array([np.sin(yaw), np.cos(yaw)])
    return (key, tuple(origin), fwd, np.array([-fwd[1], fwd[0]]))


def pose_rec(hip, key, origin, yaw):
    """a horizontal laser at `origin` (map plane) looking along yaw (counter-clockwise from map +y... any convention: fwd/left
    orthonormal and right-handed seen from above)"""
    p = np.zeros(1, hip.SCAN_POSE_DTYPE)
    p["key"] = key
    p["origin"] = origin
    fwd = np.array([np.sin(yaw), np.cos(yaw)])
    p["fwd"] = fwd
    p["left"] = [-fwd[1], fwd[0]]
    return p


def pose_array(hip, poses):
    p = np.zeros(len(poses), hip.SCAN_POSE_DTYPE)
    for i, (key, origin, fwd, left) in enumerate(poses):
        p[i]["key"] = key
        p[i]["origin"] = origin
        p[i]["fwd"] = fwd
        p[i]["left"] = left
    return p


class Session:
    """what was put into the store, mirrored for the reference"""

    def __init__(self, hip, ctx):
        self.hip, self.ctx, self.scans, self.geo = hip, ctx, {}, {}

    def put(self, key, cs, ranges, rmin, rmax, rthr):
        gkey = cs.tobytes()
        if gkey not in self.geo:
            self.geo[gkey] = self.ctx.scan_geometry_put(cs)
        self.ctx.scan_store_put(key, self.geo[gkey], ranges, rmin, rmax, rthr)
        self.scans[key] = (cs, np.asarray(ranges, np.float32), rmin, rmax, rthr)

    def load(self, puts):
        for p in puts:
            self.put(*p)

    def drop(self, key):
        self.ctx.scan_store_drop(key)
        self.scans.pop(key, None)

    def drop_all(self):
        for key in list(self.scans):
            self.drop(key)

    def reference(self, poses, max_side=4096, res=RES, clipped=False):
        ref = R.build_clipped if clipped else R.build
        return ref(self.scans, [(int(p["key"]), p["origin"], p["fwd"], p["left"]) for p in poses], res, max_side)

    def compare(self, poses, ref, max_side=4096, res=RES):
        ref_grid, ref_info = ref
        grid, info = self.ctx.occupancy_build(poses, res, max_side)
        assert info == ref_info, (info, ref_info)
        assert grid.shape == ref_grid.shape
        bad = np.argwhere(grid != ref_grid)
        assert len(bad) == 0, "%d cells differ, first %s: %d vs %d" % (len(bad), bad[0], grid[tuple(bad[0])], ref_grid[tuple(bad[0])])
        return grid, info

    def check(self, poses, max_side=4096, res=RES, clipped=False):
        return self.compare(poses, self.reference(poses, max_side, res, clipped), max_side, res)


def as_scans(puts):
    return {p[0]: (p[1], np.asarray(p[2], np.float32)) + tuple(p[3:]) for p in puts}


# ---- the inputs of test_edge_beams and test_max_side_window_cuts_rays ---------------------------------------------------------------
def edge_beam_case():
    """exact axis and 45-degree directions (ties of the closed form), beams that end in the origin cell, negative coordinates;
    puts[2] / poses[3]: range_threshold above range_max, and a beam length of exactly zero"""
    ang = np.array([0, np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, -np.pi / 4, -np.pi / 2, -3 * np.pi / 4] * 4)
    cs = np.stack([np.cos(ang), np.sin(ang)], 1)
    cs[0::8] = [1, 0]; cs[2::8] = [0, 1]; cs[4::8] = [-1, 0]; cs[6::8] = [0, -1]
    h = np.sqrt(0.5); cs[1::8] = [h, h]; cs[3::8] = [-h, h]; cs[5::8] = [h, -h]; cs[7::8] = [-h, -h]
    r = np.array([np.nan, np.inf, -np.inf, -1.0, 0.05, 0.01, 3.0, 3.0001,     # NaN, +-inf, negative, below range_min (0.1)...
                  5.0, 5.5, 6.0, 4.99, 0.2, 0.12, 1.0, 2.0,                   # at / above range_threshold (5.0), above range_max (6.0)
                  1.17, 2.33, 0.35, 4.2, 3.3, 0.11, 1.55, 0.64,
                  2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0], np.float32)
    puts = [(7, cs, r, 0.1, 6.0, 5.0), (8, cs, r[::-1].copy(), 0.1, 6.0, 5.0),
            (9, cs, np.where(np.isfinite(r), np.abs(r), 0).astype(np.float32), 0.0, 4.0, 9.0)]
    # a right-angle laser frame exactly on the axes: fwd = (0, 1), left = (-1, 0)
    poses = [(7, (-3.2, -7.9), np.array([0.0, 1.0]), np.array([-1.0, 0.0])), pose_tuple(8, (0.025, -0.025), 0.3),
             (7, (-0.05, -0.05), np.array([1.0, 0.0]), np.array([0.0, 1.0])), pose_tuple(9, (-1.23, 2.71), -1.0)]
    return puts, poses


def window_case():
    """six scans of long random ranges; their box is wider than 256 cells"""
    cs = R.beam_table(360, -np.pi, np.pi / 180)
    rng = np.random.default_rng(2)
    puts, poses = [], []
    for key in range(6):
        puts.append((100 + key, cs, rng.uniform(2.0, 20.0, 360).astype(np.float32), 0.1, 25.0, 18.0))
        poses.append(pose_tuple(100 + key, (key * 3.0 - 7.0, 1.0 - key), key * 0.7))
    return puts, poses


# ---- planted integer rays -----------------------------------------------------------------------------------------------------------
def planted_put(key, rows, free=None):
    """rows (n, 2): hit beams end `rows` cells from the origin cell, free beams `2 * rows`"""
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 2)
    free = np.zeros(len(rows), bool) if free is None else np.asarray(free, bool)
    return (key, rows, np.where(free, FREE, HIT).astype(np.float32)) + PLANT_LIMITS


def planted_pose(key, cell):
    return (key, (cell[0] + 0.5, cell[1] + 0.5), np.array([1.0, 0.0]), np.array([0.0, 1.0]))


def planted_rays(rays, key0=0):
    """rays: (gx0, gy0, gx1, gy1, free) in cells; one scan and one pose per distinct origin, in order of first appearance"""
    by_origin = {}
    for gx0, gy0, gx1, gy1, free in rays:
        by_origin.setdefault((gx0, gy0), []).append((gx1 - gx0, gy1 - gy0, free))
    puts, poses = [], []
    for i, (cell, beams) in enumerate(by_origin.items()):
        b = np.array(beams, np.float64)
        free = b[:, 2] != 0
        rows = np.where(free[:, None], b[:, :2] / 2, b[:, :2])
        puts.append(planted_put(key0 + i, rows, free))
        poses.append(planted_pose(key0 + i, cell))
    return puts, poses


def expected_records(puts, poses):
    """what a planted case intends, from integer arithmetic alone: int64 gx0, gy0, gx1, gy1 and bool counted, hit per beam, in
    the order of `poses`; a beam is not counted when its range is NaN or its end cell is outside [-2^28, 2^28)"""
    rows = {p[0]: (p[1], p[2]) for p in puts}
    out = []
    for key, origin, _, _ in poses:
        cs, ranges = rows[key]
        steps = np.where(ranges == FREE, 2, 1)[:, None] * cs
        assert (steps == np.floor(steps)).all()
        cell0 = np.array([int(np.floor(origin[0])), int(np.floor(origin[1]))], np.int64)
        cell1 = cell0 + steps.astype(np.int64)
        ok = ~np.isnan(ranges) & (cell1 >= -2 ** 28).all(1) & (cell1 < 2 ** 28).all(1)
        cell1 = np.where(ok[:, None], cell1, cell0)
        out.append((np.full(len(cs), cell0[0]), np.full(len(cs), cell0[1]), cell1[:, 0], cell1[:, 1], ok, ok & (ranges == HIT)))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(6))


def lattice_case():
    """A: every (dx, dy) of [-70, 70]^2, every third beam free (so twice as long), from five origin cells on and around tile corners:
    every slope and sign, every tie of q and every residue of a tile edge within reach"""
    d = np.arange(-70, 71)
    rows = np.stack(np.meshgrid(d, d, indexing="ij"), -1).reshape(-1, 2)
    puts = [planted_put(1, rows, np.arange(len(rows)) % 3 == 2)]
    poses = [planted_pose(1, c) for c in [(63, 63), (64, 64), (0, 0), (-1, -1), (-64, 63)]]
    return puts, poses


FAN_DA = 1000


def fan_rows(da, rng, n_random=60):
    """integer slopes db / da: the ends, the middle and its neighbour, and random ones; four sign pairs, both majors"""
    dbs = np.unique(np.concatenate([[0, 1, 2, da // 2, da // 2 + 1, da - 1, da], rng.integers(3, da - 1, n_random)]))
    rows = []
    for sa in (1, -1):
        for sb in (1, -1):
            rows += [(sa * da, sb * db) for db in dbs] + [(sb * db, sa * da) for db in dbs]
    return np.array(rows, np.float64)


def fan_case(origins, da=FAN_DA):
    """B: a full fan of `da`-cell rays (hits) from each origin cell; it spans 2 da + 1 cells, so with da = 1000 one fan fits 32
    tiles of 64 and a second origin up to 64 cells beside it adds a 33rd column"""
    puts = [planted_put(1, fan_rows(da, np.random.default_rng(11)))]
    return puts, [planted_pose(1, c) for c in origins]


SPLIT_BEAMS = 16384      # mirrors kChunkSegs of occupancy.hip: the segments one tile workgroup walks


def split_puts():
    """C: key 1 is SPLIT_BEAMS beams that stay within 10 cells of the origin cell (|row| <= 5, free beams twice as long), key 2 one
    beam; keys 3 and 4 reach 60 cells, into the neighbouring tiles"""
    rng = np.random.default_rng(12)
    return [planted_put(1, rng.integers(-5, 6, (SPLIT_BEAMS, 2)), rng.random(SPLIT_BEAMS) < 0.4),
            planted_put(2, [(3, -2)]),
            planted_put(3, rng.integers(-60, 61, (7000, 2)), rng.random(7000) < 0.2),
            planted_put(4, rng.integers(-60, 61, (4000, 2)), rng.random(4000) < 0.2)]


def split_poses(n_rays):
    """n_rays = a SPLIT_BEAMS + b rays, each exactly one segment of the tile [0, 64)^2"""
    a, b = divmod(n_rays, SPLIT_BEAMS)
    return [planted_pose(1, (10, 10))] * a + [planted_pose(2, (10, 10))] * b


def two_hot_poses():
    """tile (0, 0) gets 2 * 16384 + 7000 segments (three chunks), tile (2, 0) 16384 + 4000 (two chunks, its partials start at 3);
    tile (1, 0) between them and the other neighbours only get what crosses over"""
    return [planted_pose(1, (10, 10)), planted_pose(3, (10, 10)), planted_pose(1, (138, 10)), planted_pose(4, (138, 10)),
            planted_pose(1, (10, 10))]


def far_puts():
    """D: rays of 2 F cells; key 1 from (-F, -F), key 2 back from (F, F); key 3 two beams from (-F, -F) whose end coordinate falls
    at 2^28 - 0.5 (counted, 2^29 - 3 cells long) and 2^28 + 0.5 (skipped); key 5 the same from (F, F) downwards: -2^28 + 0.5 (counted,
    its end cell is -2^28) and -2^28 - 0.5 (skipped); key 6 four rays down the other diagonal from (-F, F); key 4 a short beam for
    the window's pose"""
    slopes = np.array([(2 * F, 2 * F), (2 * F, 2 * F - 1), (2 * F, 1), (2 * F, F), (2 * F, 0), (1, 2 * F), (2 * F - 1, 2 * F)], np.float64)
    return [planted_put(1, slopes), planted_put(2, -slopes),
            planted_put(3, [(2 ** 28 + F - 1, 5), (2 ** 28 + F, 5), (7, 2 ** 28 + F - 1), (7, 2 ** 28 + F)]),
            planted_put(4, [(3, 2)]),
            planted_put(5, [(-(2 ** 28 + F), -5), (-(2 ** 28 + F + 1), -5), (-7, -(2 ** 28 + F)), (-7, -(2 ** 28 + F + 1))]),
            planted_put(6, [(2 * F, -2 * F), (2 * F, -(2 * F - 1)), (2 * F - 1, -2 * F), (F + 1, -2 * F)])]


FAR_WINDOWS = [(100, 37), (F - 300, F - 300), (-F + 300, F - 300), (F - 100, F - 100), (-F + 130, -F + 130)]


def far_poses(window_cell):
    return [planted_pose(1, (-F, -F)), planted_pose(2, (F, F)), planted_pose(3, (-F, -F)), planted_pose(5, (F, F)),
            planted_pose(6, (-F, F)), planted_pose(4, window_cell)]


def window_rays(side):
    """E: rays around the window [0, side)^2 (the last pose, a scan without a counted beam, sits on its middle cell): one that
    touches only the corner cell at each corner, diagonal and not, ends on a corner cell, crossings with both ends outside on
    x-major and y-major slopes in both directions, zero-length rays inside and outside"""
    S = side
    rays = []
    for cx, cy, ox, oy in [(0, 0, -1, -1), (S - 1, 0, 1, -1), (0, S - 1, -1, 1), (S - 1, S - 1, 1, 1)]:
        rays.append((cx + 3 * ox, cy - 3 * oy, cx - 3 * ox, cy + 3 * oy, 0))              # diagonal across the corner cell
        rays.append((cx - 3 * ox, cy + 3 * oy, cx + 3 * ox, cy - 3 * oy, 1))              # (the same cells, walked the other way)
        rays.append((cx + 10 * ox, cy + 4 * oy, cx, cy, 0))                               # a hit on the corner cell from outside
        rays.append((cx, cy, cx + 9 * ox, cy + 7 * oy, 0))                                # from the corner cell outwards
        rays.append((cx + 7 * ox, cy - 2 * oy, cx - 1 * ox, cy + 2 * oy, 0))              # shallow, past the corner
    rays += [(-50, 10, S + 50, 40, 0), (S + 50, 41, -50, 9, 0), (-70, S - 5, S + 30, 3, 1),       # x-major crossings
             (20, -70, 45, S + 60, 0), (46, S + 60, 19, -70, 0), (S - 4, -40, 2, S + 33, 1),      # y-major crossings
             (-30, -30, S + 30, S + 30, 0), (S + 20, -21, -21, S + 20, 0),                        # 45 degrees, through two corners
             (5, 5, 5, 5, 0), (5, 5, 5, 5, 1), (S // 2, S - 1, S // 2, S - 1, 0),                 # zero length, inside
             (-20, -20, -20, -20, 0), (S, S, S, S, 0), (S + 7, 3, S + 7, 3, 1)]                   # zero length, outside
    return rays


NAN_KEY = 9000


def window_case_planted(side, rays):
    """the window [0, side)^2: the last pose's only beam is NaN, so it places the window and counts nothing"""
    puts, poses = planted_rays(rays)
    puts.append((NAN_KEY, np.array([[1.0, 0.0]]), np.array([np.nan], np.float32)) + PLANT_LIMITS)
    poses.append(planted_pose(NAN_KEY, (side // 2, side // 2)))
    return puts, poses


def missing_rays(side):
    """rays that all miss the window [0, side)^2"""
    S = side
    return [(1000, 1000, 1300, 1100, 0), (-5, 0, -5, S, 0), (-40, S + 2, S + 40, S + 2, 1), (S, -1, -1, -70, 0),
            (-1, -1, -9, -9, 0), (S + 3, S // 2, S + 3, S // 2, 0)]


STRIDE_BEAMS, STRIDE_POSES = 65536, 66


def stride_case():
    """F: one stored scan of 65536 short beams under 66 poses: more rays than 16384 blocks of 256 lanes take in one pass"""
    rng = np.random.default_rng(13)
    puts = [planted_put(1, rng.integers(-3, 4, (STRIDE_BEAMS, 2)), rng.random(STRIDE_BEAMS) < 0.3)]
    poses = [planted_pose(1, tuple(int(v) for v in rng.integers(-100, 101, 2))) for _ in range(STRIDE_POSES)]
    return puts, poses
