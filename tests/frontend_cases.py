"""Planted inputs for the ORB front end at the sizes where its kernels change regime (lpslam_amd/csrc/frontend.hip), pure numpy.
Shared by tests/test_frontend_cases_cpu.py (the CPU oracle alone shows that every case sits in its regime) and
tests/test_frontend_limits_gpu.py (the device against the oracle, bit for bit).

`level_table` restates the geometry of `build_level_table` (csrc/api.hip): level sizes, FAST cell grid, quad-tree roots, per-level
quota and slot capacity.  The GPU tests compare it with what the context reports, the CPU tests with the oracle's own sizes."""
import math

import numpy as np

EDGE, CELL, OVERLAP = 19, 64, 6          # kEdge, kCell, kOverlap
QUOTA_MAX = 2000                         # kQuotaMax
ROOT_AXIS_MAX = 256                      # root columns / rows of one level (the distribution kernel's byte tables)
DIST_THREADS, DIST_CPT = 1024, 24        # k_distribute: threads, register slots per thread
BACKGROUND = 40
DOT_MARGIN = 22                          # EDGE + the 3-px FAST border: the first pixel of a level that is tested


def _round(x):
    """C round() for the positive values of the level arithmetic"""
    return int(math.floor(x + 0.5))


# ---- level arithmetic -------------------------------------------------------------------------------------------------------
def level_scales(scale, levels):
    s = [np.float32(1.0)]
    for _ in range(1, levels):
        s.append(np.float32(scale) * s[-1])
    return s


def level_sizes(w, h, scale, levels):
    s = level_scales(scale, levels)
    return [w] + [_round(w * 1.0 / float(v)) for v in s[1:]], [h] + [_round(h * 1.0 / float(v)) for v in s[1:]]


def cell_grid(n):
    """FAST cells along an axis of n pixels: their widths (7 ... 70; a trailing strip of 6 px or less has no cell of its own)"""
    hi = n - EDGE
    out = []
    for j in range((hi - EDGE) // CELL + 1):
        lo = EDGE + j * CELL
        if hi - OVERLAP <= lo:
            continue
        out.append(min(lo + CELL + OVERLAP, hi) - lo)
    return out


def roots(w, h):
    """quad-tree root columns and rows of a w x h level"""
    width, height = w - 2 * EDGE, h - 2 * EDGE
    ratio = width / height
    return (_round(ratio), 1) if ratio > 1 else (1, _round(1 / ratio))


def quotas(max_kpts, scale, levels):
    f = 1.0 / float(np.float32(scale))
    desired = max_kpts * (1.0 - f) / (1.0 - f ** levels)
    q, total = [], 0
    for _ in range(levels - 1):
        q.append(_round(desired)); total += q[-1]; desired *= f
    return q + [max(max_kpts - total, 0)]


def level_table(w, h, max_kpts, scale, levels):
    lw, lh = level_sizes(w, h, scale, levels)
    q = quotas(max_kpts, scale, levels)
    rt = [roots(a, b) for a, b in zip(lw, lh)]
    return dict(w=lw, h=lh, quota=q, roots=rt, cells=[(cell_grid(a), cell_grid(b)) for a, b in zip(lw, lh)],
                slots=[max(n + 3, 4 * rx * ry) for n, (rx, ry) in zip(q, rt)])


def distribute_regime(n_cand):
    """(register slots per thread, 16-byte load path, candidates beyond the registers) of k_distribute for a level with n_cand corners"""
    cpt = min(DIST_CPT, -(-n_cand // DIST_THREADS))
    return cpt, cpt % 4 == 0, max(0, n_cand - DIST_THREADS * DIST_CPT)


# ---- planted dots -----------------------------------------------------------------------------------------------------------
def dot_grid(w, h, step):
    return (w - 2 * DOT_MARGIN - 1) // step + 1, (h - 2 * DOT_MARGIN - 1) // step + 1


def widest_step(w, h, n):
    """the largest spacing at which n dots fit: they spread over every FAST cell of the image"""
    for step in range(4, max(w, h)):
        c, r = dot_grid(w, h, step + 1)
        if c * r < n:
            return step
    return max(w, h)


def dot_positions(w, h, n, step):
    assert step >= 4
    cols, rows = dot_grid(w, h, step)
    assert n <= cols * rows, (n, cols * rows)
    i = np.arange(n)
    return DOT_MARGIN + step * (i % cols), DOT_MARGIN + step * (i // cols)


def dots(w, h, values, step):
    """A flat image with single pixels set, row-major, at least 22 px from every edge and `step` >= 4 apart.  On a one-level context
    every such pixel is exactly one FAST candidate after suppression (no other dot lies on its 16-ring or beside it), with the score
    value - BACKGROUND - 1."""
    values = np.asarray(values)
    assert values.min() > BACKGROUND and values.max() <= 255
    img = np.full((h, w), BACKGROUND, np.uint8)
    x, y = dot_positions(w, h, len(values), step)
    img[y, x] = values
    return img


def dot_values(n, kind, seed=0):
    """`equal`: ties everywhere (score 214); `ramp`: scores fall and rise along the candidate order in runs of 151, every score many
    times; `shuffle`: the ramp's values in a seeded random order"""
    if kind == "equal":
        return np.full(n, 255, np.uint8)
    v = (255 - (np.arange(n) * 7) % 151).astype(np.uint8)          # 105 ... 255: every dot passes the initial threshold of 20
    if kind == "ramp":
        return v
    assert kind == "shuffle"
    return np.random.default_rng(seed).permutation(v)


# candidate counts on either side of: one slot per thread (1024), the first 16-byte load (cpt 4: 3073 ... 4096), cpt 5, the last
# register slot (24576) and the global scratch beyond it
DOT_COUNTS = [1, 2, 1023, 1024, 1025, 4096, 4097, 5120, 24575, 24576, 24577, 26000]
DOT_KINDS_EXTRA = [(1025, "ramp"), (1025, "shuffle"), (4097, "ramp"), (4097, "shuffle"), (24577, "ramp"), (24577, "shuffle")]
DOT_QUEUED = [1025, 4097, 24577]


def dot_shape(n):
    """the smallest of three image sizes that holds n dots; 1280 x 1000 holds the largest counts"""
    for w, h in ((320, 240), (640, 480), (1280, 1000)):
        c, r = dot_grid(w, h, 4)
        if c * r >= n:
            return w, h
    raise ValueError(n)


def dot_budgets(n):
    """one budget far below the count; the count - 1, the count and the count + 1 where the per-level limit of 2000 allows them"""
    b = [max(1, min(n // 8, 500))]
    if n + 1 <= QUOTA_MAX:
        b += [v for v in (n - 1, n, n + 1) if v >= 1]
    return sorted(set(b))


def dot_image(n, kind="equal"):
    w, h = dot_shape(n)
    return dots(w, h, dot_values(n, kind, seed=n), widest_step(w, h, n))


# ---- quotas -----------------------------------------------------------------------------------------------------------------
# max_keypoints over 8 levels at scale 1.2 -> the quota vector: zeros on the last levels (1, 2, 5), on the first and last (1: all but
# one), 8: at least one per level and a zero at the end
QUOTA_CASES = {1: [0, 0, 0, 0, 0, 0, 0, 1], 2: [0, 0, 0, 0, 0, 0, 0, 2], 5: [1, 1, 1, 1, 1, 0, 0, 0], 8: [2, 1, 1, 1, 1, 1, 1, 0]}
QUOTA_SHAPE = (300, 200)


def noise(w, h, seed):
    return np.random.default_rng([w, h, seed]).integers(0, 256, (h, w)).astype(np.uint8)


# ---- cell edges -------------------------------------------------------------------------------------------------------------
# level sizes n with n - 38 = 8, 9 (one cell of 8 / 9 px: 2 / 3 tested columns), 63, 64, 70 (one cell; at 70 it is full), 71 (a second
# cell of 7 px: one tested column), 72, 134 (two cells, the second full), 135 (a third cell of 7 px)
EDGE_SPANS = [8, 9, 63, 64, 70, 71, 72, 128 + 6, 128 + 7]
EDGE_CELLS = {8: [8], 9: [9], 63: [63], 64: [64], 70: [70], 71: [70, 7], 72: [70, 8], 134: [70, 70], 135: [70, 70, 7]}
EDGE_SCALE = 1.39                        # level 1 of a 64-px image is 46 px: a context's own image is at least 64 px


def edge_shapes():
    """(level width, level height) of the sweep: every span as a width with two heights, every span as a height twice"""
    n = len(EDGE_SPANS)
    return [(EDGE_SPANS[i] + 2 * EDGE, EDGE_SPANS[(i + k) % n] + 2 * EDGE) for i in range(n) for k in (2, 5)]


def edge_context(lw, lh):
    """(image width, image height, levels, tested level) whose tested level is lw x lh: the image itself, or, below 64 px, level 1 of
    a two-level context at scale 1.39"""
    if lw >= 64 and lh >= 64:
        return lw, lh, 1, 0
    s = float(np.float32(EDGE_SCALE))

    def source(n):
        m = next(v for v in range(64, 4 * n + 64) if _round(v / s) == n)
        return m
    return source(lw), source(lh), 2, 1


# ---- thresholds -------------------------------------------------------------------------------------------------------------
THRESHOLDS = [(0, 0), (255, 7), (300, 300), (5, 30), (20, 20)]
THRESHOLD_SHAPE = (210, 150)
BOARD_LOW, BOARD_HIGH = 60, 200


def board(w, h, period):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // period) + (yy // period)) % 2 == 0, BOARD_LOW, BOARD_HIGH).astype(np.uint8)


def weave(w, h):
    """pixel (x, y) is bright where (x + 2 y) mod 4 >= 2.  Every pixel has a compass pair (ring positions 0 / 8 and 4 / 12) and a diagonal
    pair (2 / 10 and 6 / 14) of the other colour: all pixels pass the pre-test of fast_cells_body at any threshold below the contrast, so
    each wavefront's queue of 16 rows x 64 pixels is exactly full in a full cell."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx + 2 * yy) % 4 >= 2, BOARD_HIGH, BOARD_LOW).astype(np.uint8)


def pretest(img, thr):
    """The pre-test of fast_cells_body restated: for every pixel, is there a neighbouring compass pair AND a neighbouring diagonal pair
    of ring pixels all darker than centre - thr, or all brighter than centre + thr?  (bool image; the 3-px rim is False)"""
    a = img.astype(np.int32)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]

    def at(dy, dx):
        return a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx]
    p0, p8, p4, p12 = at(3, 0), at(-3, 0), at(0, 3), at(0, -3)
    p2, p10, p6, p14 = at(2, 2), at(-2, -2), at(-2, 2), at(2, -2)
    dark = np.maximum(np.maximum(np.minimum(p0, p8), np.minimum(p4, p12)), np.maximum(np.minimum(p2, p10), np.minimum(p6, p14))) < c - thr
    bright = np.minimum(np.minimum(np.maximum(p0, p8), np.maximum(p4, p12)), np.minimum(np.maximum(p2, p10), np.maximum(p6, p14))) > c + thr
    out = np.zeros(a.shape, bool)
    out[3:h - 3, 3:w - 3] = dark | bright
    return out


def threshold_images():
    w, h = THRESHOLD_SHAPE
    return {"noise": noise(w, h, 3), "board1": board(w, h, 1), "board2": board(w, h, 2), "weave": weave(w, h)}


# ---- extreme aspect ---------------------------------------------------------------------------------------------------------
# (width, height, levels, scale, max_keypoints); the transposes are tested too.  Budgets are reduced so that the distribution stops
# at the quota, not at the last corner.
ASPECT_CASES = [(4133, 64, 1, 1.2, 700), (4133, 500, 8, 1.2, 1200)]
# two-level contexts at scale 1.38 and 64 px height: level 1 is 46 px high (8 px inside the border) with this many root columns
ROOT_SCALE = 1.38
ROOT_SHAPES = {255: 2862, 256: 2873, 257: 2885, 300: 3359}        # root columns of level 1 -> image width
ROOT_BUDGET = 1500
ROOT_SEED = 11                           # noise with corners in the last root of every shape, transposed or not


def transpose_case(case):
    return (case[1], case[0]) + tuple(case[2:])


# ---- batches ----------------------------------------------------------------------------------------------------------------
BATCH = dict(n=65, w=110, h=64, levels=2, scale=1.2, kpts=60)     # 64 images or more: four pyramid bands per image


# ---- regime checks: the same conditions on the oracle's output (CPU test) and on the device's (GPU test) -------------------------
def per_level(kp, levels):
    return np.bincount(kp["octave"], minlength=levels)


def check_dots(cand, kp, n, kind, budget):
    assert len(cand) == n                                              # slots per thread, load path and scratch follow from it
    assert len(set(cand["score"])) == (1 if kind == "equal" else min(n, 151))
    if kind == "equal":
        assert cand["score"][0] == 255 - BACKGROUND - 1
    assert min(budget, n) <= len(kp) <= max(min(budget + 3, n), 4)     # cut at the quota, or every corner


def check_zero_quota(cand, kp, quota):
    got = per_level(kp, len(quota))
    assert 0 in quota and all(len(c) > 4 for c in cand)
    assert all(g > q for g, q in zip(got, quota) if q == 0)            # a zero quota still returns the first split pass


def check_quota_limit(cand, kp):
    assert len(cand) > 2 * QUOTA_MAX and QUOTA_MAX <= len(kp) <= QUOTA_MAX + 3


def check_edge(cand, lw, lh):
    """corners of the last cell column and row where that cell has more than a column or two to test"""
    cw, ch = cell_grid(lw)[-1], cell_grid(lh)[-1]
    if cw >= 16 and ch >= 16:
        assert len(cand) > 0
        assert cand["x"].max() >= CELL * (len(cell_grid(lw)) - 1) + 3 and cand["y"].max() >= CELL * (len(cell_grid(lh)) - 1) + 3
    assert len(cand) == 0 or (cand["x"].max() <= lw - 2 * EDGE - 4 and cand["y"].max() <= lh - 2 * EDGE - 4)


def check_threshold_counts(count, ini, mn):
    if min(ini, mn) >= 255:
        assert all(v == 0 for v in count.values())                     # no arc is stronger than 255
    else:
        assert count["noise"] > 100
    assert count["board1"] == 0                                        # its diagonal ring pixels equal the centre


def check_aspect(cand, kp, table):
    """every level stops at its quota: more corners than it returns, and more returned than one split pass of the roots can give"""
    got = per_level(kp, len(cand))
    for l, c in enumerate(cand):
        assert table["quota"][l] <= got[l] <= table["quota"][l] + 3 and got[l] < len(c), l
    rx, ry = table["roots"][0]
    assert table["quota"][0] > 4 * rx * ry or len(cand) > 1


def check_roots(cand, lw, lh, n_roots):
    """the level has n_roots roots along its long axis and the last of them holds corners"""
    assert max(roots(lw, lh)) == n_roots and min(lw, lh) == 46
    along = cand["x"] if lw > lh else cand["y"]
    span = max(lw, lh) - 2 * EDGE
    assert int((along / (span / n_roots)).max()) == n_roots - 1
