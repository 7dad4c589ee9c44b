"""The window matchers (lpslam_hip_match_projection / _fuse / _area: k_proj_topk and its host replay) against the oracle, bit for bit,
where the other matcher tests do not go: frames of more than 2048 keypoints (the second pass in the middle of the scan), equal
distances decided by the grid cell at a width where a float and a double cell differ, query values a caller may pass but a tracker
seldom does, and the single-query rescan proven by the library's own counter.  Helpers: tests/match_cases.py."""
import numpy as np
import pytest

import match_cases as M
from lpslam_amd import synth

pytestmark = pytest.mark.gpu


# ---- 752 x 480, white noise, 2607 keypoints -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(hiplib, oracle):
    """752 x 480 / 2600 keypoints / 8 levels on white noise: more keypoints than the wavefront's LDS list holds (2048) plus a scan
    iteration's worth, at a width where x * 64 / w is an integer for level-0 keypoints at x = 47 k"""
    w, h = 752, 480
    ctx = hiplib.Context(w, h, 2600, 1.2, 8, max_images=2)
    img = np.random.default_rng(1).integers(0, 256, (h, w)).astype(np.uint8)
    fr, bad = M.load_frame(oracle, ctx, oracle.params(2600, 1.2, 8), 0, img)
    assert not bad, bad
    assert len(fr.kp) > 2048 + 64
    assert (np.diff(fr.kp["octave"]) >= 0).all()                     # slots are ordered by level
    fr.desc0 = fr.desc.copy()
    yield fr
    ctx.close()


def _wide_queries(fr, rng):
    """24 queries whose window covers the image, in three groups of 8 by level bounds.  Descriptors: half are keypoints of the frame
    itself (spread over the whole index range, so the winner is met before or after the mid-scan pass) with a few bits flipped, half
    are random (the minimum over ~2600 random descriptors is often shared: the cell order decides)."""
    n = len(fr.kp)
    src = np.linspace(0, n - 1, 24).astype(int)
    rng.shuffle(src)
    q = M.queries(fr.kp["x"][src] + rng.normal(0, 3, 24), fr.kp["y"][src] + rng.normal(0, 3, 24), 4000.0)
    q["max_level"][8:16] = 1                                        # -1 / 1
    q["max_level"][16:] = 0                                         # -1 / 0
    qd = fr.desc0[src].copy()
    qd[:, 3] ^= rng.integers(0, 256, 24).astype(np.uint8)
    qd[::2] = rng.integers(0, 256, (12, 32)).astype(np.uint8)
    return q, qd


def test_more_keypoints_than_the_list_holds_projection_and_area(wide, oracle):
    """Every keypoint a candidate (-1 / -1: the list is full when the third scan iteration starts), levels 0-1 only (-1 / 1: all
    candidates met in the first two iterations, the mid-scan pass runs on a partly filled list and the end-of-scan pass on an empty
    one), level 0 only (-1 / 0: no mid-scan pass, the control); with and without a `taken` mask; projection and area policies."""
    fr = wide
    fr.set_descriptors(fr.desc0)
    lv = np.bincount(fr.kp["octave"], minlength=8)
    assert 1024 < lv[0] + lv[1] <= 2048 and lv[0] <= 1024           # the three groups take the three paths the docstring names
    q, qd = _wide_queries(fr, np.random.default_rng(2))
    taken = np.zeros(len(fr.kp), np.uint8); taken[::7] = 1
    for policy, tk, thr, ratio in (("projection", None, 256, 1.0), ("projection", taken, 256, 1.0), ("projection", None, 100, 0.8),
                                   ("area", None, 256, 1.0), ("area", None, 100, 0.9)):
        why, (oi, od, on), _ = M.compare(oracle, fr, policy, q, qd, thr, ratio, tk)
        assert not why, (policy, tk is not None, thr, why)
        assert on > 0, (policy, thr, on)
        if thr == 256 and policy == "projection":
            assert on == 24 and (fr.kp["octave"][oi[8:16]] <= 1).all() and (fr.kp["octave"][oi[16:]] == 0).all()
            assert (oi > 2048).any() and (oi < 1024).any()          # winners on both sides of the mid-scan pass
        if tk is not None:
            assert not taken[oi[oi >= 0]].any()
    # the same windows with ties planted over the whole index range: three keypoints in ten carry one of four descriptors and the
    # queries ask for exactly those, six queries each -- a wavefront's four best keys come from both sides of the mid-scan pass, equal
    # distances are ranked by cell, and the later queries of a descriptor find their list used up (rescans on the long scan)
    rng = np.random.default_rng(4)
    proto = rng.integers(0, 256, (4, 32)).astype(np.uint8)
    desc = fr.desc0.copy()
    planted = np.flatnonzero(rng.random(len(fr.kp)) < 0.3)
    desc[planted] = proto[rng.integers(0, 4, len(planted))]
    assert (planted > 2048).sum() > 50 and (planted < 1024).sum() > 50
    fr.set_descriptors(desc)
    qd = proto[np.arange(24) % 4]
    for policy, tk in (("projection", None), ("projection", taken), ("area", None)):
        why, (oi, od, on), rescans = M.compare(oracle, fr, policy, q, qd, 256, 1.0, tk)
        assert not why, ("planted", policy, tk is not None, why)
        if policy == "projection":
            assert on == 24 and (od == 0).all() and np.isin(oi, planted).all() and rescans > 0
    fr.set_descriptors(fr.desc0)


def test_more_keypoints_than_the_list_holds_fuse(wide, oracle):
    """match::fuse on the same frame: 200 queries one pixel off true keypoints over the whole index range (the chi-square gate keeps
    the lists short; the point is a scan of more than two iterations)"""
    fr = wide
    fr.set_descriptors(fr.desc0)
    rng = np.random.default_rng(3)
    src = np.linspace(0, len(fr.kp) - 1, 200).astype(int)
    oc = fr.kp["octave"][src]
    q = M.queries(fr.kp["x"][src] + 1.0, fr.kp["y"][src], 3.0 * np.float32(1.2) ** oc, np.maximum(oc - 1, 0), oc)
    qd = fr.desc0[src].copy()
    qd[:, 5] ^= (1 << rng.integers(0, 8, 200)).astype(np.uint8)
    why, (oi, od, on), rescans = M.compare(oracle, fr, "fuse", q, qd, 50)
    assert not why, why
    assert on > 150 and (oi > 2048).sum() > 10 and rescans == 0


def test_equal_distances_are_ranked_by_the_oracles_cell(wide, oracle):
    """Every descriptor of the frame and every query descriptor zero: all distances are 0 and only the scan order -- grid cell,
    column-major, then index -- decides.  At width 752 a level-0 keypoint at x = 94, 188, 376 lies in cell column x * 64 / 752 exactly;
    a float product puts it one column lower.  Single-query calls around every such keypoint and on a lattice, all three policies,
    then all queries in one call (sequential assignment under total ties).
    (With the cell computed as floorf(x * (float)(64.0 / w)) this test fails: the projection query at (96, y - 3), radius 10, next to
    keypoint 253 (x = 94) returns keypoint 253 where the oracle returns 770.)"""
    fr = wide
    fr.set_descriptors(np.zeros((len(fr.kp), 32), np.uint8))
    cd, cf = M.cell_columns(fr.kp["x"], fr.w)
    rd, rf = M.cell_rows(fr.kp["y"], fr.h)
    odd = np.flatnonzero((cd != cf) | (rd != rf))
    assert len(odd) >= 1
    probes = [(float(fr.kp["x"][i]) + 2, float(fr.kp["y"][i]) - 3, r, int(i)) for i in odd for r in (6.0, 10.0, 20.0, 40.0)]
    gx, gy = np.meshgrid((np.arange(8) + 0.5) * fr.w / 8, (np.arange(8) + 0.5) * fr.h / 8)
    lattice = [(float(x), float(y), 30.0, -1) for x, y in zip(gx.ravel(), gy.ravel())]
    zero = np.zeros((1, 32), np.uint8)
    bad, matched = [], {p: 0 for p in M.POLICIES}
    for policy in M.POLICIES:
        for x, y, r, i in probes + lattice:
            if policy == "fuse" and i >= 0: x, y = float(fr.kp["x"][i]), float(fr.kp["y"][i])       # inside the gate
            why, (oi, od, on), _ = M.compare(oracle, fr, policy, M.queries([x], y, r), zero, 256, 1.0)
            matched[policy] += on
            if why: bad.append("%s: %s" % (policy, why))
    assert not bad, "%d of %d single-query calls differ: %s" % (len(bad), 3 * len(probes + lattice), "; ".join(bad[:6]))
    assert matched["projection"] == len(probes) + len(lattice) and matched["fuse"] >= len(probes)
    allq = probes + lattice
    q = M.queries([a[0] for a in allq], [a[1] for a in allq], [a[2] for a in allq])
    qd = np.zeros((len(q), 32), np.uint8)
    for policy in M.POLICIES:
        why, (oi, od, on), _ = M.compare(oracle, fr, policy, q, qd, 256, 1.0)
        assert not why, (policy, why)
        if policy == "projection":
            m = oi[oi >= 0]
            assert on > len(lattice) and len(np.unique(m)) == len(m)


def test_four_nearest_candidates_on_one_lane(wide, oracle):
    """One query, level 0 only, a window that holds exactly 64 * 4 + 1 = 257 keypoints: candidate r of the wavefront's list is met by
    lane r % 64.  The four nearest (8, 9, 10 and 11 bits from the query, every other candidate 60) sit at list positions 5, 69, 133
    and 197 -- all lane 5 -- so the wavefront's four answers are one lane's whole list, popped four times.  8 against 9 fails a Lowe
    ratio of 0.8, 8 against a lost second (60) would pass; with the successive bests marked `taken` every entry becomes the head
    in turn, and only 11 against 60 passes."""
    fr = wide
    lvl0 = np.flatnonzero(fr.kp["octave"] == 0)
    cx, cy = np.float32(fr.w / 2), np.float32(fr.h / 2)
    cheb = np.maximum(np.abs(fr.kp["x"][lvl0] - cx), np.abs(fr.kp["y"][lvl0] - cy))          # float32, as the kernel's window test
    order = np.sort(cheb)
    assert len(lvl0) > 257 and order[257] - order[256] > 1e-3
    radius = np.float32(0.5) * (order[256] + order[257])
    cand = lvl0[cheb < radius]                                        # in index order: the order the wavefront lists them in
    assert len(cand) == 257
    best4 = cand[[5, 69, 133, 197]]

    def ones(bits):
        return np.packbits(np.arange(256) < bits)

    desc = fr.desc0.copy()
    desc[cand] = ones(60)
    for r, i in enumerate(best4):
        desc[i] = ones(8 + r)
    fr.set_descriptors(desc)
    q, qd = M.queries([cx], cy, radius, -1, 0), np.zeros((1, 32), np.uint8)
    try:
        for stage in range(5):
            taken = np.zeros(len(fr.kp), np.uint8); taken[best4[:stage]] = 1
            for ratio in (0.8, 1.0):
                why, (oi, od, on), rescans = M.compare(oracle, fr, "projection", q, qd, 256, ratio, taken if stage else None)
                assert not why, (stage, ratio, why)
                assert rescans == 0
                if ratio == 0.8:                                      # 8 : 9, 9 : 10, 10 : 11 fail, 11 : 60 passes, 60 : 60 fails
                    assert (on, oi[0]) == ((1, best4[3]) if stage == 3 else (0, -1)), (stage, oi)
                elif stage < 4:
                    assert on == 1 and oi[0] == best4[stage] and od[0] == 8 + stage, (stage, oi, od)
                else:
                    assert on == 1 and od[0] == 60 and oi[0] not in best4
    finally:
        fr.set_descriptors(fr.desc0)


# ---- 320 x 240 stereo pair: odd queries, rescans ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(hiplib, oracle):
    """Frames 0 and 1 of a 320 x 240 / 400 keypoints / 4 levels stereo sequence: slot 2 (stereo-matched against slot 3) is the matched
    frame, the keypoints of frame 0 make the queries; slot 1 receives a blank image (no keypoints at all)."""
    w, h = 320, 240
    seq = synth.StereoSequence(w, h, 5)
    l0, r0 = seq.frame(0); l1, r1 = seq.frame(1)
    k = synth.intrinsics(w, h)
    ctx = hiplib.Context(w, h, 400, 1.2, 4, max_images=4)
    p = oracle.params(400, 1.2, 4)
    f0, bad0 = M.load_frame(oracle, ctx, p, 0, l0, 1, r0, k["fxb"], k["baseline"])
    f1, bad1 = M.load_frame(oracle, ctx, p, 2, l1, 3, r1, k["fxb"], k["baseline"])
    blank, bad2 = M.load_frame(oracle, ctx, p, 1, np.full((h, w), 90, np.uint8))
    assert not (bad0 + bad1 + bad2), (bad0, bad1, bad2)
    assert len(f0.kp) > 200 and len(f1.kp) > 200 and len(blank.kp) == 0 and (f1.xr > 0).sum() > 30
    yield f0, f1, blank
    ctx.close()


def _base_queries(f0, n, rng, fuse):
    """n queries as a motion model would predict them: keypoints of frame 0 displaced a little, their descriptors"""
    src = rng.permutation(len(f0.kp))[:n]
    oc = f0.kp["octave"][src]
    jit = 1.0 if fuse else 4.0
    dx = rng.normal(0, jit, n).astype(np.float32)
    q = M.queries(f0.kp["x"][src] + dx, f0.kp["y"][src] + rng.normal(0, jit, n), (3.0 if fuse else 15.0) * np.float32(1.2) ** oc,
                  np.maximum(oc - 1, 0) if fuse else oc - 1, oc if fuse else oc + 1, np.where(f0.xr[src] > 0, f0.xr[src] + dx, -1.0))
    return q, f0.desc[src].copy()


def _odd_cases(f0, f1, policy):
    """(name, queries, descriptors, hamming_thr, lowe_ratio, taken, use_stereo, what the oracle must answer) -- `expect` is "none" (nothing may
    match), "some" (at least one match) or "any" """
    rng = np.random.default_rng(17)
    fuse = policy == "fuse"
    thr0, ratio0 = (50, 1.0) if fuse else (100, 0.9)
    W, H = f1.w, f1.h
    out = []

    def add(name, q, qd, thr=thr0, ratio=ratio0, taken=None, stereo=False, expect="any"):
        out.append((name, q, qd, thr, ratio, taken, stereo, expect))

    q, qd = _base_queries(f0, 64, rng, fuse)
    add("plain", q, qd, expect="some")
    add("plain with the stereo column", q, qd, stereo=True, expect="some")
    # query centres outside the image: windows that reach into it and windows that do not
    n = 24
    ex = np.concatenate([np.full(6, -30.0), np.full(6, W + 25.0), rng.uniform(0, W, 12)])
    ey = np.concatenate([rng.uniform(0, H, 12), np.full(6, -40.0), np.full(6, H + 10.0)])
    for r, name in ((60.0, "reaching in"), (10.0, "reaching nothing")):
        qq = M.queries(ex, ey, r)
        add("centres outside the image, " + name, qq, f1.desc[rng.integers(0, len(f1.kp), n)], thr=256 if not fuse else 50, ratio=1.0,
            expect="none" if r == 10.0 else ("any" if fuse else "some"))
    for r, expect in ((0.0, "none"), (-5.0, "none"), (4000.0, "some")):
        qq = q.copy(); qq["radius"] = r
        add("radius %g" % r, qq, qd, expect=expect)
    qq = q.copy(); qq["min_level"] = 2; qq["max_level"] = 1
    add("min_level > max_level", qq, qd, expect="none")
    qq = q.copy(); qq["min_level"] = -1; qq["max_level"] = 1
    add("upper level bound only", qq, qd, expect="some")
    qq = q.copy(); qq["min_level"] = 2; qq["max_level"] = -1; qq["radius"] = 40.0
    add("lower level bound only", qq, qd)
    qq = q.copy(); qq["min_level"] = 4; qq["max_level"] = -1
    add("lower level bound above the top level", qq, qd, expect="none")
    qq = q.copy(); qq["x_right"] = 0.0
    add("x_right == 0", qq, qd, stereo=True)
    qq = q.copy(); qq["x_right"][::2] = 0.0; qq["radius"] = 400.0
    add("x_right == 0, wide window", qq, qd, stereo=True, expect="some")
    # hamming_thr 0 / 256, lowe_ratio 0 / 1: queries ON keypoints of the matched frame with their own descriptors (distance 0 exists)
    src = rng.permutation(len(f1.kp))[:40]
    oc = f1.kp["octave"][src]
    qs = M.queries(f1.kp["x"][src], f1.kp["y"][src], 12.0, np.maximum(oc - 1, 0), oc)
    qsd = f1.desc[src].copy(); qsd[1::2, 9] ^= 0x40                  # every other one a bit off: distance 1 fails a threshold of 0
    add("hamming_thr 0", qs, qsd, thr=0, ratio=1.0, expect="some")
    add("hamming_thr 256", q, qd, thr=256, ratio=1.0, expect="some")
    add("lowe_ratio 0", qs, qsd, thr=100, ratio=0.0, expect="some" if policy != "area" else "none")       # 0 > 0 is false, 0 < 0 too
    add("lowe_ratio 1", q, qd, thr=100, ratio=1.0, expect="some")
    for m in (1, 3, 4, 5):                                          # four queries per workgroup
        add("nq %d" % m, qs[:m], qsd[:m], thr=100, ratio=1.0, expect="some")
    if policy == "projection":
        add("taken: all ones", q, qd, taken=np.ones(len(f1.kp), np.uint8), expect="none")
        tk = np.ones(len(f1.kp), np.uint8); tk[::3] = 0
        add("taken: two thirds, wide window", M.queries(q["x"], q["y"], 4000.0), qd, thr=256, ratio=1.0, taken=tk, expect="some")
    return out


@pytest.mark.parametrize("policy", M.POLICIES)
def test_query_values_a_caller_may_pass(small, oracle, policy):
    """One table per policy: centres outside the image, radius 0 / negative / larger than the image, inverted and one-sided level
    bounds, x_right == 0, hamming_thr 0 and 256, lowe_ratio 0 and 1, 1 / 3 / 4 / 5 queries, a `taken` mask of all ones, and a frame
    without keypoints.  No NaN or infinity: the oracle's (int)floor() of them is not defined."""
    f0, f1, blank = small
    bad = []
    for name, q, qd, thr, ratio, taken, stereo, expect in _odd_cases(f0, f1, policy):
        why, (oi, od, on), _ = M.compare(oracle, f1, policy, q, qd, thr, ratio, taken, stereo)
        if why: bad.append("%s: %s" % (name, why))
        if expect == "none": assert on == 0, name
        if expect == "some": assert on > 0, name
        if name == "hamming_thr 0" and policy != "area": assert (od[oi >= 0] == 0).all() and 0 < on < len(q)
    assert not bad, "; ".join(bad)
    # a frame without keypoints, five queries: nothing matched, no error
    q, qd = _base_queries(f0, 5, np.random.default_rng(1), policy == "fuse")
    q["radius"] = 4000.0
    for stereo in (False, True):
        gi, gd, gn, rescans = M.run_gpu(blank, policy, q, qd, 256, 1.0, None, stereo)
        assert gn == 0 and (gi == -1).all() and (gd == 256).all() and rescans == 0
    why, (oi, od, on), _ = M.compare(oracle, blank, policy, q, qd, 256, 1.0)
    assert not why and on == 0, why


def test_rescans_are_counted(small, oracle):
    """120 identical queries (one position, one descriptor, a wide level-free window) compete for the same keypoints: the four-entry
    candidate lists of the first scan are used up by earlier queries and the single-query rescan must run -- for the projection and
    the area policy the library's counter says it did; a fuse call and a call of one query never rescan."""
    f0, f1, blank = small
    q = M.queries(np.full(120, f0.kp["x"][0]), f0.kp["y"][0], 80.0)
    qd = np.repeat(f0.desc[:1], 120, axis=0)
    for policy in ("projection", "area"):
        why, (oi, od, on), rescans = M.compare(oracle, f1, policy, q, qd, 256, 1.0)
        assert not why, (policy, why)
        assert on > (20 if policy == "projection" else 0) and rescans > 0, (policy, on, rescans)
        m = oi[oi >= 0]
        assert len(np.unique(m)) == len(m)
    why, _, rescans = M.compare(oracle, f1, "fuse", q, qd, 256)
    assert not why and rescans == 0
    for policy in ("projection", "area"):
        why, (oi, od, on), rescans = M.compare(oracle, f1, policy, q[:1], qd[:1], 256, 1.0)
        assert not why and on == 1 and rescans == 0, (policy, why, rescans)
