"""The ORB front end at its size, quota and candidate limits (tests/frontend_cases.py), through the C ABI against the CPU oracle.
Every comparison is exact: pyramid bytes per level, FAST candidates (x, y, score, order), keypoint fields, descriptors.  Every test
also reads its regime back from the device (candidate counts, `ctx.quota`, `ctx.level_w` / `level_h`): a case that drifts out of its
regime fails instead of passing on easier ground.  tests/test_frontend_cases_cpu.py shows the same regimes on the oracle alone."""
import numpy as np
import pytest

import frontend_cases as fc

pytestmark = pytest.mark.gpu


def _assert_same_keypoints(okp, od, gkp, gd):
    assert len(okp) == len(gkp)
    for f in okp.dtype.names:
        assert np.array_equal(okp[f], gkp[f]), "keypoint field %s" % f
    assert np.array_equal(od, gd)


@pytest.fixture(scope="module")
def contexts(hiplib):
    """contexts shared per configuration; closed with the module"""
    cache = {}

    def get(w, h, kpts, scale=1.2, levels=1, ini=20, mn=7, max_images=1, reserve=0):
        key = (w, h, kpts, scale, levels, ini, mn, max_images, reserve)
        if key not in cache:
            cache[key] = hiplib.Context(w, h, kpts, scale, levels, ini, mn, max_images=max_images)
            if reserve:
                cache[key].set_mapping_reserve(reserve)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


_REFERENCE = {}


def _reference(oracle, key, img, kpts, scale, levels, ini, mn):
    """the oracle's answer, computed once per case and shared (the queued tests repeat cases of the direct ones)"""
    key = (key, img.shape, kpts, scale, levels, ini, mn)
    if key not in _REFERENCE:
        okp, od, occ, opyr = oracle.extract(img, oracle.params(kpts, scale, levels, ini, mn), True)
        _REFERENCE[key] = (okp, od, occ, opyr, [oracle.fast_level(lv, ini, mn) for lv in opyr])
    return _REFERENCE[key]


def _compare(ctx, slot, ref):
    """pyramid, candidates, keypoints and descriptors of one slot against the oracle; returns the device's candidates per level"""
    okp, od, occ, opyr, ocand = ref
    got = []
    for l in range(len(opyr)):
        assert np.array_equal(ctx.pyramid_level(slot, l), opyr[l]), "pyramid level %d" % l
        gc = ctx.candidates(slot, l)
        assert len(gc) == occ[l] == len(ocand[l]), "candidate count of level %d" % l
        assert np.array_equal(ocand[l], gc), "FAST candidates level %d" % l
        got.append(gc)
    gkp, gd = ctx.keypoints(slot)
    _assert_same_keypoints(okp, od, gkp, gd)
    return got


def _run(ctx, images):
    for i, im in enumerate(images):
        ctx.upload(i, im)
    ctx.extract(len(images))


# ---- candidate-count boundaries of k_distribute ------------------------------------------------------------------------------
def _dot_case(contexts, oracle, n, kind, reserve=0):
    img = fc.dot_image(n, kind)
    h, w = img.shape
    for budget in fc.dot_budgets(n):
        ctx = contexts(w, h, budget, reserve=reserve)
        _run(ctx, [img])
        assert ctx.quota == [budget] and ctx.level_w == [w] and ctx.level_h == [h]
        cand = _compare(ctx, 0, _reference(oracle, ("dots", n, kind), img, budget, 1.2, 1, 20, 7))[0]
        fc.check_dots(cand, ctx.keypoints(0)[0], n, kind, budget)


@pytest.mark.parametrize("n,kind", [(n, "equal") for n in fc.DOT_COUNTS] + fc.DOT_KINDS_EXTRA)
def test_candidate_count_boundaries(contexts, oracle, n, kind):
    """1 ... 26000 planted corners on one level, all of one score (ties everywhere: the split order, the first maximum in candidate
    order and newest-first emission decide everything) or with a planted ranking: 1 ... 24 register slots per thread, the 16-byte
    load path (4096, 24575, 24576), candidates in the global scratch (24577, 26000); budgets far below the count and around it."""
    _dot_case(contexts, oracle, n, kind)


# ---- quotas ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kpts", sorted(fc.QUOTA_CASES))
def test_zero_quotas(contexts, oracle, kpts):
    """levels with a quota of 0 still return the first split pass of their roots"""
    w, h = fc.QUOTA_SHAPE
    img = fc.noise(w, h, 1)
    ctx = contexts(w, h, kpts, levels=8)
    _run(ctx, [img])
    assert ctx.quota == fc.QUOTA_CASES[kpts] and 0 in ctx.quota
    cand = _compare(ctx, 0, _reference(oracle, "quota", img, kpts, 1.2, 8, 20, 7))
    fc.check_zero_quota(cand, ctx.keypoints(0)[0], ctx.quota)


def test_quota_limit(contexts, oracle, hiplib):
    """2000 keypoints on one level run and match; 2001 are refused"""
    w, h = 640, 480
    img = fc.noise(w, h, 2)
    ctx = contexts(w, h, fc.QUOTA_MAX)
    _run(ctx, [img])
    assert ctx.quota == [fc.QUOTA_MAX]
    cand = _compare(ctx, 0, _reference(oracle, "quota2000", img, fc.QUOTA_MAX, 1.2, 1, 20, 7))[0]
    fc.check_quota_limit(cand, ctx.keypoints(0)[0])
    with pytest.raises(hiplib.LpslamHipError, match="lpslam_hip error 1:"):            # LPSLAM_HIP_ERR_INVALID
        hiplib.Context(w, h, fc.QUOTA_MAX + 1, 1.2, 1, max_images=1)


# ---- cell edges --------------------------------------------------------------------------------------------------------------
def _edge_case(contexts, oracle, lw, lh, reserve=0):
    w, h, levels, level = fc.edge_context(lw, lh)
    img = fc.noise(w, h, 4)
    ctx = contexts(w, h, 100, scale=fc.EDGE_SCALE, levels=levels, reserve=reserve)
    _run(ctx, [img])
    assert ctx.level_w[level] == lw and ctx.level_h[level] == lh
    cand = _compare(ctx, 0, _reference(oracle, "edge", img, 100, fc.EDGE_SCALE, levels, 20, 7))[level]
    fc.check_edge(cand, lw, lh)


@pytest.mark.parametrize("lw,lh", fc.edge_shapes() + [(64, 64), (46, 46)])
def test_cell_edges(contexts, oracle, lw, lh):
    """levels whose last FAST cell is 7, 8, 9, 63, 64 or 70 px wide or high, or absorbed by the cell before it"""
    _edge_case(contexts, oracle, lw, lh)


# ---- thresholds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ini,mn", fc.THRESHOLDS)
def test_thresholds(contexts, oracle, ini, mn):
    """thresholds at both ends and in either order, on noise, on checkerboards of period 1 and 2 and on the pattern on which every
    pixel passes the pre-test (full queues).  (0, 0) on noise is the regression case of the suppression: a corner of strength 1 has
    score 0 and never survives it; the device once kept such corners (1953 candidates against the oracle's 1950 on this image)."""
    w, h = fc.THRESHOLD_SHAPE
    images = fc.threshold_images()
    ctx = contexts(w, h, 300, levels=2, ini=ini, mn=mn, max_images=len(images))
    _run(ctx, list(images.values()))
    count = {}
    for slot, (name, img) in enumerate(images.items()):
        count[name] = len(_compare(ctx, slot, _reference(oracle, ("thr", name), img, 300, 1.2, 2, ini, mn))[0])
    fc.check_threshold_counts(count, ini, mn)


# ---- extreme aspect ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.ASPECT_CASES + [fc.transpose_case(c) for c in fc.ASPECT_CASES], ids=lambda c: "%dx%d" % c[:2])
def test_extreme_aspect(contexts, oracle, case):
    """the widest and the tallest context there is, and the widest with eight levels (resize tables beyond 64 KB of LDS); budgets
    below what the levels hold, so that the distribution stops at the quota"""
    w, h, levels, scale, kpts = case
    img = fc.noise(w, h, 5)
    t = fc.level_table(w, h, kpts, scale, levels)
    ctx = contexts(w, h, kpts, scale=scale, levels=levels)
    _run(ctx, [img])
    assert ctx.level_w == t["w"] and ctx.level_h == t["h"] and ctx.quota == t["quota"] and max(w, h) == 4133
    cand = _compare(ctx, 0, _reference(oracle, "aspect", img, kpts, scale, levels, 20, 7))
    fc.check_aspect(cand, ctx.keypoints(0)[0], t)


def _root_case(w, h, transposed):
    return (h, w) if transposed else (w, h)


@pytest.mark.parametrize("transposed", [False, True], ids=["columns", "rows"])
@pytest.mark.parametrize("n_roots", [255, 256])
def test_root_counts_up_to_256(contexts, oracle, n_roots, transposed):
    """level 1 of a two-level context with 255 and 256 root columns (rows): the last the byte tables of k_distribute tell apart"""
    w, h = _root_case(fc.ROOT_SHAPES[n_roots], 64, transposed)
    img = fc.noise(w, h, fc.ROOT_SEED)
    t = fc.level_table(w, h, fc.ROOT_BUDGET, fc.ROOT_SCALE, 2)
    assert max(t["roots"][1]) == n_roots
    ctx = contexts(w, h, fc.ROOT_BUDGET, scale=fc.ROOT_SCALE, levels=2)
    _run(ctx, [img])
    assert ctx.level_w == t["w"] and ctx.level_h == t["h"] and min(ctx.level_w[1], ctx.level_h[1]) == 46
    cand = _compare(ctx, 0, _reference(oracle, "roots", img, fc.ROOT_BUDGET, fc.ROOT_SCALE, 2, 20, 7))[1]
    fc.check_roots(cand, ctx.level_w[1], ctx.level_h[1], n_roots)


@pytest.mark.parametrize("transposed", [False, True], ids=["columns", "rows"])
@pytest.mark.parametrize("n_roots", [257, 300])
def test_root_counts_beyond_256_are_refused(hiplib, n_roots, transposed):
    """Before the check in build_level_table the device put every corner beyond root 255 into root 255 and disagreed with the oracle."""
    w, h = _root_case(fc.ROOT_SHAPES[n_roots], 64, transposed)
    assert max(fc.level_table(w, h, fc.ROOT_BUDGET, fc.ROOT_SCALE, 2)["roots"][1]) == n_roots
    with pytest.raises(hiplib.LpslamHipError, match="lpslam_hip error 1: level 1 .*quad-tree roots"):
        hiplib.Context(w, h, fc.ROOT_BUDGET, fc.ROOT_SCALE, 2, max_images=1)


# ---- batches -----------------------------------------------------------------------------------------------------------------
def test_batch_of_65_images(contexts, oracle):
    """65 images in one extraction (four pyramid bands per image, the fewest there are) and one by one on a second context"""
    b = fc.BATCH
    images = [fc.noise(b["w"], b["h"], 100 + i) for i in range(b["n"])]
    refs = [_reference(oracle, ("batch", i), im, b["kpts"], b["scale"], b["levels"], 20, 7) for i, im in enumerate(images)]
    ctx = contexts(b["w"], b["h"], b["kpts"], scale=b["scale"], levels=b["levels"], max_images=b["n"])
    assert b["n"] >= 64 and ctx.level_h[1] == 53
    _run(ctx, images)
    for i in range(b["n"]):
        _compare(ctx, i, refs[i])
    single = contexts(b["w"], b["h"], b["kpts"], scale=b["scale"], levels=b["levels"], max_images=1)
    for i in range(b["n"]):
        _run(single, [images[i]])
        _compare(single, 0, refs[i])


# ---- queued kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fc.DOT_QUEUED)
def test_queued_candidate_counts(contexts, oracle, n):
    """the queued kernels (mapping reserve 8) share the bodies and loop over items"""
    _dot_case(contexts, oracle, n, "equal", reserve=8)


def test_queued_zero_quota_and_smallest_level(contexts, oracle):
    w, h = fc.QUOTA_SHAPE
    img = fc.noise(w, h, 1)
    ctx = contexts(w, h, 5, levels=8, reserve=8)
    _run(ctx, [img])
    assert ctx.quota == fc.QUOTA_CASES[5]
    _compare(ctx, 0, _reference(oracle, "quota", img, 5, 1.2, 8, 20, 7))
    _edge_case(contexts, oracle, 46, 46, reserve=8)
