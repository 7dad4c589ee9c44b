"""The planted front-end cases of tests/frontend_cases.py sit in their regimes: shown on the CPU oracle alone, before any GPU run.
Conditions, not tolerances: candidate counts, quota vectors, level sizes, cell widths, root counts, distinct scores, threshold retries."""
import numpy as np
import pytest

import frontend_cases as fc


def _extract(oracle, img, kpts, scale=1.2, levels=1, ini=20, mn=7):
    okp, od, occ, opyr = oracle.extract(img, oracle.params(kpts, scale, levels, ini, mn), True)
    return okp, [oracle.fast_level(lv, ini, mn) for lv in opyr], occ


def _same_geometry(oracle, w, h, kpts, scale, levels):
    """frontend_cases.level_table agrees with the oracle's own sizes and quotas"""
    t = fc.level_table(w, h, kpts, scale, levels)
    p = oracle.params(kpts, scale, levels)
    assert (t["w"], t["h"]) == tuple(oracle.pyramid_sizes(w, h, p)) and t["quota"] == oracle.keypts_per_level(p)
    return t


@pytest.mark.parametrize("n,kind", [(n, "equal") for n in fc.DOT_COUNTS] + fc.DOT_KINDS_EXTRA)
def test_dots_give_their_count(oracle, n, kind):
    img = fc.dot_image(n, kind)
    h, w = img.shape
    assert (w, h) <= (1280, 1000) and fc.widest_step(w, h, n) >= 4
    for budget in fc.dot_budgets(n):
        kp, cand, occ = _extract(oracle, img, budget)
        assert occ[0] == n and oracle.keypts_per_level(oracle.params(budget, 1.2, 1)) == [budget]
        fc.check_dots(cand[0], kp, n, kind, budget)
    x, y = fc.dot_positions(w, h, n, fc.widest_step(w, h, n))
    assert np.array_equal(np.sort(cand[0], order=("y", "x"))["x"], x - fc.EDGE) and (np.sort(cand[0]["y"]) == np.sort(y - fc.EDGE)).all()
    scores = img[y, x].astype(int) - fc.BACKGROUND - 1
    assert np.array_equal(np.sort(cand[0]["score"]), np.sort(scores))


def test_dot_counts_cover_the_regimes_of_the_distribution():
    r = {n: fc.distribute_regime(n) for n in fc.DOT_COUNTS}
    assert [r[n][0] for n in fc.DOT_COUNTS] == [1, 1, 1, 1, 2, 4, 5, 5, 24, 24, 24, 24]            # register slots per thread
    assert [r[n][1] for n in fc.DOT_COUNTS] == [False] * 5 + [True, False, False] + [True] * 4      # 16-byte loads
    assert [r[n][2] for n in fc.DOT_COUNTS] == [0] * 10 + [1, 1424]                                 # candidates in global scratch
    assert any(len(fc.dot_budgets(n)) == 4 for n in fc.DOT_COUNTS) and all(max(fc.dot_budgets(n)) <= fc.QUOTA_MAX for n in fc.DOT_COUNTS)


@pytest.mark.parametrize("kpts", sorted(fc.QUOTA_CASES))
def test_zero_quota_cases(oracle, kpts):
    w, h = fc.QUOTA_SHAPE
    assert oracle.keypts_per_level(oracle.params(kpts, 1.2, 8)) == fc.QUOTA_CASES[kpts]
    _same_geometry(oracle, w, h, kpts, 1.2, 8)
    kp, cand, _ = _extract(oracle, fc.noise(w, h, 1), kpts, levels=8)
    fc.check_zero_quota(cand, kp, fc.QUOTA_CASES[kpts])


def test_quota_limit_case(oracle):
    assert oracle.keypts_per_level(oracle.params(fc.QUOTA_MAX, 1.2, 1)) == [fc.QUOTA_MAX]
    kp, cand, _ = _extract(oracle, fc.noise(640, 480, 2), fc.QUOTA_MAX)
    fc.check_quota_limit(cand[0], kp)


@pytest.mark.parametrize("lw,lh", fc.edge_shapes() + [(64, 64), (46, 46)])
def test_edge_shapes_reach_their_level(oracle, lw, lh):
    w, h, levels, level = fc.edge_context(lw, lh)
    assert min(w, h) >= 64
    t = _same_geometry(oracle, w, h, 100, fc.EDGE_SCALE, levels)
    assert (t["w"][level], t["h"][level]) == (lw, lh)
    for n in (lw, lh):
        if n - 2 * fc.EDGE in fc.EDGE_CELLS:
            assert fc.cell_grid(n) == fc.EDGE_CELLS[n - 2 * fc.EDGE]
    _, cand, _ = _extract(oracle, fc.noise(w, h, 4), 100, fc.EDGE_SCALE, levels)
    fc.check_edge(cand[level], lw, lh)


def test_edge_sweep_covers_every_span_on_both_axes():
    shapes = fc.edge_shapes()
    assert {a - 38 for a, _ in shapes} == set(fc.EDGE_SPANS) == {b - 38 for _, b in shapes} and len(shapes) == 2 * len(fc.EDGE_SPANS)


def test_threshold_cases_take_or_skip_the_retry(oracle):
    images = fc.threshold_images()

    def n(name, ini, mn):
        return len(oracle.fast_level(images[name], ini, mn))
    for ini, mn in fc.THRESHOLDS:
        fc.check_threshold_counts({k: n(k, ini, mn) for k in images}, ini, mn)
    # (0, 0): the noise has corners of strength 1 (score 0), which cv::FAST's suppression never keeps: the device kept them once
    weak = oracle.fast(images["noise"], 0, nms=False)
    assert (weak["score"] == 0).any() and (oracle.fast_level(images["noise"], 0, 0)["score"] > 0).all()
    # (255, 7): nothing at 255, every cell is redone at 7
    assert n("noise", 255, 255) == 0 and n("noise", 255, 7) == n("noise", 7, 7) > 0
    # (5, 30) and (20, 20): no retry -- the result is that of the initial threshold, not of the minimum
    assert n("noise", 5, 30) == n("noise", 5, 5) != n("noise", 30, 30) and n("noise", 20, 20) > 0
    # the flat left part (two cell columns) of this image has corners at 7 only: (20, 7) takes the retry in some cells and not in others
    img = images["noise"].copy(); img[:, :156] = (img[:, :156] // 16) + 100
    a, b, c = (len(oracle.fast_level(img, i, m)) for i, m in ((20, 20), (20, 7), (7, 7)))
    assert a < b < c
    # full queues: every pixel of the weave passes the pre-test at 0 and at 20, none of the period-1 board's does
    inner = (slice(3, -3), slice(3, -3))
    for thr in (0, 5, 20):
        assert fc.pretest(images["weave"], thr)[inner].all() and not fc.pretest(images["board1"], thr).any()
    assert not fc.pretest(images["weave"], 255).any() and 0 < fc.pretest(images["noise"], 20)[inner].mean() < 1
    assert fc.cell_grid(fc.THRESHOLD_SHAPE[0])[0] == 70 and fc.cell_grid(fc.THRESHOLD_SHAPE[1])[0] == 70      # a full 64 x 64 cell


@pytest.mark.parametrize("case", fc.ASPECT_CASES + [fc.transpose_case(c) for c in fc.ASPECT_CASES], ids=lambda c: "%dx%d" % c[:2])
def test_aspect_cases_stop_at_their_quota(oracle, case):
    w, h, levels, scale, kpts = case
    t = _same_geometry(oracle, w, h, kpts, scale, levels)
    assert max(w, h) == 4133 and max(t["quota"]) <= fc.QUOTA_MAX and all(max(r) <= fc.ROOT_AXIS_MAX for r in t["roots"])
    kp, cand, _ = _extract(oracle, fc.noise(w, h, 5), kpts, scale, levels)
    fc.check_aspect(cand, kp, t)


@pytest.mark.parametrize("transposed", [False, True], ids=["columns", "rows"])
@pytest.mark.parametrize("n_roots", sorted(fc.ROOT_SHAPES))
def test_root_shapes_have_their_roots(oracle, n_roots, transposed):
    w, h = fc.ROOT_SHAPES[n_roots], 64
    if transposed:
        w, h = h, w
    t = _same_geometry(oracle, w, h, fc.ROOT_BUDGET, fc.ROOT_SCALE, 2)
    assert max(t["roots"][1]) == n_roots and min(t["roots"][1]) == 1 and max(t["quota"]) <= fc.QUOTA_MAX
    _, cand, _ = _extract(oracle, fc.noise(w, h, fc.ROOT_SEED), fc.ROOT_BUDGET, fc.ROOT_SCALE, 2)
    fc.check_roots(cand[1], t["w"][1], t["h"][1], n_roots)
    # beyond root 255 the oracle keeps spreading corners: the device's byte tables cannot follow it there
    along = cand[1]["y" if transposed else "x"]
    beyond = int((along / ((max(t["w"][1], t["h"][1]) - 2 * fc.EDGE) / n_roots) >= 256).sum())
    assert (beyond > 0) == (n_roots > fc.ROOT_AXIS_MAX)


def test_batch_case(oracle):
    b = fc.BATCH
    t = _same_geometry(oracle, b["w"], b["h"], b["kpts"], b["scale"], b["levels"])
    assert b["n"] >= 64 and t["h"] == [64, 53] and min(t["h"][1], t["w"][1]) > 2 * fc.EDGE + 7
    kp, cand, _ = _extract(oracle, fc.noise(b["w"], b["h"], 100), b["kpts"], b["scale"], b["levels"])
    assert len(kp) > 0 and all(len(c) > 0 for c in cand)
