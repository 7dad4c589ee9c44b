"""The planted stereo cases of tests/stereo_cases.py are what they claim, and the numpy restatement of the matcher equals the
oracle bit for bit on every one of them.  No GPU: tests/test_stereo_planted_gpu.py runs the same cases through the kernels.

The exit-reason counts asserted here are conditions on the generator (does every branch of the matcher decide something?), not
measurements of the code under test: they come from the restatement alone."""
import numpy as np
import pytest

import stereo_cases as sc

_solved = {}


def solved(oracle, name):
    """(case, restatement result, oracle result) on the oracle's own pyramids, computed once per case"""
    if name not in _solved:
        case = sc.get_case(name)
        p = oracle.params(case.max_keypoints, 1.2, case.levels)
        pl = oracle.extract(case.left_img, p, True)[3]; pr = oracle.extract(case.right_img, p, True)[3]
        res = sc.restate(pl, pr, case)
        ora = oracle.match_stereo(pl, pr, p, case.kl, case.dl, case.kr, case.dr, case.fxb, case.baseline)
        _solved[name] = (case, res, ora)
    return _solved[name]


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_restatement_equals_oracle(oracle, name):
    case, res, (oxr, odep, obi, n_valid) = solved(oracle, name)
    assert np.array_equal(res.x_right, oxr) and np.array_equal(res.depth, odep) and np.array_equal(res.best_idx, obi)
    assert n_valid == int((res.depth > 0).sum()) == sum(r in ("ok", "zero") for r in res.reason)
    assert "norow" not in res.reason


FLOORS = {"ok": 50, "median": 20, "hamming": 20, "slide_edge": 5, "border": 5, "zero": 5, "emptyrow": 5, "negx": 1, "negdisp": 1, "maxdisp": 1}


@pytest.mark.parametrize("seed", sc.MAIN_SEEDS)
def test_main_case_reaches_every_exit(oracle, seed):
    case, res, _ = solved(oracle, "main/%d" % seed)
    counts = res.counts()
    print(case.name, len(case.kl), len(case.kr), counts)
    for reason, floor in FLOORS.items():
        assert counts.get(reason, 0) >= floor, (reason, counts)
    assert set(counts) == set(FLOORS)


@pytest.mark.parametrize("seed", sc.MAIN_SEEDS)
def test_main_case_plants_resolve_as_intended(oracle, seed):
    case, res, _ = solved(oracle, "main/%d" % seed)
    sc.check_main_plants(case, res.x_right, res.depth, res.best_idx)
    P = case.plants
    # the restatement's reasons for the groups planted for one exit
    for name, reason in (("zero", "zero"), ("maxdisp", "maxdisp"), ("emptyrow", "emptyrow"), ("negx", "negx"), ("h75", "hamming"), ("far_desc", "hamming")):
        assert all(res.reason[g["left"]] == reason for g in P[name]), name
    assert all((res.reason[g["left"]] == "border") == g["refused"] for g in P["border"])
    assert all(res.reason[g["left"]] in ("ok", "median") for g in P["border"] if not g["refused"])
    assert sum(res.reason[g["left"]] == "negdisp" for g in P["negdisp"]) >= len(P["negdisp"]) // 2
    assert sum(res.reason[g["left"]] == "slide_edge" for g in P["slide"]) >= 5
    # the permutation left index order unrelated to position: at least one tie is won by the keypoint planted second
    assert any(min(g["tie"]) == g["tie"][1] for s in sc.MAIN_SEEDS for g in sc.main_case(s).plants["tie"])


def band_rows(case, j):
    rad = np.float32(2.0) * sc.level_geometry(case.w, case.h, case.levels)[0][case.kr["octave"][j]]
    return max(int(np.floor(case.kr["y"][j] - rad)), 0), min(int(np.ceil(case.kr["y"][j] + rad)), case.h - 1)


def test_long_rows_case(oracle):
    case, res, _ = solved(oracle, "long_rows")
    sc.check_long_rows_plants(case, res.best_idx)
    bands = [band_rows(case, j) for j in range(len(case.kr))]
    for row in (70, 170):
        assert sum(lo <= row <= hi for lo, hi in bands) > 3 * 64
        assert sum(int(y) == row for y in case.kl["y"]) == 8
    assert (res.depth > 0).sum() >= 6


def test_large_case(oracle):
    case, res, _ = solved(oracle, "large")
    n = sc.slots_per_image(case.max_keypoints, case.levels)
    assert len(case.kl) == len(case.kr) == n and n > 1024 and n % 4 != 0
    accepted = int((res.corr >= 0).sum())
    print(case.name, res.counts(), "accepted before the cut", accepted)
    assert accepted > 1024                                       # the stride loop of k_stereo_median
    assert res.reason.count("median") > 100 and res.reason.count("ok") > 1024
    assert set(case.kl["octave"]) == set(range(8))


@pytest.mark.parametrize("w,h", sc.TALL_SHAPES)
def test_tall_cases(oracle, w, h):
    case, res, _ = solved(oracle, "tall/%dx%d" % (w, h))
    print(case.name, res.counts())
    assert (h + 1023) // 1024 == (2 if h < 2048 else 3)         # rows per thread of block_scan_rows
    rows = {int(case.kl["y"][g["left"]]) for g in case.plants["rows"]}
    assert set(range(1000, 1095)) <= rows and (h < 2048 or set(range(2046, 2051)) <= rows)
    hit = [g for g in case.plants["rows"] if res.best_idx[g["left"]] == g["right"]]
    assert len(hit) == len(case.plants["rows"])
    assert sum(res.depth[g["left"]] > 0 for g in case.plants["rows"]) > len(rows) // 2
    assert case.kr["y"].min() < 100 and case.kr["y"].max() > h - 100       # right keypoints over the whole height


@pytest.mark.parametrize("n", sc.MEDIAN_COUNTS)
def test_median_cases(oracle, n):
    case, res, _ = solved(oracle, "median/%d" % n)
    sc.check_median_case(case, n, res)
    assert np.array_equal(case.left_img, sc.main_case(1).left_img) and np.array_equal(case.right_img, sc.main_case(1).right_img)


def test_median_zero_case(oracle):
    case, res, _ = solved(oracle, "median/zeros")
    sc.check_median_zero_case(case, res, res.depth)
    assert res.reason == ["zero"] * 3 + ["median"]
