"""The banded window solve held to an exact solution: lpslam_hip_ba_debug_solve takes (A, b) of a problem on the band solver through
k_chol_band as a solve launches it -- strips of 16 through the ring of 96 rows, from 12 strips on twisted (a helper workgroup eliminates
the last strips bottom-up and hands a 64 x 64 block to the main chain) -- and x comes back to be compared with the exact (integer
family) or long-double-refined solution of tests/solve_cases.py.

    e_dev = ||x_dev - x*||_inf / ||x*||_inf  <=  n kappa_2(A) 2^-53        the first-order bound of a Cholesky solve; no measurement in it
    e_dev <= M_BAND max(e_host, 2^-53)                                    regression margin against a float64 Cholesky on the host

M_BAND = 64: the smallest power of two >= 2 x the largest ratio measured on an MI355X over every case here, 19.56 (dim 294, known-band,
where e_host is exactly 0 and the ratio is e_dev / 2^-53; profiles/solve_accuracy_band.txt, tools/solve_accuracy.py band; DESIGN.md 39;
the factor 2 is what a re-ordered sum may move an error by).

The dimensions are those of every boundary the kernel has (solve_cases.BAND_DIMS); the scalar half-bandwidth is min(59, dim - 1), and 5
and 23 on holders whose block half-bandwidth is 0 and 3.  Same bytes alone, in a batch, beside dense problems, again and on another
problem's buffers; the upper triangle is never read; the pivot flag equals "numpy's Cholesky fails", with the first failing pivot placed
in chosen strips of the main chain and of the helper, and a flagged solve returns the zero step."""
import numpy as np
import pytest

import solve_cases as sc
import solve_runner as sr

pytestmark = pytest.mark.gpu

M_BAND = 64
REAL_AT = {6 * free: (free, hbw) for free, hbw in sr.REAL_BAND}      # dims 54, 180, 300


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def holders(hiplib, ctx):
    h = sr.BandHolders(hiplib, ctx)
    yield h
    h.close()


@pytest.fixture(scope="module")
def dense_holders(hiplib, ctx):
    h = sr.Holders(hiplib, ctx)
    yield h
    h.close()


@pytest.fixture(scope="module")
def cases_of(hiplib, ctx):
    """dimension -> its positive definite cases at the full width (computed once: the references are the expensive part)"""
    memo = {}

    def get(n):
        if n not in memo:
            memo[n] = list(sc.band_cases(n))
            if n in REAL_AT:
                memo[n].append(sr.real_band_case(hiplib, ctx, *REAL_AT[n]))
        return memo[n]
    return get


def check(case, x, flag):
    r = sr.row(case, x, sr.BAND)
    print(sr.format_row(r))
    assert flag == 0, "pivot flag on a positive definite system (%d, %s)" % (case["n"], case["family"])
    assert np.isfinite(x).all()
    assert r["e_dev"] <= r["bound"], "forward error %.3g beyond n kappa 2^-53 = %.3g (%d, %s %s)" % (r["e_dev"], r["bound"], case["n"], case["family"], case["tag"])
    assert r["e_dev"] <= M_BAND * max(case["e_host"], sc.U), "forward error %.3g is %.1f x the host's (%d, %s %s)" % (r["e_dev"], r["ratio"], case["n"], case["family"], case["tag"])


@pytest.mark.parametrize("n", sc.BAND_DIMS)
def test_forward_error_band(holders, cases_of, n):
    """every case of the dimension at the full width min(59, n - 1), one problem per call"""
    print("\n" + sr.HEADER)
    for c in cases_of(n):
        x, flag = holders.alone(c)
        check(c, x, flag)


@pytest.mark.parametrize("w,n", sc.BAND_NARROW)
def test_narrow_bands(holders, w, n):
    """scalar half-bandwidth 5 (block-diagonal: nothing couples) and 23, on holders whose band_hbw is 0 and 3"""
    hbw = (w - 5) // 6
    assert holders.take(n, 1, hbw)[0].solver() == ("band", hbw)
    print("\n" + sr.HEADER)
    for c in sc.narrow_band_cases(n, w):
        assert holders.holder_for(c) is holders.take(n, 1, hbw)[0]
        x, flag = holders.alone(c)
        check(c, x, flag)


def test_entries_outside_the_holder_band_are_refused(hiplib, holders):
    """a matrix of half-bandwidth 53 on a holder of block half-bandwidth 3 (scalar 23)"""
    c = sc.known_band(54)
    with pytest.raises(hiplib.LpslamHipError, match="not zero"):
        holders.solve(holders.take(54, 1, 3), [c])
    edge = sc.known_band(54, 23)
    x, flag = holders.solve(holders.take(54, 1, 3), [edge])
    check(edge, x[0], flag[0])


# ---- same bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.BAND_DIMS)
def test_same_bytes_alone_in_a_batch_again_and_elsewhere(holders, n):
    a, b = sc.ladder_band(n, 10), sc.known_band(n)
    xa, fa = holders.alone(a)
    xb, fb = holders.alone(b)
    assert fa == 0 and fb == 0
    xs, flags = holders.batch([a, b, b, a])                   # gridDim.y = 4; a and b each on two problems
    assert not any(flags)
    assert xs[0].tobytes() == xa.tobytes() and xs[3].tobytes() == xa.tobytes()
    assert xs[1].tobytes() == xb.tobytes() and xs[2].tobytes() == xb.tobytes()
    assert holders.alone(a)[0].tobytes() == xa.tobytes(), "a second solve on the buffers the first one left"
    assert holders.alone(a, which=3)[0].tobytes() == xa.tobytes(), "another problem's buffers"
    if n >= 180:
        # twisted: three solves in a row on one problem, of two different systems, so that a block or a flag the previous solve left
        # behind would show (the entry fails with LPSLAM_HIP_ERR_DEVICE if a hand-over word is not back at zero behind a solve)
        assert sc.band_layout(n)[1] > 0
        for c, want in ((b, xb), (a, xa), (b, xb)):
            x, flag = holders.alone(c, which=2)
            assert flag == 0 and x.tobytes() == want.tobytes()


def test_mixed_batch_band_and_dense(holders, dense_holders):
    """band problems of dims 54, 180 and 300 beside dense problems of dims 54 and 306 in one call: both launch families run, each kernel
    skips the other's views, and every system gets the bytes it gets alone"""
    band = [sc.ladder_band(54, 10), sc.known_band(180), sc.ladder_band(300, 10)]
    dense = [sc.ladder(54, 10), sc.known(306)]
    probs = [holders.holder_for(band[0]), dense_holders.take(54)[0], holders.holder_for(band[1]), dense_holders.take(306)[0], holders.holder_for(band[2])]
    cases = [band[0], dense[0], band[1], dense[1], band[2]]
    assert [p.solver()[0] for p in probs] == ["band", "dense", "band", "dense", "band"]
    xs, flags = holders.solve(probs, cases)
    assert not any(flags)
    print("\n" + sr.HEADER)
    for i in (0, 2, 4):
        check(cases[i], xs[i], flags[i])
        assert xs[i].tobytes() == holders.alone(cases[i])[0].tobytes(), (cases[i]["n"], cases[i]["family"])
    for i in (1, 3):
        r = sr.row(cases[i], xs[i], sr.CHAIN)
        print(sr.format_row(r))
        assert r["e_dev"] <= r["bound"]
        assert xs[i].tobytes() == dense_holders.alone(cases[i])[0].tobytes(), (cases[i]["n"], cases[i]["family"])


# ---- the upper triangle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (54, 300))
def test_upper_triangle_is_never_read(holders, n):
    """untwisted and twisted (the flipped helper reads F(r, c) = S(n-1-c, n-1-r): the lower triangle too)"""
    for c in (sc.known_band(n), sc.ladder_band(n, 10)):
        x, flag = holders.alone(c)
        A = c["A"].copy()
        A[np.triu_indices(n, 1)] = np.nan
        xs, flags = holders.hip.ba_debug_solve([holders.holder_for(c)], [A], [c["b"]])
        assert int(flags[0]) == 0 and flag == 0
        assert xs[0].tobytes() == x.tobytes()


# ---- the pivot flag -------------------------------------------------------------------------------------------------------------
def _flagged(holders, good, bad):
    """flag == numpy's Cholesky fails; a flagged solve gives the zero step; the next solve on the same problem starts clean"""
    fresh = holders.hip.BundleAdjuster(holders.ctx, *_window_args(holders, good["n"]))
    try:
        assert fresh.solver()[0] == "band"
        xs, flags = holders.solve([fresh], [good])
    finally:
        fresh.close()
    check(good, xs[0], flags[0])
    xb, flag = holders.alone(bad)
    assert not bad["pd"] and not sc.is_pd(bad["A"])
    assert flag == 1, "no pivot flag (%d, %s %s)" % (bad["n"], bad["family"], bad["tag"])
    assert np.isfinite(xb).all() and not xb.any(), "a flagged solve gives the zero step"
    x2, flag = holders.alone(good)
    check(good, x2, flag)
    assert x2.tobytes() == xs[0].tobytes(), "the solve behind a flagged one differs from a solve on fresh buffers"


def _window_args(holders, dim):
    pr = sr.band_window(dim // 6, min(9, dim // 6 - 1))
    return pr["poses"], pr["fixed"], pr["points"], holders.hip.ba_obs_array(pr), pr["cam"]


@pytest.mark.parametrize("n,p,where", sc.BAND_NOTPD_TOP, ids=["%d-p%d" % (n, p) for n, p, _ in sc.BAND_NOTPD_TOP])
def test_pivot_flag_top_down(holders, n, p, where):
    _flagged(holders, *sc.notpd_band(n, p))


@pytest.mark.parametrize("n,q,where", sc.BAND_NOTPD_BOTTOM, ids=["%d-q%d" % (n, q) for n, q, _ in sc.BAND_NOTPD_BOTTOM])
def test_pivot_flag_bottom_up(holders, n, q, where):
    """the first failing pivot is in the helper's strips: its failure reaches the main workgroup with the hand-over"""
    _flagged(holders, *sc.notpd_band(n, q, bottom=True))


@pytest.mark.parametrize("n,p", sc.BAND_ZERO_PIVOT)
def test_zero_pivot_band(holders, n, p):
    _flagged(holders, sc.ladder_band(n, 2), sc.zero_pivot_band(n, p))


def test_pivot_flags_in_one_batch(holders):
    """flagged and positive definite systems side by side in one launch: every view gets its own flag and its own zero step"""
    cases = []
    for n, p in ((54, 20), (180, 70), (300, 100)):
        cases += list(sc.notpd_band(n, p))
    cases += list(sc.notpd_band(180, 47, bottom=True)) + list(sc.notpd_band(300, 111, bottom=True))
    xs, flags = holders.batch(cases)
    for c, x, flag in zip(cases, xs, flags):
        assert flag == (0 if c["pd"] else 1), (c["n"], c["family"], c["tag"])
        if c["pd"]:
            check(c, x, flag)
        else:
            assert np.isfinite(x).all() and not x.any()
