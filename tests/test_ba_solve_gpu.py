"""The dense window solve held to an exact solution: lpslam_hip_ba_debug_solve takes (A, b) through the launches the product's
solve takes -- the panel-pair chain k_chol_pair + k_chol_xsolve for a problem alone, k_chol_wg for the small systems of a batch of
40 -- and x comes back to be compared with the exact (integer family) or long-double-refined solution of tests/solve_cases.py.

    e_dev = ||x_dev - x*||_inf / ||x*||_inf  <=  n kappa_2(A) 2^-53        the first-order bound of a Cholesky solve; no measurement in it
    e_dev <= M max(e_host, 2^-53)                                         regression margin against a float64 Cholesky on the host

M = 32: the smallest power of two >= 2 x the largest ratio measured on an MI355X over every case here, 9.87 (profiles/solve_accuracy.txt,
tools/solve_accuracy.py; DESIGN.md "Accuracy of the dense window solve"; the factor 2 is what a re-ordered sum may move an error by).

The dimensions are those of the panel, strip and launch boundaries (solve_cases.DIMS); the matrices are ill conditioned up to
kappa = 1e12, graded like rotation against translation columns, real (S + lambda I of three windows, read through the step API), and not
positive definite with the first failing pivot placed in every kind of strip: the pivot flag equals "numpy's Cholesky fails".
Finite inputs only; control flow in these kernels does not depend on data."""
import numpy as np
import pytest

import solve_cases as sc
import solve_runner as sr

pytestmark = pytest.mark.gpu

M = 32
BYTES_DIMS = (18, 54, 132, 306, 600)


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def holders(hiplib, ctx):
    h = sr.Holders(hiplib, ctx)
    yield h
    h.close()


@pytest.fixture(scope="module")
def cases_of(hiplib, ctx):
    """dimension -> its positive definite cases (computed once: the references are the expensive part)"""
    memo = {}

    def get(n):
        if n not in memo:
            memo[n] = list(sc.synthetic_cases(n))
            if n in sc.WIDE_DIMS:
                memo[n] += [sr.real_case(hiplib, ctx, kind, n // 6) for kind in sr.REAL_KINDS]
        return memo[n]
    return get


def check(case, x, flag, kernel):
    r = sr.row(case, x, kernel)
    print(sr.format_row(r))
    assert flag == 0, "pivot flag on a positive definite system (%d, %s, %s)" % (case["n"], case["family"], kernel)
    assert np.isfinite(x).all()
    assert r["e_dev"] <= r["bound"], "forward error %.3g beyond n kappa 2^-53 = %.3g (%d, %s, %s)" % (r["e_dev"], r["bound"], case["n"], case["family"], kernel)
    assert r["e_dev"] <= M * max(case["e_host"], sc.U), "forward error %.3g is %.1f x the host's (%d, %s, %s)" % (r["e_dev"], r["ratio"], case["n"], case["family"], kernel)


@pytest.mark.parametrize("n", sc.DIMS)
def test_forward_error_chain(holders, cases_of, n):
    """every case of the dimension through the panel-pair chain (one problem per call)"""
    print("\n" + sr.HEADER)
    for c in cases_of(n):
        x, flag = holders.alone(c)
        check(c, x, flag, sr.CHAIN)


@pytest.mark.parametrize("n", [n for n in sc.DIMS if n <= sc.WG_MAX_DIM])
def test_forward_error_wg(holders, cases_of, n):
    """... and inside a batch of 40 problems, where k_chol_wg takes them"""
    print("\n" + sr.HEADER)
    cases = cases_of(n)
    xs, flags, launches = holders.wg_batch(cases)
    assert launches == 1, "the batch did not go through k_chol_wg"
    for c, x, flag in zip(cases, xs, flags):
        check(c, x, flag, sr.WG)
    holders.drop(n)                                     # 40 problems of this size: not kept for the rest of the module


def test_mixed_batch_runs_both_kernels(holders):
    """dims 18 and 300 (k_chol_wg) beside 306 and 600 (the chain, which skips the small ones) in one batch of 40: every system gets the
    bytes its kernel gives it elsewhere"""
    small = [sc.ladder(18, 10), sc.known(300), sc.ladder(300, 10), sc.graded(18, +1)]
    large = [sc.ladder(306, 10), sc.known(600)]
    full = [small[i % 4] for i in range(sr.CW_MIN_BATCH - 2)] + large
    xs, flags, launches = holders.batch(full)
    assert launches == 1 and not any(flags)
    print("\n" + sr.HEADER)
    for c, x in zip(full[:4], xs[:4]):
        check(c, x, 0, sr.WG)
    for c, x in zip(large, xs[-2:]):
        check(c, x, 0, sr.CHAIN)
    for i, c in enumerate(full[:-2]):
        assert xs[i].tobytes() == xs[i % 4].tobytes(), "copies of one system differ inside the batch"
    wg_only, _, _ = holders.wg_batch(small)
    for c, a, b in zip(small, xs[:4], wg_only):
        assert a.tobytes() == b.tobytes(), (c["n"], c["family"])
    for c, a in zip(large, xs[-2:]):
        assert a.tobytes() == holders.alone(c)[0].tobytes(), (c["n"], c["family"])
    holders.drop(18); holders.drop(300)


def test_wg_batch_is_not_the_chain(holders):
    """The launch counter is advanced by the host where it decides for k_chol_wg, so it shows the decision; that another kernel ran shows
    in the bytes: the two kernels sum in different orders (profiles/solve_accuracy.txt: their e_dev differ at most dimensions)."""
    cases = [sc.ladder(n, 10) for n in (36, 66, 132)]
    xs, _, launches = holders.wg_batch(cases)
    assert launches == 1
    assert any(x.tobytes() != holders.alone(c)[0].tobytes() for c, x in zip(cases, xs))
    for n in (36, 66, 132):
        holders.drop(n)


@pytest.mark.parametrize("n", BYTES_DIMS)
def test_same_bytes_alone_in_a_chain_batch_and_again(holders, n):
    a, b = sc.ladder(n, 10), sc.known(n)
    xa, _ = holders.alone(a)
    xb, _ = holders.alone(b)
    xs, flags, launches = holders.batch([a, b])
    assert launches == 0 and not any(flags), "two problems take the chain"
    assert xs[0].tobytes() == xa.tobytes() and xs[1].tobytes() == xb.tobytes()
    assert holders.alone(a)[0].tobytes() == xa.tobytes(), "a second solve on the buffers the first one left"
    assert holders.alone(a, which=1)[0].tobytes() == xa.tobytes(), "another problem's buffers"


# ---- the pivot flag ---------------------------------------------------------------------------------------------------------
def _flag_cases():
    out = []
    for n, p, where in sc.NOTPD:
        good, bad = sc.notpd(n, p)
        out += [good, bad]
    return out + [sc.zero_pivot(n, p) for n, p in sc.ZERO_PIVOT]


@pytest.mark.parametrize("n,p,where", sc.NOTPD, ids=["%d-p%d" % (n, p) for n, p, _ in sc.NOTPD])
def test_pivot_flag_chain(holders, n, p, where):
    """flag == numpy's Cholesky fails; a flagged solve leaves finite numbers, and the next solve on the same problem starts clean"""
    good, bad = sc.notpd(n, p)
    x, flag = holders.alone(good)
    check(good, x, flag, sr.CHAIN)
    xb, flag = holders.alone(bad)
    assert flag == 1 and not bad["pd"], where
    assert np.isfinite(xb).all() and not xb.any(), "a flagged solve gives the zero step"
    x2, flag = holders.alone(good)
    check(good, x2, flag, sr.CHAIN)
    assert x2.tobytes() == x.tobytes()


@pytest.mark.parametrize("n,p", sc.ZERO_PIVOT)
def test_zero_pivot_chain(holders, n, p):
    c = sc.zero_pivot(n, p)
    x, flag = holders.alone(c)
    assert flag == 1 and np.isfinite(x).all() and not x.any()
    good = sc.ladder(n, 2)
    check(good, *holders.alone(good), sr.CHAIN)


def test_pivot_flag_wg(holders):
    """all of them that fit, good and bad side by side in batches of 40; then the good ones on the problems that were flagged"""
    cases = [c for c in _flag_cases() if c["n"] <= sc.WG_MAX_DIM]
    assert len(cases) <= sr.CW_MIN_BATCH
    xs, flags, launches = holders.wg_batch(cases)
    assert launches == 1
    for c, x, flag in zip(cases, xs, flags):
        assert flag == (0 if c["pd"] else 1), (c["n"], c["family"], c["tag"])
        assert np.isfinite(x).all()
        if c["pd"]:
            check(c, x, flag, sr.WG)
        else:
            assert not x.any(), "a flagged solve gives the zero step"
    # the same problems again: every flagged one now solves the positive definite partner (the order within a dimension is kept)
    partner = [c if c["pd"] else (sc.notpd(c["n"], c["p"])[0] if c["family"] == "notpd" else sc.ladder(c["n"], 2)) for c in cases]
    xs, flags, launches = holders.wg_batch(partner)
    assert launches == 1
    for c, x, flag in zip(partner, xs, flags):
        check(c, x, flag, sr.WG)


def test_pivot_flag_rejects_the_trial_on_the_product_path(hiplib, ctx):
    """One LM trial through the step API as dist_ba.PartitionedBA runs it, with S overwritten by a matrix that is not positive definite
    between the reduction and the solve (an all-reducer may write there): the trial is rejected, the state keeps its bytes and lambda
    doubles (g2o: lambda *= ni, ni = 2 -- the oracle's ok = 0 branch).  The next trial, on the real S again, is accepted."""
    pr = sr.real_window("random", 9)
    ba = hiplib.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hiplib.ba_obs_array(pr), pr["cam"])
    ba.set_solver("dense")
    dim = 54
    S, rhs, lam0, n = sr.first_trial_system(ba, dim)
    p0, x0 = ba.state()
    w, v = np.linalg.eigh(S)
    bad = S - 2.0 * w[-1] * np.outer(v[:, -1], v[:, -1])
    bad = 0.5 * (bad + bad.T)
    assert not sc.is_pd(bad + lam0 * np.eye(dim)) and sc.is_pd(S + lam0 * np.eye(dim))
    padded = sr.read_S(ba, n)
    real_S = padded[:dim, :dim].copy()
    padded[:dim, :dim] = bad
    sr.device_write(ba.lib, ba.reduced_buffer()[0], padded)
    ba.step_solve()
    accepted, finished = ba.step_end()
    st = ba.status()
    p1, x1 = ba.state()
    assert not accepted and not finished
    assert p1.tobytes() == p0.tobytes() and x1.tobytes() == x0.tobytes()
    assert st["lam"] == 2.0 * lam0
    # second trial: the reduction puts the real S back -- the Schur complement of the same linearisation for the doubled lambda
    # (lambda sits in (H_ll + lambda I)^-1, so the bytes are not those of the first reduction; nothing of the overwritten matrix is left)
    ba.step_begin(True, False)
    S2 = sr.read_S(ba, n)[:dim, :dim]
    assert sc.is_pd(np.tril(S2) + np.tril(S2, -1).T + 2.0 * lam0 * np.eye(dim))
    assert np.linalg.eigvalsh(np.tril(S2) + np.tril(S2, -1).T).min() > -lam0 and np.abs(S2 - real_S).max() < np.abs(S2 - bad).max()
    ba.step_solve()
    accepted, _ = ba.step_end()
    assert accepted
    p2, _ = ba.state()
    assert p2.tobytes() != p0.tobytes()
    assert 1 / 3 - 1e-12 <= ba.status()["lam"] / (2.0 * lam0) <= 2 / 3 + 1e-12
    ba.close()
