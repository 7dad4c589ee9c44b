"""tests/solve_cases.py proved without a device: the matrices are what the table says, the references are converged, and a plain
float64 Cholesky solve sits far inside the bound n kappa_2 2^-53 that tests/test_ba_solve_gpu.py holds the device to."""
import numpy as np
import pytest

import solve_cases as sc

SYNTH = [(n, i) for n in sc.DIMS for i in range(len(sc.synthetic_cases(n)) if n < 1000 else 1)]


def _case(n, i):
    return sc.synthetic_cases(n)[i]


def test_dims_are_the_boundary_table():
    assert sc.DIMS == (6, 18, 30, 36, 48, 54, 66, 96, 102, 114, 132, 300, 306, 600, 1194)
    assert sc.WG_MAX_DIM + 1 <= 16 * 19 < sc.DIMS[sc.DIMS.index(sc.WG_MAX_DIM) + 1] + 1      # cw_fits: 19 tile rows of 16


@pytest.mark.parametrize("n", sc.DIMS)
def test_known_family_is_exact(n):
    c = sc.known(n)
    L, A, x, b = c["L_int"], c["A_int"], c["x_int"], c["b_int"]
    assert np.array_equal(np.tril(L), L) and (np.diag(L) == sc.KNOWN_DIAG).all()
    for col in sc.DENSE_COLS + (n - 1,):
        if col < n:
            assert (np.abs(L[col + 1:, col]) == 1).all(), "column %d is dense" % col
    assert np.array_equal(A, L @ L.T) and np.array_equal(b, A @ x)
    assert np.abs(A).max() < 2 ** 30 and c["kappa"] < 1e4
    # exact in float64 too, and no tile of the lower triangle is empty
    assert np.array_equal(c["A"].astype(np.int64), A) and np.array_equal(c["b"].astype(np.int64), b)
    for r in range(0, n, 16):
        for q in range(0, r + 1, 16):
            assert np.any(A[r:r + 16, q:q + 16] != 0)
    assert sc.forward_error(sc.host_solve(c["A"], c["b"]), c["x"]) <= sc.bound(c) / 16


@pytest.mark.parametrize("n,k", [(n, k) for n in sc.DIMS if n < 1000 for k in ((2, 6, 10, 12) if n in sc.WIDE_DIMS else (2, 10))])
def test_ladder_condition_is_as_designed(n, k):
    c = sc.ladder(n, k)
    assert c["family"] == "ladder%d" % k and any(c is s for s in sc.synthetic_cases(n))
    assert 0.5 * 10.0 ** k <= c["kappa"] <= 2.0 * 10.0 ** k
    w = np.linalg.eigvalsh(c["A"])
    assert w.min() > 0 and abs(w.max() - 1.0) < 1e-12


@pytest.mark.parametrize("n", sc.WIDE_DIMS)
@pytest.mark.parametrize("sign", (+1, -1))
def test_graded_condition(n, sign):
    """D A D with kappa(A) = 100 and D of 1 and 10^+-3: between kappa(D)^2 / kappa(A) and kappa(D)^2 kappa(A)"""
    c = sc.graded(n, sign)
    assert 1e6 / 100 <= c["kappa"] <= 1e6 * 100
    d = np.sqrt(np.diag(c["A"]) / np.diag(sc.ladder(n, 2)["A"]))
    want = np.where((np.arange(n) // 3) % 2 == 1, 10.0 ** (3 * sign), 1.0)
    assert np.allclose(d, want, rtol=1e-12)


@pytest.mark.parametrize("n,i", SYNTH)
def test_reference_and_host_error(n, i):
    c = _case(n, i)
    assert c["pd"] and np.array_equal(c["A"], c["A"].T)
    assert c["residual"] < 1e-17, "refinement ended at a normwise residual of %.3g" % c["residual"]
    assert sc.residual_norm(c["A"], c["b"], c["x"]) < 1e-17
    assert c["e_host"] <= sc.bound(c) / 16, (c["family"], c["e_host"], sc.bound(c))


@pytest.mark.parametrize("n,p,where", sc.NOTPD)
def test_not_positive_definite_where_meant(n, p, where):
    good, bad = sc.notpd(n, p)
    assert good["pd"] and not bad["pd"]
    assert good["residual"] < 1e-17 and good["e_host"] <= sc.bound(good) / 16
    assert np.isfinite(bad["A"]).all() and np.array_equal(bad["A"], bad["A"].T)
    w = np.linalg.eigvalsh(bad["A"])
    assert (w < 0).sum() == 1 and -w.min() >= 1e-3 * np.abs(w).max(), "one eigenvalue, clearly negative"
    # the flip is 2 lambda_k v_k v_k^T of an eigenpair of the positive definite matrix
    diff = good["A"] - bad["A"]
    lam, vec = np.linalg.eigh(diff)
    assert abs(lam[-1] - 2.0) < 1e-12 and np.abs(lam[:-1]).max() < 1e-12
    assert np.allclose(good["A"] @ vec[:, -1], vec[:, -1], atol=1e-12)
    assert sc.first_failing_pivot(bad["A"]) == p, where
    # which strip, panel and launch that pivot belongs to
    nb = (n + 1 + 31) // 32
    panel, strip_b = p // 32, (p % 32) >= 16
    if "strip A of the first" in where:
        assert panel == 0 and not strip_b
    if "strip B of the first" in where:
        assert panel == 0 and strip_b
    if "second column of a pair" in where:
        assert panel % 2 == 1 and panel + 1 < nb
    if "single" in where:
        assert nb % 2 == 1 and panel == nb - 1
    if "trimmed" in where:
        assert panel == nb - 1 and n - 32 * (nb - 1) < 32
    if "cw_fits" in where:
        assert n == sc.WG_MAX_DIM
    if "chain only" in where:
        assert n > sc.WG_MAX_DIM


@pytest.mark.parametrize("n,p", sc.ZERO_PIVOT)
def test_zero_pivot(n, p):
    c = sc.zero_pivot(n, p)
    assert not c["pd"] and np.isfinite(c["A"]).all()
    assert not c["A"][p].any() and not c["A"][:, p].any()
    assert sc.first_failing_pivot(c["A"]) == p
