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


# ---- band systems (k_chol_band; tests/test_ba_band_solve_gpu.py) ---------------------------------------------------------------
BAND_PD = [(n, None, i) for n in sc.BAND_DIMS for i in range(len(sc.band_cases(n)))] + \
          [(n, w, i) for w, n in sc.BAND_NARROW for i in range(3)]


def _band_case(n, w, i):
    return sc.band_cases(n)[i] if w is None else sc.narrow_band_cases(n, w)[i]


def _band_is_all_there_is(c):
    """A float64 Cholesky solve that never looks beyond the band returns the bytes of the same operations on the whole matrix; the factor
    host_solve gets from LAPACK is exactly zero outside the band; and the band solve is as good a reference as host_solve.  (The bytes of
    host_solve itself are LAPACK's blocked order of operations, which no second implementation reproduces -- not even at dim 6, where the
    band is the whole matrix.)"""
    Lb, xb = sc.band_cholesky_solve(c["A"], c["b"], c["w"])
    Lf, xf = sc.band_cholesky_solve(c["A"], c["b"], None)
    assert xb.tobytes() == xf.tobytes() and np.array_equal(Lb, Lf)
    assert not np.linalg.cholesky(c["A"])[~sc.band_mask(c["n"], c["w"])].any()
    assert sc.forward_error(xb, c["x"]) <= sc.bound(c) / 8
    assert sc.forward_error(xb, sc.host_solve(c["A"], c["b"])) <= sc.bound(c) / 4


def test_band_dims_are_the_boundary_table():
    assert sc.BAND_DIMS == (6, 12, 18, 30, 48, 54, 66, 84, 96, 102, 114, 132, 162, 174, 180, 192, 198, 222, 228, 258, 276, 294, 300)
    lay = {n: sc.band_layout(n) for n in sc.BAND_DIMS}
    assert [lay[n][0] for n in sc.BAND_DIMS] == [1, 1, 2, 2, 3, 4, 5, 6, 6, 7, 8, 9, 11, 11, 12, 12, 13, 14, 15, 17, 18, 19, 19]
    assert all(lay[n][1] == 0 for n in sc.BAND_DIMS if n <= 174) and lay[174][0] == sc.BAND_TWIST_MIN - 1
    assert lay[180] == (12, 3, 132, 4) and lay[192] == (12, 3, 144, 5) and lay[198][:2] == (13, 4)
    assert lay[222][2] == 158 and lay[222][2] % 16 == 14
    assert lay[228][:2] == (15, 5) and lay[258] == (17, 6, 162, 6) and lay[294][:2] == (19, 7) and lay[300][:2] == (19, 7)
    assert lay[276][0] == 18 and (lay[276][2] + 15) // 16 == 12                     # main chain of 12
    assert {lay[n][1] for n in sc.BAND_DIMS if n >= 180} == {3, 4, 5, 6, 7}          # one, two and three helper runs of three
    assert 300 + 1 <= 16 * 19 < 306 + 1                                             # bc_fits
    assert sc.BAND_MAX_W == 6 * 9 + 5 and [(w - 5) // 6 for w in (5, 23, 59)] == [0, 3, 9]


@pytest.mark.parametrize("n,w", [(n, sc.band_width(n)) for n in sc.BAND_DIMS] + [(n, w) for w, n in sc.BAND_NARROW])
def test_known_band_family_is_exact(n, w):
    c = sc.known_band(n, w)
    L, A, x, b = c["L_int"], c["A_int"], c["x_int"], c["b_int"]
    assert np.array_equal(np.tril(L), L) and (np.diag(L) == sc.KNOWN_DIAG).all()
    assert sc.half_bandwidth(L) == w and sc.half_bandwidth(A) == w, "the half-bandwidth is exactly w"
    assert all(abs(L[i, i - w]) == 1 for i in range(w, n)), "the band's edge is set in every row"
    for col in sc.BAND_FULL_COLS + (n - 17, n - 16):
        if 0 <= col < n - 1:
            assert (np.abs(L[col + 1:col + w + 1, col]) == 1).all(), "column %d is full to the band's edge" % col
    assert np.array_equal(A, L @ L.T) and np.array_equal(b, A @ x)
    assert np.abs(A).max() < 2 ** 30
    assert np.array_equal(c["A"].astype(np.int64), A) and np.array_equal(c["b"].astype(np.int64), b)
    # measured with this generator: 1.25 (dim 6) .. 2.55 (dim 174); diagonal 24 against at most 59 + 15 unit entries per row and column
    assert 1.2 <= c["kappa"] <= 2.6, c["kappa"]


@pytest.mark.parametrize("n,w,k", [(n, sc.band_width(n), k) for n in sc.BAND_DIMS for k in ((2, 6, 10, 12) if n in sc.BAND_WIDE_DIMS else (2, 10))]
                         + [(n, w, k) for w, n in sc.BAND_NARROW for k in (2, 10)])
def test_ladder_band_condition_is_as_designed(n, w, k):
    c = sc.ladder_band(n, k, w)
    assert 0.5 * 10.0 ** k <= c["kappa"] <= 2.0 * 10.0 ** k
    assert sc.half_bandwidth(c["A"]) == w and np.array_equal(c["A"], c["A"].T)
    B = c["A"] - 10.0 ** -k * np.eye(n)
    assert np.linalg.matrix_rank(B, tol=1e-9) <= n - n // 3, "B = G G^T with every third column of G zero is singular"


@pytest.mark.parametrize("n", sc.BAND_WIDE_DIMS)
@pytest.mark.parametrize("sign", (+1, -1))
def test_graded_band_condition(n, sign):
    c = sc.graded_band(n, sign)
    assert 1e6 / 101 <= c["kappa"] <= 1e6 * 101 and sc.half_bandwidth(c["A"]) == sc.band_width(n)
    d = np.sqrt(np.diag(c["A"]) / np.diag(sc.ladder_band(n, 2)["A"]))
    assert np.allclose(d, np.where((np.arange(n) // 3) % 2 == 1, 10.0 ** (3 * sign), 1.0), rtol=1e-12)


@pytest.mark.parametrize("n,w,i", BAND_PD)
def test_band_reference_host_error_and_band_cholesky(n, w, i):
    c = _band_case(n, w, i)
    assert c["pd"] and np.array_equal(c["A"], c["A"].T) and sc.half_bandwidth(c["A"]) == c["w"]
    assert c["residual"] < 1e-17 and sc.residual_norm(c["A"], c["b"], c["x"]) < 1e-17
    assert c["e_host"] <= sc.bound(c) / 8, (c["family"], c["e_host"], sc.bound(c))
    _band_is_all_there_is(c)


def _notpd_band_params():
    return [(n, p, False, where) for n, p, where in sc.BAND_NOTPD_TOP] + [(n, q, True, where) for n, q, where in sc.BAND_NOTPD_BOTTOM]


@pytest.mark.parametrize("n,p,bottom,where", _notpd_band_params())
def test_band_not_positive_definite_where_meant(n, p, bottom, where):
    good, bad = sc.notpd_band(n, p, bottom)
    w = sc.band_width(n)
    assert good["pd"] and not bad["pd"]
    assert sc.half_bandwidth(good["A"]) == w and sc.half_bandwidth(bad["A"]) <= w
    for c in (good, bad):
        assert np.array_equal(c["A"].astype(np.int64), c["A_int"]) and np.array_equal(c["b_int"], c["A_int"] @ c["x_int"])
    assert good["e_host"] <= sc.bound(good) / 8
    _band_is_all_there_is(good)
    strips, sB, dimA, sM = sc.band_layout(n)
    if bottom:
        assert sc.first_failing_pivot(bad["A"][::-1, ::-1]) == p and sc.first_failing_pivot(good["A"][::-1, ::-1]) == -1
        assert p < 16 * sB, "in the helper's strips"
        if "last strip" in where:
            assert p // 16 == sB - 1
        if "first strip" in where:
            assert p // 16 == 0
    else:
        assert sc.first_failing_pivot(bad["A"]) == p
        assert p < dimA, "in the main chain's strips"
        if "hand-over strip" in where:
            assert p // 16 == sM
        if "before the hand-over" in where:
            assert sB and p // 16 < sM
        if "after the hand-over" in where:
            assert sB and p // 16 > sM
        if "last strip" in where:
            assert p // 16 == strips - 1 and sB == 0
        if "first wrap" in where:
            assert p // 16 == 6
        if "first strip" in where:
            assert p < 16


@pytest.mark.parametrize("n,p", sc.BAND_ZERO_PIVOT)
def test_band_zero_pivot(n, p):
    c = sc.zero_pivot_band(n, p)
    assert not c["pd"] and np.isfinite(c["A"]).all() and sc.half_bandwidth(c["A"]) <= sc.band_width(n)
    assert not c["A"][p].any() and not c["A"][:, p].any()
    assert sc.first_failing_pivot(c["A"]) == p
