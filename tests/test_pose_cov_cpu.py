"""The host form of the pose covariance call (lpslam_pose_covariance_batch_host, lpslam_pose_sigmas_host: csrc/pose_cov_math.h) against
tests/pose_cov_ref.py, the same operation in long double with plain sums.

  H and chi2        entry by entry |host - ref| <= ((n_used + C) T + 19 X) 2^-53.  T is the companion sum of absolute values as
                    tests/ba_ref.py forms it (|B|^T w |B|; w |e|^2 + 2 w |e| e_abs), X the first-order effect of one rounding of pc
                    relative to |R| |X| + |t| (pose_cov_ref's docstring); 19 are pc's roundings: a rotation entry 15 (a quaternion
                    component 6 -- four squares, three additions deep 4, sqrt, division --, two of them, product, sum, the difference
                    from 1), the product with X, three additions.
                    C counts the longest chain behind pc.  H, C_H = 28: 1 / z 1, its square 3, B[0][1] = -(1 + x x / z^2) fx 7 (x x 1,
                    the product 1 + 3 + 1, the addition, fx), the stereo row's B[2][1] 8, a term (w B) B 8 + 8 + 2 = 18, the three rows
                    20; the lane's running sum and the tree of eight levels add at most n_used + 8.  chi2, C_chi2 = 14: the projection
                    4 (1 / z, two products, cx) and e 5, the stereo e[2] 6, all relative to e_abs, so 6 on 2 w |e| e_abs; the
                    square, the two additions and the weight 4 on w |e|^2; n_used + 8 for the sum.  The reference's own error is
                    2^-11 of this.
  Sigma             the first-order bound of the inverse: |host - ref|_ij <= kappa_2(A) (||D bar(H) D||_2 / ||A||_2 + 6 x 2^-53) |Sigma|_ij,
                    A = D H D, with |Sigma|_ij = sqrt(Sigma_ii Sigma_jj) -- Sigma_ij itself on the diagonal, its Cauchy-Schwarz ceiling
                    off it, where an entry near 0 bounds nothing: d(A^-1)_ij = -(A^-1 e_i)^T dA (A^-1 e_j) and |A^-1 e_i|^2 = (A^-2)_ii
                    <= ||A^-1|| (A^-1)_ii
  status, n_used    equal
  census            every case meant to succeed has min_pivot >= 1e-6, every planted degenerate one |min_pivot| <= 1e-9
  the reference     H against central differences of its own residual under g2o's oplus (tests/ba_ref.py), and five planted defects that
                    each move a checked quantity by more than 100 bars
  pose_sigmas       position variances against the formula in long double, the orientation sigma against numpy.linalg.eigvalsh, quarter
                    turns about each axis
  refusals          every rule of the argument check"""
import ctypes as C

import numpy as np
import pytest

import ba_ref
import pose_cov_ref as ref

LD = np.longdouble
U = 2.0 ** -53
C_H, C_CHI2, C_PC = 28, 14, 19
SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 513, 2000)
GOOD = [(n, kind) for n in SIZES for kind in ("mono", "stereo", "mixed")] + [(40, "behind")]
DEGENERATE = ("same_point", "collinear", "two_stereo")


@pytest.fixture(scope="module")
def hip():
    from lpslam_amd import _build, hip
    _build.host_library()
    return hip


def _host(hip, c):
    return hip.pose_covariance_batch_host([0, len(c["obs"])], c["pose7"], c["obs"], c["active"], c["cam"])


@pytest.fixture(scope="module")
def results(hip):
    """(case, host result, long-double reference) of every case, computed once"""
    out = {}
    for n, kind in GOOD + [(0, k) for k in DEGENERATE] + [(0, "mixed"), (2, "mixed"), (30, "inactive")]:
        c = ref.case(7, n, kind)
        out[(n, kind)] = (c, _host(hip, c), ref.reference(c["pose7"], c["obs"], c["active"], c["cam"]))
    return out


def _h_bars(r):
    bar_h = ((r["n_used"] + C_H) * r["info21_abs"] + C_PC * r["info21_x"]).astype(np.float64) * U
    return bar_h, float((r["n_used"] + C_CHI2) * r["chi2_abs"] + C_PC * r["chi2_x"]) * U


def test_sums_lie_within_their_bars(results):
    worst = 0.0
    for key, (c, h, r) in results.items():
        bar_h, bar_c = _h_bars(r)
        dh = np.abs(h["info21"][0].astype(LD) - r["info21"]).astype(np.float64)
        dc = float(abs(LD(h["chi2"][0]) - r["chi2"]))
        print(key, "H: worst |host - ref| / bar %.3g, chi2: %.3g" % ((dh / np.maximum(bar_h, 1e-300)).max(), dc / max(bar_c, 1e-300)))
        assert (dh <= bar_h).all(), (key, dh, bar_h)
        assert dc <= bar_c, (key, dc, bar_c)
        worst = max(worst, (dh / np.maximum(bar_h, 1e-300)).max())
    assert worst > 0, "the host and the long-double reference cannot agree to the last bit everywhere"


def test_status_and_count_equal_the_reference(results):
    for key, (c, h, r) in results.items():
        assert h["status"][0] == r["status"] and h["n_used"][0] == r["n_used"], (key, h["status"], r["status"], h["n_used"], r["n_used"])
        if r["status"] != 0:
            assert not h["cov21"][0].any(), key
    assert results[(40, "behind")][1]["n_used"][0] == 37
    assert results[(30, "inactive")][1]["n_used"][0] == 0 and results[(30, "inactive")][1]["status"][0] == 1
    assert results[(2, "mixed")][1]["status"][0] == 1 and results[(0, "mixed")][1]["status"][0] == 1
    assert results[(0, "same_point")][1]["status"][0] == 2 and results[(0, "collinear")][1]["status"][0] == 2
    assert results[(0, "two_stereo")][1]["status"][0] == 1      # (two observations: too few comes first; its pivot is in the census)


def test_covariance_lies_within_the_first_order_bound(results):
    for key in GOOD:
        c, h, r = results[key]
        assert r["status"] == 0, key
        bar_h, _ = _h_bars(r)
        A, d = r["A"].astype(np.float64), r["d"].astype(np.float64)
        kappa = np.linalg.cond(A)
        rel = np.linalg.norm(ref.full(bar_h) * np.outer(d, d), 2) / np.linalg.norm(A, 2) + 6 * U
        sd = np.sqrt(np.diag(ref.full(r["cov21"]).astype(np.float64)))
        bound = kappa * rel * np.outer(sd, sd)
        diff = np.abs(ref.full(h["cov21"][0].astype(LD), LD) - ref.full(r["cov21"], LD)).astype(np.float64)
        print(key, "kappa %.3g, worst |host - ref| / bound %.3g" % (kappa, (diff / bound).max()))
        assert (diff <= bound).all(), (key, kappa, (diff / bound).max())
        # and it is an inverse: H Sigma = I to the same condition
        assert np.abs(ref.full(h["info21"][0]) @ ref.full(h["cov21"][0]) - np.eye(6)).max() <= 1e3 * kappa * U * 6


def test_census_no_case_sits_near_the_pivot_rule(results):
    for key in GOOD:
        c, h, r = results[key]
        print(key, "min_pivot %.3g" % h["min_pivot"][0])
        assert h["min_pivot"][0] >= 1e-6 and h["min_pivot"][0] <= 1.0 + 8 * U, (key, h["min_pivot"][0])
        assert abs(h["min_pivot"][0] - float(r["min_pivot"])) <= 1e-6 * h["min_pivot"][0] + 1e-12, key
    for kind in DEGENERATE:
        c, h, r = results[(0, kind)]
        print(kind, "min_pivot %.3g (reference %.3g)" % (h["min_pivot"][0], float(r["min_pivot"])))
        assert abs(h["min_pivot"][0]) <= 1e-9 and abs(float(r["min_pivot"])) <= 1e-9, (kind, h["min_pivot"][0], float(r["min_pivot"]))


# ---- the reference against something that is not the header --------------------------------------------------------------------
def _residual(pose7, obs, cam):
    return ref.terms(pose7, obs, cam, LD)["e"]


def test_reference_information_equals_central_differences():
    c = ref.case(11, 64, "mixed")
    r = ref.reference(c["pose7"], c["obs"], c["active"], c["cam"])
    pose = c["pose7"].astype(LD); pose[:4] /= np.sqrt((pose[:4] * pose[:4]).sum())
    h = LD(1e-7)
    J = np.zeros((len(c["obs"]), 3, 6), LD)
    for k in range(6):
        d = np.zeros(6, LD); d[k] = h
        J[:, :, k] = (_residual(ba_ref.oplus(pose, d), c["obs"], c["cam"]) - _residual(ba_ref.oplus(pose, -d), c["obs"], c["cam"])) / (2 * h)
    H = np.einsum("n,nra,nrc->ac", c["obs"][:, 3].astype(LD), J, J)
    scale = np.sqrt(np.outer(np.diag(r["H"]), np.diag(r["H"])))
    assert (np.abs(H - r["H"]) <= 1e-7 * scale).all(), np.abs((H - r["H"]) / scale).max()


def test_reference_derivatives_equal_central_differences():
    """dB / dpc and de / dpc, which the companions X are made of: pc = R X + t, so a step of t is a step of pc"""
    c = ref.case(11, 64, "mixed")
    tm = ref.terms(c["pose7"], c["obs"], c["cam"], LD)
    h = LD(1e-6)
    for j in range(3):
        dp = np.zeros(7, LD); dp[4 + j] = h
        plus, minus = ref.terms(c["pose7"].astype(LD) + dp, c["obs"], c["cam"], LD), ref.terms(c["pose7"].astype(LD) - dp, c["obs"], c["cam"], LD)
        numB = (plus["B"] - minus["B"]) / (2 * h); nume = (plus["e"] - minus["e"]) / (2 * h)
        assert (np.abs(numB - tm["dB"][..., j]) <= 1e-7 * np.abs(tm["dB"]).max(axis=(1, 2, 3))[:, None, None]).all(), j
        assert (np.abs(nume - tm["de"][..., j]) <= 1e-7 * np.abs(tm["de"]).max(axis=(1, 2))[:, None]).all(), j
    assert tm["mono"].any() and not tm["dB"][tm["mono"], 2].any() and not tm["de"][tm["mono"], 2].any()


def _planted():
    """(name, case, mutation): the observation each defect touches is chosen so that the defect has something to change"""
    out = []
    c = ref.case(13, 64, "mixed")
    mono = c["obs"][:, 2] < 0
    out.append(("drop_row3", c, {"drop_row3": int(np.flatnonzero(~mono)[0])}))
    out.append(("mono_row3", c, {"mono_row3": int(np.flatnonzero(mono)[0])}))
    ci = dict(c, active=c["active"].copy()); ci["active"][5] = 0
    out.append(("count_inactive", ci, {"count_inactive": 5}))
    ch = dict(c, obs=c["obs"].copy()); ch["obs"][7, 0] += 9.0        # a residual of nine pixels: chi2 far above 7.815 at every weight of the generator
    out.append(("huber", ch, {"huber": 7}))
    cb = ref.case(13, 40, "behind")
    out.append(("count_behind", cb, {"count_behind": 1}))
    return out


@pytest.mark.parametrize("name,c,mutation", _planted(), ids=[p[0] for p in _planted()])
def test_a_planted_defect_moves_a_checked_quantity_by_100_bars(hip, name, c, mutation):
    r = ref.reference(c["pose7"], c["obs"], c["active"], c["cam"])
    bad = ref.reference(c["pose7"], c["obs"], c["active"], c["cam"], mutate=mutation)
    bar_h, bar_c = _h_bars(r)
    moved = max(float((np.abs(bad["info21"] - r["info21"]).astype(np.float64) / np.maximum(bar_h, 1e-300)).max()), float(abs(bad["chi2"] - r["chi2"])) / bar_c)      # (H[3][4] is 0 by structure, and so is its bar)
    print(name, "moves a sum by %.3g bars" % moved)
    assert moved > 100, (name, moved)
    # the host form does not have the defect
    h = _host(hip, c)
    assert (np.abs(h["info21"][0].astype(LD) - r["info21"]).astype(np.float64) <= bar_h).all() and h["n_used"][0] == r["n_used"]


# ---- covariance -> sigmas ---------------------------------------------------------------------------------------------------------
def test_pose_sigmas_follow_the_formula(hip, results):
    for key in ((64, "mixed"), (3, "mono"), (2000, "stereo")):
        c, h, r = results[key]
        s = hip.pose_sigmas_host(c["pose7"], h["cov21"][0])
        var, vabs, Sww = ref.sigmas(c["pose7"], h["cov21"][0])
        assert (s > 0).all() and np.isfinite(s).all()
        err = np.abs(s[:3].astype(LD) ** 2 - var).astype(np.float64)
        # (squaring the returned sigma adds the sqrt's and the square's roundings: 3 x 2^-53 of the variance itself)
        print(key, "variance error / (2^-53 sum of |terms|): %s" % (err / (U * vabs.astype(np.float64))))
        assert (err <= 16 * U * vabs.astype(np.float64) + 3 * U * var.astype(np.float64)).all(), (key, err / (U * vabs.astype(np.float64)))
        w = np.linalg.eigvalsh(Sww.astype(np.float64))
        assert np.isclose(s[3] ** 2, w.max(), rtol=1e-12, atol=1e-12 * w.max()), (key, s[3] ** 2, w.max())


def test_a_quarter_turn_permutes_the_position_sigmas(hip, results):
    """Sigma_C = R^T Sigma_uu R: at a pose that is a quarter turn about one camera axis a diagonal Sigma_uu = diag(a, b, c) keeps that axis'
    variance and swaps the other two; in lpslam order (x_sigma from Sigma_C[1][1], y_sigma from Sigma_C[0][0]) that is stated case by case"""
    diag = np.zeros((6, 6)); diag[np.arange(6), np.arange(6)] = [1e-4, 4e-4, 9e-4, 0.01, 0.04, 0.09]
    cov = [diag[a, b] for a, b in ref.TRI]
    assert np.allclose(hip.pose_sigmas_host([1, 0, 0, 0, 0.3, -0.2, 0.1], cov), [0.2, 0.1, 0.3, 0.03], rtol=1e-14)
    r = np.sqrt(0.5)
    want = {0: [0.3, 0.1, 0.2], 1: [0.2, 0.3, 0.1], 2: [0.1, 0.2, 0.3]}      # Sigma_C diagonal: (a, c, b), (c, b, a), (b, a, c)
    for axis in range(3):
        q = [r, 0, 0, 0]; q[1 + axis] = r
        s = hip.pose_sigmas_host(q + [0.3, -0.2, 0.1], cov)
        assert np.allclose(s[:3], want[axis], rtol=1e-12), (axis, s)
        assert s[3] == hip.pose_sigmas_host([1, 0, 0, 0, 0, 0, 0], cov)[3], "the orientation sigma does not depend on the pose"
        # a full covariance at the turned pose: the formula in long double
        c, h, _ = results[(64, "mixed")]
        var, vabs, _ = ref.sigmas(np.array(q + [0.3, -0.2, 0.1]), h["cov21"][0])
        s = hip.pose_sigmas_host(q + [0.3, -0.2, 0.1], h["cov21"][0])
        assert (np.abs(s[:3].astype(LD) ** 2 - var).astype(np.float64) <= 16 * U * vabs.astype(np.float64) + 3 * U * var.astype(np.float64)).all(), axis


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _raw(hip, n_sets, start, args):
    f = hip.host_lib().lpslam_pose_covariance_batch_host
    f.argtypes = [C.c_int32] + [C.c_void_p] * 11; f.restype = C.c_int
    return f(n_sets, start.ctypes.data_as(C.c_void_p) if start is not None else None, *[a.ctypes.data_as(C.c_void_p) if a is not None else None for a in args])


def test_refusals(hip):
    c = ref.case(3, 20, "mixed")
    start = np.array([0, 20], np.int32)
    good = [np.ascontiguousarray(c["pose7"]), np.ascontiguousarray(c["obs"]), c["active"], c["cam"], np.full(21, 7.0), np.full(21, 7.0), np.full(1, 7.0), np.full(1, 7.0),
            np.full(1, 7, np.int32), np.full(1, 7, np.int32)]
    INVALID, CAPACITY = 1, 3
    assert _raw(hip, 1, start, good) == 0 and good[9][0] == 0
    for a in good[4:]:
        a[...] = 7
    assert _raw(hip, 1, None, good) == INVALID
    for k in range(len(good)):
        assert _raw(hip, 1, start, [None if i == k else a for i, a in enumerate(good)]) == INVALID, k
    assert _raw(hip, 0, start, good) == INVALID and _raw(hip, -1, start, good) == INVALID
    assert _raw(hip, 1, np.array([5, 3], np.int32), good) == INVALID and _raw(hip, 1, np.array([-1, 3], np.int32), good) == INVALID
    assert _raw(hip, 2, np.array([0, 12, 8], np.int32), good) == INVALID
    assert _raw(hip, 4097, np.zeros(4098, np.int32), good) == CAPACITY
    assert _raw(hip, 1, np.array([0, (1 << 18) + 1], np.int32), good) == CAPACITY
    assert all((a == 7).all() for a in good[4:]), "a refused call wrote an output"
    # an empty set needs neither observations nor flags
    assert _raw(hip, 1, np.array([0, 0], np.int32), [good[0], None, None] + good[3:]) == 0 and good[9][0] == 1 and good[8][0] == 0
