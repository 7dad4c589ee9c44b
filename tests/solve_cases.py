"""Linear systems A x = b for the dense window solve (k_chol_pair + k_chol_xsolve, k_chol_wg) and their references.  numpy only.

A stands for S + lambda I of a window: full symmetric, dim = 6 x free keyframes.  Every case carries
    A, b        float64, what the device is given
    x           the solution of exactly that (A, b): known by construction (integer family) or refined in np.longdouble
    kappa       kappa_2(A) from the eigenvalues of the float64 matrix
    e_host      forward error (infinity norm, relative) of a plain float64 Cholesky with two substitutions on the same input
    pd          numpy's Cholesky succeeds
The bound every solver must meet is the first-order one of a Cholesky solve, bound(case) = n kappa_2 2^-53.

Families
    known       A = L L^T with an integer L: diagonal 24, two +-1 entries per row at random places, columns 0, 15, 16, 31, 32, 33, 63,
                64 and dim - 1 dense with +-1.  x is an integer vector and b = A x is computed in int64: exact, no extended precision.
                The dense columns make A dense, so every tile of the trailing update carries weight.
    ladder      A = Q diag(10^(-k t)) Q^T, t = linspace(0, 1), k = 2, 6, 10, 12.
    graded      D A D with A = ladder k = 2 and D = 1, 1, 1, 10^+-3, 10^+-3, 10^+-3, 1, ...: the rotation and translation columns
                of a window differ like that.
    real        S + lambda I and rhs of a window, read from the device by the caller (case_from)
    notpd       A <- A - 2 lambda_k v_k v_k^T on a ladder k = 2 matrix whose eigenvector v_k (eigenvalue lambda_k = 1 = ||A||_2) is
                sqrt(0.9) e_p + sqrt(0.1) u with u supported behind p: the leading p x p block keeps its Cholesky factor and pivot p is
                the first one that fails, where a table says (NOTPD).  Each comes with the unflipped (positive definite) matrix.
    zero pivot  row and column p of a ladder matrix are zero: pivot p is exactly 0 in any arithmetic.
"""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended np.longdouble (x87: 64-bit significand)"

# free keyframes of every boundary the two kernels have (dim = 6 free); panels are 32 columns, strips 16, a launch factors two panels
FREE = (1, 3, 5, 6, 8, 9, 11, 16, 17, 19, 22, 50, 51, 100, 199)
DIMS = tuple(6 * f for f in FREE)
WG_MAX_DIM = 300                     # the largest system k_chol_wg takes (cw_fits: dim + 1 <= 304)
WIDE_DIMS = (18, 54, 96, 132, 300, 306, 600)      # ladder k = 6, 12, graded and real systems
DENSE_COLS = (0, 15, 16, 31, 32, 33, 63, 64)


def bound(case):
    return case["n"] * case["kappa"] * U


def _rng(*key):
    return np.random.Generator(np.random.PCG64([20240611] + [int(k) for k in key]))


def kappa2(A):
    w = np.linalg.eigvalsh(A)
    return float(np.abs(w).max() / np.abs(w).min())


def is_pd(A):
    try:
        np.linalg.cholesky(A)
        return True
    except np.linalg.LinAlgError:
        return False


def first_failing_pivot(A):
    """index of the first pivot <= 0 of an unblocked float64 Cholesky, or -1"""
    A = np.array(A, np.float64)
    n = len(A)
    for j in range(n):
        d = A[j, j]
        if not d > 0.0:
            return j
        A[j:, j] /= np.sqrt(d)
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return -1


def _substitute(L, b, dtype):
    """x with L L^T x = b: forward and backward substitution, row by row, in `dtype`"""
    n = len(b)
    L = L.astype(dtype); y = np.zeros(n, dtype); b = b.astype(dtype)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype)
    Lt = np.ascontiguousarray(L.T)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - Lt[i, i + 1:] @ x[i + 1:]) / L[i, i]
    return x


def host_solve(A, b):
    """plain float64: Cholesky, two substitutions"""
    return _substitute(np.linalg.cholesky(A), b, np.float64)


def residual_norm(A, b, x):
    """normwise relative residual ||b - A x|| / (||A|| ||x|| + ||b||), infinity norms, in np.longdouble"""
    Al, xl, bl = A.astype(LD), np.asarray(x, LD), b.astype(LD)
    r = bl - Al @ xl
    return float(np.abs(r).max() / (np.abs(Al).sum(1).max() * np.abs(xl).max() + np.abs(bl).max()))


def refine(A, b, max_steps=60):
    """The solution of the float64 system (A, b) by iterative refinement: residuals and the iterate in np.longdouble, corrections
    from the float64 Cholesky factor, until the residual stops falling.  Returns (x in longdouble, final normwise residual)."""
    L = np.linalg.cholesky(A)
    Al, bl = A.astype(LD), b.astype(LD)
    scale_a = np.abs(Al).sum(1).max()
    x = _substitute(L, b, np.float64).astype(LD)
    best, best_x = np.inf, x
    for _ in range(max_steps):
        r = bl - Al @ x
        rn = float(np.abs(r).max() / (scale_a * np.abs(x).max() + np.abs(bl).max()))
        if not rn < 0.5 * best:                         # no longer falling (by a factor of two at least): keep the best iterate
            if rn < best:
                best, best_x = rn, x
            break
        best, best_x = rn, x
        # the correction in float64 on a scaled residual (its entries may be far below the float64 range of b)
        s = float(np.abs(r).max())
        if s == 0.0:
            break
        d = _substitute(L, (r / s).astype(np.float64), np.float64)
        x = x + d.astype(LD) * LD(s)
    return best_x, best


def forward_error(x, x_ref):
    x_ref = np.asarray(x_ref, LD)
    return float(np.abs(np.asarray(x, LD) - x_ref).max() / np.abs(x_ref).max())


def case_from(A, b, family, x=None, tag=""):
    """A case of caller-given arrays (real systems); x is refined when it is not known"""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    assert np.array_equal(A, A.T) and np.isfinite(A).all() and np.isfinite(b).all()
    n = len(b)
    c = dict(n=n, family=family, tag=tag, A=A, b=b, kappa=kappa2(A), pd=is_pd(A), residual=0.0)
    if c["pd"]:
        if x is None:
            x, c["residual"] = refine(A, b)
        c["x"] = x
        c["e_host"] = forward_error(host_solve(A, b), x)
    return c


# ---- known solution ---------------------------------------------------------------------------------------------------------
KNOWN_DIAG = 24


def known_factor(n):
    """the integer L"""
    rng = _rng(1, n)
    L = np.zeros((n, n), np.int64)
    for i in range(1, n):
        for j in rng.integers(0, i, 2):
            L[i, j] = rng.choice((-1, 1))
    for c in DENSE_COLS + (n - 1,):
        if c < n:
            L[c + 1:, c] = rng.choice((-1, 1), n - c - 1)
    L[np.arange(n), np.arange(n)] = KNOWN_DIAG
    return L


@functools.lru_cache(maxsize=None)
def known(n):
    L = known_factor(n)
    Ai = L @ L.T
    xi = _rng(2, n).integers(-9, 10, n)
    xi[xi == 0] = 7
    bi = Ai @ xi
    assert np.abs(Ai).max() < 2 ** 30 and np.abs(bi).max() < 2 ** 53      # exact in int64 and in float64
    c = case_from(Ai.astype(np.float64), bi.astype(np.float64), "known", x=xi.astype(LD))
    c["L_int"], c["A_int"], c["x_int"], c["b_int"] = L, Ai, xi, bi
    assert c["kappa"] < 1e4, (n, c["kappa"])
    return c


# ---- conditioning ladder, graded scalings ------------------------------------------------------------------------------------
def _orthogonal(n, *key):
    Q, R = np.linalg.qr(_rng(*key).normal(size=(n, n)))
    return Q * np.sign(np.diag(R))


def _spectral(Q, w):
    A = (Q * w) @ Q.T
    return 0.5 * (A + A.T)


def _with_rhs(A, family, tag, *key):
    x0 = _rng(*key).uniform(0.5, 1.5, len(A)) * _rng(9, *key).choice((-1.0, 1.0), len(A))
    return case_from(A, A @ x0, family, tag=tag)


@functools.lru_cache(maxsize=None)
def ladder(n, k):
    A = _spectral(_orthogonal(n, 3, n), 10.0 ** (-k * np.linspace(0.0, 1.0, n)) if n > 1 else np.ones(1))
    return _with_rhs(A, "ladder%d" % k, "", 4, n, k)


@functools.lru_cache(maxsize=None)
def graded(n, sign):
    A = ladder(n, 2)["A"]
    d = np.where((np.arange(n) // 3) % 2 == 1, 10.0 ** (3 * sign), 1.0)
    return _with_rhs(A * np.outer(d, d), "graded%+d" % (3 * sign), "", 5, n, sign + 1)     # A_ij (d_i d_j): symmetric to the bit


# ---- not positive definite ----------------------------------------------------------------------------------------------------
# (dim, first failing pivot p, where that is)
NOTPD = ((54, 5, "strip A of the first panel"),
         (54, 20, "strip B of the first panel"),
         (102, 40, "second column of a pair"),
         (102, 90, "second pair, strip B of its first column"),
         (132, 129, "`single` last launch"),
         (54, 50, "trimmed last column, strip B"),
         (18, 16, "trimmed last column of a one-panel system"),
         (300, 290, "last panel of the largest cw_fits system"),
         (306, 200, "panel-pair chain only"))
ZERO_PIVOT = ((54, 20), (132, 64))


@functools.lru_cache(maxsize=None)
def notpd(n, p):
    """(positive definite case, flipped case): they differ by 2 lambda_k v_k v_k^T"""
    assert 0 <= p < n - 1
    rng = _rng(6, n, p)
    v = np.zeros(n)
    u = rng.normal(size=n - p - 1)
    v[p] = np.sqrt(0.9); v[p + 1:] = np.sqrt(0.1) * u / np.linalg.norm(u)
    # an orthonormal basis whose first vector is v: eigenvalue 1 = ||A|| goes to v, the rest of the k = 2 ladder to the others
    M = rng.normal(size=(n, n)); M[:, 0] = v
    Q, R = np.linalg.qr(M)
    Q = Q * np.sign(np.diag(R))
    w = 10.0 ** (-2 * np.linspace(0.0, 1.0, n))
    good = _with_rhs(_spectral(Q, w), "notpd-base", "p=%d" % p, 7, n, p)
    wf = w.copy(); wf[0] = -w[0]
    bad = case_from(_spectral(Q, wf), good["b"], "notpd", tag="p=%d" % p)
    bad["p"] = p
    return good, bad


@functools.lru_cache(maxsize=None)
def zero_pivot(n, p):
    A = ladder(n, 2)["A"].copy()
    A[p, :] = 0.0; A[:, p] = 0.0
    c = case_from(A, ladder(n, 2)["b"], "zero-pivot", tag="p=%d" % p)
    c["p"] = p
    return c


def synthetic_cases(n):
    """the positive definite synthetic cases the device runs at dimension n (real systems come from the device)"""
    out = [known(n), ladder(n, 2), ladder(n, 10)] if n < 1000 else [known(n)]        # 1194: one case only (the reference's cost)
    if n in WIDE_DIMS:
        out += [ladder(n, 6), ladder(n, 12), graded(n, +1), graded(n, -1)]
    return out


# ---- band systems (k_chol_band) ------------------------------------------------------------------------------------------------
# A is symmetric with scalar half-bandwidth w = 6 hbw + 5 (hbw: the block half-bandwidth of the window) at most; the kernel takes it in
# strips of 16 columns through a ring of 96 rows, from 12 strips on from both ends (a helper workgroup eliminates the last sB strips
# bottom-up and hands a 64 x 64 block over in front of strip sM of the main chain), and substitutes backwards in runs of three strips.
#   known-band    A = L L^T, integer lower-banded L: diagonal 24, the band's edge (i, i - w) +-1 in every row, two more +-1 per row inside
#                 the band, BAND_FULL_COLS full to the band's edge.  Integer x, b = A x in int64: exact.
#   ladder-band k A = B + 10^-k I, B = G G^T / ||G G^T||_2 with a lower-banded normal G whose every third column is zero (B is singular,
#                 kappa_2(A) = 1 + 10^k); graded: D A D on k = 2.
#   notpd-band    A = L D L^T with the integer L, D = I except D_pp = -1: the first failing pivot of a top-down elimination is exactly p.
#                 Flipped (A[::-1, ::-1]) it fails at q counted from the bottom: the helper's strips.  Partner: D = I.
#   zero pivot    row and column p of a ladder-band k = 2 matrix are zero.
BAND_FREE = (1, 2, 3, 5, 8, 9, 11, 14, 16, 17, 19, 22, 27, 29, 30, 32, 33, 37, 38, 43, 46, 49, 50)
BAND_DIMS = tuple(6 * f for f in BAND_FREE)
BAND_MAX_W = 59                      # 6 BD_MAXHBW + 5
BAND_TWIST_MIN = 12                  # strips from which on the factorisation runs from both ends
BAND_WIDE_DIMS = (18, 54, 96, 132, 174, 180, 300)      # ladder-band k = 6, 12 and graded
BAND_NARROW = tuple((w, n) for w in (5, 23) for n in (54, 102, 180, 300))       # block half-bandwidth 0 and 3
BAND_FULL_COLS = (0, 15, 16, 31, 32, 63, 64, 79, 80, 95, 96)                    # and dim - 17, dim - 16
# (dim, first failing pivot p of the top-down elimination, where that is)
BAND_NOTPD_TOP = ((54, 5, "first strip"), (54, 20, "second strip"), (54, 50, "last strip, padding beside it"),
                  (102, 97, "behind the ring's first wrap"), (174, 170, "last strip of the largest untwisted system"),
                  (180, 40, "main chain, before the hand-over"), (180, 70, "the hand-over strip"), (180, 125, "main chain, after the hand-over"),
                  (300, 100, "main chain"))
# (dim, q: first failing pivot of the bottom-up elimination, counted from the end)
BAND_NOTPD_BOTTOM = ((180, 3, "helper's first strip"), (180, 47, "helper's last strip"), (300, 60, "helper"), (300, 111, "helper's last strip"))
BAND_ZERO_PIVOT = ((54, 20), (180, 70), (300, 290))


def band_width(n):
    return min(BAND_MAX_W, n - 1)


def band_layout(n):
    """(strips, sB, dimA, sM) as k_chol_band computes them"""
    strips = (n + 15) // 16
    sB = (strips - 5) // 2 if strips >= BAND_TWIST_MIN else 0
    dimA = n - 16 * sB
    return strips, sB, dimA, ((dimA - 64) // 16 if sB else -1)


def half_bandwidth(A):
    """the largest |i - j| with A_ij != 0"""
    i, j = np.nonzero(A)
    return int(np.abs(i - j).max()) if len(i) else 0


def band_mask(n, w):
    i = np.arange(n)
    return np.abs(i[:, None] - i[None, :]) <= w


def band_cholesky_solve(A, b, w=None):
    """float64 right-looking Cholesky and two column-oriented substitutions that touch nothing beyond row j + w of column j (w=None: no
    limit, the same operations on the whole matrix).  Every operation is elementwise -- no sum whose grouping could depend on a length --
    so the two forms agree to the byte exactly when nothing outside the band matters.  Returns (L, x)."""
    n = len(b)
    w = n if w is None else w
    L = np.tril(np.array(A, np.float64)); y = np.array(b, np.float64)
    for j in range(n):
        hi = min(n, j + w + 1)
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:hi, j] /= L[j, j]
        L[j + 1:hi, j + 1:hi] -= np.tril(np.outer(L[j + 1:hi, j], L[j + 1:hi, j]))
        y[j] /= L[j, j]
        y[j + 1:hi] -= L[j + 1:hi, j] * y[j]
    x = y
    for j in range(n - 1, -1, -1):
        lo = max(0, j - w)
        x[j] /= L[j, j]
        x[lo:j] -= L[j, lo:j] * x[j]
    return L, x


def known_band_factor(n, w):
    rng = _rng(11, n, w)
    L = np.zeros((n, n), np.int64)
    for i in range(1, n):
        lo = max(0, i - w)
        for j in rng.integers(lo, i, 2):
            L[i, j] = rng.choice((-1, 1))
        if i - w >= 0:
            L[i, i - w] = rng.choice((-1, 1))
    for c in BAND_FULL_COLS + (n - 17, n - 16):
        if 0 <= c < n - 1:
            hi = min(n, c + w + 1)
            L[c + 1:hi, c] = rng.choice((-1, 1), hi - c - 1)
    L[np.arange(n), np.arange(n)] = KNOWN_DIAG
    return L


def _int_case(Ai, xi, family, tag=""):
    bi = Ai @ xi
    assert np.abs(Ai).max() < 2 ** 30 and np.abs(bi).max() < 2 ** 53      # exact in int64 and in float64
    c = case_from(Ai.astype(np.float64), bi.astype(np.float64), family, x=xi.astype(LD), tag=tag)
    c["A_int"], c["x_int"], c["b_int"] = Ai, xi, bi
    return c


def _int_x(n, *key):
    xi = _rng(*key).integers(-9, 10, n)
    xi[xi == 0] = 7
    return xi


@functools.lru_cache(maxsize=None)
def known_band(n, w=None):
    w = band_width(n) if w is None else w
    L = known_band_factor(n, w)
    c = _int_case(L @ L.T, _int_x(n, 12, n, w), "known-band")
    c["L_int"], c["w"] = L, w
    return c


def _banded_normal(n, w, *key):
    G = np.tril(_rng(*key).normal(size=(n, n))) * band_mask(n, w)
    G[:, 2::3] = 0.0
    return G


@functools.lru_cache(maxsize=None)
def ladder_band(n, k, w=None):
    w = band_width(n) if w is None else w
    G = _banded_normal(n, w, 13, n, w)
    B = G @ G.T
    B = 0.5 * (B + B.T)
    A = B / np.linalg.norm(B, 2)
    A[np.arange(n), np.arange(n)] += 10.0 ** -k
    c = _with_rhs(A, "ladder-band%d" % k, "", 14, n, k, w)
    c["w"] = w
    return c


@functools.lru_cache(maxsize=None)
def graded_band(n, sign):
    A = ladder_band(n, 2)["A"]
    d = np.where((np.arange(n) // 3) % 2 == 1, 10.0 ** (3 * sign), 1.0)
    c = _with_rhs(A * np.outer(d, d), "graded-band%+d" % (3 * sign), "", 15, n, sign + 1)
    c["w"] = band_width(n)
    return c


@functools.lru_cache(maxsize=None)
def notpd_band(n, p, bottom=False):
    """(positive definite partner, case that fails at pivot p): top-down, or with bottom=True both flipped, so that the bottom-up
    elimination fails at p counted from the end"""
    w = band_width(n)
    L = known_band_factor(n, w)
    D = np.ones(n, np.int64); D[p] = -1
    good_i, bad_i = L @ L.T, (L * D) @ L.T
    if bottom:
        good_i, bad_i = good_i[::-1, ::-1].copy(), bad_i[::-1, ::-1].copy()
    tag = ("q=%d" if bottom else "p=%d") % p
    xi = _int_x(n, 16, n, p)
    good = _int_case(good_i, xi, "notpd-band-base", tag)
    bad = _int_case(bad_i, xi, "notpd-band", tag)
    for c in (good, bad):
        c["w"], c["p"], c["bottom"] = w, p, bottom
    return good, bad


@functools.lru_cache(maxsize=None)
def zero_pivot_band(n, p):
    base = ladder_band(n, 2)
    A = base["A"].copy()
    A[p, :] = 0.0; A[:, p] = 0.0
    c = case_from(A, base["b"], "zero-pivot-band", tag="p=%d" % p)
    c["p"], c["w"] = p, band_width(n)
    return c


def band_cases(n):
    """the positive definite synthetic band cases at dimension n and the full width min(59, n - 1)"""
    out = [known_band(n), ladder_band(n, 2), ladder_band(n, 10)]
    if n in BAND_WIDE_DIMS:
        out += [ladder_band(n, 6), ladder_band(n, 12), graded_band(n, +1), graded_band(n, -1)]
    return out


def narrow_band_cases(n, w):
    return [known_band(n, w), ladder_band(n, 2, w), ladder_band(n, 10, w)]
