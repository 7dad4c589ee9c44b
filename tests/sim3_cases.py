"""Generators, tolerances and the high-precision reference shared by the Sim3 tests (test_sim3_gpu.py, test_sim3_limits_gpu.py,
test_sim3_ref_cpu.py, the Sim3 family of fuzz_cases.py) and by tools/make_golden_sim3.py.

Measured figures the tests lean on (tests/test_sim3_ref_cpu.py re-measures the first table on every run):

Oracle against mpmath (50 digits), |log M|^2 of the 45 probes of tests/golden/g10_sim3_probes.npz: largest relative deviation
per theta class, over the five sigma values.  Two places lose digits, in the formulas and not in their restatement: in the
small-angle branch with |sigma| >= 1e-5 the coefficients A = ((sigma - 1) s + 1) / sigma^2 and B = (...) / sigma^3 cancel (at
sigma = 2e-5 B keeps one digit; it is the only probe of the classes 3e-3 and 4.4e-3 above 5e-16), and towards theta = pi
sqrt(1 - d^2) does.  Everywhere else the oracle is within a few ulp.

    theta     oracle vs mpmath    GPU bound = max(8 x, 64 ulp)
    0         1.9e-16             1.4e-14
    1e-7      3.7e-16             1.4e-14
    3e-3      1.5e-09             1.2e-08
    4.4e-3    4.4e-09             3.5e-08
    4.5e-3    4.4e-16             1.4e-14
    0.5       4.8e-16             1.4e-14
    2.0       3.6e-16             1.4e-14
    3.0       1.3e-14             1.0e-13
    3.14      6.1e-11             4.9e-10

(ORACLE_VS_MP below holds the same figures.)

Pair optimiser, cases of PAIR_CASES at chi_sq = 10: smallest |w e^2 / chi_sq - 1| over both edges of every pair at the oracle's
final S12 (how far the nearest pair sits from the inlier threshold).  An identical inlier mask is a fair demand only above 1e-4
(test_pair_cases_are_what_they_claim asserts it); no seed had to change for it.

    n / outlier_frac    scale 1, fixed    scale 1.15, free
    9 / 0               6.8e-01           6.8e-01
    10 / 0              5.4e-01           4.2e-01
    10 / 0.3            3.2e-01           4.7e-01
    12 / 0.2            6.4e-01           5.1e-01
    64 / 0.1            3.1e-01           8.1e-02
    255 / 0.1           3.9e-02           2.3e-02
    256 / 0.1           1.8e-01           1.2e-01
    257 / 0.1           8.6e-02           4.9e-04      <- the minimum
    513 / 0.1           7.4e-02           1.0e-02
    1025 / 0.3          9.7e-03           3.2e-02

Pose graphs: what the seeds of GRAPH_SEEDS / PANEL_SEEDS were chosen for is written next to them."""
import math

import numpy as np

from lpslam_amd import synth

ROT_TOL, TRANS_TOL, CHI_RTOL = 1e-4, 1e-3, 5e-4

NB = 32                                     # panel width of the dense solve (lpslam_amd/csrc/ba_common.h)


def rot_err(q1, q2):
    return 2 * np.arccos(np.clip(np.abs(np.sum(q1 * q2, axis=1)), 0, 1))


def _check(vg, vo, lg, lo, n_cmp):
    n_cmp = min(n_cmp, len(lo), len(lg))
    assert np.allclose(lg["chi2_before"][:n_cmp], lo["chi2_before"][:n_cmp], rtol=CHI_RTOL)
    assert np.allclose(lg["chi2_after"][:n_cmp], lo["chi2_after"][:n_cmp], rtol=CHI_RTOL)
    assert np.array_equal(lg["trials"][:n_cmp], lo["trials"][:n_cmp])
    assert np.allclose(lg["lambda"][:n_cmp], lo["lambda"][:n_cmp], rtol=CHI_RTOL)      # lambda follows rho, a ratio of chi2 differences
    assert rot_err(vg[:, :4], vo[:, :4]).max() < ROT_TOL
    assert np.abs(vg[:, 4:7] - vo[:, 4:7]).max() < TRANS_TOL and np.abs(vg[:, 7] - vo[:, 7]).max() < 1e-4


def panel_shape(n_free):
    """(nb, need) of the dense solve for 7 n_free unknowns: panels of NB columns over dim + 1 rows (the rhs rides as row `dim`),
    `need` = the columns of H that fall into the last panel."""
    dim = 7 * n_free
    nb = (dim + 1 + NB - 1) // NB
    return nb, dim - NB * (nb - 1)


# ---- Sim3 as 8 doubles (qw qx qy qz tx ty tz s) in numpy: x -> s R x + t ----------------------------------------------------
def q_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def q_rot(q, v):
    u = 2 * np.cross(q[1:], v)
    return v + q[0] * u + np.cross(q[1:], u)


def s3_mul(a, b):
    return np.concatenate([q_mul(a[:4], b[:4]), a[7] * q_rot(a[:4], b[4:7]) + a[4:7], [a[7] * b[7]]])


def s3_inv(a):
    qi = a[:4] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([qi, q_rot(qi, -a[4:7] / a[7]), [1.0 / a[7]]])


def s3_exp(u):
    """exp of (omega, upsilon, sigma) through the 4 x 4 matrix exponential: no branch table, independent of the code under test."""
    from scipy.linalg import expm
    u = np.asarray(u, np.float64)
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    th = np.linalg.norm(u[:3])
    q = np.concatenate([[math.cos(th / 2)], (math.sin(th / 2) / th if th > 0 else 0.5) * u[:3]])
    return np.concatenate([q, expm(G)[:3, 3], [math.exp(u[6])]])


# ---- pose graphs ------------------------------------------------------------------------------------------------------------
def irregular_graph(n, seed, n_fixed=1, fix_scale=True, drift_scale=0.0):
    """A pose graph of every shape synth.pose_graph_problem never takes.  Ground truth and drifting estimates are that generator's
    (chain only); the edges are the spanning chain, 2 n random pairs in either orientation, a hub (vertex n // 2) joined to every
    other vertex, five exact duplicates and five reversed copies of earlier edges (measurement retaken for that direction).
    Measurements are S_j S_i^-1 of the ground truth times exp(N(0, 1e-3)) on the six non-scale components.  Then every vertex is
    relabelled by a random permutation and `n_fixed` vertices are fixed at random: fixed vertices sit in the middle of the slot
    numbering, and with more than one of them edges join fixed to fixed and fixed to free.  `fix_scale` only travels with the
    problem (the caller hands it to both optimisers)."""
    assert n >= 2 and 1 <= n_fixed < n
    p = synth.pose_graph_problem(n, seed, covis=1, n_loop=0, drift_scale=drift_scale)
    rng = np.random.default_rng([0x51E3, int(n), int(seed), int(n_fixed)])
    gt = p["verts_gt"]
    pairs = [(i, i + 1) for i in range(n - 1)]
    while len(pairs) < n - 1 + 2 * n:
        i, j = (int(x) for x in rng.integers(0, n, 2))
        if i != j:
            pairs.append((i, j))
    hub = n // 2
    pairs += [((hub, v) if rng.integers(0, 2) else (v, hub)) for v in range(n) if v != hub]

    def measure(i, j):
        noise = s3_exp(np.concatenate([rng.normal(0, 1e-3, 6), [0.0]]))
        return s3_mul(noise, s3_mul(gt[j], s3_inv(gt[i])))

    meas = [measure(i, j) for i, j in pairs]
    for k in rng.integers(0, len(pairs), 5):
        pairs.append(pairs[k]); meas.append(meas[k].copy())
    for k in rng.integers(0, len(pairs), 5):
        i, j = pairs[k]
        pairs.append((j, i)); meas.append(measure(j, i))
    perm = rng.permutation(n)                                         # old label -> new label
    verts = np.empty_like(p["verts"]); verts[perm] = p["verts"]
    verts_gt = np.empty_like(gt); verts_gt[perm] = gt
    fixed = np.zeros(n, np.uint8); fixed[rng.choice(n, n_fixed, replace=False)] = 1
    e = np.array(pairs)
    return dict(verts=verts, verts_gt=verts_gt, fixed=fixed, edge_i=perm[e[:, 0]].astype(np.int32), edge_j=perm[e[:, 1]].astype(np.int32),
                meas=np.array(meas), fix_scale=bool(fix_scale))


# (n, n_fixed, fix_scale, drift_scale) -> seed: the first seed at which
#   - the oracle's run takes at least four converging iterations (converging_prefix),
#   - every fixed vertex lies strictly inside the numbering and, with several of them, edges join fixed to fixed and fixed to free,
#   - the oracle is steady (oracle_is_steady with 8 one-ulp changes of the input): its own wobble is within a quarter of each bound.
# All three are conditions on the oracle alone; tests/test_sim3_ref_cpu.py asserts them.  Small graphs start close to their optimum
# and Gauss-Newton is there in two steps: (11, 2, True, 0) has a prefix of four or more at 40 seeds of 6000, the first of them 477.
# With the scale free the oracle's own chi2 trajectory on 65 vertices moves by 1e-3 ... 1e-1 under a one-ulp change at most seeds
# (seed 0: 2e-3, four times CHI_RTOL); seed 80 is the first of 0 ... 80 that meets all three (wobble 8.5e-5).
GRAPH_SEEDS = {(6, 1, True, 0.0): 25, (10, 1, False, 0.01): 1, (11, 2, True, 0.0): 477, (35, 3, True, 0.0): 10, (42, 1, True, 0.0): 0, (65, 1, False, 0.01): 80}
# n_free -> seed of irregular_graph(n_free + 1, seed), chosen the same way.  One free vertex joined to the fixed one by all 16 edges
# is a single 7 x 7 system that converges at once: over 3000 seeds the prefix is 1 or 2, never more, so that row asks for 2.
PANEL_SEEDS = {1: 0, 2: 32, 4: 1, 5: 25, 9: 1, 32: 0, 41: 0, 50: 0, 64: 0}
PANEL_MIN_PREFIX = {1: 2}


def converging_prefix(lo):
    """The leading oracle iterations that take their first trial and still move chi2 by more than 1 %: beyond them both sides decide
    lambda on differences at rounding level (tests/test_sim3_gpu.py draws the same line with a fixed 8)."""
    k = 0
    while k < len(lo) and lo["trials"][k] == 1 and lo["chi2_after"][k] < 0.99 * lo["chi2_before"][k]:
        k += 1
    return k


def oracle_wobble(O, p, iters, trials=4):
    """How far the oracle's own run moves when every measurement and free vertex is changed by at most one ulp: the largest relative
    change of chi2_before / chi2_after / lambda over the converging prefix (1.0 if a trial count changes), and the largest change of
    the final rotations, translations and scales.  Both optimisers differentiate numerically with delta = 1e-9, and with the scale
    free the coefficients of log / exp cancel for small sigma: there the reference itself is only good to 1e-3 ... 1e-1 and a
    comparison at CHI_RTOL says nothing about the kernels.  Returns (chi, rot, trans, scale)."""
    fix_scale, free = p["fix_scale"], p["fixed"] == 0
    e = O.sim3_edges(p["edge_i"], p["edge_j"], p["meas"])
    v0, l0 = O.sim3_graph_optimize(p["verts"], p["fixed"], e, fix_scale, iters)
    k = converging_prefix(l0)
    chi = rot = trans = scale = 0.0
    for trial in range(trials):
        rng = np.random.default_rng([0x0B1E, trial])
        q = O.sim3_edges(p["edge_i"], p["edge_j"], p["meas"] * (1 + rng.integers(-1, 2, p["meas"].shape) * 2.0 ** -52))
        verts = p["verts"].copy(); verts[free] *= 1 + rng.integers(-1, 2, verts[free].shape) * 2.0 ** -52
        v1, l1 = O.sim3_graph_optimize(verts, p["fixed"], q, fix_scale, iters)
        if len(l1) < k or not np.array_equal(l1["trials"][:k], l0["trials"][:k]):
            chi = 1.0
        else:
            chi = max([chi] + [float(np.abs(l1[f][:k] / l0[f][:k] - 1).max()) for f in ("chi2_before", "chi2_after", "lambda") if k])
        rot = max(rot, float(rot_err(v1[:, :4], v0[:, :4]).max())); trans = max(trans, float(np.abs(v1[:, 4:7] - v0[:, 4:7]).max()))
        scale = max(scale, float(np.abs(v1[:, 7] - v0[:, 7]).max()))
    return chi, rot, trans, scale


def oracle_is_steady(O, p, iters, trials=4):
    """The precondition of a comparison at CHI_RTOL / ROT_TOL / TRANS_TOL / 1e-4: the oracle's own answer to a one-ulp change of its
    input stays within a quarter of each bound."""
    chi, rot, trans, scale = oracle_wobble(O, p, iters, trials)
    return chi <= CHI_RTOL / 4 and rot <= ROT_TOL / 4 and trans <= TRANS_TOL / 4 and scale <= 1e-4 / 4


def compare_graph(hip, O, ctx, p, iters, min_prefix=4, first_step_only=False):
    """The comparisons of an irregular graph with the oracle: per-edge chi2 before, the logs over the converging prefix, the final
    vertices, fixed vertices and (scale fixed) scales bit for bit.  `first_step_only` (for a graph on which the oracle is not steady,
    see oracle_wobble): the logs over the first iteration alone -- one linearisation, assembly, solve and update, which a one-ulp
    change moves by 1e-6 at most -- and no final vertices.  Returns (checks, info): a dict of booleans and the figures."""
    fix_scale = p["fix_scale"]
    eo = O.sim3_edges(p["edge_i"], p["edge_j"], p["meas"])
    vo, lo = O.sim3_graph_optimize(p["verts"], p["fixed"], eo, fix_scale, iters)
    chi_o = np.array([O.sim3_graph_chi2(p["verts"], eo[k:k + 1]) for k in range(len(eo))])
    pg = hip.PoseGraph(ctx, p["verts"], p["fixed"], hip.sim3_edges(p["edge_i"], p["edge_j"], p["meas"]), fix_scale)
    try:
        chi_g = pg.chi2()
        lg = pg.optimize(iters)
        vg = pg.get()
    finally:
        pg.close()
    k = min(converging_prefix(lo), len(lg))
    if first_step_only:
        k = min(k, 1)
    fx = p["fixed"] != 0
    checks = dict(
        chi_edges=bool(np.allclose(chi_g, chi_o, rtol=1e-12, atol=0.0)),
        prefix=k >= min_prefix,
        chi_before=bool(np.allclose(lg["chi2_before"][:k], lo["chi2_before"][:k], rtol=CHI_RTOL)),
        chi_after=bool(np.allclose(lg["chi2_after"][:k], lo["chi2_after"][:k], rtol=CHI_RTOL)),
        trials=bool(np.array_equal(lg["trials"][:k], lo["trials"][:k])),
        lam=bool(np.allclose(lg["lambda"][:k], lo["lambda"][:k], rtol=CHI_RTOL)),
        rot=bool(first_step_only or rot_err(vg[:, :4], vo[:, :4]).max() < ROT_TOL),
        trans=bool(first_step_only or np.abs(vg[:, 4:7] - vo[:, 4:7]).max() < TRANS_TOL),
        scale=bool(first_step_only or np.abs(vg[:, 7] - vo[:, 7]).max() < 1e-4),
        fixed_kept=bool(np.array_equal(vg[fx], p["verts"][fx]) and np.array_equal(vo[fx], p["verts"][fx])),
        scale_kept=bool(not fix_scale or np.array_equal(vg[:, 7], p["verts"][:, 7])))
    return checks, dict(prefix=k, lg=lg, lo=lo, vg=vg, vo=vo, n_edges=len(eo), rot_dev=float(rot_err(vg[:, :4], vo[:, :4]).max()),
                        trans_dev=float(np.abs(vg[:, 4:7] - vo[:, 4:7]).max()))


# ---- pair problems ----------------------------------------------------------------------------------------------------------
def exact_pair_problem(n, seed, **kw):
    """synth.sim3_pair_problem drops the points that fall behind camera 1, so its sizes are not exact: draw 40 more and cut every
    per-pair array to exactly n."""
    p = synth.sim3_pair_problem(n + 40, seed, **kw)
    for key in ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "outlier"):
        p[key] = p[key][:n]
        assert len(p[key]) == n, (key, len(p[key]), n)
    return p


PAIR_CASES = [(9, 0.0), (10, 0.0), (10, 0.3), (12, 0.2), (64, 0.1), (255, 0.1), (256, 0.1), (257, 0.1), (513, 0.1), (1025, 0.3)]   # n, outlier_frac; seed = n
PAIR_MODES = [(1.0, True), (1.15, False)]                              # scale, fix_scale


def pair_problems(scale, fix_scale):
    return [exact_pair_problem(n, n, scale=scale, outlier_frac=frac, init_noise=(0.02, 0.15, 0.0 if fix_scale else 0.03)) for n, frac in PAIR_CASES]


def pair_threshold_gap(s12, p, chi_sq):
    """Smallest |w e^2 / chi_sq - 1| over both reprojection edges of every pair at S12, in numpy: how far the nearest pair is from
    flipping between inlier and outlier."""
    q, t, s = s12[:4], s12[4:7], s12[7]
    cam1, cam2 = p["cam1"], p["cam2"]
    si = s3_inv(np.asarray(s12, np.float64))
    x1 = np.array([s * q_rot(q, v) + t for v in p["p2c"]])
    x2 = np.array([si[7] * q_rot(si[:4], v) + si[4:7] for v in p["p1c"]])
    e1 = p["obs1"] - np.stack([cam1[0] * x1[:, 0] / x1[:, 2] + cam1[2], cam1[1] * x1[:, 1] / x1[:, 2] + cam1[3]], axis=1)
    e2 = p["obs2"] - np.stack([cam2[0] * x2[:, 0] / x2[:, 2] + cam2[2], cam2[1] * x2[:, 1] / x2[:, 2] + cam2[3]], axis=1)
    r = np.concatenate([p["inv_sigma2_1"] * (e1 ** 2).sum(1), p["inv_sigma2_2"] * (e2 ** 2).sum(1)]) / chi_sq
    return float(np.abs(r - 1).min()) if len(r) else np.inf


# ---- log / exp probes and their 50-digit reference ---------------------------------------------------------------------------------
PROBE_THETA = [0.0, 1e-7, 3e-3, 4.4e-3, 4.5e-3, 0.5, 2.0, 3.0, 3.14]  # 4.4e-3 / 4.5e-3 straddle d = 1 - 1e-5
PROBE_SIGMA = [0.0, 5e-6, 2e-5, 0.4, -0.7]                             # 5e-6 / 2e-5 straddle |sigma| = 1e-5
PROBE_SEED = 10

# largest relative deviation of the oracle's |log M|^2 from mpmath per theta class (see the module docstring)
ORACLE_VS_MP = {0.0: 1.9e-16, 1e-7: 3.7e-16, 3e-3: 1.5e-9, 4.4e-3: 4.4e-9, 4.5e-3: 4.4e-16, 0.5: 4.8e-16, 2.0: 3.6e-16, 3.0: 1.3e-14, 3.14: 6.1e-11}
ULP64 = 64 * 2.0 ** -52                                                # 1.4e-14


def log_bound(theta):
    """Relative bound of the device's |log M|^2 against mpmath for a probe of class theta: both sides restate the same formulas in
    double precision with different acos / sqrt / log and no contraction, hence 8 x the oracle's own deviation, 64 ulp at least."""
    return max(8 * ORACLE_VS_MP[theta], ULP64)


def probe_updates():
    """The 45 probes u = (theta axis, upsilon, sigma), theta-major; returns (u 45 x 7, theta class per probe)."""
    rng = np.random.default_rng(PROBE_SEED)
    u, cls = [], []
    for theta in PROBE_THETA:
        for sigma in PROBE_SIGMA:
            axis = rng.normal(0, 1, 3); axis /= np.linalg.norm(axis)
            u.append(np.concatenate([theta * axis, rng.normal(0, 1, 3), [sigma]])); cls.append(theta)
    return np.array(u), np.array(cls)


def mp_sim3_log_chi2(meas):
    """|log M|^2 at 50 digits: g2o's Sim3::log as oracle/ora_sim3.c restates it, the same four branches, the quaternion turned into
    R as the code does it (no normalisation), W x = t solved by LU."""
    import mpmath as mp
    with mp.workdps(50):
        w, x, y, z = (mp.mpf(float(v)) for v in meas[:4])
        t = mp.matrix([mp.mpf(float(v)) for v in meas[4:7]])
        s = mp.mpf(float(meas[7]))
        R = mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        sigma = mp.log(s)
        d = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
        dR = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        eps = mp.mpf("0.00001")
        small = d > 1 - eps
        if small:
            theta, omega = mp.mpf(0), dR / 2
        else:
            theta = mp.acos(d)
            omega = dR * (theta / (2 * mp.sqrt(1 - d * d)))
        if abs(sigma) < eps:
            C = mp.mpf(1)
            if small:
                A, B = mp.mpf(1) / 2, mp.mpf(1) / 6
            else:
                A, B = (1 - mp.cos(theta)) / theta ** 2, (theta - mp.sin(theta)) / theta ** 3
        else:
            C = (s - 1) / sigma
            if small:
                A = ((sigma - 1) * s + 1) / sigma ** 2
                B = ((sigma ** 2 / 2 - sigma + 1) * s - 1) / sigma ** 3
            else:
                a, b, c = s * mp.sin(theta), s * mp.cos(theta), theta ** 2 + sigma ** 2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
        Om = mp.matrix([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
        W = A * Om + B * (Om * Om) + C * mp.eye(3)
        ups = mp.lu_solve(W, t)
        return float(sum(v * v for v in omega) + sum(v * v for v in ups) + sigma * sigma)


# ---- two-vertex problems with a closed-form optimum --------------------------------------------------------------------------
CLOSED_FORM = [(0.3, 0.0, True), (2.5, 0.0, True), (2.5, 0.5, False), (3.1, -0.6, False)]     # theta, sigma, fix_scale
V0 = np.array([0.8, 0.2, -0.4, 0.4, 1.5, -0.7, 2.0, 1.0])             # the fixed vertex: a unit quaternion, a translation, scale 1


def two_vertex_problem(theta, sigma, seed=5):
    """Vertex 0 fixed at V0, vertex 1 started there, one edge 0 -> 1 carrying M = exp(u): error = log(M v0 v1^-1), so the optimum
    is v1 = M v0 (scale free), and with the scale fixed and sigma != 0 everything but sigma^2 can be taken out of the error.
    The oracle reaches M v0 to 4e-15 only where no update of its run falls between 1e-8 and 1e-5 rad: there exp takes g2o's
    small-angle R = I + Omega + Omega^2, which is off orthonormal by the update squared, the products are not renormalised, and
    the vertex ends 1e-12 ... 3e-11 from M v0 with chi2 at 1e-31 all the same.  With upsilon ~ N(0, 0.5) the theta = 0.3
    problem does so at every one of 30 seeds; with N(0, 2) most seeds avoid it, and seed 5 does for all four problems."""
    rng = np.random.default_rng([0xC105, int(seed)])
    axis = rng.normal(0, 1, 3); axis /= np.linalg.norm(axis)
    u = np.concatenate([theta * axis, rng.normal(0, 2.0, 3), [sigma]])
    M = s3_exp(u)
    return dict(verts=np.stack([V0, V0]), fixed=np.array([1, 0], np.uint8), edge_i=np.array([0], np.int32), edge_j=np.array([1], np.int32),
                meas=M[None], u=u, want=s3_mul(M, V0))
