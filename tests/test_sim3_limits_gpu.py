"""The Sim3 optimisers (lpslam_hip_sim3_*) where tests/test_sim3_gpu.py does not go: pose graphs of irregular shape (reversed and
duplicated edges, a hub, fixed vertices in the middle of the slot numbering, an isolated vertex), every panel boundary of the dense
solve that 7 n_free unknowns can reach, all four branches of log / exp against a 50-digit reference, large updates against a
closed-form optimum, and the pair optimiser on either side of its workgroup width and of its ten-pair gate.  The generators, the
tolerances and the measured figures the bounds come from are in tests/sim3_cases.py; tests/test_sim3_ref_cpu.py checks the
references against each other."""
import numpy as np
import pytest

import sim3_cases as S3
from conftest import golden
from sim3_cases import CHI_RTOL, ROT_TOL, TRANS_TOL, rot_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


def _assert_graph(hiplib, oracle, ctx, p, iters=15, min_prefix=4):
    checks, info = S3.compare_graph(hiplib, oracle, ctx, p, iters, min_prefix)
    print("edges %d prefix %d oracle trials %s" % (info["n_edges"], info["prefix"], list(info["lo"]["trials"])))
    assert all(checks.values()), [k for k, ok in checks.items() if not ok]
    return info


# ---- (a) irregular graphs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_fixed,fix_scale,drift_scale", list(S3.GRAPH_SEEDS))
def test_irregular_graph_parity(hiplib, oracle, ctx, n, n_fixed, fix_scale, drift_scale):
    p = S3.irregular_graph(n, S3.GRAPH_SEEDS[(n, n_fixed, fix_scale, drift_scale)], n_fixed, fix_scale, drift_scale)
    fx = p["fixed"] != 0
    assert fx.sum() == n_fixed and not fx[0] and not fx[-1]                            # fixed vertices inside the slot numbering
    both, one = fx[p["edge_i"]] & fx[p["edge_j"]], fx[p["edge_i"]] ^ fx[p["edge_j"]]
    assert one.any() and (n_fixed == 1 or both.any())                                 # fixed-free edges, and fixed-fixed ones with several fixed
    assert (np.bincount(np.r_[p["edge_i"], p["edge_j"]]).max() >= n - 1)             # the hub
    _assert_graph(hiplib, oracle, ctx, p)


def test_isolated_free_vertex(hiplib, oracle, ctx):
    """A 12-vertex chain (each vertex joined to its next two) with every edge at one vertex dropped: that vertex's diagonal block is
    lambda I and its rhs zero, and it must come back bit for bit on both sides (the oracle keeps it and runs all 15 iterations)."""
    p = S3.synth.pose_graph_problem(12, 3, covis=2, n_loop=0)          # neighbours and next neighbours: the rest stays in one piece
    lone = 7
    keep = (p["edge_i"] != lone) & (p["edge_j"] != lone)
    assert keep.sum() == len(keep) - 4
    ei, ej, meas = p["edge_i"][keep], p["edge_j"][keep], p["meas"][keep]
    vo, lo = oracle.sim3_graph_optimize(p["verts"], p["fixed"], oracle.sim3_edges(ei, ej, meas), True, 15)
    pg = hiplib.PoseGraph(ctx, p["verts"], p["fixed"], hiplib.sim3_edges(ei, ej, meas), True)
    lg = pg.optimize(15)
    vg = pg.get()
    assert len(lo) == 15 and np.array_equal(vo[lone], p["verts"][lone])
    assert np.array_equal(vg[lone], p["verts"][lone]) and np.array_equal(vg[0], p["verts"][0])
    k = S3.converging_prefix(lo)
    assert k >= 4
    S3._check(vg, vo, lg, lo, k)


# ---- (b) panel boundaries of the dense solve --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_free,nb,need", [(1, 1, 7), (2, 1, 14), (4, 1, 28), (5, 2, 3), (9, 2, 31), (32, 8, 0), (41, 9, 31), (50, 11, 30), (64, 15, 0)])
def test_panel_boundaries(hiplib, oracle, ctx, n_free, nb, need):
    """dim = 7 n_free through the panel-pair chain: a single panel, an odd `need`, need = 31 (the rhs column last in its panel, no
    identity padding at all when dim + 1 = 64), an empty last column under odd and even nb.  Parity as for the irregular graphs,
    and two graphs built from the same input agree byte for byte."""
    assert S3.panel_shape(n_free) == (nb, need)
    n = n_free + 1
    p = S3.irregular_graph(n, S3.PANEL_SEEDS[n_free], 1, True, 0.0)
    assert int((p["fixed"] == 0).sum()) == n_free
    info = _assert_graph(hiplib, oracle, ctx, p, min_prefix=S3.PANEL_MIN_PREFIX.get(n_free, 4))
    e = hiplib.sim3_edges(p["edge_i"], p["edge_j"], p["meas"])
    again = hiplib.PoseGraph(ctx, p["verts"], p["fixed"], e, True)
    la = again.optimize(15)
    assert la.tobytes() == info["lg"].tobytes() and again.get().tobytes() == info["vg"].tobytes()


# ---- (c) log branches -------------------------------------------------------------------------------------------------------
def test_log_branches_against_mpmath(hiplib, oracle, ctx):
    """The fixture's 45 probes as 45 parallel edges between two identity vertices: the edge error is log(M) itself.  Per edge the
    device's chi2 lies within log_bound(theta) of the 50-digit value (8 x the oracle's own deviation in that theta class, 64 ulp at
    least: the table in sim3_cases.py), and up to theta = 2 within 1e-12 of the oracle."""
    g = golden("g10_sim3_probes.npz")
    M, theta, want = g["M"], g["theta"], g["chi2_mp"]
    assert len(M) == 45
    ident = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0]), (2, 1))
    zeros, ones = np.zeros(45, np.int32), np.ones(45, np.int32)
    pg = hiplib.PoseGraph(ctx, ident, np.array([1, 0], np.uint8), hiplib.sim3_edges(zeros, ones, M), False)
    got = pg.chi2()
    ora = np.array([oracle.sim3_graph_chi2(ident, oracle.sim3_edges([0], [1], m[None])) for m in M])
    rel, rel_o = np.abs(got - want) / want, np.abs(got - ora) / ora
    bound = np.array([S3.log_bound(t) for t in theta])
    for t in S3.PROBE_THETA:
        print("theta %-7g device vs mpmath %.3e (bound %.1e)   device vs oracle %.3e" % (t, rel[theta == t].max(), S3.log_bound(t), rel_o[theta == t].max()))
    assert np.all(rel <= bound), [(float(theta[k]), float(g["u"][k, 6]), float(rel[k])) for k in np.nonzero(rel > bound)[0]]
    assert np.all(rel_o[theta <= 2.0] <= 1e-12)


# ---- (d) closed form on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta,sigma,fix_scale", S3.CLOSED_FORM + [(0.3, 0.3, True)])
def test_closed_form_two_vertex(hiplib, oracle, ctx, theta, sigma, fix_scale):
    """One edge M = exp(u) from a fixed v0 to a vertex started at v0: the optimum is M v0, reached through updates of up to three
    radians and |sigma| 0.6 -- the only place where exp's large-angle and sigma != 0 branches see large arguments.  With the scale
    fixed and sigma = 0.3 the optimum keeps v0's scale and chi2 ends at sigma^2."""
    p = S3.two_vertex_problem(theta, sigma)
    vo, lo = oracle.sim3_graph_optimize(p["verts"], p["fixed"], oracle.sim3_edges(p["edge_i"], p["edge_j"], p["meas"]), fix_scale, 15)
    pg = hiplib.PoseGraph(ctx, p["verts"], p["fixed"], hiplib.sim3_edges(p["edge_i"], p["edge_j"], p["meas"]), fix_scale)
    lg = pg.optimize(15)
    vg = pg.get()
    want = p["want"]
    if fix_scale and sigma:
        want = S3.s3_mul(np.array([1.0, 0, 0, 0, 0, 0, 0, np.exp(-sigma)]), want)      # the scale cannot follow: D^-1 M v0
        assert np.isclose(lg["chi2_after"][-1], lo["chi2_after"][-1], rtol=CHI_RTOL) and np.isclose(lo["chi2_after"][-1], sigma ** 2, rtol=1e-9)
    for ref in (want[None], vo[1:2]):
        assert rot_err(vg[1:2, :4], ref[:, :4]).max() < ROT_TOL
        assert np.abs(vg[1, 4:7] - ref[0, 4:7]).max() < TRANS_TOL and abs(vg[1, 7] - ref[0, 7]) < 1e-4
    assert np.array_equal(vg[0], S3.V0) and (not fix_scale or vg[1, 7] == S3.V0[7])


# ---- (e) pair optimiser sizes -----------------------------------------------------------------------------------------------
ORACLE_INLIERS = {(1.0, True): [0, 10, 0, 10, 48, 229, 226, 232, 451, 725], (1.15, False): [0, 10, 0, 10, 49, 228, 226, 230, 452, 726]}


@pytest.fixture(scope="module", params=S3.PAIR_MODES, ids=["fixed_scale", "free_scale"])
def pair_set(request, oracle):
    """The ten problems of one mode with the oracle's answer to each, computed once."""
    scale, fix_scale = request.param
    probs = S3.pair_problems(scale, fix_scale)
    ref = [oracle.sim3_transform_optimize(p["s12"], oracle.sim3_pairs(p), p["cam1"], p["cam2"], 10.0, fix_scale) for p in probs]
    return scale, fix_scale, probs, ref


def _run_pairs(hiplib, ctx, probs, fix_scale):
    if not probs:
        return np.zeros((0, 8)), [], np.zeros(0, np.int32)
    return hiplib.sim3_transform_optimize(ctx, np.array([p["s12"] for p in probs]), [hiplib.sim3_pairs(p) for p in probs], probs[0]["cam1"], probs[0]["cam2"], 10.0, fix_scale)


def _assert_pair(p, got, ref, fix_scale):
    (sg, inl_g, cnt_g), (so, inl_o, cnt_o) = got, ref
    assert cnt_g == cnt_o and np.array_equal(inl_g, inl_o.astype(bool))                # identical inlier sets
    assert rot_err(sg[None, :4], so[None, :4]).max() < ROT_TOL and np.abs(sg[4:7] - so[4:7]).max() < TRANS_TOL
    assert abs(sg[7] - so[7]) < 1e-4
    if fix_scale:
        assert sg[7] == p["s12"][7]


def test_pair_cases_are_what_they_claim(pair_set):
    """The oracle's side alone: exact sizes, the inlier counts that put the cases on the gate (9 pairs: none; 10 clean pairs: 10;
    10 pairs with one outlier: 9 survive the cut, none; 12 with two outliers: exactly 10), and no pair closer than 1e-4 to the
    inlier threshold at the oracle's final S12 -- only then is an identical inlier mask a fair demand."""
    scale, fix_scale, probs, ref = pair_set
    assert [len(p["p1c"]) for p in probs] == [n for n, _ in S3.PAIR_CASES]
    assert [r[2] for r in ref] == ORACLE_INLIERS[(scale, fix_scale)]
    assert [int(p["outlier"].sum()) for p in probs[:4]] == [0, 0, 1, 2]
    gaps = [S3.pair_threshold_gap(r[0], p, 10.0) for p, r in zip(probs, ref)]
    print("threshold gaps", ["%.2e" % g for g in gaps])
    assert min(gaps) >= 1e-4


def test_pair_sizes_one_batch(hiplib, ctx, pair_set):
    """All ten sizes in one launch: one workgroup each, 256 threads striding over 9 ... 1025 pairs."""
    scale, fix_scale, probs, ref = pair_set
    s, inl, cnt = _run_pairs(hiplib, ctx, probs, fix_scale)
    for i, p in enumerate(probs):
        _assert_pair(p, (s[i], inl[i], cnt[i]), ref[i], fix_scale)
        assert np.abs(s[i] - p["s12_gt"]).max() < 0.5 * np.abs(p["s12"] - p["s12_gt"]).max()          # and it moved towards the truth


def test_pair_layouts_and_batch_independence(hiplib, ctx, pair_set):
    """An empty problem between two full ones, and the 1025-pair problem first: pair_start offsets that are no multiple of
    anything.  Every problem's result in a batch equals, byte for byte, the same problem run alone."""
    scale, fix_scale, probs, ref = pair_set
    alone = [_run_pairs(hiplib, ctx, [p], fix_scale) for p in probs]
    batch = _run_pairs(hiplib, ctx, probs, fix_scale)
    for i in range(len(probs)):
        assert batch[0][i].tobytes() == alone[i][0][0].tobytes() and np.array_equal(batch[1][i], alone[i][1][0]) and batch[2][i] == alone[i][2][0]
    empty = dict(probs[7])
    for key in ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        empty[key] = empty[key][:0]
    for order in ([7, None, 5], [9, 3, 8, 1]):
        sel = [empty if k is None else probs[k] for k in order]
        s, inl, cnt = _run_pairs(hiplib, ctx, sel, fix_scale)
        for slot, k in enumerate(order):
            if k is None:
                assert cnt[slot] == 0 and len(inl[slot]) == 0 and np.array_equal(s[slot], empty["s12"])
                continue
            _assert_pair(probs[k], (s[slot], inl[slot], cnt[slot]), ref[k], fix_scale)
            assert s[slot].tobytes() == alone[k][0][0].tobytes() and np.array_equal(inl[slot], alone[k][1][0]) and cnt[slot] == alone[k][2][0]
