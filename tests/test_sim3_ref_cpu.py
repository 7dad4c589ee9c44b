"""The references of the Sim3 limit tests, checked against each other without a GPU: the probe fixture against its generator and
against mpmath, the CPU oracle against mpmath per theta class (the table the GPU bound of test_sim3_limits_gpu.py is derived
from), and the oracle against the closed-form optimum of the two-vertex problems."""
import numpy as np
import pytest

import sim3_cases as S3
from conftest import golden


@pytest.fixture(scope="module")
def probes():
    return golden("g10_sim3_probes.npz")


def test_fixture_is_the_generators(oracle, probes):
    u, theta = S3.probe_updates()
    assert len(u) == 45 and np.array_equal(probes["u"], u) and np.array_equal(probes["theta"], theta)
    assert np.array_equal(probes["M"], np.array([oracle.sim3_exp(x) for x in u]))                  # bit for bit
    assert not np.any(np.isclose(np.abs(u[:, 6]), 1e-5, rtol=1e-3, atol=0))                           # no probe on a threshold


def test_fixture_mpmath_values_regenerate(probes):
    pytest.importorskip("mpmath")
    assert np.array_equal(probes["chi2_mp"], np.array([S3.mp_sim3_log_chi2(m) for m in probes["M"]]))


def test_oracle_against_mpmath_per_theta_class(oracle, probes):
    """The oracle's |log M|^2 on a two-vertex identity graph with one edge carrying M, against the 50-digit value: the largest
    relative deviation of every theta class is the one tabulated in sim3_cases.ORACLE_VS_MP (measured; the table rounds up to two
    digits), so the GPU bound derived from it stays a measured one."""
    ident = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0]), (2, 1))
    got = np.array([oracle.sim3_graph_chi2(ident, oracle.sim3_edges([0], [1], m[None])) for m in probes["M"]])
    rel = np.abs(got - probes["chi2_mp"]) / probes["chi2_mp"]
    for theta in S3.PROBE_THETA:
        worst = rel[probes["theta"] == theta].max()
        print("theta %-7g oracle vs mpmath %.3e (table %.1e, GPU bound %.1e)" % (theta, worst, S3.ORACLE_VS_MP[theta], S3.log_bound(theta)))
        assert worst <= S3.ORACLE_VS_MP[theta]
    # where the branch table is well conditioned the oracle is good to a few ulp; the classes that are not are named in the table
    assert all(S3.ORACLE_VS_MP[t] < 1e-15 for t in (0.0, 1e-7, 4.5e-3, 0.5, 2.0))


GRAPHS = sorted(set([c + (seed,) for c, seed in S3.GRAPH_SEEDS.items()] + [(n_free + 1, 1, True, 0.0, seed) for n_free, seed in S3.PANEL_SEEDS.items()]))


@pytest.mark.parametrize("n,n_fixed,fix_scale,drift_scale,seed", GRAPHS)
def test_graph_cases_are_a_fair_demand(oracle, n, n_fixed, fix_scale, drift_scale, seed):
    """What the GPU tests presuppose of their graphs, on the oracle alone: it converges, its run has a converging prefix of four
    iterations (two for the single free vertex), fixed vertices stay bit for bit, and a one-ulp change of the input moves its own
    logs and vertices by no more than a quarter of the bounds the device is held to."""
    p = S3.irregular_graph(n, seed, n_fixed, fix_scale, drift_scale)
    fx = p["fixed"] != 0
    v, lo = oracle.sim3_graph_optimize(p["verts"], p["fixed"], oracle.sim3_edges(p["edge_i"], p["edge_j"], p["meas"]), fix_scale, 15)
    assert S3.converging_prefix(lo) >= (S3.PANEL_MIN_PREFIX.get(n - 1, 4) if n_fixed == 1 and fix_scale else 4)
    assert lo["chi2_after"][-1] < 1e-2 * lo["chi2_before"][0] and np.array_equal(v[fx], p["verts"][fx])
    wobble = S3.oracle_wobble(oracle, p, 15, 8)
    print("n %d: prefix %d, wobble chi %.1e rot %.1e trans %.1e scale %.1e" % ((n, S3.converging_prefix(lo)) + wobble))
    assert wobble[0] <= S3.CHI_RTOL / 4 and wobble[1] <= S3.ROT_TOL / 4 and wobble[2] <= S3.TRANS_TOL / 4 and wobble[3] <= 1e-4 / 4


def _aligned(v, want):
    return np.concatenate([np.sign(np.dot(v[:4], want[:4])) * v[:4], v[4:]])


@pytest.mark.parametrize("theta,sigma,fix_scale", S3.CLOSED_FORM)
def test_oracle_reaches_the_closed_form_optimum(oracle, theta, sigma, fix_scale):
    """Vertex 0 fixed at a non-trivial v0, one edge M = exp(u), vertex 1 started at v0: the optimum is S_1 = M v0, and the oracle is
    there to 4e-15 within 8 iterations."""
    p = S3.two_vertex_problem(theta, sigma)
    v, log = oracle.sim3_graph_optimize(p["verts"], p["fixed"], oracle.sim3_edges(p["edge_i"], p["edge_j"], p["meas"]), fix_scale, 8)
    dev = np.abs(_aligned(v[1], p["want"]) - p["want"]).max()
    print("theta %g sigma %g fix_scale %d: %d iterations, |S_1 - M v0| %.2e, chi2 %.2e" % (theta, sigma, fix_scale, len(log), dev, log["chi2_after"][-1]))
    assert dev <= 4e-15 and np.array_equal(v[0], S3.V0)


def test_fixed_scale_leaves_sigma_squared(oracle):
    """Scale fixed and sigma = 0.3 in the measurement: rotation and translation can be matched, the scale cannot, chi2 ends at
    sigma^2 = 9.000e-02."""
    p = S3.two_vertex_problem(0.3, 0.3)
    v, log = oracle.sim3_graph_optimize(p["verts"], p["fixed"], oracle.sim3_edges(p["edge_i"], p["edge_j"], p["meas"]), True, 8)
    print("chi2 %.15e" % log["chi2_after"][-1])
    assert abs(log["chi2_after"][-1] - 0.3 ** 2) < 1e-12 and v[1, 7] == S3.V0[7]
    # the optimum in closed form: M v0 with the scale taken back out, D^-1 M v0 with D the pure scaling by exp(sigma)
    want = S3.s3_mul(np.array([1.0, 0, 0, 0, 0, 0, 0, np.exp(-0.3)]), p["want"])
    assert np.abs(_aligned(v[1], want) - want).max() < 1e-9
