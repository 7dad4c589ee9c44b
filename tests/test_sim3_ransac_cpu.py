"""LpSlam::sim3_solve_ransac (lpslam_amd/host/two_view.cpp) against tests/golden/sim3_ransac_draw.npz, byte for byte: the count, the
eight doubles of s12 and the inlier flags of six seeded cases, recorded through lpslam_sim3_solve_ransac BEFORE the solver's 3-match
draw moved to draw<3> of csrc/ransac_sample.h.  A draw that differs in one index picks other hypotheses: the count or s12 changes.
(tests/test_two_view_cpu.py holds the solver to the numpy oracle, to a tolerance; the 4- and 8-match tables are replayed in
tests/test_pnp_cpu.py and tests/test_two_view_batch_cpu.py.)

  n = 3 (one sample possible, drawn in six orders), 4, 37 (about 30 % planted outliers) x fix_scale 0, 1 x seeds 0 (means 1), 1,
  0x9E3779B9 (the tracker's), 50 iterations

Everything the solver computes is + - * / sqrt under -ffp-contract=off: the same bits on every machine.
Recording (deterministic; only ever from a library whose draw is known good): python tests/test_sim3_ransac_cpu.py"""
import ctypes as C
import os

import numpy as np
import pytest

import pnp_cases as P
import solver_cases as S

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_ransac_draw.npz")
CASES = [(3, 0, 0), (3, 1, 1), (4, 0, P.SEED), (4, 1, 0), (37, 0, 1), (37, 1, P.SEED)]          # (n, fix_scale, seed)


def _inputs(n, fix_scale):
    rng = np.random.default_rng(900 + 10 * n + fix_scale)
    c64 = lambda a: np.ascontiguousarray(a, np.float64)
    x2 = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)])
    r = P.rot([0.2, 1.0, -0.1], 0.4); t = np.array([0.8, -0.1, 0.3])
    x1 = (1.0 if fix_scale else 1.37) * (x2 @ r.T) + t
    proj = lambda x: np.column_stack([P.CAM[0] * x[:, 0] / x[:, 2] + P.CAM[2], P.CAM[1] * x[:, 1] / x[:, 2] + P.CAM[3]])
    obs1 = proj(x1) + rng.normal(0, 0.3, (n, 2)); obs2 = proj(x2) + rng.normal(0, 0.3, (n, 2))
    x1n = x1 + rng.normal(0, 0.01, x1.shape)
    if n == 37:
        bad = rng.choice(n, 11, replace=False)                                # 11 of 37: 30 %
        x1n[bad] += rng.normal(0, 1.5, (11, 3))
    w = 1.0 / (1.2 ** rng.integers(0, 4, n)) ** 2
    return dict(p1c=c64(x1n), p2c=c64(x2), obs1=c64(obs1), obs2=c64(obs2), is1=c64(w), is2=c64(w[::-1]), cam=P.CAM)


def _host_lib():
    from lpslam_amd import _build
    return C.CDLL(_build.host_library())


@pytest.fixture(scope="module")
def recorded():
    return S.load(FIXTURE)


def test_the_fixture_holds_the_six_cases(recorded):
    assert [(a["n"], a["fix_scale"], a["seed"], a["iterations"]) for _, _, a, _, _ in recorded] == [(n, f, int(s), 50) for n, f, s in CASES]
    for _, tag, args, arrays, out in recorded:
        assert out["count"][0] >= 3, tag                                   # every case found a similarity: s12 and the flags are results
        assert arrays["p1c"].shape == (args["n"], 3) and out["inlier"].sum() == out["count"][0], tag
    assert any(0 < out["count"][0] < args["n"] for _, _, args, _, out in recorded)          # and the outliers are left out somewhere


@pytest.mark.parametrize("k", range(len(CASES)))
def test_sim3_ransac_returns_the_recorded_bytes(recorded, k):
    fn, tag, args, arrays, want = recorded[k]
    got = S.run(_host_lib(), fn, args, arrays)
    for name in ("count", "s12", "inlier"):
        assert got[name].tobytes() == want[name].tobytes(), (tag, name, got[name], want[name])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    lib = _host_lib()
    cases = [("sim3_ransac", "n %d, fix_scale %d, seed %#x" % (n, f, s), {"n": n, "fix_scale": f, "iterations": 50, "seed": int(s)}, _inputs(n, f)) for n, f, s in CASES]
    S.save(FIXTURE, cases, [S.run(lib, fn, args, arrays) for fn, _, args, arrays in cases])
    print(os.path.basename(FIXTURE), os.path.getsize(FIXTURE), "bytes,", len(cases), "cases")
