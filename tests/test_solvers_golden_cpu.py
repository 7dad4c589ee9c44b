"""CPU replay of tests/golden/g20_solvers.npz (tools/make_golden_solvers.py): the host library's eigen-solver, EPnP, PnP RANSAC, Sim3
RANSAC and two-view initialiser return the recorded bytes -- the fixture was written before their arithmetic was folded onto the
shared headers, and every later change of those headers answers to it.  Comparisons are of tobytes(): exact
and NaN-safe.  The one exception is the two-view parallax, which goes through acos (libm may round it differently on another
machine): 1e-12 relative."""
import ctypes as C
import os

import numpy as np
import pytest

import solver_cases as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_solvers.npz")


@pytest.fixture(scope="module")
def lib():
    from lpslam_amd import _build
    return C.CDLL(_build.host_library())


@pytest.fixture(scope="module")
def cases():
    return S.load(GOLDEN)


@pytest.mark.parametrize("fn,at_least", [("sym_eigen", 32), ("epnp", 40), ("pnp_ransac", 60), ("sim3_ransac", 18), ("two_view", 2)])
def test_solver_returns_the_recorded_bytes(lib, cases, fn, at_least):
    mine = [c for c in cases if c[0] == fn]
    assert len(mine) >= at_least
    for _, tag, args, arrays, want in mine:
        got = S.run(lib, fn, args, arrays)
        assert sorted(got) == sorted(want), tag
        for name, w in want.items():
            g = np.ascontiguousarray(got[name])
            assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
            if fn == "two_view" and name == "parallax_deg":
                assert abs(g[0] - w[0]) <= 1e-12 * abs(w[0]), (tag, g[0], w[0])
            else:
                assert g.tobytes() == w.tobytes(), (fn, tag, args, name)


def test_the_fixture_holds_both_refit_outcomes_and_a_sign_flip(cases):
    tags = [tag for fn, tag, *_ in cases if fn == "pnp_ransac"]
    assert any(t.endswith("refit kept") for t in tags) and any(t.endswith("refit rejected") for t in tags)
    assert any(fn == "epnp" and ", 0 guesses" not in tag and "refused" not in tag for fn, tag, *_ in cases)
