"""The register Cholesky of a 32-column panel (csrc/chol_panel.inl) on small dense windows: the block product between the two
strips in full panels (chol_panel_core: the diagonal workgroup without a riding block, row workgroups, Minv rows) and in the
trimmed last panel column (chol_panel_trim with more than 16 real columns: the product and strip B run there too), in a pair's
second column and in a `single` last launch.  Tolerances are those of test_ba_window_gpu.py: chi2 trajectory relative 1e-9,
identical trials / status, lambda relative 1e-6, poses within 1e-4 rad / 1e-3 m of the CPU oracle; a window alone, inside
ba_optimize_batch (where small systems go through k_chol_wg, chol_panel_core<48>) and solved a second time gives the same bytes.

The reduced system has six columns per free keyframe, so a last panel column holds 0, 2, 4, ... real columns: 18 and 30 are the
one-panel windows next to 17 and 31.  S + lambda I is positive definite for every lambda > 0 an LM trial uses -- a keyframe
without observations still has lambda on its diagonal -- so no window here makes the factorisation raise its pivot flag.  The strip's
pivot guard, the flag and its reset have a test of their own: tests/test_ba_solve_gpu.py gives the factor-and-solve matrices that are
not positive definite, with the first failing pivot in every kind of strip, and holds x_p itself to an exact solution."""
import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL, CHI_RTOL = 1e-4, 1e-3, 1e-9
NB = 32                                                     # panel width of the dense factorisation
ITERS = 8


def rot_err(q1, q2):
    return 2 * np.arccos(np.clip(np.abs(np.sum(q1 * q2, axis=1)), 0, 1))


@pytest.fixture(scope="module")
def ctx(hiplib):
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


def _make(hiplib, ctx, pr):
    ba = hiplib.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hiplib.ba_obs_array(pr), pr["cam"])
    ba.set_solver("dense")
    return ba


# (n_kf, n_pts, n_obs) -> panels, real columns of the last panel column; one keyframe of a synthetic window is fixed
CASES = [((4, 150, 450), 1, 18),          # one panel, trimmed: the product, then two pivots of strip B
         ((6, 150, 700), 1, 30),          # ... fourteen pivots of strip B
         ((8, 150, 900), 2, 10),          # a full first panel in the diagonal workgroup and in two Minv rows; the pair's second column ends in strip A
         ((10, 150, 1100), 2, 22),        # ... ends in strip B: full and trimmed product in one launch
         ((14, 150, 1300), 3, 14),        # a row workgroup beside the pair, then a `single` launch
         ((16, 150, 1500), 3, 26),        # the `single` launch's column runs the trimmed product
         ((24, 300, 2400), 5, 10)]        # three launches, lookahead with a previous pair in front of every full panel


@pytest.fixture(scope="module")
def problems():
    return {spec: synth.ba_problem(*spec, 640, 480, seq_id=100 + spec[0]) for spec, _, _ in CASES}


@pytest.fixture(scope="module")
def alone(hiplib, ctx, problems):
    """Every window solved once on its own: (log, poses, points)."""
    out = {}
    for spec, pr in problems.items():
        ba = _make(hiplib, ctx, pr)
        out[spec] = (ba.optimize(True, ITERS),) + ba.state()
        ba.close()
    return out


@pytest.mark.parametrize("spec,nb,need", CASES, ids=["%dkf" % c[0][0] for c in CASES])
def test_panel_against_oracle(oracle, problems, alone, spec, nb, need):
    pr = problems[spec]
    dim = 6 * int((pr["fixed"] == 0).sum())
    assert (dim + 1 + NB - 1) // NB == nb and dim - NB * (nb - 1) == need, "the window is meant to end %d columns into panel %d" % (need, nb)
    glog, gp, gx = alone[spec]
    op, ox, olog = oracle.ba_optimize(pr["poses"], pr["fixed"], pr["points"], oracle.ba_obs(pr), pr["cam"], True, ITERS)
    assert len(glog) == len(olog)
    assert np.allclose(glog["chi2_before"], olog["chi2_before"], rtol=CHI_RTOL)
    assert np.allclose(glog["chi2_after"], olog["chi2_after"], rtol=CHI_RTOL)
    assert np.array_equal(glog["trials"], olog["trials"]) and np.array_equal(glog["status"], olog["status"])
    assert np.allclose(glog["lambda"], olog["lambda"], rtol=1e-6)
    assert rot_err(gp[:, :4], op[:, :4]).max() < ROT_TOL and np.abs(gp[:, 4:] - op[:, 4:]).max() < TRANS_TOL
    assert np.abs(gx - ox).max() < TRANS_TOL


def test_batch_gives_the_bytes_of_every_window_alone(hiplib, ctx, problems, alone):
    """All seven windows in one batch: the chain is as long as the largest system's, the small ones may take k_chol_wg."""
    batch = [_make(hiplib, ctx, problems[spec]) for spec, _, _ in CASES]
    logs = hiplib.ba_optimize_batch(batch, True, ITERS)
    for (spec, _, _), b, log in zip(CASES, batch, logs):
        wl, wp, wx = alone[spec]
        bp, bx = b.state()
        assert log.tobytes() == wl.tobytes() and bp.tobytes() == wp.tobytes() and bx.tobytes() == wx.tobytes(), spec
    for b in batch:
        b.close()


@pytest.mark.parametrize("spec", [CASES[3][0], CASES[5][0]], ids=["10kf", "16kf"])
def test_second_solve_gives_the_same_bytes(hiplib, ctx, problems, alone, spec):
    """The scratch behind the panel blocks holds the previous panel's product when the next one starts."""
    ba = _make(hiplib, ctx, problems[spec])
    ba.optimize(True, ITERS)
    ba.reset()
    log = ba.optimize(True, ITERS)
    p, x = ba.state()
    wl, wp, wx = alone[spec]
    assert log.tobytes() == wl.tobytes() and p.tobytes() == wp.tobytes() and x.tobytes() == wx.tobytes()
    ba.close()
