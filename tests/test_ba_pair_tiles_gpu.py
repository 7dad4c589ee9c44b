"""The tile schedule of the panel-pair launch (k_chol_pair): lookahead and second-column products run left halves
first, the factoring wavefronts start strip A on them and take the right halves behind an announcement in LDS (chol_panel_split),
the tiles nobody reads are not computed and the first column's blocks leave for memory beside the second column's panel.  None of
it may change a bit: every tile keeps its own chain of matrix instructions.

Small dense windows with random tracks at the sizes where the schedule takes another path.  The reduced system has six columns per
free keyframe (one keyframe of a synthetic window is fixed) plus the rhs row:

    free  nb  launches                               real columns of the last panel column
      3    1  `single`, no previous pair             18   stops in strip B
      6    2  pair, no previous pair                  4   step-3 split only, ends in strip A
      8    2  pair, no previous pair                 16   exactly strip A
      9    2  pair, no previous pair                 22   strip B
     11    3  pair, `single` WITH a previous pair     2
     16    4  two pairs                               0   the last column holds the rhs row alone
     17    4  two pairs                               6
     19    4  two pairs                              18
     22    5  pair, pair, `single` with previous      4

Three LM iterations each; the seeds are such that the CPU oracle accepts every trial, so three iterations are three units.
Tolerances against the oracle are those of test_ba_window_gpu.py: chi2 trajectory relative 1e-9, identical trials / status, lambda
relative 1e-6, poses within 1e-4 rad / 1e-3 m, points within 1e-3 m.  A window alone, inside one ba_optimize_batch of all nine and
solved a second time gives the same bytes, and the bytes are those the parent commit's library gave for the same inputs on an
MI355X (tests/golden/pair_tiles/, written by tools/dev/pair_tiles_golden.py)."""
import os

import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL, CHI_RTOL = 1e-4, 1e-3, 1e-9
NB = 32                                                     # panel width of the dense factorisation
ITERS = 3
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_tiles")

# free keyframes -> panels, real columns of the last panel column
CASES = [(3, 1, 18), (6, 2, 4), (8, 2, 16), (9, 2, 22), (11, 3, 2), (16, 4, 0), (17, 4, 6), (19, 4, 18), (22, 5, 4)]
IDS = ["%dfree" % c[0] for c in CASES]


def window(free):
    """The synthetic window with `free` free keyframes (the generator of the stored arrays builds the same)."""
    n_kf = free + 1
    return synth.ba_problem(n_kf, 150 if n_kf < 20 else 300, 110 * n_kf, 640, 480, seq_id=300 + free)


def rot_err(q1, q2):
    return 2 * np.arccos(np.clip(np.abs(np.sum(q1 * q2, axis=1)), 0, 1))


def make(hiplib, ctx, pr):
    ba = hiplib.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hiplib.ba_obs_array(pr), pr["cam"])
    ba.set_solver("dense")
    return ba


@pytest.fixture(scope="module")
def ctx(hiplib):
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


@pytest.fixture(scope="module")
def problems():
    return {free: window(free) for free, _, _ in CASES}


@pytest.fixture(scope="module")
def alone(hiplib, ctx, problems):
    """Every window solved once on its own: (log, poses, points)."""
    out = {}
    for free, pr in problems.items():
        ba = make(hiplib, ctx, pr)
        out[free] = (ba.optimize(True, ITERS),) + ba.state()
        ba.close()
    return out


@pytest.mark.parametrize("free,nb,need", CASES, ids=IDS)
def test_against_oracle(oracle, problems, alone, free, nb, need):
    pr = problems[free]
    dim = 6 * int((pr["fixed"] == 0).sum())
    assert dim == 6 * free and (dim + 1 + NB - 1) // NB == nb and dim - NB * (nb - 1) == need
    glog, gp, gx = alone[free]
    op, ox, olog = oracle.ba_optimize(pr["poses"], pr["fixed"], pr["points"], oracle.ba_obs(pr), pr["cam"], True, ITERS)
    assert len(olog) == ITERS and np.all(olog["trials"] == 1), "the seed is meant to give three accepted trials"
    assert len(glog) == len(olog)
    assert np.allclose(glog["chi2_before"], olog["chi2_before"], rtol=CHI_RTOL)
    assert np.allclose(glog["chi2_after"], olog["chi2_after"], rtol=CHI_RTOL)
    assert np.array_equal(glog["trials"], olog["trials"]) and np.array_equal(glog["status"], olog["status"])
    assert np.allclose(glog["lambda"], olog["lambda"], rtol=1e-6)
    assert rot_err(gp[:, :4], op[:, :4]).max() < ROT_TOL and np.abs(gp[:, 4:] - op[:, 4:]).max() < TRANS_TOL
    assert np.abs(gx - ox).max() < TRANS_TOL


@pytest.mark.parametrize("free", [c[0] for c in CASES], ids=IDS)
def test_bytes_of_the_parent_commit(alone, free):
    _, gp, gx = alone[free]
    pp = np.load(os.path.join(GOLDEN_DIR, "poses_%d.npy" % free))
    px = np.load(os.path.join(GOLDEN_DIR, "points_%d.npy" % free))
    assert gp.dtype == pp.dtype and gp.shape == pp.shape and gp.tobytes() == pp.tobytes()
    assert gx.dtype == px.dtype and gx.shape == px.shape and gx.tobytes() == px.tobytes()


def test_batch_gives_the_bytes_of_every_window_alone(hiplib, ctx, problems, alone):
    batch = [make(hiplib, ctx, problems[free]) for free, _, _ in CASES]
    logs = hiplib.ba_optimize_batch(batch, True, ITERS)
    for (free, _, _), b, log in zip(CASES, batch, logs):
        wl, wp, wx = alone[free]
        bp, bx = b.state()
        assert log.tobytes() == wl.tobytes() and bp.tobytes() == wp.tobytes() and bx.tobytes() == wx.tobytes(), free
    for b in batch:
        b.close()


@pytest.mark.parametrize("free", [c[0] for c in CASES], ids=IDS)
def test_second_solve_gives_the_same_bytes(hiplib, ctx, problems, alone, free):
    """The announcement counters and the scratch behind the panel blocks hold the previous launch's values when the next one starts."""
    ba = make(hiplib, ctx, problems[free])
    ba.optimize(True, ITERS)
    ba.reset()
    log = ba.optimize(True, ITERS)
    p, x = ba.state()
    wl, wp, wx = alone[free]
    assert log.tobytes() == wl.tobytes() and p.tobytes() == wp.tobytes() and x.tobytes() == wx.tobytes()
    ba.close()
