"""The local window's dense solve where its last panel column is cut short (chol_panel_trim, csrc/ba.hip) and the window's
begin / end hand-over.  Tolerances are those of test_ba_gpu.py: chi2 trajectory relative 1e-9, identical trials / status,
lambda relative 1e-6, poses within 1e-4 rad / 1e-3 m of the CPU oracle."""
import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL, CHI_RTOL = 1e-4, 1e-3, 1e-9
NB = 32                                                     # panel width of the dense factorisation


def rot_err(q1, q2):
    return 2 * np.arccos(np.clip(np.abs(np.sum(q1 * q2, axis=1)), 0, 1))


@pytest.fixture(scope="module")
def ctx(hiplib):
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


def _make(hiplib, ctx, pr):
    return hiplib.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hiplib.ba_obs_array(pr), pr["cam"])


def _against_oracle(oracle, pr, robust, iters, glog, gp, gx):
    op, ox, olog = oracle.ba_optimize(pr["poses"], pr["fixed"], pr["points"], oracle.ba_obs(pr), pr["cam"], robust, iters)
    assert len(glog) == len(olog)
    assert np.allclose(glog["chi2_before"], olog["chi2_before"], rtol=CHI_RTOL)
    assert np.allclose(glog["chi2_after"], olog["chi2_after"], rtol=CHI_RTOL)
    assert np.array_equal(glog["trials"], olog["trials"]) and np.array_equal(glog["status"], olog["status"])
    assert np.allclose(glog["lambda"], olog["lambda"], rtol=1e-6)
    assert rot_err(gp[:, :4], op[:, :4]).max() < ROT_TOL and np.abs(gp[:, 4:] - op[:, 4:]).max() < TRANS_TOL
    assert np.abs(gx - ox).max() < TRANS_TOL
    return olog


# (n_kf, n_pts, n_obs) -> panels, real columns of the last panel column; one keyframe of a synthetic window is fixed
PANEL_CASES = [((2, 60, 120), 1, 6),          # one panel, 6 real columns
               ((4, 150, 450), 1, 18),        # strip B in part
               ((6, 150, 700), 1, 30),
               ((7, 150, 800), 2, 4),         # two panels, the trimmed one is the second of the pair
               ((9, 150, 1000), 2, 16),       # exactly one strip: the block product and strip B are skipped
               ((12, 150, 1200), 3, 2),       # odd panel count: the last launch factors one column
               ((17, 150, 1500), 4, 0)]       # dim = 96: the last panel column holds the rhs row and padding only


@pytest.fixture(scope="module")
def panel_problems():
    return {spec: synth.ba_problem(*spec, 640, 480, seq_id=spec[0]) for spec, _, _ in PANEL_CASES}


@pytest.mark.parametrize("spec,nb,need", PANEL_CASES, ids=["%dkf" % c[0][0] for c in PANEL_CASES])
def test_last_panel_boundaries(hiplib, oracle, ctx, panel_problems, spec, nb, need):
    pr = panel_problems[spec]
    dim = 6 * int((pr["fixed"] == 0).sum())
    assert (dim + 1 + NB - 1) // NB == nb and dim - NB * (nb - 1) == need, "the window is meant to end %d columns into panel %d" % (need, nb)
    iters = 8
    ba = _make(hiplib, ctx, pr)
    ba.set_solver("dense")
    glog = ba.optimize(True, iters)
    gp, gx = ba.state()
    olog = _against_oracle(oracle, pr, True, iters, glog, gp, gx)
    assert olog["trials"].max() == 1 and not olog["status"].any()
    # the same window inside a batch of three different sizes (the batch's chain is as long as its largest system's)
    others = [s for s, _, _ in PANEL_CASES if s != spec]
    mates = [panel_problems[others[0]], panel_problems[others[-1]]]
    batch = [_make(hiplib, ctx, mates[0]), _make(hiplib, ctx, pr), _make(hiplib, ctx, mates[1])]
    for b in batch:
        b.set_solver("dense")
    logs = hiplib.ba_optimize_batch(batch, True, iters)
    bp, bx = batch[1].state()
    assert logs[1].tobytes() == glog.tobytes() and bp.tobytes() == gp.tobytes() and bx.tobytes() == gx.tobytes()
    for b in batch + [ba]:
        b.close()


def test_rejected_trials_through_begin_and_end(hiplib, oracle):
    """A window whose fifth iteration rejects trials, solved in two halves on one stream signature until the launch graph is
    replayed: every round gives the bytes of the first, directly launched one, and follows the oracle."""
    pr = synth.ba_problem(6, 150, 800, 640, 480, seq_id=46, pose_noise=(0.5, 3.0), point_noise=3.0)
    own = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)
    ba = _make(hiplib, own, pr)
    before = own.ba_counters()["replays"]
    rounds = []
    for _ in range(4):
        ba.reset()
        ba.optimize_begin(True, 10)
        log = ba.optimize_end()
        rounds.append((log,) + ba.state())
    assert own.ba_counters()["replays"] - before >= 2, "the later rounds were meant to replay the captured graph"
    first = rounds[0]
    assert first[0]["trials"].max() > 1
    _against_oracle(oracle, pr, True, 10, *first)
    for log, p, x in rounds[1:]:
        assert log.tobytes() == first[0].tobytes() and p.tobytes() == first[1].tobytes() and x.tobytes() == first[2].tobytes()
    ba.close(); own.close()


def test_pipelined_windows_equal_plain_solves(hiplib):
    """The mapping thread's pattern: window k + 1 is created beside the solve of window k, receives its values and starts once k
    has ended, then k is read back and released.  Every window gives the bytes of a plain optimize() on a fresh problem."""
    probs = [synth.ba_problem(8, 300, 2400, 640, 480, seq_id=60 + i) for i in range(6)]
    iters = 10
    ref = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)
    want = []
    for pr in probs:
        b = _make(hiplib, ref, pr)
        want.append((b.optimize(True, iters),) + b.state())
        b.close()
    own = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)

    def start(b, pr):
        b.set_state(pr["poses"], pr["points"])
        b.optimize_begin(True, iters)
    cur = _make(hiplib, own, probs[0])
    start(cur, probs[0])
    got = []
    for i in range(len(probs)):
        nxt = _make(hiplib, own, probs[i + 1]) if i + 1 < len(probs) else None
        log = cur.optimize_end()
        if nxt is not None:
            start(nxt, probs[i + 1])
        got.append((log,) + cur.state())
        cur.close()
        cur = nxt
    for (gl, gp, gx), (wl, wp, wx) in zip(got, want):
        assert gl.tobytes() == wl.tobytes() and gp.tobytes() == wp.tobytes() and gx.tobytes() == wx.tobytes()
    ref.close(); own.close()
