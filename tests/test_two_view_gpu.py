"""lpslam_hip_two_view_ransac_batch and lpslam_hip_two_view_check_poses (csrc/two_view.hip) against their CPU
definitions lpslam_two_view_ransac_batch_host / lpslam_two_view_check_poses_host -- steps 1 and 4 of LpSlam::two_view_initialize -- on
the same inputs.  [UPSTREAM] initialize::perspective.  Iterations, score bits, matrices, flags, codes, points and cosines are compared
exactly: the kernels run the text of csrc/two_view_math.h that the host runs, both sides without FMA contraction, FP64 + - * / sqrt
round correctly on both, and the score is added in the host's order."""
import ctypes as C

import numpy as np
import pytest

import two_view_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    from lpslam_amd import _build
    _build.host_library()
    c = hiplib.Context(640, 480, max_keypoints=500, num_levels=2, max_images=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches():
    return T.batches()


@pytest.fixture(scope="module")
def reference(hiplib, batches):
    """(batch, iterations) -> the host's answer, computed once"""
    cache = {}

    def get(name, iterations):
        if (name, iterations) not in cache:
            off, p1, p2 = T.concat(batches[name])
            cache[(name, iterations)] = hiplib.two_view_ransac_batch_host(off, p1, p2, 1.0, iterations, T.SEED)
        return cache[(name, iterations)]
    return get


def _same(got, want):
    best, score, model, fh, ff = got
    wbest, wscore, wmodel, wfh, wff = want
    assert np.array_equal(best, wbest), (best, wbest)
    assert score.tobytes() == wscore.tobytes(), (score, wscore)
    assert model.tobytes() == wmodel.tobytes(), np.abs(model - wmodel).max()
    assert np.array_equal(fh, wfh) and np.array_equal(ff, wff)


@pytest.mark.parametrize("iterations", [1, 7, 100])
@pytest.mark.parametrize("name", ["S1", "S8", "S11"])
def test_batch_equals_the_host_loop(hiplib, ctx, batches, reference, name, iterations):
    sets = batches[name]
    off, p1, p2 = T.concat(sets)
    got = hiplib.two_view_ransac_batch(ctx, off, p1, p2, 1.0, iterations, T.SEED)
    _same(got, reference(name, iterations))
    best, score, model, fh, ff = got
    for i, s in enumerate(sets):
        n = len(s["p1"])
        if n < 8 or (name == "S11" and i == 4):                 # too few matches / the one-point set: none, the neighbours undisturbed
            assert (best[i] == -1).all() and (score[i] == 0).all() and not model[i].any() and not fh[off[i]:off[i + 1]].any() and not ff[off[i]:off[i + 1]].any()
        elif n >= 9 and not (name == "S11" and i == 5):
            assert (best[i] >= 0).any() and (score[i] > 0).any(), i
    if name == "S11" and iterations == 100:                     # the planar and the rotation scene: the homography explains them, by the rule of the model choice
        for i in (6, 7):
            assert score[i, 0] / (score[i, 0] + score[i, 1]) > 0.40, (i, score[i])
        assert score[0, 0] / (score[0, 0] + score[0, 1]) <= 0.40          # and a general scene not


def test_no_sets_is_ok_and_does_nothing(hiplib, ctx):
    best, score, model, fh, ff = hiplib.two_view_ransac_batch(ctx, np.zeros(1, np.int32), np.zeros((0, 2)), np.zeros((0, 2)))
    assert len(best) == 0 and len(score) == 0 and len(model) == 0 and len(fh) == 0 and len(ff) == 0


def test_sigma_and_seed_reach_the_kernels(hiplib, ctx, batches):
    off, p1, p2 = T.concat(batches["S8"])
    for sigma, seed in ((1.5, 0), (0.7, 1), (2.0, 77)):
        _same(hiplib.two_view_ransac_batch(ctx, off, p1, p2, sigma, 30, seed), hiplib.two_view_ransac_batch_host(off, p1, p2, sigma, 30, seed))
    # offsets that do not start at 0
    _same(hiplib.two_view_ransac_batch(ctx, off[5:], p1, p2, 1.0, 30, 5), hiplib.two_view_ransac_batch_host(off[5:], p1, p2, 1.0, 30, 5))


def test_the_same_call_twice_gives_the_same_bytes(hiplib, ctx, batches):
    off, p1, p2 = T.concat(batches["S8"])
    a = hiplib.two_view_ransac_batch(ctx, off, p1, p2, 1.0, 100, T.SEED)
    b = hiplib.two_view_ransac_batch(ctx, off, p1, p2, 1.0, 100, T.SEED)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_refusals_write_nothing_and_leave_the_context_usable(hiplib, ctx, batches, reference):
    off, p1, p2 = T.concat(batches["S1"])
    n = len(p1)
    f = ctx.lib.lpslam_hip_two_view_ransac_batch
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_uint32] + [C.c_void_p] * 5
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    best = np.full(2, 55, np.int32); score = np.full(2, 7.5); model = np.full(18, 7.5); fh = np.full(n, 9, np.uint8); ff = np.full(n, 9, np.uint8)
    two = np.array([0, 100, 50], np.int32)

    def call(n_sets=1, offsets=off, sigma=1.0, iterations=100, q1=p1, out_model=model, out_ff=ff):
        return f(ctx.h, n_sets, p(offsets), p(q1), p(p2), sigma, iterations, T.SEED, p(best), p(score), p(out_model), p(fh), p(out_ff))
    for kw in (dict(n_sets=-1), dict(n_sets=2, offsets=two), dict(offsets=np.array([-1, 20], np.int32)), dict(iterations=0), dict(iterations=-3),
               dict(iterations=hiplib.TWO_VIEW_MAX_ITERATIONS + 1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
               dict(offsets=None), dict(q1=None), dict(out_model=None), dict(out_ff=None)):
        assert call(**kw) != 0, kw
        assert ctx.lib.lpslam_hip_last_error().decode() != ""
        assert (best == 55).all() and (score == 7.5).all() and (model == 7.5).all() and (fh == 9).all() and (ff == 9).all(), kw
    assert call() == 0                                                   # a valid call right after
    wbest, wscore, wmodel, wfh, wff = reference("S1", 100)
    assert np.array_equal(best, wbest[0]) and score.tobytes() == wscore[0].tobytes() and model.tobytes() == wmodel[0].tobytes()
    assert np.array_equal(fh, wfh) and np.array_equal(ff, wff)
    # the cap itself is accepted
    _same(hiplib.two_view_ransac_batch(ctx, off, p1, p2, 1.0, hiplib.TWO_VIEW_MAX_ITERATIONS, 3),
          hiplib.two_view_ransac_batch_host(off, p1, p2, 1.0, hiplib.TWO_VIEW_MAX_ITERATIONS, 3))


def _hypotheses(P, s):
    """P motions: the planted one, the planted one with t reversed (every depth negative), then wrong ones"""
    t = s["t"] / np.linalg.norm(s["t"])
    R = [s["R"], s["R"]] + [T.rot([0.3 * k, 1.0, -0.2], 0.05 * k) @ s["R"] for k in range(1, 7)]
    ts = [t, -t] + [T.rot([1.0, 0.1 * k, 0.4], 0.4 * k) @ t for k in range(1, 7)]
    if P == 1:
        return np.stack(R[1:2]), np.stack(ts[1:2])                       # the reversed one alone
    return np.stack(R[:P]), np.stack(ts[:P])


@pytest.mark.parametrize("flags", ["all", "none", "alternating"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("P", [1, 4, 8])
def test_check_poses_equals_the_host_check(hiplib, ctx, P, n, flags):
    s = T.general(300, 2)
    p1, p2 = s["p1"][:n], s["p2"][:n]
    fl = dict(all=np.ones(n, np.uint8), none=np.zeros(n, np.uint8), alternating=(np.arange(n) % 2).astype(np.uint8))[flags]
    R, t = _hypotheses(P, s)
    X, cosp, code = hiplib.two_view_check_poses(ctx, R, t, T.K, p1, p2, fl, 4.0)
    wX, wcosp, wcode = hiplib.two_view_check_poses_host(R, t, T.K, p1, p2, fl, 4.0)
    assert X.shape == (P, n, 3) and np.array_equal(code, wcode)
    assert X.tobytes() == wX.tobytes() and cosp.tobytes() == wcosp.tobytes()          # bits, NaN included
    assert not code[:, fl == 0].any() and np.isnan(X[code == 0]).all()
    reversed_t = 0 if P == 1 else 1
    assert not code[reversed_t].any()                                    # every depth negative, parallax of degrees: nothing is plausible
    if P > 1 and flags == "all" and n >= 63:
        assert (code[0] == 2).sum() > 0.9 * n                            # the planted motion explains the matches


def test_check_poses_refusals_and_empty_calls(hiplib, ctx):
    s = T.general(64, 2)
    R, t = _hypotheses(4, s)
    fl = np.ones(64, np.uint8)
    f = ctx.lib.lpslam_hip_two_view_check_poses
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    X = np.full((9, 64, 3), 7.5); cosp = np.full((9, 64), 7.5); code = np.full((9, 64), 9, np.uint8)
    R9 = np.ascontiguousarray(np.tile(np.eye(3), (9, 1, 1))); t9 = np.zeros((9, 3))
    Rc, tc = np.ascontiguousarray(R), np.ascontiguousarray(t)

    def call(P=4, n=64, Rm=Rc, K=T.K, out=X):
        return f(ctx.h, P, p(Rm), p(tc if P <= 4 else t9), p(K), n, p(s["p1"]), p(s["p2"]), p(fl), 4.0, p(out), p(cosp), p(code))
    for kw in (dict(P=9, Rm=R9), dict(P=-1), dict(n=-1), dict(Rm=None), dict(K=None), dict(out=None)):
        assert call(**kw) != 0, kw
        assert (X == 7.5).all() and (cosp == 7.5).all() and (code == 9).all(), kw
    assert call(P=0) == 0 and call(n=0) == 0 and (X == 7.5).all() and (code == 9).all()
    assert call() == 0
    wX, wcosp, wcode = hiplib.two_view_check_poses_host(R, t, T.K, s["p1"], s["p2"], fl, 4.0)
    assert X[:4].tobytes() == wX.tobytes() and np.array_equal(code[:4], wcode) and (X[4:] == 7.5).all()
