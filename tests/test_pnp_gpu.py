"""lpslam_hip_pnp_ransac_batch (csrc/pnp.hip) against its CPU definition lpslam_pnp_ransac_batch_host -- the
relocaliser's LpSlam::pnp_solve_ransac on each set -- on the same inputs.  [UPSTREAM] solve::pnp_solver.  Counts, flags, the winning
sample and pose7 are compared exactly: the kernels run the operations of the host solver in its order, both sides without FMA
contraction, and FP64 + - * / sqrt round correctly on both (the equality held in every case of this file on the MI355X)."""
import ctypes as C

import numpy as np
import pytest

import pnp_cases as P

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
    return P.batches()


@pytest.fixture(scope="module")
def reference(hiplib, batches):
    """(batch, iterations) -> the host's answer, computed once"""
    cache = {}

    def get(name, iterations):
        if (name, iterations) not in cache:
            off, pw, obs, w = P.concat(batches[name])
            cache[(name, iterations)] = hiplib.pnp_ransac_batch_host(off, pw, obs, w, P.CAM, iterations, P.SEED)
        return cache[(name, iterations)]
    return get


def _same(got, want):
    pose, cnt, fl, best = got
    wpose, wcnt, wfl, wbest = want
    assert np.array_equal(cnt, wcnt), (cnt, wcnt)
    assert np.array_equal(best, wbest), (best, wbest)
    assert np.array_equal(fl, wfl)
    assert pose.tobytes() == wpose.tobytes(), np.abs(pose - wpose).max()


@pytest.mark.parametrize("iterations", [1, 7, 100])
@pytest.mark.parametrize("name", ["S1", "S8", "S11"])
def test_batch_equals_the_host_solver(hiplib, ctx, batches, reference, name, iterations):
    sets = batches[name]
    off, pw, obs, w = P.concat(sets)
    got = hiplib.pnp_ransac_batch(ctx, off, pw, obs, w, P.CAM, iterations, P.SEED)
    _same(got, reference(name, iterations))
    pose, cnt, fl, best = got
    for i, s in enumerate(sets):
        n = len(s["w"])
        if n < 4 or (name == "S11" and i == 5):                 # too few matches / the coplanar set: nothing found, the neighbours undisturbed
            assert cnt[i] == 0 and best[i] == -1 and not fl[off[i]:off[i + 1]].any() and np.array_equal(pose[i], [1, 0, 0, 0, 0, 0, 0])
        elif iterations == 100:
            # the condition: the planted inliers exactly, and a pose as good as the host solver's on this set (tests/test_pnp_cpu.py
            # checks that the host solver alone recovers these sets)
            assert np.array_equal(fl[off[i]:off[i + 1]].astype(bool), ~s["bad"]), i
            if n >= 15:
                host_pose = reference(name, iterations)[0][i]
                assert P.pose_error(pose[i], s) <= P.pose_error(host_pose, s)


def test_no_sets_is_ok_and_does_nothing(hiplib, ctx):
    pose, cnt, fl, best = hiplib.pnp_ransac_batch(ctx, np.zeros(1, np.int32), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0), P.CAM, 100, P.SEED)
    assert len(pose) == 0 and len(cnt) == 0 and len(fl) == 0


def test_planted_ties_go_to_the_lowest_iteration(hiplib, ctx):
    """six exact matches: many of the 100 samples explain all six, the first of them must win, as the host's `count > best` has it"""
    s = P.planted(6, 0.0, 11)
    off, pw, obs, w = P.concat([s, s])
    tied = 0
    for seed in range(1, 21):
        want = hiplib.pnp_ransac_batch_host(off, pw, obs, w, P.CAM, 100, seed)
        _same(hiplib.pnp_ransac_batch(ctx, off, pw, obs, w, P.CAM, 100, seed), want)
        assert want[3][0] == want[3][1]                                   # the same seed for every set
        # (how many samples reach the winner's count: the case is only a tie test where there are several)
        table = hiplib.pnp_sample_table(6, 100, seed)
        reach = 0
        for row in table:
            h = hiplib.epnp4_host(s["pw"][row], s["obs"][row], P.CAM)
            if h is None:
                continue
            xc = s["pw"] @ h[0].T + h[1]
            e = np.column_stack([P.CAM[0] * xc[:, 0] / xc[:, 2] + P.CAM[2], P.CAM[1] * xc[:, 1] / xc[:, 2] + P.CAM[3]]) - s["obs"]
            reach += int(((xc[:, 2] > 0) & ((e * e).sum(1) * s["w"] < 5.991)).sum() == 6)
        tied += reach >= 2
    assert tied >= 15, tied


def test_the_same_call_twice_gives_the_same_bytes(hiplib, ctx, batches):
    off, pw, obs, w = P.concat(batches["S8"])
    a = hiplib.pnp_ransac_batch(ctx, off, pw, obs, w, P.CAM, 100, P.SEED)
    b = hiplib.pnp_ransac_batch(ctx, off, pw, obs, w, P.CAM, 100, P.SEED)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_refusals_write_nothing_and_leave_the_context_usable(hiplib, ctx, batches, reference):
    off, pw, obs, w = P.concat(batches["S1"])
    f = ctx.lib.lpslam_hip_pnp_ransac_batch
    f.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_uint32] + [C.c_void_p] * 4
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pose = np.full(7, 7.5); cnt = np.full(1, 77, np.int32); fl = np.full(len(w), 9, np.uint8); best = np.full(1, 55, np.int32)
    two = np.array([0, 100, 50], np.int32)

    def call(n_sets=1, offsets=off, iterations=100, pose7=pose):
        return f(ctx.h, n_sets, p(offsets), p(pw), p(obs), p(w), p(P.CAM), iterations, P.SEED, None if pose7 is None else p(pose7), p(cnt), p(fl), p(best))
    for kw in (dict(n_sets=2, offsets=two), dict(iterations=0), dict(pose7=None), dict(iterations=hiplib.PNP_MAX_ITERATIONS + 1), dict(n_sets=-1)):
        assert call(**kw) != 0, kw
        assert ctx.lib.lpslam_hip_last_error().decode() != ""
        assert (pose == 7.5).all() and cnt[0] == 77 and (fl == 9).all() and best[0] == 55, kw
    assert call() == 0                                                   # a valid call right after
    wpose, wcnt, wfl, wbest = reference("S1", 100)
    assert pose.tobytes() == wpose[0].tobytes() and cnt[0] == wcnt[0] and np.array_equal(fl, wfl) and best[0] == wbest[0]
    # the cap itself is accepted
    _same(hiplib.pnp_ransac_batch(ctx, off, pw, obs, w, P.CAM, hiplib.PNP_MAX_ITERATIONS, 3),
          hiplib.pnp_ransac_batch_host(off, pw, obs, w, P.CAM, hiplib.PNP_MAX_ITERATIONS, 3))
