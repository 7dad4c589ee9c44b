"""lpslam_sim3_ransac_batch_host (lpslam_amd/host/sim3_batch.cpp), the CPU definition the device call
lpslam_hip_sim3_ransac_batch is held to: set by set it is LpSlam::sim3_solve_ransac, byte for byte, with what the single solver leaves
open when it finds nothing fixed (count 0, best_iteration -1, flags cleared, s12 = 1 0 0 0 0 0 0 1); the winning iteration it reports
is the one a numpy replay of the sample table finds; and the solver alone recovers every planted set the GPU tests use, so those never
compare two failures.  No device."""
import numpy as np
import pytest

import sim3_batch_cases as SC
from lpslam_amd import hip


def _expect_single(pairs, fix_scale, iterations, seed):
    got, s12, inl = SC.solve_single(pairs, fix_scale, iterations, seed)
    if got == 0:
        return 0, SC.NONE_S12, np.zeros(len(pairs), np.uint8)
    return got, s12, inl


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("iterations", [1, 200])
@pytest.mark.parametrize("seed", SC.SEEDS)
def test_batch_equals_the_single_solver_set_by_set(seed, iterations, fix_scale):
    """n = 3, 4, 37 and 300 with the edge sets in the middle of the batch: two pairs, none, all pairs on one point"""
    sets = [SC.planted(3, 1)[0], SC.planted(2, 2)[0], SC.planted(4, 3)[0], SC.planted(0, 4)[0], SC.planted(37, 5, 0.3)[0], SC.coincident(), SC.planted(300, 6, 0.5)[0]]
    s12, cnt, inl, best = hip.sim3_ransac_batch_host(sets, SC.CAM, SC.CAM, fix_scale, iterations, seed)
    for i, p in enumerate(sets):
        want = _expect_single(p, fix_scale, iterations, seed)
        assert cnt[i] == want[0] and s12[i].tobytes() == want[1].tobytes() and np.array_equal(inl[i], want[2]), i
        assert (best[i] == -1) == (cnt[i] == 0) and best[i] < iterations
    # nothing found: fewer than three pairs, and -- with a free scale -- the set whose every sample Horn refuses
    for i in (1, 3) + (() if fix_scale else (5,)):
        assert cnt[i] == 0 and best[i] == -1 and not inl[i].any() and s12[i].tobytes() == SC.NONE_S12.tobytes()
    # without the iteration asked for, and from a pair_start that does not begin at 0: the same
    again = hip.sim3_ransac_batch_host(sets, SC.CAM, SC.CAM, fix_scale, iterations, seed, want_iteration=False, first=5)
    assert SC.same((s12, cnt, inl, None), again)


def test_refusals_write_nothing():
    import ctypes as C
    f = hip.host_lib().lpslam_sim3_ransac_batch_host
    f.argtypes = hip._SIM3_RANSAC_ARGS; f.restype = C.c_int
    pairs = SC.planted(5, 9)[0]
    s12 = np.full(8, 7.0); cnt = np.full(1, 7, np.int32); inl = np.full(5, 7, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = np.array([0, 5], np.int32); cam = SC.CAM.copy(); nan_cam = cam.copy(); nan_cam[1] = np.nan
    for n_sets, start, c1, iterations in ((-1, ok, cam, 10), (1, np.array([5, 0], np.int32), cam, 10), (1, np.array([-1, 4], np.int32), cam, 10), (1, ok, cam, 0), (1, ok, nan_cam, 10)):
        assert f(n_sets, p(pairs), p(start), p(c1), p(cam), 1, iterations, 1, p(s12), p(cnt), p(inl), None) == 1
        assert (s12 == 7.0).all() and cnt[0] == 7 and (inl == 7).all()
    assert f(1, p(pairs), p(ok), p(cam), p(cam), 1, 10, 1, p(s12), None, p(inl), None) == 1 and (s12 == 7.0).all()
    assert f(0, None, p(ok), p(cam), p(cam), 1, 10, 1, None, None, None, None) == 0


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("n,bad,seed,iterations", [(4, 0.0, 0, 200), (37, 0.3, 0x9E3779B9, 200), (300, 0.5, 0, 200), (37, 0.3, 0, 1)])
def test_winning_iteration_is_the_replay_of_the_sample_table(n, bad, seed, iterations, fix_scale):
    """The table (lpslam_sim3_sample_table) through the oracle's Horn and the solver's scoring rule in numpy: the first iteration with
    the largest count is the one the batch form reports, with that count."""
    from oracle import two_view as TV
    p, _ = SC.planted(n, 60 + n, bad, scale=1.0 if fix_scale else 1.07)
    _, cnt, _, best = hip.sim3_ransac_batch_host([p], SC.CAM, SC.CAM, fix_scale, iterations, seed)
    table = hip.sim3_sample_table(n, iterations, seed)
    assert table.shape == (iterations, 3) and (np.sort(table, 1)[:, 1:] != np.sort(table, 1)[:, :-1]).all() and table.min() >= 0 and table.max() < n
    top, top_it = 0, -1
    for it, idx in enumerate(table):
        h = TV.horn(p["p1c"][idx], p["p2c"][idx], bool(fix_scale))
        if h is None:
            continue
        r, t, s = h
        q1 = s * (p["p2c"] @ r.T) + t
        q2 = ((p["p1c"] - t) @ r) / s
        e1 = np.stack([SC.CAM[0] * q1[:, 0] / q1[:, 2] + SC.CAM[2], SC.CAM[1] * q1[:, 1] / q1[:, 2] + SC.CAM[3]], 1) - p["obs1"]
        e2 = np.stack([SC.CAM[0] * q2[:, 0] / q2[:, 2] + SC.CAM[2], SC.CAM[1] * q2[:, 1] / q2[:, 2] + SC.CAM[3]], 1) - p["obs2"]
        c = int(((q1[:, 2] > 0) & (q2[:, 2] > 0) & ((e1 * e1).sum(1) * p["inv_sigma2_1"] < 9.210) & ((e2 * e2).sum(1) * p["inv_sigma2_2"] < 9.210)).sum())
        if c > top:
            top, top_it = c, it
    assert (top_it, top) == (int(best[0]), int(cnt[0]))


@pytest.mark.parametrize("fix_scale", [0, 1])
def test_the_host_solver_recovers_every_planted_set_of_the_gpu_tests(fix_scale):
    """count >= planted inliers - 2 at the tracker's parameters (200 iterations, both seeds): the GPU tests compare successes"""
    for sets, want in (SC.edge_batch(), SC.tracker_batch()):
        for seed in SC.SEEDS:
            _, cnt, _, best = hip.sim3_ransac_batch_host(sets, SC.CAM, SC.CAM, fix_scale, 200, seed)
            for i, good in enumerate(want):
                if good is not None:
                    assert cnt[i] >= good - 2 and best[i] >= 0, (i, seed, int(cnt[i]), good)
    for case in range(20):
        _, cnt, _, best = hip.sim3_ransac_batch_host([SC.exact6(case)], SC.CAM, SC.CAM, fix_scale, 200, case)
        assert cnt[0] == 6 and best[0] >= 0
