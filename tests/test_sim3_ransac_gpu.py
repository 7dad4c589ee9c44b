"""lpslam_hip_sim3_ransac_batch (lpslam_amd/csrc/sim3.hip) against its CPU definition
lpslam_sim3_ransac_batch_host, exactly: the counts, the winning iterations, all eight doubles of s12 and the per-pair flags of every
set.  Both sides run the same FP64 text (csrc/sim3_math.h, horn of csrc/epnp_math.h) without contraction, so there is no tolerance.
tests/test_sim3_batch_cpu.py shows that the host solver recovers the planted sets used here."""
import ctypes as C

import numpy as np
import pytest

import sim3_batch_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


def _both(hiplib, ctx, sets, fix_scale, iterations, seed, **kw):
    dev = hiplib.sim3_ransac_batch(ctx, sets, SC.CAM, SC.CAM, fix_scale, iterations, seed, **kw)
    host = hiplib.sim3_ransac_batch_host(sets, SC.CAM, SC.CAM, fix_scale, iterations, seed, **kw)
    assert SC.same(dev, host), (dev[1], host[1], dev[3], host[3])
    return dev


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("iterations", [1, 7, 200, 1024])
def test_single_set(hiplib, ctx, iterations, fix_scale):
    for seed in SC.SEEDS:
        _, cnt, _, best = _both(hiplib, ctx, [SC.planted(37, 40, 0.3)[0]], fix_scale, iterations, seed)
        assert iterations < 200 or (cnt[0] >= 24 and 0 <= best[0] < iterations)


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("iterations", [1, 7, 200, 1024])
def test_the_trackers_shape(hiplib, ctx, iterations, fix_scale):
    sets, want = SC.tracker_batch()
    for seed in SC.SEEDS:
        _, cnt, _, _ = _both(hiplib, ctx, sets, fix_scale, iterations, seed)
        assert iterations < 200 or all(c >= g - 2 for c, g in zip(cnt, want))


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("iterations", [1, 7, 200, 1024])
def test_nine_sets_with_every_edge(hiplib, ctx, iterations, fix_scale):
    """n = 0, 2, 3, 4, 64, 65, 300 at 60 % wrong matches, all pairs on one point, and the whole batch behind pair_start[0] > 0"""
    sets, want = SC.edge_batch()
    for seed in SC.SEEDS:
        s12, cnt, inl, best = _both(hiplib, ctx, sets, fix_scale, iterations, seed)
        for i in (0, 1) + (() if fix_scale else (7,)):
            assert cnt[i] == 0 and best[i] == -1 and not inl[i].any() and s12[i].tobytes() == SC.NONE_S12.tobytes()
        assert iterations < 200 or all(c >= g - 2 for c, g in zip(cnt, want) if g is not None)
        shifted = _both(hiplib, ctx, sets, fix_scale, iterations, seed, first=11)
        assert SC.same(shifted, (s12, cnt, inl, best))


@pytest.mark.parametrize("fix_scale", [0, 1])
def test_planted_ties_go_to_the_lowest_iteration(hiplib, ctx, fix_scale):
    """six exact pairs: most samples explain all six, the first of them must win"""
    for seed in range(20):
        sets = [SC.exact6(seed), SC.exact6(seed + 20)]
        _, cnt, _, best = _both(hiplib, ctx, sets, fix_scale, 200, seed)
        assert (cnt == 6).all() and (best >= 0).all() and (best < 20).all()


def test_the_same_call_twice_and_without_the_iteration(hiplib, ctx):
    sets, _ = SC.tracker_batch()
    a = _both(hiplib, ctx, sets, 1, 200, 0x9E3779B9)
    b = hiplib.sim3_ransac_batch(ctx, sets, SC.CAM, SC.CAM, 1, 200, 0x9E3779B9)
    c = hiplib.sim3_ransac_batch(ctx, sets, SC.CAM, SC.CAM, 1, 200, 0x9E3779B9, want_iteration=False)
    assert SC.same(a, b) and SC.same((a[0], a[1], a[2], None), c)


def test_every_refusal_leaves_the_context_usable(hiplib, ctx):
    f = ctx.lib.lpslam_hip_sim3_ransac_batch
    f.argtypes = [C.c_void_p] + hiplib._SIM3_RANSAC_ARGS
    good = [SC.planted(37, 40, 0.3)[0]]
    want = hiplib.sim3_ransac_batch_host(good, SC.CAM, SC.CAM, 1, 50, 3)
    pairs = np.ascontiguousarray(good[0]); n = len(pairs)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ok = np.array([0, n], np.int32); cam = SC.CAM.copy()
    nan1 = cam.copy(); nan1[0] = np.nan; inf2 = cam.copy(); inf2[3] = np.inf
    s12 = np.full(8, 7.0); cnt = np.full(1, 7, np.int32); inl = np.full(n, 7, np.uint8); best = np.full(1, 7, np.int32)
    cap = hiplib.SIM3_RANSAC_MAX_ITERATIONS
    refused = [dict(n_sets=-1), dict(start=np.array([3, 1], np.int32)), dict(start=np.array([-2, 5], np.int32)), dict(start=None), dict(iterations=0), dict(iterations=cap + 1),
               dict(cam1=nan1), dict(cam2=inf2), dict(cam1=None), dict(cam2=None), dict(pairs=None), dict(s12=None), dict(cnt=None), dict(inl=None)]
    for r in refused:
        a = dict(n_sets=1, pairs=pairs, start=ok, cam1=cam, cam2=cam, iterations=50, s12=s12, cnt=cnt, inl=inl)
        a.update(r)
        rc = f(ctx.h, a["n_sets"], p(a["pairs"]), p(a["start"]), p(a["cam1"]), p(a["cam2"]), 1, a["iterations"], 3, p(a["s12"]), p(a["cnt"]), p(a["inl"]), p(best))
        assert rc == 1, r                                                                       # LPSLAM_HIP_ERR_INVALID
        assert (s12 == 7.0).all() and cnt[0] == 7 and (inl == 7).all() and best[0] == 7, r
        assert SC.same(hiplib.sim3_ransac_batch(ctx, good, SC.CAM, SC.CAM, 1, 50, 3), want), r
    assert f(ctx.h, 0, None, p(ok), p(cam), p(cam), 1, 50, 3, None, None, None, None) == 0       # no set: nothing to do
    assert (s12 == 7.0).all()
    # the cap itself is served
    _both(hiplib, ctx, good, 0, cap, 3)
