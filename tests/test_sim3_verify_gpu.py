"""lpslam_hip_sim3_verify_batch (lpslam_amd/csrc/sim3.hip): RANSAC, gate and transform optimiser of a batch of loop
candidates in one call, against the same steps one after the other -- lpslam_sim3_ransac_batch_host, the gate, and
lpslam_hip_sim3_transform_optimize on the sets that pass it.  The comparison is exact (seed_inliers, the eight doubles of s12,
n_inliers, the flags): the RANSAC is the same FP64 text on both sides and the optimiser is one device function behind both kernels.
The existing entry point itself is held to the bytes it returned before that function was split off
(tests/golden/sim3_transform_bytes.npz)."""
import numpy as np
import pytest

import sim3_batch_cases as SC
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hiplib):
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


def _steps(hiplib, ctx, sets, fix_scale, iterations, seed, gate, chi_sq):
    """the reference: host solver, gate, the optimiser call for the survivors"""
    s12, cnt, _, _ = hiplib.sim3_ransac_batch_host(sets, SC.CAM, SC.CAM, fix_scale, iterations, seed)
    out_s = s12.copy(); out_n = np.zeros(len(sets), np.int32); out_f = [np.zeros(len(p), np.uint8) for p in sets]
    surv = [i for i in range(len(sets)) if cnt[i] >= gate]
    if surv:
        so, fo, co = hiplib.sim3_transform_optimize(ctx, s12[surv], [sets[i] for i in surv], SC.CAM, SC.CAM, chi_sq, fix_scale)
        for k, i in enumerate(surv):
            out_s[i] = so[k]; out_n[i] = co[k]; out_f[i] = fo[k].astype(np.uint8)
    return cnt, out_s, out_n, out_f, s12


def _check(hiplib, ctx, sets, fix_scale, iterations, seed, gate, chi_sq=10.0):
    want = _steps(hiplib, ctx, sets, fix_scale, iterations, seed, gate, chi_sq)
    got = hiplib.sim3_verify_batch(ctx, sets, SC.CAM, SC.CAM, fix_scale, iterations, seed, gate, chi_sq)
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]), (got[0], want[0], got[2], want[2])
    assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))
    bare = hiplib.sim3_verify_batch(ctx, sets, SC.CAM, SC.CAM, fix_scale, iterations, seed, gate, chi_sq, want_inlier=False)
    assert np.array_equal(bare[0], got[0]) and bare[1].tobytes() == got[1].tobytes() and np.array_equal(bare[2], got[2]) and bare[3] is None
    return got, want[4]


@pytest.mark.parametrize("fix_scale", [0, 1])
def test_the_gate_at_its_edge(hiplib, ctx, fix_scale):
    sets = [SC.planted(63, 51, 0.3)[0]]
    _, cnt, _, _ = hiplib.sim3_ransac_batch_host(sets, SC.CAM, SC.CAM, fix_scale, 200, 0x9E3779B9)
    c = int(cnt[0])
    assert c >= 40
    (seed_cnt, s12, n_inl, fl), seed12 = _check(hiplib, ctx, sets, fix_scale, 200, 0x9E3779B9, c)
    assert seed_cnt[0] == c and n_inl[0] >= 20 and fl[0].sum() == n_inl[0] and s12[0].tobytes() != seed12[0].tobytes()       # passed: optimised
    (seed_cnt, s12, n_inl, fl), seed12 = _check(hiplib, ctx, sets, fix_scale, 200, 0x9E3779B9, c + 1)
    assert seed_cnt[0] == c and n_inl[0] == 0 and not fl[0].any() and s12[0].tobytes() == seed12[0].tobytes()               # gated: the RANSAC's seed


def test_the_optimisers_own_edge(hiplib, ctx):
    """nine good pairs pass a gate of 5, but fewer than 10 pairs are left behind the optimiser's first cut: n_inliers 0 by its rule"""
    sets = [SC.planted(9, 70)[0], SC.planted(63, 51, 0.3)[0]]
    (seed_cnt, _, n_inl, fl), _ = _check(hiplib, ctx, sets, 1, 200, 0, 5)
    assert seed_cnt[0] >= 7 and n_inl[0] == 0 and not fl[0].any() and n_inl[1] >= 20


@pytest.mark.parametrize("fix_scale", [0, 1])
def test_batches(hiplib, ctx, fix_scale):
    sets, want = SC.tracker_batch()
    # the tracker's call: all three pass
    (seed_cnt, _, n_inl, _), _ = _check(hiplib, ctx, sets, fix_scale, 200, 0x9E3779B9, 12)
    assert all(c >= g - 2 for c, g in zip(seed_cnt, want)) and (n_inl >= 12).all()
    # the middle set gated: a gate between its count and the third set's; the first set is replaced by a larger one
    mid = [SC.planted(300, 26, 0.6)[0], sets[1], sets[2]]
    (seed_cnt, _, n_inl, _), _ = _check(hiplib, ctx, mid, fix_scale, 200, 0x9E3779B9, int(seed_cnt[1]) + 1)
    assert n_inl[1] == 0 and n_inl[0] >= 20 and n_inl[2] >= 20
    # one set; every set gated; the edge sets of the RANSAC tests (none, two pairs, the coincident one) behind a gate of 3
    _check(hiplib, ctx, sets[2:], fix_scale, 200, 0, 12)
    (_, _, n_inl, _), _ = _check(hiplib, ctx, sets, fix_scale, 200, 0, 1000)
    assert (n_inl == 0).all()
    _check(hiplib, ctx, SC.edge_batch()[0], fix_scale, 7, 0, 3)


def test_refusals_and_the_same_call_twice(hiplib, ctx):
    sets, _ = SC.tracker_batch()
    a = hiplib.sim3_verify_batch(ctx, sets, SC.CAM, SC.CAM, 1, 200, 5, 12, 10.0)
    for kw in (dict(chi_sq=0.0), dict(chi_sq=float("nan")), dict(min_seed_inliers=-1), dict(iterations=0), dict(iterations=hiplib.SIM3_RANSAC_MAX_ITERATIONS + 1)):
        args = dict(iterations=200, min_seed_inliers=12, chi_sq=10.0); args.update(kw)
        with pytest.raises(hiplib.LpslamHipError):
            hiplib.sim3_verify_batch(ctx, sets, SC.CAM, SC.CAM, 1, args["iterations"], 5, args["min_seed_inliers"], args["chi_sq"])
        b = hiplib.sim3_verify_batch(ctx, sets, SC.CAM, SC.CAM, 1, 200, 5, 12, 10.0)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    assert len(hiplib.sim3_verify_batch(ctx, [], SC.CAM, SC.CAM, 1, 200, 5, 12, 10.0)[0]) == 0


def test_the_existing_entry_point_returns_the_bytes_it_did(hiplib, ctx):
    """lpslam_hip_sim3_transform_optimize on the calls of tests/test_sim3_gpu.py: s12, counts and flags as recorded before its kernel's
    body became the device function both kernels call"""
    g = golden("sim3_transform_bytes.npz")
    for name, s0, pairs, cam1, cam2, fix_scale in SC.transform_cases():
        s, fl, cnt = hiplib.sim3_transform_optimize(ctx, s0, pairs, cam1, cam2, 10.0, fix_scale)
        assert s.tobytes() == g[name + "_s12"].tobytes(), name
        assert np.array_equal(cnt, g[name + "_count"]) and np.array_equal(np.concatenate(fl).astype(np.uint8), g[name + "_inlier"]), name
