"""lpslam_hip_pose_covariance_batch (lpslam_amd/csrc/pose_cov.hip) against its CPU definition
lpslam_pose_covariance_batch_host, exactly: every output array, byte for byte.  Both sides run the same FP64 text
(csrc/pose_cov_math.h) without contraction and add in the same stated order, so there is no tolerance.  tests/test_pose_cov_cpu.py holds
the host form to the long-double reference on the cases used here."""
import ctypes as C

import numpy as np
import pytest

import pose_cov_ref as ref

pytestmark = pytest.mark.gpu

KEYS = ("info21", "cov21", "chi2", "min_pivot", "n_used", "status")
INVALID, CAPACITY = 1, 3


@pytest.fixture(scope="module")
def ctx(hiplib):
    from lpslam_amd import _build
    _build.host_library()
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


def _batch(cases, first=0):
    start = np.full(len(cases) + 1, first, np.int32); start[1:] += np.cumsum([len(c["obs"]) for c in cases]).astype(np.int32)
    pad = np.full((first, 7), np.nan)          # the records in front of set_start[0] belong to nobody: whoever reads them shows it
    obs = np.concatenate([pad] + [c["obs"] for c in cases])
    active = np.concatenate([np.ones(first, np.uint8)] + [c["active"] for c in cases])
    return start, np.array([c["pose7"] for c in cases]), obs, active


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in KEYS)


def _both(hiplib, ctx, cases, first=0):
    start, pose, obs, active = _batch(cases, first)
    dev = hiplib.pose_covariance_batch(ctx, start, pose, obs, active, ref.CAM)
    host = hiplib.pose_covariance_batch_host(start, pose, obs, active, ref.CAM)
    assert _same(dev, host), {k: (dev[k], host[k]) for k in KEYS if dev[k].tobytes() != host[k].tobytes()}
    return dev


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("n", [0, 2, 3, 4, 63, 64, 65, 255, 256, 257, 513, 2000])
def test_single_set(hiplib, ctx, n, kind):
    d = _both(hiplib, ctx, [ref.case(7, n, kind)])
    assert d["n_used"][0] == n and d["status"][0] == (0 if n >= 3 else 1)
    assert (d["cov21"][0, [0, 6, 11, 15, 18, 20]] > 0).all() if n >= 3 else not d["cov21"].any()


def test_three_sets_with_an_empty_one_in_the_middle(hiplib, ctx):
    d = _both(hiplib, ctx, [ref.case(1, 70, "mixed"), ref.case(1, 0, "mixed"), ref.case(2, 300, "stereo")])
    assert list(d["n_used"]) == [70, 0, 300] and list(d["status"]) == [0, 1, 0] and not d["info21"][1].any()


def test_nine_sets_with_every_edge(hiplib, ctx):
    """the three degenerate sets, a set whose every observation is inactive, three pc_z <= 0 observations among 40, and set_start[0] > 0"""
    cases = [ref.case(3, 64, "mixed"), ref.case(3, 0, "same_point"), ref.case(3, 0, "collinear"), ref.case(3, 0, "two_stereo"), ref.case(3, 30, "inactive"),
             ref.case(3, 40, "behind"), ref.case(3, 257, "mono"), ref.case(3, 3, "stereo"), ref.case(3, 513, "mixed")]
    d = _both(hiplib, ctx, cases)
    assert list(d["status"]) == [0, 2, 2, 1, 1, 0, 0, 0, 0] and list(d["n_used"]) == [64, 5, 7, 2, 0, 37, 257, 3, 513]
    assert (np.abs(d["min_pivot"][1:4]) <= 1e-9).all() and not d["cov21"][1:5].any()
    shifted = _both(hiplib, ctx, cases, first=11)
    assert _same(shifted, d)


def test_the_same_call_twice_gives_the_same_bytes(hiplib, ctx):
    cases = [ref.case(5, n, "mixed") for n in (2000, 65, 513)]
    assert _same(_both(hiplib, ctx, cases), _both(hiplib, ctx, cases))


def _raw(hiplib, ctx, n_sets, start, args, handle=True):
    f = ctx.lib.lpslam_hip_pose_covariance_batch
    f.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 11; f.restype = C.c_int
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return f(ctx.h if handle else None, n_sets, p(start), *[p(a) for a in args])


def test_every_refusal_is_followed_by_a_good_call(hiplib, ctx):
    c = ref.case(3, 20, "mixed")
    start = np.array([0, 20], np.int32)
    good = [np.ascontiguousarray(c["pose7"]), np.ascontiguousarray(c["obs"]), c["active"], ref.CAM, np.full(21, 7.0), np.full(21, 7.0), np.full(1, 7.0), np.full(1, 7.0),
            np.full(1, 7, np.int32), np.full(1, 7, np.int32)]
    want = _both(hiplib, ctx, [c])
    refusals = [(INVALID, 1, None, good, True), (INVALID, 1, start, good, False)]
    refusals += [(INVALID, 1, start, [None if i == k else a for i, a in enumerate(good)], True) for k in range(len(good))]
    refusals += [(INVALID, 0, start, good, True), (INVALID, -1, start, good, True), (INVALID, 1, np.array([5, 3], np.int32), good, True),
                 (INVALID, 1, np.array([-1, 3], np.int32), good, True), (INVALID, 2, np.array([0, 12, 8], np.int32), good, True),
                 (CAPACITY, 4097, np.zeros(4098, np.int32), good, True), (CAPACITY, 1, np.array([0, (1 << 18) + 1], np.int32), good, True)]
    for code, n_sets, st, args, handle in refusals:
        assert _raw(hiplib, ctx, n_sets, st, args, handle) == code, (code, n_sets, st)
        assert hiplib.load().lpslam_hip_last_error()
        assert all((a == 7).all() for a in good[4:]), "a refused call wrote an output"
        assert _same(_both(hiplib, ctx, [c]), want)


def test_the_cap_on_observations(hiplib, ctx):
    """1 << 18 observations pass (one set: 1024 strides of the 256 lanes), one more is refused"""
    n = 1 << 18
    base = ref.case(9, 4096, "mixed")
    big = dict(base, obs=np.tile(base["obs"], (n // 4096, 1)), active=np.ones(n, np.uint8))
    d = _both(hiplib, ctx, [big])
    assert d["n_used"][0] == n and d["status"][0] == 0
    one_more = dict(big, obs=np.concatenate([big["obs"], big["obs"][:1]]), active=np.ones(n + 1, np.uint8))
    start, pose, obs, active = _batch([one_more])
    with pytest.raises(hiplib.LpslamHipError, match="error 3"):
        hiplib.pose_covariance_batch(ctx, start, pose, obs, active, ref.CAM)
    with pytest.raises(hiplib.LpslamHipError) as e:
        hiplib.pose_covariance_batch_host(start, pose, obs, active, ref.CAM)
    assert e.value.code == CAPACITY
    # 4096 sets pass too (one observation each: status 1 everywhere)
    many = [dict(base, obs=base["obs"][i:i + 1], active=np.ones(1, np.uint8)) for i in range(4096)]
    d = _both(hiplib, ctx, many)
    assert (d["status"] == 1).all() and (d["n_used"] == 1).all()
