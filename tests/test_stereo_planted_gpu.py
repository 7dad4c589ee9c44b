"""The stereo matcher (k_stereo_rows, k_stereo, k_stereo_median of lpslam_amd/csrc/match.hip) on the planted cases of
tests/stereo_cases.py: keypoints on both sides of every guard, band end and size threshold, which extractor output never reaches.

Keypoints and descriptors are written straight into the image slots (lpslam_hip_set_descriptors for descriptors and count,
lpslam_hip_keypoint_buffers + hipMemcpy for the keypoint array); only upload and the pyramid stage run before the matcher.  Both
references, the oracle and the numpy restatement, are fed the device's own pyramid, so nothing here depends on pyramid parity.
Every comparison is np.array_equal on x_right, depth and best index: no tolerance."""
import ctypes as C

import numpy as np
import pytest

import stereo_cases as sc

pytestmark = pytest.mark.gpu


def set_keypoints(ctx, slot, kp, desc):
    """descriptors and count through the C ABI, the keypoint array by a host-to-device copy into the slot's buffer"""
    assert len(kp) == len(desc) <= ctx.max_kp and kp.dtype.itemsize == 28
    ctx.set_descriptors(slot, desc)
    ptr = C.c_void_p()
    rc = ctx.lib.lpslam_hip_keypoint_buffers(ctx.h, slot, C.byref(ptr), None, None)
    assert rc == 0 and ptr.value
    ctx.sync()
    if len(kp):
        kp = np.ascontiguousarray(kp)
        # hipMemcpy is looked up through the library's own handle: the HIP runtime it is linked against, whatever else is loaded
        hip_memcpy = ctx.lib.hipMemcpy
        hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip_memcpy(ptr, kp.ctypes.data, kp.nbytes, 1) == 0                  # hipMemcpyHostToDevice
    ctx.sync()


def load(ctx, case, left, right, n_images=None):
    """upload, pyramid stage (of the slots 0 .. n_images - 1), keypoints"""
    assert ctx.max_kp == sc.slots_per_image(case.max_keypoints, case.levels)
    ctx.upload(left, case.left_img); ctx.upload(right, case.right_img)
    ctx.stage("pyramid", max(left, right) + 1 if n_images is None else n_images)
    set_keypoints(ctx, left, case.kl, case.dl)
    set_keypoints(ctx, right, case.kr, case.dr)


def references(ctx, oracle, case, left, right):
    """(oracle's x_right, depth, best index), restatement result, both on the device's pyramid of the two slots"""
    pl = [ctx.pyramid_level(left, l) for l in range(case.levels)]; pr = [ctx.pyramid_level(right, l) for l in range(case.levels)]
    assert np.array_equal(pl[0], case.left_img) and np.array_equal(pr[0], case.right_img)
    p = oracle.params(case.max_keypoints, 1.2, case.levels)
    ora = oracle.match_stereo(pl, pr, p, case.kl, case.dl, case.kr, case.dr, case.fxb, case.baseline)[:3]
    res = sc.restate(pl, pr, case)
    assert all(np.array_equal(a, b) for a, b in zip(ora, (res.x_right, res.depth, res.best_idx))), "the references disagree"
    return ora, res


def assert_equal(got, want, what):
    for name, g, w in zip(("x_right", "depth", "best_idx"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.nonzero(g != w)[0][:10] if g.shape == w.shape else (g.shape, w.shape))


def run_case(ctx, oracle, case, left=0, right=1):
    """loads the case, matches the pair, compares with both references; returns (device result, restatement result)"""
    load(ctx, case, left, right)
    ctx.match_stereo(left, right, case.fxb, case.baseline)
    got = ctx.stereo(left)
    ora, res = references(ctx, oracle, case, left, right)
    assert_equal(got, ora, case.name)
    return got, res


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(320, 240, 400, 1.2, 4, max_images=6)
    yield c
    c.close()


@pytest.mark.parametrize("seed", sc.MAIN_SEEDS)
def test_main_case(ctx, oracle, seed):
    case = sc.main_case(seed)
    (xr, dep, bi), res = run_case(ctx, oracle, case)
    sc.check_main_plants(case, xr, dep, bi)
    # the one-round-trip read-back returns the keypoints as written and the same stereo columns
    kp, desc, fxr, fdep = ctx.frame(0)
    assert kp.tobytes() == case.kl.tobytes() and np.array_equal(desc, case.dl)
    assert np.array_equal(fxr, xr) and np.array_equal(fdep, dep)
    assert res.reason.count("ok") >= 50 and res.reason.count("median") >= 20


def test_long_rows(ctx, oracle):
    """rows of about 200 candidates: four trips of the lane loop; the row list's order comes from LDS atomics and must not show"""
    case = sc.long_rows_case()
    (xr, dep, bi), _ = run_case(ctx, oracle, case)
    sc.check_long_rows_plants(case, bi)
    ctx.match_stereo(0, 1, case.fxb, case.baseline)
    again = ctx.stereo(0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (xr, dep, bi)))


def test_large_counts(hiplib, oracle):
    """both slots full (2025 keypoints, not a multiple of the four wavefronts of a workgroup), more than 1024 accepted matches:
    the stride loops of k_stereo_rows and k_stereo_median"""
    case = sc.large_case()
    c = hiplib.Context(*case.ctx_args(), max_images=2)
    assert len(case.kl) == len(case.kr) == c.max_kp and c.max_kp > 1024 and c.max_kp % 4
    (xr, dep, bi), res = run_case(c, oracle, case)
    assert int((res.corr >= 0).sum()) > 1024 and int((dep > 0).sum()) > 1024 and res.reason.count("median") > 100
    c.close()


@pytest.mark.parametrize("w,h", sc.TALL_SHAPES)
def test_tall_images(hiplib, oracle, w, h):
    """H > 1024 and H > 2048: block_scan_rows of k_stereo_rows runs with two and three rows per thread"""
    case = sc.tall_case(w, h)
    c = hiplib.Context(*case.ctx_args(), max_images=2)
    (xr, dep, bi), _ = run_case(c, oracle, case)
    assert all(bi[g["left"]] == g["right"] for g in case.plants["rows"])
    assert sum(dep[g["left"]] > 0 for g in case.plants["rows"]) > 48
    c.close()


@pytest.mark.parametrize("n", sc.MEDIAN_COUNTS)
def test_median_edges(ctx, oracle, n):
    case = sc.median_case(n)
    (xr, dep, bi), res = run_case(ctx, oracle, case)
    sc.check_median_case(case, n, res)
    assert int((dep > 0).sum()) == {0: 0, 1: 1, 2: 2, 3: 2, 4: 3}[n]


def test_median_of_zero(ctx, oracle):
    """median and threshold 0: the cut is `threshold < correlation`, the matches with correlation 0 stay"""
    case = sc.median_zero_case()
    (xr, dep, bi), res = run_case(ctx, oracle, case)
    sc.check_median_zero_case(case, res, dep)


def test_batch_and_reused_slot(ctx, oracle):
    """one strided launch over pairs of very different sizes (the full main case, an empty left, an empty right), then the main
    slot matched again with three keypoints"""
    main, small = sc.main_case(sc.MAIN_SEEDS[0]), sc.median_case(3)
    no_left, no_right = main.without_left(), main.without_right()
    run_case(ctx, oracle, small)                                 # what the slots 0 and 1 hold before the batch is not the main case's result
    for case, l, r in ((main, 0, 1), (no_left, 2, 3), (no_right, 4, 5)):
        ctx.upload(l, case.left_img); ctx.upload(r, case.right_img)
    ctx.stage("pyramid", 6)
    for case, l, r in ((main, 0, 1), (no_left, 2, 3), (no_right, 4, 5)):
        set_keypoints(ctx, l, case.kl, case.dl); set_keypoints(ctx, r, case.kr, case.dr)
    ctx.match_stereo_strided(0, 1, 2, 3, main.fxb, main.baseline)
    batch = [ctx.stereo(l) for l in (0, 2, 4)]
    for case, l, got in zip((main, no_left, no_right), (0, 2, 4), batch):
        ora, _ = references(ctx, oracle, case, l, l + 1)
        assert len(got[0]) == len(case.kl)
        assert_equal(got, ora, case.name)
    assert len(batch[1][0]) == 0
    assert len(batch[2][0]) == len(main.kl) and (batch[2][0] == -1).all() and (batch[2][1] == -1).all() and (batch[2][2] == -1).all()
    for l, got in zip((0, 2, 4), batch):                         # each slot equals its single-pair result
        ctx.match_stereo(l, l + 1, main.fxb, main.baseline)
        assert_equal(ctx.stereo(l), got, "single pair %d" % l)
    # the main slot again, with few keypoints: the entries below the new count are rewritten and the count is right
    got, res = run_case(ctx, oracle, small)
    assert len(got[0]) == 3 and res.reason.count("median") == 1 and int((got[1] > 0).sum()) == 2
    kp, _, fxr, fdep = ctx.frame(0)
    assert len(kp) == 3 and np.array_equal(fxr, got[0]) and np.array_equal(fdep, got[1])
