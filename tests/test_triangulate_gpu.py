"""The triangulation step between keyframes on the device: k_epi_topk, k_tri_pairs and k_tri_pair_list of
lpslam_amd/csrc/triangulate.hip against tests/triangulate_ref.py -- planted pairs, planted candidate sets at every wave and list
edge, extracted stereo frames, a session context, the refusals -- and the tracker option triangulateNeighbours through the manager."""
import ctypes as C
import time

import numpy as np
import pytest

import triangulate_cases as tc
import triangulate_ref as tr
from lpslam_amd import synth
from test_triangulate_cpu import assert_pairs, check_planted_pairs

pytestmark = pytest.mark.gpu

W, H, KPTS, LEVELS = 640, 480, 2000, 3


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    yield c
    c.close()


def dev_cam(hiplib, cam):
    return hiplib.TriCamera(cam.fx, cam.fy, cam.cx, cam.cy, cam.fxb, cam.scale_factor)


def set_keypoints(ctx, slot, kp, desc):
    """descriptors and count through the C ABI, the keypoint array by a host-to-device copy into the slot's buffer"""
    assert len(kp) == len(desc) <= ctx.max_kp and kp.dtype.itemsize == 28
    ctx.set_descriptors(slot, np.ascontiguousarray(desc).reshape(-1, 32))
    ptr = C.c_void_p()
    assert ctx.lib.lpslam_hip_keypoint_buffers(ctx.h, slot, C.byref(ptr), None, None) == 0 and ptr.value
    ctx.sync()
    if len(kp):
        kp = np.ascontiguousarray(kp)
        hip_memcpy = ctx.lib.hipMemcpy
        hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip_memcpy(ptr, kp.ctypes.data, kp.nbytes, 1) == 0
    ctx.sync()


# ---- 1. pairs ------------------------------------------------------------------------------------------------------------------
def test_pairs(hiplib, ctx):
    """codes equal on every planted pair; X within 1e-12 (back-projections) and four times the measured SVD / Jacobi distance
    (triangulated points) of the reference -- the constants and their derivation are in test_triangulate_cpu.py"""
    refs = check_planted_pairs()
    for g, r in zip(tc.planted_pairs(), refs):
        code, X = ctx.triangulate_pairs(dev_cam(hiplib, g["cam"]), g["pose1"], g["pose2"], g["k1"], g["k2"], scale=tc.SCALE)
        assert_pairs(g, r, code, X)
    code, X = ctx.triangulate_pairs(dev_cam(hiplib, tc.CAM_MONO), tc.ORIGIN, tc.ORIGIN, np.zeros(0, tr.TRI_KP), np.zeros(0, tr.TRI_KP), scale=tc.SCALE)
    assert len(code) == 0 and X.shape == (0, 3)


# ---- 2. candidate lists ----------------------------------------------------------------------------------------------------------
# What the list tests ask of a listed candidate's landmark: the code, and a point that is the SAME point as the reference's -- a wrong
# branch, operand or keypoint moves it by centimetres at least (relative 1e-3 and more).  How close the arithmetic comes is test_pairs'
# question, on geometry planted for it; a listed candidate may have any parallax above the bound, and with it any conditioning.
X_SAME_BRANCH = 1e-6


def run_lists(hiplib, c, slot, cam, q, sets, check_codes=True):
    """plants the queries into the slot, runs the call and compares every list, count and code with the reference"""
    set_keypoints(c, slot, q["kp"], q["desc"])
    q_depth = None
    if cam.fxb > 0:                                                   # the slot's stereo columns are whatever its last stereo match left there
        q_xr, q_depth = c.frame(slot)[2:4]
    out = c.triangulate_neighbours(slot, q["group"], tc.ORIGIN, dev_cam(hiplib, cam), list(sets), scale=tc.SCALE)
    n1 = len(q["kp"])
    assert out["j"].shape == (len(sets), n1, 8) and out["count"].shape == (len(sets), n1)
    ref = [tr.candidates(cam, tc.SCALE, q["kp"], q["desc"], q["group"], q_depth, s["kpts"], s["desc"], s["group"], s["depth"], s["F"], s["epipole"]) for s in sets]
    for k, (s, (j, dist, count)) in enumerate(zip(sets, ref)):
        assert np.array_equal(out["count"][k], count), (k, np.flatnonzero(out["count"][k] != count)[:10])
        assert np.array_equal(out["j"][k], j), (k, np.argwhere(out["j"][k] != j)[:10])
        assert np.array_equal(out["dist"][k], dist)
        if not check_codes:
            continue
        k1 = tc.to_tri_keypoints(q["kp"], None if q_depth is None else q_xr, q_depth); k2 = tc.to_tri_keypoints(s["kpts"], s["x_right"], s["depth"])
        for i, r in np.argwhere(j >= 0)[:400]:                        # (the codes of the first 400 listed candidates of the set)
            w = tr.tri_pair(cam, tc.SCALE, tc.ORIGIN, s["pose"], k1[i], k2[j[i, r]])
            if w["margin"] < 1e-9:
                continue
            assert out["code"][k, i, r] == w["code"], (k, i, r, w["reason"])
            if w["code"]:
                assert np.linalg.norm(out["X"][k, i, r] - w["X"]) <= X_SAME_BRANCH * np.linalg.norm(w["X"])
        assert (out["code"][k][j < 0] == 0).all() and np.isnan(out["X"][k][out["code"][k] == 0]).all()
    return out, ref


# query and target counts 0, 1, 63, 64, 65, 257 and the slot maximum (-1); 1, 3 and 32 neighbours
LIST_SHAPES = [(0, 65, 1), (65, 0, 1), (1, 1, 1), (63, 64, 3), (64, 65, 3), (65, 63, 1), (257, 257, 32), (65, 257, 32), (-1, -1, 3), (-1, 257, 1), (257, -1, 3)]


@pytest.mark.parametrize("groups", ["zero", "vocab"])
@pytest.mark.parametrize("shape", LIST_SHAPES)
def test_candidate_lists(hiplib, ctx, shape, groups):
    n1, n2, n_sets = (ctx.max_kp if v < 0 else v for v in shape)
    cam, q, sets = tc.planted_sets(n1, n2, n_sets, groups=groups)
    out, ref = run_lists(hiplib, ctx, 0, cam, q, sets, check_codes=n1 <= 257)
    if min(n1, n2) >= 63:
        assert sum(int(c.sum()) for _, _, c in ref) > 0


def test_candidate_edge_cases(hiplib, ctx):
    """a degenerate line, has_epipole = 0, groups with negatives, ties, more than eight passing candidates, the epipole rule switched
    by the targets' stereo flags (that these cases are in the planted sets is established by test_triangulate_cpu.py as well)"""
    cam, q, sets = tc.planted_sets(257, 257, 3, groups="vocab", degenerate=(1,), no_epipole=(2,))
    out, ref = run_lists(hiplib, ctx, 0, cam, q, sets)
    j, dist, count = ref[0]
    assert count.max() > tr.LISTED and ref[1][2].sum() == 0 and (count[q["group"] < 0] == 0).all()
    assert any(j[i, r + 1] >= 0 and dist[i, r] == dist[i, r + 1] for i in range(len(j)) for r in range(tr.LISTED - 1))
    s0 = dict(sets[0]); s0["epipole"] = None
    assert run_lists(hiplib, ctx, 0, cam, q, [s0])[1][0][2].sum() > count.sum()
    cam_s, q_s, sets_s = tc.planted_sets(257, 257, 1, groups="vocab", target_stereo=True)
    # (a camera with a baseline reads the slot's stereo columns, which nothing has written: the lists depend on their sign only and are
    # compared, the codes would depend on their values and are not)
    _, ref_s = run_lists(hiplib, ctx, 0, cam_s, q_s, sets_s, check_codes=False)
    mono = dict(sets_s[0]); mono["depth"] = None; mono["x_right"] = None
    _, ref_m = run_lists(hiplib, ctx, 0, cam_s, q_s, [mono], check_codes=False)
    assert ref_m[0][2].sum() <= ref_s[0][2].sum()


def test_eight_nearest_candidates_on_one_lane(hiplib, ctx):
    """One query and 64 * 8 + 1 = 513 keypoints of one neighbour that all pass the gate (every one a copy of the query's partner, half a
    pixel around it): candidate j is met by lane j % 64.  The eight nearest (1 .. 8 bits from the query, every other one 40) are
    keypoints 5, 69, ..., 453 -- all lane 5 -- so the wavefront's eight answers are one lane's whole list, popped eight times."""
    cam, q, sets = tc.planted_sets(1, 513, 1)
    q = {k: v.copy() for k, v in q.items()}
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sets[0].items()}
    rng = np.random.default_rng(47)
    X = np.array([[0.4, -0.3, 7.0]])
    u, v, _ = tr.project(cam, tc.ORIGIN, X); pu, pv, _ = tr.project(cam, s["pose"], X)
    q["kp"]["x"] = u; q["kp"]["y"] = v; q["kp"]["octave"] = 0; q["group"][:] = 0
    s["kpts"]["x"] = pu + rng.uniform(-0.5, 0.5, 513); s["kpts"]["y"] = pv + rng.uniform(-0.5, 0.5, 513); s["kpts"]["octave"] = 0; s["group"][:] = 0
    best8 = 5 + 64 * np.arange(8)
    for j in range(513):
        s["desc"][j] = tc._flip(rng, q["desc"][0], 40)
    for r, j in enumerate(best8):
        s["desc"][j] = tc._flip(rng, q["desc"][0], 1 + r)
    out, ref = run_lists(hiplib, ctx, 0, cam, q, [s])
    j, dist, count = ref[0]
    assert count[0] == 513 and j[0].tolist() == best8.tolist() and dist[0].tolist() == list(range(1, 9))


# ---- 3. through extraction -------------------------------------------------------------------------------------------------------
def seq_pose(seq, k):
    R, t = seq.pose(k)
    return tr.pose_from(R, t)


def test_through_extraction(hiplib):
    """frames k and k + 4 of the stereo sequence extracted and stereo-matched into slots: lists, counts and codes equal the reference
    computed from the read-back keypoints, with real stereo flags on both sides"""
    w, h = 320, 240
    seq = synth.StereoSequence(w, h, 4, n_points=3000)
    k = synth.intrinsics(w, h)
    c = hiplib.Context(w, h, 800, 1.2, LEVELS, max_images=4)
    try:
        for slot, frame in ((0, 3), (2, 7)):
            l, r = seq.frame(frame)
            c.upload(slot, l); c.upload(slot + 1, r)
        c.extract_range(0, 4)
        c.match_stereo(0, 1, k["fxb"], k["baseline"]); c.match_stereo(2, 3, k["fxb"], k["baseline"])
        kp_n, desc_n, xr_n, dep_n = c.frame(0)
        kp_c, desc_c, xr_c, dep_c = c.frame(2)
        assert len(kp_n) > 100 and len(kp_c) > 100 and (dep_c > 0).any() and (dep_c <= 0).any()
        cam = tr.Cam(k["fx"], k["fy"], k["cx"], k["cy"], k["fxb"], 1.2)
        pose_c, pose_n = seq_pose(seq, 7), seq_pose(seq, 3)
        F, ep = tr.epipolar(cam, pose_c, pose_n)
        s = {"kpts": kp_n, "desc": desc_n, "group": np.zeros(len(kp_n), np.int32), "x_right": xr_n, "depth": dep_n, "pose": pose_n, "F": F, "epipole": ep}
        group1 = np.zeros(len(kp_c), np.int32)
        scale = np.asarray(c.scale, np.float32)
        out = c.triangulate_neighbours(2, group1, pose_c, dev_cam(hiplib, cam), [s], scale=scale)
        j, dist, count = tr.candidates(cam, scale, kp_c, desc_c, group1, dep_c, kp_n, desc_n, s["group"], dep_n, F, ep)
        assert np.array_equal(out["count"][0], count) and np.array_equal(out["j"][0], j) and np.array_equal(out["dist"][0], dist)
        assert (count > 0).sum() > 30
        k1 = tc.to_tri_keypoints(kp_c, xr_c, dep_c); k2 = tc.to_tri_keypoints(kp_n, xr_n, dep_n)
        codes = set()
        for i, r in np.argwhere(j >= 0):
            wnt = tr.tri_pair(cam, scale, pose_c, pose_n, k1[i], k2[j[i, r]])
            if wnt["margin"] < 1e-9:
                continue
            assert out["code"][0, i, r] == wnt["code"], (i, r, wnt["reason"])
            codes.add(wnt["code"])
            if wnt["code"]:
                assert np.linalg.norm(out["X"][0, i, r] - wnt["X"]) <= X_SAME_BRANCH * np.linalg.norm(wnt["X"])
        assert codes - {0}                                            # some pair makes a landmark
    finally:
        c.close()


# ---- 4. session ------------------------------------------------------------------------------------------------------------------
def test_session_context_gives_the_same(hiplib, ctx):
    cam, q, sets = tc.planted_sets(257, 257, 3, groups="vocab")
    plain, _ = run_lists(hiplib, ctx, 1, cam, q, sets, check_codes=False)
    s = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=2, session=True)
    try:
        sess, _ = run_lists(hiplib, s, 1, cam, q, sets, check_codes=False)
    finally:
        s.close()
    for key in ("j", "dist", "code", "count"):
        assert np.array_equal(plain[key], sess[key]), key
    assert np.array_equal(plain["X"], sess["X"], equal_nan=True)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(hiplib, ctx):
    cam, q, sets = tc.planted_sets(65, 63, 1)
    set_keypoints(ctx, 0, q["kp"], q["desc"])
    dc = dev_cam(hiplib, cam)

    def refused(code, **kw):
        args = dict(image=0, group1=q["group"], pose1=tc.ORIGIN, cam=dc, sets=list(sets), scale=tc.SCALE)
        args.update(kw)
        with pytest.raises(hiplib.LpslamHipError) as e:
            ctx.triangulate_neighbours(args.pop("image"), args.pop("group1"), args.pop("pose1"), args.pop("cam"), args.pop("sets"), **args)
        assert "error %d" % code in str(e.value), str(e.value)

    INVALID, CAPACITY = 1, 3
    refused(CAPACITY, sets=list(sets) * 33)                           # more than 32 neighbours
    big = dict(sets[0]); big["n"] = ctx.max_kp + 1
    refused(CAPACITY, sets=[big])                                     # a set above the slot maximum
    refused(CAPACITY, image=4); refused(CAPACITY, image=-1)           # an image slot out of range
    refused(CAPACITY, capacity=64)                                    # result rows below the slot's count
    refused(INVALID, group1=None)                                     # a null argument
    negative = dict(sets[0]); negative["n"] = -1
    refused(INVALID, sets=[negative])                                 # a negative count
    bad_oct = dict(sets[0]); bad_oct["kpts"] = sets[0]["kpts"].copy(); bad_oct["kpts"]["octave"][3] = len(tc.SCALE)
    refused(INVALID, sets=[bad_oct])                                  # an octave outside the scale table
    nan_F = dict(sets[0]); nan_F["F"] = np.full((3, 3), np.nan)
    refused(INVALID, sets=[nan_F])
    refused(INVALID, scale=np.ones(17, np.float32)); refused(INVALID, scale=np.zeros(3, np.float32))
    refused(INVALID, cam=hiplib.TriCamera(0.0, 500.0, 320.0, 240.0))
    refused(INVALID, pose1=np.zeros(7))
    refused(INVALID, image=3)                                         # a slot that never held an extraction
    ctx.triangulate_neighbours(0, q["group"], tc.ORIGIN, dc, list(sets) * 32, scale=tc.SCALE)      # the limits themselves are accepted
    with pytest.raises(hiplib.LpslamHipError):
        ctx.triangulate_pairs(dc, tc.ORIGIN, tc.ORIGIN, np.zeros(1, tr.TRI_KP), np.zeros(1, tr.TRI_KP), scale=np.ones(17, np.float32))
    k_bad = np.zeros(1, tr.TRI_KP); k_bad["octave"] = 9
    with pytest.raises(hiplib.LpslamHipError):
        ctx.triangulate_pairs(dc, tc.ORIGIN, tc.ORIGIN, k_bad, np.zeros(1, tr.TRI_KP), scale=tc.SCALE)


# ---- 6, 7. through the manager ---------------------------------------------------------------------------------------------------
def run_stereo(tmp_path, frames, k, option, tag):
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h, n_frames = 640, 480, len(frames)
    m = manager.Manager()
    for num in (0, 1):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = w; c.resolution_y = h; c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    assert m.add_tracker("VSLAMStereo", '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "asyncMapping": true, "triangulateNeighbours": %d}' % option)
    m.collect_results(); m.provide_odometry()
    log = tmp_path / ("slam_%s.log" % tag)
    m.log_to_file(log)
    m.start()
    for i, (l, r) in enumerate(frames):
        assert m.add_stereo((i + 1) * 40_000_000, l, r)
    t0 = time.time()
    while len(m.results) < n_frames and time.time() - t0 < 60:
        time.sleep(0.01)
    st = m.status()
    feats = m.features()
    m.stop()
    return m.results, st, feats, manager.Manager.statistics(log)


def test_stereo_sequence_grows_the_map_beyond_the_depth_threshold(hiplib, tmp_path):
    """the sequence of test_stereo_sequence_through_the_manager with triangulateNeighbours = 10: that test's assertions, and a map
    that holds more landmarks -- among them more beyond 40 baselines than the first keyframe and the top-up give"""
    w, h, n_frames = 640, 480, 24
    k = synth.intrinsics(w, h)
    seq = synth.StereoSequence(w, h, 4, n_points=6000)
    frames = [seq.frame(i) for i in range(n_frames)]
    res, st, feats, st_log = run_stereo(tmp_path, frames, k, 10, "on")
    assert len(res) == n_frames
    assert st_log["motion_tracked"] >= n_frames - 6
    assert st_log["keyframes"] == st.key_frames and st_log["local_ba"] >= 2 and st_log["lost"] == 0
    assert st_log["fused_added"] + st_log["fused_merged"] > 0
    valid = [r for r in res if r["valid"]]
    assert len(valid) >= n_frames - 2 and st.localization == 2 and st.key_frames >= 3 and st.feature_points > 100
    assert len(feats) == st.feature_points
    last = valid[-1]
    kf = n_frames - 1
    assert abs(last["p"][2] - 0.05 * kf) < 0.1 * 0.05 * kf and abs(last["p"][0]) < 0.05 and abs(last["p"][1]) < 0.05
    zs = [r["p"][2] for r in valid]
    assert all(b > a - 0.01 for a, b in zip(zs, zs[1:]))
    assert abs(last["q"][0]) > 0.999
    res0, st0, feats0, st_log0 = run_stereo(tmp_path, frames, k, 0, "off")
    assert st_log0["triangulated"] == 0 and st_log0["tri_pairs"] == 0
    assert st_log["triangulated"] > 0 and st_log["tri_pairs"] > 0
    assert st.feature_points > st0.feature_points
    # further than 40 baselines from EVERY keyframe: beyond 4.8 m in front of the last camera position
    far_limit = 40 * k["baseline"] + 0.05 * kf
    far = sum(f[2] > far_limit for f in feats); far0 = sum(f[2] > far_limit for f in feats0)
    print("stereo, triangulateNeighbours 10 / 0: landmarks %d / %d, beyond 40 baselines %d / %d, triangulated %d over %d pairs, %d exhausted, %.4f ms per frame"
          % (st.feature_points, st0.feature_points, far, far0, st_log["triangulated"], st_log["tri_pairs"], st_log["tri_exhausted"], st_log["ms_kf_triangulate"]))
    assert far > far0


def run_mono(frames, k, extra):
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h = 640, 480
    m = manager.Manager()
    c = manager.default_camera()
    c.camera_number = 0; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]; c.resolution_x = w; c.resolution_y = h
    m.set_camera(c)
    assert m.add_tracker("VSLAMMono", '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4%s}' % extra)
    m.collect_results(); m.provide_odometry()
    m.start()
    for i, img in enumerate(frames):
        assert m.add_image((i + 1) * 40_000_000, img)
    t0 = time.time()
    while len(m.results) < len(frames) and time.time() - t0 < 60:
        time.sleep(0.01)
    st = m.status()
    m.stop()
    return m.results, st, m.tracker_statistics()


def test_monocular_sequence_with_covisible_neighbours(hiplib):
    """the wall sequence of test_monocular_sequence_initialises_and_tracks with triangulateNeighbours = 20 and baselineDistThresh =
    0.02: that test's assertions, at least as many landmarks as without the option, and more than one neighbour served per keyframe"""
    w, h, n_frames = 640, 480, 30
    k = synth.intrinsics(w, h)
    seq = synth.WallSequence(w, h, 11)
    centres = [seq.centre(i) for i in range(n_frames)]
    frames = [seq.frame(i) for i in range(n_frames)]
    res, st, stats = run_mono(frames, k, ', "triangulateNeighbours": 20, "baselineDistThresh": 0.02')
    valid = [(i, r) for i, r in enumerate(res) if r["valid"]]
    assert len(res) == n_frames and len(valid) >= n_frames - 12
    assert st.localization == 2 and st.key_frames >= 4 and st.feature_points > 150
    i0, r0 = valid[0]; i1, r1 = valid[-1]
    d = np.array(r1["p"]) - np.array(r0["p"])
    truth = centres[i1] - centres[i0]
    truth_lp = np.array([-truth[1], truth[0], truth[2]])
    assert d @ truth_lp / (np.linalg.norm(d) * np.linalg.norm(truth_lp)) > 0.995
    mid_i, mid_r = valid[len(valid) // 2]
    frac = np.linalg.norm(np.array(mid_r["p"]) - np.array(r0["p"])) / np.linalg.norm(d)
    frac_true = np.linalg.norm(centres[mid_i] - centres[i0]) / np.linalg.norm(truth)
    assert abs(frac - frac_true) < 0.1
    res0, st0, stats0 = run_mono(frames, k, "")
    print("monocular, triangulateNeighbours 20 / 0: landmarks %d / %d, triangulated %d over %d pairs in %d keyframes, %d exhausted"
          % (st.feature_points, st0.feature_points, stats["triangulated"], stats["tri_pairs"], stats["keyframes"], stats["tri_exhausted"]))
    assert st.feature_points >= st0.feature_points
    assert stats["triangulated"] > 0 and stats["tri_pairs"] > stats["keyframes"]          # some keyframe was served by more than one neighbour
    assert stats0["triangulated"] == 0 and stats0["tri_pairs"] == 0


def test_option_out_of_range_refuses_the_start(hiplib, tmp_path):
    from lpslam_amd import _build, manager
    _build.host_library()
    k = synth.intrinsics(640, 480)
    for value, refused in ((33, True), (-1, True), (32, False)):
        m = manager.Manager()
        c = manager.default_camera()
        c.camera_number = 0; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]; c.resolution_x = 640; c.resolution_y = 480
        m.set_camera(c)
        assert m.add_tracker("VSLAMMono", '{"cameraSetup": "monocular", "triangulateNeighbours": %d}' % value)
        log = tmp_path / ("start_%d.log" % value)
        m.log_to_file(log)
        m.start()
        m.stop()
        text = open(log, errors="replace").read()
        assert ("triangulateNeighbours %d outside 0 .. 32" % value in text) == refused, text
        assert ("Tracker VSLAMMono failed to start" in text) == refused, text
