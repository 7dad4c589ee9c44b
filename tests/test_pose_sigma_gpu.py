"""The tracker option poseSigma: the short stereo session of test_stereo_sequence_through_the_manager
(tests/test_host_gpu.py; here with the mapping on the tracking thread so that a session repeats) with the option absent, false and true.
The option only adds a call behind each pose, so the three sessions agree on every frame's pose exactly and on the keyframe count; only the
session with the option on hands out sigmas.  One monocular session (that of test_monocular_sequence_initialises_and_tracks) with the option
on: sigmas in map units behind the initialisation."""
import math
import time

import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

W, H, N_FRAMES = 640, 480, 24
CFG = '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "asyncMapping": false%s}'


def _run(m, n_frames, feed):
    m.collect_results(); m.provide_odometry()
    m.start()
    feed(m)
    t0 = time.time()
    while len(m.results) < n_frames and time.time() - t0 < 60:
        time.sleep(0.01)
    m.stop()
    return m.tracker_statistics(), list(m.results)


def _stereo_session(manager, frames, extra):
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in (0, 1):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    assert m.add_tracker("VSLAMStereo", CFG % extra)

    def feed(m):
        for i, (l, r) in enumerate(frames):
            assert m.add_stereo((i + 1) * 40_000_000, l, r)
    return _run(m, len(frames), feed)


@pytest.fixture(scope="module")
def runs(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    seq = synth.StereoSequence(W, H, 4, n_points=6000)
    frames = [seq.frame(i) for i in range(N_FRAMES)]
    return {name: _stereo_session(manager, frames, extra) for name, extra in (("absent", ""), ("false", ', "poseSigma": false'), ("true", ', "poseSigma": true'))}


def test_the_three_sessions_agree_on_every_pose(runs):
    sa, ra = runs["absent"]
    assert len(ra) == N_FRAMES and sa["lost"] == 0 and sa["keyframes"] >= 3
    for name in ("false", "true"):
        s, r = runs[name]
        assert s["keyframes"] == sa["keyframes"] and s["pose_fits"] == sa["pose_fits"] and len(r) == len(ra), name
        differ = [i for i, (a, b) in enumerate(zip(r, ra)) if (a["valid"], a["p"], a["q"]) != (b["valid"], b["p"], b["q"])]
        assert not differ, (name, differ[:5], r[differ[0]], ra[differ[0]])


def test_without_the_option_every_sigma_is_zero(runs):
    for name in ("absent", "false"):
        s, r = runs[name]
        assert all(x["sigma"] == (0.0, 0.0, 0.0, 0.0) for x in r), name
        assert s["pose_sigmas"] == 0 and s["pose_sigma_refused"] == 0 and s["ms_dev_pose_sigma"] == 0.0, name
        assert s["pose_fits"] >= N_FRAMES - 6, name      # (at least the motion-model fit of most frames: test_stereo_sequence_through_the_manager)


def test_with_the_option_every_tracked_pose_has_sigmas(runs):
    s, r = runs["true"]
    print("statistics:", {k: s[k] for k in ("pose_fits", "pose_sigmas", "pose_sigma_refused", "ms_dev_pose", "ms_dev_pose_sigma", "ms_per_frame")},
          "ms_per_frame without the option:", runs["absent"][0]["ms_per_frame"], runs["false"][0]["ms_per_frame"])
    assert r[0]["sigma"] == (0.0, 0.0, 0.0, 0.0)      # the first frame's pose is the map's origin: no poseFromMatches behind it
    with_sigmas = [x for x in r[1:] if all(math.isfinite(v) and v > 0 for v in x["sigma"])]
    without = [x for x in r[1:] if x["sigma"] == (0.0, 0.0, 0.0, 0.0)]
    assert len(with_sigmas) + len(without) == len(r) - 1, "a result with some sigmas only"
    assert len(without) <= s["pose_sigma_refused"]
    assert s["pose_sigmas"] >= 1 and s["pose_sigmas"] + s["pose_sigma_refused"] == s["pose_fits"]
    assert s["ms_dev_pose_sigma"] > 0
    # a stereo pose from hundreds of points a few metres away at one pixel of noise: centimetres and milliradians, never half a metre or half a radian
    print("largest sigma of the session:", max(max(x["sigma"]) for x in with_sigmas))
    assert all(v < 0.5 for x in with_sigmas for v in x["sigma"]), max(max(x["sigma"]) for x in with_sigmas)


def test_a_monocular_session_delivers_sigmas_after_initialisation(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    n_frames = 30
    k = synth.intrinsics(W, H)
    seq = synth.WallSequence(W, H, 11)
    frames = [seq.frame(i) for i in range(n_frames)]
    m = manager.Manager()
    c = manager.default_camera()
    c.camera_number = 0; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]; c.resolution_x = W; c.resolution_y = H
    m.set_camera(c)
    assert m.add_tracker("VSLAMMono", '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4, "poseSigma": true}')

    def feed(m):
        for i, img in enumerate(frames):
            assert m.add_image((i + 1) * 40_000_000, img)
    s, r = _run(m, n_frames, feed)
    valid = [x for x in r if x["valid"]]
    assert len(r) == n_frames and len(valid) >= n_frames - 12
    tracked = valid[1:]          # the first valid result is the initialisation's own pose
    assert s["pose_sigmas"] >= 1 and s["pose_sigmas"] + s["pose_sigma_refused"] == s["pose_fits"]
    with_sigmas = [x for x in tracked if all(math.isfinite(v) and v > 0 for v in x["sigma"])]
    assert len(with_sigmas) >= len(tracked) - s["pose_sigma_refused"] and len(with_sigmas) >= 1
