"""The tracker option initialiseOnDevice: one short monocular session on the three-wall scene of
tests/test_track_gpu.py (g15_track_mono: the map exists from the third frame on), run with the RANSAC loop and the pose check of
LpSlam::two_view_initialize on the host (the default), on the device (lpslam_hip_two_view_ransac_batch,
lpslam_hip_two_view_check_poses) and with the option absent.  The device steps return the host steps' bits, so the outcome is the same."""
import math
import time

import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

W, H, FRAMES = 640, 480, 6
CFG = '"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4, "localWindow": 10, "asyncMapping": false'
ROT_TOL, TRANS_TOL = 1e-4, 1e-3            # tests/test_track_gpu.py: the same session twice agrees within these


@pytest.fixture(scope="module")
def runs(hiplib, tmp_path_factory):
    from lpslam_amd import _build, manager
    _build.host_library()
    d = tmp_path_factory.mktemp("init")
    walls = synth.WallSequence(W, H, 11)
    frames = [walls.frame(i) for i in range(FRAMES)]
    k = synth.intrinsics(W, H)
    out = {}
    for name, extra in (("host", ', "initialiseOnDevice": false'), ("device", ', "initialiseOnDevice": true'), ("absent", "")):
        m = manager.Manager()
        c = manager.default_camera()
        c.camera_number = 0; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]; c.resolution_x = W; c.resolution_y = H
        m.set_camera(c)
        assert m.add_tracker("VSLAMMono", "{" + CFG + extra + "}"), name
        m.collect_results(); m.provide_odometry()
        m.log_to_file(d / (name + ".log"))
        m.start()
        for i, f in enumerate(frames):
            assert m.add_image((i + 1) * 40_000_000, f)
        t0 = time.time()
        while len(m.results) < len(frames) and time.time() - t0 < 60:
            time.sleep(0.01)
        m.stop()
        out[name] = (m.tracker_statistics(), list(m.results))
    return out


def _first_valid(results):
    i = next(i for i, r in enumerate(results) if r["valid"])
    return i, np.array(results[i]["q"], float), np.array(results[i]["p"], float)


@pytest.mark.parametrize("other", ["device", "absent"])
def test_the_session_initialises_the_same_way(runs, other):
    (sh, rh), (so, ro) = runs["host"], runs[other]
    assert len(rh) == FRAMES and len(ro) == FRAMES
    (ih, qh, ph), (io, qo, po) = _first_valid(rh), _first_valid(ro)
    assert ih == io == 2                                                 # the frame of initialisation (the golden's)
    assert [r["valid"] for r in ro] == [r["valid"] for r in rh]
    dot = min(1.0, abs(float(np.dot(qh / np.linalg.norm(qh), qo / np.linalg.norm(qo)))))
    assert 2 * math.acos(dot) < ROT_TOL and np.abs(ph - po).max() < TRANS_TOL
    assert so["landmarks"] == sh["landmarks"] and sh["landmarks"] > 0
    assert so["init_attempts"] == sh["init_attempts"] >= 1 and so["keyframes"] == sh["keyframes"]


def test_the_device_steps_ran_only_with_the_option_on(runs):
    assert runs["device"][0]["init_device_calls"] >= 1
    assert runs["device"][0]["init_device_calls"] <= 2 * runs["device"][0]["init_attempts"]
    assert runs["host"][0]["init_device_calls"] == 0 and runs["absent"][0]["init_device_calls"] == 0
    for name in runs:
        assert runs[name][0]["ms_init_attempt"] > 0
