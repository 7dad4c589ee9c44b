"""The tracker option verifyLoopsOnDevice: the session of test_loop_is_detected_and_closed (tests/test_host_gpu.py;
a full turn inside a ring of structure, here with the mapping on the tracking thread so that a session repeats) with the loop
candidates verified on the host, by lpslam_hip_sim3_verify_batch, and with the option absent.  The device call returns the host path's
numbers bit for bit, and two sessions with the option off agree pose for pose, so the three sessions must agree on every counter and on
every frame's pose exactly."""
import time

import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

W, H = 640, 480
CFG = '{"cameraSetup": "stereo", %s"slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 3, "localWindow": 4, "loopClosure": true, "asyncMapping": false%s}'


def _session(manager, frames, log, extra, vocab=""):
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in (0, 1):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    assert m.add_tracker("VSLAMStereo", CFG % (vocab, extra))
    m.collect_results(); m.provide_odometry()
    m.log_to_file(log)
    m.start()
    for i, (l, r) in enumerate(frames):
        assert m.add_stereo((i + 1) * 40_000_000, l, r)
    t0 = time.time()
    while len(m.results) < len(frames) and time.time() - t0 < 60:
        time.sleep(0.01)
    m.stop()
    return manager.Manager.statistics(log), [(r["valid"], r["p"], r["q"]) for r in m.results]


@pytest.fixture(scope="module")
def runs(hiplib, tmp_path_factory):
    from lpslam_amd import _build, manager
    _build.host_library()
    frames, _ = synth.turning_sequence(W, H)
    d = tmp_path_factory.mktemp("loop_device")
    out = {name: _session(manager, frames, d / (name + ".log"), extra)
           for name, extra in (("host", ', "verifyLoopsOnDevice": false'), ("device", ', "verifyLoopsOnDevice": true'), ("absent", ""))}
    out["n_frames"] = len(frames)
    return out


def test_the_three_sessions_agree(runs):
    sh, ph = runs["host"]
    assert sh["loops_closed"] >= 1 and sh["loop_tries"] >= 1 and len(ph) == runs["n_frames"]
    for name in ("device", "absent"):
        s, p = runs[name]
        for k in ("loops_closed", "loop_fused", "global_ba", "lost", "keyframes", "loop_tries"):
            assert s[k] == sh[k], (name, k, s[k], sh[k])
        assert len(p) == len(ph)
        differ = [i for i, (a, b) in enumerate(zip(p, ph)) if a != b]
        assert not differ, (name, differ[:5], p[differ[0]], ph[differ[0]])


def test_only_the_option_sends_batches_to_the_device(runs):
    assert runs["device"][0]["sim3_batches"] >= 1 and runs["device"][0]["sim3_batches"] <= runs["device"][0]["loop_tries"]
    assert runs["host"][0]["sim3_batches"] == 0 and runs["absent"][0]["sim3_batches"] == 0
    for name in ("host", "device", "absent"):
        assert runs[name][0]["ms_loop_try"] > 0


def test_vocabulary_candidates_are_verified_on_the_device(hiplib, tmp_path):
    """the session of test_loop_is_closed_with_vocabulary_candidates with the option on"""
    from bow_util import VOCAB
    from lpslam_amd import _build, manager
    _build.host_library()
    frames, _ = synth.turning_sequence(W, H, n_frames=210)
    s, _ = _session(manager, frames, tmp_path / "slam.log", ', "verifyLoopsOnDevice": true', '"vocabFile": "%s", ' % VOCAB)
    assert s["loops_closed"] >= 1 and s["sim3_batches"] >= 1 and s["lost"] == 0
