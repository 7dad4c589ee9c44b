"""The recorder in tracked sessions on the MI355X (lpslam_amd/host/record.cpp, the device encoder of csrc/jpeg.hip): what the
navigation callback returned and what the trackers returned land in the recording file in the worker's order, the images are the host
encoder's bytes encoded on the device, a recording replays to the trajectory of a live session fed the same decoded frames, and
stop() leaves a complete file."""
import ctypes as C
import glob
import json
import math
import time

import numpy as np
import pytest

import record_reader as rr
from lpslam_amd import synth

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-4, 1e-3          # the golden tolerances of tests/test_track_gpu.py
STEREO_CFG = '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "localWindow": 10, "asyncMapping": false, "loopClosure": false}'
MONO_CFG = '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4, "localWindow": 10, "asyncMapping": true}'


@pytest.fixture(scope="module")
def jpeg(hiplib):
    from lpslam_amd import _build
    lib = C.CDLL(_build.host_library())
    lib.lpslam_jpeg_encode_gray.restype = C.c_size_t
    lib.lpslam_jpeg_encode_gray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.lpslam_jpeg_decode_gray.restype = C.c_int

    def encode(img):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(4096 + 4 * img.size, np.uint8)
        n = lib.lpslam_jpeg_encode_gray(img.ctypes.data, img.shape[1], img.shape[0], 95, out.ctypes.data, out.size)
        return out[:n].tobytes()

    def decode(data):
        d = np.frombuffer(data, np.uint8).copy()
        out = np.zeros(1 << 22, np.uint8); w, h = C.c_int(0), C.c_int(0)
        assert lib.lpslam_jpeg_decode_gray(d.ctypes.data_as(C.c_void_p), C.c_size_t(len(d)), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(w), C.byref(h)) == 0
        return out[:w.value * h.value].reshape(h.value, w.value).copy()
    return dict(encode=encode, decode=decode)


def _manager(w, h, mono, tracker_cfg, config=None):
    from lpslam_amd import _build, manager
    _build.host_library()
    k = synth.intrinsics(w, h)
    m = manager.Manager()
    for num in ((0,) if mono else (0, 1)):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = w; c.resolution_y = h
        if not mono:
            c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    if config is not None:
        assert m.read_configuration_file(config)
    assert m.add_tracker("VSLAMMono" if mono else "VSLAMStereo", tracker_cfg)
    m.collect_results()
    return m


def _wait_frames(m, n, timeout=90):
    t0 = time.time()
    while len({r["timestamp"] for r in m.results}) < n and time.time() - t0 < timeout:
        time.sleep(0.01)


def _recording(tmp_path):
    files = glob.glob(str(tmp_path / "slam_*.pb"))
    assert len(files) == 1, files
    return files[0]


def _nav_callback(m, answers):
    """a navigation callback that answers with a different odometry per frame and a map state on every third frame; answers[ros ns]
    = (odom (p, p_sigma, q, q_sigma), map or None)"""
    from lpslam_amd import manager

    def fill(s, i, scale):
        s.state.position.x, s.state.position.y, s.state.position.z = 0.5 * scale * i, -0.25 * i, 1.0 + scale
        s.state.position.x_sigma, s.state.position.y_sigma, s.state.position.z_sigma = 0.01, 0.02 * scale, 0.0
        c, sn = math.cos(0.01 * i), math.sin(0.01 * i)
        s.state.orientation.w, s.state.orientation.x, s.state.orientation.y, s.state.orientation.z = c, 0.0, 0.0, sn
        s.state.orientation.sigma = 0.001 * scale
        s.state.valid = True
        return ((s.state.position.x, s.state.position.y, s.state.position.z), (0.01, 0.02 * scale, 0.0), (c, 0.0, 0.0, sn), 0.001 * scale)

    def cb(ts, odom, mp, _):
        i = int(ts.nanoseconds) // 40_000_000
        o = fill(odom.contents, i, 1.0)
        if i % 3 == 0:
            answers[int(ts.nanoseconds)] = (o, fill(mp.contents, i, 2.0))
            return 3                                                   # OdomAndMap
        answers[int(ts.nanoseconds)] = (o, None)
        return 1                                                       # OdomOnly
    f = manager.NAV_CB(cb); m._keep.append(f)
    m.lib.lpslam_manager_request_nav_data(m.h, f, None)


def _state_equal(rec, want):
    p, ps, q, qs = want
    return rec["p"] == p and rec["p_sigma"] == ps and rec["q"] == q and rec["q_sigma"] == qs


def test_stereo_session_records_frames_states_and_results(hiplib, jpeg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    w, h, n = 640, 480, 24
    seq = synth.StereoSequence(w, h, 4, n_points=6000)
    frames = [seq.frame(i) for i in range(n)]
    m = _manager(w, h, False, STEREO_CFG)
    answers = {}
    _nav_callback(m, answers)
    m.set_record(True)
    m.start()
    for i, (l, r) in enumerate(frames):
        assert m.add_stereo((i + 1) * 40_000_000, l, r)
    _wait_frames(m, n)
    m.stop()
    counters = m.recorder_counters()
    recs = rr.read_records(_recording(tmp_path))
    cams = [(k, rr.camera_image(p)) for k, (t, p) in enumerate(recs) if t == rr.CAMERA_IMAGE]
    results = [(k, rr.result(p)) for k, (t, p) in enumerate(recs) if t == rr.RESULT]
    assert len(cams) == n and len(cams) + len(results) == len(recs)
    for (_, c), (l, r), i in zip(cams, frames, range(n)):
        ts = (i + 1) * 40_000_000
        assert c["timestamp"] == ts and c["camera"] == 0 and c["camera_second"] == 1
        assert c["image"] == jpeg["encode"](l) and c["image_second"] == jpeg["encode"](r)
        odom, mp = answers[ts]
        assert c["has_odom"] and _state_equal(c["odom"], odom)
        assert c["has_map"] == (mp is not None)
        if mp is not None:
            assert _state_equal(c["map"], mp)
        else:
            assert c["map"]["p"] == (0, 0, 0) and c["map"]["q"] == (1, 0, 0, 0)
    valid = [r for r in m.results if r["valid"]]
    assert len(valid) >= n - 2 and len(results) == len(valid)
    for (_, rec), want in zip(results, valid):                         # in order and value: what the reconstruction callback received
        assert rec["timestamp"] == want["timestamp"] and rec["state"]["p"] == want["p"] and rec["state"]["q"] == want["q"]
        assert rec["state"]["velocity"] is None and rec["numbers"] == [1, 2]
    cam_pos = {c["timestamp"]: k for k, c in cams}
    for k, rec in results:                                             # each camera record precedes its frame's results
        assert cam_pos[rec["timestamp"]] < k
        assert max(p for p in cam_pos.values() if p < k) == cam_pos[rec["timestamp"]]
    assert counters["device_images"] == 2 * n and counters["host_images"] == 0 and counters["records"] == len(recs)
    rr.check_canonical(recs)


def test_replay_of_a_recording_follows_the_live_session(hiplib, jpeg, tmp_path, monkeypatch):
    """the recording replayed with "require_odometry": false against a live session fed the JPEG-decoded frames directly"""
    monkeypatch.chdir(tmp_path)
    w, h, n = 640, 480, 24
    seq = synth.StereoSequence(w, h, 4, n_points=6000)
    frames = [seq.frame(i) for i in range(n)]
    rec = _manager(w, h, False, STEREO_CFG)
    rec.provide_odometry()
    rec.set_record(True)
    rec.start()
    for i, (l, r) in enumerate(frames):
        assert rec.add_stereo((i + 1) * 40_000_000, l, r)
    _wait_frames(rec, n)
    rec.stop()
    path = _recording(tmp_path)
    cfg = tmp_path / "replay.json"
    cfg.write_text(json.dumps({"manager": {"require_odometry": False}}))

    replay = _manager(w, h, False, STEREO_CFG, config=str(cfg))
    assert replay.read_replay_items(path)
    replay.start()
    _wait_frames(replay, n)
    replay.stop()

    live = _manager(w, h, False, STEREO_CFG, config=str(cfg))
    decoded = [(jpeg["decode"](c["image"]), jpeg["decode"](c["image_second"]))
               for c in (rr.camera_image(p) for t, p in rr.read_records(path) if t == rr.CAMERA_IMAGE)]
    assert len(decoded) == n
    live.start()
    for i, (l, r) in enumerate(decoded):
        assert live.add_stereo((i + 1) * 40_000_000, l, r, ros=False)
    _wait_frames(live, n)
    live.stop()

    a = [r for r in replay.results if r["valid"]]
    b = [r for r in live.results if r["valid"]]
    assert len(a) == len(b) >= n - 2
    for x, y in zip(a, b):
        assert x["timestamp"] == y["timestamp"]
        dq = abs(float(np.dot(np.array(x["q"]) / np.linalg.norm(x["q"]), np.array(y["q"]) / np.linalg.norm(y["q"]))))
        assert 2 * math.acos(min(1.0, dq)) < ROT_TOL and float(np.abs(np.array(x["p"]) - np.array(y["p"])).max()) < TRANS_TOL


def test_monocular_session_has_no_second_fields(hiplib, jpeg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    w, h, n = 640, 480, 16
    walls = synth.WallSequence(w, h, 11)
    frames = [walls.frame(i) for i in range(n)]
    m = _manager(w, h, True, MONO_CFG)
    m.provide_odometry()
    m.set_record(True)
    m.start()
    for i, img in enumerate(frames):
        assert m.add_image((i + 1) * 40_000_000, img)
    _wait_frames(m, n)
    m.stop()
    recs = rr.read_records(_recording(tmp_path))
    cams = [rr.camera_image(p) for t, p in recs if t == rr.CAMERA_IMAGE]
    assert len(cams) == n
    for c, img in zip(cams, frames):
        assert c["image_second"] is None and c["base_second"] is None and 7 not in c["numbers"] and 8 not in c["numbers"]
        assert c["image"] == jpeg["encode"](img)
    assert len([t for t, _ in recs if t == rr.RESULT]) == len([r for r in m.results if r["valid"]])
    assert m.recorder_counters()["device_images"] == n


def test_stop_after_a_burst_leaves_a_complete_file(hiplib, tmp_path, monkeypatch):
    """the worker's camera backlog is dropped at stop(), the recorder's queue is written out (RecordEngine.cpp:330-350)"""
    monkeypatch.chdir(tmp_path)
    w, h, n = 1280, 720, 40
    seq = synth.StereoSequence(w, h, 4)
    frames = [seq.frame(i % 8) for i in range(n)]
    m = _manager(w, h, False, '{"cameraSetup": "stereo", "slamKeypoints": 2000, "numLevels": 8}')
    m.provide_odometry()
    m.set_record(True)
    m.start()
    for i, (l, r) in enumerate(frames):
        assert m.add_stereo((i + 1) * 40_000_000, l, r)
    m.stop()
    counters = m.recorder_counters()
    recs = rr.read_records(_recording(tmp_path))                      # no truncated tail
    cams = [rr.camera_image(p) for t, p in recs if t == rr.CAMERA_IMAGE]
    taken = sorted({r["timestamp"] for r in m.results})                # every frame the worker took gave the client a result
    assert [c["timestamp"] for c in cams] == taken and len(taken) >= 1
    assert all(len(c["image"]) > 1000 and len(c["image_second"]) > 1000 for c in cams)
    assert counters["records"] == len(recs) and counters["device_images"] == 2 * len(cams)
