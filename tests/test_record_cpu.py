"""The recorder (lpslam_amd/host/record.cpp) through LpSlamManager, without a tracker: setRecord / setRecordImages /
setWriteImageFiles and the "record" / "record_raw" configuration keys write the reference's recording file (RecordEngine,
src/Manager/SlamManager.cpp:70-85,187,565-572,642-666; INTEGRATION.md "Recording file").  The images are compared with the host
encoder's bytes; which encoder wrote them is not asserted (these tests also run where a GPU is present)."""
import ctypes as C
import glob
import json
import os
import time

import numpy as np
import pytest

import record_reader as rr


@pytest.fixture(scope="module")
def mgrlib(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    manager.load()
    return manager


@pytest.fixture(scope="module")
def host_jpeg():
    from lpslam_amd import _build
    lib = C.CDLL(_build.host_library())
    f = lib.lpslam_jpeg_encode_gray
    f.restype = C.c_size_t
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]

    def encode(img, quality=95):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(4096 + 4 * img.size, np.uint8)
        n = f(img.ctypes.data, img.shape[1], img.shape[0], quality, out.ctypes.data, out.size)
        assert n > 0
        return out[:n].tobytes()
    return encode


def _frames(n, w=160, h=120, seed=0):
    from lpslam_amd import synth
    seq = synth.StereoSequence(w, h, seed, n_points=400)
    return [seq.frame(i) for i in range(n)]


def _wait(m, n, timeout=20):
    t0 = time.time()
    while len(m.results) < n and time.time() - t0 < timeout:
        time.sleep(0.01)
    assert len(m.results) == n


def _session(mgrlib, frames, mono=(), setup=None, nav=False):
    """a manager without tracker: stereo frames, then monocular ones (camera 2); every frame taken gives one result"""
    m = mgrlib.Manager()
    m.collect_results()
    if nav:
        m.provide_odometry()
    if setup:
        setup(m)
    m.start()
    for i, (l, r) in enumerate(frames):
        assert m.add_stereo((i + 1) * 40_000_000, l, r)
    for i, img in enumerate(mono):
        assert m.add_image((len(frames) + i + 1) * 40_000_000, img, camera=2)
    _wait(m, len(frames) + len(mono))
    m.stop()
    return m


def _recording(tmp_path):
    files = glob.glob(str(tmp_path / "slam_*.pb"))
    assert len(files) == 1, files
    name = os.path.basename(files[0])
    assert len(name) == len("slam_2026-01-01_00-00-00.pb") and name[15] == "_"
    return files[0]


def test_record_writes_one_camera_record_per_frame(mgrlib, host_jpeg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = _frames(3)
    mono = [f[0] for f in _frames(2, seed=1)]
    m = _session(mgrlib, frames, mono, setup=lambda m: m.set_record(True))
    recs = rr.read_records(_recording(tmp_path))
    assert [t for t, _ in recs] == [rr.CAMERA_IMAGE] * 5                  # no tracker: no result records (the "consumed" entries are not written)
    cams = [rr.camera_image(p) for _, p in recs]
    for i, c in enumerate(cams):
        assert c["timestamp"] == (i + 1) * 40_000_000 and not c["has_odom"] and not c["has_map"]
        for s in (c["odom"], c["map"]):                                   # the default state, velocity an empty message
            assert s["has_position"] and s["has_orientation"] and s["p"] == (0, 0, 0) and s["q"] == (1, 0, 0, 0) and s["velocity"] == b""
        assert c["base"] is not None and rr.orientation(rr._as_dict(c["base"])[2])[0] == (1, 0, 0, 0)
    for c, (l, r) in zip(cams[:3], frames):
        assert c["camera"] == 0 and c["camera_second"] == 1 and c["image"] == host_jpeg(l) and c["image_second"] == host_jpeg(r)
        assert c["numbers"] == [1, 3, 4, 5, 7, 8, 9, 10]                  # camera 0 and the flags are defaults: omitted
        assert c["base_second"] is not None
    for c, img in zip(cams[3:], mono):
        assert c["camera"] == 2 and c["image"] == host_jpeg(img) and c["image_second"] is None and c["base_second"] is None
        assert c["numbers"] == [1, 3, 4, 5, 6, 9]
    cnt = m.recorder_counters()
    assert cnt["records"] == 5 and cnt["bytes"] == os.path.getsize(_recording(tmp_path)) and cnt["device_images"] + cnt["host_images"] == 8


def test_payloads_are_canonical_proto3(mgrlib, tmp_path, monkeypatch):
    """every payload parses as SlamSerialize.proto's message and deterministic re-serialisation gives the same bytes"""
    if rr.message_classes() is None:
        pytest.skip("google.protobuf is absent")
    monkeypatch.chdir(tmp_path)
    _session(mgrlib, _frames(2), [_frames(1, seed=2)[0][0]], setup=lambda m: m.set_record(True), nav=True)
    recs = rr.read_records(_recording(tmp_path))
    assert len(recs) == 3 and rr.check_canonical(recs)
    m = rr.message_classes()["CameraImage"]()
    m.ParseFromString(recs[0][1])
    assert m.hasGlobalState_odom and not m.hasGlobalState_map and m.state_odom.orientation.w == 1.0 and m.cameraNumber_second == 1
    assert m.HasField("imageBase") and m.HasField("imageBase_second") and m.state_map.HasField("velocity")


def test_navigation_states_are_recorded(mgrlib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _session(mgrlib, _frames(2), setup=lambda m: m.set_record(True), nav=True)
    recs = rr.read_records(_recording(tmp_path))
    cams = [rr.camera_image(p) for _, p in recs]
    assert len(cams) == 2 and all(c["has_odom"] and not c["has_map"] for c in cams)
    assert all(c["numbers"] == [1, 3, 4, 5, 7, 8, 9, 10, 11] for c in cams)


def test_record_images_off_drops_camera_records(mgrlib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)

    def setup(m):
        m.set_record(True); m.set_record_images(False)
    m = _session(mgrlib, _frames(3), setup=setup)
    assert rr.read_records(_recording(tmp_path)) == []
    assert m.recorder_counters()["records"] == 0


def test_configuration_record_and_record_raw(mgrlib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = _frames(2)
    cfg = tmp_path / "rec.json"
    cfg.write_text(json.dumps({"manager": {"record": True, "record_raw": True}}))
    _session(mgrlib, frames, setup=lambda m: m.read_configuration_file(str(cfg)))
    cams = [rr.camera_image(p) for _, p in rr.read_records(_recording(tmp_path))]
    assert len(cams) == 2
    assert sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "*.jpg"))) == \
        ["000000_left.jpg", "000000_right.jpg", "000001_left.jpg", "000001_right.jpg"]
    for k, c in enumerate(cams):
        assert open(tmp_path / ("%06d_left.jpg" % k), "rb").read() == c["image"]
        assert open(tmp_path / ("%06d_right.jpg" % k), "rb").read() == c["image_second"]


def test_every_configuration_file_resets_record_raw(mgrlib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a, b = tmp_path / "a.json", tmp_path / "b.json"
    a.write_text(json.dumps({"manager": {"record": True, "record_raw": True}}))
    b.write_text(json.dumps({"manager": {"thread_num": 2}}))

    def setup(m):
        assert m.read_configuration_file(str(a)) and m.read_configuration_file(str(b))
    _session(mgrlib, _frames(2), setup=setup)
    assert len(rr.read_records(_recording(tmp_path))) == 2                # "record" stays on, record_raw was reset
    assert glob.glob(str(tmp_path / "*.jpg")) == []


def test_write_image_files_every_tenth_frame(mgrlib, host_jpeg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = _frames(12)
    m = _session(mgrlib, frames, setup=lambda m: m.set_write_image_files(True))
    assert sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "*.jpg"))) == ["0_left.jpg", "0_right.jpg", "10_left.jpg", "10_right.jpg"]
    for n in (0, 10):
        assert open(tmp_path / ("%d_left.jpg" % n), "rb").read() == host_jpeg(frames[n][0])
        assert open(tmp_path / ("%d_right.jpg" % n), "rb").read() == host_jpeg(frames[n][1])
    assert glob.glob(str(tmp_path / "*.pb")) == [] and m.recorder_counters()["records"] == 0


def test_recording_reads_back_through_read_replay_items(mgrlib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = _frames(4)
    _session(mgrlib, frames, setup=lambda m: m.set_record(True))
    path = _recording(tmp_path)
    from lpslam_amd import _build
    lib = C.CDLL(_build.host_library())
    stats = (C.c_long * 8)(); first = (C.c_long * 6)(); state = (C.c_double * 14)()
    lib.lpslam_replay_probe.restype = C.c_long
    assert lib.lpslam_replay_probe(path.encode(), stats, first, state) == 4
    assert list(stats)[:2] == [4, 4] and stats[6] == 0                    # every image decodes
    assert list(first)[:5] == [40_000_000, 0, 1, 160, 120]
    m = mgrlib.Manager()
    m.collect_results()
    assert m.read_replay_items(path)
    m.start()
    _wait(m, 4)
    m.stop()
    assert [r["timestamp"] for r in m.results] == [(i + 1) * 40_000_000 for i in range(4)]


def test_recording_off_creates_nothing(mgrlib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    m = _session(mgrlib, _frames(3))
    assert os.listdir(tmp_path) == []
    assert m.recorder_counters() == dict(device_images=0, host_images=0, records=0, bytes=0)


def test_a_later_start_opens_a_new_file(mgrlib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    m = mgrlib.Manager()
    m.collect_results()
    m.set_record(True)
    frames = _frames(2)
    m.start()
    assert m.add_stereo(40_000_000, *frames[0])
    _wait(m, 1)
    m.stop()
    first = _recording(tmp_path)
    time.sleep(1.1)                                                       # the file name has a one-second granularity
    m.start()
    assert m.add_stereo(80_000_000, *frames[1])
    _wait(m, 2)
    m.stop()
    files = sorted(glob.glob(str(tmp_path / "slam_*.pb")))
    assert len(files) == 2 and first in files
    assert [rr.camera_image(p)["timestamp"] for f in files for _, p in rr.read_records(f)] == [40_000_000, 80_000_000]
