"""Replay and ingest of compressed frames through the device JPEG decoder (lpslam_amd/host/jpeg_device.cpp, csrc/jpeg_dec.hip): a
session decoded on the device gives the poses of the same session decoded on the host, bit for bit, and the manager's counters say
where every image was decoded."""
import ctypes as C
import glob
import json
import time

import numpy as np
import pytest

import record_reader as rr
import replay_format as rf
from lpslam_amd import synth

pytestmark = pytest.mark.gpu

STEREO_CFG = '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "localWindow": 10, "asyncMapping": false, "loopClosure": false}'
W, H, N = 640, 480, 16


def _manager(tmp_path, device):
    from lpslam_amd import _build, manager
    _build.host_library()
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in (0, 1):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    cfg = tmp_path / ("decode_%d.json" % int(device))
    cfg.write_text(json.dumps({"manager": {"require_odometry": False, manager.JPEG_DECODE_DEVICE_KEY: bool(device)}}))
    assert m.read_configuration_file(str(cfg))
    assert m.add_tracker("VSLAMStereo", STEREO_CFG)
    m.collect_results()
    return m


def _wait_frames(m, n, timeout=90):
    t0 = time.time()
    while len({r["timestamp"] for r in m.results}) < n and time.time() - t0 < timeout:
        time.sleep(0.01)


def _poses(m):
    return [(r["timestamp"], r["valid"], tuple(r["p"]), tuple(r["q"])) for r in m.results]


@pytest.fixture(scope="module")
def frames():
    seq = synth.StereoSequence(W, H, 4, n_points=6000)
    return [seq.frame(i) for i in range(N)]


@pytest.fixture(scope="module")
def recording(hiplib, frames, tmp_path_factory):
    """a short stereo session written by the recorder"""
    import os
    d = tmp_path_factory.mktemp("rec")
    cwd = os.getcwd(); os.chdir(d)
    try:
        m = _manager(d, True)
        m.provide_odometry()
        m.set_record(True)
        m.start()
        for i, (l, r) in enumerate(frames):
            assert m.add_stereo((i + 1) * 40_000_000, l, r)
        _wait_frames(m, N)
        m.stop()
    finally:
        os.chdir(cwd)
    files = glob.glob(str(d / "slam_*.pb"))
    assert len(files) == 1
    return files[0]


def _replay(tmp_path, path, device):
    m = _manager(tmp_path, device)
    assert m.read_replay_items(path)
    m.start()
    _wait_frames(m, N)
    m.stop()
    return _poses(m), m.decoder_counters()


def test_replay_on_the_device_equals_replay_on_the_host(hiplib, recording, tmp_path):
    dev, cd = _replay(tmp_path, recording, True)
    hst, ch = _replay(tmp_path, recording, False)
    assert len(dev) == len(hst) >= N - 2 and dev == hst                # the same results, bitwise equal poses
    assert sum(1 for r in dev if r[1]) >= N - 2
    assert cd == dict(device_images=2 * N, host_images=0, refused_images=0)
    assert ch == dict(device_images=0, host_images=2 * N, refused_images=0)


def test_compressed_frames_handed_in(hiplib, recording, tmp_path):
    cams = [rr.camera_image(p) for t, p in rr.read_records(recording) if t == rr.CAMERA_IMAGE]
    assert len(cams) == N
    runs = []
    for device in (True, False):
        m = _manager(tmp_path, device)
        m.start()
        for i, c in enumerate(cams):
            assert m.add_jpeg_pair((i + 1) * 40_000_000, c["image"], c["image_second"], ros=False)
        _wait_frames(m, N)
        m.stop()
        runs.append((_poses(m), m.decoder_counters()))
    (dev, cd), (hst, ch) = runs
    assert len(dev) == len(hst) >= N - 2 and dev == hst
    assert cd == dict(device_images=2 * N, host_images=0, refused_images=0)
    assert ch == dict(device_images=0, host_images=2 * N, refused_images=0)
    # one image per call (LpSlamImageStructure_OneImage): counted the same way
    for device in (True, False):
        m = _manager(tmp_path, device)
        for i, c in enumerate(cams[:4]):
            assert m.add_jpeg((i + 1) * 40_000_000, c["image"], ros=False)
        want = dict(device_images=4, host_images=0, refused_images=0) if device else dict(device_images=0, host_images=4, refused_images=0)
        assert m.decoder_counters() == want
        assert not m.add_jpeg(1, b"\xff\xd8\xff\xe0JFIF-not-decodable", ros=False)
        assert m.decoder_counters()["refused_images"] == 1


def test_a_pgm_recording_never_touches_the_device_path(hiplib, frames, tmp_path):
    path = tmp_path / "pgm.pb"
    path.write_bytes(b"".join(rf.record(rf.CAMERA_IMAGE, rf.camera_image((i + 1) * 40_000_000, l, r)) for i, (l, r) in enumerate(frames)))
    runs = [_replay(tmp_path, str(path), device) for device in (True, False)]
    for poses, counters in runs:
        assert counters == dict(device_images=0, host_images=0, refused_images=0)
        assert len({p[0] for p in poses}) == N and sum(1 for p in poses if p[1]) >= N - 2
    assert runs[0][0] == runs[1][0]
