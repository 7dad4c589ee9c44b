"""Without a device the replay reader decodes JPEG payloads on the host, as it always has: the device decoder cannot be created, which
is logged once, and lpslam_replay_probe and a manager's replay give what they gave before."""
import ctypes as C
import json
import time

import numpy as np
import pytest

import replay_format as rf


@pytest.fixture(scope="module")
def lib(hiplib):
    from lpslam_amd import _build
    l = C.CDLL(_build.host_library())
    l.lpslam_jpeg_encode_gray.restype = C.c_size_t
    l.lpslam_jpeg_encode_gray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    l.lpslam_replay_probe.restype = C.c_long
    return l


def _encode(lib, img):
    out = np.zeros(4096 + 4 * img.size, np.uint8)
    n = lib.lpslam_jpeg_encode_gray(img.ctypes.data, img.shape[1], img.shape[0], 95, out.ctypes.data, out.size)
    assert n > 0
    return out[:n].tobytes()


def _stereo_jpeg_record(lib, ts, left, right):
    """a CameraImage record as the recorder writes it: both payloads JPEG"""
    m = rf.camera_image(ts, left, right, raw_left=_encode(lib, left))
    return rf.record(rf.CAMERA_IMAGE, m.replace(rf.f_bytes(7, rf.pgm(right)), rf.f_bytes(7, _encode(lib, right))))


def _recording(lib, tmp_path, n=5):
    rng = np.random.default_rng(3)
    frames = [(rng.integers(0, 256, (60, 88), dtype=np.uint8), rng.integers(0, 256, (60, 88), dtype=np.uint8)) for _ in range(n)]
    stream = [_stereo_jpeg_record(lib, (i + 1) * 1000, l, r) for i, (l, r) in enumerate(frames)]
    stream.append(rf.record(rf.CAMERA_IMAGE, rf.camera_image(9000, frames[0][0], frames[0][1], raw_left=_encode(lib, frames[0][0]))))   # JPEG beside PGM
    stream.append(rf.record(rf.CAMERA_IMAGE, rf.camera_image(9500, frames[0][0], raw_left=b"\xff\xd8\xff\xe0JFIF-not-decodable")))
    path = tmp_path / "jpeg.pb"
    path.write_bytes(b"".join(stream))
    return str(path), n


def test_probe_reads_a_jpeg_recording_as_before(lib, hiplib, tmp_path):
    path, n = _recording(lib, tmp_path)
    stats = (C.c_long * 8)(); first = (C.c_long * 6)(); state = (C.c_double * 14)()
    for _ in range(2):                                                 # a second reader in the same process behaves the same
        assert lib.lpslam_replay_probe(path.encode(), stats, first, state) == n + 1
        assert list(stats) == [n + 2, n + 2, 0, 0, 0, 0, 1, 0]
        assert list(first) == [1000, 0, 1, 88, 60, 1]


def test_a_manager_replays_on_the_host_where_no_device_is(lib, hiplib, tmp_path):
    if hiplib.device_count() > 0:
        pytest.skip("a GPU is present")
    from lpslam_amd import manager
    path, n = _recording(lib, tmp_path)
    for key in (True, False):
        cfg = tmp_path / ("cfg_%d.json" % int(key))
        cfg.write_text(json.dumps({"manager": {"require_odometry": False, manager.JPEG_DECODE_DEVICE_KEY: key}}))
        m = manager.Manager()
        log = tmp_path / ("log_%d.txt" % int(key))
        m.log_to_file(log)
        assert m.read_configuration_file(str(cfg))
        assert m.read_replay_items(path)
        assert m.decoder_counters() == dict(device_images=0, host_images=2 * n + 1, refused_images=1)
        # n + 2 records with a JPEG payload: the reader says once that it decodes on the host, and never when the key asks for the host
        assert log.read_text().count("The device JPEG decoder cannot be created") == (1 if key else 0)
