"""The map database file (lpslam_amd/host/map_file.cpp, layout in INTEGRATION.md "Map database file"): a small map written here with
struct, field by field as documented, is read by the library (lpslam_map_file_info), written back byte for byte
(lpslam_map_file_rewrite), and every damaged variant is rejected with its own reason."""
import struct

import numpy as np
import pytest

MAGIC = b"LPSLMAP\0"


def _fnv1a64(b):
    h = 1469598103934665603
    for x in b:
        h ^= x
        h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _map_bytes(version=1, bad_landmark_id=False, n_kp=5):
    rng = np.random.default_rng(3)
    b = bytearray(MAGIC)
    b += struct.pack("<I", version)
    b += struct.pack("<Iii", 1, 640, 480)                                    # stereo, resolution
    b += struct.pack("<5d", 500.0, 500.0, 320.0, 240.0, 60.0)                # fx fy cx cy focal_x_baseline
    b += struct.pack("<id", 4, 1.2)                                          # numLevels, scaleFactor
    n_kf, n_lm, next_id, segment = 3, 4, 6, 0
    b += struct.pack("<IIii", n_kf, n_lm, next_id, segment)
    lm_ids = [0, 2, 3, 5]
    for k in range(n_kf):
        if k == 1:
            b += struct.pack("<B", 1)                                        # erased: an empty record
            continue
        b += struct.pack("<B", 0)
        b += struct.pack("<4d3d", 1.0, 0.0, 0.0, 0.0, 0.1 * k, 0.0, 0.0)    # q (w x y z), t
        b += struct.pack("<iI", 0, n_kp)
        for i in range(n_kp):
            b += struct.pack("<5f2i", 10.0 * i, 20.0, 31.0, 45.0, 30.0, 0, -1)      # x y size angle response octave class_id
        b += rng.integers(0, 256, n_kp * 32, dtype=np.uint8).tobytes()
        b += struct.pack("<%df" % n_kp, *([300.0] * n_kp)) + struct.pack("<%df" % n_kp, *([5.0] * n_kp))
        lms = [lm_ids[i] if i < len(lm_ids) else -1 for i in range(n_kp)]
        if bad_landmark_id and k == 2:
            lms[1] = next_id                                                  # one past the last id
        b += struct.pack("<%di" % n_kp, *lms)
    for j, lid in enumerate(lm_ids):
        b += struct.pack("<i3d", lid, 1.0 * j, 0.5, 5.0)
        b += bytes(range(32))
        b += struct.pack("<3d2d", 0.0, 0.0, 1.0, 1.0, 20.0)                  # normal, min / max valid distance
        b += struct.pack("<iiiI", 0, 3, 2, 2)                                # ref_kf, n_observable, n_observed, observations
        b += struct.pack("<2i2i", 0, j, 2, j)                                # (keyframe, keypoint) x 2
    b += struct.pack("<Q", _fnv1a64(bytes(b)))
    return bytes(b)


@pytest.fixture(scope="module")
def mgr():
    from lpslam_amd import _build, manager
    _build.host_library()
    return manager


def test_map_file_counts_and_byte_identical_rewrite(mgr, tmp_path):
    p = tmp_path / "map.lpsmap"
    p.write_bytes(_map_bytes())
    ok, info = mgr.map_file_info(p)
    assert ok, info
    assert info == {"keyframes": 3, "live_keyframes": 2, "landmarks": 4, "next_landmark_id": 6, "stereo": 1}
    out = tmp_path / "again.lpsmap"
    assert mgr.map_file_rewrite(p, out) == (True, "")
    assert out.read_bytes() == p.read_bytes()
    assert not (tmp_path / "again.lpsmap.tmp").exists()             # written under <name>.tmp, then renamed


def test_map_file_rejections_each_say_why(mgr, tmp_path):
    good = _map_bytes()
    flipped = bytearray(good)
    flipped[200] ^= 0x10                                             # inside the first keyframe's keypoints
    cases = {
        "checksum": bytes(flipped),
        "truncated": good[:-40],
        "bad magic": b"LPSLMAQ\0" + good[8:],
        "unsupported format version": _map_bytes(version=2),
        "landmark id 6 out of range": _map_bytes(bad_landmark_id=True),
    }
    reasons = set()
    for want, data in cases.items():
        p = tmp_path / ("bad_%d.lpsmap" % len(reasons))
        p.write_bytes(data)
        ok, why = mgr.map_file_info(p)
        assert not ok and want in why, (want, why)
        reasons.add(why)
        assert mgr.map_file_rewrite(p, tmp_path / "never.lpsmap")[0] is False
    assert len(reasons) == len(cases)
    assert not (tmp_path / "never.lpsmap").exists()
    ok, why = mgr.map_file_info(tmp_path / "missing.lpsmap")
    assert not ok and "cannot open" in why
