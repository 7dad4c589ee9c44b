"""The map database through LpSlamManager (reference: src/Trackers/OpenVSLAMTrackerBase.cpp:241-255 load, :287-294 save): a stereo
session saves its map at stop, a later session loads it, relocalises against it without a pose prior (whole-map place ranking on the
device) and then tracks it -- localisation only with enableMapping off, extending it with mapping on.  The world of
synth.turning_sequence depends only on seq_id / n_points / radius, so another step_deg sees the same place from new angles."""
import hashlib
import math
import time

import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

W, H = 640, 480
CFG = '"cameraSetup": "%s", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 3, "localWindow": 4'


@pytest.fixture(scope="module")
def mgr(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    return manager


@pytest.fixture(scope="module")
def lap():
    return synth.turning_sequence(W, H, n_frames=120, step_deg=3.0)[0]


@pytest.fixture(scope="module")
def revisit():
    frames, yaws = synth.turning_sequence(W, H, n_frames=45, step_deg=2.0)
    return frames[20:45], yaws[20:45]                       # yaw 40 .. 88 degrees


def _manager(manager, cfg, log, stereo=True, fx_scale=1.0):
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in ((0, 1) if stereo else (0,)):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"] * fx_scale; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"] * fx_scale
        m.set_camera(c)
    assert m.add_tracker("VSLAMStereo" if stereo else "VSLAMMono", "{" + cfg + "}")
    m.collect_results(); m.provide_odometry()
    m.log_to_file(log)
    return m


def _feed(m, frames, stereo=True, step_ns=40_000_000):
    for i, f in enumerate(frames):
        assert m.add_stereo((i + 1) * step_ns, f[0], f[1]) if stereo else m.add_image((i + 1) * step_ns, f[0])
    t0 = time.time()
    while len(m.results) < len(frames) and time.time() - t0 < 60:
        time.sleep(0.01)


def _sha(p):
    return hashlib.sha256(p.read_bytes()).hexdigest()


def _stats(manager, log):
    return manager.Manager.statistics(log)


@pytest.fixture(scope="module")
def saved(mgr, lap, tmp_path_factory):
    d = tmp_path_factory.mktemp("mapdb")
    path = d / "place.lpsmap"
    log = d / "save.log"
    m = _manager(mgr, CFG % "stereo" + ', "mapFilename": "%s"' % path, log)
    m.start(); _feed(m, lap); m.stop()
    return path, _stats(mgr, log)


def test_save_writes_the_map(mgr, saved):
    path, st = saved
    assert path.exists(), "no map file written at stop"
    ok, info = mgr.map_file_info(path)
    assert ok, info
    assert info["live_keyframes"] == st["live_keyframes"] and info["landmarks"] == st["landmarks"] and info["stereo"] == 1
    assert info["landmarks"] > 500 and info["live_keyframes"] >= 5


def _check_poses(results, yaws, frames_from=0):
    errs = []
    for r, yaw in zip(results[frames_from:], yaws[frames_from:]):
        if not r["valid"]:
            continue
        q = np.array(r["q"])
        ang = 2 * math.degrees(math.acos(min(1.0, abs(float(q[0])))))
        errs.append((abs(ang - math.degrees(yaw)), max(abs(v) for v in r["p"])))
    return errs


def test_localise_only_against_a_loaded_map(mgr, saved, revisit, tmp_path):
    path, st = saved
    before = _sha(path)
    frames, yaws = revisit
    log = tmp_path / "loc.log"
    m = _manager(mgr, CFG % "stereo" + ', "mapFilename": "%s", "enableMapping": false' % path, log)
    m.start()
    assert m.features_count() == st["landmarks"]            # the map is there before the first frame
    _feed(m, frames); m.stop()
    s = _stats(mgr, log)
    assert s["relocalised"] >= 1 and s["keyframes"] == 0 and s["reinitialised"] == 0
    first_valid = next(i for i, r in enumerate(m.results) if r["valid"])
    assert first_valid <= 3, first_valid
    errs = _check_poses(m.results, yaws)
    assert len(errs) >= len(frames) - 4
    # the bounds start from 1 degree / 0.1 m and are tightened to 0.5 degrees / 0.05 m, which the MI355X run meets
    assert max(e[0] for e in errs) < 0.5 and max(e[1] for e in errs) < 0.05, max(errs)
    assert _sha(path) == before                             # localisation only: nothing saved


def test_resume_mapping_on_a_loaded_map(mgr, saved, revisit, tmp_path):
    path0, st = saved
    path = tmp_path / "resume.lpsmap"
    path.write_bytes(path0.read_bytes())
    frames, yaws = revisit
    log = tmp_path / "resume.log"
    m = _manager(mgr, CFG % "stereo" + ', "mapFilename": "%s"' % path, log)
    m.start(); _feed(m, frames); m.stop()
    s = _stats(mgr, log)
    assert s["relocalised"] >= 1 and s["keyframes"] >= 1 and s["reinitialised"] == 0
    ok, info = mgr.map_file_info(path)
    assert ok and info["keyframes"] > mgr.map_file_info(path0)[1]["keyframes"]
    errs = _check_poses(m.results, yaws)
    assert len(errs) >= len(frames) - 4 and max(e[0] for e in errs) < 1.0 and max(e[1] for e in errs) < 0.1


def test_round_trip_without_frames_is_byte_identical(mgr, saved, tmp_path):
    path0, _ = saved
    path = tmp_path / "rt.lpsmap"
    path.write_bytes(path0.read_bytes())
    m = _manager(mgr, CFG % "stereo" + ', "mapFilename": "%s"' % path, tmp_path / "rt.log")
    m.start(); m.stop()
    assert path.read_bytes() == path0.read_bytes()


def test_off_and_rejected(mgr, saved, lap, tmp_path):
    path0, st = saved
    # useMapDb off: nothing read, nothing written
    path = tmp_path / "off.lpsmap"
    path.write_bytes(path0.read_bytes())
    before = _sha(path)
    m = _manager(mgr, CFG % "stereo" + ', "useMapDb": false, "mapFilename": "%s"' % path, tmp_path / "off.log")
    m.start()
    assert m.features_count() == 0
    _feed(m, lap[:10]); m.stop()
    assert _sha(path) == before
    fresh = tmp_path / "none.lpsmap"
    m = _manager(mgr, CFG % "stereo" + ', "useMapDb": false, "mapFilename": "%s"' % fresh, tmp_path / "off2.log")
    m.start(); _feed(m, lap[:10]); m.stop()
    assert not fresh.exists()
    # another camera (fx): rejected, the session starts empty, the file is not overwritten
    log = tmp_path / "rej.log"
    m = _manager(mgr, CFG % "stereo" + ', "mapFilename": "%s"' % path, log, fx_scale=1.05)
    m.start()
    assert m.features_count() == 0
    _feed(m, lap[:10]); m.stop()
    assert _sha(path) == before
    assert "another camera" in log.read_text()


def test_filename_through_mapping_set_filename(mgr, saved, tmp_path):
    """mappingSetFilename names the file as the mapFilename key does; mappingSetMode(false) is localisation only"""
    path0, st = saved
    path = tmp_path / "set.lpsmap"
    path.write_bytes(path0.read_bytes())
    m = _manager(mgr, CFG % "stereo", tmp_path / "set.log")
    assert m.mapping_set_filename(path) and m.mapping_set_mode(False)
    m.start()
    assert m.features_count() == st["landmarks"]
    m.stop()
    assert path.read_bytes() == path0.read_bytes()


def test_monocular_save_and_load(mgr, lap, tmp_path):
    path = tmp_path / "mono.lpsmap"
    log = tmp_path / "mono.log"
    mono = [(f[0],) for f in lap[:60]]
    m = _manager(mgr, CFG % "monocular" + ', "mapFilename": "%s"' % path, log, stereo=False)
    m.start(); _feed(m, mono, stereo=False); m.stop()
    st = _stats(mgr, log)
    ok, info = mgr.map_file_info(path)
    assert ok and info["stereo"] == 0 and info["landmarks"] == st["landmarks"] and info["live_keyframes"] == st["live_keyframes"]
    m = _manager(mgr, CFG % "monocular" + ', "mapFilename": "%s", "enableMapping": false' % path, tmp_path / "mono2.log", stereo=False)
    m.start()
    assert m.features_count() == st["landmarks"]
    m.stop()
    # a monocular map is refused by the stereo tracker (camera setup)
    m = _manager(mgr, CFG % "stereo" + ', "mapFilename": "%s"' % path, tmp_path / "mono3.log")
    m.start()
    assert m.features_count() == 0
    m.stop()
    assert mgr.map_file_info(path)[1]["stereo"] == 0


def test_localise_with_a_vocabulary(mgr, saved, revisit, tmp_path):
    """with vocabFile the loaded keyframes' BoW vectors are rebuilt and relocalisation asks the BoW database"""
    import os
    from conftest import GOLDEN
    path, st = saved
    voc = os.path.join(GOLDEN, "vocab_k10_L3.dbow2")
    frames, yaws = revisit
    log = tmp_path / "voc.log"
    m = _manager(mgr, CFG % "stereo" + ', "mapFilename": "%s", "enableMapping": false, "vocabFile": "%s"' % (path, voc), log)
    m.start(); _feed(m, frames); m.stop()
    s = _stats(mgr, log)
    assert s["relocalised"] >= 1 and s["keyframes"] == 0
    errs = _check_poses(m.results, yaws)
    assert len(errs) >= len(frames) // 2 and max(e[0] for e in errs) < 1.0 and max(e[1] for e in errs) < 0.1
