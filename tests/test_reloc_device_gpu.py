"""The tracker option relocaliseOnDevice: a stereo session saves its map, later sessions load it with
enableMapping off -- they start Lost and relocalise -- once with the candidates' pose solver on the host (the default), once in one
device call per Lost frame (lpslam_hip_pnp_ransac_batch).  By construction the outcome is the same.  The session is the one of
tests/test_map_db_gpu.py (synth.turning_sequence: the world depends on seq_id / n_points / radius only)."""
import math
import time

import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

W, H = 640, 480
CFG = '"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 3, "localWindow": 4'


@pytest.fixture(scope="module")
def mgr(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    return manager


def _manager(manager, cfg, log):
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in (0, 1):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    assert m.add_tracker("VSLAMStereo", "{" + cfg + "}")
    m.collect_results(); m.provide_odometry()
    m.log_to_file(log)
    return m


def _feed(m, frames, step_ns=40_000_000):
    for i, f in enumerate(frames):
        assert m.add_stereo((i + 1) * step_ns, f[0], f[1])
    t0 = time.time()
    while len(m.results) < len(frames) and time.time() - t0 < 60:
        time.sleep(0.01)


@pytest.fixture(scope="module")
def runs(mgr, tmp_path_factory):
    """the statistics and results of three localisation-only sessions on one saved map: option false, true, absent"""
    d = tmp_path_factory.mktemp("reloc")
    path = d / "place.lpsmap"
    m = _manager(mgr, CFG + ', "mapFilename": "%s"' % path, d / "save.log")
    m.start(); _feed(m, synth.turning_sequence(W, H, n_frames=120, step_deg=3.0)[0]); m.stop()
    assert path.exists()
    frames, yaws = synth.turning_sequence(W, H, n_frames=45, step_deg=2.0)
    frames, yaws = frames[20:45], yaws[20:45]
    out = {}
    for name, extra in (("host", ', "relocaliseOnDevice": false'), ("device", ', "relocaliseOnDevice": true'), ("absent", "")):
        log = d / (name + ".log")
        m = _manager(mgr, CFG + ', "mapFilename": "%s", "enableMapping": false' % path + extra, log)
        m.start(); _feed(m, frames); m.stop()
        out[name] = (mgr.Manager.statistics(log), list(m.results))
    return out, yaws


def _first_valid(results):
    i = next(i for i, r in enumerate(results) if r["valid"])
    return i, np.array(results[i]["q"], float), np.array(results[i]["p"], float)


def test_the_device_solver_relocalises_like_the_host_solver(runs):
    out, _ = runs
    (sh, rh), (sd, rd) = out["host"], out["device"]
    assert sh["relocalised"] >= 1
    assert sd["relocalised"] == sh["relocalised"] and sd["lost"] == sh["lost"]
    assert sum(r["valid"] for r in rd) == sum(r["valid"] for r in rh)
    (ih, qh, ph), (i_d, qd, pd) = _first_valid(rh), _first_valid(rd)
    assert i_d == ih
    # the tolerance of tests/test_map_db_gpu.py for a reloaded session's poses: 0.5 degrees, 0.05 m
    dot = min(1.0, abs(float(np.dot(qh, qd))))
    assert 2 * math.degrees(math.acos(dot)) < 0.5 and np.abs(ph - pd).max() < 0.05


def test_the_batch_entry_point_ran_only_with_the_option_on(runs):
    out, _ = runs
    assert out["device"][0]["pnp_batches"] >= 1 and out["device"][0]["reloc_frames"] >= out["device"][0]["pnp_batches"]
    assert out["host"][0]["pnp_batches"] == 0 and out["host"][0]["reloc_frames"] == out["device"][0]["reloc_frames"]


def test_the_option_absent_is_the_option_off(runs):
    out, _ = runs
    (sh, rh), (sa, ra) = out["host"], out["absent"]
    assert sa["pnp_batches"] == 0 and sa["relocalised"] == sh["relocalised"] and sa["lost"] == sh["lost"]
    assert [r["valid"] for r in ra] == [r["valid"] for r in rh]
    (ih, qh, ph), (ia, qa, pa) = _first_valid(rh), _first_valid(ra)
    assert ia == ih and min(1.0, abs(float(np.dot(qh, qa)))) > math.cos(math.radians(0.25)) and np.abs(ph - pa).max() < 0.05
