"""CPU tests of the fisheye keypoint camera of the monocular tracker: the host forms of
lpslam_amd/csrc/fisheye_math.h against tests/fisheye_ref.py, the configuration paths, the version-2 map file, and the stand-alone
sanitizer program tests/cpp/fisheye_host_main.cpp."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import fisheye_ref as fr
from test_host_cpu import _cam
from test_map_file_cpu import _fnv1a64, _map_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 848, 800


def cam_model(max_angle_deg=70.0, **over):
    c = _cam(**over)
    return fr.Model(c["fx"], c["fy"], c["cx"], c["cy"], c["distortion"], max_angle_deg)


# a coefficient set whose derivative polynomial 1 + 3 k1 t^2 changes sign inside (0, pi/2), at t = 0.577: theta (1 - theta^2) has its
# maximum 0.385 there, so a pixel with theta_d > 0.385 has NO root on the positive side -- Newton wanders or lands on the negative root
BAD_K = (-1.0, 0.0, 0.0, 0.0)
BAD_PIXELS = [(416.94 + 286.18 * 0.5, 403.27), (416.94, 403.27 - 286.39 * 0.9), (416.94 + 286.18 * 0.8, 403.27 + 286.39 * 0.8), (600.0, 700.0)]

FIXED_PIXELS = [(416.94, 403.27), (416.94 + 1e-7, 403.27), (0.0, 0.0), (847.0, 799.0), (100.5, 650.25), (424.0, 400.0), (640.0, 120.0), (30.0, 410.0),
                (0.0, 400.0), (847.0, 400.0), (424.0, 0.0), (424.0, 799.0)]      # the last four: the mid-edge pixels


def planted_pixels(m):
    """pixels placed on purpose: the fixed list, either side of the angle limit, and 2000 seeded ones"""
    rng = np.random.default_rng(7)
    edge = [fr.pixel_at(m, m.max_angle + s * 1e-6, phi) for s in (-1, 1) for phi in (0.0, 1.0, 2.5, 4.0)]
    rnd = np.stack([rng.uniform(0, W, 2000), rng.uniform(0, H, 2000)], 1)
    return np.concatenate([np.array(FIXED_PIXELS), np.array(edge), rnd])


@pytest.fixture(scope="module")
def mgr(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    manager.load()
    return manager


def check_against_ref(mgr, m, xy):
    r = fr.undistort(m, xy)
    out, valid, theta = mgr.fisheye_undistort(m.as_array(), xy)
    dec = fr.decisive(m, r)
    assert (~dec).sum() == 0                                         # the planted lists hide nothing
    assert (valid == r["valid"]).all(), np.flatnonzero(valid != r["valid"])
    assert np.isnan(out[~valid]).all()
    # both sides compute in FP64 and differ by a few FP64 ulps of tan and hypot at the most: only the final rounding can flip
    assert fr.ulp_diff(out[valid], r["out"][valid]).max(initial=0) <= 1
    return r, out, valid


def test_host_undistort_matches_reference(mgr):
    m = cam_model()
    xy = planted_pixels(m)
    r, out, valid = check_against_ref(mgr, m, xy)
    assert valid[0] and valid[1]                                     # the principal point and a pixel 1e-7 from it: the theta_d <= 1e-8 branch
    assert out[0, 0] == np.float32(m.cx) and out[0, 1] == np.float32(m.cy)
    assert r["theta_d0"][1] <= fr.EPS and r["theta_d0"][1] > 0
    n_fixed = len(FIXED_PIXELS)
    assert not valid[n_fixed - 4:n_fixed].any()                      # the four mid-edge pixels: three beyond 90 degrees with this calibration, the bottom one at 87
    assert (r["theta"][n_fixed - 4:n_fixed] > np.deg2rad(87.0)).all() and (r["theta"][n_fixed - 4:n_fixed - 1] > fr.HALF_PI).all()
    assert valid[n_fixed:n_fixed + 4].all() and not valid[n_fixed + 4:n_fixed + 8].any()      # 1e-6 rad inside / outside the angle limit
    share_out = 1.0 - valid[n_fixed + 8:].mean()
    assert 0.35 < share_out < 0.55                                   # about 45 % of uniformly drawn pixels fall outside 70 degrees


def test_half_pi_rule(mgr):
    """theta_d0 1e-6 either side of pi/2, with coefficients that keep theta itself small: only the theta_d0 rule separates them"""
    m = fr.Model(286.18, 286.39, 416.94, 403.27, (0.5, 0.0, 0.0, 0.0), 70.0)
    xy = np.array([[m.cx + m.fx * (fr.HALF_PI - 1e-6), m.cy], [m.cx + m.fx * (fr.HALF_PI + 1e-6), m.cy],
                   [m.cx, m.cy - m.fy * (fr.HALF_PI - 1e-6)], [m.cx, m.cy - m.fy * (fr.HALF_PI + 1e-6)]])
    r, out, valid = check_against_ref(mgr, m, xy)
    assert list(valid) == [True, False, True, False]
    assert (r["converged"]).all() and (r["theta"] < m.max_angle).all()


def test_zero_coefficients_are_f_tan(mgr):
    m = fr.Model(300.0, 310.0, 320.0, 240.0, (0, 0, 0, 0), 80.0)
    rng = np.random.default_rng(11)
    xy = np.stack([rng.uniform(0, 640, 500), rng.uniform(0, 480, 500)], 1)
    r, out, valid = check_against_ref(mgr, m, xy)
    assert valid.all()
    x = (xy[:, 0] - m.cx) / m.fx; y = (xy[:, 1] - m.cy) / m.fy
    td = np.hypot(x, y)
    want = np.stack([m.fx * x * (np.tan(td) / td) + m.cx, m.fy * y * (np.tan(td) / td) + m.cy], 1).astype(np.float32)
    assert fr.ulp_diff(out, want).max() <= 1


def test_sign_change_of_the_derivative_is_invalid(mgr):
    m = fr.Model(286.18, 286.39, 416.94, 403.27, BAD_K, 70.0)
    xy = np.array(BAD_PIXELS)
    r = fr.undistort(m, xy)
    assert (r["theta_d0"] > 0.3850).all() and (r["theta_d0"] < fr.HALF_PI).all()      # above the maximum of theta (1 - theta^2): no positive root
    assert (~r["converged"] | (r["theta"] < 0)).all(), (r["converged"], r["theta"])   # the reference's Newton does not converge, or flips
    out, valid, theta = mgr.fisheye_undistort(m.as_array(), xy)
    assert not valid.any() and not r["valid"].any()


def test_forward_then_undistort_round_trips(mgr):
    m = cam_model()
    rng = np.random.default_rng(5)
    theta = rng.uniform(0.0, m.max_angle - 1e-3, 1000); phi = rng.uniform(0, 2 * np.pi, 1000); z = rng.uniform(0.5, 20.0, 1000)
    xyz = np.stack([z * np.tan(theta) * np.cos(phi), z * np.tan(theta) * np.sin(phi), z], 1)
    s_ref, th_ref, vis_ref = fr.forward(m, xyz, 10 ** 6, 10 ** 6)
    s, th, vis = mgr.fisheye_forward(m.as_array(), xyz, 10 ** 6, 10 ** 6)
    assert np.abs(s - s_ref).max() < 1e-9 and np.abs(th - th_ref).max() < 1e-12
    out, valid, _ = mgr.fisheye_undistort(m.as_array(), s)
    assert valid.all()
    u = m.fx * xyz[:, 0] / xyz[:, 2] + m.cx; v = m.fy * xyz[:, 1] / xyz[:, 2] + m.cy
    # Newton stops within 1e-8 rad of the root: at 70 degrees that is 286 * 1e-8 / cos^2 = 2.4e-5 px; the float32 rounding of a position
    # below 2048 adds 6.1e-5 px
    assert np.abs(out[:, 0] - u).max() < 1e-4 and np.abs(out[:, 1] - v).max() < 1e-4


def test_visibility_at_the_sensor_edges_and_the_angle_limit(mgr):
    # a sensor window whose edges lie inside the angle limit (about 60 degrees at the mid-edges)
    Ws, Hs = 600, 560
    m = fr.Model(286.18, 286.39, 300.0, 280.0, _cam()["distortion"], 89.0)
    px = np.array([[0.01, 280.0], [-0.01, 280.0], [599.99, 280.0], [600.01, 280.0], [300.0, 0.01], [300.0, -0.01], [300.0, 559.99], [300.0, 560.01]])
    r = fr.undistort(m, px)
    assert r["valid"].all()
    rays = np.stack([(r["out"][:, 0].astype(np.float64) - m.cx) / m.fx, (r["out"][:, 1].astype(np.float64) - m.cy) / m.fy, np.ones(len(px))], 1) * 3.0
    want = [True, False, True, False, True, False, True, False]
    s, th, vis = mgr.fisheye_forward(m.as_array(), rays, Ws, Hs)
    assert list(vis) == want and list(fr.forward(m, rays, Ws, Hs)[2]) == want
    # the angle limit, where the sensor pixel is well inside the image
    m50 = fr.Model(286.18, 286.39, 300.0, 280.0, _cam()["distortion"], 50.0)
    th = np.array([m50.max_angle - 1e-6, m50.max_angle + 1e-6])
    rays = np.stack([np.tan(th), np.zeros(2), np.ones(2)], 1)
    s, th_out, vis = mgr.fisheye_forward(m50.as_array(), rays, Ws, Hs)
    assert list(vis) == [True, False] and (s[:, 0] < Ws - 10).all()
    # behind the camera, and on the axis
    s, th_out, vis = mgr.fisheye_forward(m50.as_array(), np.array([[0.1, 0.1, -1.0], [0.0, 0.0, 2.0]]), Ws, Hs)
    assert list(vis) == [False, True] and s[1, 0] == 300.0 and s[1, 1] == 280.0


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_configuration_paths(mgr, tmp_path):
    # JSON: cameras[] + a VSLAMMono tracker that sets the angle limit
    m = mgr.Manager()
    cfg = {"trackers": [{"type": "VSLAMMono", "configuration": {"fisheyeMaxAngleDeg": 60.0}}], "cameras": [_cam()]}
    assert m.read_configuration_file(_write(tmp_path, "fe.json", json.dumps(cfg)))
    rc, model = mgr.fisheye_session_model(m, None, 60.0)
    assert rc == 1
    c = _cam()
    assert list(model[:8]) == [c["fx"], c["fy"], c["cx"], c["cy"]] + c["distortion"] and abs(model[8] - np.deg2rad(60.0)) < 1e-15
    # the angle limit out of range is refused: (0, 89]
    for bad in (0.0, -5.0, 89.5, 120.0, float("nan")):
        rc, why = mgr.fisheye_session_model(m, None, bad)
        assert rc == -1 and "fisheyeMaxAngleDeg" in why, (bad, rc, why)
    assert mgr.fisheye_session_model(m, None, 89.0)[0] == 1
    # every other model reaches the monocular tracker without coefficients
    for other in ("perspective", "no_distortion"):
        m2 = mgr.Manager()
        assert m2.read_configuration_file(_write(tmp_path, other + ".json", json.dumps({"cameras": [_cam(model=other)]})))
        assert mgr.fisheye_session_model(m2, None, 70.0) == (0, None)
    # the YAML keys of the file-configuration path, nested and flat, over a camera that says nothing
    m3 = mgr.Manager()
    assert m3.read_configuration_file(_write(tmp_path, "p.json", json.dumps({"cameras": [_cam(model="perspective", distortion=[0.0] * 4)]})))
    nested = _write(tmp_path, "n.yaml", "Camera:\n  model: fisheye\n  k1: -0.01\n  k2: 0.02\n  k3: -0.03\n  k4: 0.004\n")
    flat = _write(tmp_path, "f.yaml", "Camera.model: \"fisheye\"\nCamera.k1: -0.01\nCamera.k2: 0.02\nCamera.k3: -0.03\nCamera.k4: 0.004\n")
    for path in (nested, flat):
        rc, model = mgr.fisheye_session_model(m3, path, 70.0)
        assert rc == 1 and list(model[4:8]) == [-0.01, 0.02, -0.03, 0.004], (path, rc, model)
    rc, why = mgr.fisheye_session_model(m3, _write(tmp_path, "b.yaml", "Camera.model: fisheye\nCamera.k2: much\n"), 70.0)
    assert rc == -1 and "Camera.k2" in why
    assert mgr.fisheye_session_model(m, _write(tmp_path, "pp.yaml", "Camera:\n  model: perspective\n"), 70.0) == (0, None)


def _map_bytes_v2(k=(-0.0115, 0.0479, -0.0451, 0.0083), max_angle=np.deg2rad(70.0), model=1):
    """_map_bytes of test_map_file_cpu with the version-2 camera record: model (u32), k[4] (f64), max_angle (f64) behind scale_factor"""
    v1 = _map_bytes()
    head = 8 + 4 + 12 + 40 + 12                                      # magic, version, stereo + resolution, five doubles, levels + scale
    b = bytearray(v1[:8]) + struct.pack("<I", 2) + v1[12:head] + struct.pack("<I4dd", model, *k, max_angle) + v1[head:-8]
    b[12:16] = struct.pack("<I", 0)                                  # a monocular session
    return bytes(b) + struct.pack("<Q", _fnv1a64(bytes(b)))


SESSION_V1 = [1, 640, 480, 500.0, 500.0, 320.0, 240.0, 60.0, 4, 1.2, 0, 0, 0, 0, 0, 0]
SESSION_V2 = [0, 640, 480, 500.0, 500.0, 320.0, 240.0, 60.0, 4, 1.2, 1, -0.0115, 0.0479, -0.0451, 0.0083, float(np.deg2rad(70.0))]


def test_map_file_version_2_round_trip_and_version_1_unchanged(mgr, tmp_path):
    p2 = tmp_path / "fe.lpsmap"
    p2.write_bytes(_map_bytes_v2())
    ok, info = mgr.map_file_info(p2)
    assert ok and info["keyframes"] == 3 and info["stereo"] == 0, info
    out = tmp_path / "fe_again.lpsmap"
    assert mgr.map_file_rewrite(p2, out) == (True, "")
    assert out.read_bytes() == p2.read_bytes() and out.read_bytes()[8:12] == struct.pack("<I", 2)
    # a pinhole session's file: version 1, the bytes the format has always had (written here field by field, as before this record existed)
    p1 = tmp_path / "ph.lpsmap"
    p1.write_bytes(_map_bytes())
    out1 = tmp_path / "ph_again.lpsmap"
    assert mgr.map_file_rewrite(p1, out1) == (True, "")
    assert out1.read_bytes() == _map_bytes() and out1.read_bytes()[8:12] == struct.pack("<I", 1)
    assert len(p2.read_bytes()) == len(p1.read_bytes()) + 4 + 40
    assert mgr.map_file_camera_check(p1, SESSION_V1) == (1, "") and mgr.map_file_camera_check(p2, SESSION_V2) == (1, "")


def test_map_file_camera_model_rejections(mgr, tmp_path):
    p1 = tmp_path / "ph.lpsmap"; p1.write_bytes(_map_bytes())
    p2 = tmp_path / "fe.lpsmap"; p2.write_bytes(_map_bytes_v2())
    fisheye_stereo_shape = list(SESSION_V1); fisheye_stereo_shape[10:] = SESSION_V2[10:]
    assert mgr.map_file_camera_check(p1, fisheye_stereo_shape) == (0, "camera model")      # a version-1 file in a fisheye session
    pinhole_mono = list(SESSION_V2); pinhole_mono[10:] = [0] * 6
    assert mgr.map_file_camera_check(p2, pinhole_mono) == (0, "camera model")              # a fisheye file in a pinhole session
    other_k = list(SESSION_V2); other_k[12] = 0.05
    assert mgr.map_file_camera_check(p2, other_k) == (0, "camera model")
    other_angle = list(SESSION_V2); other_angle[15] = float(np.deg2rad(60.0))
    assert mgr.map_file_camera_check(p2, other_angle) == (0, "camera model")
    other_fx = list(SESSION_V2); other_fx[3] = 501.0
    assert mgr.map_file_camera_check(p2, other_fx) == (0, "intrinsics")                    # the earlier checks keep their reasons and their order
    # a version-2 file that names another model, and one cut inside the new record
    p3 = tmp_path / "m2.lpsmap"; p3.write_bytes(_map_bytes_v2(model=2))
    ok, why = mgr.map_file_info(p3)
    assert not ok and "unsupported format version 2 with camera model 2" in why
    p4 = tmp_path / "cut.lpsmap"; p4.write_bytes(_map_bytes_v2()[:100])
    ok, why = mgr.map_file_info(p4)
    assert not ok and "truncated" in why
    assert mgr.map_file_camera_check(p4, SESSION_V2)[0] == -1


def test_standalone_sanitizer_program(mgr, tmp_path):
    """tests/cpp/fisheye_host_main.cpp: the host forms and the map-file reader in a program of its own, built with
    -fsanitize=address,undefined, on cases this test writes: pixels with the reference's answers, and the two map files"""
    m = cam_model()
    xy = planted_pixels(m)[:200]
    r = fr.undistort(m, xy)
    cases = tmp_path / "cases.txt"
    with open(cases, "w") as f:
        f.write("%d\n" % len(xy))
        f.write(" ".join(repr(float(v)) for v in m.as_array()) + "\n")
        for p, o, v in zip(xy, r["out"], r["valid"]):
            f.write("%r %r %d %d %d\n" % (float(p[0]), float(p[1]), int(v), int(o[0].view(np.int32)) if v else 0, int(o[1].view(np.int32)) if v else 0))
    p1 = tmp_path / "ph.lpsmap"; p1.write_bytes(_map_bytes())
    p2 = tmp_path / "fe.lpsmap"; p2.write_bytes(_map_bytes_v2())
    p3 = tmp_path / "cut.lpsmap"; p3.write_bytes(_map_bytes_v2()[:100])
    exe = tmp_path / "fisheye_host_main"
    host = os.path.join(ROOT, "lpslam_amd", "host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "fisheye_host_main.cpp"), os.path.join(host, "map_file.cpp")])
    out = subprocess.run([str(exe), str(cases), str(p1), str(p2), str(p3)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "points ok 200" in out.stdout and "maps ok" in out.stdout, out.stdout
