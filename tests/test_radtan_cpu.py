"""CPU tests of the radial-tangential keypoint camera of the monocular tracker: the host forms of
lpslam_amd/csrc/radtan_math.h against tests/radtan_ref.py, the visibility rule and the bounds, the configuration-file keys, the
version-3 map file, and the stand-alone sanitizer program tests/cpp/radtan_host_main.cpp."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import radtan_ref as rr
from test_fisheye_cpu import SESSION_V1, SESSION_V2, _map_bytes_v2
from test_host_cpu import _cam
from test_map_file_cpu import _fnv1a64, _map_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480
# a barrel lens whose polynomial folds over OUTSIDE the image (r (1 - 0.18 r^2) has its maximum at r = 1.361; the corner lies at 0.769)
BARREL = rr.Model(520.0, 520.0, 320.0, 240.0, -0.18)
PINCUSHION = rr.Model(520.0, 520.0, 320.0, 240.0, 0.08)


def planted_points(n=200000, seed=7):
    """seeded float32 points from [-20, 660) x [-20, 500): beyond every edge of the image"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-20, 660, n), rng.uniform(-20, 500, n)], 1).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def mgr(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    manager.load()
    return manager


def check_against_ref(mgr, m, xy):
    r = rr.undistort(m, xy)
    out, valid, res2, min_den = mgr.radtan_undistort(m.as_array(), xy)
    dec = rr.decisive(r)
    assert (~dec).sum() == 0                                         # the planted points hide nothing
    assert (valid == r["valid"]).all(), np.flatnonzero(valid != r["valid"])[:10]
    assert np.isnan(out[~valid]).all()
    # both sides run the same five steps in FP64: only the final rounding can differ
    assert rr.ulp_diff(out[valid], r["out"][valid]).max(initial=0) <= 1
    return r, out, valid


def test_host_undistort_matches_reference_mild(mgr):
    xy = planted_points()
    r, out, valid = check_against_ref(mgr, rr.MILD, xy)
    assert valid.all() and r["res2"].max() < 0.25 ** 2              # every point valid, the largest residual under a quarter of a pixel
    inside = (xy[:, 0] >= 0) & (xy[:, 0] < W) & (xy[:, 1] >= 0) & (xy[:, 1] < H)
    assert np.sqrt(r["res2"][inside].max()) < 0.14                   # (0.134 px at the corner of the image)
    # the principal point maps to itself
    out0, valid0, _, _ = mgr.radtan_undistort(rr.MILD.as_array(), np.array([[320.0, 240.0]]))
    assert valid0[0] and out0[0, 0] == 320.0 and out0[0, 1] == 240.0


def test_host_undistort_matches_reference_fold_over(mgr):
    xy = planted_points()
    r, out, valid = check_against_ref(mgr, rr.FOLD, xy)
    nonpos = ~(r["den"] > 0).all(axis=1)
    far = (r["den"] > 0).all(axis=1) & ~(r["res2"] <= rr.MAX_RES2)
    # every branch of the rule is reached: valid points, a non-positive denominator, and a result that does not map back
    assert 0.25 < valid.mean() < 0.40 and 0.30 < nonpos.mean() < 0.40 and far.mean() > 0.2
    print("fold-over: %.1f %% valid, %.1f %% with a non-positive denominator, %.1f %% beyond half a pixel; closest residual margin %.2g, closest |den| %.2g"
          % (100 * valid.mean(), 100 * nonpos.mean(), 100 * far.mean(), np.nanmin(np.abs(r["res2"] - rr.MAX_RES2)), np.nanmin(np.abs(r["den"]))))


def test_zero_coefficients_are_the_identity_and_non_finite_pixels_invalid(mgr):
    m = rr.Model(400.0, 410.0, 320.0, 240.0)
    xy = planted_points(500, 11)
    out, valid, res2, _ = mgr.radtan_undistort(m.as_array(), xy)
    assert valid.all() and rr.ulp_diff(out, xy.astype(np.float32)).max() <= 1
    out, valid, _, _ = mgr.radtan_undistort(rr.MILD.as_array(), np.array([[np.nan, 1.0], [np.inf, 2.0], [3.0, -np.inf], [1e200, 1e200]]))
    assert not valid.any() and np.isnan(out).all()
    assert not rr.undistort(rr.MILD, np.array([[np.nan, 1.0], [np.inf, 2.0], [3.0, -np.inf], [1e200, 1e200]]))["valid"].any()


def test_forward_matches_reference_and_round_trips(mgr):
    m = rr.MILD
    rng = np.random.default_rng(5)
    b, _ = rr.bounds(m, W, H)
    z = rng.uniform(0.5, 20.0, 1000)
    xyz = np.stack([z * rng.uniform(-0.6, 0.6, 1000), z * rng.uniform(-0.45, 0.45, 1000), z], 1)
    s, vis = mgr.radtan_forward(m.as_array(), xyz, b, W, H)
    assert np.abs(s - rr.forward(m, xyz)).max() < 1e-9 and (vis == rr.visible(m, b, xyz, W, H)).all()
    out, valid, res2, _ = mgr.radtan_undistort(m.as_array(), s[vis])
    assert valid.all()
    u = m.fx * xyz[vis, 0] / xyz[vis, 2] + m.cx; v = m.fy * xyz[vis, 1] / xyz[vis, 2] + m.cy
    # five steps leave up to 0.134 px of residual on the sensor at the corner of this lens; the undistorted
    # position is off by that times the local magnification, under 1.5 here
    assert np.hypot(out[:, 0] - u, out[:, 1] - v).max() < 0.134 * 1.5


def test_visibility(mgr):
    m = BARREL
    b, share = mgr.radtan_bounds(m.as_array(), W, H)
    assert b is not None and share == 0.0
    pts = np.array([
        [2.0, 0.0, 1.0],        # far off axis: the polynomial folds it back to 320 + 520 * 2 * (1 - 0.18 * 4) = 611.2 on the sensor
        [-2.1, 0.2, 1.0],       # likewise on the other side
        [0.7115, 0.0, 1.0],     # u = 690: inside the bounds box (the corners reach further) but the sensor pixel 320 + 520 * 0.6467 = 656 is off the image
        [0.0, -0.48, 1.0],      # v = -9.6, above the top edge of the image and inside the box: sensor row 240 - 520 * 0.4601 = 0.76 is inside -> visible
        [0.1, 0.1, -1.0], [0.1, 0.1, 0.0],      # behind the camera, and in its plane
        [0.0, 0.0, 2.0], [0.3, -0.2, 5.0],      # on the axis, and an ordinary point
    ])
    want = [False, False, False, True, False, False, True, True]
    s, vis = mgr.radtan_forward(m.as_array(), pts, b, W, H)
    assert list(vis) == want and list(rr.visible(m, b, pts, W, H)) == want
    # what rejects each one: the first two have their SENSOR pixel inside the image -- only the bounds reject them
    assert ((s[:2, 0] >= 0) & (s[:2, 0] < W) & (s[:2, 1] >= 0) & (s[:2, 1] < H)).all()
    u = m.fx * pts[:3, 0] + m.cx
    assert u[0] > b[1] and u[1] < b[0] and b[0] <= u[2] <= b[1] and s[2, 0] >= W
    assert s[6, 0] == 320.0 and s[6, 1] == 240.0


def test_bounds_of_barrel_and_pincushion_lenses(mgr):
    corners = np.array([[0.0, 0.0], [W - 1.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0]])
    mid = np.array([[0.0, 240.0], [W - 1.0, 240.0], [320.0, 0.0], [320.0, H - 1.0]])
    for m, where in ((BARREL, "corners"), (PINCUSHION, "mid-edges"), (rr.MILD, "corners")):
        b, share = mgr.radtan_bounds(m.as_array(), W, H)
        b_ref, share_ref = rr.bounds(m, W, H)
        assert b == b_ref and share == share_ref == 0.0
        c = rr.undistort(m, corners)["out"].astype(np.float64); e = rr.undistort(m, mid)["out"].astype(np.float64)
        if where == "corners":
            assert b == (c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max())
            assert e[0, 0] > b[0] + 5 and e[1, 0] < b[1] - 5 and e[2, 1] > b[2] + 5 and e[3, 1] < b[3] - 5
        else:
            assert b == (e[0, 0], e[1, 0], e[2, 1], e[3, 1])
            assert c[:, 0].min() > b[0] + 1 and c[:, 0].max() < b[1] - 1 and c[:, 1].min() > b[2] + 1 and c[:, 1].max() < b[3] - 1
    # the fold-over lens: no border pixel of a 640 x 480 image has an undistorted position -- such a start is refused
    assert mgr.radtan_bounds(rr.FOLD.as_array(), W, H) == (None, 1.0) and rr.bounds(rr.FOLD, W, H) == (None, 1.0)
    # the same lens on a smaller sensor window loses part of its border, and says how much
    small = rr.Model(400.0, 405.0, 200.0, 150.0, -0.6, 0.05, 0.002, -0.001, 0.0)
    b, share = mgr.radtan_bounds(small.as_array(), 400, 300)
    b_ref, share_ref = rr.bounds(small, 400, 300)
    assert b == b_ref and share == share_ref and 0.0 < share < 1.0


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_configuration_file_keys(mgr, tmp_path):
    pin = _cam(model="perspective", fx=458.654, fy=457.296, cx=367.215, cy=248.375, resolution_x=752, resolution_y=480, distortion=[0.0] * 5)
    m = mgr.Manager()
    assert m.read_configuration_file(_write(tmp_path, "p.json", json.dumps({"cameras": [pin]})))
    coeff = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]
    nested = _write(tmp_path, "n.yaml", "Camera:\n  name: \"EuRoC monocular\"\n  setup: monocular\n  model: perspective\n  fx: 458.654\n  k1: -0.28340811\n  k2: 0.07395907\n"
                    "  p1: 0.00019359\n  p2: 1.76187114e-05\n  k3: 0.0\n  fps: 20.0\n")
    flat = _write(tmp_path, "f.yaml", "Camera.model: \"perspective\"\nCamera.k1: -0.28340811\nCamera.k2: 0.07395907\nCamera.p1: 0.00019359\nCamera.p2: 1.76187114e-05\nCamera.k3: 0.0\n")
    no_model = _write(tmp_path, "nm.yaml", "Camera.k1: -0.28340811\nCamera.k2: 0.07395907\nCamera.p1: 0.00019359\nCamera.p2: 1.76187114e-05\n")
    for path in (nested, flat, no_model):
        rc, model = mgr.radtan_session_model(m, path)
        assert rc == 1 and list(model) == [458.654, 457.296, 367.215, 248.375] + coeff, (path, rc, model)
        assert mgr.fisheye_session_model(m, path, 70.0) == (0, None)
    # the file's intrinsics go with its coefficients
    rc, model = mgr.radtan_session_model(m, _write(tmp_path, "fx.yaml", "Camera:\n  fx: 500.0\n  cy: 250.5\n  p2: 0.001\n"))
    assert rc == 1 and list(model) == [500.0, 457.296, 367.215, 250.5, 0.0, 0.0, 0.0, 0.001, 0.0]
    # all-zero or absent coefficients: no model
    for text in ("Camera.model: perspective\nCamera.k1: 0.0\nCamera.k2: 0\nCamera.p1: 0.0\nCamera.p2: -0.0\nCamera.k3: 0\n", "Camera:\n  model: perspective\n  fx: 458.0\n",
                 "Feature.num_levels: 3\n"):
        assert mgr.radtan_session_model(m, _write(tmp_path, "z.yaml", text)) == (0, None)
    # a key that is present but no number refuses the start, naming the key
    for key in ("k1", "k2", "p1", "p2", "k3"):
        rc, why = mgr.radtan_session_model(m, _write(tmp_path, "b.yaml", "Camera.model: perspective\nCamera.k1: -0.1\nCamera.%s: much\n" % key))
        assert rc == -1 and ("Camera." + key) in why, (key, rc, why)
    rc, why = mgr.radtan_session_model(m, _write(tmp_path, "inf.yaml", "Camera.k1: inf\n"))
    assert rc == -1 and "finite" in why
    # model: fisheye is still resolved as fisheye, and as nothing else
    fe = _write(tmp_path, "fe.yaml", "Camera:\n  model: fisheye\n  k1: -0.01\n  k2: 0.02\n  k3: -0.03\n  k4: 0.004\n")
    rc, model = mgr.fisheye_session_model(m, fe, 70.0)
    assert rc == 1 and list(model[4:8]) == [-0.01, 0.02, -0.03, 0.004]
    assert mgr.radtan_session_model(m, fe) == (0, None)
    assert mgr.radtan_session_model(m, _write(tmp_path, "eq.yaml", "Camera.model: equirectangular\nCamera.k1: -0.1\n")) == (0, None)
    # a fisheye camera of the JSON configuration with a file that names no model stays a fisheye camera
    m_fe = mgr.Manager()
    assert m_fe.read_configuration_file(_write(tmp_path, "fe.json", json.dumps({"cameras": [_cam()]})))
    assert mgr.radtan_session_model(m_fe, no_model) == (0, None) and mgr.fisheye_session_model(m_fe, no_model, 70.0)[0] == 1
    assert mgr.radtan_session_model(m_fe, flat)[0] == 1 and mgr.fisheye_session_model(m_fe, flat, 70.0) == (0, None)      # ... unless the file says perspective
    # a Pinhole camera of the JSON configuration with dist[] set and no file gets no model (the reference writes zeros there)
    m_d = mgr.Manager()
    assert m_d.read_configuration_file(_write(tmp_path, "d.json", json.dumps({"cameras": [dict(pin, distortion=coeff[:4] + [0.01])]})))
    assert mgr.radtan_session_model(m_d, None) == (0, None) and mgr.radtan_session_model(m_d, "") == (0, None)
    assert mgr.fisheye_session_model(m_d, None, 70.0) == (0, None)


D3 = (-0.25, 0.06, 0.001, -0.0005, 0.002)


def _map_bytes_v3(d=D3, model=2):
    """_map_bytes of test_map_file_cpu with the version-3 camera record: model (u32), k1 k2 p1 p2 k3 (f64) behind scale_factor"""
    v1 = _map_bytes()
    head = 8 + 4 + 12 + 40 + 12                                      # magic, version, stereo + resolution, five doubles, levels + scale
    b = bytearray(v1[:8]) + struct.pack("<I", 3) + v1[12:head] + struct.pack("<I5d", model, *d) + v1[head:-8]
    b[12:16] = struct.pack("<I", 0)                                  # a monocular session
    return bytes(b) + struct.pack("<Q", _fnv1a64(bytes(b)))


SESSION_V3 = [0, 640, 480, 500.0, 500.0, 320.0, 240.0, 60.0, 4, 1.2, 2, *D3]


def test_map_file_version_3_round_trip_and_the_others_unchanged(mgr, tmp_path):
    p3 = tmp_path / "rt.lpsmap"
    p3.write_bytes(_map_bytes_v3())
    ok, info = mgr.map_file_info(p3)
    assert ok and info["keyframes"] == 3 and info["stereo"] == 0, info
    out = tmp_path / "rt_again.lpsmap"
    assert mgr.map_file_rewrite(p3, out) == (True, "")
    assert out.read_bytes() == p3.read_bytes() and out.read_bytes()[8:12] == struct.pack("<I", 3)
    assert mgr.map_file_camera_check(p3, SESSION_V3) == (1, "")
    # a pinhole session's file: version 1, byte for byte what the format has always had, write after write; a fisheye one: version 2
    p1 = tmp_path / "ph.lpsmap"; p1.write_bytes(_map_bytes())
    a = tmp_path / "ph_a.lpsmap"; b = tmp_path / "ph_b.lpsmap"
    assert mgr.map_file_rewrite(p1, a) == (True, "") and mgr.map_file_rewrite(a, b) == (True, "")
    assert a.read_bytes() == b.read_bytes() == _map_bytes() and a.read_bytes()[8:12] == struct.pack("<I", 1)
    p2 = tmp_path / "fe.lpsmap"; p2.write_bytes(_map_bytes_v2())
    assert mgr.map_file_rewrite(p2, a) == (True, "") and a.read_bytes() == _map_bytes_v2()
    assert len(p3.read_bytes()) == len(p1.read_bytes()) + 4 + 40
    assert mgr.map_file_camera_check(p1, SESSION_V1) == (1, "") and mgr.map_file_camera_check(p2, SESSION_V2) == (1, "")


def test_map_file_camera_model_rejections(mgr, tmp_path):
    p1 = tmp_path / "ph.lpsmap"; p1.write_bytes(_map_bytes())
    p2 = tmp_path / "fe.lpsmap"; p2.write_bytes(_map_bytes_v2())
    p3 = tmp_path / "rt.lpsmap"; p3.write_bytes(_map_bytes_v3())
    radtan_stereo_shape = list(SESSION_V1); radtan_stereo_shape[10:] = SESSION_V3[10:]
    assert mgr.map_file_camera_check(p1, radtan_stereo_shape) == (0, "camera model")       # a version-1 file in a radial-tangential session
    assert mgr.map_file_camera_check(p2, SESSION_V3) == (0, "camera model")                # a version-2 (fisheye) file in a radial-tangential session
    pinhole_mono = list(SESSION_V3); pinhole_mono[10:] = [0] * 6
    assert mgr.map_file_camera_check(p3, pinhole_mono) == (0, "camera model")              # a version-3 file in a pinhole session
    assert mgr.map_file_camera_check(p3, SESSION_V2) == (0, "camera model")                # ... and in a fisheye session
    for i in range(5):                                                                       # each coefficient
        other = list(SESSION_V3); other[11 + i] += 0.01
        assert mgr.map_file_camera_check(p3, other) == (0, "camera model"), i
    other_fx = list(SESSION_V3); other_fx[3] = 501.0
    assert mgr.map_file_camera_check(p3, other_fx) == (0, "intrinsics")                    # the earlier checks keep their reasons and their order
    # a version-3 header that names another model is an unsupported format; a file cut inside the new record is truncated
    for model in (0, 1, 3):
        p = tmp_path / "m.lpsmap"; p.write_bytes(_map_bytes_v3(model=model))
        ok, why = mgr.map_file_info(p)
        assert not ok and ("unsupported format version 3 with camera model %d" % model) in why
    p4 = tmp_path / "cut.lpsmap"; p4.write_bytes(_map_bytes_v3()[:100])
    ok, why = mgr.map_file_info(p4)
    assert not ok and "truncated" in why
    assert mgr.map_file_camera_check(p4, SESSION_V3)[0] == -1
    p5 = tmp_path / "v4.lpsmap"; p5.write_bytes(_map_bytes(version=4))
    ok, why = mgr.map_file_info(p5)
    assert not ok and "unsupported format version 4" in why


def test_standalone_sanitizer_program(mgr, tmp_path):
    """tests/cpp/radtan_host_main.cpp: the host forms and the map-file reader in a program of its own, built with
    -fsanitize=address,undefined and run directly on cases this test writes; its printed results are compared with the reference"""
    p1 = tmp_path / "ph.lpsmap"; p1.write_bytes(_map_bytes())
    p3 = tmp_path / "rt.lpsmap"; p3.write_bytes(_map_bytes_v3())
    pc = tmp_path / "cut.lpsmap"; pc.write_bytes(_map_bytes_v3()[:100])
    exe = tmp_path / "radtan_host_main"
    host = os.path.join(ROOT, "lpslam_amd", "host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "radtan_host_main.cpp"), os.path.join(host, "map_file.cpp")])
    for name, m in (("fold", rr.FOLD), ("mild", rr.MILD)):
        xy = planted_points(400, 13)
        r = rr.undistort(m, xy)
        assert rr.decisive(r).all()
        cases = tmp_path / (name + ".txt")
        with open(cases, "w") as f:
            f.write("%d %d %d\n" % (len(xy), W, H))
            f.write(" ".join(repr(float(v)) for v in m.as_array()) + "\n")
            for p, o, v in zip(xy, r["out"], r["valid"]):
                f.write("%r %r %d %d %d\n" % (float(p[0]), float(p[1]), int(v), int(o[0].view(np.int32)) if v else 0, int(o[1].view(np.int32)) if v else 0))
        out = subprocess.run([str(exe), str(cases), str(p1), str(p3), str(pc)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        assert ("points ok %d" % len(xy)) in out.stdout and "maps ok" in out.stdout, out.stdout
        # the printed results against the reference: validity equal, positions within one float32 ulp
        got = np.array([[int(t) for t in line.split()[1:]] for line in out.stdout.splitlines() if line.startswith("point ")], np.int64)
        assert len(got) == len(xy) and (got[:, 0] == np.arange(len(xy))).all()
        valid = got[:, 1] == 1
        assert (valid == r["valid"]).all()
        pos = got[valid, 2:].astype(np.int32).view(np.float32)
        assert rr.ulp_diff(pos, r["out"][valid]).max(initial=0) <= 1
        b_line = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("bounds ")][0]
        b_ref, share_ref = rr.bounds(m, W, H)
        assert int(b_line[0]) == (b_ref is not None) and int(b_line[6]) == 2 * W + 2 * (H - 2) and int(b_line[5]) == round(share_ref * int(b_line[6]))
        if b_ref is not None:
            assert tuple(float(t) for t in b_line[1:5]) == b_ref
    assert 0.2 < rr.undistort(rr.FOLD, planted_points(400, 13))["valid"].mean() < 0.5      # the fold-over cases hold both verdicts
