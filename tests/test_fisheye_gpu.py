"""The fisheye keypoint camera on the device: k_undistort_points and k_undistort_compact of
lpslam_amd/csrc/frontend.hip against tests/fisheye_ref.py -- on caller points, on planted slots at every wave and chunk edge, through
extraction and the prefetch path, inside a shared launch chain beside a pinhole session -- and a warped monocular sequence through the
manager.  Coordinates are compared within 1 float32 ulp: both sides compute in FP64, and up to 89 degrees the conditioning of tan keeps
their difference below 1e-12 relative, far under half a float32 ulp, so only the final rounding can differ."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import fisheye_ref as fr
from lpslam_amd import synth
from test_fisheye_cpu import BAD_K, BAD_PIXELS, cam_model, planted_pixels

pytestmark = pytest.mark.gpu

W, H, KPTS, LEVELS = 640, 480, 2000, 3
K4 = (-0.0115, 0.0479, -0.0451, 0.0083)


def dev_model(hiplib, m):
    f = hiplib.Fisheye(m.fx, m.fy, m.cx, m.cy, m.k)
    f.max_angle = m.max_angle                                         # the very number the reference uses
    return f


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    yield c
    c.close()


def assert_points(m, xy32, out, valid):
    r = fr.undistort(m, xy32.astype(np.float64))
    dec = fr.decisive(m, r)
    assert (~dec).sum() == 0                                          # nothing is excluded
    assert np.array_equal(valid, r["valid"]), np.flatnonzero(valid != r["valid"])[:10]
    assert np.isnan(out[~valid]).all()
    assert fr.ulp_diff(out[valid], r["out"][valid]).max(initial=0) <= 1
    return r


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_points(hiplib, ctx, n):
    m = cam_model()
    xy = planted_pixels(m).astype(np.float32)[:n]                    # (float32 is what a keypoint holds: the reference sees the same values)
    out, valid = ctx.undistort_points(dev_model(hiplib, m), xy)
    assert out.shape == (n, 2) and valid.shape == (n,)
    r = assert_points(m, xy, out, valid)
    if n >= 65:
        assert valid.any() and (~valid).any()
    # the coefficient set whose derivative changes sign: invalid on the device too
    mb = fr.Model(m.fx, m.fy, m.cx, m.cy, BAD_K, 70.0)
    xb = np.array(BAD_PIXELS, np.float32)
    ob, vb = ctx.undistort_points(dev_model(hiplib, mb), xb)
    assert not vb.any() and not fr.undistort(mb, xb.astype(np.float64))["valid"].any()


def set_keypoints(ctx, slot, kp, desc):
    """descriptors and count through the C ABI, the keypoint array by a host-to-device copy into the slot's buffer"""
    assert len(kp) == len(desc) <= ctx.max_kp and kp.dtype.itemsize == 28
    ctx.set_descriptors(slot, desc)
    ptr = C.c_void_p()
    assert ctx.lib.lpslam_hip_keypoint_buffers(ctx.h, slot, C.byref(ptr), None, None) == 0 and ptr.value
    ctx.sync()
    if len(kp):
        kp = np.ascontiguousarray(kp)
        hip_memcpy = ctx.lib.hipMemcpy
        hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip_memcpy(ptr, kp.ctypes.data, kp.nbytes, 1) == 0
    ctx.sync()


PLANT_MODEL = fr.Model(200.0, 205.0, 320.0, 240.0, K4, 70.0)


def pattern(name, n):
    v = np.ones(n, bool)
    if name == "all_invalid":
        v[:] = False
    elif name == "alternating":
        v[1::2] = False
    elif name == "first":
        v[:1] = False
    elif name == "last":
        v[n - 1:] = False
    elif name == "edges":                                             # one invalid on each side of every wave and chunk edge
        e = np.arange(64, n + 1, 64)
        v[e[e < n]] = False; v[e - 1] = False
    return v


def planted_slot(hiplib, n, valid, seed):
    rng = np.random.default_rng(seed)
    kp = np.zeros(n, hiplib.KP_DTYPE)
    kp["x"] = np.where(valid, rng.uniform(220, 420, n), rng.uniform(0, 20, n)).astype(np.float32)      # theta_d <= 0.7 / >= 1.5
    kp["y"] = np.where(valid, rng.uniform(140, 340, n), rng.uniform(0, 479, n)).astype(np.float32)
    if (~valid).any():
        kp["x"][np.flatnonzero(~valid)[0]] = np.nan                   # a position that is no number is no position
    kp["size"] = rng.uniform(31, 45, n); kp["angle"] = rng.uniform(0, 360, n); kp["response"] = rng.uniform(7, 200, n)
    kp["octave"] = rng.integers(0, LEVELS, n); kp["class_id"] = np.arange(n, dtype=np.int32) - 5
    desc = (np.arange(n, dtype=np.uint32)[:, None] * np.uint32(2654435761) + np.arange(8, dtype=np.uint32)[None, :]).astype("<u4").view(np.uint8).reshape(n, 32)
    return kp, desc


def check_slot(ctx, slot, kp, desc, m):
    want_kp, want_desc, dropped, r = fr.compact(m, kp, desc)
    assert (~fr.decisive(m, r)).sum() == 0
    got_kp, got_desc = ctx.keypoints(slot)
    assert len(got_kp) == len(want_kp), (len(got_kp), len(want_kp))
    for f in ("size", "angle", "response", "octave", "class_id"):     # untouched fields, and the order (class_id encodes the source index)
        assert np.array_equal(got_kp[f].view(np.int32), want_kp[f].view(np.int32)), f
    assert np.array_equal(got_desc, want_desc)                        # each descriptor travelled with its keypoint
    if len(want_kp):
        assert fr.ulp_diff(got_kp["x"], want_kp["x"]).max() <= 1 and fr.ulp_diff(got_kp["y"], want_kp["y"]).max() <= 1
    assert ctx.undistort_dropped(slot) == dropped
    return dropped


@pytest.fixture()
def big_ctx(hiplib):
    c = hiplib.Context(W, H, 4800, 1.2, LEVELS, max_images=2)         # 4809 slots per image: five chunks of 1024
    yield c
    c.close()


def test_stage_planted(hiplib, big_ctx):
    ctx = big_ctx
    names = ["all_valid", "all_invalid", "alternating", "first", "last", "edges"]
    counts = [0, 1, 64, 65, 1024, 1025, ctx.max_kp]
    assert ctx.max_kp > 4096                                          # the chunk loop runs five times on a full slot
    # without a model: OK, and the slot is unchanged to the bit
    kp, desc = planted_slot(hiplib, 1025, pattern("alternating", 1025), 1)
    set_keypoints(ctx, 0, kp, desc)
    ctx.stage_undistort(1)
    g_kp, g_desc = ctx.keypoints(0)
    assert g_kp.tobytes() == kp.tobytes() and np.array_equal(g_desc, desc) and ctx.undistort_dropped(0) == 0
    ctx.set_keypoint_camera(dev_model(hiplib, PLANT_MODEL))
    try:
        seed = 10
        for n in counts:
            for a in range(0, len(names), 2):                         # two images with different patterns in one call
                slots = []
                for slot, name in ((0, names[a]), (1, names[a + 1])):
                    kp, desc = planted_slot(hiplib, n, pattern(name, n), seed); seed += 1
                    set_keypoints(ctx, slot, kp, desc)
                    slots.append((slot, kp, desc, name))
                ctx.stage_undistort(2)
                for slot, kp, desc, name in slots:
                    dropped = check_slot(ctx, slot, kp, desc, PLANT_MODEL)
                    want = {"all_valid": 0, "all_invalid": n, "alternating": n // 2, "first": min(n, 1), "last": min(n, 1)}.get(name)
                    assert want is None or dropped == want, (n, name, dropped)
        # clearing the model: the stage launches nothing again
        ctx.set_keypoint_camera(None)
        kp, desc = planted_slot(hiplib, 65, pattern("edges", 65), 99)
        set_keypoints(ctx, 0, kp, desc)
        ctx.stage_undistort(1)
        assert ctx.keypoints(0)[0].tobytes() == kp.tobytes()
    finally:
        ctx.set_keypoint_camera(None)


EXTRACT_MODEL = fr.Model(220.0, 222.0, 322.5, 238.25, K4, 70.0)


def assert_frame(got_kp, got_desc, ref_kp, ref_desc, m):
    want_kp, want_desc, dropped, r = fr.compact(m, ref_kp, ref_desc)
    assert (~fr.decisive(m, r)).sum() == 0
    assert len(got_kp) == len(want_kp) and 0 < dropped < len(ref_kp) and len(want_kp) > 100, (len(got_kp), len(want_kp), dropped)
    for f in ("size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(got_kp[f], want_kp[f]), f
    assert np.array_equal(got_desc, want_desc)
    assert fr.ulp_diff(got_kp["x"], want_kp["x"]).max() <= 1 and fr.ulp_diff(got_kp["y"], want_kp["y"]).max() <= 1
    return dropped


def test_through_extraction(hiplib):
    img = synth.random_image(W, H, 3)
    a = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    b = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    try:
        b.set_keypoint_camera(dev_model(hiplib, EXTRACT_MODEL))
        a.upload(0, img); a.extract(1)
        ref_kp, ref_desc = a.keypoints(0)
        b.upload(0, img); b.extract(1)
        got_kp, got_desc = b.keypoints(0)
        dropped = assert_frame(got_kp, got_desc, ref_kp, ref_desc, EXTRACT_MODEL)
        assert b.undistort_dropped(0) == dropped
        # the prefetch path: front end with the frame, then the delivered copy
        b.front_end_images(2, img)
        kp2, desc2, _, _ = b.frame_view(2, False)
        assert_frame(kp2, desc2, ref_kp, ref_desc, EXTRACT_MODEL)
        assert b.undistort_dropped(2) == dropped
        a.front_end_images(2, img)                                    # and a context without a model delivers what it always did
        kp3, desc3, _, _ = a.frame_view(2, False)
        assert kp3.tobytes() == ref_kp.tobytes() and np.array_equal(desc3, ref_desc)
    finally:
        a.close(); b.close()


def test_shared_chain_carries_fisheye_and_pinhole_sessions(hiplib):
    rounds = 4
    images = [[synth.random_image(W, H, 20 + 10 * s + r) for r in range(rounds)] for s in range(2)]
    ref = {}
    for s in range(2):                                                # session 0 is the fisheye one
        c = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=2)
        if s == 0:
            c.set_keypoint_camera(dev_model(hiplib, EXTRACT_MODEL))
        for r in range(rounds):
            c.upload(0, images[s][r]); c.extract_range(0, 1); c.prefetch_frame(0, False)
            kp, desc, _, _ = c.frame_view(0, False)
            ref[(s, r)] = (kp.copy(), desc.copy())
        c.close()
    got, errors = {}, []
    try:
        hiplib.set_shared_launches(1)
        b0, r0 = hiplib.shared_front_end_counters(0)
        sessions = [hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=6, session=True) for _ in range(2)]
        sessions[0].set_keypoint_camera(dev_model(hiplib, EXTRACT_MODEL))
        barrier = threading.Barrier(2)

        def run(s):
            try:
                for r in range(rounds):
                    slot = 2 * (r % 3)
                    barrier.wait()
                    sessions[s].front_end_images(slot, images[s][r])
                    kp, desc, _, _ = sessions[s].frame_view(slot, False)
                    got[(s, r)] = (kp.copy(), desc.copy())
            except BaseException as e:
                errors.append(e); barrier.abort()

        th = [threading.Thread(target=run, args=(s,)) for s in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        b1, r1 = hiplib.shared_front_end_counters(0)
        for c in sessions:
            c.close()
        # a session that takes the fisheye session's place in the pool starts without a model
        again = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=6, session=True)
        again.front_end_images(0, images[1][0])
        kp, desc, _, _ = again.frame_view(0, False)
        again.close()
    finally:
        hiplib.set_shared_launches(None)
    assert not errors, errors
    assert r1 - r0 == 2 * rounds and b1 - b0 < r1 - r0, (r1 - r0, b1 - b0)      # fewer chains than requests: the two shared one
    for key, (rk, rd) in ref.items():
        gk, gd = got[key]
        assert len(gk) == len(rk) and len(rk) > 100, (key, len(gk), len(rk))
        assert gk.tobytes() == rk.tobytes() and np.array_equal(gd, rd), key      # the same device function on the same bits
    assert kp.tobytes() == ref[(1, 0)][0].tobytes() and np.array_equal(desc, ref[(1, 0)][1])


def test_refusals(hiplib, ctx):
    good = dict(fx=200.0, fy=200.0, cx=320.0, cy=240.0, k=K4, max_angle_deg=70.0)
    for bad in (dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")), dict(k=(0.0, float("inf"), 0.0, 0.0)), dict(max_angle_deg=0.0), dict(max_angle_deg=89.5), dict(max_angle_deg=-3.0)):
        with pytest.raises(hiplib.LpslamHipError):
            ctx.set_keypoint_camera(hiplib.Fisheye(**{**good, **bad}))
        with pytest.raises(hiplib.LpslamHipError):
            ctx.undistort_points(hiplib.Fisheye(**{**good, **bad}), np.zeros((4, 2), np.float32))
    ctx.set_keypoint_camera(hiplib.Fisheye(**{**good, "max_angle_deg": 89.0}))
    try:
        with pytest.raises(hiplib.LpslamHipError):
            ctx.match_stereo(0, 1, 60.0, 0.12)
        with pytest.raises(hiplib.LpslamHipError):
            ctx.match_stereo_strided(0, 1, 2, 1, 60.0, 0.12)
        with pytest.raises(hiplib.LpslamHipError):
            ctx.front_end(0, True, 60.0, 0.12)
    finally:
        ctx.set_keypoint_camera(None)
    ctx.upload(0, synth.random_image(W, H, 1)); ctx.upload(1, synth.random_image(W, H, 2))
    ctx.extract(2)
    ctx.match_stereo(0, 1, 60.0, 0.12)                                # without a model the stereo matcher runs as before


SEQ_MODEL = fr.Model(640.0, 640.0, 320.0, 240.0, (-0.03, 0.02, -0.01, 0.002), 70.0)


def warp_to_fisheye(img, m, k_src):
    """the frame a fisheye camera `m` sees where a pinhole camera k_src saw `img`: per sensor pixel the definition's own undistortion
    (a position of the pinhole camera with m's intrinsics), moved to the source's intrinsics, sampled bilinearly"""
    h, w = img.shape
    ys, xs = np.mgrid[0:h, 0:w]
    r = fr.undistort(m, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64))
    assert r["valid"].all()
    u = (r["out"][:, 0].astype(np.float64) - m.cx) / m.fx * k_src["fx"] + k_src["cx"]
    v = (r["out"][:, 1].astype(np.float64) - m.cy) / m.fy * k_src["fy"] + k_src["cy"]
    assert u.min() >= 0 and v.min() >= 0 and u.max() <= w - 1 and v.max() <= h - 1      # no unfilled pixels: the source covers the whole image
    x0 = np.minimum(np.floor(u).astype(int), w - 2); y0 = np.minimum(np.floor(v).astype(int), h - 2)
    ax = u - x0; ay = v - y0
    f = img.astype(np.float64)
    val = (f[y0, x0] * (1 - ax) + f[y0, x0 + 1] * ax) * (1 - ay) + (f[y0 + 1, x0] * (1 - ax) + f[y0 + 1, x0 + 1] * ax) * ay
    return np.clip(np.rint(val), 0, 255).astype(np.uint8).reshape(h, w)


def run_sequence(manager, frames, m, fisheye):
    n_frames = len(frames)
    mg = manager.Manager()
    c = manager.default_camera()
    c.camera_number = 0; c.f_x = m.fx; c.f_y = m.fy; c.c_x = m.cx; c.c_y = m.cy; c.resolution_x = W; c.resolution_y = H
    c.distortion_function = 1 if fisheye else 0                        # LpSlamCameraDistortionFunction_Fisheye / _Pinhole ("perspective")
    for i in range(4):
        c.dist[i] = m.k[i] if fisheye else 0.0
    mg.set_camera(c)
    assert mg.add_tracker("VSLAMMono", '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4}')
    mg.collect_results(); mg.provide_odometry()
    mg.start()
    for i, img in enumerate(frames):
        assert mg.add_image((i + 1) * 40_000_000, img)
    t0 = time.time()
    while len(mg.results) < n_frames and time.time() - t0 < 60:
        time.sleep(0.01)
    st = mg.status()
    mg.stop()
    return mg.results, st, mg.tracker_statistics()


def direction_cosine(results, centres):
    valid = [(i, r) for i, r in enumerate(results) if r["valid"]]
    if len(valid) < 2:
        return None, valid
    i0, r0 = valid[0]; i1, r1 = valid[-1]
    d = np.array(r1["p"]) - np.array(r0["p"])
    truth = centres[i1] - centres[i0]
    truth_lp = np.array([-truth[1], truth[0], truth[2]])
    return float(d @ truth_lp / (np.linalg.norm(d) * np.linalg.norm(truth_lp))), valid


def test_fisheye_sequence_initialises_and_tracks(hiplib):
    """The wall sequence of test_monocular_sequence_initialises_and_tracks seen through a fisheye lens, with the camera declared
    "fisheye": the assertions are exactly that test's.  The same frames with the camera declared "perspective" -- what a fisheye session
    amounted to before the model was honoured -- are run and reported, not judged."""
    from lpslam_amd import _build, manager
    _build.host_library()
    n_frames = 30
    k = synth.intrinsics(W, H)
    seq = synth.WallSequence(W, H, 11)
    centres = [seq.centre(i) for i in range(n_frames)]
    frames = [warp_to_fisheye(seq.frame(i), SEQ_MODEL, k) for i in range(n_frames)]
    results, st, stats = run_sequence(manager, frames, SEQ_MODEL, True)
    cosang, valid = direction_cosine(results, centres)
    assert len(results) == n_frames and len(valid) >= n_frames - 12
    assert st.localization == 2 and st.key_frames >= 4 and st.feature_points > 150
    assert cosang > 0.995
    i0, r0 = valid[0]; i1, r1 = valid[-1]
    d = np.array(r1["p"]) - np.array(r0["p"]); truth = centres[i1] - centres[i0]
    mid_i, mid_r = valid[len(valid) // 2]
    frac = np.linalg.norm(np.array(mid_r["p"]) - np.array(r0["p"])) / np.linalg.norm(d)
    frac_true = np.linalg.norm(centres[mid_i] - centres[i0]) / np.linalg.norm(truth)
    assert abs(frac - frac_true) < 0.1
    assert "fisheye_dropped" in stats and stats["frames"] == n_frames
    results_p, st_p, stats_p = run_sequence(manager, frames, SEQ_MODEL, False)
    cos_p, valid_p = direction_cosine(results_p, centres)
    assert stats_p["fisheye_dropped"] == 0
    print("fisheye sequence: declared fisheye cos %.5f (%d valid, %d dropped); declared perspective cos %s (%d valid)" %
          (cosang, len(valid), stats["fisheye_dropped"], "none" if cos_p is None else "%.5f" % cos_p, len(valid_p)))
