"""The radial-tangential keypoint camera on the device: k_undistort_points and k_undistort_compact of
lpslam_amd/csrc/frontend.hip, dispatched on the kind of the slot's table entry, against tests/radtan_ref.py -- on caller points, on
planted slots at every wave and chunk edge, through extraction and the prefetch path, inside a shared launch chain beside a fisheye and
a pinhole session -- and a warped monocular sequence through the manager with a configuration file that names the coefficients.
Coordinates are compared within 1 float32 ulp: both sides run the same five steps in FP64 and differ at most by the rounding of single
operations, orders of magnitude under a float32 ulp on valid points, so only the final rounding can differ."""
import threading
import time

import numpy as np
import pytest

import fisheye_ref as fr
import radtan_ref as rr
from lpslam_amd import synth
from test_fisheye_gpu import EXTRACT_MODEL as FISHEYE_MODEL, dev_model as fisheye_dev_model, direction_cosine, planted_slot, set_keypoints
from test_radtan_cpu import planted_points

pytestmark = pytest.mark.gpu

W, H, KPTS, LEVELS = 640, 480, 2000, 3


def dev_model(hiplib, m):
    return hiplib.Radtan(m.fx, m.fy, m.cx, m.cy, m.k1, m.k2, m.p1, m.p2, m.k3)


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def points():
    """the planted float32 points and, per planted model, the reference's answer: computed once"""
    xy = planted_points(5000, 7).astype(np.float32)
    return xy, {name: rr.undistort(m, xy.astype(np.float64)) for name, m in (("mild", rr.MILD), ("fold", rr.FOLD))}


@pytest.mark.parametrize("name", ["mild", "fold"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 5000])
def test_points(hiplib, ctx, points, name, n):
    m = {"mild": rr.MILD, "fold": rr.FOLD}[name]
    xy, refs = points
    r = {k: v[:n] for k, v in refs[name].items()}
    out, valid = ctx.undistort_points_radtan(dev_model(hiplib, m), xy[:n])
    assert out.shape == (n, 2) and valid.shape == (n,)
    assert (~rr.decisive(r)).sum() == 0                               # nothing is excluded
    assert np.array_equal(valid, r["valid"]), np.flatnonzero(valid != r["valid"])[:10]
    assert np.isnan(out[~valid]).all()
    assert rr.ulp_diff(out[valid], r["out"][valid]).max(initial=0) <= 1
    if n >= 63:
        assert valid.all() if name == "mild" else (valid.any() and (~valid).any())


# planted slots (planted_slot of the fisheye tests: valid points in [220, 420) x [140, 340), invalid ones in [0, 20) x [0, 479) and one
# NaN): valid points lie within r = 0.47 of the axis, invalid ones beyond r = 1.0, where r (1 - 0.6 r^2 + 0.05 r^4) has long folded
# over (its maximum is at r = 0.778)
PLANT_MODEL = rr.Model(300.0, 305.0, 320.0, 240.0, -0.6, 0.05, 0.002, -0.001, 0.0)
PATTERNS = ["all_valid", "all_invalid", "alternating", "last_lane", "chunk_first"]


def pattern(name, n):
    i = np.arange(n)
    return {"all_valid": np.ones(n, bool), "all_invalid": np.zeros(n, bool), "alternating": i % 2 == 0,
            "last_lane": i % 64 == 63,                                # only the last lane of each wave
            "chunk_first": i % 1024 == 0}[name]                       # only the first slot of each chunk


def check_slot(ctx, slot, kp, desc, m, compact=rr.compact, decisive=rr.decisive):
    want_kp, want_desc, dropped, r = compact(m, kp, desc)
    assert (~decisive(r)).sum() == 0
    got_kp, got_desc = ctx.keypoints(slot)
    assert len(got_kp) == len(want_kp), (len(got_kp), len(want_kp))
    for f in ("size", "angle", "response", "octave", "class_id"):     # untouched fields, and the order (class_id encodes the source index)
        assert np.array_equal(got_kp[f].view(np.int32), want_kp[f].view(np.int32)), f
    assert np.array_equal(got_desc, want_desc)                        # each descriptor travelled with its keypoint
    if len(want_kp):
        assert rr.ulp_diff(got_kp["x"], want_kp["x"]).max() <= 1 and rr.ulp_diff(got_kp["y"], want_kp["y"]).max() <= 1
    assert ctx.undistort_dropped(slot) == dropped
    return dropped, r


@pytest.fixture()
def big_ctx(hiplib):
    c = hiplib.Context(W, H, 4800, 1.2, LEVELS, max_images=2)         # 4809 slots per image: five chunks of 1024
    yield c
    c.close()


def test_stage_planted(hiplib, big_ctx):
    ctx = big_ctx
    counts = [0, 1, 64, 65, 1024, 1025, ctx.max_kp]
    assert ctx.max_kp > 4096                                          # the chunk loop runs five times on a full slot
    ctx.set_keypoint_camera_radtan(dev_model(hiplib, PLANT_MODEL))
    try:
        seed = 10
        for n in counts:
            for a in range(0, len(PATTERNS), 2):                      # two images with different patterns in one call
                slots = []
                for slot, name in ((0, PATTERNS[a]), (1, PATTERNS[(a + 1) % len(PATTERNS)])):
                    kp, desc = planted_slot(hiplib, n, pattern(name, n), seed); seed += 1
                    set_keypoints(ctx, slot, kp, desc)
                    slots.append((slot, kp, desc, name))
                ctx.stage_undistort(2)
                for slot, kp, desc, name in slots:
                    dropped, r = check_slot(ctx, slot, kp, desc, PLANT_MODEL)
                    assert np.array_equal(r["valid"], pattern(name, n)), (n, name)      # the plant is what it says
                    assert dropped == n - int(pattern(name, n).sum()), (n, name, dropped)
    finally:
        ctx.set_keypoint_camera_radtan(None)


def test_model_handling(hiplib, big_ctx):
    """no model: the slot is unchanged to the bit; either setter clears; one setter replaces what the other one set"""
    ctx = big_ctx
    n = 1025
    kp, desc = planted_slot(hiplib, n, pattern("alternating", n), 1)
    fe = fisheye_dev_model(hiplib, FISHEYE_MODEL)
    rt = dev_model(hiplib, PLANT_MODEL)

    def unchanged():
        set_keypoints(ctx, 0, kp, desc)
        ctx.stage_undistort(1)
        g_kp, g_desc = ctx.keypoints(0)
        assert g_kp.tobytes() == kp.tobytes() and np.array_equal(g_desc, desc) and ctx.undistort_dropped(0) == 0

    def as_radtan():
        set_keypoints(ctx, 0, kp, desc)
        ctx.stage_undistort(1)
        assert check_slot(ctx, 0, kp, desc, PLANT_MODEL)[0] == n // 2

    def as_fisheye():
        set_keypoints(ctx, 0, kp, desc)
        ctx.stage_undistort(1)
        check_slot(ctx, 0, kp, desc, FISHEYE_MODEL, compact=fr.compact, decisive=lambda r: fr.decisive(FISHEYE_MODEL, r))

    try:
        unchanged()                                                   # a fresh context has no model
        ctx.set_keypoint_camera_radtan(rt); as_radtan()
        ctx.set_keypoint_camera_radtan(None); unchanged()             # cleared through its own setter
        ctx.set_keypoint_camera_radtan(rt)
        ctx.set_keypoint_camera(None); unchanged()                    # ... and through the other one
        ctx.set_keypoint_camera(fe); as_fisheye()
        ctx.set_keypoint_camera_radtan(rt); as_radtan()               # radial-tangential over fisheye
        ctx.set_keypoint_camera(fe); as_fisheye()                     # ... and back
        ctx.set_keypoint_camera_radtan(None); unchanged()             # a fisheye model cleared through the radial-tangential setter
        ctx.set_keypoint_camera_radtan(rt)
        ctx.set_keypoint_camera_radtan(hiplib.Radtan(300.0, 305.0, 320.0, 240.0)); unchanged()      # all-zero coefficients are no model
    finally:
        ctx.set_keypoint_camera(None)


EXTRACT_MODEL = rr.Model(300.0, 302.0, 322.5, 238.25, -0.6, 0.05, 0.002, -0.001, 0.0)      # folds over 233 pixels from the principal point


def assert_frame(got_kp, got_desc, ref_kp, ref_desc, m):
    want_kp, want_desc, dropped, r = rr.compact(m, ref_kp, ref_desc)
    assert (~rr.decisive(r)).sum() == 0
    assert len(got_kp) == len(want_kp) and 0 < dropped < len(ref_kp) and len(want_kp) > 100, (len(got_kp), len(want_kp), dropped)
    for f in ("size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(got_kp[f], want_kp[f]), f
    assert np.array_equal(got_desc, want_desc)
    assert rr.ulp_diff(got_kp["x"], want_kp["x"]).max() <= 1 and rr.ulp_diff(got_kp["y"], want_kp["y"]).max() <= 1
    return dropped


def test_through_extraction(hiplib):
    img = synth.random_image(W, H, 3)
    a = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    b = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    try:
        b.set_keypoint_camera_radtan(dev_model(hiplib, EXTRACT_MODEL))
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


def test_shared_chain_carries_radtan_fisheye_and_pinhole_sessions(hiplib):
    rounds, n_sess = 4, 3

    def set_model(c, s):                                              # session 0: radial-tangential, 1: fisheye, 2: pinhole
        if s == 0:
            c.set_keypoint_camera_radtan(dev_model(hiplib, EXTRACT_MODEL))
        elif s == 1:
            c.set_keypoint_camera(fisheye_dev_model(hiplib, FISHEYE_MODEL))

    images = [[synth.random_image(W, H, 20 + 10 * s + r) for r in range(rounds)] for s in range(n_sess)]
    ref = {}
    for s in range(n_sess):                                           # each session's own direct context
        c = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=2)
        set_model(c, s)
        for r in range(rounds):
            c.upload(0, images[s][r]); c.extract_range(0, 1); c.prefetch_frame(0, False)
            kp, desc, _, _ = c.frame_view(0, False)
            ref[(s, r)] = (kp.copy(), desc.copy())
        c.close()
    assert len(ref[(0, 0)][0]) < len(ref[(2, 0)][0]) and len(ref[(1, 0)][0]) < len(ref[(2, 0)][0])      # both lenses remove keypoints
    got, errors = {}, []
    try:
        hiplib.set_shared_launches(1)
        b0, r0 = hiplib.shared_front_end_counters(0)
        sessions = [hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=6, session=True) for _ in range(n_sess)]
        for s in range(n_sess):
            set_model(sessions[s], s)
        barrier = threading.Barrier(n_sess)

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

        th = [threading.Thread(target=run, args=(s,)) for s in range(n_sess)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        b1, r1 = hiplib.shared_front_end_counters(0)
        for c in sessions:
            c.close()
        # a session that takes the radial-tangential session's place in the pool starts without a model
        again = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=6, session=True)
        again.front_end_images(0, images[2][0])
        kp, desc, _, _ = again.frame_view(0, False)
        again.close()
    finally:
        hiplib.set_shared_launches(None)
    assert not errors, errors
    assert r1 - r0 == n_sess * rounds and b1 - b0 < r1 - r0, (r1 - r0, b1 - b0)      # fewer chains than requests: sessions shared one
    for key, (rk, rd) in ref.items():
        gk, gd = got[key]
        assert len(gk) == len(rk) and len(rk) > 100, (key, len(gk), len(rk))
        assert gk.tobytes() == rk.tobytes() and np.array_equal(gd, rd), key      # the same device function on the same bits
    assert kp.tobytes() == ref[(2, 0)][0].tobytes() and np.array_equal(desc, ref[(2, 0)][1])


def test_refusals(hiplib, ctx):
    good = dict(fx=400.0, fy=400.0, cx=320.0, cy=240.0, k1=-0.2, k2=0.05, p1=0.001, p2=-0.001, k3=0.0)
    ctx.set_keypoint_camera_radtan(hiplib.Radtan(**good))
    try:
        for bad in (dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")), dict(k2=float("inf")), dict(p1=float("nan")), dict(k3=float("-inf"))):
            with pytest.raises(hiplib.LpslamHipError):
                ctx.set_keypoint_camera_radtan(hiplib.Radtan(**{**good, **bad}))
            with pytest.raises(hiplib.LpslamHipError):
                ctx.undistort_points_radtan(hiplib.Radtan(**{**good, **bad}), np.zeros((4, 2), np.float32))
        # the context kept what it had: stereo matching is still refused
        with pytest.raises(hiplib.LpslamHipError):
            ctx.match_stereo(0, 1, 60.0, 0.12)
        with pytest.raises(hiplib.LpslamHipError):
            ctx.match_stereo_strided(0, 1, 2, 1, 60.0, 0.12)
        with pytest.raises(hiplib.LpslamHipError):
            ctx.front_end(0, True, 60.0, 0.12)
    finally:
        ctx.set_keypoint_camera_radtan(None)
    ctx.upload(0, synth.random_image(W, H, 1)); ctx.upload(1, synth.random_image(W, H, 2))
    ctx.extract(2)
    ctx.match_stereo(0, 1, 60.0, 0.12)                                # without a model the stereo matcher runs as before


SEQ_MODEL = rr.MILD                                                   # (520, 520, 320, 240; -0.25, 0.06, 0.001, -0.0005, 0)
FILL, FEATHER = 110.0, 16.0


def sensor_to_source(m, k_src, w, h):
    """per sensor pixel of camera `m` the position in a pinhole frame with intrinsics k_src: the forward model inverted to convergence
    (the fixed-point step of the definition, 200 times: this lens contracts it everywhere in the image)"""
    ys, xs = np.mgrid[0:h, 0:w]
    x0 = (xs.ravel() - m.cx) / m.fx; y0 = (ys.ravel() - m.cy) / m.fy
    x, y = x0.copy(), y0.copy()
    for _ in range(200):
        r2 = x * x + y * y
        den = 1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2
        x, y = (x0 - (2.0 * m.p1 * x * y + m.p2 * (r2 + 2.0 * x * x))) / den, (y0 - (m.p1 * (r2 + 2.0 * y * y) + 2.0 * m.p2 * x * y)) / den
    xd, yd = rr.distort(m, x, y)
    assert np.abs(xd - x0).max() * m.fx < 1e-9 and np.abs(yd - y0).max() * m.fy < 1e-9      # it IS the inverse of the forward model
    return k_src["fx"] * x + k_src["cx"], k_src["fy"] * y + k_src["cy"]


def warp_through_lens(img, u, v):
    """the frame the lens sees where a pinhole camera saw `img`, sampled bilinearly.  The lens sees further out than the pinhole frame
    reaches (its corner looks 20.7 % further from the axis): there the frame is flat grey, and the scene fades into it over 16 pixels so
    that the edge of the scene -- which does not move with the camera -- plants no corners of its own"""
    h, w = img.shape
    uc = np.clip(u, 0, w - 1); vc = np.clip(v, 0, h - 1)
    x0 = np.minimum(np.floor(uc).astype(int), w - 2); y0 = np.minimum(np.floor(vc).astype(int), h - 2)
    ax = uc - x0; ay = vc - y0
    f = img.astype(np.float64)
    val = (f[y0, x0] * (1 - ax) + f[y0, x0 + 1] * ax) * (1 - ay) + (f[y0 + 1, x0] * (1 - ax) + f[y0 + 1, x0 + 1] * ax) * ay
    weight = np.clip(np.minimum(np.minimum(u, w - 1 - u), np.minimum(v, h - 1 - v)) / FEATHER, 0.0, 1.0)
    return np.clip(np.rint(FILL + weight * (val - FILL)), 0, 255).astype(np.uint8).reshape(h, w)


def run_sequence(manager, frames, m, yaml_path):
    n_frames = len(frames)
    mg = manager.Manager()
    c = manager.default_camera()
    c.camera_number = 0; c.f_x = m.fx; c.f_y = m.fy; c.c_x = m.cx; c.c_y = m.cy; c.resolution_x = W; c.resolution_y = H
    c.distortion_function = 0                                          # LpSlamCameraDistortionFunction_Pinhole ("perspective"), no coefficients: the file has them
    mg.set_camera(c)
    assert mg.add_tracker("VSLAMMono", '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4, "configFromFile": "%s"}' % yaml_path)
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


def test_radtan_sequence_initialises_and_tracks(hiplib, tmp_path):
    """The wall sequence of test_monocular_sequence_initialises_and_tracks seen through a radial-tangential lens, with a configuration
    file that names the coefficients: the assertions are exactly that test's, plus perspective_dropped == 0.  The same frames with a file
    that omits the coefficients -- what such a session amounted to before the model was honoured -- are run and reported, not judged."""
    from lpslam_amd import _build, manager
    _build.host_library()
    n_frames = 30
    m = SEQ_MODEL
    seq = synth.WallSequence(W, H, 11)
    centres = [seq.centre(i) for i in range(n_frames)]
    u, v = sensor_to_source(m, synth.intrinsics(W, H), W, H)
    corner = np.hypot(u[0] - 320.0, v[0] - 240.0) / np.hypot(320.0, 240.0) * (m.fx / synth.intrinsics(W, H)["fx"])
    assert 1.19 < corner < 1.22                                        # the corner of the image is displaced by about 20.7 %
    frames = [warp_through_lens(seq.frame(i), u, v) for i in range(n_frames)]
    head = "Camera:\n  name: \"planted lens\"\n  setup: monocular\n  model: perspective\n  fx: %r\n  fy: %r\n  cx: %r\n  cy: %r\n  cols: %d\n  rows: %d\n" % (m.fx, m.fy, m.cx, m.cy, W, H)
    with_k = tmp_path / "with.yaml"
    with_k.write_text(head + "  k1: %r\n  k2: %r\n  p1: %r\n  p2: %r\n  k3: %r\n" % (m.k1, m.k2, m.p1, m.p2, m.k3))
    without_k = tmp_path / "without.yaml"
    without_k.write_text(head)
    results, st, stats = run_sequence(manager, frames, m, with_k)
    cosang, valid = direction_cosine(results, centres)
    print("radial-tangential sequence, coefficients honoured: cos %s, %d of %d valid, %d keyframes, %d feature points, %s dropped"
          % ("none" if cosang is None else "%.5f" % cosang, len(valid), len(results), st.key_frames, st.feature_points, stats.get("perspective_dropped")))
    assert len(results) == n_frames and len(valid) >= n_frames - 12
    assert st.localization == 2 and st.key_frames >= 4 and st.feature_points > 150
    assert cosang > 0.995
    i0, r0 = valid[0]; i1, r1 = valid[-1]
    d = np.array(r1["p"]) - np.array(r0["p"]); truth = centres[i1] - centres[i0]
    mid_i, mid_r = valid[len(valid) // 2]
    frac = np.linalg.norm(np.array(mid_r["p"]) - np.array(r0["p"])) / np.linalg.norm(d)
    frac_true = np.linalg.norm(centres[mid_i] - centres[i0]) / np.linalg.norm(truth)
    assert abs(frac - frac_true) < 0.1
    assert stats["frames"] == n_frames and stats["perspective_dropped"] == 0
    results_p, st_p, stats_p = run_sequence(manager, frames, m, without_k)
    cos_p, valid_p = direction_cosine(results_p, centres)
    assert stats_p["perspective_dropped"] == 0
    print("radial-tangential sequence, coefficients omitted: cos %s (%d valid)" % ("none" if cos_p is None else "%.5f" % cos_p, len(valid_p)))
