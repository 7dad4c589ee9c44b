"""The AdjustIntensity processor on the device (lpslam_amd/csrc/intensity.hip): the slot call, the raw path and the error paths of the
C ABI against the numpy restatement in tests/intensity_ref.py, and the end-to-end equivalence through LpSlamManager -- a session
with the processor fed frames F tracks exactly what a session without it tracks on adjust(F).  Every comparison is exact."""
import ctypes as C
import glob
import json
import threading
import time

import numpy as np
import pytest

import intensity_ref as ir
import record_reader as rr
from lpslam_amd import synth

pytestmark = pytest.mark.gpu


def dim(img):
    return (img.astype(np.float64) * 0.2 + 8).astype(np.uint8)


def two_level(h, w, a, b):
    img = np.full((h, w), a, np.uint8)
    img[:, w // 2:] = b
    return img


def images(w, h):
    """the image list of tests/test_processor_cpu.py at a context's size (a context is at least 64 x 64: the N < 100 case is the host's)"""
    l, r = synth.StereoSequence(w, h, 3, n_points=3000).frame(0)
    return {"synth_left": l, "synth_right": r, "dimmed": dim(l), "random": synth.random_image(w, h, 1),
            "constant_97": np.full((h, w), 97, np.uint8), "zeros": np.zeros((h, w), np.uint8), "all_255": np.full((h, w), 255, np.uint8),
            "two_level_lo_eq_hi": two_level(h, w, 100, 102)}


def read_slot(ctx, image):
    """level 0 of a slot through lpslam_hip_image_ptr and a device-to-host copy of the whole pitched block: (pixels, padding)"""
    # hipMemcpy is looked up through the library's own handle, i.e. in the HIP runtime it is linked against: once another copy of
    # the runtime is in the process (torch brings one), a handle opened by name may be that copy, which knows no device
    hip_memcpy = ctx.lib.hipMemcpy
    hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    ctx.sync()
    ptr, pitch = ctx.image_ptr(image)
    h, w = ctx.cfg.height, ctx.cfg.width
    buf = np.zeros((h, pitch), np.uint8)
    assert hip_memcpy(buf.ctypes.data, ptr, buf.size, 2) == 0             # hipMemcpyDeviceToHost
    return buf[:, :w].copy(), buf[:, w:].copy()


def check_pair(ctx, a, b, params=None, **kw):
    """uploads a, b into slots 0, 1, adjusts both in one call, compares pixels, limits and histogram with numpy"""
    ctx.upload(0, a); ctx.upload(1, b)
    ctx.adjust_intensity(0, 2, params)
    for slot, img in ((0, a), (1, b)):
        want, lo, hi, hist = ir.adjust_full(img, **kw)
        got, pad = read_slot(ctx, slot)
        glo, ghi, ghist = ctx.adjust_intensity_last(slot)
        assert (glo, ghi) == (lo, hi), (slot, glo, ghi, lo, hi)
        assert np.array_equal(ghist, hist)
        assert np.array_equal(got, want)
        assert not pad.any()                                                      # row padding is neither counted nor written


@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720), (322, 64), (333, 77)])
def test_slot_call_equals_the_numpy_restatement(hiplib, w, h):
    ctx = hiplib.Context(w, h, 300, 1.2, 2, max_images=2)
    try:
        cases = images(w, h)
        names = sorted(cases)
        # consecutive calls on the same slots: every one must give its own frame's result (the histogram words were cleared on the stream)
        for i, name in enumerate(names):
            check_pair(ctx, cases[name], cases[names[(i + 3) % len(names)]])
        hp = hiplib.AdjustParams(-0.1, 1.2, 0.05, 0.9)
        check_pair(ctx, cases["dimmed"], cases["random"], hp, low_out=-0.1, high_out=1.2, low_fraction=0.05, high_fraction=0.9)
        hp = hiplib.AdjustParams(0.0, 1.0, 0.0, 1.0)
        check_pair(ctx, cases["synth_left"], cases["constant_97"], hp, low_out=0.0, high_out=1.0, low_fraction=0.0, high_fraction=1.0)
        # the constant image's worked value (tests/intensity_ref.py)
        ctx.upload(0, cases["constant_97"]); ctx.adjust_intensity(0, 1)
        lo, hi, grey = ir.constant_expectation(97, w * h)
        assert ctx.adjust_intensity_last(0)[:2] == (lo, hi) and np.all(read_slot(ctx, 0)[0] == grey)
        # one slot only, the second one: its neighbour stays as it is
        ctx.upload(0, cases["random"]); ctx.upload(1, cases["dimmed"])
        ctx.adjust_intensity(1, 1)
        assert np.array_equal(read_slot(ctx, 0)[0], cases["random"]) and np.array_equal(read_slot(ctx, 1)[0], ir.adjust(cases["dimmed"]))
    finally:
        ctx.close()


def test_slot_call_at_1920x1080_and_inside_a_prefetch_section(hiplib):
    w, h = 1920, 1080
    ctx = hiplib.Context(w, h, 300, 1.2, 2, max_images=4)
    try:
        l, r = synth.StereoSequence(w, h, 5, n_points=3000).frame(0)
        check_pair(ctx, dim(l), r)
        # the next frame into slots 2, 3 on the prefetch stream; joined, then read
        a, b = dim(r), synth.random_image(w, h, 7)
        with ctx.prefetch():
            for slot, img in ((2, a), (3, b)):
                hiplib._check(ctx.lib.lpslam_hip_upload_image(ctx.h, slot, hiplib._p(img), img.shape[1]))
            ctx.adjust_intensity(2, 2)
        ctx.prefetch_join()
        for slot, img in ((2, a), (3, b)):
            want, lo, hi, hist = ir.adjust_full(img)
            assert np.array_equal(read_slot(ctx, slot)[0], want)
            glo, ghi, ghist = ctx.adjust_intensity_last(slot)
            assert (glo, ghi) == (lo, hi) and np.array_equal(ghist, hist)
    finally:
        ctx.close()


def test_front_end_images_adjusted_extracts_the_adjusted_frame(hiplib):
    """the one-call front end with the adjustment: same keypoints and descriptors as uploading numpy's adjusted frames"""
    w, h = 640, 480
    k = synth.intrinsics(w, h)
    l, r = (dim(e) for e in synth.StereoSequence(w, h, 4, n_points=6000).frame(0))
    ctx = hiplib.Context(w, h, 1000, 1.2, 4, max_images=2)
    try:
        ctx.front_end_images_adjusted(0, l, r, k["fxb"], k["baseline"])
        got = ctx.frame(0)
        assert np.array_equal(read_slot(ctx, 0)[0], ir.adjust(l)) and np.array_equal(read_slot(ctx, 1)[0], ir.adjust(r))
        ctx.front_end_images(0, ir.adjust(l), ir.adjust(r), k["fxb"], k["baseline"])
        want = ctx.frame(0)
        assert len(got[0]) == len(want[0]) > 100
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_)
        ctx.front_end_images(0, l, r, k["fxb"], k["baseline"])
        plain = ctx.frame(0)
        print("keypoints on the dimmed frame: %d without the adjustment, %d with it" % (len(plain[0]), len(got[0])))
    finally:
        ctx.close()


def test_raw_path_adjusts_before_it_remaps(hiplib):
    from oracle import rectify as rect
    w, h = 320, 240
    ctx = hiplib.Context(w, h, 300, 1.2, 4, max_images=2)
    try:
        rng = np.random.default_rng(5)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        maps = [(xx + rng.uniform(-4, 4, xx.shape).astype(np.float32), yy + rng.uniform(-4, 4, xx.shape).astype(np.float32)),
                (xx * 1.1 - 20, yy * 1.15 - 25)]
        l, r = synth.StereoSequence(w, h, 2, n_points=2500).frame(0)
        raws = [dim(l), r]
        for eye in (0, 1):
            ctx.set_rectify_map(eye, *maps[eye])
        for eye in (0, 1):                                # the staging buffer is reused by the second eye
            ctx.upload_raw_adjusted(eye, eye, raws[eye])
        for eye in (0, 1):
            mx, my = maps[eye]
            want = rect.remap_linear_u8(ir.adjust(raws[eye]), mx, my)
            other = ir.adjust(rect.remap_linear_u8(raws[eye], mx, my))
            got = read_slot(ctx, eye)[0]
            assert np.array_equal(got, want), eye
            assert not np.array_equal(want, other)                                # the order is pinned: the two differ on this input
            lo, hi, hist = ir.limits(raws[eye])
            glo, ghi, ghist = ctx.adjust_intensity_last(eye)
            assert (glo, ghi) == (lo, hi) and np.array_equal(ghist, hist)          # the histogram is the RAW frame's
        hp = hiplib.AdjustParams(0.0, 1.0, 0.02, 0.98)
        ctx.upload_raw_adjusted(0, 0, raws[0], hp)
        assert np.array_equal(read_slot(ctx, 0)[0], rect.remap_linear_u8(ir.adjust(raws[0], 0.0, 1.0, 0.02, 0.98), *maps[0]))
        ctx.upload_raw(0, 0, raws[0])                                             # the plain call still does not adjust
        assert np.array_equal(read_slot(ctx, 0)[0], rect.remap_linear_u8(raws[0], *maps[0]))
    finally:
        ctx.close()


def _rc(hiplib, call):
    with pytest.raises(hiplib.LpslamHipError) as e:
        call()
    return int(str(e.value).split("error ")[1].split(":")[0])


def test_error_paths_return_the_stated_codes_and_touch_nothing(hiplib):
    INVALID, CAPACITY = 1, 3
    w, h = 320, 240
    ctx = hiplib.Context(w, h, 300, 1.2, 2, max_images=2)
    try:
        img = dim(synth.random_image(w, h, 2))
        ctx.upload(0, img); ctx.upload(1, img)
        P = hiplib.AdjustParams
        assert _rc(hiplib, lambda: ctx.adjust_intensity(0, 0)) == CAPACITY
        assert _rc(hiplib, lambda: ctx.adjust_intensity(-1, 1)) == CAPACITY
        assert _rc(hiplib, lambda: ctx.adjust_intensity(1, 2)) == CAPACITY
        assert _rc(hiplib, lambda: ctx.adjust_intensity(2, 1)) == CAPACITY
        for bad in (P(1.0, 1.0), P(2.0, 1.0), P(float("nan"), 1.0), P(0.0, float("inf")), P(-0.3, 1.4, 0.5, 0.5), P(-0.3, 1.4, 0.99, 0.01),
                    P(-0.3, 1.4, -0.01, 0.99), P(-0.3, 1.4, 0.01, 1.01)):
            assert _rc(hiplib, lambda: ctx.adjust_intensity(0, 2, bad)) == INVALID
            assert _rc(hiplib, lambda: ctx.front_end_images_adjusted(0, img, img, 50.0, 0.1, bad)) == INVALID
        f = ctx.lib.lpslam_hip_adjust_intensity
        f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        assert f(ctx.h, 0, 2, None) == INVALID and b"null" in ctx.lib.lpslam_hip_last_error()
        assert _rc(hiplib, lambda: ctx.adjust_intensity_last(0)) == INVALID        # nothing has been adjusted
        assert _rc(hiplib, lambda: ctx.adjust_intensity_last(2)) == CAPACITY
        assert _rc(hiplib, lambda: ctx.upload_raw_adjusted(0, 0, img)) == INVALID  # no rectify map
        for slot in (0, 1):
            assert np.array_equal(read_slot(ctx, slot)[0], img)                   # nothing was enqueued
    finally:
        ctx.close()
    # 2^24 pixels and more are rejected by lp_adjust_check, but no context gets there: the front end's own limit (fewer than 2048 FAST
    # cells per level, about 2600 x 2600) refuses such an image at creation.  The host implementation's rejection is tested on the CPU.
    assert _rc(hiplib, lambda: hiplib.Context(4096, 4096, 300, 1.2, 1, max_images=1)) == INVALID


# ---- through the manager -------------------------------------------------------------------------------------------------------
TRACKER = '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "asyncMapping": false, "prefetch": %s}'


def _manager(manager, w, h, tracker_cfg, log, processor, setup_camera=None, mono=False):
    k = synth.intrinsics(w, h)
    m = manager.Manager()
    for num in ((0,) if mono else (0, 1)):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = w; c.resolution_y = h; c.focal_x_baseline = k["fxb"]
        if setup_camera:
            setup_camera(c)
        m.set_camera(c)
    assert m.add_tracker("VSLAMMono" if mono else "VSLAMStereo", tracker_cfg)
    if processor is not None:
        assert m.add_processor("AdjustIntensity", processor)
    m.collect_results(); m.provide_odometry()
    m.log_to_file(log)
    return m


def _run(m, frames, queue_first=True, mono=False):
    def feed():
        for i, f in enumerate(frames):
            assert m.add_image((i + 1) * 40_000_000, f) if mono else m.add_stereo((i + 1) * 40_000_000, *f)
    if queue_first:           # queued before the worker starts: every frame has a successor waiting (the prefetch path carries it)
        feed(); m.start()
    else:
        m.start(); feed()
    t0 = time.time()
    while len(m.results) < len(frames) and time.time() - t0 < 90:
        time.sleep(0.01)
    m.stop()
    assert len(m.results) == len(frames)
    return [(r["valid"], tuple(r["p"]), tuple(r["q"])) for r in m.results], m.tracker_statistics()


def _dimmed_stereo(w, h, n, seq_id=4):
    seq = synth.StereoSequence(w, h, seq_id, n_points=6000)
    return [tuple(dim(e) for e in seq.frame(i)) for i in range(n)]


@pytest.mark.parametrize("prefetch", ["true", "false"])
def test_session_with_the_processor_equals_a_session_fed_adjusted_frames(hiplib, tmp_path, prefetch):
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h, n = 640, 480, 16
    F = _dimmed_stereo(w, h, n)
    G = [tuple(ir.adjust(e) for e in f) for f in F]
    a, sa = _run(_manager(manager, w, h, TRACKER % prefetch, tmp_path / "a.log", ""), F)
    b, sb = _run(_manager(manager, w, h, TRACKER % prefetch, tmp_path / "b.log", None), G)
    c, sc = _run(_manager(manager, w, h, TRACKER % prefetch, tmp_path / "c.log", None), F)
    print("prefetch %s: valid poses %d with the processor, %d on the same dimmed frames without it; landmarks %d / %d; ms_per_frame %.4f / %.4f"
          % (prefetch, sum(v for v, _, _ in a), sum(v for v, _, _ in c), sa["landmarks"], sc["landmarks"], sa["ms_per_frame"], sc["ms_per_frame"]))
    assert a == b
    assert sum(v for v, _, _ in a) >= n - 2
    assert sa["intensity_adjusted"] == n and sb["intensity_adjusted"] == 0 and sc["intensity_adjusted"] == 0
    assert sa["prefetched"] == sb["prefetched"] == (n - 1 if prefetch == "true" else 0)
    for key in ("frames", "keyframes", "landmarks", "motion_tracked", "local_ba"):
        assert sa[key] == sb[key], key


def test_non_default_keys_reach_the_device(hiplib, tmp_path):
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h, n = 640, 480, 8
    F = _dimmed_stereo(w, h, n)
    kw = dict(low_out=-0.1, high_out=1.2, low_fraction=0.03, high_fraction=0.97)
    G = [tuple(ir.adjust(e, **kw) for e in f) for f in F]
    cfg = json.dumps({"lowOut": -0.1, "highOut": 1.2, "lowFraction": 0.03, "highFraction": 0.97})
    a, sa = _run(_manager(manager, w, h, TRACKER % "true", tmp_path / "a.log", cfg), F)
    b, _ = _run(_manager(manager, w, h, TRACKER % "true", tmp_path / "b.log", None), G)
    assert a == b and sa["intensity_adjusted"] == n
    assert G[0][0].tobytes() != ir.adjust(F[0][0]).tobytes()                      # the keys matter on these frames


def test_raw_path_session_equals_a_session_fed_adjusted_raw_frames(hiplib, tmp_path):
    """cameras with distortion: the tracker rectifies on the device; the processor's adjustment runs on the raw frame in front of it"""
    from oracle import rectify as rect
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h, n = 640, 480, 16
    k = synth.intrinsics(w, h)
    K = np.array([[k["fx"], 0, k["cx"]], [0, k["fy"], k["cy"]], [0, 0, 1.0]])
    D = np.array([-0.05, 0.01, 0.0003, -0.0002, 0.0])
    T = np.array([-k["baseline"], 0.0, 0.0])
    R1, R2, P1, P2 = rect.stereo_rectify(K, D, K, D, (w, h), np.eye(3), T)

    def raw_from_ideal(img, Rk, P):      # as tests/test_rectify_gpu.py builds its raw frames
        v, u = np.mgrid[0:h, 0:w].astype(np.float64)
        x = (u - K[0, 2]) / K[0, 0]; y = (v - K[1, 2]) / K[1, 1]
        x0, y0 = x.copy(), y.copy()
        for _ in range(5):
            r2 = x * x + y * y
            ic = 1.0 / (1 + ((D[4] * r2 + D[1]) * r2 + D[0]) * r2)
            dx = 2 * D[2] * x * y + D[3] * (r2 + 2 * x * x); dy = D[2] * (r2 + 2 * y * y) + 2 * D[3] * x * y
            x = (x0 - dx) * ic; y = (y0 - dy) * ic
        RR = P[:, :3] @ Rk
        ww = RR[2, 0] * x + RR[2, 1] * y + RR[2, 2]
        mx = ((RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]) / ww).astype(np.float32)
        my = ((RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]) / ww).astype(np.float32)
        return rect.remap_linear_u8(img, mx, my)

    def camera(c):
        c.distortion_function = manager.PINHOLE
        for i, v in enumerate(D):
            c.dist[i] = v
        for i, v in enumerate(T):
            c.translation[i] = v

    seq = synth.StereoSequence(w, h, 4, n_points=6000)
    F = []
    for i in range(n):
        l, r = seq.frame(i)
        F.append((dim(raw_from_ideal(l, R1, P1)), dim(raw_from_ideal(r, R2, P2))))
    G = [tuple(ir.adjust(e) for e in f) for f in F]
    a, sa = _run(_manager(manager, w, h, TRACKER % "true", tmp_path / "a.log", "", camera), F)
    b, sb = _run(_manager(manager, w, h, TRACKER % "true", tmp_path / "b.log", None, camera), G)
    assert a == b and sum(v for v, _, _ in a) >= n - 3
    assert sa["intensity_adjusted"] == n and sb["intensity_adjusted"] == 0 and sa["prefetched"] == n - 1


def test_monocular_session_equals_a_session_fed_adjusted_frames(hiplib, tmp_path):
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h, n = 640, 480, 24
    seq = synth.WallSequence(w, h, 11)
    F = [dim(seq.frame(i)) for i in range(n)]
    G = [ir.adjust(f) for f in F]
    cfg = '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4, "asyncMapping": false}'
    a, sa = _run(_manager(manager, w, h, cfg, tmp_path / "a.log", "", mono=True), F, mono=True)
    b, sb = _run(_manager(manager, w, h, cfg, tmp_path / "b.log", None, mono=True), G, mono=True)
    assert a == b and sa["intensity_adjusted"] == n and sb["intensity_adjusted"] == 0
    assert sum(v for v, _, _ in a) >= n - 14


def test_four_managers_with_the_processor_share_their_launches(hiplib, tmp_path):
    """four sessions at once, shared launches in automatic mode: the adjustment rides behind each session's uploads in front of the
    shared front-end chain, and every session equals the single session fed adjusted frames"""
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h, n = 640, 480, 16
    F = _dimmed_stereo(w, h, n)
    G = [tuple(ir.adjust(e) for e in f) for f in F]
    b, _ = _run(_manager(manager, w, h, TRACKER % "true", tmp_path / "b.log", None), G, queue_first=False)
    b0, r0 = hiplib.shared_front_end_counters(0)
    four = [_manager(manager, w, h, TRACKER % "true", tmp_path / ("a%d.log" % i), "") for i in range(4)]
    out = [None] * 4

    def run(i):
        out[i] = _run(four[i], F, queue_first=False)
    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b1, r1 = hiplib.shared_front_end_counters(0)
    print("shared front ends: %d requests in %d launches" % (r1 - r0, b1 - b0))
    for poses, st in out:
        assert poses == b
        assert st["intensity_adjusted"] == n


def test_recording_session_tracks_and_records_the_adjusted_frames(hiplib, tmp_path, monkeypatch):
    """recording on: the host helper adjusts the frame for the recorder, the tracker uploads the adjusted pixels and the device has
    nothing left to do ("Processors"): poses and recorded frames equal those of a session fed adjusted frames"""
    from lpslam_amd import _build, manager
    _build.host_library()
    w, h, n = 640, 480, 12
    F = _dimmed_stereo(w, h, n)
    G = [tuple(ir.adjust(e) for e in f) for f in F]
    runs = {}
    for name, frames, proc in (("a", F, ""), ("b", G, None)):
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        m = _manager(manager, w, h, TRACKER % "true", d / "slam.log", proc)
        m.set_record(True)
        poses, st = _run(m, frames)
        files = glob.glob(str(d / "slam_*.pb"))
        assert len(files) == 1
        cams = [rr.camera_image(p) for t, p in rr.read_records(files[0]) if t == rr.CAMERA_IMAGE]
        runs[name] = (poses, st, cams)
    (pa, sa, ca), (pb, sb, cb) = runs["a"], runs["b"]
    assert pa == pb and sum(v for v, _, _ in pa) >= n - 2
    assert len(ca) == len(cb) == n
    for x, y in zip(ca, cb):
        assert x["timestamp"] == y["timestamp"] and x["image"] == y["image"] and x["image_second"] == y["image_second"]
    assert sa["intensity_adjusted"] == 0 and sb["intensity_adjusted"] == 0
    assert sa["prefetched"] == sb["prefetched"] == n - 1                          # the prefetch carried the host-adjusted pixels
