"""Colour and YUV frames at ingest, on the device (lpslam_amd/csrc/ingest.hip): the three colour calls of the C ABI against the numpy
restatement in tests/ingest_ref.py, and the end-to-end equivalence through LpSlamManager -- a session fed colour frames F tracks
exactly what a session fed grey(F) as 8UC1 tracks.  Every comparison is exact."""
import ctypes as C
import glob
import threading
import time

import numpy as np
import pytest

import ingest_ref as ref
import intensity_ref as ir
import record_reader as rr
from lpslam_amd import synth

pytestmark = pytest.mark.gpu

COLOUR = (ref.RGB8, ref.BGR8, ref.NV12, ref.UYVY)


def read_slot(ctx, image):
    """level 0 of a slot and its row padding, as tests/test_processor_gpu.py reads them: (pixels, padding)"""
    hip_memcpy = ctx.lib.hipMemcpy
    hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    ctx.sync()
    ptr, pitch = ctx.image_ptr(image)
    h, w = ctx.cfg.height, ctx.cfg.width
    buf = np.zeros((h, pitch), np.uint8)
    assert hip_memcpy(buf.ctypes.data, ptr, buf.size, 2) == 0             # hipMemcpyDeviceToHost
    return buf[:, :w].copy(), buf[:, w:].copy()


def formats_for(w, h):
    return [f for f in COLOUR if not (f == ref.NV12 and (w | h) & 1) and not (f == ref.UYVY and w & 1)]


def widened(buf, extra=13):
    """the frame's rows inside a wider buffer: (the wide array, its view of the frame's rows)"""
    rows = buf.reshape(buf.shape[0], -1)
    wide = np.full((rows.shape[0], rows.shape[1] + extra), 0x5A, np.uint8)
    wide[:, :rows.shape[1]] = rows
    return wide


# ---- the slot call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(65, 64), (333, 77), (66, 64), (322, 64), (64, 64), (640, 480)])
def test_slot_call_equals_the_numpy_restatement(hiplib, w, h):
    ctx = hiplib.Context(w, h, 300, 1.2, 2, max_images=2)
    try:
        fmts = formats_for(w, h)
        assert len(fmts) == (2 if w & 1 else 4)
        assert not read_slot(ctx, 0)[1].any() and not read_slot(ctx, 1)[1].any()
        # consecutive calls on the same slots, another format each time: every one gives its own frame's grey
        for i, fmt in enumerate(fmts + fmts):
            a, b = ref.random_frame(fmt, w, h, 10 + i), ref.random_frame(fmts[(i + 1) % len(fmts)], w, h, 30 + i)
            ctx.upload_pixels(0, hiplib.Pixels(a, fmt))
            ctx.upload_pixels(1, hiplib.Pixels(b, fmts[(i + 1) % len(fmts)]))
            for slot, buf, f in ((0, a, fmt), (1, b, fmts[(i + 1) % len(fmts)])):
                got, pad = read_slot(ctx, slot)
                assert np.array_equal(got, ref.grey(buf, f)), (slot, f)
                assert not pad.any()                                              # the destination's row padding is never written
        # a source stride larger than the row; NV12 also with chroma rows of their own
        for fmt in fmts:
            buf = ref.random_frame(fmt, w, h, 50 + fmt)
            wide = widened(buf)
            ctx.upload_pixels(0, hiplib.Pixels(wide, fmt))
            assert np.array_equal(read_slot(ctx, 0)[0], ref.grey(buf, fmt)), fmt
            if fmt == ref.NV12:
                chroma = widened(buf[h:], 7)
                ctx.upload_pixels(1, hiplib.Pixels(wide[:h], fmt, chroma=chroma))
                assert np.array_equal(read_slot(ctx, 1)[0], ref.grey(buf, fmt))
        # GRAY8 through the new call is the grey call
        g = synth.random_image(w, h, 3)
        ctx.upload_pixels(1, hiplib.Pixels(g, ref.GRAY8))
        assert np.array_equal(read_slot(ctx, 1)[0], g) and not read_slot(ctx, 1)[1].any()
        # the grey call after a colour one on the same slot
        ctx.upload(0, g)
        assert np.array_equal(read_slot(ctx, 0)[0], g)
    finally:
        ctx.close()


def test_every_rgb_and_nv12_triple_on_the_device(hiplib):
    ctx = hiplib.Context(512, 512, 300, 1.2, 2, max_images=2)
    try:
        for k in range(64):
            img = ref.rgb_sweep(k)
            ctx.upload_pixels(0, hiplib.Pixels(img, ref.RGB8)); ctx.upload_pixels(1, hiplib.Pixels(img, ref.BGR8))
            assert np.array_equal(read_slot(ctx, 0)[0], ref.grey(img, ref.RGB8)), k
            assert np.array_equal(read_slot(ctx, 1)[0], ref.grey(img, ref.BGR8)), k
        for k in range(0, 64, 2):
            a, b = ref.nv12_sweep(k), ref.nv12_sweep(k + 1)
            ctx.upload_pixels(0, hiplib.Pixels(a, ref.NV12)); ctx.upload_pixels(1, hiplib.Pixels(b, ref.NV12))
            assert np.array_equal(read_slot(ctx, 0)[0], ref.grey_nv12(a)), k
            assert np.array_equal(read_slot(ctx, 1)[0], ref.grey_nv12(b)), k + 1
    finally:
        ctx.close()


def test_every_uyvy_triple_on_the_device(hiplib):
    ctx = hiplib.Context(512, 256, 300, 1.2, 2, max_images=2)
    try:
        for k in range(0, 128, 2):
            a, b = ref.uyvy_sweep(k), ref.uyvy_sweep(k + 1)
            ctx.upload_pixels(0, hiplib.Pixels(a, ref.UYVY)); ctx.upload_pixels(1, hiplib.Pixels(b, ref.UYVY))
            assert np.array_equal(read_slot(ctx, 0)[0], ref.grey_uyvy(a)), k
            assert np.array_equal(read_slot(ctx, 1)[0], ref.grey_uyvy(b)), k + 1
        for (y, u, v), want in ref.WORKED_YUV.items():
            buf = np.empty((256, 1024), np.uint8)
            buf[:, 0::4] = u; buf[:, 2::4] = v; buf[:, 1::2] = y
            ctx.upload_pixels(0, hiplib.Pixels(buf, ref.UYVY))
            assert np.all(read_slot(ctx, 0)[0] == want), (y, u, v)
    finally:
        ctx.close()


# ---- the raw path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(320, 240), (65, 64)])
def test_raw_path_converts_then_adjusts_then_remaps(hiplib, w, h):
    ctx = hiplib.Context(w, h, 300, 1.2, 2, max_images=2)
    ctx2 = hiplib.Context(w, h, 300, 1.2, 2, max_images=2)
    try:
        rng = np.random.default_rng(5)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        maps = [(xx + rng.uniform(-4, 4, xx.shape).astype(np.float32), yy + rng.uniform(-4, 4, xx.shape).astype(np.float32)),
                (xx * 1.1 - 5, yy * 1.15 - 4)]
        for c in (ctx, ctx2):
            for eye in (0, 1):
                c.set_rectify_map(eye, *maps[eye])
        for i, fmt in enumerate(formats_for(w, h)):
            eye = i & 1
            buf = (ref.random_frame(fmt, w, h, 70 + i).astype(np.float64) * 0.3 + 40).astype(np.uint8)      # flat: the adjustment matters
            grey = ref.grey(buf, fmt)
            # the existing grey calls on numpy's conversion (and numpy's adjustment) are the expectation
            for params in (None, hiplib.AdjustParams(), hiplib.AdjustParams(0.0, 1.0, 0.02, 0.98)):
                if params is None:
                    ctx2.upload_raw(eye, eye, grey)
                else:
                    ctx2.upload_raw(eye, eye, ir.adjust(grey, params.low_out, params.high_out, params.low_fraction, params.high_fraction))
                ctx.upload_raw_pixels(eye, eye, hiplib.Pixels(buf, fmt), params)
                got, pad = read_slot(ctx, eye)
                assert np.array_equal(got, read_slot(ctx2, eye)[0]), (fmt, params is not None)
                assert not pad.any()
                if params is not None:
                    lo, hi, hist = ir.limits(grey, params.low_fraction, params.high_fraction)
                    glo, ghi, ghist = ctx.adjust_intensity_last(eye)
                    assert (glo, ghi) == (lo, hi) and np.array_equal(ghist, hist)  # the histogram is the CONVERTED raw frame's
            assert not np.array_equal(ir.adjust(grey), grey)
        # GRAY8 through the new call is the existing raw call
        g = synth.random_image(w, h, 8)
        ctx.upload_raw_pixels(0, 0, hiplib.Pixels(g, ref.GRAY8)); ctx2.upload_raw(0, 0, g)
        assert np.array_equal(read_slot(ctx, 0)[0], read_slot(ctx2, 0)[0])
    finally:
        ctx.close(); ctx2.close()


# ---- the one-call front end -------------------------------------------------------------------------------------------------------
def affine_rgb(img):
    """three different affine maps of one grey frame: the channels differ, the picture stays trackable"""
    f = img.astype(np.float64)
    return np.stack([f * 0.9 + 10, f * 0.7 + 40, f * 0.5 + 90], axis=-1).clip(0, 255).astype(np.uint8)


def yuv_planes(img):
    """Y, U, V planes (U, V at half resolution) of a trackable limited-range picture whose chroma varies with the frame"""
    f = img.astype(np.float64)
    y = (16 + f * 0.8).astype(np.uint8)
    sub = f[0::2, 0::2]
    return y, (128 + (sub - 128) * 0.25).astype(np.uint8), (128 - (sub - 128) * 0.2).astype(np.uint8)


def nv12_of(img):
    y, u, v = yuv_planes(img)
    return np.concatenate([y, np.stack([u, v], axis=-1).reshape(u.shape[0], -1)], axis=0)


def uyvy_of(img):
    y, u, v = yuv_planes(img)
    h, w = y.shape
    out = np.empty((h, w // 2, 4), np.uint8)
    out[..., 0] = np.repeat(u, 2, axis=0); out[..., 2] = np.repeat(v, 2, axis=0)      # 4:2:2: the chroma rows doubled
    out[..., 1] = y[:, 0::2]; out[..., 3] = y[:, 1::2]
    return out.reshape(h, 2 * w)


def colour_of(img, fmt):
    return {ref.RGB8: affine_rgb, ref.BGR8: affine_rgb, ref.NV12: nv12_of, ref.UYVY: uyvy_of}[fmt](img)


@pytest.mark.parametrize("prefetch", [False, True])
def test_front_end_pixels_extracts_the_converted_frame(hiplib, prefetch):
    w, h = 640, 480
    k = synth.intrinsics(w, h)
    l, r = synth.StereoSequence(w, h, 4, n_points=6000).frame(0)
    ctx = hiplib.Context(w, h, 1000, 1.2, 4, max_images=4)
    try:
        for i, (fl, fr) in enumerate(((ref.RGB8, ref.RGB8), (ref.BGR8, ref.NV12), (ref.NV12, ref.NV12), (ref.UYVY, ref.UYVY), (ref.UYVY, ref.GRAY8))):
            cl, cr = colour_of(l, fl), (colour_of(r, fr) if fr != ref.GRAY8 else r)
            gl, gr = ref.grey(cl, fl), ref.grey(cr, fr)
            slot = 2 if prefetch else 0
            params = hiplib.AdjustParams() if i & 1 else None
            if prefetch:
                with ctx.prefetch():
                    ctx.front_end_pixels(slot, hiplib.Pixels(cl, fl), hiplib.Pixels(cr, fr), k["fxb"], k["baseline"], params)
                ctx.prefetch_join()
            else:
                ctx.front_end_pixels(slot, hiplib.Pixels(cl, fl), hiplib.Pixels(cr, fr), k["fxb"], k["baseline"], params)
            got = ctx.frame(slot)
            if params is not None:
                gl, gr = ir.adjust(gl), ir.adjust(gr)
            assert np.array_equal(read_slot(ctx, slot)[0], gl) and np.array_equal(read_slot(ctx, slot + 1)[0], gr)
            ctx.front_end_images(0, gl, gr, k["fxb"], k["baseline"])              # the existing grey call on the converted picture
            want = ctx.frame(0)
            assert len(got[0]) == len(want[0]) > 100
            for g, w_ in zip(got, want):
                assert np.array_equal(g, w_)
        # monocular
        c = affine_rgb(l)
        ctx.front_end_pixels(0, hiplib.Pixels(c, ref.RGB8)); got = ctx.frame(0)
        ctx.front_end_images(0, ref.grey(c, ref.RGB8)); want = ctx.frame(0)
        assert len(got[0]) > 100 and all(np.array_equal(g, w_) for g, w_ in zip(got[:2], want[:2]))
    finally:
        ctx.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def _rc(hiplib, call):
    with pytest.raises(hiplib.LpslamHipError) as e:
        call()
    return int(str(e.value).split("error ")[1].split(":")[0])


def test_error_paths_return_the_stated_codes_and_touch_nothing(hiplib):
    INVALID, CAPACITY = 1, 3
    P = hiplib.Pixels
    for w, h, bad_fmts in ((65, 64, (ref.NV12, ref.UYVY)), (66, 65, (ref.NV12,))):      # an odd width / height where the format needs an even one
        ctx = hiplib.Context(w, h, 300, 1.2, 2, max_images=2)
        try:
            img = synth.random_image(w, h, 2)
            ctx.upload(0, img); ctx.upload(1, img)
            big = np.zeros((2 * h, 4 * w), np.uint8)
            for fmt in bad_fmts:
                assert _rc(hiplib, lambda: ctx.upload_pixels(0, P(big, fmt))) == INVALID
                assert _rc(hiplib, lambda: ctx.front_end_pixels(0, P(big, fmt), P(big, ref.RGB8), 50.0, 0.1)) == INVALID
                assert _rc(hiplib, lambda: ctx.front_end_pixels(0, P(big, ref.RGB8), P(big, fmt), 50.0, 0.1)) == INVALID
            for fmt in (5, -1, 99):                                                      # an unknown format
                assert _rc(hiplib, lambda: ctx.upload_pixels(1, P(big, fmt))) == INVALID
                assert _rc(hiplib, lambda: ctx.front_end_pixels(0, P(big, ref.GRAY8), P(big, fmt), 50.0, 0.1)) == INVALID
            assert _rc(hiplib, lambda: ctx.upload_pixels(0, P(big, ref.RGB8, stride=3 * w - 1))) == INVALID      # a stride smaller than a row
            assert _rc(hiplib, lambda: ctx.upload_pixels(0, P(big, ref.GRAY8, stride=w - 1))) == INVALID
            if not w & 1:
                assert _rc(hiplib, lambda: ctx.upload_pixels(0, P(big, ref.UYVY, stride=2 * w - 1))) == INVALID
            assert _rc(hiplib, lambda: ctx.upload_pixels(2, P(big, ref.RGB8))) == CAPACITY
            assert _rc(hiplib, lambda: ctx.upload_pixels(-1, P(big, ref.RGB8))) == CAPACITY
            assert _rc(hiplib, lambda: ctx.front_end_pixels(1, P(big, ref.RGB8), P(big, ref.RGB8), 50.0, 0.1)) == CAPACITY
            assert _rc(hiplib, lambda: ctx.front_end_pixels(0, P(big, ref.RGB8), P(big, ref.RGB8), 50.0, 0.1, hiplib.AdjustParams(1.0, 1.0))) == INVALID
            assert _rc(hiplib, lambda: ctx.upload_raw_pixels(0, 0, P(big, ref.RGB8))) == INVALID             # no rectify map
            f = ctx.lib.lpslam_hip_upload_pixels
            f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            assert f(ctx.h, 0, None) == INVALID and b"null" in ctx.lib.lpslam_hip_last_error()
            null = P(big, ref.RGB8); null.data = None
            assert _rc(hiplib, lambda: ctx.upload_pixels(0, null)) == INVALID
            for slot in (0, 1):
                assert np.array_equal(read_slot(ctx, slot)[0], img)                     # nothing was enqueued
        finally:
            ctx.close()
    ctx = hiplib.Context(64, 64, 300, 1.2, 2, max_images=2)
    try:
        ctx.set_rectify_map(0, *np.mgrid[0:64, 0:64].astype(np.float32)[::-1])
        img = synth.random_image(64, 64, 2)
        ctx.upload_raw(0, 0, img)
        before = read_slot(ctx, 0)[0]
        big = np.zeros((128, 256), np.uint8)
        assert _rc(hiplib, lambda: ctx.upload_raw_pixels(0, 0, P(big, 7))) == INVALID
        assert _rc(hiplib, lambda: ctx.upload_raw_pixels(0, 0, P(big, ref.NV12, stride=63))) == INVALID
        assert _rc(hiplib, lambda: ctx.upload_raw_pixels(0, 0, P(big, ref.RGB8), hiplib.AdjustParams(2.0, 1.0))) == INVALID
        assert _rc(hiplib, lambda: ctx.upload_raw_pixels(0, 2, P(big, ref.RGB8))) == INVALID
        assert np.array_equal(read_slot(ctx, 0)[0], before)
    finally:
        ctx.close()


# ---- through the manager ------------------------------------------------------------------------------------------------------------
TRACKER = '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "asyncMapping": false, "prefetch": %s}'
W, H = 640, 480          # the size of tests/test_processor_gpu.py's session tests


def _manager(manager, tracker_cfg, log, processor=None, setup_camera=None, mono=False):
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in ((0,) if mono else (0, 1)):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
        if setup_camera:
            setup_camera(c)
        m.set_camera(c)
    assert m.add_tracker("VSLAMMono" if mono else "VSLAMStereo", tracker_cfg)
    if processor is not None:
        assert m.add_processor("AdjustIntensity", processor)
    m.collect_results(); m.provide_odometry()
    m.log_to_file(log)
    return m


def _run(m, feeds, queue_first=True):
    """feeds: one callable (manager, timestamp) -> bool per frame"""
    def feed():
        for i, f in enumerate(feeds):
            assert f(m, (i + 1) * 40_000_000)
    if queue_first:           # queued before the worker starts: every frame has a successor waiting (the prefetch path carries it)
        feed(); m.start()
    else:
        m.start(); feed()
    t0 = time.time()
    while len(m.results) < len(feeds) and time.time() - t0 < 90:
        time.sleep(0.01)
    m.stop()
    assert len(m.results) == len(feeds)
    return [(r["valid"], tuple(r["p"]), tuple(r["q"])) for r in m.results], m.tracker_statistics()


def feed_colour(manager, fmt, left, right):
    """one stereo frame as a client has it in `fmt`, and what the tracker must see: (feed callable, (grey left, grey right))"""
    cl, cr = colour_of(left, fmt), colour_of(right, fmt)
    grey = (ref.grey(cl, fmt), ref.grey(cr, fmt))
    if fmt in (ref.RGB8, ref.BGR8):
        conv = manager.CONVERSION_BGR2RGB if fmt == ref.BGR8 else manager.CONVERSION_NONE
        return (lambda m, ts: m.add_stereo(ts, cl, cr, fmt=manager.FORMAT_8UC3, conversion=conv)), grey
    # LeftTop_RightBottom as the reference lays the YUV formats out: the UPPER block is the right camera's picture, the LOWER the left's
    buf = np.concatenate([cr.reshape(-1), cl.reshape(-1)])
    mf = manager.FORMAT_NV12 if fmt == ref.NV12 else manager.FORMAT_YUV16
    return (lambda m, ts: m.add_buffer(ts, buf, W, 2 * H, mf, manager.STEREO_LEFT_TOP_RIGHT_BOTTOM)), grey


def feed_grey(pair):
    return lambda m, ts: m.add_stereo(ts, *pair)


@pytest.fixture(scope="module")
def stereo_frames():
    seq = synth.StereoSequence(W, H, 4, n_points=6000)
    return [seq.frame(i) for i in range(12)]


@pytest.fixture(scope="module")
def mgr(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    return manager


@pytest.mark.parametrize("fmt", COLOUR)
def test_session_fed_colour_frames_equals_a_session_fed_their_grey(mgr, stereo_frames, tmp_path, fmt):
    n = len(stereo_frames)
    fed = [feed_colour(mgr, fmt, l, r) for l, r in stereo_frames]
    a, sa = _run(_manager(mgr, TRACKER % "true", tmp_path / "a.log"), [f for f, _ in fed])
    b, sb = _run(_manager(mgr, TRACKER % "true", tmp_path / "b.log"), [feed_grey(g) for _, g in fed])
    assert a == b and sum(v for v, _, _ in a) >= n - 2
    assert sa["color_converted"] == n and sb["color_converted"] == 0
    assert sa["prefetched"] == sb["prefetched"] == n - 1
    for key in ("frames", "keyframes", "landmarks", "motion_tracked", "local_ba"):
        assert sa[key] == sb[key], key
    if fmt == ref.RGB8:      # the channels differ: the grey of the other byte order is another picture
        assert not np.array_equal(fed[0][1][0], ref.grey(colour_of(stereo_frames[0][0], fmt), ref.BGR8))


def test_session_without_prefetch_and_with_the_processor_counts_both(mgr, stereo_frames, tmp_path):
    n = len(stereo_frames)
    dimmed = [tuple((e.astype(np.float64) * 0.2 + 8).astype(np.uint8) for e in f) for f in stereo_frames]
    for prefetch in ("false", "true"):
        fed = [feed_colour(mgr, ref.RGB8 if i & 1 else ref.NV12, l, r) for i, (l, r) in enumerate(dimmed)]      # the format may change from frame to frame
        a, sa = _run(_manager(mgr, TRACKER % prefetch, tmp_path / "a.log", ""), [f for f, _ in fed])
        b, sb = _run(_manager(mgr, TRACKER % prefetch, tmp_path / "b.log"), [feed_grey(tuple(ir.adjust(e) for e in g)) for _, g in fed])
        assert a == b and sum(v for v, _, _ in a) >= n - 2
        assert sa["color_converted"] == n and sa["intensity_adjusted"] == n
        assert sb["color_converted"] == 0 and sb["intensity_adjusted"] == 0
        assert sa["prefetched"] == (n - 1 if prefetch == "true" else 0)


def test_raw_path_session_equals_a_session_fed_grey_raw_frames(mgr, stereo_frames, tmp_path):
    """cameras with distortion: the tracker rectifies on the device, behind the conversion (and the adjustment)"""
    from oracle import rectify as rect
    n = len(stereo_frames)
    k = synth.intrinsics(W, H)
    K = np.array([[k["fx"], 0, k["cx"]], [0, k["fy"], k["cy"]], [0, 0, 1.0]])
    D = np.array([-0.05, 0.01, 0.0003, -0.0002, 0.0])
    T = np.array([-k["baseline"], 0.0, 0.0])
    R1, R2, P1, P2 = rect.stereo_rectify(K, D, K, D, (W, H), np.eye(3), T)

    def raw_from_ideal(img, Rk, P):      # as tests/test_processor_gpu.py builds its raw frames
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
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
        c.distortion_function = mgr.PINHOLE
        for i, v in enumerate(D):
            c.dist[i] = v
        for i, v in enumerate(T):
            c.translation[i] = v

    raws = [(raw_from_ideal(l, R1, P1), raw_from_ideal(r, R2, P2)) for l, r in stereo_frames]
    for processor, fmt in ((None, ref.UYVY), ("", ref.RGB8)):
        fed = [feed_colour(mgr, fmt, l, r) for l, r in raws]
        adj = (lambda e: ir.adjust(e)) if processor is not None else (lambda e: e)
        a, sa = _run(_manager(mgr, TRACKER % "true", tmp_path / "a.log", processor, camera), [f for f, _ in fed])
        b, sb = _run(_manager(mgr, TRACKER % "true", tmp_path / "b.log", None, camera), [feed_grey(tuple(adj(e) for e in g)) for _, g in fed])
        assert a == b and sum(v for v, _, _ in a) >= n - 3
        assert sa["color_converted"] == n and sa["intensity_adjusted"] == (n if processor is not None else 0) and sa["prefetched"] == n - 1


def test_monocular_session_equals_a_session_fed_grey_frames(mgr, tmp_path):
    n = 24
    seq = synth.WallSequence(W, H, 11)
    F = [affine_rgb(seq.frame(i)) for i in range(n)]
    cfg = '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4, "asyncMapping": false}'
    a, sa = _run(_manager(mgr, cfg, tmp_path / "a.log", mono=True),
                 [(lambda m, ts, f=f: m.add_buffer(ts, f, W, H, mgr.FORMAT_8UC3, mgr.ONE_IMAGE, mgr.CONVERSION_BGR2RGB)) for f in F])
    b, sb = _run(_manager(mgr, cfg, tmp_path / "b.log", mono=True), [(lambda m, ts, f=f: m.add_image(ts, ref.grey(f, ref.BGR8))) for f in F])
    assert a == b and sa["color_converted"] == n and sb["color_converted"] == 0
    assert sum(v for v, _, _ in a) >= n - 14


def test_four_managers_fed_colour_frames_share_their_launches(hiplib, mgr, stereo_frames, tmp_path):
    """four sessions at once, shared launches in automatic mode: the conversion rides behind each session's uploads in front of the
    shared front-end chain, and every session equals the single session fed grey frames"""
    n = len(stereo_frames)
    fed = [feed_colour(mgr, ref.NV12, l, r) for l, r in stereo_frames]
    b, _ = _run(_manager(mgr, TRACKER % "true", tmp_path / "b.log"), [feed_grey(g) for _, g in fed], queue_first=False)
    b0, r0 = hiplib.shared_front_end_counters(0)
    four = [_manager(mgr, TRACKER % "true", tmp_path / ("a%d.log" % i)) for i in range(4)]
    out = [None] * 4

    def run(i):
        out[i] = _run(four[i], [f for f, _ in fed], queue_first=False)
    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b1, r1 = hiplib.shared_front_end_counters(0)
    print("shared front ends: %d requests in %d launches" % (r1 - r0, b1 - b0))
    for poses, st in out:
        assert poses == b
        assert st["color_converted"] == n


def test_recording_session_records_the_grey_frames_and_takes_the_host_path(mgr, stereo_frames, tmp_path, monkeypatch):
    """recording on: the host function converts the frame for the recorder, the tracker uploads grey pixels and the device has nothing
    left to convert: poses and recorded frames equal those of a session fed grey frames"""
    frames = stereo_frames[:8]
    n = len(frames)
    fed = [feed_colour(mgr, ref.UYVY, l, r) for l, r in frames]
    runs = {}
    for name, feeds in (("a", [f for f, _ in fed]), ("b", [feed_grey(g) for _, g in fed])):
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        m = _manager(mgr, TRACKER % "true", d / "slam.log")
        m.set_record(True)
        poses, st = _run(m, feeds)
        files = glob.glob(str(d / "slam_*.pb"))
        assert len(files) == 1
        runs[name] = (poses, st, [rr.camera_image(p) for t, p in rr.read_records(files[0]) if t == rr.CAMERA_IMAGE])
    (pa, sa, ca), (pb, sb, cb) = runs["a"], runs["b"]
    assert pa == pb and sum(v for v, _, _ in pa) >= n - 2
    assert len(ca) == len(cb) == n
    for x, y in zip(ca, cb):
        assert x["timestamp"] == y["timestamp"] and x["image"] == y["image"] and x["image_second"] == y["image_second"]
    assert sa["color_converted"] == 0 and sb["color_converted"] == 0              # the host path was taken
    assert sa["prefetched"] == sb["prefetched"] == n - 1                          # the prefetch carried the host-converted pixels
