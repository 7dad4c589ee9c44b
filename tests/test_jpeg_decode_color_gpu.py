"""The device JPEG decoder on three-component (YCbCr) baseline streams (lpslam_hip_jpeg_dec_create2 with LPSLAM_HIP_JPEG_DEC_COLOR,
lpslam_amd/csrc/jpeg_dec.hip): component 0 of 4:4:4, 4:2:2 and 4:2:0 files, bit for bit what the host decoder
LpSlam::decode_jpeg_gray gives and what libjpeg gave as grey output when the fixture was written (tests/golden/g18_jpeg_color.npz,
tools/make_jpeg_color_fixture.py; tests/test_jpeg_color_cpu.py holds the host decoder to the same samples).  Everything that must
not skip reads the fixture; the two tests that need an encoder for larger frames ask for Pillow."""
import ctypes as C
import io
import json

import numpy as np
import pytest

from conftest import golden
from lpslam_amd import synth

pytestmark = pytest.mark.gpu

DECODED, NOT_TAKEN, IRREGULAR = 0, 1, 2
BIG = "noise_320x240_q75_420"                  # 47 kB, 361 subsequences: two workgroups of k_jdec_sync / k_jdec_write


@pytest.fixture(scope="module")
def fx():
    g = golden("g18_jpeg_color.npz")
    return dict(taken=[str(n) for n in g["names_taken"]], other=[str(n) for n in g["names_not_taken"]],
                jpeg={k[5:]: g[k].tobytes() for k in g.files if k.startswith("jpeg_")},
                grey={k[5:]: g[k] for k in g.files if k.startswith("grey_")})


@pytest.fixture(scope="module")
def host():
    from lpslam_amd import _build
    lib = C.CDLL(_build.host_library())
    enc = lib.lpslam_jpeg_encode_gray
    enc.restype = C.c_size_t
    enc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    dec = lib.lpslam_jpeg_decode_gray
    dec.restype = C.c_int
    dec.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]

    def encode(img, quality):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(4096 + 4 * img.size, np.uint8)
        n = enc(img.ctypes.data, img.shape[1], img.shape[0], int(quality), out.ctypes.data, out.size)
        assert n > 0
        return out[:n].tobytes()

    def decode(data):
        """the yardstick: (image or None)"""
        d = np.frombuffer(bytes(data), np.uint8).copy()
        out = np.zeros(1 << 20, np.uint8); w, h = C.c_int(0), C.c_int(0)
        rc = dec(d.ctypes.data, len(d), out.ctypes.data, out.size, C.byref(w), C.byref(h))
        assert rc in (0, 2)
        return out[:w.value * h.value].reshape(h.value, w.value).copy() if rc == 0 else None
    return dict(encode=encode, decode=decode, raw_decode=dec)


@pytest.fixture(scope="module")
def dec(hiplib):
    d = hiplib.JpegDecoder(1920, 1080, 4, color=True)
    yield d
    d.close()


def test_every_fixture_stream_equals_the_host_decoder_and_libjpeg(dec, host, fx):
    assert len(fx["taken"]) >= 20
    for name in fx["taken"]:
        data = fx["jpeg"][name]
        (status, img), = dec.decode([data])
        want = host["decode"](data)
        assert want is not None and status == DECODED, (name, status)
        assert img.shape == want.shape and np.array_equal(img, want), (name, img.shape, want.shape)
        assert np.array_equal(img, fx["grey"][name]), name


def test_the_long_constant_streams_need_the_hand_over(dec, host, fx):
    """a constant colour image is one short period of codes per MCU: a subsequence started at (0, DC next, place 0) stays out of step in
    some part of the state until the true state reaches it, so the states are handed over round by round"""
    for name in ("constant_640x480_q90_420", "constant_640x480_q90_444"):
        (status, img), = dec.decode([fx["jpeg"][name]])
        assert status == DECODED and np.array_equal(img, fx["grey"][name])
        rounds, subs, blocks = dec.last(1)[0]
        assert subs > 30 and 1 <= rounds <= subs + 1, (name, rounds, subs)
        if name.endswith("420"):                                       # 4:4:4 (three blocks an MCU) happens to fall into step at once
            assert rounds > 1, (rounds, subs)


def test_a_restart_interval_is_not_taken(dec, fx):
    data = fx["jpeg"]["restart_53x41_q90_420"]
    rc, status, w, h, outs = dec.decode_raw([data])
    assert rc == 0 and status[0] == NOT_TAKEN and (w[0], h[0]) == (53, 41) and (outs[0] == 0xA5).all()


def test_a_decoder_made_without_the_flag_leaves_colour_streams_alone(hiplib, fx):
    d = hiplib.JpegDecoder(640, 480, 2)
    for name in ("noise_53x41_q90_420", "noise_53x41_q90_444"):
        rc, status, w, h, outs = d.decode_raw([fx["jpeg"][name]])
        assert rc == 0 and status[0] == NOT_TAKEN and (w[0], h[0]) == (53, 41) and (outs[0] == 0xA5).all()
    d.close()


def test_a_batch_of_colour_and_grey_streams(dec, host, fx):
    grey = host["encode"](synth.StereoSequence(640, 480, 4).frame(0)[0][:200, :312], 95)
    batch = [fx["jpeg"]["synth_320x240_q95_420"], grey, fx["jpeg"]["noise_96x64_q95_optimised_444"], fx["jpeg"]["noise_53x41_q90_422"]]
    res = dec.decode(batch)
    for data, (status, img) in zip(batch, res):
        assert status == DECODED and np.array_equal(img, host["decode"](data))
    # a smaller colour call after a larger one: nothing of the first is left
    small = [fx["jpeg"]["noise_17x16_q90_420"], fx["jpeg"]["constant_64x48_q90_444"]]
    for data, (status, img) in zip(small, dec.decode(small)):
        assert status == DECODED and np.array_equal(img, host["decode"](data))


def test_a_cut_stream_is_irregular(dec, fx):
    data = fx["jpeg"][BIG]
    rc, status, w, h, outs = dec.decode_raw([data[:len(data) // 2]])
    assert rc == 0 and status[0] == IRREGULAR and (w[0], h[0]) == (320, 240) and (outs[0] == 0xA5).all()


def test_a_flipped_byte_never_decodes_to_other_samples(dec, host, fx):
    """one fixed byte in the middle of the entropy-coded data inverted, once: decoded with the host decoder's samples, or irregular"""
    data = bytearray(fx["jpeg"][BIG])
    data[len(data) // 2] ^= 0xFF
    (status, img), = dec.decode([bytes(data)])
    assert status in (DECODED, IRREGULAR)
    if status == DECODED:
        want = host["decode"](bytes(data))
        assert want is not None and np.array_equal(img, want)


def test_stride_and_capacity(dec, fx):
    pair = [fx["jpeg"][BIG], fx["jpeg"]["synth_320x240_q95_420"]]
    want = [fx["grey"][BIG], fx["grey"]["synth_320x240_q95_420"]]
    rc, status, w, h, outs = dec.decode_raw(pair[:1], caps=[500 * 240], strides=[500])       # a row stride larger than the width
    assert rc == 0 and status[0] == DECODED
    assert np.array_equal(outs[0].reshape(240, 500)[:, :320], want[0]) and (outs[0].reshape(240, 500)[:, 320:] == 0xA5).all()
    rc, status, w, h, outs = dec.decode_raw(pair, caps=[320 * 240, 320 * 240 - 1], strides=[320, 320])      # one byte short
    assert rc == 1                                                     # LPSLAM_HIP_ERR_INVALID
    assert list(w) == [320, 320] and list(h) == [240, 240]
    assert all((o == 0xA5).all() for o in outs)                        # untouched
    rc, status, w, h, outs = dec.decode_raw(pair, caps=[320 * 240, 320 * 240], strides=[320, 320])
    assert rc == 0 and list(status) == [DECODED, DECODED]
    assert all(np.array_equal(o.reshape(240, 320), g) for o, g in zip(outs, want))


def test_the_same_batch_three_times_gives_identical_bytes(dec, fx):
    batch = [fx["jpeg"][n] for n in ("synth_320x240_q95_420", BIG, "noise_96x64_q95_optimised_444", "noise_53x41_q90_422")]
    runs = [dec.decode(batch) for _ in range(3)]
    for r in runs[1:]:
        for (s0, a), (s1, b) in zip(runs[0], r):
            assert s0 == s1 == DECODED and a.tobytes() == b.tobytes()


def test_last_counts_the_blocks_of_all_components(dec, fx):
    (status, _), = dec.decode([fx["jpeg"][BIG]])
    assert status == DECODED
    rounds, subs, blocks = dec.last(1)[0]
    assert blocks == 20 * 15 * 6
    assert subs > 256 and 1 <= rounds <= subs + 1, (rounds, subs)


def test_create2_refuses_unknown_flag_bits(hiplib):
    lib = hiplib.load()
    lib.lpslam_hip_jpeg_dec_create2.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p]
    for flags in (2, 3, 0x80000000):
        h = C.c_void_p()
        assert lib.lpslam_hip_jpeg_dec_create2(64, 48, 1, flags, C.byref(h)) == 1 and not h.value       # LPSLAM_HIP_ERR_INVALID
    h = C.c_void_p()
    assert lib.lpslam_hip_jpeg_dec_create2(64, 48, 1, 0, C.byref(h)) == 0 and h.value
    lib.lpslam_hip_jpeg_dec_destroy.argtypes = [C.c_void_p]
    lib.lpslam_hip_jpeg_dec_destroy(h)


def _manager(tmp_path, color_device):
    from lpslam_amd import _build, manager
    _build.host_library()
    m = manager.Manager()
    k = synth.intrinsics(320, 240)
    c = manager.default_camera()
    c.camera_number = 0; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]; c.resolution_x = 320; c.resolution_y = 240
    m.set_camera(c)
    section = {"require_odometry": False}
    if color_device is not None:
        section[manager.JPEG_DECODE_COLOR_DEVICE_KEY] = bool(color_device)
    cfg = tmp_path / ("color_%s.json" % color_device)
    cfg.write_text(json.dumps({"manager": section}))
    assert m.read_configuration_file(str(cfg))
    return m


def test_colour_frames_handed_to_the_manager(hiplib, host, fx, tmp_path):
    names = ["synth_320x240_q95_420", BIG, "noise_96x64_q95_optimised_444", "noise_53x41_q90_422"]
    grey = host["encode"](fx["grey"][BIG], 95)
    for color_device, want in ((None, (4, 0, 0)), (True, (4, 0, 0)), (False, (0, 4, 0))):
        m = _manager(tmp_path, color_device)
        for i, name in enumerate(names):
            assert m.add_jpeg((i + 1) * 40_000_000, fx["jpeg"][name], ros=False)
        assert m.decoder_counters() == dict(device_images=want[0], host_images=want[1], refused_images=want[2]), color_device
        assert m.add_jpeg(5 * 40_000_000, grey, ros=False)                         # grey streams go to the device whatever the key says
        assert m.decoder_counters()["device_images"] == want[0] + 1
        assert m.add_jpeg(6 * 40_000_000, fx["jpeg"]["restart_53x41_q90_420"], ros=False)      # not of the class: the host, as before
        assert m.decoder_counters() == dict(device_images=want[0] + 1, host_images=want[1] + 1, refused_images=0)


def _pillow_colour(g, **kw):
    Image = pytest.importorskip("PIL.Image")
    rgb = np.dstack([g, np.roll(g, 7, 1), np.roll(g, 11, 0)])
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", **kw)
    return buf.getvalue(), Image


def test_pillow_streams_of_a_synth_frame(dec, host):
    g = synth.StereoSequence(640, 480, 4).frame(0)[0]
    for subsampling in (0, 1, 2):
        data, Image = _pillow_colour(g, quality=75, subsampling=subsampling)
        (status, img), = dec.decode([data])
        assert status == DECODED and np.array_equal(img, host["decode"](data))
        im = Image.open(io.BytesIO(data)); im.draft("L", im.size); im.load()
        assert im.mode == "L" and np.array_equal(img, np.asarray(im))


def test_the_colour_stereo_pair_is_decoded_more_than_twice_as_fast_as_on_the_host(dec, host):
    """1280 x 720 synth made colour, quality 95, 4:2:0, the two eyes in one call, streams in host memory in, samples in host memory out:
    the median of 21 wall clocks after a warm-up against the host decoder on the same two streams in the same run, one thread.  2: two
    host threads would give 2 without any device code.  Measured on an MI355X: 3.13 ms against 17.2 ms, 5.5 times."""
    import time
    pair_g = synth.StereoSequence(1280, 720, 4).frame(0)              # the frames of tools/time_jpeg_decode_color.py
    pair = [np.frombuffer(_pillow_colour(g, quality=95, subsampling=2)[0], np.uint8).copy() for g in pair_g]
    outs = [np.empty(1280 * 720, np.uint8) for _ in pair]
    sp = (C.c_void_p * 2)(*[s.ctypes.data for s in pair]); op = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    ss = np.array([len(s) for s in pair], np.int64); st = np.array([1280, 1280], np.int32); cp = np.array([1280 * 720] * 2, np.int64)
    ws = np.zeros(2, np.int32); hs = np.zeros(2, np.int32); status = np.zeros(2, np.int32)

    def call():
        return dec.lib.lpslam_hip_jpeg_decode(dec.h, 2, sp, ss.ctypes.data, op, st.ctypes.data, cp.ctypes.data, ws.ctypes.data, hs.ctypes.data, status.ctypes.data)
    for _ in range(3):
        assert call() == 0 and list(status) == [DECODED, DECODED]
    td = []
    for _ in range(21):
        t0 = time.perf_counter(); rc = call(); td.append(time.perf_counter() - t0)
        assert rc == 0
    hb = [np.empty(1280 * 720, np.uint8) for _ in pair]            # the host side as the device side: buffers made before, one direct call
    hw, hh = C.c_int(0), C.c_int(0)
    hdec = host["raw_decode"]
    for _ in range(3):
        assert [hdec(s.ctypes.data, len(s), b.ctypes.data, b.size, C.byref(hw), C.byref(hh)) for s, b in zip(pair, hb)] == [0, 0]
    th = []
    for _ in range(21):
        t0 = time.perf_counter()
        rcs = [hdec(s.ctypes.data, len(s), b.ctypes.data, b.size, C.byref(hw), C.byref(hh)) for s, b in zip(pair, hb)]
        th.append(time.perf_counter() - t0)
        assert rcs == [0, 0]
    assert all(np.array_equal(o, b) for o, b in zip(outs, hb))
    device_ms, host_ms = float(np.median(td)) * 1e3, float(np.median(th)) * 1e3
    print("device pair %.3f ms, host pair %.3f ms, ratio %.1f, rounds %s" % (device_ms, host_ms, host_ms / device_ms, dec.last(2)))
    assert host_ms > 2.0 * device_ms, (device_ms, host_ms)
