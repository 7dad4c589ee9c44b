"""The device JPEG decoder on streams with a restart interval (lpslam_hip_jpeg_dec_take_restart, lpslam_amd/csrc/jpeg_dec.hip): a DRI
segment in the header, RSTn markers in the entropy-coded data, one component or one interleaved Y/Cb/Cr scan.  Bit for bit what the
host decoder LpSlam::decode_jpeg_gray gives and what libjpeg gave when the fixture was written (tests/golden/g19_jpeg_restart.npz,
tools/make_jpeg_restart_fixture.py; tests/test_jpeg_restart_cpu.py holds the host decoder to the same samples).  The switch is off
by default: the same streams on a decoder without it are left to the host.  Nothing here needs Pillow: larger frames come from the
host encoder with a restart interval (lpslam_jpeg_encode_gray_restart)."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import golden
from lpslam_amd import synth

pytestmark = pytest.mark.gpu

DECODED, NOT_TAKEN, IRREGULAR = 0, 1, 2
MANY = "constant_320x240_q90_ri1"              # 1200 intervals of two bytes: every subsequence holds about 64 boundaries
LONG = "noise_320x240_q75_ri1000"              # the first interval spans more than one workgroup of subsequences
BASE = "noise_53x41_q90_ri7"                   # the damaged streams: 42 blocks, one block row an interval, 5 markers


def layout(data):
    """(restart interval or None, blocks of all components in the scan, offset of the entropy-coded data, offsets of the FF of every RSTn
    marker relative to that, offset of the marker that ends the data)"""
    data = bytes(data)
    pos, dri, blocks = 2, None, 0
    while True:
        assert data[pos] == 0xFF
        m, ln = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if m == 0xDD:
            dri = (data[pos + 4] << 8) | data[pos + 5]
        if m == 0xC0:
            h, w, nc = (data[pos + 5] << 8) | data[pos + 6], (data[pos + 7] << 8) | data[pos + 8], data[pos + 9]
            hs, vs = (data[pos + 11] >> 4, data[pos + 11] & 15) if nc == 3 else (1, 1)
            blocks = ((w + 8 * hs - 1) // (8 * hs)) * ((h + 8 * vs - 1) // (8 * vs)) * (hs * vs + nc - 1)
        pos += 2 + ln
        if m == 0xDA:
            break
    start, marks = pos, []
    while True:
        pos = data.index(b"\xff", pos)
        nxt = data[pos + 1]
        if nxt == 0:
            pos += 2
        elif 0xD0 <= nxt <= 0xD7:
            marks.append(pos - start)
            pos += 2
        else:
            return dri, blocks, start, marks, pos - start


@pytest.fixture(scope="module")
def fx():
    g = golden("g19_jpeg_restart.npz")
    g17, g18 = golden("g17_jpeg.npz"), golden("g18_jpeg_color.npz")
    jpeg = {k[5:]: g[k].tobytes() for k in g.files if k.startswith("jpeg_")}
    grey = {k[5:]: g[k] for k in g.files if k.startswith("grey_")}
    older = []
    for src, name in ((g17, "grey_restart_markers"), (g17, "colour_422_restart"), (g18, "restart_53x41_q90_420")):
        jpeg[name] = src["jpeg_" + name].tobytes(); grey[name] = src["grey_" + name]
        older.append(name)
    return dict(grey_names=[str(n) for n in g["names_grey"]], colour_names=[str(n) for n in g["names_colour"]], older=older, jpeg=jpeg, grey=grey)


@pytest.fixture(scope="module")
def host():
    from lpslam_amd import _build
    lib = C.CDLL(_build.host_library())
    enc = lib.lpslam_jpeg_encode_gray_restart
    enc.restype = C.c_size_t
    enc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    dec = lib.lpslam_jpeg_decode_gray
    dec.restype = C.c_int
    dec.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]

    def encode(img, quality, ri):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(8192 + 6 * img.size, np.uint8)
        n = enc(img.ctypes.data, img.shape[1], img.shape[0], int(quality), int(ri), out.ctypes.data, out.size)
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
    d = hiplib.JpegDecoder(1280, 720, 4, color=True, restart=True)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec_grey(hiplib):
    d = hiplib.JpegDecoder(640, 480, 2, restart=True)
    yield d
    d.close()


def test_every_fixture_stream_is_decoded_to_the_recorded_samples(dec, dec_grey, host, fx):
    assert len(fx["grey_names"]) == 10 and len(fx["colour_names"]) == 8
    for name in fx["grey_names"] + fx["colour_names"] + fx["older"]:
        data = fx["jpeg"][name]
        for d in (dec, dec_grey) if name in fx["grey_names"] else (dec,):              # a grey stream: the one-table-pair kernels too
            (status, img), = d.decode([data])
            assert status == DECODED, (name, status)
            assert img.shape == fx["grey"][name].shape and np.array_equal(img, fx["grey"][name]), name
            rounds, subs, blocks = d.last(1)[0]
            assert blocks == layout(data)[1] and subs >= 1 and 1 <= rounds <= subs + 1, (name, rounds, subs, blocks)
        assert np.array_equal(img, host["decode"](data)), name


def test_without_the_switch_the_same_streams_are_left_to_the_host(hiplib, fx):
    """off at creation, for create and create2 alike; switched on and off again on one object"""
    for color in (False, True):
        d = hiplib.JpegDecoder(640, 480, 2, color=color)
        for name in fx["grey_names"] + fx["colour_names"] + fx["older"]:
            rc, status, w, h, outs = d.decode_raw([fx["jpeg"][name]])
            assert rc == 0 and status[0] == NOT_TAKEN, (name, color, status)
            assert (h[0], w[0]) == fx["grey"][name].shape and (outs[0] == 0xA5).all(), name
        d.take_restart(True)
        (status, img), = d.decode([fx["jpeg"]["noise_53x41_q90_ri5"]])
        assert status == DECODED and np.array_equal(img, fx["grey"]["noise_53x41_q90_ri5"])
        (status, img), = d.decode([fx["jpeg"]["noise_53x41_q90_420_ri4"]])
        assert status == (DECODED if color else NOT_TAKEN)
        d.take_restart(False)
        rc, status, w, h, outs = d.decode_raw([fx["jpeg"]["noise_53x41_q90_ri5"]])
        assert rc == 0 and status[0] == NOT_TAKEN and (outs[0] == 0xA5).all()
        d.close()


def test_every_subsequence_with_a_boundary_is_final_after_the_first_round(dec, dec_grey, fx):
    """an interval start is a true entry state, so the exit state of a subsequence that holds one does not depend on what it was
    entered with: round 0 gives every true exit state (2: room for how the last subsequence is counted).  The stream: 1200 intervals
    of at most three bytes (a DC code of at most 6 + 8 bits and an EOB of 4, the predictor starts at 0 every time), so its clean
    string cannot have more than 1200 * 24 / 1024 = 29 subsequences of 1024 bits; two bytes each would give 19.  Every one of them
    holds a boundary, which is what the argument needs and what is checked here on the bytes."""
    data = fx["jpeg"][MANY]
    dri, blocks, start, marks, end = layout(data)
    assert data.count(b"\xff\x00", start, start + end) == 0
    bounds = [m - 2 * k for k, m in enumerate(marks)]                  # in the clean string: the markers in front taken off
    nsub = ((end - 2 * len(marks)) * 8 + 1023) // 1024
    assert nsub >= 19 and all(any(128 * s <= b < 128 * (s + 1) for b in bounds) for s in range(nsub))
    for d in (dec, dec_grey):
        (status, img), = d.decode([data])
        assert status == DECODED and np.array_equal(img, fx["grey"][MANY])
        rounds, subs, blocks = d.last(1)[0]
        print("rounds %d, subsequences %d" % (rounds, subs))
        assert subs == nsub and rounds <= 2 and blocks == 1200, (rounds, subs, blocks)


def test_a_first_interval_longer_than_a_workgroup(dec, dec_grey, fx):
    for d in (dec, dec_grey):
        (status, img), = d.decode([fx["jpeg"][LONG]])
        assert status == DECODED and np.array_equal(img, fx["grey"][LONG])
        rounds, subs, blocks = d.last(1)[0]
        assert subs > 256 and blocks == 1200, (rounds, subs, blocks)


def test_mixed_batches(dec, host, fx):
    plain = host["encode"](synth.StereoSequence(640, 480, 4).frame(0)[0][:200, :312], 95, 0)
    batches = [
        [fx["jpeg"]["synth_320x240_q95_rows1"], plain],                                            # a restart stream beside one without
        [fx["jpeg"]["noise_53x41_q90_ri1"], fx["jpeg"]["noise_53x41_q90_420_ri4"]],                # grey Ri = 1 beside 4:2:0 Ri = 4
        [plain, fx["jpeg"][LONG], fx["jpeg"]["synth_320x240_q95_420_rows1"], fx["jpeg"][MANY]],    # a large call ...
        [fx["jpeg"]["constant_64x48_q90_420_ri1"], fx["jpeg"]["noise_53x41_q90_ri42"]],            # ... and a small one after it
    ]
    for batch in batches:
        for data, (status, img) in zip(batch, dec.decode(batch)):
            want = host["decode"](data)
            assert status == DECODED and want is not None and np.array_equal(img, want)


def test_the_same_batch_three_times_gives_identical_bytes(dec, fx):
    batch = [fx["jpeg"][n] for n in ("noise_160x120_q100_ri1", LONG, "noise_53x41_q90_444_ri1", MANY)]
    runs = [dec.decode(batch) for _ in range(3)]
    for r in runs[1:]:
        for (s0, a), (s1, b) in zip(runs[0], r):
            assert s0 == s1 == DECODED and a.tobytes() == b.tobytes()


def _damage(case, data):
    dri, blocks, start, marks, end = layout(data)
    assert dri == 7 and len(marks) == 5
    b = bytearray(data)
    at = [start + m for m in marks]                                    # the FF of every marker
    mid = (at[1] + at[2]) // 2                                         # inside the third interval, not next to an FF
    while 0xFF in b[mid - 1:mid + 2]:
        mid += 1
    if case == "marker_deleted":
        del b[at[2]:at[2] + 2]
    elif case == "marker_duplicated_mid_interval":
        b[mid:mid] = b[at[1]:at[1] + 2]
    elif case == "header_interval_7_to_5":
        i = bytes(b).index(b"\xff\xdd\x00\x04")
        assert b[i + 5] == 7
        b[i + 5] = 5
    elif case == "markers_renumbered":
        b[at[0] + 1], b[at[1] + 1], b[at[3] + 1] = 0xD5, 0xD0, 0xD1
    elif case == "fill_byte_before_a_marker":
        b[at[2]:at[2]] = b"\xff"
    elif case == "marker_replaced_by_eoi":
        b[at[2] + 1] = 0xD9
    elif case == "cut_mid_interval":
        del b[mid:]
    elif case == "cut_in_the_last_interval":
        del b[(at[4] + 2 + start + end) // 2:]
    elif case == "byte_inverted":
        b[mid] ^= 0xFF
    else:
        raise AssertionError(case)
    return bytes(b)


@pytest.mark.parametrize("case", ["marker_deleted", "marker_duplicated_mid_interval", "header_interval_7_to_5", "markers_renumbered",
                                  "fill_byte_before_a_marker", "marker_replaced_by_eoi", "cut_mid_interval", "cut_in_the_last_interval",
                                  "byte_inverted"])
def test_a_damaged_stream_never_decodes_to_other_samples(dec, host, fx, case):
    """decoded with the host decoder's samples, or irregular (the host decoder gives the verdict): never left alone, never other samples"""
    bad = _damage(case, fx["jpeg"][BASE])
    assert bad != fx["jpeg"][BASE]
    (status, img), = dec.decode([bad])
    assert status in (DECODED, IRREGULAR), (case, status)
    if status == DECODED:
        want = host["decode"](bad)
        assert want is not None and np.array_equal(img, want), case
    # the decoder is none the worse for it
    (status, img), = dec.decode([fx["jpeg"][BASE]])
    assert status == DECODED and np.array_equal(img, fx["grey"][BASE])


def test_larger_frames_from_the_host_encoder(dec, host):
    frame = synth.StereoSequence(640, 480, 4).frame(0)[0]
    for img, ri in ((frame, 80), (frame[:200, :312], 1)):
        data = host["encode"](img, 95, ri)
        want = host["decode"](data)
        assert want is not None and want.shape == img.shape
        (status, got), = dec.decode([data])
        assert status == DECODED and np.array_equal(got, want), ri
        assert dec.last(1)[0][2] == ((img.shape[0] + 7) // 8) * ((img.shape[1] + 7) // 8)


def _manager(tmp_path, restart_device):
    from lpslam_amd import _build, manager
    _build.host_library()
    m = manager.Manager()
    k = synth.intrinsics(320, 240)
    c = manager.default_camera()
    c.camera_number = 0; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]; c.resolution_x = 320; c.resolution_y = 240
    m.set_camera(c)
    section = {"require_odometry": False}
    if restart_device is not None:
        section[manager.JPEG_DECODE_RESTART_DEVICE_KEY] = bool(restart_device)
    cfg = tmp_path / ("restart_%s.json" % restart_device)
    cfg.write_text(json.dumps({"manager": section}))
    assert m.read_configuration_file(str(cfg))
    return m


def test_restart_frames_handed_to_the_manager(hiplib, fx, tmp_path):
    from lpslam_amd import manager
    assert manager.JPEG_DECODE_RESTART_DEVICE_KEY == "jpeg_decode_restart_device"
    names = ["synth_320x240_q95_rows1", LONG, "synth_320x240_q95_420_rows1", "noise_53x41_q90_422_ri4"]
    for restart_device, want in ((True, (4, 0, 0)), (None, (0, 4, 0)), (False, (0, 4, 0))):
        m = _manager(tmp_path, restart_device)
        for i, name in enumerate(names):
            assert m.add_jpeg((i + 1) * 40_000_000, fx["jpeg"][name], ros=False)
        assert m.decoder_counters() == dict(device_images=want[0], host_images=want[1], refused_images=want[2]), restart_device


def test_the_restart_stereo_pair_is_decoded_more_than_twice_as_fast_as_on_the_host(dec, host):
    """1280 x 720 synth, quality 95, one block row an interval (Ri = 160), the two eyes in one call, streams in host memory in, samples
    in host memory out: the median of 21 wall clocks after a warm-up against the host decoder on the same two streams in the same run,
    one thread.  2: two host threads would give 2 without any device code (DESIGN.md sections 18, 23, 26).  The same pair without
    restarts goes through the same decoder for comparison; only the figures are printed for it."""
    import time
    pair_g = synth.StereoSequence(1280, 720, 4).frame(0)              # the frames of tools/time_jpeg_decode.py
    hdec = host["raw_decode"]
    res = {}
    for tag, ri in (("restart", 160), ("plain", 0)):
        pair = [np.frombuffer(host["encode"](g, 95, ri), np.uint8).copy() for g in pair_g]
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
        for _ in range(3):
            assert [hdec(s.ctypes.data, len(s), b.ctypes.data, b.size, C.byref(hw), C.byref(hh)) for s, b in zip(pair, hb)] == [0, 0]
        th = []
        for _ in range(21):
            t0 = time.perf_counter()
            rcs = [hdec(s.ctypes.data, len(s), b.ctypes.data, b.size, C.byref(hw), C.byref(hh)) for s, b in zip(pair, hb)]
            th.append(time.perf_counter() - t0)
            assert rcs == [0, 0]
        assert all(np.array_equal(o, b) for o, b in zip(outs, hb))
        res[tag] = (float(np.median(td)) * 1e3, float(np.median(th)) * 1e3, dec.last(2))
        print("%s: device pair %.3f ms, host pair %.3f ms, ratio %.1f, (rounds, subsequences, blocks) %s" % (
            tag, res[tag][0], res[tag][1], res[tag][1] / res[tag][0], res[tag][2]))
    device_ms, host_ms, _ = res["restart"]
    assert host_ms > 2.0 * device_ms, (device_ms, host_ms)
