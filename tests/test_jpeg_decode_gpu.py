"""The device JPEG decoder (lpslam_hip_jpeg_dec_*, lpslam_amd/csrc/jpeg_dec.hip) against the host decoder LpSlam::decode_jpeg_gray
(lpslam_jpeg_decode_gray), which gives libjpeg's samples (tests/test_jpeg_cpu.py): equal width, equal height and equal samples, with
status "decoded", for every input of the class the device has to take."""
import ctypes as C
import io

import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

DECODED, NOT_TAKEN, IRREGULAR = 0, 1, 2


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
        out = np.zeros(1 << 22, np.uint8); w, h = C.c_int(0), C.c_int(0)
        rc = dec(d.ctypes.data, len(d), out.ctypes.data, out.size, C.byref(w), C.byref(h))
        assert rc in (0, 2)
        return out[:w.value * h.value].reshape(h.value, w.value).copy() if rc == 0 else None
    return dict(encode=encode, decode=decode, raw_decode=dec)


@pytest.fixture(scope="module")
def dec(hiplib):
    d = hiplib.JpegDecoder(1920, 1080, 4)
    yield d
    d.close()


def _check(dec, host, data):
    """one stream through the device decoder: decoded, and the host decoder's image"""
    (status, img), = dec.decode([data])
    want = host["decode"](data)
    assert want is not None
    assert status == DECODED, status
    assert img.shape == want.shape and np.array_equal(img, want), (img.shape, want.shape)
    return img


def _synth(w, h):
    return synth.StereoSequence(w, h, 4, n_points=max(2000, w * h // 150)).frame(0)


@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720), (1920, 1080)])
def test_synth_frames_equal_the_host_decoder(dec, host, w, h):
    for img in _synth(w, h):
        _check(dec, host, host["encode"](img, 95))


def test_sizes(dec, host):
    frame = _synth(1920, 1080)[0]
    for w, h in [(1, 1), (7, 9), (8, 8), (17, 33), (1279, 719)]:
        img = _check(dec, host, host["encode"](np.ascontiguousarray(frame[:h, :w]), 95))
        assert img.shape == (h, w)


def test_qualities_1_50_70_100(dec, host):
    img = _synth(640, 480)[0]
    for quality in (1, 50, 70, 100):
        _check(dec, host, host["encode"](img, quality))


def test_uniform_noise_at_quality_100(dec, host):
    """16-bit codes and dense FF 00 stuffing"""
    noise = np.random.default_rng(7).integers(0, 256, (480, 640), dtype=np.uint8)
    data = host["encode"](noise, 100)
    assert data.count(b"\xff\x00") > 1000
    _check(dec, host, data)


def test_constant_and_periodic_images_need_the_hand_over(dec, host):
    """a constant image's stream is periodic (one short code pair per block): a subsequence started in the wrong phase stays there until
    the true state reaches it, so more than one round has to run -- the hand-over between rounds is exercised"""
    imgs = [np.full((480, 640), v, np.uint8) for v in (0, 128, 255)]
    two = np.zeros((480, 640), np.uint8)
    for x in range(8, 640, 16):
        two[:, x:x + 8] = 255                                          # two constant blocks that alternate: a stream of period two blocks
    imgs.append(two)
    for img in imgs:
        _check(dec, host, host["encode"](img, 95))
        rounds, subs, blocks = dec.last(1)[0]
        assert blocks == 80 * 60 and subs > 1
        assert rounds > 1, (rounds, subs)
        assert rounds <= subs + 1


def test_impulses_zrl_runs_and_coefficient_63(dec, host):
    rng = np.random.default_rng(11)
    imgs = []
    img = np.full((64, 64), 128, np.uint8)
    img[::8, ::8] = 255                                                # one impulse per block: every coefficient non-zero
    imgs.append(img)
    img = np.full((64, 64), 128, np.uint8)
    img[7::8, 7::8] = 131                                              # small impulse: long zero runs between the survivors
    imgs.append(img)
    img = np.full((64, 64), 100, np.uint8)
    blk = np.indices((8, 8)).sum(0) % 2 == 0
    img[:8, :8] = np.where(blk, 108, 92)                               # checker inside a block: coefficient 63 dominates
    imgs.append(img)
    for _ in range(4):                                                 # sparse random impulses
        img = np.full((72, 88), 128, np.uint8)
        ys, xs = rng.integers(0, 72, 20), rng.integers(0, 88, 20)
        img[ys, xs] = rng.integers(0, 256, 20)
        imgs.append(img)
    for img in imgs:
        for quality in (30, 95, 100):
            _check(dec, host, host["encode"](img, quality))


def _pillow(img, **kw):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue(), Image


def test_pillow_streams_with_their_own_huffman_tables(dec, host):
    img = _synth(640, 480)[0]
    for kw in (dict(quality=75), dict(quality=75, optimize=True)):
        data, Image = _pillow(img, **kw)
        ours = _check(dec, host, data)
        assert np.array_equal(ours, np.asarray(Image.open(io.BytesIO(data))))


def test_batches(dec, host):
    left, right = _synth(1280, 720)
    pair = [host["encode"](left, 95), host["encode"](right, 95)]
    both = dec.decode(pair)
    for data, (status, img) in zip(pair, both):
        assert status == DECODED and np.array_equal(img, _check(dec, host, data))
    rng = np.random.default_rng(5)
    frame = _synth(1920, 1080)[0]
    mixed = [np.ascontiguousarray(frame[:720, :1280]), rng.integers(0, 256, (37, 53), dtype=np.uint8),
             np.ascontiguousarray(frame[100:1080, 300:1920]), np.full((8, 8), 17, np.uint8)]
    res = dec.decode([host["encode"](m, 95) for m in mixed])
    for m, (status, img) in zip(mixed, res):
        assert status == DECODED and np.array_equal(img, host["decode"](host["encode"](m, 95)))
    # a smaller call after a larger one: nothing of the first is left
    small = [np.ascontiguousarray(right[:99, :201]), np.full((16, 24), 200, np.uint8)]
    res = dec.decode([host["encode"](m, 95) for m in small])
    for m, (status, img) in zip(small, res):
        assert status == DECODED and np.array_equal(img, host["decode"](host["encode"](m, 95)))


def test_status_not_taken_and_irregular(dec, host):
    rgb = np.dstack([_synth(640, 480)[0]] * 3)
    data, _ = _pillow(rgb, quality=90)
    rc, status, w, h, outs = dec.decode_raw([data])
    assert rc == 0 and status[0] == NOT_TAKEN and (w[0], h[0]) == (640, 480) and (outs[0] == 0xA5).all()


def test_a_cut_stream_is_irregular(dec, host):
    data = host["encode"](_synth(640, 480)[0], 95)
    cut = data[:len(data) // 2]
    rc, status, w, h, outs = dec.decode_raw([cut])
    assert rc == 0 and status[0] == IRREGULAR and (w[0], h[0]) == (640, 480) and (outs[0] == 0xA5).all()


def test_a_flipped_byte_never_decodes_to_other_samples(dec, host):
    """one fixed byte in the middle of the entropy-coded data inverted, once: decoded with the host decoder's samples, or irregular"""
    data = bytearray(host["encode"](_synth(640, 480)[0], 95))
    data[len(data) // 2] ^= 0xFF
    (status, img), = dec.decode([bytes(data)])
    assert status in (DECODED, IRREGULAR)
    if status == DECODED:
        want = host["decode"](bytes(data))
        assert want is not None and np.array_equal(img, want)


def test_too_small_capacity_writes_nothing(dec, host):
    left, right = _synth(640, 480)
    pair = [host["encode"](left, 95), host["encode"](right, 95)]
    rc, status, w, h, outs = dec.decode_raw(pair, caps=[640 * 480, 640 * 480 - 1], strides=[640, 640])
    assert rc == 1                                                     # LPSLAM_HIP_ERR_INVALID
    assert list(w) == [640, 640] and list(h) == [480, 480]
    assert all((o == 0xA5).all() for o in outs)                        # untouched
    rc, status, w, h, outs = dec.decode_raw(pair, caps=[640 * 480, 640 * 480], strides=[640, 640])
    assert rc == 0 and list(status) == [DECODED, DECODED]
    assert np.array_equal(outs[0].reshape(480, 640), host["decode"](pair[0])) and np.array_equal(outs[1].reshape(480, 640), host["decode"](pair[1]))
    rc, status, w, h, outs = dec.decode_raw(pair[:1], caps=[1000 * 480], strides=[1000])       # a row stride larger than the width
    assert rc == 0 and np.array_equal(outs[0].reshape(480, 1000)[:, :640], host["decode"](pair[0])) and (outs[0].reshape(480, 1000)[:, 640:] == 0xA5).all()


def test_bad_arguments_are_refused(hiplib, host):
    d = hiplib.JpegDecoder(64, 48, 2)
    data = host["encode"](np.zeros((48, 64), np.uint8), 95)
    assert d.decode_raw([data, data, data])[0] == 1                    # n > max_images
    assert d.decode_raw([])[0] == 1
    assert d.decode_raw([data], strides=[63])[0] == 1                  # a stride below the width
    assert d.lib.lpslam_hip_jpeg_decode(d.h, 1, None, None, None, None, None, None, None, None) == 1
    rc, status, w, h, _ = d.decode_raw([host["encode"](np.zeros((49, 64), np.uint8), 95)])      # taller than the maximum: left to the host
    assert rc == 0 and status[0] == NOT_TAKEN and (w[0], h[0]) == (64, 49)
    rc, status, _, _, _ = d.decode_raw([data])
    assert rc == 0 and status[0] == DECODED                            # and the decoder still works
    d.close()
    with pytest.raises(hiplib.LpslamHipError):
        hiplib.JpegDecoder(0, 48, 1)


def test_the_same_batch_three_times_gives_identical_bytes(dec, host):
    left, right = _synth(1280, 720)
    pair = [host["encode"](left, 95), host["encode"](right, 95)]
    runs = [dec.decode(pair) for _ in range(3)]
    for r in runs[1:]:
        for (s0, a), (s1, b) in zip(runs[0], r):
            assert s0 == s1 == DECODED and a.tobytes() == b.tobytes()


def test_the_stereo_pair_is_decoded_five_times_faster_than_on_the_host(dec, host):
    """1280 x 720 synth, quality 95, the two eyes in one call, streams in host memory in, samples in host memory out: the median of 21
    wall clocks after a warm-up against the host decoder on the same two streams in the same run, one thread.  5: two host threads would
    give 2 without any device code, and the spread between runs is about 3 %."""
    import time
    left, right = synth.StereoSequence(1280, 720, 4).frame(0)         # the frames of tools/time_jpeg_decode.py and of DESIGN section 18
    pair = [np.frombuffer(host["encode"](im, 95), np.uint8).copy() for im in (left, right)]
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
    assert host_ms >= 5.0 * device_ms, (device_ms, host_ms)
