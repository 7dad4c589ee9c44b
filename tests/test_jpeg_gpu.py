"""The device JPEG encoder (lpslam_hip_jpeg_*, lpslam_amd/csrc/jpeg.hip) against the host encoder LpSlam::encode_jpeg_gray
(lpslam_jpeg_encode_gray), which writes libjpeg's stream (tests/test_jpeg_cpu.py): byte for byte, for every case."""
import ctypes as C
import io

import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from lpslam_amd import _build
    lib = C.CDLL(_build.host_library())
    f = lib.lpslam_jpeg_encode_gray
    f.restype = C.c_size_t
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]

    def encode(img, quality):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(4096 + 4 * img.size, np.uint8)
        n = f(img.ctypes.data, img.shape[1], img.shape[0], int(quality), out.ctypes.data, out.size)
        assert n > 0
        return out[:n].tobytes()
    return encode


@pytest.fixture(scope="module")
def enc(hiplib):
    e = hiplib.JpegEncoder(1920, 1080, 4)
    yield e
    e.close()


def _pillow(img, quality):
    try:
        from PIL import Image
    except ImportError:
        return None
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def _check(enc, host, img, quality, pillow=False):
    ours = enc.encode([img], quality)[0]
    want = host(img, quality)
    assert len(ours) == len(want) and ours == want, (img.shape, quality, len(ours), len(want))
    if pillow:
        theirs = _pillow(np.ascontiguousarray(img), quality)
        if theirs is not None:
            assert ours == theirs, (img.shape, quality)
    return ours


def _synth(w, h):
    return synth.StereoSequence(w, h, 4, n_points=max(2000, w * h // 150)).frame(0)


@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720), (1920, 1080)])
def test_synth_frames_equal_the_host_encoder(enc, host, w, h):
    left, right = _synth(w, h)
    for quality in (70, 95):
        _check(enc, host, left, quality, pillow=True)
        _check(enc, host, right, quality)


def test_sizes_that_are_not_multiples_of_8(enc, host):
    frame = _synth(1920, 1080)[0]
    for h, w in [(1, 1), (9, 7), (99, 201), (721, 1281)]:
        for quality in (70, 95):
            _check(enc, host, np.ascontiguousarray(frame[:h, :w]), quality, pillow=True)
    _check(enc, host, frame[13:13 + 99, 5:5 + 201], 95)            # a row stride larger than the width


def test_qualities_1_50_100(enc, host):
    img = _synth(640, 480)[0]
    for quality in (1, 50, 100):
        _check(enc, host, img, quality, pillow=True)


def test_uniform_noise_at_quality_100(enc, host):
    """many 0xFF bytes to stuff, DC differences of category 11 and AC coefficients of category 10"""
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (480, 640), dtype=np.uint8)
    data = _check(enc, host, noise, 100, pillow=True)
    assert data.count(b"\xff\x00") > 1000
    checker = np.where((np.indices((64, 64)).sum(0) // 8) % 2 == 0, 0, 255).astype(np.uint8)      # blocks of 0 beside blocks of 255
    _check(enc, host, checker, 100, pillow=True)
    stripes = np.tile(np.array([0, 255], np.uint8), (64, 32))                                      # the highest horizontal frequency
    _check(enc, host, stripes, 100, pillow=True)


def test_constant_images(enc, host):
    for v in (0, 128, 255):
        for quality in (50, 95):
            _check(enc, host, np.full((48, 80), v, np.uint8), quality, pillow=True)


def test_impulses_force_zrl_runs_and_coefficient_63(enc, host):
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
            _check(enc, host, img, quality, pillow=True)


def test_mixed_batch_equals_single_calls(enc, host):
    frame = _synth(1920, 1080)[0]
    rng = np.random.default_rng(5)
    batch = [np.ascontiguousarray(frame[:720, :1280]), rng.integers(0, 256, (37, 53), dtype=np.uint8),
             frame[100:1080, 300:1920], np.full((8, 8), 17, np.uint8)]
    together = enc.encode(batch, 95)
    for img, data in zip(batch, together):
        assert data == enc.encode([img], 95)[0] == host(img, 95)


def test_too_small_capacity_writes_nothing(enc, host):
    left, right = _synth(640, 480)
    want = [host(left, 95), host(right, 95)]
    rc, sizes, outs = enc.encode_raw([left, right], 95, caps=[len(want[0]) + 10, len(want[1]) - 1])
    assert rc == 1                                                     # LPSLAM_HIP_ERR_INVALID
    assert list(sizes) == [len(want[0]), len(want[1])]
    assert all((o == 0xA5).all() for o in outs)                        # untouched
    rc, sizes, outs = enc.encode_raw([left, right], 95, caps=[len(want[0]), len(want[1])])
    assert rc == 0 and [o[:s].tobytes() for o, s in zip(outs, sizes)] == want


def test_bad_arguments_are_refused(hiplib):
    e = hiplib.JpegEncoder(64, 48, 2)
    img = np.zeros((48, 64), np.uint8)
    assert e.encode_raw([img, img, img], 95)[0] == 1                   # n > max_images
    assert e.encode_raw([np.zeros((49, 64), np.uint8)], 95)[0] == 1    # taller than the encoder's maximum
    assert e.encode_raw([np.zeros((48, 65), np.uint8)], 95)[0] == 1    # wider
    assert e.encode_raw([img], 0)[0] == 1 and e.encode_raw([img], 101)[0] == 1
    assert e.encode_raw([], 95)[0] == 1
    assert e.encode_raw([img], 95)[0] == 0                             # and the encoder still works
    e.close()
    with pytest.raises(hiplib.LpslamHipError):
        hiplib.JpegEncoder(0, 48, 1)
