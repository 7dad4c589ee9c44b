"""Restart intervals on the host side: the fixture of the device decoder's restart path (tests/golden/g19_jpeg_restart.npz,
tools/make_jpeg_restart_fixture.py: streams written by Pillow = libjpeg-turbo with restart_marker_blocks / restart_marker_rows, grey
samples by libjpeg's draft("L")) holds what the device tests rely on; the host decoder (lpslam_amd/host/jpeg.cpp), which defines what
the device has to give, decodes every stream to libjpeg's samples bit for bit; the host encoder with a restart interval
(lpslam_jpeg_encode_gray_restart) writes what libjpeg writes; and the classification the device decoder and the host layer share
(host/jpeg_header.h) lets a restart interval through only when it is allowed."""
import ctypes as C
import io

import numpy as np
import pytest

from conftest import golden
from lpslam_amd import synth

PIECE = 256


def layout(data):
    """(restart interval of the DRI segment or None, MCUs of the frame, offset of the entropy-coded data, offsets of the FF of every
    RSTn marker relative to that, offset of the marker that ends the data)"""
    data = bytes(data)
    pos, dri, mcus = 2, None, 0
    while True:
        assert data[pos] == 0xFF
        m, ln = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if m == 0xDD:
            dri = (data[pos + 4] << 8) | data[pos + 5]
        if m == 0xC0:
            h, w, nc = (data[pos + 5] << 8) | data[pos + 6], (data[pos + 7] << 8) | data[pos + 8], data[pos + 9]
            hs, vs = (data[pos + 11] >> 4, data[pos + 11] & 15) if nc == 3 else (1, 1)
            mcus = ((w + 8 * hs - 1) // (8 * hs)) * ((h + 8 * vs - 1) // (8 * vs))
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
            return dri, mcus, start, marks, pos - start


@pytest.fixture(scope="module")
def fx():
    g = golden("g19_jpeg_restart.npz")
    names = [str(n) for n in g["names_grey"]] + [str(n) for n in g["names_colour"]]
    return dict(grey_names=[str(n) for n in g["names_grey"]], colour_names=[str(n) for n in g["names_colour"]], names=names,
                dri=dict(zip(names, (int(v) for v in g["dri"]))), markers=dict(zip(names, (int(v) for v in g["markers"]))),
                piece_edge=str(g["piece_edge"]),
                jpeg={k[5:]: g[k].tobytes() for k in g.files if k.startswith("jpeg_")},
                grey={k[5:]: g[k] for k in g.files if k.startswith("grey_")})


@pytest.fixture(scope="module")
def lib():
    from lpslam_amd import _build
    l = C.CDLL(_build.host_library())
    l.lpslam_jpeg_decode_gray.restype = C.c_int
    l.lpslam_jpeg_decode_gray.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    l.lpslam_jpeg_encode_gray.restype = C.c_size_t
    l.lpslam_jpeg_encode_gray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    l.lpslam_jpeg_encode_gray_restart.restype = C.c_size_t
    l.lpslam_jpeg_encode_gray_restart.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    l.lpslam_jpeg_device_class.restype = C.c_int
    l.lpslam_jpeg_device_class.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    return l


def decode(lib, data):
    d = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.zeros(1 << 20, np.uint8); w, h = C.c_int(0), C.c_int(0)
    rc = lib.lpslam_jpeg_decode_gray(d.ctypes.data, len(d), out.ctypes.data, out.size, C.byref(w), C.byref(h))
    return out[:w.value * h.value].reshape(h.value, w.value).copy() if rc == 0 else None


def encode(lib, img, quality, ri=None):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(8192 + 6 * img.size, np.uint8)
    if ri is None:
        n = lib.lpslam_jpeg_encode_gray(img.ctypes.data, img.shape[1], img.shape[0], quality, out.ctypes.data, out.size)
    else:
        n = lib.lpslam_jpeg_encode_gray_restart(img.ctypes.data, img.shape[1], img.shape[0], quality, ri, out.ctypes.data, out.size)
    assert n > 0
    return out[:n].tobytes()


def device_class(lib, data, color, restart):
    d = np.frombuffer(bytes(data), np.uint8).copy()
    return lib.lpslam_jpeg_device_class(d.ctypes.data, len(d), int(color), int(restart))


def test_the_fixture_holds_what_the_device_tests_need(fx):
    assert fx["grey_names"] == ["noise_53x41_q90_ri%d" % r for r in (1, 5, 7, 42, 100)] + [
        "constant_320x240_q90_ri1", "noise_160x120_q100_ri1", "noise_320x240_q75_ri1000", "synth_320x240_q95_rows1", "noise_96x64_q95_optimised_ri3"]
    assert fx["colour_names"] == ["noise_53x41_q90_%s_ri%d" % (s, r) for s in ("444", "422", "420") for r in (1, 4)] + [
        "constant_64x48_q90_420_ri1", "synth_320x240_q95_420_rows1"]
    want_dri = {"noise_53x41_q90_ri1": 1, "noise_53x41_q90_ri5": 5, "noise_53x41_q90_ri7": 7, "noise_53x41_q90_ri42": 42, "noise_53x41_q90_ri100": 100,
                "constant_320x240_q90_ri1": 1, "noise_160x120_q100_ri1": 1, "noise_320x240_q75_ri1000": 1000, "synth_320x240_q95_rows1": 40,
                "noise_96x64_q95_optimised_ri3": 3, "constant_64x48_q90_420_ri1": 1, "synth_320x240_q95_420_rows1": 20}
    for name in fx["names"]:
        dri, mcus, start, marks, end = layout(fx["jpeg"][name])
        assert dri == fx["dri"][name] and dri > 0, name                                   # every stream has a DRI segment
        if name in want_dri:
            assert dri == want_dri[name], name
        else:
            assert dri == int(name.rsplit("ri", 1)[1]), name
        want = (mcus + dri - 1) // dri - 1 if dri < mcus else 0
        assert len(marks) == fx["markers"][name] == want, (name, len(marks), want)
        data = fx["jpeg"][name]
        assert [data[start + m + 1] for m in marks] == [0xD0 + (k & 7) for k in range(len(marks))], name      # numbered in turn
        assert fx["grey"][name].dtype == np.uint8 and fx["grey"][name].ndim == 2
    assert fx["markers"]["noise_53x41_q90_ri1"] == 41 and fx["markers"]["noise_53x41_q90_ri5"] == 8 and fx["markers"]["noise_53x41_q90_ri7"] == 5
    assert fx["markers"]["noise_53x41_q90_ri42"] == 0 and fx["markers"]["noise_53x41_q90_ri100"] == 0       # DRI present, no marker
    # intervals of two bytes: many boundaries in every subsequence of 1024 bits, and more than 30 subsequences
    dri, mcus, start, marks, end = layout(fx["jpeg"]["constant_320x240_q90_ri1"])
    assert len(marks) == 1199 and end * 8 > 30 * 1024
    gaps = np.diff([-2] + marks + [end]) - 2
    assert gaps.max() <= 3 and gaps.min() >= 2, (gaps.min(), gaps.max())
    # a marker whose FF is the last byte of a 256-byte piece of the data, and one directly behind a stuffed FF 00
    data = fx["jpeg"][fx["piece_edge"]]
    dri, mcus, start, marks, end = layout(data)
    assert any(m % PIECE == PIECE - 1 for m in marks)
    assert any(m >= 2 and data[start + m - 2] == 0xFF and data[start + m - 1] == 0 for m in marks)
    # a first interval longer than a workgroup of subsequences (256 x 1024 bits of clean data: stuffed zeros taken off)
    data = fx["jpeg"]["noise_320x240_q75_ri1000"]
    dri, mcus, start, marks, end = layout(data)
    clean = marks[0] - data[start:start + marks[0]].count(b"\xff\x00")
    assert len(marks) == 1 and clean * 8 > 256 * 1024


def test_the_host_decoder_gives_libjpegs_samples_for_every_stream(lib, fx):
    for name in fx["names"]:
        img = decode(lib, fx["jpeg"][name])
        assert img is not None, name
        assert img.shape == fx["grey"][name].shape and np.array_equal(img, fx["grey"][name]), name


def test_pillow_agrees_when_present(lib, fx):
    Image = pytest.importorskip("PIL.Image")
    for name in ("noise_160x120_q100_ri1", "noise_53x41_q90_420_ri4"):
        im = Image.open(io.BytesIO(fx["jpeg"][name])); im.draft("L", im.size); im.load()
        assert np.array_equal(np.asarray(im), fx["grey"][name])


def _encoder_cases():
    frame = synth.StereoSequence(640, 480, 4).frame(0)[0]
    return [("synth_201x99", np.ascontiguousarray(frame[3:102, 5:206]), 95), ("noise_64x48", np.random.default_rng(5).integers(0, 256, (48, 64), dtype=np.uint8), 100)]


def test_restart_interval_zero_gives_the_bytes_of_the_plain_encoder(lib):
    for _, img, quality in _encoder_cases():
        assert encode(lib, img, quality, 0) == encode(lib, img, quality)


def test_the_restart_encoder_changes_no_sample(lib):
    for tag, img, quality in _encoder_cases():
        bw, bh = (img.shape[1] + 7) // 8, (img.shape[0] + 7) // 8
        plain = encode(lib, img, quality, 0)
        want = decode(lib, plain)
        assert want is not None and want.shape == img.shape
        for ri in (1, 7, bw, bw * bh, bw * bh + 5):
            data = encode(lib, img, quality, ri)
            dri, mcus, start, marks, end = layout(data)
            assert dri == ri and mcus == bw * bh
            assert len(marks) == ((mcus + ri - 1) // ri - 1 if ri < mcus else 0), (tag, ri)
            assert [data[start + m + 1] for m in marks] == [0xD0 + (k & 7) for k in range(len(marks))]
            got = decode(lib, data)
            assert got is not None and np.array_equal(got, want), (tag, ri)
            if ri >= mcus:                                                             # no marker: the plain stream plus the DRI segment
                assert len(data) == len(plain) + 6


def test_the_restart_encoder_writes_what_libjpeg_writes(lib):
    Image = pytest.importorskip("PIL.Image")
    for tag, img, quality in _encoder_cases():
        bw, bh = (img.shape[1] + 7) // 8, (img.shape[0] + 7) // 8
        for ri in (1, 7, bw, bw * bh):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=quality, restart_marker_blocks=ri)
            theirs = buf.getvalue()
            ours = encode(lib, img, quality, ri)
            assert ours == theirs, (tag, ri, len(ours), len(theirs))
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours))), decode(lib, ours)), (tag, ri)


def test_a_restart_interval_is_of_the_devices_class_only_when_allowed(lib, fx):
    g17 = golden("g17_jpeg.npz")
    for name in fx["grey_names"]:
        data = fx["jpeg"][name]
        assert device_class(lib, data, False, False) == 0 and device_class(lib, data, True, False) == 0, name
        assert device_class(lib, data, False, True) == 1 and device_class(lib, data, True, True) == 1, name
    for name in fx["colour_names"]:
        data = fx["jpeg"][name]
        assert device_class(lib, data, True, False) == 0 and device_class(lib, data, False, False) == 0, name
        assert device_class(lib, data, True, True) == 1, name
        assert device_class(lib, data, False, True) == 0, name                            # three components need a decoder made for colour
    # without a restart interval the argument changes nothing
    plain = encode(lib, np.full((16, 16), 90, np.uint8), 90)
    assert [device_class(lib, plain, c, r) for c in (0, 1) for r in (0, 1)] == [1, 1, 1, 1]
    # a non-interleaved file (one scan per component) is never of the class, restart interval or not
    for k in g17.files:
        if not k.startswith("jpeg_"):
            continue
        data = g17[k].tobytes()
        if _scan_components(data) == 1 and _frame_components(data) == 3:
            assert [device_class(lib, data, c, r) for c in (0, 1) for r in (0, 1)] == [0, 0, 0, 0], k
    non = _non_interleaved(fx["jpeg"]["noise_53x41_q90_444_ri4"])
    assert _scan_components(non) == 1 and _frame_components(non) == 3
    assert [device_class(lib, non, c, r) for c in (0, 1) for r in (0, 1)] == [0, 0, 0, 0]
    assert device_class(lib, b"\xff\xd8\xff\xd9", 1, 1) == -1


def _segments(data):
    out, pos = [], 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        m, ln = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        out.append((m, pos, pos + 2 + ln))
        if m == 0xDA:
            break
        pos += 2 + ln
    return out


def _frame_components(data):
    sof = [s for s in _segments(data) if s[0] == 0xC0][0]
    return data[sof[1] + 9]


def _scan_components(data):
    sos = [s for s in _segments(data) if s[0] == 0xDA][0]
    return data[sos[1] + 4]


def _non_interleaved(data):
    """the header of a three-component stream with its scan header rewritten to name the first component alone (the entropy-coded data
    no longer fits it; the classification reads the headers only)"""
    sos = [s for s in _segments(data) if s[0] == 0xDA][0]
    head = data[:sos[1]]
    first = data[sos[1] + 5:sos[1] + 7]
    return head + b"\xff\xda\x00\x08\x01" + first + b"\x00\x3f\x00" + data[sos[2]:]
