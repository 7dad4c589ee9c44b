"""Colour and YUV frames at ingest, without a GPU: the host implementation of the grey conversion (lpslam_amd/host/ingest.cpp) against the
numpy restatement in tests/ingest_ref.py -- every (R, G, B) triple in both byte orders, every (Y, U, V) triple as NV12 and as UYVY, the
values worked by hand -- the manager's ingest of the two YUV layouts (frames only enqueued, never started), and realiseGray +
realiseAdjust against what the manager's earlier scalar conversion followed by the adjustment gave.  Every comparison is exact."""
import numpy as np
import pytest

import ingest_ref as ref
import intensity_ref as ir


@pytest.fixture(scope="module")
def mgrlib(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    manager.load()
    return manager


def host_grey(mgr, buf, fmt, w, h, **kw):
    return mgr.gray_from_pixels(buf, w, h, fmt, **kw)


# ---- every triple -----------------------------------------------------------------------------------------------------------------
def test_every_rgb_triple_in_both_byte_orders(mgrlib):
    for k in range(64):
        img = ref.rgb_sweep(k)
        for fmt in (ref.RGB8, ref.BGR8):
            assert np.array_equal(host_grey(mgrlib, img, fmt, 512, 512), ref.grey(img, fmt)), (k, fmt)
    # the two orders differ, and the sweep reaches every value of every channel
    img = ref.rgb_sweep(17)
    assert not np.array_equal(ref.grey(img, ref.RGB8), ref.grey(img, ref.BGR8))
    assert ref.rgb_sweep(0)[..., 0].min() == 0 and ref.rgb_sweep(63)[..., 0].max() == 255
    assert len(np.unique(img[..., 1].astype(np.int32) * 256 + img[..., 2])) == 65536


def test_every_yuv_triple_as_nv12(mgrlib):
    for k in range(64):
        buf = ref.nv12_sweep(k)
        assert np.array_equal(host_grey(mgrlib, buf, ref.NV12, 512, 512), ref.grey_nv12(buf)), k
    buf = ref.nv12_sweep(63)
    uv = buf[512:].reshape(256, 256, 2).astype(np.int32)
    assert len(np.unique(uv[..., 0] * 256 + uv[..., 1])) == 65536 and sorted(np.unique(buf[:512])) == [252, 253, 254, 255]


def test_every_yuv_triple_as_uyvy(mgrlib):
    for k in range(128):
        buf = ref.uyvy_sweep(k)
        assert np.array_equal(host_grey(mgrlib, buf, ref.UYVY, 512, 256), ref.grey_uyvy(buf)), k
    q = ref.uyvy_sweep(127).reshape(256, 256, 4).astype(np.int32)
    assert len(np.unique(q[..., 0] * 256 + q[..., 2])) == 65536 and sorted(np.unique(q[..., [1, 3]])) == [254, 255]


def test_the_worked_values_of_the_definition(mgrlib):
    for (y, u, v), want in ref.WORKED_YUV.items():
        assert int(ref.grey_of_yuv(y, u, v)) == want, (y, u, v)
        nv12 = np.array([[y, y], [y, y], [u, v]], np.uint8)
        assert np.all(host_grey(mgrlib, nv12, ref.NV12, 2, 2) == want), (y, u, v)
        uyvy = np.array([[u, y, v, y]], np.uint8)
        assert np.all(host_grey(mgrlib, uyvy, ref.UYVY, 2, 1) == want), (y, u, v)
    # RGB: white, black, the three primaries ((255 * weight + 8192) >> 14) and the byte order
    for rgb, want in (((255, 255, 255), 255), ((0, 0, 0), 0), ((255, 0, 0), 76), ((0, 255, 0), 150), ((0, 0, 255), 29)):
        px = np.array([[rgb]], np.uint8)
        assert int(host_grey(mgrlib, px, ref.RGB8, 1, 1)[0, 0]) == want == int(ref.grey_rgb(px)[0, 0])
        assert int(host_grey(mgrlib, px[..., ::-1].copy(), ref.BGR8, 1, 1)[0, 0]) == want


# ---- shapes, strides, errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,w,h", [(ref.RGB8, 65, 64), (ref.BGR8, 333, 77), (ref.RGB8, 1, 1), (ref.NV12, 66, 64), (ref.NV12, 322, 64), (ref.NV12, 2, 2),
                                      (ref.UYVY, 66, 64), (ref.UYVY, 322, 63), (ref.UYVY, 2, 1), (ref.GRAY8, 65, 3)])
def test_odd_and_minimal_shapes_strides_and_output_padding(mgrlib, fmt, w, h):
    buf = ref.random_frame(fmt, w, h, 7)
    want = ref.grey(buf, fmt)
    pad = []
    assert np.array_equal(host_grey(mgrlib, buf, fmt, w, h, padding=pad, out_stride=w + 5), want)
    assert np.all(pad[0] == 0xA5)                                                # the bytes between the output rows are not written
    # a source stride larger than the row: the frame as a view of a wider buffer
    rows = buf.reshape(buf.shape[0], -1)
    wide = np.full((rows.shape[0], rows.shape[1] + 11), 0x5A, np.uint8)
    wide[:, :rows.shape[1]] = rows
    assert np.array_equal(host_grey(mgrlib, wide, fmt, w, h, stride=wide.shape[1]), want)
    if fmt == ref.NV12:      # chroma rows of their own, with a stride of their own
        chroma = np.full((h // 2, w + 3), 0x5A, np.uint8)
        chroma[:, :w] = buf[h:]
        assert np.array_equal(host_grey(mgrlib, wide[:h], fmt, w, h, stride=wide.shape[1], chroma=chroma, chroma_stride=w + 3), want)


def test_host_conversion_refuses_what_the_definition_excludes(mgrlib):
    z = np.zeros(4096, np.uint8)
    assert host_grey(mgrlib, z, 5, 8, 8) is None                                 # unknown format
    assert host_grey(mgrlib, z, -1, 8, 8) is None
    assert host_grey(mgrlib, z, ref.NV12, 7, 8) is None and host_grey(mgrlib, z, ref.NV12, 8, 7) is None
    assert host_grey(mgrlib, z, ref.UYVY, 7, 8) is None
    assert host_grey(mgrlib, z, ref.UYVY, 8, 7) is not None                      # UYVY needs an even width only
    assert host_grey(mgrlib, z, ref.RGB8, 8, 8, stride=23) is None               # a stride smaller than a row
    assert host_grey(mgrlib, z, ref.UYVY, 8, 8, stride=15) is None
    assert host_grey(mgrlib, z, ref.NV12, 8, 8, stride=7) is None
    assert host_grey(mgrlib, z, ref.NV12, 8, 8, stride=8, chroma=z, chroma_stride=7) is None
    assert host_grey(mgrlib, z, ref.RGB8, 0, 8) is None


# ---- the manager's ingest, no GPU: frames are enqueued and never started -----------------------------------------------------------
def _stereo_yuv(fmt, w, h, seed=3):
    """a LeftTop_RightBottom buffer of two complete w x h pictures; returns (buffer, desc.height)"""
    a, b = ref.random_frame(fmt, w, h, seed), ref.random_frame(fmt, w, h, seed + 1)
    return np.concatenate([a.reshape(-1), b.reshape(-1)]), 2 * h


def test_manager_accepts_nv12_and_yuv16_left_top_right_bottom(mgrlib):
    m = mgrlib.Manager(log_level=4)
    try:
        for w, h in ((64, 64), (322, 64), (66, 2)):
            buf, H = _stereo_yuv(ref.NV12, w, h)
            assert buf.size == w * H * 3 // 2
            assert m.add_buffer(1, buf, w, H, mgrlib.FORMAT_NV12, mgrlib.STEREO_LEFT_TOP_RIGHT_BOTTOM)
        for w, h in ((64, 64), (322, 63), (2, 1)):
            buf, H = _stereo_yuv(ref.UYVY, w, h)
            assert buf.size == 2 * w * H
            assert m.add_buffer(2, buf, w, H, mgrlib.FORMAT_YUV16, mgrlib.STEREO_LEFT_TOP_RIGHT_BOTTOM)
    finally:
        m.close()


def test_manager_refuses_malformed_yuv_frames(mgrlib):
    m = mgrlib.Manager(log_level=4)
    NV12, YUV16, LTRB = mgrlib.FORMAT_NV12, mgrlib.FORMAT_YUV16, mgrlib.STEREO_LEFT_TOP_RIGHT_BOTTOM
    try:
        big = np.zeros(64 * 1024, np.uint8)
        w, H = 64, 128
        assert not m.add_buffer(1, big, w, H, NV12, LTRB, image_size=w * H * 3 // 2 - 1)      # imageSize is not w H 3 / 2
        assert not m.add_buffer(1, big, w, H, NV12, LTRB, image_size=w * H * 2)
        assert not m.add_buffer(1, big, w, H, YUV16, LTRB, image_size=w * H * 3 // 2)         # ... not 2 w H
        assert not m.add_buffer(1, big, w, H, YUV16, LTRB, image_size=0)
        assert not m.add_buffer(1, big, 63, H, NV12, LTRB, image_size=63 * H * 3 // 2)        # odd width
        assert not m.add_buffer(1, big, 63, H, YUV16, LTRB, image_size=2 * 63 * H)
        assert not m.add_buffer(1, big, w, 126, NV12, LTRB, image_size=w * 126 * 3 // 2)      # NV12: the height is no multiple of 4
        assert not m.add_buffer(1, big, w, 127, YUV16, LTRB, image_size=2 * w * 127)          # YUV16: not of 2
        assert m.add_buffer(1, big, w, 126, YUV16, LTRB, image_size=2 * w * 126)
        for structure in (mgrlib.ONE_IMAGE, mgrlib.STEREO_LEFT_LEFT_RIGHT_RIGHT):             # the two YUV formats exist in one structure only
            assert not m.add_buffer(1, big, w, H, NV12, structure, image_size=w * H * 3 // 2)
            assert not m.add_buffer(1, big, w, H, YUV16, structure, image_size=2 * w * H)
        assert not m.add_buffer(1, big, w, H, mgrlib.FORMAT_8UC4, mgrlib.ONE_IMAGE)           # 8UC4 stays refused at ingest
        # the two-buffer call keeps its two formats
        l = np.zeros((64, 64), np.uint8)
        assert m.add_stereo(1, l, l) and m.add_stereo(1, np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64, 3), np.uint8), fmt=mgrlib.FORMAT_8UC3)
        assert not m.add_stereo(1, l, l, fmt=NV12) and not m.add_stereo(1, l, l, fmt=YUV16)
    finally:
        m.close()


def test_manager_still_takes_8uc3_in_every_structure(mgrlib):
    m = mgrlib.Manager(log_level=4)
    try:
        rgb = ref.random_frame(ref.RGB8, 66, 64, 1)
        for structure in (mgrlib.ONE_IMAGE, mgrlib.STEREO_LEFT_TOP_RIGHT_BOTTOM, mgrlib.STEREO_LEFT_LEFT_RIGHT_RIGHT):
            for conv in (mgrlib.CONVERSION_NONE, mgrlib.CONVERSION_BGR2RGB):
                assert m.add_buffer(1, rgb, 66, 64, mgrlib.FORMAT_8UC3, structure, conv)
    finally:
        m.close()


# ---- realiseGray + realiseAdjust ---------------------------------------------------------------------------------------------------
def parent_to_gray(rgb, bgr):
    """the scalar loop the manager ran at enqueue before the conversion moved behind the upload, restated: per pixel
    (r 4899 + g 9617 + b 1868 + (1 << 13)) >> 14 with r, b swapped for BGR2RGB"""
    flat = rgb.reshape(-1, 3).astype(np.int64)
    r, g, b = flat[:, 2 if bgr else 0], flat[:, 1], flat[:, 0 if bgr else 2]
    return ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8).reshape(rgb.shape[:2])


@pytest.mark.parametrize("w,h", [(320, 240), (65, 64), (333, 77)])
def test_realise_gray_then_adjust_equals_the_earlier_conversion_then_adjust(mgrlib, w, h):
    from lpslam_amd import synth
    base = synth.random_image(w, h, 5).astype(np.float64)
    rgb = np.stack([base * 0.2 + 8, base * 0.35 + 3, 60 - base * 0.15], axis=-1).clip(0, 255).astype(np.uint8)      # dark, channels differ
    for bgr, fmt in ((False, ref.RGB8), (True, ref.BGR8)):
        grey = parent_to_gray(rgb, bgr)
        assert np.array_equal(mgrlib.realise_entry(rgb, w, h, fmt), grey)
        got = mgrlib.realise_entry(rgb, w, h, fmt, adjust=(-0.3, 1.4, 0.01, 0.99))
        assert np.array_equal(got, ir.adjust(grey))
        assert not np.array_equal(got, grey)                                     # the adjustment matters on these frames
    # the YUV sources go the same way
    for fmt, hh in ((ref.NV12, h & ~1), (ref.UYVY, h)):
        ww = w & ~1
        buf = ref.random_frame(fmt, ww, hh, 9)
        assert np.array_equal(mgrlib.realise_entry(buf, ww, hh, fmt, adjust=(-0.3, 1.4, 0.01, 0.99)), ir.adjust(ref.grey(buf, fmt)))


def test_compress_image_of_a_colour_buffer_is_unchanged(mgrlib):
    """LpSlamManager::compressImage calls the same host function for 8UC3: the stream is the grey picture's"""
    import ctypes as C
    from lpslam_amd import _build
    rgb = ref.random_frame(ref.RGB8, 64, 48, 2) // 4 * 4
    lib = C.CDLL(_build.host_library())
    enc = lib.lpslam_jpeg_encode_gray
    enc.restype = C.c_size_t; enc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    grey = np.ascontiguousarray(ref.grey_rgb(rgb))
    want = np.zeros(65536, np.uint8)
    n = enc(grey.ctypes.data, 64, 48, 95, want.ctypes.data, want.size)
    d = mgrlib.ImageDescription(0, mgrlib.FORMAT_8UC3, 0, 48, 64, rgb.size, 0, 0, mgrlib.ROSTimestamp(0, 0))
    out = np.zeros(rgb.size, np.uint8); m = C.c_uint32(0)
    f = lib.lpslam_manager_compress_image
    f.restype = C.c_int; f.argtypes = [C.c_void_p, C.POINTER(mgrlib.ImageDescription), C.c_void_p, C.POINTER(C.c_uint32)]
    assert f(rgb.ctypes.data, C.byref(d), out.ctypes.data, C.byref(m)) and n > 0
    assert out[:m.value].tobytes() == want[:n].tobytes()
