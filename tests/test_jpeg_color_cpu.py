"""The host decoder LpSlam::decode_jpeg_gray (lpslam_jpeg_decode_gray) on three-component streams: for every stream of
tests/golden/g18_jpeg_color.npz (tools/make_jpeg_color_fixture.py: 4:4:4, 4:2:2 and 4:2:0 files written by Pillow = libjpeg-turbo) it
gives the grey samples libjpeg gave when the fixture was made (Image.draft("L"): the Y plane), bit for bit.  This pins the
definition that the device decoder's colour path is compared against (tests/test_jpeg_decode_color_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden


@pytest.fixture(scope="module")
def lib():
    from lpslam_amd import _build
    l = C.CDLL(_build.host_library())
    l.lpslam_jpeg_decode_gray.restype = C.c_int
    l.lpslam_jpeg_decode_gray.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return l


def _decode(lib, data):
    data = np.ascontiguousarray(data, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    out = np.zeros(1 << 19, np.uint8)
    rc = lib.lpslam_jpeg_decode_gray(data.ctypes.data, len(data), out.ctypes.data, out.size, C.byref(w), C.byref(h))
    return rc, (out[:w.value * h.value].reshape(h.value, w.value).copy() if rc == 0 else None)


def test_the_fixture_holds_what_the_device_tests_need():
    g = golden("g18_jpeg_color.npz")
    taken, other = [str(n) for n in g["names_taken"]], [str(n) for n in g["names_not_taken"]]
    assert len(taken) == 4 * 3 + 3 + 3 + 2 + 2 and other == ["restart_53x41_q90_420"]
    for ss in ("444", "422", "420"):
        assert sum(n.endswith(ss) for n in taken) >= 6
    for name in taken + other:
        data = g["jpeg_" + name].tobytes()
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        sof = data.index(b"\xff\xc0")
        assert data[sof + 9] == 3, name                                    # three components
        hv = {"444": 0x11, "422": 0x21, "420": 0x22}[name[-3:]]
        assert (data[sof + 11], data[sof + 14], data[sof + 17]) == (hv, 0x11, 0x11), name
        assert (b"\xff\xdd" in data) == (name in other), name             # DRI
    assert len(g["jpeg_noise_320x240_q75_420"]) * 8 > 256 * 1024          # more than one workgroup of subsequences


def test_the_host_decoder_gives_libjpegs_grey_samples_for_every_stream(lib):
    g = golden("g18_jpeg_color.npz")
    for name in [str(n) for n in g["names_taken"]] + [str(n) for n in g["names_not_taken"]]:
        rc, img = _decode(lib, g["jpeg_" + name])
        want = g["grey_" + name]
        assert rc == 0, name
        assert img.shape == want.shape, (name, img.shape, want.shape)
        assert np.array_equal(img, want), (name, int(np.abs(img.astype(int) - want).max()), int((img != want).sum()))


def test_pillow_agrees_when_present(lib):
    """the recorded samples against the Pillow of this machine (skipped where there is none)"""
    Image = pytest.importorskip("PIL.Image")
    import io
    g = golden("g18_jpeg_color.npz")
    for name in ("noise_53x41_q90_420", "noise_96x64_q95_optimised_422", "constant_64x48_q90_444"):
        im = Image.open(io.BytesIO(g["jpeg_" + name].tobytes())); im.draft("L", im.size); im.load()
        assert np.array_equal(np.asarray(im), g["grey_" + name])
