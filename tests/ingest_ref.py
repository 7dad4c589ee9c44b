"""The grey value of a colour or YUV frame, restated in numpy: the definition the device kernel
(lpslam_amd/csrc/ingest.hip) and the host function (lpslam_amd/host/ingest.cpp) are compared against, exactly.

  RGB -> grey   g = (R 4899 + G 9617 + B 1868 + 8192) >> 14; BGR swaps the roles of bytes 0 and 2
  YUV -> RGB    BT.601 limited range, 8 bit: y = max(0, Y - 16) 1220542, u = U - 128, v = V - 128, int32, arithmetic shift
                  R = sat8((y + 1673527 v + 2^19) >> 20)
                  G = sat8((y - 852492 v - 409993 u + 2^19) >> 20)
                  B = sat8((y + 2116026 u + 2^19) >> 20)
                then the grey formula; chroma is replicated, not interpolated
  NV12          (3 h / 2, w) bytes: the Y plane, then h / 2 rows of U V pairs, one pair per 2 x 2 block
  UYVY          (h, 2 w) bytes: U0 Y0 V0 Y1 per pixel pair
"""
import numpy as np

GRAY8, RGB8, BGR8, NV12, UYVY = range(5)          # LPSLAM_HIP_PIXEL_*


def grey_of_rgb(r, g, b):
    r, g, b = (np.asarray(v).astype(np.int32) for v in (r, g, b))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def rgb_of_yuv(y, u, v):
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    yy = np.maximum(0, y - 16) * np.int32(1220542)
    u = u - 128; v = v - 128
    r = np.clip((yy + 1673527 * v + (1 << 19)) >> 20, 0, 255)
    g = np.clip((yy - 852492 * v - 409993 * u + (1 << 19)) >> 20, 0, 255)
    b = np.clip((yy + 2116026 * u + (1 << 19)) >> 20, 0, 255)
    return r, g, b


def grey_of_yuv(y, u, v):
    return grey_of_rgb(*rgb_of_yuv(y, u, v))


def grey_rgb(img, bgr=False):
    """(h, w, 3) -> (h, w)"""
    img = np.asarray(img)
    return grey_of_rgb(img[..., 2], img[..., 1], img[..., 0]) if bgr else grey_of_rgb(img[..., 0], img[..., 1], img[..., 2])


def grey_nv12(buf):
    """(3 h / 2, w) -> (h, w)"""
    buf = np.asarray(buf)
    h = buf.shape[0] * 2 // 3
    w = buf.shape[1]
    assert h % 2 == 0 and w % 2 == 0 and h * 3 // 2 == buf.shape[0]
    uv = buf[h:].reshape(h // 2, w // 2, 2)
    u = np.repeat(np.repeat(uv[..., 0], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(uv[..., 1], 2, axis=0), 2, axis=1)
    return grey_of_yuv(buf[:h], u, v)


def grey_uyvy(buf):
    """(h, 2 w) -> (h, w)"""
    buf = np.asarray(buf)
    h, w = buf.shape[0], buf.shape[1] // 2
    assert w % 2 == 0
    q = buf.reshape(h, w // 2, 4)
    u = np.repeat(q[..., 0], 2, axis=1); v = np.repeat(q[..., 2], 2, axis=1)
    y = q[..., [1, 3]].reshape(h, w)
    return grey_of_yuv(y, u, v)


def grey(buf, fmt):
    return {GRAY8: lambda b: np.asarray(b).copy(), RGB8: grey_rgb, BGR8: lambda b: grey_rgb(b, True), NV12: grey_nv12, UYVY: grey_uyvy}[fmt](buf)


def frame_shape(fmt, w, h):
    """shape of the byte array that holds a w x h frame of the format"""
    return {GRAY8: (h, w), RGB8: (h, w, 3), BGR8: (h, w, 3), NV12: (h * 3 // 2, w), UYVY: (h, 2 * w)}[fmt]


def random_frame(fmt, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, frame_shape(fmt, w, h), dtype=np.uint8)


# ---- every triple ---------------------------------------------------------------------------------------------------------------
def rgb_sweep(k):
    """frame k of 64 (512 x 512 x 3): first channel in {4 k .. 4 k + 3}, the other two over all 65 536 pairs -- together every triple"""
    a = np.arange(512 * 512, dtype=np.int64).reshape(512, 512)
    img = np.empty((512, 512, 3), np.uint8)
    img[..., 0] = 4 * k + (a >> 16)
    img[..., 1] = (a >> 8) & 255
    img[..., 2] = a & 255
    return img


def nv12_sweep(k):
    """frame k of 64 (512 x 512 NV12): the 2 x 2 block b carries (U, V) = (b >> 8, b & 255) and Y = 4 k .. 4 k + 3 on its four pixels"""
    buf = np.empty((768, 512), np.uint8)
    buf[0:512:2, 0::2] = 4 * k; buf[0:512:2, 1::2] = 4 * k + 1
    buf[1:512:2, 0::2] = 4 * k + 2; buf[1:512:2, 1::2] = 4 * k + 3
    b = np.arange(65536, dtype=np.int64).reshape(256, 256)
    uv = buf[512:].reshape(256, 256, 2)
    uv[..., 0] = b >> 8; uv[..., 1] = b & 255
    return buf


def uyvy_sweep(k):
    """frame k of 128 (512 x 256 UYVY, 65 536 pixel pairs): pair p carries (U, V) = (p >> 8, p & 255) and Y = 2 k, 2 k + 1"""
    buf = np.empty((256, 1024), np.uint8)
    q = buf.reshape(256, 256, 4)
    p = np.arange(65536, dtype=np.int64).reshape(256, 256)
    q[..., 0] = p >> 8; q[..., 2] = p & 255
    q[..., 1] = 2 * k; q[..., 3] = 2 * k + 1
    return buf


# worked by hand: (Y, U, V) -> grey
WORKED_YUV = {
    (16, 128, 128): 0,         # black: y = 0, R = G = B = (2^19) >> 20 = 0
    (235, 128, 128): 255,      # white: y = 219 * 1220542 = 267298698, + 2^19 = 267822986, >> 20 = 255 on all three
    (0, 128, 128): 0,          # Y < 16 clamps to the black level
    (15, 128, 128): 0,
    # (255, 255, 255): y = 239 * 1220542 = 291709538; u = v = 127
    #   R = (291709538 + 212537929 + 524288) >> 20 = 504771755 >> 20 = 481 -> 255
    #   G = (291709538 - 108266484 - 52069111 + 524288) >> 20 = 131898231 >> 20 = 125
    #   B = (291709538 + 268735302 + 524288) >> 20 = 560969128 >> 20 = 534 -> 255
    #   grey = (255 * 4899 + 125 * 9617 + 255 * 1868 + 8192) >> 14 = 2935902 >> 14 = 179
    (255, 255, 255): 179,
    # (0, 0, 0): y = 0; u = v = -128
    #   R = (-214211456 + 524288) >> 20 = -213687168 >> 20 = -204 -> 0
    #   G = (109118976 + 52479104 + 524288) >> 20 = 162122368 >> 20 = 154
    #   B = (-270851328 + 524288) >> 20 -> 0
    #   grey = (154 * 9617 + 8192) >> 14 = 1489210 >> 14 = 90
    (0, 0, 0): 90,
    # (255, 0, 255): y = 291709538; u = -128, v = 127
    #   R = 481 -> 255 (as above)
    #   G = (291709538 - 108266484 + 52479104 + 524288) >> 20 = 236446446 >> 20 = 225
    #   B = (291709538 - 270851328 + 524288) >> 20 = 21382498 >> 20 = 20
    #   grey = (255 * 4899 + 225 * 9617 + 20 * 1868 + 8192) >> 14 = 3458622 >> 14 = 211
    (255, 0, 255): 211,
}
