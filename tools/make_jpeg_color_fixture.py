#!/usr/bin/env python3
"""Generates tests/golden/g18_jpeg_color.npz: three-component (YCbCr) baseline JPEG streams written by Pillow (libjpeg-turbo) as
4:4:4, 4:2:2 and 4:2:0, and for each the grey samples libjpeg decodes from it (Image.draft("L") = JCS_GRAYSCALE, what
cv::imdecode(..., IMREAD_GRAYSCALE) asks for: the Y plane).  The fixtures of the device decoder's colour path (csrc/jpeg_dec.hip,
tests/test_jpeg_decode_color_gpu.py) and of the host decoder that defines it (tests/test_jpeg_color_cpu.py).  Seeded numpy and the
project's synth frames only.  Keys: "jpeg_<name>" (the stream), "grey_<name>" (the samples); "names_taken" lists the streams the
device decoder has to take, in the order they were made, "names_not_taken" the others."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lpslam_amd import synth            # noqa: E402

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def grey_of(data):
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    im.load()
    assert im.mode == "L", im.mode
    return np.asarray(im).copy()


def colour_of(g):
    """a grey frame made colour: R = g, G = g rolled by 7 columns, B = g rolled by 11 rows"""
    return np.dstack([g, np.roll(g, 7, 1), np.roll(g, 11, 0)])


def main():
    rng = np.random.default_rng(18)
    out, taken, not_taken = {}, [], []

    def add(name, img, into, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **kw)
        data = buf.getvalue()
        out["jpeg_" + name] = np.frombuffer(data, np.uint8).copy()
        out["grey_" + name] = grey_of(data)
        into.append(name)
        print("%-28s %6d bytes -> %dx%d" % (name, len(data), img.shape[1], img.shape[0]))
    # edge MCUs in both directions, an image smaller than one MCU
    for w, h in ((7, 5), (16, 16), (17, 16), (53, 41)):
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for ss, code in SUBSAMPLING.items():
            add("noise_%dx%d_q90_%s" % (w, h, ss), noise, taken, quality=90, subsampling=code)
    # the file's own Huffman tables for both table pairs
    noise = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    for ss, code in SUBSAMPLING.items():
        add("noise_96x64_q95_optimised_%s" % ss, noise, taken, quality=95, optimize=True, subsampling=code)
    # phase-locked in all three parts of the state: the hand-over between rounds
    const = np.empty((48, 64, 3), np.uint8)
    const[:] = (200, 30, 90)
    for ss, code in SUBSAMPLING.items():
        add("constant_64x48_q90_%s" % ss, const, taken, quality=90, subsampling=code)
    # the same over many subsequences (5 kB of stream, samples that compress to nothing)
    const = np.empty((480, 640, 3), np.uint8)
    const[:] = (200, 30, 90)
    for ss in ("444", "420"):
        add("constant_640x480_q90_%s" % ss, const, taken, quality=90, subsampling=SUBSAMPLING[ss])
    # more than 256 subsequences: two workgroups, the block scan crosses one
    add("noise_320x240_q75_420", rng.integers(0, 256, (240, 320, 3), dtype=np.uint8), taken, quality=75, subsampling=2)
    frame = synth.StereoSequence(640, 480, 4).frame(0)[0]
    add("synth_320x240_q95_420", colour_of(np.ascontiguousarray(frame[100:340, 100:420])), taken, quality=95, subsampling=2)
    # a restart interval: left to the host
    add("restart_53x41_q90_420", rng.integers(0, 256, (41, 53, 3), dtype=np.uint8), not_taken, quality=90, subsampling=2, restart_marker_blocks=4)
    out["names_taken"] = np.array(taken)
    out["names_not_taken"] = np.array(not_taken)
    path = os.path.join(ROOT, "tests", "golden", "g18_jpeg_color.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
