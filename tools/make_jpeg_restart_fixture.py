#!/usr/bin/env python3
"""Generates tests/golden/g19_jpeg_restart.npz: baseline JPEG streams with a restart interval (a DRI segment, RSTn markers in the
entropy-coded data) written by Pillow (libjpeg-turbo; restart_marker_blocks / restart_marker_rows), one component and YCbCr as 4:4:4,
4:2:2 and 4:2:0, and for each the grey samples libjpeg decodes from it (Image.draft("L")).  The fixtures of the device decoder's
restart path (csrc/jpeg_dec.hip, tests/test_jpeg_decode_restart_gpu.py) and of the host decoder that defines it
(tests/test_jpeg_restart_cpu.py).  Seeded numpy and the project's synth frames only.  Keys: "jpeg_<name>" (the stream),
"grey_<name>" (the samples); "names_grey" / "names_colour" list the streams in the order they were made, "dri" and "markers" hold
for each name of names_grey + names_colour the restart interval of its header and the RSTn markers in its data; "piece_edge" names
the stream that has a marker whose FF is the last byte of a 256-byte piece of the entropy-coded data and a marker directly behind a
stuffed FF 00."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lpslam_amd import synth            # noqa: E402

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
PIECE = 256


def grey_of(data):
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    im.load()
    assert im.mode == "L", im.mode
    return np.asarray(im).copy()


def colour_of(g):
    """a grey frame made colour: R = g, G = g rolled by 7 columns, B = g rolled by 11 rows"""
    return np.dstack([g, np.roll(g, 7, 1), np.roll(g, 11, 0)])


def layout(data):
    """(restart interval of the DRI segment or None, MCUs of the frame, offset of the entropy-coded data, offsets of the FF of every
    RSTn marker in it relative to that, offset of the marker that ends it)"""
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


def main():
    rng = np.random.default_rng(19)
    out, names_grey, names_colour, dris, counts = {}, [], [], [], []

    def encode(img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **kw)
        return buf.getvalue()

    def add(name, data, into, want_dri):
        dri, mcus, start, marks, end = layout(data)
        assert dri == want_dri, (name, dri, want_dri)
        want = (mcus + dri - 1) // dri - 1 if 0 < dri < mcus else 0
        assert len(marks) == want, (name, len(marks), want)
        out["jpeg_" + name] = np.frombuffer(data, np.uint8).copy()
        out["grey_" + name] = grey_of(data)
        into.append(name); dris.append(dri); counts.append(len(marks))
        print("%-36s %6d bytes  Ri %5d  %4d markers, first interval %6d bytes" % (name, len(data), dri, len(marks), marks[0] if marks else end))
        return marks, end

    # 7 x 6 = 42 blocks: an interval per block (13 to 54 bytes), a short last interval, an interval per block row, and DRI without a marker
    noise = rng.integers(0, 256, (41, 53), dtype=np.uint8)
    for ri in (1, 5, 7, 42, 100):
        add("noise_53x41_q90_ri%d" % ri, encode(noise, quality=90, restart_marker_blocks=ri), names_grey, ri)
    # 1200 intervals of two bytes: about 64 boundaries in every subsequence of 1024 bits
    marks, end = add("constant_320x240_q90_ri1", encode(np.full((240, 320), 77, np.uint8), quality=90, restart_marker_blocks=1), names_grey, 1)
    assert len(marks) == 1199 and end * 8 > 30 * 1024
    # intervals of about 800 bits that drift across the 1024-bit grid; a marker whose FF is the last byte of a 256-byte piece and one
    # directly behind a stuffed FF 00: seeds until one stream has both
    for seed in range(1000):
        img = np.random.default_rng(1900 + seed).integers(0, 256, (120, 160), dtype=np.uint8)
        data = encode(img, quality=100, restart_marker_blocks=1)
        _, _, start, marks, _ = layout(data)
        edge = [m for m in marks if m % PIECE == PIECE - 1]
        stuffed = [m for m in marks if m >= 2 and data[start + m - 2] == 0xFF and data[start + m - 1] == 0x00]
        if edge and stuffed:
            break
    assert edge and stuffed, "no seed gives both markers"
    add("noise_160x120_q100_ri1", data, names_grey, 1)
    out["piece_edge"] = np.array("noise_160x120_q100_ri1")
    print("  seed %d: FF at the end of a piece at %s, behind FF 00 at %s" % (1900 + seed, edge[:3], stuffed[:3]))
    # the first interval is longer than a workgroup of subsequences (256 x 1024 bits); a boundary lies in the second one
    marks, end = add("noise_320x240_q75_ri1000", encode(rng.integers(0, 256, (240, 320), dtype=np.uint8), quality=75, restart_marker_blocks=1000), names_grey, 1000)
    assert len(marks) == 1 and marks[0] * 8 > 256 * 1024
    # (50 points, not the 20000 of the other fixtures' frame: that crop alone is 75 kB of stream, and the file has to stay below 400 kB)
    frame = synth.StereoSequence(640, 480, 4, n_points=50).frame(0)[0]
    crop = np.ascontiguousarray(frame[100:340, 100:420])
    add("synth_320x240_q95_rows1", encode(crop, quality=95, restart_marker_rows=1), names_grey, 40)
    add("noise_96x64_q95_optimised_ri3", encode(rng.integers(0, 256, (64, 96), dtype=np.uint8), quality=95, optimize=True, restart_marker_blocks=3), names_grey, 3)
    # colour: the interval counts MCUs
    noise = rng.integers(0, 256, (41, 53, 3), dtype=np.uint8)
    for ss, code in SUBSAMPLING.items():
        for ri in (1, 4):
            add("noise_53x41_q90_%s_ri%d" % (ss, ri), encode(noise, quality=90, subsampling=code, restart_marker_blocks=ri), names_colour, ri)
    const = np.empty((48, 64, 3), np.uint8)
    const[:] = (200, 30, 90)
    add("constant_64x48_q90_420_ri1", encode(const, quality=90, subsampling=2, restart_marker_blocks=1), names_colour, 1)
    add("synth_320x240_q95_420_rows1", encode(colour_of(crop), quality=95, subsampling=2, restart_marker_rows=1), names_colour, 20)
    out["names_grey"] = np.array(names_grey)
    out["names_colour"] = np.array(names_colour)
    out["dri"] = np.array(dris, np.int32)
    out["markers"] = np.array(counts, np.int32)
    path = os.path.join(ROOT, "tests", "golden", "g19_jpeg_restart.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    assert size < 400_000, size


if __name__ == "__main__":
    main()
