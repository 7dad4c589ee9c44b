#!/usr/bin/env python3
"""Times the device JPEG decoder on three-component streams (a decoder made with LPSLAM_HIP_JPEG_DEC_COLOR) against the host decoder
(LpSlam::decode_jpeg_gray, one thread), by the method of tools/time_jpeg_decode.py: one stereo pair, streams in host memory in,
samples in host memory out, the median of --reps wall clocks around the whole call after a warm-up; the host decoder on the same
two streams in the same run, preallocated buffers.  The samples of both must be equal.  Pairs: synth.StereoSequence(1280, 720,
4).frame(0) made colour (R = g, G = g rolled by 7 columns, B = g rolled by 11 rows), quality 70 and 95, 4:2:0 and 4:4:4, written by
Pillow; and, last, the grey pair of the gate of tests/test_jpeg_decode_gpu.py (host encoder, quality 95) through a decoder made
without the flag, which shows whether the grey path moved.

The streams come from Pillow where it is present, or from a file written before with --make-streams (a machine without Pillow).

usage: time_jpeg_decode_color.py [--reps N] [--streams FILE.npz | --make-streams FILE.npz] [--out FILE.json] [--txt FILE.txt]"""
import argparse, ctypes as C, io, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(70, "420", 2), (70, "444", 0), (95, "420", 2), (95, "444", 0)]


def colour_streams():
    from PIL import Image
    from lpslam_amd import synth
    out = {}
    for quality, name, subsampling in ROWS:
        for eye, g in zip("lr", synth.StereoSequence(1280, 720, 4).frame(0)):
            buf = io.BytesIO()
            Image.fromarray(np.dstack([g, np.roll(g, 7, 1), np.roll(g, 11, 0)])).save(buf, "JPEG", quality=quality, subsampling=subsampling)
            out["q%d_%s_%s" % (quality, name, eye)] = np.frombuffer(buf.getvalue(), np.uint8).copy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--streams", default=None)
    ap.add_argument("--make-streams", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if args.make_streams:
        np.savez(args.make_streams, **colour_streams())
        return
    from lpslam_amd import _build, hip, synth
    host = C.CDLL(_build.host_library())
    henc = host.lpslam_jpeg_encode_gray
    henc.restype = C.c_size_t
    henc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    hdec = host.lpslam_jpeg_decode_gray
    hdec.restype = C.c_int
    hdec.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    streams = dict(np.load(args.streams)) if args.streams else colour_streams()
    w, h = 1280, 720
    cases = [("colour %s q%d" % (name, quality), True, [np.ascontiguousarray(streams["q%d_%s_%s" % (quality, name, eye)]) for eye in "lr"]) for quality, name, _ in ROWS]
    grey = []
    for g in synth.StereoSequence(w, h, 4).frame(0):
        buf = np.zeros(4096 + 4 * g.size, np.uint8)
        n = henc(np.ascontiguousarray(g).ctypes.data, w, h, 95, buf.ctypes.data, buf.size)
        assert n > 0
        grey.append(buf[:n].copy())
    cases.append(("grey q95 (the grey gate)", False, grey))
    out = {"reps": args.reps, "cases": []}
    for label, color, pair in cases:
        dec = hip.JpegDecoder(1920, 1080, 2, color=color)
        f = dec.lib.lpslam_hip_jpeg_decode
        outs = [np.empty(w * h, np.uint8) for _ in pair]
        sp = (C.c_void_p * 2)(*[s.ctypes.data for s in pair]); op = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
        ss = np.array([len(s) for s in pair], np.int64); st = np.array([w, w], np.int32); cp = np.array([w * h, w * h], np.int64)
        ws = np.zeros(2, np.int32); hs = np.zeros(2, np.int32); status = np.zeros(2, np.int32)
        call = lambda: f(dec.h, 2, sp, ss.ctypes.data, op, st.ctypes.data, cp.ctypes.data, ws.ctypes.data, hs.ctypes.data, status.ctypes.data)
        for _ in range(3):
            assert call() == 0 and list(status) == [0, 0], (label, list(status))
        td = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); rc = call(); td.append(time.perf_counter() - t0)
            assert rc == 0 and list(status) == [0, 0]
        last = dec.last(2)
        dec.close()
        hb = [np.empty(w * h, np.uint8) for _ in pair]
        hw, hh = C.c_int(0), C.c_int(0)
        th = []
        for k in range(3 + args.reps):
            t0 = time.perf_counter()
            rcs = [hdec(s.ctypes.data, len(s), b.ctypes.data, b.size, C.byref(hw), C.byref(hh)) for s, b in zip(pair, hb)]
            if k >= 3:
                th.append(time.perf_counter() - t0)
            assert rcs == [0, 0]
        assert all(np.array_equal(a, b) for a, b in zip(outs, hb)), "device and host samples differ"
        res = {"pair": label, "width": w, "height": h, "bytes": [len(s) for s in pair],
               "device_pair_ms_median": float(np.median(td)) * 1e3, "device_pair_ms_min": min(td) * 1e3,
               "host_pair_ms_median": float(np.median(th)) * 1e3, "rounds": [l[0] for l in last], "subsequences": [l[1] for l in last],
               "blocks": [l[2] for l in last]}
        res["speedup"] = res["host_pair_ms_median"] / res["device_pair_ms_median"]
        out["cases"].append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if args.txt:
        with open(args.txt, "w") as fh:
            fh.write("pair (1280x720)             bytes (L)  device pair ms (median / min)  host pair ms  speedup  rounds  subsequences\n")
            for r in out["cases"]:
                fh.write("%-26s  %9d  %8.3f / %-8.3f             %9.2f  %7.1f  %6d  %d\n" % (
                    r["pair"], r["bytes"][0], r["device_pair_ms_median"], r["device_pair_ms_min"],
                    r["host_pair_ms_median"], r["speedup"], max(r["rounds"]), r["subsequences"][0]))


if __name__ == "__main__":
    main()
