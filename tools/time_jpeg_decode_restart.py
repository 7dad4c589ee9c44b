#!/usr/bin/env python3
"""Times the device JPEG decoder on streams with a restart interval (a decoder switched on with lpslam_hip_jpeg_dec_take_restart)
against the host decoder (LpSlam::decode_jpeg_gray, one thread), by the method of tools/time_jpeg_decode.py: one 1280 x 720 synth
stereo pair at quality 95 from the host encoder (lpslam_jpeg_encode_gray_restart), streams in host memory in, samples in host memory
out, the median wall clock around the whole call after a warm-up.  Rows: no restart interval, one block row an interval (Ri = 160, the
gate of tests/test_jpeg_decode_restart_gpu.py), and shorter intervals, to see what the entry states every interval buy: rounds and time.

usage: time_jpeg_decode_restart.py [--reps N] [--out FILE.json] [--txt FILE.txt]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INTERVALS = (0, 160, 40, 8, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    from lpslam_amd import _build, hip, synth
    host = C.CDLL(_build.host_library())
    henc = host.lpslam_jpeg_encode_gray_restart
    henc.restype = C.c_size_t
    henc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    hdec = host.lpslam_jpeg_decode_gray
    hdec.restype = C.c_int
    hdec.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    w, h = 1280, 720
    frames = [np.ascontiguousarray(g) for g in synth.StereoSequence(w, h, 4).frame(0)]
    dec = hip.JpegDecoder(1920, 1080, 2, restart=True)
    f = dec.lib.lpslam_hip_jpeg_decode
    out = {"reps": args.reps, "cases": []}
    for ri in INTERVALS:
        pair = []
        for g in frames:
            buf = np.zeros(8192 + 6 * g.size, np.uint8)
            n = henc(g.ctypes.data, w, h, 95, ri, buf.ctypes.data, buf.size)
            assert n > 0
            pair.append(buf[:n].copy())
        outs = [np.empty(w * h, np.uint8) for _ in pair]
        sp = (C.c_void_p * 2)(*[s.ctypes.data for s in pair]); op = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
        ss = np.array([len(s) for s in pair], np.int64); st = np.array([w, w], np.int32); cp = np.array([w * h, w * h], np.int64)
        ws = np.zeros(2, np.int32); hs = np.zeros(2, np.int32); status = np.zeros(2, np.int32)
        call = lambda: f(dec.h, 2, sp, ss.ctypes.data, op, st.ctypes.data, cp.ctypes.data, ws.ctypes.data, hs.ctypes.data, status.ctypes.data)
        for _ in range(3):
            assert call() == 0 and list(status) == [0, 0], (ri, list(status))
        td = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); rc = call(); td.append(time.perf_counter() - t0)
            assert rc == 0 and list(status) == [0, 0]
        last = dec.last(2)
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
        res = {"restart_interval": ri, "width": w, "height": h, "bytes": [len(s) for s in pair],
               "device_pair_ms_median": float(np.median(td)) * 1e3, "device_pair_ms_min": min(td) * 1e3,
               "host_pair_ms_median": float(np.median(th)) * 1e3, "rounds": [l[0] for l in last], "subsequences": [l[1] for l in last]}
        res["speedup"] = res["host_pair_ms_median"] / res["device_pair_ms_median"]
        out["cases"].append(res)
        print(json.dumps(res), flush=True)
    dec.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if args.txt:
        with open(args.txt, "w") as fh:
            fh.write("1280x720 synth q95 pair   Ri  bytes (L)  device pair ms (median / min)  host pair ms  speedup  rounds  subsequences\n")
            for r in out["cases"]:
                fh.write("                       %5d  %9d  %8.3f / %-8.3f             %9.2f  %7.1f  %6d  %d\n" % (
                    r["restart_interval"], r["bytes"][0], r["device_pair_ms_median"], r["device_pair_ms_min"],
                    r["host_pair_ms_median"], r["speedup"], max(r["rounds"]), r["subsequences"][0]))


if __name__ == "__main__":
    main()
