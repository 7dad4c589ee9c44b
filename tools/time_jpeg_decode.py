#!/usr/bin/env python3
"""Times the device JPEG decoder (lpslam_hip_jpeg_decode) against the host decoder (LpSlam::decode_jpeg_gray, one thread) on one
stereo pair, as the replay reader decodes it: 1280 x 720 and 1920 x 1080, quality 70 and 95, `synth` frames and uniform noise, and a
constant 1280 x 720 image (the slow-synchronisation case).  Device: the median wall clock around the whole call -- streams in host
memory in, header parse, staging copy, one upload, the launch chain, the waits, and the copy of the samples out of page-locked
memory -- after a warm-up.  Host: the median of the two streams decoded one after the other on the same machine.  The samples of both
must be equal.  The kernel split comes from a separate run under rocprofv3 --kernel-trace --stats (--profile-case runs one case a few
times and nothing else).

usage: time_jpeg_decode.py [--reps N] [--out FILE.json] [--txt FILE.txt] [--profile-case]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--profile-case", action="store_true")
    args = ap.parse_args()
    from lpslam_amd import _build, hip, synth
    host = C.CDLL(_build.host_library())
    henc = host.lpslam_jpeg_encode_gray
    henc.restype = C.c_size_t
    henc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    hdec = host.lpslam_jpeg_decode_gray
    hdec.restype = C.c_int
    hdec.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]

    def encode(img, quality):
        buf = np.zeros(4096 + 4 * img.size, np.uint8)
        n = henc(img.ctypes.data, img.shape[1], img.shape[0], quality, buf.ctypes.data, buf.size)
        assert n > 0
        return buf[:n].copy()

    dec = hip.JpegDecoder(1920, 1080, 2)
    f = dec.lib.lpslam_hip_jpeg_decode
    out = {"reps": args.reps, "cases": []}
    rng = np.random.default_rng(1)
    cases = []
    for w, h in ((1280, 720), (1920, 1080)):
        seq = synth.StereoSequence(w, h, 4)
        contents = {"synth": seq.frame(0), "noise": tuple(rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2))}
        for content, pair in contents.items():
            for quality in (70, 95):
                cases.append((w, h, content, quality, [np.ascontiguousarray(p) for p in pair]))
    cases.append((1280, 720, "constant", 95, [np.full((720, 1280), 128, np.uint8)] * 2))
    if args.profile_case:
        cases = [c for c in cases if c[:4] == (1280, 720, "synth", 95)]
    for w, h, content, quality, pair in cases:
        streams = [encode(p, quality) for p in pair]
        outs = [np.empty(w * h, np.uint8) for _ in pair]
        sp = (C.c_void_p * 2)(*[s.ctypes.data for s in streams]); op = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
        ss = np.array([len(s) for s in streams], np.int64); st = np.array([w, w], np.int32); cp = np.array([w * h, w * h], np.int64)
        ws = np.zeros(2, np.int32); hs = np.zeros(2, np.int32); status = np.zeros(2, np.int32)
        call = lambda: f(dec.h, 2, sp, ss.ctypes.data, op, st.ctypes.data, cp.ctypes.data, ws.ctypes.data, hs.ctypes.data, status.ctypes.data)
        for _ in range(3):
            assert call() == 0 and list(status) == [0, 0]
        td = []
        for _ in range(5 if args.profile_case else args.reps):
            t0 = time.perf_counter(); rc = call(); td.append(time.perf_counter() - t0)
            assert rc == 0 and list(status) == [0, 0]
        if args.profile_case:
            continue
        last = dec.last(2)
        hb = [np.empty(w * h, np.uint8) for _ in pair]
        hw, hh = C.c_int(0), C.c_int(0)
        th = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rcs = [hdec(s.ctypes.data, len(s), b.ctypes.data, b.size, C.byref(hw), C.byref(hh)) for s, b in zip(streams, hb)]
            th.append(time.perf_counter() - t0)
            assert rcs == [0, 0]
        assert all(np.array_equal(a, b) for a, b in zip(outs, hb)), "device and host samples differ"
        res = {"width": w, "height": h, "content": content, "quality": quality, "bytes": [len(s) for s in streams],
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
            fh.write("size        content   q   bytes (L)  device pair ms (median / min)  host pair ms  speedup  rounds  subsequences\n")
            for r in out["cases"]:
                fh.write("%4dx%-5d  %-8s %3d  %9d  %8.3f / %-8.3f             %9.2f  %7.1f  %6d  %d\n" % (
                    r["width"], r["height"], r["content"], r["quality"], r["bytes"][0], r["device_pair_ms_median"], r["device_pair_ms_min"],
                    r["host_pair_ms_median"], r["speedup"], max(r["rounds"]), r["subsequences"][0]))


if __name__ == "__main__":
    main()
