#!/usr/bin/env python3
"""Times the device JPEG encoder (lpslam_hip_jpeg_encode) against the host encoder (LpSlam::encode_jpeg_gray, one thread) on one
stereo pair, as the recorder encodes it: 1280 x 720 and 1920 x 1080, quality 70 and 95, `synth` frames and uniform noise.
Device: the median wall clock around the whole call -- host samples in, staging copy, upload, six launches, one wait, headers and
the copy of the streams out of page-locked memory -- after a warm-up.  Host: the median of the two images encoded one after the other
on the same machine.  The streams of both must be equal.  The kernel split comes from a separate run under rocprofv3 --kernel-trace
--stats.

usage: time_jpeg.py [--reps N] [--out FILE]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lpslam_amd import _build, hip, synth
    host = C.CDLL(_build.host_library())
    henc = host.lpslam_jpeg_encode_gray
    henc.restype = C.c_size_t
    henc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    enc = hip.JpegEncoder(1920, 1080, 2)
    f = enc.lib.lpslam_hip_jpeg_encode
    out = {"reps": args.reps, "cases": []}
    rng = np.random.default_rng(1)
    for w, h in ((1280, 720), (1920, 1080)):
        seq = synth.StereoSequence(w, h, 4)
        contents = {"synth": seq.frame(0), "noise": tuple(rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2))}
        for content, pair in contents.items():
            pair = [np.ascontiguousarray(p) for p in pair]
            for quality in (70, 95):
                caps = np.array([4096 + 3 * p.size for p in pair], np.int64)
                outs = [np.empty(int(c), np.uint8) for c in caps]
                px = (C.c_void_p * 2)(*[p.ctypes.data for p in pair]); op = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
                ws = np.array([w, w], np.int32); hs = np.array([h, h], np.int32); sz = np.zeros(2, np.int64)
                call = lambda: f(enc.h, 2, px, ws.ctypes.data, hs.ctypes.data, ws.ctypes.data, quality, op, caps.ctypes.data, sz.ctypes.data)
                for _ in range(3):
                    assert call() == 0
                td = []
                for _ in range(args.reps):
                    t0 = time.perf_counter(); rc = call(); td.append(time.perf_counter() - t0)
                    assert rc == 0
                dev = [o[:s].tobytes() for o, s in zip(outs, sz)]
                hb = [np.empty(int(c), np.uint8) for c in caps]
                th = []
                for _ in range(max(3, args.reps // 4)):
                    t0 = time.perf_counter()
                    n = [henc(p.ctypes.data, w, h, quality, b.ctypes.data, b.size) for p, b in zip(pair, hb)]
                    th.append(time.perf_counter() - t0)
                assert [b[:k].tobytes() for b, k in zip(hb, n)] == dev, "device and host streams differ"
                res = {"width": w, "height": h, "content": content, "quality": quality, "bytes": [len(d) for d in dev],
                       "device_pair_ms_median": float(np.median(td)) * 1e3, "device_pair_ms_min": min(td) * 1e3,
                       "host_pair_ms_median": float(np.median(th)) * 1e3}
                res["speedup"] = res["host_pair_ms_median"] / res["device_pair_ms_median"]
                out["cases"].append(res)
                print(json.dumps(res), flush=True)
    enc.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
