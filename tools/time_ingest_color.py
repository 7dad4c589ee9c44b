"""Frames per second of one manager fed 1280 x 720 stereo 8UC3 frames (two buffers), with the compiled identity-odometry and counting
callbacks: the measurement of DESIGN.md section 29.  Uses only what the library had before the conversion moved to the device, so the
same script runs on the commit before it.

    python tools/time_ingest_color.py [--frames 600] [--warmup 60] [--repeats 3] [--gray] [--out FILE]

Prints one JSON line per repeat: frames per second from the first timed frame fed to the last result, and the milliseconds per frame
the feeding thread spent inside addStereoImageFromBuffer (where the host conversion used to run).  --gray feeds the grey of the same
frames as 8UC1, for scale.  At most 4 frames are in flight, so the queue holds a successor for the prefetch and memory stays bounded."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1280, 720
TRACKER = '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "prefetch": true}'


def colour(img):
    f = img.astype(np.float64)
    return np.ascontiguousarray(np.stack([f * 0.9 + 10, f * 0.7 + 40, f * 0.5 + 90], axis=-1).clip(0, 255).astype(np.uint8))


def grey(rgb):
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    return np.ascontiguousarray(((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8))


def one_run(manager, synth, frames, n, warmup, as_grey):
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in (0, 1):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    assert m.add_tracker("VSLAMStereo", TRACKER)
    m.count_results(); m.provide_odometry(native=True)
    m.start()
    fmt = manager.FORMAT_8UC1 if as_grey else manager.FORMAT_8UC3
    add = m.lib.lpslam_manager_add_stereo_image
    t_add = 0.0
    t0 = None
    order = list(range(len(frames))) + list(range(len(frames) - 2, 0, -1))      # forth and back: the motion stays continuous
    for i in range(warmup + n):
        if i == warmup:
            while m.result_counts()[0] < i:
                time.sleep(0.0002)
            t0 = time.perf_counter()
        while i - m.result_counts()[0] >= 4:
            time.sleep(0.0001)
        l, r = frames[order[i % len(order)]]
        ts = (i + 1) * 40_000_000
        d = manager.ImageDescription(manager.STEREO_TWO_BUFFER, fmt, 0, H, W, l.size, r.size, 1, manager.ROSTimestamp(int(ts // 10**9), int(ts)))
        ta = time.perf_counter()
        assert add(m.h, 0, int(ts), l.ctypes.data, r.ctypes.data, C.byref(d))
        if i >= warmup:
            t_add += time.perf_counter() - ta
    while m.result_counts()[0] < warmup + n:
        time.sleep(0.0002)
    dt = time.perf_counter() - t0
    results, valid = m.result_counts()
    m.stop()
    stats = m.tracker_statistics()
    m.close()
    return {"format": "8UC1" if as_grey else "8UC3", "frames": n, "fps": n / dt, "ms_in_add_per_frame": 1e3 * t_add / n, "valid": valid,
            "color_converted": stats.get("color_converted"), "ms_front_end": stats.get("ms_front_end"), "ms_per_frame": stats.get("ms_per_frame")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--gray", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lpslam_amd import hip, manager, synth
    if hip.device_count() < 1:
        raise SystemExit("time_ingest_color needs an MI355X: no HIP device visible")
    manager.load()
    seq = synth.StereoSequence(W, H, 4, n_points=6000)
    frames = []
    for i in range(12):
        l, r = seq.frame(i)
        cl, cr = colour(l), colour(r)
        frames.append((grey(cl), grey(cr)) if a.gray else (cl, cr))
    lines = []
    for rep in range(a.repeats):
        res = one_run(manager, synth, frames, a.frames, a.warmup, a.gray)
        res["repeat"] = rep
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
