"""The keypoint-camera stage's own time (DESIGN.md sections 30 and 32): k_undistort_compact on one image slot that holds an extraction's
keypoints, taken with the context's event timers after a warm-up.  The slot is restored before every sample (the stage rewrites it); the
timed region is the one launch.  Usage: python tools/time_undistort.py [--model fisheye|radtan] [--samples 30]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lpslam_amd import hip, synth  # noqa: E402


def restore(ctx, slot, kp, desc):
    ctx.set_descriptors(slot, desc)
    ptr = C.c_void_p()
    assert ctx.lib.lpslam_hip_keypoint_buffers(ctx.h, slot, C.byref(ptr), None, None) == 0
    f = ctx.lib.hipMemcpy
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert f(ptr, kp.ctypes.data, kp.nbytes, 1) == 0
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", choices=("fisheye", "radtan"), default="fisheye")
    args = ap.parse_args()
    for (w, h, levels) in ((640, 480, 3), (1280, 720, 8)):
        ctx = hip.Context(w, h, 2000, 1.2, levels, max_images=2)
        ctx.upload(0, synth.random_image(w, h, 5))
        ctx.extract(1)
        kp, desc = ctx.keypoints(0)
        kp = np.ascontiguousarray(kp)
        if args.model == "fisheye":
            # a lens whose 70-degree circle cuts the image: a part of the keypoints is removed
            ctx.set_keypoint_camera(hip.Fisheye(0.34 * w, 0.34 * w, w / 2.0, h / 2.0, (-0.0115, 0.0479, -0.0451, 0.0083), 70.0))
        else:
            # a lens that folds over 0.778 f = 0.39 w from the principal point: the corners and the ends of the image are removed
            ctx.set_keypoint_camera_radtan(hip.Radtan(0.5 * w, 0.5 * w, w / 2.0, h / 2.0, -0.6, 0.05, 0.002, -0.001, 0.0))
        ms = []
        for i in range(args.warmup + args.samples):
            restore(ctx, 0, kp, desc)
            ctx.timer_begin(0); ctx.stage_undistort(1); ctx.timer_end(0)
            ctx.sync()
            if i >= args.warmup:
                ms.append(ctx.timer_ms(0))
        kept = len(ctx.keypoints(0)[0])
        us = 1e3 * np.array(ms)
        print(json.dumps({"model": args.model, "image": "%dx%d" % (w, h), "keypoints": len(kp), "kept": kept, "dropped": ctx.undistort_dropped(0), "samples": len(ms),
                          "us_median": round(float(np.median(us)), 2), "us_min": round(float(us.min()), 2), "us_max": round(float(us.max()), 2)}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
