"""The triangulation step's own time: lpslam_hip_triangulate_neighbours on a slot of 2000 keypoints against 10
and 20 neighbour keyframes of 2000 keypoints -- the chain on the stream (upload, k_epi_topk, k_tri_pairs) by the context's event timers,
the whole call by the wall clock -- and the host form (csrc/triangulate_math.h through the C shim) on the same inputs, for the ratio.
Usage: python tools/time_triangulate.py [--samples 30]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lpslam_amd import _build, hip, manager  # noqa: E402

W, H, N, LEVELS = 640, 480, 2000, 3
CAM = (525.0, 525.0, 320.0, 240.0, 0.0, 1.2)


def pose_at(centre, yaw):
    """world -> camera pose (qw qx qy qz tx ty tz) of a camera at `centre` turned by yaw about y"""
    c, s = math.cos(yaw), math.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
    t = -R @ np.asarray(centre, np.float64)
    return np.array([math.cos(yaw / 2), 0.0, -math.sin(yaw / 2), 0.0, t[0], t[1], t[2]])


def project(pose, X):
    yaw = -2.0 * math.atan2(pose[2], pose[0])
    c, s = math.cos(yaw), math.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
    Xc = X @ R.T + pose[4:7]
    return CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]


def keyframe(rng, pose, X, base_desc):
    """the scene's points seen from `pose`: keypoints in a shuffled order, descriptors with up to 40 flipped bits"""
    n = len(X)
    u, v = project(pose, X)
    order = rng.permutation(n)
    kp = np.zeros(n, hip.KP_DTYPE)
    kp["x"] = u[order] + rng.uniform(-0.4, 0.4, n); kp["y"] = v[order] + rng.uniform(-0.4, 0.4, n)
    kp["octave"] = rng.integers(0, LEVELS, n); kp["size"] = 31.0; kp["class_id"] = -1
    bits = np.unpackbits(base_desc[order], axis=1)
    flip = rng.random(bits.shape) < rng.uniform(0.0, 0.15, (n, 1))
    return kp, np.packbits(bits ^ flip, axis=1)


def plant(ctx, slot, kp, desc):
    ctx.set_descriptors(slot, desc)
    ptr = C.c_void_p()
    assert ctx.lib.lpslam_hip_keypoint_buffers(ctx.h, slot, C.byref(ptr), None, None) == 0
    f = ctx.lib.hipMemcpy
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    kp = np.ascontiguousarray(kp)
    assert f(ptr, kp.ctypes.data, kp.nbytes, 1) == 0
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    _build.host_library()
    rng = np.random.default_rng(3)
    z = rng.uniform(4, 20, N)
    X = np.stack([rng.uniform(-0.25, 0.25, N) * z, rng.uniform(-0.18, 0.18, N) * z, z], 1)
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    pose_c = pose_at([0, 0, 0], 0.0)
    ctx = hip.Context(W, H, N, 1.2, LEVELS, max_images=2)
    scale = np.asarray(ctx.scale, np.float32)
    kp_c, desc_c = keyframe(rng, pose_c, X, base)
    plant(ctx, 0, kp_c, desc_c)
    group1 = np.zeros(N, np.int32)
    cam = hip.TriCamera(*CAM)
    for n_sets in (10, 20):
        sets = []
        for s in range(n_sets):
            pose = pose_at([0.3 * math.cos(s), 0.05 * math.sin(s), -0.15 * (s + 1)], 0.01 * (s % 5 - 2))
            kp, desc = keyframe(rng, pose, X, base)
            F, ep = manager.tri_epipolar(CAM, pose_c, pose)
            sets.append({"kpts": kp, "desc": desc, "group": np.zeros(N, np.int32), "pose": pose, "F": F, "epipole": ep})
        chain, wall = [], []
        for i in range(args.warmup + args.samples):
            t0 = time.perf_counter()
            ctx.timer_begin(0)
            out = ctx.triangulate_neighbours(0, group1, pose_c, cam, sets, scale=scale)
            ctx.timer_end(0)
            t1 = time.perf_counter()
            ctx.sync()
            if i >= args.warmup:
                chain.append(1e3 * ctx.timer_ms(0)); wall.append(1e6 * (t1 - t0))
        k1 = np.zeros(N, np.dtype(manager.TRI_KP_DTYPE)); k1["x"] = kp_c["x"]; k1["y"] = kp_c["y"]; k1["octave"] = kp_c["octave"]; k1["x_right"] = -1; k1["depth"] = -1
        host = []
        for i in range(3):
            t0 = time.perf_counter()
            listed = 0
            for s in sets:
                k2 = np.zeros(N, np.dtype(manager.TRI_KP_DTYPE)); k2["x"] = s["kpts"]["x"]; k2["y"] = s["kpts"]["y"]; k2["octave"] = s["kpts"]["octave"]; k2["x_right"] = -1; k2["depth"] = -1
                j, dist, count, keys = manager.tri_candidates_host(CAM, scale, k1, desc_c, group1, k2, s["desc"], s["group"], s["F"], s["epipole"])
                qi, r = np.nonzero(j >= 0)
                manager.tri_pair_host(CAM, scale, pose_c, s["pose"], k1[qi], k2[j[qi, r]])
                listed += len(qi)
            host.append(1e6 * (time.perf_counter() - t0))
        assert listed == int((out["j"] >= 0).sum())
        chain, wall, host = np.array(chain), np.array(wall), np.array(host)
        print(json.dumps({"keypoints": N, "neighbours": n_sets, "listed_candidates": listed, "landmarks": int((out["code"] > 0).sum()), "samples": len(chain),
                          "chain_us_median": round(float(np.median(chain)), 1), "chain_us_min": round(float(chain.min()), 1), "chain_us_max": round(float(chain.max()), 1),
                          "call_us_median": round(float(np.median(wall)), 1), "call_us_min": round(float(wall.min()), 1), "call_us_max": round(float(wall.max()), 1),
                          "host_form_us_median": round(float(np.median(host)), 1), "host_form_us_min": round(float(host.min()), 1), "host_form_us_max": round(float(host.max()), 1)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
