#!/usr/bin/env python3
"""Times the loop closer's verification of a keyframe's candidates: 3 sets of 20, 100 and 500 planted pairs
(30 % wrong matches), 200 iterations, the tracker's seed, gate 12, chi-square 10.
  (a) host:    LpSlam::sim3_solve_ransac on each set, one thread (lpslam_sim3_ransac_batch_host) -- the solver loop of the host path
  (b) present: lpslam_hip_sim3_transform_optimize alone on the seeds of (a) -- its allocations, copies, launch, synchronisation
  (c) device:  lpslam_hip_sim3_verify_batch end to end -- host arrays in, seed counts, s12 and counts out
Each is the median wall clock of --reps calls after 3 warm-up calls, (a), (b) and (c) alternating within one run; the results of
(c) must equal those of (a) followed by (b).  --manager adds the time per verified keyframe of the loop session of
tests/test_loop_device_gpu.py with the tracker option off and on (ms_loop_try of the tracker statistics).  --kernels N only makes N
verify calls at 100 pairs: the run to put under rocprofv3 --kernel-trace --stats for the kernel split.

usage: time_sim3_verify.py [--reps N] [--manager] [--kernels N] [--out STEM]      (writes STEM.json and STEM.txt)"""
import argparse, json, os, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAM = np.array([520.0, 515.0, 318.5, 243.25])


def planted(n, share, seed, hip):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3); a /= np.linalg.norm(a); ang = rng.uniform(0.05, 0.3)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
    t = rng.normal(0, 0.4, 3)
    p2 = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), rng.uniform(5, 20, n)])
    p1 = p2 @ R.T + t
    s1, s2 = 1.2 ** rng.integers(0, 4, n), 1.2 ** rng.integers(0, 4, n)
    proj = lambda p: np.column_stack([CAM[0] * p[:, 0] / p[:, 2] + CAM[2], CAM[1] * p[:, 1] / p[:, 2] + CAM[3]])
    o1 = proj(p1) + 0.4 * rng.normal(0, 1, (n, 2)) * s1[:, None]; o2 = proj(p2) + 0.4 * rng.normal(0, 1, (n, 2)) * s2[:, None]
    k = int(round(share * n))
    bad = rng.choice(n, k, replace=False)
    d = rng.uniform(0, 2 * np.pi, k)
    o1[bad] += np.column_stack([np.cos(d), np.sin(d)]) * rng.uniform(40.0, 80.0, (k, 1))
    out = np.zeros(n, hip.SIM3_PAIR_DTYPE)
    out["p1c"] = p1 + rng.normal(0, 0.004, p1.shape); out["p2c"] = p2; out["obs1"] = o1; out["obs2"] = o2
    out["inv_sigma2_1"] = 1.0 / s1 ** 2; out["inv_sigma2_2"] = 1.0 / s2 ** 2
    return out


def loop_session_ms():
    """ms per verified keyframe of the turning session with loop closing, option off and on"""
    from lpslam_amd import manager, synth
    W, H = 640, 480
    cfg = '"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 3, "localWindow": 4, "loopClosure": true, "asyncMapping": false'
    d = tempfile.mkdtemp(prefix="sim3_verify_time_")
    frames = synth.turning_sequence(W, H)[0]
    out = {}
    for name, flag in (("host", "false"), ("device", "true")):
        k = synth.intrinsics(W, H)
        m = manager.Manager()
        for num in (0, 1):
            c = manager.default_camera()
            c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
            c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
            m.set_camera(c)
        log = os.path.join(d, name + ".log")
        assert m.add_tracker("VSLAMStereo", "{" + cfg + ', "verifyLoopsOnDevice": %s}' % flag)
        m.collect_results(); m.provide_odometry(); m.log_to_file(log)
        m.start()
        for i, f in enumerate(frames):
            assert m.add_stereo((i + 1) * 40_000_000, f[0], f[1])
        t0 = time.time()
        while len(m.results) < len(frames) and time.time() - t0 < 60:
            time.sleep(0.01)
        m.stop()
        s = manager.Manager.statistics(log)
        out[name] = {k: s.get(k) for k in ("loop_tries", "ms_loop_try", "sim3_batches", "loops_closed", "ms_kf_loop")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--manager", action="store_true")
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_verify_time"))
    args = ap.parse_args()
    from lpslam_amd import _build, hip
    _build.host_library()
    ctx = hip.Context(640, 480, max_keypoints=500, num_levels=2)
    if args.kernels:
        sets = [planted(100, 0.3, 200 + i, hip) for i in range(3)]
        for _ in range(args.kernels):
            hip.sim3_verify_batch(ctx, sets, CAM, CAM, True, 200, 0x9E3779B9, 12, 10.0, want_inlier=False)
        ctx.close()
        return
    out = {"reps": args.reps, "sets": 3, "iterations": 200, "outlier_share": 0.3, "min_seed_inliers": 12, "chi_sq": 10.0, "cases": []}
    lines = []
    for n in (20, 100, 500):
        sets = [planted(n, 0.3, 100 * n + i, hip) for i in range(3)]
        host = lambda: hip.sim3_ransac_batch_host(sets, CAM, CAM, True, 200, 0x9E3779B9, want_iteration=False)
        seeds, cnt = host()[:2]
        assert (cnt >= 12).all(), cnt
        present = lambda: hip.sim3_transform_optimize(ctx, seeds, sets, CAM, CAM, 10.0, True)
        dev = lambda: hip.sim3_verify_batch(ctx, sets, CAM, CAM, True, 200, 0x9E3779B9, 12, 10.0, want_inlier=False)
        for _ in range(3):
            a = host(); b = present(); c = dev()
        assert np.array_equal(c[0], a[1]) and c[1].tobytes() == b[0].tobytes() and np.array_equal(c[2], b[2]), "device and host results differ"
        ta, tb, tc = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); host(); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); present(); tb.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); dev(); tc.append(time.perf_counter() - t0)
        res = {"pairs_per_set": n, "seed_inliers": [int(v) for v in c[0]], "n_inliers": [int(v) for v in c[2]],
               "a_host_ransac_ms_median": float(np.median(ta)) * 1e3, "a_host_ransac_ms_min": min(ta) * 1e3,
               "b_transform_optimize_ms_median": float(np.median(tb)) * 1e3, "b_transform_optimize_ms_min": min(tb) * 1e3,
               "c_verify_batch_ms_median": float(np.median(tc)) * 1e3, "c_verify_batch_ms_min": min(tc) * 1e3}
        res["a_plus_b_over_c"] = (res["a_host_ransac_ms_median"] + res["b_transform_optimize_ms_median"]) / res["c_verify_batch_ms_median"]
        out["cases"].append(res)
        lines.append("3 sets x %3d pairs, 200 iterations: (a) host RANSAC %.3f ms, (b) transform_optimize %.3f ms, (c) verify_batch %.3f ms (median of %d), (a + b) / c %.2f" %
                     (n, res["a_host_ransac_ms_median"], res["b_transform_optimize_ms_median"], res["c_verify_batch_ms_median"], args.reps, res["a_plus_b_over_c"]))
        print(lines[-1], flush=True)
    ctx.close()
    if args.manager:
        out["loop_session"] = loop_session_ms()
        for k, v in out["loop_session"].items():
            lines.append("loop session, verifyLoopsOnDevice %s: %s" % ("false" if k == "host" else "true", json.dumps(v)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as fh:
        json.dump(out, fh, indent=1)
    with open(args.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
