#!/usr/bin/env python3
"""Times the pose covariance call at S = 1, n = 20, 100, 500, 2000 observations (half of them stereo; points 2 to
20 m in front of a random pose, weights 1.2^-2o, residuals of up to 2 pixels):
  (a) device:   lpslam_hip_pose_covariance_batch end to end -- host arrays in, the six result arrays out
  (b) host:     lpslam_pose_covariance_batch_host on one thread -- the same arithmetic
  (c) optimise: lpslam_hip_pose_optimize on the same observations from the same pose -- the call the covariance follows in the tracker
Each is the median wall clock of 21 calls after 3 warm-up calls, (a), (b) and (c) alternating within one run; the results of (a) must
equal those of (b) byte for byte.  --manager adds the stereo session of tests/test_pose_sigma_gpu.py with the tracker option off and on:
ms_dev_pose_sigma beside ms_dev_pose, and ms_per_frame of both sessions (each run --sessions times, every value listed).

usage: time_pose_covariance.py [--reps N] [--manager] [--sessions N] [--out STEM]      (writes STEM.json and STEM.txt)"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAM = np.array([500.0, 500.0, 320.0, 240.0, 60.0])


def make_set(n, seed):
    rng = np.random.default_rng([seed, n])
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    t = rng.uniform(-2, 2, 3)
    d = rng.uniform(2, 20, n); u = rng.uniform(60, 620, n); v = rng.uniform(20, 460, n)
    pc = np.column_stack([(u - CAM[2]) / CAM[0] * d, (v - CAM[3]) / CAM[1] * d, d])
    stereo = rng.random(n) < 0.5
    r = rng.uniform(-2, 2, (n, 3))
    obs = np.zeros((n, 7))
    obs[:, 0] = u + r[:, 0]; obs[:, 1] = v + r[:, 1]; obs[:, 2] = np.where(stereo, u - CAM[4] / d + r[:, 2], -1.0)
    obs[:, 3] = 1.2 ** (-2.0 * rng.integers(0, 8, n)); obs[:, 4:] = (pc - t) @ R
    return np.concatenate([q, t]), obs, np.ones(n, np.uint8)


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def session(flag, frames):
    from lpslam_amd import manager, synth
    W, H = 640, 480
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    for num in (0, 1):
        c = manager.default_camera()
        c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
        c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
        m.set_camera(c)
    assert m.add_tracker("VSLAMStereo", '{"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 4, "asyncMapping": false%s}' % flag)
    m.collect_results(); m.provide_odometry(); m.start()
    for i, (l, r) in enumerate(frames):
        assert m.add_stereo((i + 1) * 40_000_000, l, r)
    t0 = time.time()
    while len(m.results) < len(frames) and time.time() - t0 < 60:
        time.sleep(0.01)
    m.stop()
    s = m.tracker_statistics()
    return {k: s[k] for k in ("frames", "pose_fits", "pose_sigmas", "pose_sigma_refused", "ms_dev_pose", "ms_dev_pose_sigma", "ms_per_frame")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21); ap.add_argument("--manager", action="store_true"); ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cov_time"))
    a = ap.parse_args()
    from lpslam_amd import _build, hip
    _build.hip_library(); _build.host_library()
    ctx = hip.Context(320, 240, 400, 1.2, 4, max_images=1)
    cam = dict(fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], fxb=CAM[4])
    res = {"reps": a.reps, "sizes": {}}
    lines = ["pose covariance, S = 1: median (min .. max) ms of %d calls after 3 warm-up calls" % a.reps,
             "%6s %28s %28s %28s" % ("n", "device call", "host form, one thread", "lpslam_hip_pose_optimize")]
    for n in (20, 100, 500, 2000):
        pose, obs, active = make_set(n, 5)
        start = [0, n]
        bo = np.zeros(n, hip.BA_OBS_DTYPE)
        bo["point"] = np.arange(n); bo["u"] = obs[:, 0]; bo["v"] = obs[:, 1]; bo["ur"] = obs[:, 2]; bo["inv_sigma2"] = obs[:, 3]
        pts = np.ascontiguousarray(obs[:, 4:])
        d = hip.pose_covariance_batch(ctx, start, pose, obs, active, CAM); h = hip.pose_covariance_batch_host(start, pose, obs, active, CAM)
        assert all(d[k].tobytes() == h[k].tobytes() for k in d), "device and host differ at n = %d" % n
        t_dev = median_ms(lambda: hip.pose_covariance_batch(ctx, start, pose, obs, active, CAM), a.reps)
        t_host = median_ms(lambda: hip.pose_covariance_batch_host(start, pose, obs, active, CAM), a.reps)
        t_opt = median_ms(lambda: hip.pose_optimize(ctx, pose, pts, bo, cam), a.reps)
        res["sizes"][str(n)] = {"device_ms": t_dev, "host_ms": t_host, "pose_optimize_ms": t_opt, "status": int(d["status"][0]), "n_used": int(d["n_used"][0])}
        fmt = lambda t: "%8.4f (%7.4f .. %7.4f)" % t
        lines.append("%6d %28s %28s %28s" % (n, fmt(t_dev), fmt(t_host), fmt(t_opt)))
    if a.manager:
        from lpslam_amd import synth
        seq = synth.StereoSequence(640, 480, 4, n_points=6000)
        frames = [seq.frame(i) for i in range(24)]
        res["sessions"] = {"off": [], "on": []}
        for _ in range(a.sessions):
            res["sessions"]["off"].append(session("", frames)); res["sessions"]["on"].append(session(', "poseSigma": true', frames))
        lines.append("")
        lines.append("stereo session of tests/test_pose_sigma_gpu.py (24 frames), option off / on alternating, %d sessions each:" % a.sessions)
        for name in ("off", "on"):
            for s in res["sessions"][name]:
                lines.append("  %-3s %s" % (name, " ".join("%s=%s" % kv for kv in s.items())))
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
