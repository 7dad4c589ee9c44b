#!/usr/bin/env python3
"""Times the relocaliser's pose solver for a Lost frame's candidates: 8 sets of 50, 200 and 1000 planted
matches (30 % outliers), 100 iterations, the tracker's seed.
Host: LpSlam::pnp_solve_ransac on each set, one thread (lpslam_pnp_ransac_batch_host) -- what the tracker does with
relocaliseOnDevice off.  Device: lpslam_hip_pnp_ransac_batch end to end -- host arrays in, pose7 and flags out, with the sample
table, the upload, the wait and the host refits.  Both are the median wall clock of --reps calls after a warm-up, in the same run;
the results of both must be equal.  --manager adds the time per Lost frame of a localisation-only session on a saved map with the
tracker option off and on (ms_reloc_frame of the tracker statistics).  The kernel split comes from a separate run under rocprofv3
--kernel-trace --stats.

usage: time_pnp.py [--reps N] [--manager] [--out STEM]      (writes STEM.json and STEM.txt)"""
import argparse, ctypes as C, json, os, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAM = np.array([525.0, 525.0, 320.0, 240.0])


def planted(n, share, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3); a /= np.linalg.norm(a); ang = rng.uniform(0.2, 1.0)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
    t = rng.normal(0, 1.0, 3)
    z = rng.uniform(2.0, 10.0, n)
    xc = np.column_stack([(rng.uniform(20, 620, n) - CAM[2]) / CAM[0] * z, (rng.uniform(20, 460, n) - CAM[3]) / CAM[1] * z, z])
    pw = (xc - t) @ R
    obs = np.column_stack([CAM[0] * xc[:, 0] / z + CAM[2], CAM[1] * xc[:, 1] / z + CAM[3]]) + rng.uniform(-0.3, 0.3, (n, 2))
    k = int(round(share * n))
    bad = rng.choice(n, k, replace=False)
    d = rng.uniform(0, 2 * np.pi, k)
    obs[bad] += np.column_stack([np.cos(d), np.sin(d)]) * rng.uniform(30.0, 120.0, (k, 1))
    return pw, obs, 1.0 / (1.2 ** rng.integers(0, 4, n)) ** 2


def lost_frame_ms(on):
    """ms per Lost frame of a localisation-only stereo session on a saved map (the session of tests/test_reloc_device_gpu.py)"""
    from lpslam_amd import manager, synth
    W, H = 640, 480
    cfg = '"cameraSetup": "stereo", "slamKeypoints": 1000, "numLevels": 4, "keyframeInterval": 3, "localWindow": 4'
    d = tempfile.mkdtemp(prefix="pnp_time_")
    path = os.path.join(d, "place.lpsmap")

    def run(extra, frames, log):
        k = synth.intrinsics(W, H)
        m = manager.Manager()
        for num in (0, 1):
            c = manager.default_camera()
            c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
            c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
            m.set_camera(c)
        assert m.add_tracker("VSLAMStereo", "{" + cfg + ', "mapFilename": "%s"' % path + extra + "}")
        m.collect_results(); m.provide_odometry(); m.log_to_file(log)
        m.start()
        for i, f in enumerate(frames):
            assert m.add_stereo((i + 1) * 40_000_000, f[0], f[1])
        t0 = time.time()
        while len(m.results) < len(frames) and time.time() - t0 < 60:
            time.sleep(0.01)
        m.stop()
        return manager.Manager.statistics(log)
    run("", synth.turning_sequence(W, H, n_frames=120, step_deg=3.0)[0], os.path.join(d, "save.log"))
    # the revisit of the place: Lost until a candidate succeeds
    frames = synth.turning_sequence(W, H, n_frames=45, step_deg=2.0)[0][20:45]
    out = {}
    for name, flag in (("host", "false"), ("device", "true")):
        if name == "device" and not on:
            continue
        s = run(', "enableMapping": false, "relocaliseOnDevice": %s' % flag, frames, os.path.join(d, name + ".log"))
        out[name] = {k: s.get(k) for k in ("reloc_frames", "ms_reloc_frame", "pnp_batches", "relocalised", "lost")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--manager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_time"))
    args = ap.parse_args()
    from lpslam_amd import _build, hip
    _build.host_library()
    ctx = hip.Context(640, 480, max_keypoints=500, num_levels=2)
    out = {"reps": args.reps, "sets": 8, "iterations": 100, "outlier_share": 0.3, "cases": []}
    lines = []
    for n in (50, 200, 1000):
        sets = [planted(n, 0.3, 100 + i) for i in range(8)]
        off = np.arange(9, dtype=np.int32) * n
        pw = np.ascontiguousarray(np.concatenate([s[0] for s in sets])); obs = np.ascontiguousarray(np.concatenate([s[1] for s in sets])); w = np.ascontiguousarray(np.concatenate([s[2] for s in sets]))
        dev = lambda: hip.pnp_ransac_batch(ctx, off, pw, obs, w, CAM, 100, 0x9E3779B9, want_iteration=False)
        host = lambda: hip.pnp_ransac_batch_host(off, pw, obs, w, CAM, 100, 0x9E3779B9, want_iteration=False)
        for _ in range(3):
            a = dev(); b = host()
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "device and host results differ"
        td, th = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); dev(); td.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); host(); th.append(time.perf_counter() - t0)
        res = {"matches_per_set": n, "inliers": [int(v) for v in a[1]], "host_ms_median": float(np.median(th)) * 1e3, "host_ms_min": min(th) * 1e3,
               "device_ms_median": float(np.median(td)) * 1e3, "device_ms_min": min(td) * 1e3}
        res["host_over_device"] = res["host_ms_median"] / res["device_ms_median"]
        out["cases"].append(res)
        lines.append("8 sets x %4d matches, 100 iterations: host %.3f ms, device %.3f ms (median of %d), host / device %.2f" %
                     (n, res["host_ms_median"], res["device_ms_median"], args.reps, res["host_over_device"]))
        print(lines[-1], flush=True)
    ctx.close()
    if args.manager:
        out["lost_frame"] = lost_frame_ms(True)
        for k, v in out["lost_frame"].items():
            lines.append("localisation-only session, relocaliseOnDevice %s: %s" % ("false" if k == "host" else "true", json.dumps(v)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as fh:
        json.dump(out, fh, indent=1)
    with open(args.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
