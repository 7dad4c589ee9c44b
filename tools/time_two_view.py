#!/usr/bin/env python3
"""Times the monocular two-view initialiser: LpSlam::two_view_initialize on 100, 300 and 1000 matches of a
general scene (the fundamental matrix wins) and of a planar scene (the homography wins), 100 iterations, one thread.
Host: the function as the tracker calls it with initialiseOnDevice off, and its split into RANSAC loop, refit with model choice,
decomposition and pose check (the seconds TwoViewSteps collects, with both steps taken from the host forms).  Device: the same function
with steps 1 and 4 taken from lpslam_hip_two_view_ransac_batch / lpslam_hip_two_view_check_poses, end to end -- keypoints and matches
in, the result out, with normalisation, sample table, uploads and waits.  Host and device alternate in one run; each figure is the
median wall clock of --reps calls after 3 warm-ups; the results of both must be equal.  --host-only leaves the device out (the
measurement before any kernel existed).  --parent-lib times lpslam_two_view_initialize of another build of the host library (the parent
commit's) in the same run.  --manager adds ms_init_attempt of a short monocular session with the tracker option off and on (few
samples: one attempt per frame until the map exists).  The kernel split comes from a separate run under rocprofv3 --kernel-trace --stats.

usage: time_two_view.py [--reps N] [--host-only] [--parent-lib PATH] [--manager] [--out STEM]      (writes STEM.json and STEM.txt)"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = np.array([525.0, 525.0, 320.0, 240.0])
OUT_NAMES = ("R", "t", "H", "F", "scores", "par", "model", "inl", "tri", "pts")


def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx


def scene(n, planar, seed):
    """keypoints of both frames (float32) and the matches: 0.3 px noise, 10 % wrong matches"""
    rng = np.random.default_rng(seed)
    r, t = (rot([0.1, 1.0, 0.2], 0.14), np.array([-0.6, -0.34, 0.14])) if planar else (rot([0.1, 1.0, 0.2], 0.06), np.array([-0.4, 0.05, 0.1]))
    x = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)])
    if planar:
        x[:, 2] = 6.0 + 1.16 * x[:, 0] - 0.82 * x[:, 1]
    proj = lambda p: np.column_stack([K[0] * p[:, 0] / p[:, 2] + K[2], K[1] * p[:, 1] / p[:, 2] + K[3]])
    p1 = proj(x) + rng.normal(0, 0.3, (n, 2)); p2 = proj(x @ r.T + t) + rng.normal(0, 0.3, (n, 2))
    bad = rng.choice(n, n // 10, replace=False)
    p2[bad] = np.column_stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))])
    perm = rng.permutation(n)
    kp_cur = np.zeros((n, 2), np.float32); kp_cur[perm] = p2
    return np.ascontiguousarray(p1, np.float32), kp_cur, np.ascontiguousarray(np.column_stack([np.arange(n), perm]), np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Caller:
    """two_view_initialize through one of the C shims: plain (the tracker's host path) or with the steps handed in"""

    def __init__(self, lib, sc, ctx=None, fns=(None, None), plain=False):
        self.kp_ref, self.kp_cur, self.m = sc
        n = len(self.m)
        self.o = dict(R=np.zeros(9), t=np.zeros(3), H=np.zeros(9), F=np.zeros(9), scores=np.zeros(2), par=np.zeros(1), model=np.zeros(1, np.int32),
                      inl=np.zeros(n, np.uint8), tri=np.zeros(n, np.uint8), pts=np.zeros((n, 3)))
        self.calls = np.zeros(2, np.int32); self.seconds = np.zeros(4)
        head = [C.c_void_p] * 4 + [C.c_int, C.c_double, C.c_int, C.c_uint32] + [C.c_void_p] * 10
        if plain:
            self.f = lib.lpslam_two_view_initialize; self.f.argtypes = head; self.pre, self.post = [], []
        else:
            self.f = lib.lpslam_two_view_initialize_with; self.f.argtypes = [C.c_void_p] * 3 + head + [C.c_void_p] * 2
            self.pre, self.post = [ctx, fns[0], fns[1]], [_p(self.calls), _p(self.seconds)]
        self.f.restype = C.c_int

    def __call__(self):
        self.ok = self.f(*self.pre, _p(K), _p(self.kp_ref), _p(self.kp_cur), _p(self.m), len(self.m), 1.0, 100, 0x9E3779B9, *[_p(self.o[k]) for k in OUT_NAMES], *self.post)
        return self.ok

    def bytes(self):
        return bytes([self.ok]) + b"".join(self.o[k].tobytes() for k in OUT_NAMES)


def session(option):
    """the statistics of a six-frame monocular session on the three-wall scene (tests/test_init_device_gpu.py)"""
    from lpslam_amd import manager, synth
    W, H = 640, 480
    walls = synth.WallSequence(W, H, 11)
    k = synth.intrinsics(W, H)
    m = manager.Manager()
    c = manager.default_camera()
    c.camera_number = 0; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]; c.resolution_x = W; c.resolution_y = H
    m.set_camera(c)
    assert m.add_tracker("VSLAMMono", '{"cameraSetup": "monocular", "slamKeypoints": 2000, "numLevels": 3, "keyframeInterval": 4, "localWindow": 10, "asyncMapping": false, "initialiseOnDevice": %s}' % option)
    m.collect_results(); m.provide_odometry()
    m.start()
    for i in range(6):
        assert m.add_image((i + 1) * 40_000_000, walls.frame(i))
    t0 = time.time()
    while len(m.results) < 6 and time.time() - t0 < 60:
        time.sleep(0.01)
    m.stop()
    s = m.tracker_statistics()
    return {k: s.get(k) for k in ("init_attempts", "init_device_calls", "ms_init_attempt", "landmarks")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--manager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_time"))
    args = ap.parse_args()
    from lpslam_amd import _build, hip
    _build.host_library()
    lib = hip.host_lib()
    parent = C.CDLL(args.parent_lib) if args.parent_lib else None
    ctx, fns = None, (None, None)
    if not args.host_only:
        ctx = hip.Context(640, 480, max_keypoints=500, num_levels=2)
        fns = tuple(C.cast(getattr(ctx.lib, name), C.c_void_p) for name in ("lpslam_hip_two_view_ransac_batch", "lpslam_hip_two_view_check_poses"))
    out = {"reps": args.reps, "iterations": 100, "threads": 1, "cases": []}
    lines = []
    med = lambda v: float(np.median(v)) * 1e3
    for planar in (False, True):
        for n in (100, 300, 1000):
            sc = scene(n, planar, 7 + n)
            runs = {"host": Caller(lib, sc, plain=True), "host_steps": Caller(lib, sc)}
            if parent is not None:
                runs["parent"] = Caller(parent, sc, plain=True)
            if ctx is not None:
                runs["device"] = Caller(lib, sc, ctx.h, fns)
            times = {k: [] for k in runs}
            split = {k: [] for k in runs if k in ("host_steps", "device")}
            for rep in range(3 + args.reps):
                for name, r in runs.items():                 # alternating
                    if name in split:
                        r.seconds[:] = 0
                    t0 = time.perf_counter(); r(); dt = time.perf_counter() - t0
                    if rep >= 3:
                        times[name].append(dt)
                        if name in split:
                            split[name].append(r.seconds.copy())
            want = runs["host"].bytes()
            assert all(r.bytes() == want for r in runs.values()), "the results differ"
            if ctx is not None:
                assert runs["device"].calls[1] == 0 and runs["device"].calls[0] >= 1, "a device step failed"
            res = {"scene": "planar" if planar else "general", "matches": n, "ok": int(runs["host"].ok), "model": int(runs["host"].o["model"][0])}
            for name in runs:
                res[name + "_ms_median"] = med(times[name]); res[name + "_ms_min"] = min(times[name]) * 1e3
            for name, v in split.items():
                s = np.median(np.array(v), axis=0) * 1e3
                res[name + "_split_ms"] = dict(ransac=float(s[0]), refit=float(s[1]), decompose=float(s[2]), pose_check=float(s[3]))
            text = "%-7s %4d matches (model %d, ok %d): host %.3f ms" % (res["scene"], n, res["model"], res["ok"], res["host_ms_median"])
            sp = res["host_steps_split_ms"]
            text += " [RANSAC %.3f, refit %.3f, decomposition %.3f, pose check %.3f]" % (sp["ransac"], sp["refit"], sp["decompose"], sp["pose_check"])
            if parent is not None:
                text += ", parent's host %.3f ms" % res["parent_ms_median"]
            if ctx is not None:
                sp = res["device_split_ms"]
                res["host_over_device"] = res["host_ms_median"] / res["device_ms_median"]
                text += ", device %.3f ms [RANSAC %.3f, refit %.3f, decomposition %.3f, pose check %.3f], host / device %.2f" % (
                    res["device_ms_median"], sp["ransac"], sp["refit"], sp["decompose"], sp["pose_check"], res["host_over_device"])
            out["cases"].append(res)
            lines.append(text + " (median of %d)" % args.reps)
            print(lines[-1], flush=True)
    if ctx is not None:
        ctx.close()
    if args.manager:
        out["session"] = {"off": session("false"), "on": session("true")}
        for k, v in out["session"].items():
            lines.append("six-frame monocular session, initialiseOnDevice %s: %s" % ("false" if k == "off" else "true", json.dumps(v)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as fh:
        json.dump(out, fh, indent=1)
    with open(args.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
