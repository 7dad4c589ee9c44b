#!/usr/bin/env python3
"""Times the occupancy-grid build, lpslam_hip_occupancy_build, on two workloads of 2000 scans x 1081 beams (270 degrees, 0.25 degree
steps, 5 cm cells):
  W1  a robot path through the rooms of a 48 x 30 m hall: walls 1 - 25 m away (range_max 25 m, longer beams count as free)
  W2  2000 scans turning in place at one origin of the same hall: every ray passes the origin tile (the contention worst case)
Each timing is the median of wall clocks around the whole call (upload of the poses, four launches, read-back of the grid) after a
warm-up.  Beside it: the plain ray-per-lane kernel with one global atomic per cell visit (tools/dev/occ_atomic_baseline.hip, fed the
same ray records and box; its grid must equal the library's) -- kernel time from events -- and the numpy reference's CPU time on a
200-scan subset, scaled to 2000, for context.  The kernel split comes from a separate run under rocprofv3 --kernel-trace --stats.

usage: time_occupancy.py [--reps N] [--no-ref] [--no-baseline] [--out FILE]"""
import argparse, ctypes as C, json, math, os, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
N_SCANS, N_BEAMS, ANGLE_MIN, INC, RES, RMAX = 2000, 1081, -0.75 * math.pi, 0.25 * math.pi / 180, 0.05, 25.0


def hall():
    """wall segments (map plane): the outline and inner walls with door gaps"""
    w = [((0, 0), (48, 0)), ((48, 0), (48, 30)), ((48, 30), (0, 30)), ((0, 30), (0, 0))]
    for x in (12, 24, 36):
        w += [((x, 0), (x, 12)), ((x, 14), (x, 30))]
    w += [((0, 15), (10, 15)), ((14, 15), (34, 15)), ((38, 15), (48, 15))]
    return np.array(w, np.float64)


def cast(origin, fwd, left, walls, cs):
    d = cs[:, :1] * fwd + cs[:, 1:] * left
    a, e = walls[:, 0], walls[:, 1] - walls[:, 0]
    den = d[:, None, 0] * e[None, :, 1] - d[:, None, 1] * e[None, :, 0]
    ox, oy = a[None, :, 0] - origin[0], a[None, :, 1] - origin[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (ox * e[None, :, 1] - oy * e[None, :, 0]) / den
        u = (ox * d[:, None, 1] - oy * d[:, None, 0]) / den
    t = np.where((np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1), t, np.inf)
    return t.min(axis=1).astype(np.float32)


def workload(kind, hip):
    import occupancy_ref as R
    cs = R.beam_table(N_BEAMS, ANGLE_MIN, INC)
    walls = hall()
    rng = np.random.default_rng(7)
    poses = np.zeros(N_SCANS, hip.SCAN_POSE_DTYPE)
    ranges = []
    for i in range(N_SCANS):
        if kind == "W1":        # a loop through the rooms: along y = 13 (the corridor between the two rows) and back through the rooms
            s = i / N_SCANS
            o = np.array([2 + 44 * (2 * s if s < 0.5 else 2 - 2 * s), 13.0 + (6 * math.sin(12 * math.pi * s) if s >= 0.5 else 0)])
            yaw = 0.0 if s < 0.5 else math.pi
            yaw += 0.3 * math.sin(40 * math.pi * s)
        else:
            o, yaw = np.array([18.0, 7.0]), i * math.radians(0.7)
        fwd = np.array([math.cos(yaw), math.sin(yaw)]); left = np.array([-fwd[1], fwd[0]])
        r = cast(o, fwd, left, walls, cs) + rng.normal(0, 0.01, N_BEAMS).astype(np.float32)
        poses[i]["key"] = i; poses[i]["origin"] = o; poses[i]["fwd"] = fwd; poses[i]["left"] = left
        ranges.append(r)
    return cs, ranges, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lpslam_amd import hip
    import occupancy_ref as R
    base = None
    if not args.no_baseline:
        so = os.path.join(tempfile.mkdtemp(), "occ_base.so")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-w", "-o", so,
                               os.path.join(ROOT, "tools", "dev", "occ_atomic_baseline.hip")])
        base = C.CDLL(so)
        base.occ_atomic_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    ctx = hip.Context(320, 240, 500, 1.2, 3, max_images=2)
    out = {"scans": N_SCANS, "beams": N_BEAMS, "res": RES, "reps": args.reps}
    for kind in ("W1", "W2"):
        cs, ranges, poses = workload(kind, hip)
        gid = ctx.scan_geometry_put(cs)
        for i, r in enumerate(ranges):
            ctx.scan_store_put(i, gid, r, 0.1, RMAX, RMAX)
        grid, info = ctx.occupancy_build(poses, RES, 4096)        # warm-up (buffers grow once)
        buf = np.empty(grid.size, np.int8)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            g, _ = ctx.occupancy_build(poses, RES, 4096, out=buf)
            ts.append(time.perf_counter() - t0)
        assert np.array_equal(g, grid)
        med = float(np.median(ts))
        res = {"grid": [info["width"], info["height"]], "rays": info["rays"], "cell_visits": info["cell_visits"],
               "build_ms_median": med * 1e3, "build_ms_min": min(ts) * 1e3, "rays_per_s": info["rays"] / med, "visits_per_s": info["cell_visits"] / med}
        inv = 1.0 / RES
        if base is not None:
            recs = [R.ray_records(cs, r, 0.1, RMAX, RMAX, p["origin"], p["fwd"], p["left"], inv) for r, p in zip(ranges, poses)]
            rays = np.ascontiguousarray(np.stack([np.concatenate([q[j] for q in recs]) for j in range(4)], 1).astype(np.int32))
            flags = np.ascontiguousarray((np.concatenate([q[4] for q in recs]).astype(np.uint8) | (np.concatenate([q[5] for q in recs]).astype(np.uint8) << 1)))
            bo = np.empty(grid.size, np.int8); kms = np.zeros(args.reps, np.float32)
            rc = base.occ_atomic_build(rays.ctypes.data, flags.ctypes.data, len(flags), info["x0"], info["y0"], info["width"], info["height"],
                                       args.reps, bo.ctypes.data, kms.ctypes.data)
            assert rc == 0
            res["atomic_baseline_kernel_ms_median"] = float(np.median(kms))
            res["atomic_baseline_equal"] = bool(np.array_equal(bo.reshape(grid.shape), grid))
        if not args.no_ref:
            sub = 200
            t0 = time.perf_counter()
            R.build({i: (cs, ranges[i], 0.1, RMAX, RMAX) for i in range(sub)}, [(i, p["origin"], p["fwd"], p["left"]) for i, p in enumerate(poses[:sub])], RES, 4096)
            res["numpy_ref_s_200_scans"] = time.perf_counter() - t0
            res["numpy_ref_s_scaled_2000"] = res["numpy_ref_s_200_scans"] * N_SCANS / sub
        for i in range(N_SCANS):
            ctx.scan_store_drop(i)
        out[kind] = res
        print(kind, json.dumps(res), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
