"""The pair sets of the batched Sim3 RANSAC tests (tests/test_sim3_batch_cpu.py, test_sim3_ransac_gpu.py, test_sim3_verify_gpu.py): planted
similarities with a known share of wrong matches, the edge sets (two pairs, none, all pairs on one point) and the single-set host solver
through its C shim.  Every set is a SIM3_PAIR_DTYPE array, the input format of the optimiser and of the batch calls."""
import ctypes as C

import numpy as np

from lpslam_amd import hip

CAM = np.array([520.0, 515.0, 318.5, 243.25])
SEEDS = (0, 0x9E3779B9)


def _rot(v):
    a = float(np.linalg.norm(v))
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def planted(n, case, outliers=0.0, scale=1.0, noise=0.4):
    """exactly n pairs under x1 = scale R x2 + t; the first round(outliers * n) keypoints of image 1 are moved 40 .. 80 px away (wrong
    matches, at fixed places so that the planted inliers are n minus that number); pixel noise `noise` times the level's scale"""
    rng = np.random.default_rng(1000 + case)
    R = _rot(rng.normal(0, 0.12, 3) + 1e-3); t = rng.normal(0, 0.4, 3)
    p2 = np.stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), rng.uniform(5, 20, n)], 1)
    p1 = scale * (p2 @ R.T) + t
    lv1, lv2 = rng.integers(0, 4, n), rng.integers(0, 4, n)
    s1, s2 = 1.2 ** lv1, 1.2 ** lv2
    proj = lambda p: np.stack([CAM[0] * p[:, 0] / p[:, 2] + CAM[2], CAM[1] * p[:, 1] / p[:, 2] + CAM[3]], 1)
    o1 = proj(p1) + noise * rng.normal(0, 1, (n, 2)) * s1[:, None]
    o2 = proj(p2) + noise * rng.normal(0, 1, (n, 2)) * s2[:, None]
    n_bad = int(round(outliers * n))
    ang = rng.uniform(0, 2 * np.pi, n_bad); far = rng.uniform(40, 80, n_bad)
    o1[:n_bad] += np.stack([far * np.cos(ang), far * np.sin(ang)], 1)
    out = np.zeros(n, hip.SIM3_PAIR_DTYPE)
    out["p1c"] = p1 + (rng.normal(0, 0.004, p1.shape) if noise else 0.0); out["p2c"] = p2
    out["obs1"] = o1; out["obs2"] = o2; out["inv_sigma2_1"] = 1.0 / s1 ** 2; out["inv_sigma2_2"] = 1.0 / s2 ** 2
    return out, n - n_bad


def coincident(n=8):
    """n times the same pair: centred, every sample is the zero matrix -- with a free scale Horn finds no positive scale and refuses it.
    (Coordinates in 64ths: three times such a number is exact, so the mean of three equal points is the point itself.)"""
    one, _ = planted(1, 77)
    one["p1c"] = np.floor(one["p1c"] * 64) / 64; one["p2c"] = np.floor(one["p2c"] * 64) / 64
    return np.repeat(one, n)


def edge_batch():
    """S = 9 for the GPU test and the CPU batch test: n = 0, 2, 3, 4, 64, 65 and 300 (60 % wrong matches), the coincident set; the ninth
    set is one more planted one (the batch is also run from pair_start[0] > 0).  (sets, planted inliers or None where nothing is planted)"""
    sets, want = [], []
    for case, (n, bad) in enumerate(((0, 0), (2, 0), (3, 0), (4, 0), (64, 0.25), (65, 0.25), (300, 0.6))):
        p, good = planted(n, 20 + case, bad)
        sets.append(p); want.append(good if n >= 20 else None)
    sets.append(coincident()); want.append(None)
    p, good = planted(37, 40, 0.3)
    sets.append(p); want.append(good)
    return sets, want


def tracker_batch():
    """S = 3, the tracker's shape: 20, 63 and 257 pairs"""
    out = [planted(n, 50 + i, bad) for i, (n, bad) in enumerate(((20, 0.2), (63, 0.3), (257, 0.3)))]
    return [p for p, _ in out], [g for _, g in out]


def exact6(case):
    """six exact pairs (no noise): every sample reproduces the similarity, many iterations reach the same count"""
    return planted(6, 300 + case, 0.0, noise=0.0)[0]


def solve_single(pairs, fix_scale, iterations, seed, cam1=CAM, cam2=CAM):
    """lpslam_sim3_solve_ransac on one set: (count, s12 as left by the solver from zeros, flags as left from zeros)"""
    f = hip.host_lib().lpslam_sim3_solve_ransac
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    n = len(pairs)
    a = [np.ascontiguousarray(pairs[k], np.float64) for k in ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")]
    s12 = np.zeros(8); inl = np.zeros(max(n, 1), np.uint8)
    c1 = np.ascontiguousarray(cam1, np.float64); c2 = np.ascontiguousarray(cam2, np.float64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    got = f(*[p(x) for x in a], n, p(c1), p(c2), int(fix_scale), int(iterations), int(seed) & 0xffffffff, p(s12), p(inl))
    return got, s12, inl[:n]


def transform_cases():
    """The calls of lpslam_hip_sim3_transform_optimize that tests/test_sim3_gpu.py makes (its batch of four at both scale settings, the
    set of mostly wrong matches beside one of six pairs, the empty set): (name, s12, pair arrays, cam1, cam2, fix_scale).  Their results
    at the commit before the optimiser's kernel body became a function of its own are tests/golden/sim3_transform_bytes.npz."""
    from lpslam_amd import synth
    out = []
    for scale, fix_scale in ((1.0, True), (1.15, False)):
        probs = [synth.sim3_pair_problem(n, sid, scale=scale, init_noise=(0.02, 0.15, 0.0 if fix_scale else 0.03)) for sid, n in enumerate((150, 40, 300, 700))]
        out.append(("batch_fix%d" % fix_scale, np.array([p["s12"] for p in probs]), [hip.sim3_pairs(p) for p in probs], probs[0]["cam1"], probs[0]["cam2"], fix_scale))
    p = synth.sim3_pair_problem(30, 9, outlier_frac=0.8); few = synth.sim3_pair_problem(6, 10)
    out.append(("rejects", np.array([p["s12"], few["s12"]]), [hip.sim3_pairs(p), hip.sim3_pairs(few)], p["cam1"], p["cam2"], True))
    out.append(("empty", np.array([p["s12"]]), [hip.sim3_pairs(p)[:0]], p["cam1"], p["cam2"], True))
    return out


NONE_S12 = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])


def same(a, b):
    """two results of a RANSAC batch call, byte for byte"""
    if not (np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()):
        return False
    if (a[3] is None) != (b[3] is None) or (a[3] is not None and not np.array_equal(a[3], b[3])):
        return False
    return len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
