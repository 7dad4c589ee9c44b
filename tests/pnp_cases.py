"""Planted match sets for the PnP RANSAC tests (tests/test_pnp_cpu.py, tests/test_pnp_gpu.py): landmarks 2 .. 10 m in front of a
known pose, exact projections plus uniform noise of at most 0.3 px, outliers moved by 30 px or more, keypoints of mixed octaves."""
import ctypes as C

import numpy as np

CAM = np.array([525.0, 525.0, 320.0, 240.0])
SEED = 0x9E3779B9          # the tracker's


def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx


def planted(n, outlier_share=0.0, seed=0):
    """dict: pw (n, 3), obs (n, 2), w (n) = 1 / 1.2^(2 octave), bad (n) bool, R, t (world -> camera)"""
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(0.2, 1.0)); t = rng.normal(0, 1.0, 3)
    z = rng.uniform(2.0, 10.0, n)
    u = rng.uniform(20, 620, n); v = rng.uniform(20, 460, n)
    xc = np.column_stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z])
    pw = (xc - t) @ R                                                    # xc = R pw + t
    xr = pw @ R.T + t
    obs = np.column_stack([CAM[0] * xr[:, 0] / xr[:, 2] + CAM[2], CAM[1] * xr[:, 1] / xr[:, 2] + CAM[3]]) + rng.uniform(-0.3, 0.3, (n, 2))
    bad = np.zeros(n, bool)
    k = int(round(outlier_share * n))
    if k:
        bad[rng.choice(n, k, replace=False)] = True
        ang = rng.uniform(0, 2 * np.pi, k)
        obs[bad] += np.column_stack([np.cos(ang), np.sin(ang)]) * rng.uniform(30.0, 120.0, (k, 1))
    w = 1.0 / (1.2 ** rng.integers(0, 4, n)) ** 2
    return dict(pw=np.ascontiguousarray(pw), obs=np.ascontiguousarray(obs), w=w, bad=bad, R=R, t=t)


def coplanar(n, seed=0):
    """every landmark in the world plane z = 1.5 (the centred z are exact zeros): every four of them span no volume"""
    rng = np.random.default_rng(seed)
    pw = np.column_stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), np.full(n, 1.5)])
    R = rot([0.3, 1.0, 0.1], 0.2); t = np.array([0.1, -0.2, 4.0])
    xc = pw @ R.T + t
    obs = np.column_stack([CAM[0] * xc[:, 0] / xc[:, 2] + CAM[2], CAM[1] * xc[:, 1] / xc[:, 2] + CAM[3]])
    return dict(pw=np.ascontiguousarray(pw), obs=np.ascontiguousarray(obs), w=np.ones(n), bad=np.zeros(n, bool), R=R, t=t)


def empty(n):
    """a set of n < 4 matches (any values)"""
    s = planted(max(n, 1), 0.0, 99)
    return {k: (v[:n] if k in ("pw", "obs", "w", "bad") else v) for k, v in s.items()}


def concat(sets):
    """offsets (S + 1), pw, obs, w of the sets one after the other"""
    off = np.zeros(len(sets) + 1, np.int32)
    off[1:] = np.cumsum([len(s["w"]) for s in sets])
    cat = lambda k, width: np.ascontiguousarray(np.concatenate([np.asarray(s[k], float).reshape(-1, width) for s in sets], 0)) if sets else np.zeros((0, width))
    return off, cat("pw", 3), cat("obs", 2), cat("w", 1).reshape(-1)


def solve_one(lib, s, iterations, seed):
    """lpslam_pnp_solve_ransac on one set: count, pose7, flags"""
    f = lib.lpslam_pnp_solve_ransac
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    n = len(s["w"])
    pose = np.zeros(7); pose[0] = 1.0
    inl = np.zeros(max(n, 1), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    got = f(p(s["pw"]), p(s["obs"]), p(np.ascontiguousarray(s["w"])), n, p(CAM), iterations, seed, p(pose), p(inl))
    return got, pose, inl[:n]


def pose_error(pose7, s):
    """(largest difference of R's elements, of t's) between pose7 and the planted pose"""
    w, x, y, z = pose7[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return float(np.abs(R - s["R"]).max()), float(np.abs(pose7[4:] - s["t"]).max())


# (n, outlier share, data seed): the sizes at which the kernels can go wrong -- the minimum, one wave and its edges, several
# rounds of a wave -- chosen so that the HOST solver alone recovers the planted inliers exactly (tests/test_pnp_cpu.py checks that)
SIZES = {
    "n4": (4, 0.0, 0), "n5": (5, 0.0, 0), "n15": (15, 0.0, 0), "n37": (37, 0.3, 0), "n63": (63, 0.3, 0), "n64": (64, 0.3, 0), "n65": (65, 0.3, 0),
    "n257_0": (257, 0.0, 0), "n257_30": (257, 0.3, 0), "n257_60": (257, 0.6, 0), "n2048": (2048, 0.3, 0),
}


def sized(name):
    n, share, seed = SIZES[name]
    return planted(n, share, seed)


def batches():
    """name -> list of sets: S = 1; S = 8 with all sizes different; S = 11 (more than the tracker sends) with n = 0, n = 3 and a
    coplanar set in the middle, and the 2048-match set"""
    return {
        "S1": [sized("n257_30")],
        "S8": [sized(k) for k in ("n4", "n5", "n15", "n63", "n64", "n65", "n257_60", "n37")],
        "S11": [sized("n15"), sized("n63"), empty(0), sized("n257_0"), empty(3), coplanar(40), sized("n64"), sized("n65"), sized("n257_60"), sized("n5"), sized("n2048")],
    }
