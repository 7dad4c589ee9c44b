"""Seeded match sets for the two-view initialiser's batch tests (tests/test_two_view_batch_cpu.py, tests/test_two_view_gpu.py): a set
is a dict p1, p2 (n, 2) float64 pixels in the reference / current image -- values a float32 keypoint holds exactly, so that
two_view_initialize (float32 keypoints) and the batch calls (float64 matches) see the same numbers -- and the planted motion."""
import numpy as np

K = np.array([525.0, 525.0, 320.0, 240.0])
SEED = 0x9E3779B9          # the tracker's (TwoViewParams::seed)


def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx


def _project(x):
    return np.column_stack([K[0] * x[:, 0] / x[:, 2] + K[2], K[1] * x[:, 1] / x[:, 2] + K[3]])


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float64))


def scene(n, seed=0, planar=False, r=None, t=None, noise=0.3, outliers=0.0, slope=(0.25, -0.1)):
    """points 4 .. 9 m in front of the reference camera (or on a tilted plane), seen again after the motion (r, t); gaussian pixel
    noise; a share of the matches replaced by uniformly random current keypoints (`bad`)"""
    rng = np.random.default_rng(seed)
    r = rot([0.1, 1.0, 0.2], 0.06) if r is None else r
    t = np.array([-0.4, 0.05, 0.1]) if t is None else np.asarray(t, float)
    x = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)])
    if planar:
        x[:, 2] = 6.0 + slope[0] * x[:, 0] + slope[1] * x[:, 1]
    p1 = _project(x) + rng.normal(0, noise, (n, 2))
    p2 = _project(x @ r.T + t) + rng.normal(0, noise, (n, 2))
    bad = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        bad[rng.choice(n, k, replace=False)] = True
        p2[bad] = np.column_stack([rng.uniform(0, 640, k), rng.uniform(0, 480, k)])
    return dict(p1=_f32(p1), p2=_f32(p2), bad=bad, R=r, t=t, x=x)


def general(n=300, seed=2, outliers=0.0):
    """depth variation and a baseline: the fundamental matrix wins"""
    return scene(n, seed, outliers=outliers)


def planar(n=300, seed=21):
    """a strongly tilted plane under a motion for which one of Faugeras' solutions is the clear winner (tests/test_two_view_cpu.py): the homography wins"""
    return scene(n, seed, planar=True, r=rot([0.1, 1.0, 0.2], 0.14), t=[-0.6, -0.34, 0.14], slope=(1.16, -0.82))


def rotation(n=300, seed=4):
    """no baseline at all: the homography wins and no hypothesis has parallax"""
    return scene(n, seed, r=rot([0.2, 1.0, -0.1], 0.08), t=[0.0, 0.0, 0.0])


def one_point(n=20):
    """every match on one point: the mean deviations are 0, the normalisation is not finite"""
    return dict(p1=np.tile([[100.0, 120.0]], (n, 1)), p2=np.tile([[130.0, 90.0]], (n, 1)), bad=np.zeros(n, bool))


def collinear8():
    """eight matches on one line in both images"""
    s = np.arange(8, dtype=float)
    return dict(p1=_f32(np.column_stack([50 + 60 * s, 40 + 45 * s])), p2=_f32(np.column_stack([70 + 58 * s, 55 + 44 * s])), bad=np.zeros(8, bool))


def first(s, n):
    """the first n matches of a set"""
    return {k: (v[:n] if k in ("p1", "p2", "bad", "x") else v) for k, v in s.items()}


def concat(sets):
    """offsets (S + 1), p1, p2 of the sets one after the other"""
    off = np.zeros(len(sets) + 1, np.int32)
    off[1:] = np.cumsum([len(s["p1"]) for s in sets])
    cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(s[k], float).reshape(-1, 2) for s in sets], 0)) if sets else np.zeros((0, 2))
    return off, cat("p1"), cat("p2")


def as_keypoints(s, seed=0):
    """the set as two_view_initialize takes it: kp_ref, kp_cur (float32; the current frame lists its keypoints in another order), matches"""
    n = len(s["p1"])
    perm = np.random.default_rng(seed).permutation(n)
    kp_cur = np.zeros((n, 2), np.float32); kp_cur[perm] = s["p2"]
    return np.ascontiguousarray(s["p1"], np.float32), kp_cur, np.ascontiguousarray(np.column_stack([np.arange(n), perm]), np.int32)


def batches():
    """name -> list of sets: S = 1; S = 8 with the sizes at a wave's edges, 60 % gross outliers; S = 11 with n = 0, n = 7, the one-point
    set, the collinear eight, the planar and the rotation scene, and 1024 matches"""
    return {
        "S1": [general(300, 2, 0.3)],
        "S8": [scene(n, 10 + i, outliers=0.6) for i, n in enumerate((8, 9, 15, 63, 64, 65, 129, 300))],
        "S11": [general(37, 3), first(general(37, 5), 0), general(65, 6, 0.3), first(general(37, 7), 7), one_point(20), collinear8(), planar(300), rotation(129),
                general(64, 8), general(9, 9), general(1024, 11, 0.3)],
    }
