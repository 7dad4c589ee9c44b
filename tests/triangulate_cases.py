"""Planted inputs of the triangulation tests, shared by the CPU and the GPU tests: pairs that reach every code and
every rejection of tri_pair, and keypoint sets for the candidate gate with the planted edge cases (ties, more than eight passing
candidates, keypoints at the epipole, groups with negatives).  The reference's answers are computed once per process."""
import functools
import math

import numpy as np

import triangulate_ref as tr

SCALE = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)      # the pyramid's scale table, 8 levels
CAM_MONO = tr.Cam(500.0, 505.0, 320.0, 240.0, 0.0, 1.2)
CAM_STEREO = tr.Cam(500.0, 505.0, 320.0, 240.0, 500.0 * 0.12, 1.2)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
ORIGIN = tr.look_pose([0, 0, 0])


def _kp(cam, pose, Xw, octave, stereo, dy=0.0, dxr=0.0, depth_factor=1.0):
    """keypoints of world points in a view; stereo: depth and right-image column; dy / dxr: planted offsets in pixels; depth_factor
    scales the stereo depth (x_right follows it)"""
    u, v, z = tr.project(cam, pose, Xw)
    k = np.zeros(len(u), tr.TRI_KP)
    k["x"] = u; k["y"] = v + dy; k["octave"] = octave
    stereo = np.broadcast_to(stereo, u.shape)
    d = np.where(stereo, z * depth_factor, -1.0)
    k["depth"] = d
    k["x_right"] = np.where(stereo, k["x"].astype(np.float64) - cam.fxb / np.where(stereo, d, 1.0) + dxr, -1.0)
    return k


def _points(rng, n, z_lo, z_hi, spread=0.35):
    z = rng.uniform(z_lo, z_hi, n)
    return np.stack([rng.uniform(-spread, spread, n) * z, rng.uniform(-spread * 0.7, spread * 0.7, n) * z, z], 1)


@functools.lru_cache(maxsize=None)
def planted_pairs():
    """-> list of groups {name, cam, pose1, pose2, k1, k2}; about 2000 pairs"""
    rng = np.random.default_rng(31)
    G = []

    def add(name, cam, pose1, pose2, k1, k2):
        G.append({"name": name, "cam": cam, "pose1": pose1, "pose2": pose2, "k1": k1, "k2": k2})

    n = 100
    side = tr.look_pose([1.0, 0.1, 0.2], yaw=-0.05, pitch=0.02)
    # monocular, good parallax: triangulated; equal octaves agree with nearly equal distances
    X = _points(rng, n, 3, 12); o = rng.integers(0, 7, n)
    add("mono_ok", CAM_MONO, ORIGIN, side, _kp(CAM_MONO, ORIGIN, X, o, False), _kp(CAM_MONO, side, X, o, False))
    # the same with a third of a pixel of noise
    add("mono_noise", CAM_MONO, ORIGIN, side, _kp(CAM_MONO, ORIGIN, X, o, False, dy=rng.uniform(-0.3, 0.3, n)), _kp(CAM_MONO, side, X, o, False, dy=rng.uniform(-0.3, 0.3, n)))
    # far points: no parallax, no stereo keypoint to fall back on
    Xf = _points(rng, n, 200, 600)
    add("mono_far", CAM_MONO, ORIGIN, side, _kp(CAM_MONO, ORIGIN, Xf, 1, False), _kp(CAM_MONO, side, Xf, 1, False))
    # a keypoint 12 scaled pixels off the epipolar line: both views miss, the first is reported
    s = SCALE[o].astype(np.float64)
    add("mono_reproj1", CAM_MONO, ORIGIN, side, _kp(CAM_MONO, ORIGIN, X, o, False), _kp(CAM_MONO, side, X, o, False, dy=12.0 * s))
    # 7 pixels off with a coarse octave in view 1 and the finest in view 2: view 1 accepts its half, view 2 does not
    add("mono_reproj2", CAM_MONO, ORIGIN, side, _kp(CAM_MONO, ORIGIN, X, 4, False), _kp(CAM_MONO, side, X, 0, False, dy=7.0))
    # points behind one of the cameras
    ahead = tr.look_pose([0.3, 0.1, 10.0])
    Xm = _points(rng, n, 3, 7)
    add("depth2", CAM_MONO, ORIGIN, ahead, _kp(CAM_MONO, ORIGIN, Xm, 2, False), _kp(CAM_MONO, ahead, Xm, 2, False))
    add("depth1", CAM_MONO, ahead, ORIGIN, _kp(CAM_MONO, ahead, Xm, 2, False), _kp(CAM_MONO, ORIGIN, Xm, 2, False))
    # cameras that face each other: the rays' cosine is negative
    facing = tr.look_pose([0.2, 0.0, 10.0], yaw=math.pi)
    add("cos_neg", CAM_MONO, ORIGIN, facing, _kp(CAM_MONO, ORIGIN, Xm, 2, False), _kp(CAM_MONO, facing, Xm, 2, False))
    # distances 3 : 9 with equal octaves, both ways round, and with octaves that explain them
    back = tr.look_pose([2.0, 0.0, -6.0])
    Xn = _points(rng, n, 2.5, 3.5, 0.2)
    add("ratio_low", CAM_MONO, ORIGIN, back, _kp(CAM_MONO, ORIGIN, Xn, 3, False), _kp(CAM_MONO, back, Xn, 3, False))
    add("ratio_high", CAM_MONO, back, ORIGIN, _kp(CAM_MONO, back, Xn, 3, False), _kp(CAM_MONO, ORIGIN, Xn, 3, False))
    add("ratio_explained", CAM_MONO, ORIGIN, back, _kp(CAM_MONO, ORIGIN, Xn, 5, False), _kp(CAM_MONO, back, Xn, 0, False))
    # stereo keypoints with parallax beyond their stereo angle: triangulated under the three-term bound
    Xs = _points(rng, n, 4, 40); os_ = rng.integers(0, 6, n)
    add("st_tri", CAM_STEREO, ORIGIN, side, _kp(CAM_STEREO, ORIGIN, Xs, os_, True), _kp(CAM_STEREO, side, Xs, os_, True))
    add("st_reproj1", CAM_STEREO, ORIGIN, side, _kp(CAM_STEREO, ORIGIN, Xs, 0, True, dxr=6.0), _kp(CAM_STEREO, side, Xs, 0, True))
    add("st_reproj2", CAM_STEREO, ORIGIN, side, _kp(CAM_STEREO, ORIGIN, Xs, 0, True), _kp(CAM_STEREO, side, Xs, 0, True, dxr=-6.0))
    # one stereo keypoint is enough to triangulate below the monocular parallax bound's reach
    add("st_mixed_tri", CAM_STEREO, ORIGIN, side, _kp(CAM_STEREO, ORIGIN, Xs, os_, True), _kp(CAM_STEREO, side, Xs, os_, False))
    # cameras 4 cm apart: the rays are closer than the stereo angle, the keypoint with the smaller depth is back-projected
    Xb = _points(rng, n, 4, 10)
    near_b = tr.look_pose([0.04, 0.0, 0.01]); near_f = tr.look_pose([0.04, 0.0, -0.01])
    add("st_back3", CAM_STEREO, ORIGIN, near_b, _kp(CAM_STEREO, ORIGIN, Xb, 1, True), _kp(CAM_STEREO, near_b, Xb, 1, True))
    add("st_back2", CAM_STEREO, ORIGIN, near_f, _kp(CAM_STEREO, ORIGIN, Xb, 1, True), _kp(CAM_STEREO, near_f, Xb, 1, True))
    add("st_only1", CAM_STEREO, ORIGIN, near_b, _kp(CAM_STEREO, ORIGIN, Xb, 1, True), _kp(CAM_STEREO, near_b, Xb, 1, False))
    add("st_only2", CAM_STEREO, ORIGIN, near_b, _kp(CAM_STEREO, ORIGIN, Xb, 1, False), _kp(CAM_STEREO, near_b, Xb, 1, True))
    # a back-projection at 0.4 of the depth (its own right-image column agrees with it): the other view rejects it
    near_s = tr.look_pose([0.1, 0.0, 0.0])
    add("st_back_reproj2", CAM_STEREO, ORIGIN, near_s, _kp(CAM_STEREO, ORIGIN, Xb, 0, True, depth_factor=0.4), _kp(CAM_STEREO, near_s, Xb, 0, False))
    return G


@functools.lru_cache(maxsize=None)
def pair_reference():
    """per group: the reference's results (SVD) of every pair, and per code-1 pair the Jacobi restatement's X"""
    out = []
    for g in planted_pairs():
        svd = [tr.tri_pair(g["cam"], SCALE, g["pose1"], g["pose2"], a, b) for a, b in zip(g["k1"], g["k2"])]
        jac = [tr.tri_pair(g["cam"], SCALE, g["pose1"], g["pose2"], a, b, linear=tr.linear_jacobi) if r["code"] == 1 else None for a, b, r in zip(g["k1"], g["k2"], svd)]
        out.append({"svd": svd, "jacobi": jac})
    return out


def svd_jacobi_deviation():
    """the largest relative distance |X_svd - X_jacobi| / |X_svd| over the planted code-1 pairs, and how many there are"""
    worst, n = 0.0, 0
    for r in pair_reference():
        for a, b in zip(r["svd"], r["jacobi"]):
            if b is None:
                continue
            assert b["code"] == 1, (a["reason"], b["reason"])
            worst = max(worst, float(np.linalg.norm(a["X"] - b["X"]) / np.linalg.norm(a["X"]))); n += 1
    return worst, n


def to_slot_keypoints(k):
    kp = np.zeros(len(k), KP_DTYPE)
    kp["x"] = k["x"]; kp["y"] = k["y"]; kp["octave"] = k["octave"]; kp["size"] = 31.0; kp["angle"] = 0.0; kp["response"] = 50.0; kp["class_id"] = -1
    return kp


def to_tri_keypoints(kp, x_right=None, depth=None):
    k = np.zeros(len(kp), tr.TRI_KP)
    k["x"] = kp["x"]; k["y"] = kp["y"]; k["octave"] = kp["octave"]
    k["x_right"] = -1.0 if x_right is None else x_right; k["depth"] = -1.0 if depth is None else depth
    return k


def _flip(rng, desc, bits):
    d = np.unpackbits(desc.copy())
    d[rng.choice(256, bits, replace=False)] ^= 1
    return np.packbits(d)


def neighbour_pose(s):
    """neighbour s of the planted sets: mostly forward motion, so that the epipole lies inside the image"""
    return tr.look_pose([0.25 * math.cos(1.7 * s), 0.15 * math.sin(1.3 * s), 0.7 + 0.1 * (s % 3)], yaw=0.02 * ((s % 5) - 2), pitch=0.01 * ((s % 3) - 1))


@functools.lru_cache(maxsize=None)
def planted_sets(n1, n2, n_sets, groups="zero", seed=5, target_stereo=False, degenerate=(), no_epipole=()):
    """-> (cam, query dict {kp, desc, group}, [set dicts {kp, desc, group, depth, x_right, pose, F, epipole}]).  groups: "zero" (every
    participant 0) or "vocab" (node-like ids with negatives).  target_stereo: the sets' keypoints carry a depth, which switches the
    epipole rule off.  degenerate: sets whose F maps every query to a line with l0 = l1 = 0; no_epipole: sets with has_epipole = 0."""
    rng = np.random.default_rng(seed + 1000 * n1 + 10 * n2 + n_sets)
    cam = CAM_STEREO if target_stereo else CAM_MONO
    m = min(n1, n2 if n2 < 32 else n2 - 24)              # partners; a larger set keeps 24 keypoints for the planted copies
    X = _points(rng, max(n1, 1), 4, 15, 0.25)              # world points seen by every view
    q = {"kp": np.zeros(n1, KP_DTYPE), "desc": rng.integers(0, 256, (n1, 32), dtype=np.uint8)}
    u, v, _ = tr.project(cam, ORIGIN, X[:n1])
    q["kp"]["x"] = u; q["kp"]["y"] = v; q["kp"]["octave"] = rng.integers(0, 3, n1); q["kp"]["angle"] = rng.uniform(0, 360, n1); q["kp"]["size"] = 31.0; q["kp"]["class_id"] = -1
    node = rng.integers(0, 7, max(n1, 1)).astype(np.int32)[:n1]
    q["group"] = np.zeros(n1, np.int32) if groups == "zero" else np.where(rng.random(n1) < 0.15, -1, node).astype(np.int32)
    sets = []
    for s in range(n_sets):
        pose = neighbour_pose(s)
        F, ep = tr.epipolar(cam, ORIGIN, pose)
        true_ep = ep
        if s in degenerate:
            F = np.zeros((3, 3)); F[2, 2] = 1.0
        if s in no_epipole:
            ep = None
        kp = np.zeros(n2, KP_DTYPE); desc = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        kp["x"] = rng.uniform(0, 640, n2); kp["y"] = rng.uniform(0, 480, n2); kp["octave"] = rng.integers(0, 3, n2); kp["angle"] = rng.uniform(0, 360, n2); kp["size"] = 31.0; kp["class_id"] = -1
        grp = np.zeros(n2, np.int32) if groups == "zero" else np.where(rng.random(n2) < 0.15, -1, rng.integers(0, 7, n2)).astype(np.int32)
        depth = np.full(n2, -1.0, np.float32)
        perm = rng.permutation(n2)[:m]                    # target perm[i] is the partner of query i
        if m:
            pu, pv, pz = tr.project(cam, pose, X[:m])
            kp["x"][perm] = pu + rng.uniform(-0.4, 0.4, m); kp["y"][perm] = pv + rng.uniform(-0.4, 0.4, m)
            for i in range(m):
                desc[perm[i]] = _flip(rng, q["desc"][i], int(rng.integers(0, 45)) if rng.random() > 0.1 else 70)
            if groups != "zero":
                grp[perm] = np.where(rng.random(m) < 0.1, -1, node[:m])
            if target_stereo:
                depth[perm] = np.where(rng.random(m) < 0.7, pz, -1.0)
        free = np.setdiff1d(np.arange(n2), perm)
        # ties: two more copies of a partner, descriptor and all; more than eight: twelve near copies of query 0's partner
        plan = [(1, 2, 0)] * 3 + [(0, 12, 1)] if m >= 8 else []
        at = 0
        if m >= 8:
            desc[perm[0]] = _flip(rng, q["desc"][0], 5)
        for qi_off, copies, spread_bits in plan:
            if at + copies > len(free):
                break
            i = int(rng.integers(1, m)) if qi_off else 0
            for c_ in range(copies):
                t = free[at]; at += 1
                kp[t] = kp[perm[i]]; desc[t] = _flip(rng, desc[perm[i]], c_ % 4) if spread_bits else desc[perm[i]]
                grp[t] = grp[perm[i]]; depth[t] = depth[perm[i]]
        # every epipolar line passes through the epipole: three keypoints next to it that copy a query's descriptor pass every rule but the third
        for _ in range(3):
            if at >= len(free) or n1 == 0 or true_ep is None:
                break
            t = free[at]; at += 1
            i = int(rng.integers(0, n1))
            kp["x"][t] = true_ep[0] + rng.uniform(-3, 3); kp["y"][t] = true_ep[1] + rng.uniform(-3, 3); kp["octave"][t] = 0
            desc[t] = q["desc"][i]; grp[t] = q["group"][i]
            if target_stereo:
                depth[t] = 8.0 if _ == 0 else -1.0
        xr = np.where(depth > 0, kp["x"] - np.float32(cam.fxb) / np.where(depth > 0, depth, 1), -1.0).astype(np.float32)
        sets.append({"kpts": kp, "desc": desc, "group": grp, "depth": depth if target_stereo else None, "x_right": xr if target_stereo else None,
                     "pose": pose, "F": F, "epipole": ep})
    return cam, q, sets


def reference_lists(cam, q, sets, q_depth=None):
    """(j, dist, count) per set by the reference"""
    return [tr.candidates(cam, SCALE, q["kp"], q["desc"], q["group"], q_depth, s["kpts"], s["desc"], s["group"], s["depth"], s["F"], s["epipole"]) for s in sets]
