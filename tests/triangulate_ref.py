"""numpy FP64 reference of the triangulation step between keyframes, written from the definition and not from
lpslam_amd/csrc/triangulate_math.h: the candidate gate with its eight-nearest lists, the ordered replay, tri_pair with np.linalg.svd
for the linear triangulation -- and a second restatement of that triangulation by cyclic Jacobi on A^T A, whose distance from the SVD
result is what the device's tolerance is derived from.  View 1 is the new keyframe c, view 2 the neighbour n; poses are world ->
camera, qw qx qy qz tx ty tz."""
import math

import numpy as np

LISTED = 8
HAMMING_MAX = 50
TRI_KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("x_right", "<f4"), ("depth", "<f4")])


class Cam:
    def __init__(self, fx, fy, cx, cy, fxb=0.0, scale_factor=1.2):
        self.fx, self.fy, self.cx, self.cy, self.fxb, self.scale_factor = float(fx), float(fy), float(cx), float(cy), float(fxb), float(scale_factor)

    @property
    def baseline(self):
        return self.fxb / self.fx

    def as6(self):
        return np.array([self.fx, self.fy, self.cx, self.cy, self.fxb, self.scale_factor], np.float64)


def view(pose):
    q = np.asarray(pose[:4], np.float64)
    w, x, y, z = q / math.sqrt(float(q @ q))
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)
    return R, np.asarray(pose[4:7], np.float64)


def centre(pose):
    R, t = view(pose)
    return -R.T @ t


def pose_from(R, t):
    """(R, t) -> qw qx qy qz tx ty tz (test construction only)"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s; q[1 + i] = 0.25 * s; q[1 + j] = (R[j, i] + R[i, j]) / s; q[1 + k] = (R[k, i] + R[i, k]) / s
    return np.array(list(q) + list(t), np.float64)


def look_pose(centre_w, yaw=0.0, pitch=0.0, roll=0.0):
    """a camera at centre_w whose optical axis is +z turned by yaw (about y), pitch (about x), roll (about z); returns the pose"""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]); Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    Rwc = Ry @ Rx @ Rz                       # camera -> world
    R = Rwc.T
    return pose_from(R, -R @ np.asarray(centre_w, np.float64))


def epipolar(cam, pose_c, pose_n):
    """F (x_n^T F x_c = 0, pixels), the epipole of c in n (None when c's centre has z = 0 in n's frame)"""
    Rc, tc = view(pose_c); Rn, tn = view(pose_n)
    R = Rn @ Rc.T
    t = tn - R @ tc
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.array([[1 / cam.fx, 0, -cam.cx / cam.fx], [0, 1 / cam.fy, -cam.cy / cam.fy], [0, 0, 1]])
    F = Ki.T @ (tx @ R) @ Ki
    ep = None if t[2] == 0.0 else (cam.fx * t[0] / t[2] + cam.cx, cam.fy * t[1] / t[2] + cam.cy)
    return F, ep


def is_stereo(cam, depth):
    return np.logical_and(cam.fxb > 0.0, np.asarray(depth) > 0)


_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def hamming_matrix(d1, d2):
    """(n1, 32) x (n2, 32) uint8 -> (n1, n2) int32, by bit planes: h = |a| + |b| - 2 a.b"""
    if len(d1) == 0 or len(d2) == 0:
        return np.zeros((len(d1), len(d2)), np.int32)
    a = np.unpackbits(np.ascontiguousarray(d1, np.uint8), axis=1).astype(np.float32); b = np.unpackbits(np.ascontiguousarray(d2, np.uint8), axis=1).astype(np.float32)
    return np.rint(a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)


def candidates(cam, scale, kp1, desc1, group1, depth1, kp2, desc2, group2, depth2, F, ep):
    """kp: structured arrays with x, y, octave; depth1 / depth2: float arrays or None.  Returns j (n1, 8; -1), dist (n1, 8; 256), count (n1,)."""
    n1, n2 = len(kp1), len(kp2)
    out_j = np.full((n1, LISTED), -1, np.int32); out_d = np.full((n1, LISTED), 256, np.int32); count = np.zeros(n1, np.int32)
    if n1 == 0 or n2 == 0:
        return out_j, out_d, count
    F = np.asarray(F, np.float64).reshape(3, 3)
    scale = np.asarray(scale, np.float32).astype(np.float64)
    st1 = is_stereo(cam, depth1) if depth1 is not None else np.zeros(n1, bool)
    st2 = is_stereo(cam, depth2) if depth2 is not None else np.zeros(n2, bool)
    xj = kp2["x"].astype(np.float64); yj = kp2["y"].astype(np.float64); sj = scale[kp2["octave"]]
    H = hamming_matrix(desc1, desc2)
    g1 = np.asarray(group1); g2 = np.asarray(group2)
    if ep is not None:
        dx = xj - float(ep[0]); dy = yj - float(ep[1])
        far = dx * dx + dy * dy >= 100.0 * sj
    for i in range(n1):
        if g1[i] < 0:
            continue
        x, y = float(kp1["x"][i]), float(kp1["y"][i])
        l = [F[k, 0] * x + F[k, 1] * y + F[k, 2] for k in range(3)]
        ok = (g2 >= 0) & (g2 == g1[i]) & (H[i] <= HAMMING_MAX)
        if ep is not None:
            ok &= far | st2 | bool(st1[i])
        nn = l[0] * l[0] + l[1] * l[1]
        if not nn > 0.0:
            continue
        num = l[0] * xj + l[1] * yj + l[2]
        with np.errstate(invalid="ignore"):
            ok &= num * num <= 3.84 * (sj * sj) * nn
        idx = np.flatnonzero(ok)
        count[i] = len(idx)
        order = idx[np.lexsort((idx, H[i, idx]))][:LISTED]
        out_j[i, :len(order)] = order; out_d[i, :len(order)] = H[i, order]
    return out_j, out_d, count


def replay(j, count, n2, skip=None):
    """ordered replay of one neighbour: (match (n1,), rank (n1,), exhausted)"""
    n1 = len(j)
    taken = np.zeros(max(n2, 1), bool)
    match = np.full(n1, -1, np.int32); rank = np.full(n1, -1, np.int32)
    exhausted = 0
    for i in range(n1):
        if (skip is not None and skip[i]) or count[i] <= 0:
            continue
        for r in range(LISTED):
            if j[i, r] < 0:
                break
            if not taken[j[i, r]]:
                taken[j[i, r]] = True; match[i] = j[i, r]; rank[i] = r
                break
        if match[i] < 0 and count[i] > LISTED:
            exhausted += 1
    return match, rank, exhausted


def proj_matrix(cam, pose):
    R, t = view(pose)
    K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1.0]])
    return K @ np.hstack([R, t[:, None]])


def dlt_rows(P1, P2, x1, y1, x2, y2):
    return np.array([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]], np.float64)


def linear_svd(A):
    v = np.linalg.svd(A)[2][3]
    return None if v[3] == 0.0 else v[:3] / v[3]


def linear_jacobi(A):
    """the eigenvector of the smallest eigenvalue of A^T A by cyclic Jacobi (threshold 1e-30 on the off-diagonal share, 64 sweeps)"""
    a = (A.T @ A).tolist()
    n = 4
    v = [[1.0 if r == c else 0.0 for c in range(n)] for r in range(n)]
    for _ in range(64):
        off = sum(a[r][c] ** 2 for r in range(n) for c in range(n) if r != c); diag = sum(a[r][r] ** 2 for r in range(n))
        if off <= 1e-30 * (diag + 1e-300):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if a[p][q] == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1.0)) if theta != 0 else 1.0
                c = 1.0 / math.sqrt(t * t + 1.0); s = t * c
                for k in range(n):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq
                for k in range(n):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk
                for k in range(n):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq
    m = min(range(n), key=lambda c: a[c][c])
    vec = np.array([v[r][m] for r in range(n)])
    return None if vec[3] == 0.0 else vec[:3] / vec[3]


def _rel(a, b):
    """how far a lies from the bound b, relative to the bound (absolute when the bound is 0)"""
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def tri_pair(cam, scale, pose1, pose2, k1, k2, linear=linear_svd):
    """-> dict(code, X, reason, margin, parallax_deg): margin = the smallest relative distance of a tested quantity from its bound"""
    R1, t1 = view(pose1); R2, t2 = view(pose2)
    scale = np.asarray(scale, np.float32).astype(np.float64)
    st1 = bool(is_stereo(cam, k1["depth"])); st2 = bool(is_stereo(cam, k2["depth"]))
    x1, y1, x2, y2 = float(k1["x"]), float(k1["y"]), float(k2["x"]), float(k2["y"])
    r1 = R1.T @ np.array([(x1 - cam.cx) / cam.fx, (y1 - cam.cy) / cam.fy, 1.0]); r2 = R2.T @ np.array([(x2 - cam.cx) / cam.fx, (y2 - cam.cy) / cam.fy, 1.0])
    cos_rays = float(r1 @ r2) / (math.sqrt(float(r1 @ r1)) * math.sqrt(float(r2 @ r2)))
    b = cam.baseline
    cs1 = math.cos(2.0 * math.atan2(b / 2.0, float(k1["depth"]))) if st1 else 2.0
    cs2 = math.cos(2.0 * math.atan2(b / 2.0, float(k2["depth"]))) if st2 else 2.0
    cs = min(cs1, cs2)
    margins = [_rel(cos_rays, cs), abs(cos_rays)]
    if not (st1 or st2):
        margins.append(_rel(cos_rays, 0.9998))
    out = {"code": 0, "X": None, "reason": "", "parallax_deg": math.degrees(math.acos(max(-1.0, min(1.0, cos_rays))))}

    def done(reason, code=0, X=None):
        out.update(code=code, X=X if code else None, reason=reason, margin=min(margins))
        return out

    if cos_rays < cs and cos_rays > 0.0 and (st1 or st2 or cos_rays < 0.9998):
        X = linear(dlt_rows(proj_matrix(cam, pose1), proj_matrix(cam, pose2), x1, y1, x2, y2))
        if X is None:
            return done("w0")
        code = 1
    else:
        if st1 or st2:
            margins.append(_rel(cs1, cs2) if (st1 and st2) else 1.0)
        if st1 and cs1 < cs2:
            z = float(k1["depth"]); X = R1.T @ (np.array([(x1 - cam.cx) * z / cam.fx, (y1 - cam.cy) * z / cam.fy, z]) - t1); code = 2
        elif st2 and cs2 < cs1:
            z = float(k2["depth"]); X = R2.T @ (np.array([(x2 - cam.cx) * z / cam.fx, (y2 - cam.cy) * z / cam.fy, z]) - t2); code = 3
        else:
            return done("cos<=0" if cos_rays <= 0.0 else "parallax")
    dist = []
    for name, R, t, k, st in (("1", R1, t1, k1, st1), ("2", R2, t2, k2, st2)):
        Xc = R @ X + t
        d = math.sqrt(float((X + R.T @ t) @ (X + R.T @ t)))
        margins.append(abs(Xc[2]) / max(d, 1e-300))
        if not Xc[2] > 0:
            return done("depth" + name)
        s2 = scale[int(k["octave"])] ** 2
        ex = cam.fx * Xc[0] / Xc[2] + cam.cx - float(k["x"]); ey = cam.fy * Xc[1] / Xc[2] + cam.cy - float(k["y"])
        if st:
            er = cam.fx * Xc[0] / Xc[2] + cam.cx - cam.fxb / Xc[2] - float(k["x_right"])
            e2, bound = ex * ex + ey * ey + er * er, 7.81473 * s2
        else:
            e2, bound = ex * ex + ey * ey, 5.991 * s2
        margins.append(_rel(e2, bound))
        if not e2 <= bound:
            return done("reproj" + name + ("_stereo" if st else ""))
        if not d > 0:
            return done("dist" + name)
        dist.append(d)
    ratio_d = dist[0] / dist[1]; ratio_o = scale[int(k2["octave"])] / scale[int(k1["octave"])]; rf = 1.5 * cam.scale_factor
    margins += [_rel(ratio_d * rf, ratio_o), _rel(ratio_d, ratio_o * rf)]
    if ratio_d * rf < ratio_o:
        return done("ratio_low")
    if ratio_d > ratio_o * rf:
        return done("ratio_high")
    return done("ok%d" % code, code, X)


def project(cam, pose, Xw):
    """pixel, depth of world points (n, 3) in a view (test construction)"""
    R, t = view(pose)
    Xc = np.asarray(Xw, np.float64) @ R.T + t
    return cam.fx * Xc[:, 0] / Xc[:, 2] + cam.cx, cam.fy * Xc[:, 1] / Xc[:, 2] + cam.cy, Xc[:, 2]
