"""ctypes binding of the CPU oracle (oracle/liblpslam_oracle.so).  TEST INFRASTRUCTURE ONLY.

Importable from tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg only; the product
package lpslam_amd never imports this module.  PARITY UNPINNED: see oracle/ora.h.
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "liblpslam_oracle.so")
MAX_LEVELS = 16


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in ("ora_orb.c", "ora_match.c", "ora_ba.c", "ora_sim3.c", "ora_bow.c", "ora.h", "orb_pattern.inc")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs if os.path.exists(s)):
        subprocess.check_call(["make", "-C", _HERE, "-B" if force else "-s"], stdout=subprocess.DEVNULL)
    return _LIB


class Keypoint(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int32), ("class_id", C.c_int32)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CORNER_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("score", "<i4")])
OBS_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("u", "<f8"), ("v", "<f8"), ("ur", "<f8"),
                      ("inv_sigma2", "<f8")])
LOG_DTYPE = np.dtype([("chi2_before", "<f8"), ("chi2_after", "<f8"), ("lambda", "<f8"),
                      ("trials", "<i4"), ("status", "<i4")])


class OrbParams(C.Structure):
    _fields_ = [("max_num_keypts", C.c_int32), ("scale_factor", C.c_float), ("num_levels", C.c_int32),
                ("ini_fast_thr", C.c_int32), ("min_fast_thr", C.c_int32)]


class BaCam(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("fxb", C.c_double), ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]


_lib = None


def use_native_build(on=True):
    """Switches every later call to the -march=native build (bench.py's second CPU-baseline leg; same sources, built with
    `make native` on the machine that runs it) or back to the default build."""
    global _lib
    if on:
        path = os.path.join(_HERE, "liblpslam_oracle_native.so")
        # always rebuilt: a library made on another machine (the repository snapshot travels) may use instructions this CPU lacks
        subprocess.check_call(["make", "-C", _HERE, "-s", "-B", "native"], stdout=subprocess.DEVNULL)
        _lib = None
        _load(path)
    else:
        _lib = None
        lib()


def lib():
    global _lib
    if _lib is None:
        build()
        _load(_LIB)
    return _lib


def _load(path):
    global _lib
    _lib = C.CDLL(path)
    _lib.ora_fast_atan2.restype = C.c_float
    _lib.ora_fast_atan2.argtypes = [C.c_float, C.c_float]
    _lib.ora_ic_angle.restype = C.c_float
    return _lib


def _p(a, t=C.c_void_p):
    return a.ctypes.data_as(t) if a is not None else None


def params(max_kpts=2000, scale=1.2, levels=8, ini=20, mn=7):
    return OrbParams(int(max_kpts), float(scale), int(levels), int(ini), int(mn))


def pyramid_sizes(w, h, p):
    lw = (C.c_int * MAX_LEVELS)(); lh = (C.c_int * MAX_LEVELS)()
    lib().ora_pyramid_sizes(w, h, C.byref(p), lw, lh)
    return list(lw[:p.num_levels]), list(lh[:p.num_levels])


def scale_factors(p):
    s = (C.c_float * MAX_LEVELS)(); i = (C.c_float * MAX_LEVELS)()
    lib().ora_scale_factors(C.byref(p), s, i)
    return np.array(s[:p.num_levels], np.float32), np.array(i[:p.num_levels], np.float32)


def keypts_per_level(p):
    q = (C.c_int * MAX_LEVELS)()
    lib().ora_keypts_per_level(C.byref(p), q)
    return list(q[:p.num_levels])


def resize(src, dw, dh):
    src = np.ascontiguousarray(src, np.uint8)
    dst = np.empty((dh, dw), np.uint8)
    lib().ora_resize_linear_u8(_p(src), src.shape[1], src.shape[0], src.shape[1], _p(dst), dw, dh, dw)
    return dst


def fast_level(img, ini=20, mn=7, mask=None, scale=1.0):
    """mask: level-0 mask (0 = masked out), scale: this level's scale factor"""
    img = np.ascontiguousarray(img, np.uint8)
    cap = img.size // 4 + 16
    out = np.zeros(cap, CORNER_DTYPE)
    if mask is None:
        n = lib().ora_fast_level(_p(img), img.shape[1], img.shape[0], img.shape[1], ini, mn, _p(out), cap)
    else:
        mask = np.ascontiguousarray(mask, np.uint8)
        f = lib().ora_fast_level_masked
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int]
        n = f(_p(img), img.shape[1], img.shape[0], img.shape[1], ini, mn, _p(mask), mask.shape[1], mask.shape[0], mask.shape[1], float(scale), _p(out), cap)
    return out[:n].copy()


def fast(img, thr, nms=True):
    img = np.ascontiguousarray(img, np.uint8)
    cap = img.size + 16
    out = np.zeros(cap, CORNER_DTYPE)
    n = lib().ora_fast9_16(_p(img), img.shape[1], img.shape[0], img.shape[1], thr, int(nms), _p(out), cap)
    return out[:n].copy()


def distribute(cand, w, h, quota):
    cand = np.ascontiguousarray(cand, CORNER_DTYPE)
    out = np.zeros(len(cand) + 8, np.int32)
    n = lib().ora_distribute(_p(cand), len(cand), 19, w - 19, 19, h - 19, quota, _p(out), len(out))
    return out[:n].copy()


def gauss7(img):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty_like(img)
    lib().ora_gauss7x7_u8(_p(img), img.shape[1], img.shape[0], img.shape[1], _p(out), img.shape[1])
    return out


def ic_angle(img, x, y):
    img = np.ascontiguousarray(img, np.uint8)
    f = lib().ora_ic_angle
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    return f(_p(img), img.shape[1], int(x), int(y))


def sincos_deg(a):
    s = C.c_float(); c = C.c_float()
    f = lib().ora_sincos_deg
    f.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    f(float(a), C.byref(s), C.byref(c))
    return s.value, c.value


def extract(img, p, want_pyramid=False, mask=None):
    """Returns (keypoints[KP_DTYPE], descriptors[n,32], cand_count[levels], pyramid levels or None).
    mask: optional uint8 image of the same size, 0 = masked out ([UPSTREAM] orb_extractor::extract's mask argument)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    if mask is not None:
        mask = np.ascontiguousarray(mask, np.uint8)
        assert mask.shape == img.shape
    # a level returns up to max(quota + 3, 4 * roots) corners, roots = the aspect ratio of the level's BORDERED area (19 px each side):
    # a 1531 x 97 image has 23-30 root cells per level, not 16
    # (taken per level: level 1 of a 2873 x 64 image at scale 1.38 is 2082 x 46 and has 256 roots, the image itself 109)
    lw, lh = pyramid_sizes(w, h, p)
    roots = max([1, int(round((w - 32) / max(h - 32, 1))) + 1, int(round((h - 32) / max(w - 32, 1))) + 1] +
                [int(round(max(a - 38, 1) / max(b - 38, 1))) + int(round(max(b - 38, 1) / max(a - 38, 1))) + 1 for a, b in zip(lw, lh)])
    cap = p.max_num_keypts + (4 * roots + 8) * p.num_levels + 64
    kp = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8)
    cc = np.zeros(p.num_levels, np.int32)
    pyr = np.zeros(sum(a * b for a, b in zip(lw, lh)), np.uint8) if want_pyramid else None
    n = lib().ora_orb_extract_masked(_p(img), w, h, w, C.byref(p), _p(mask), w, _p(kp), _p(desc), cap, _p(pyr), _p(cc))
    assert n <= cap
    levels = None
    if want_pyramid:
        levels, off = [], 0
        for a, b in zip(lw, lh):
            levels.append(pyr[off:off + a * b].reshape(b, a)); off += a * b
    return kp[:n].copy(), desc[:n].copy(), cc, levels


def match_bf_knn2(q, t):
    q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
    bi = np.zeros(len(q), np.int32); bd = np.zeros(len(q), np.int32); sd = np.zeros(len(q), np.int32)
    lib().ora_match_bf_knn2(_p(q), len(q), _p(t), len(t), _p(bi), _p(bd), _p(sd))
    return bi, bd, sd


def match_bf(q, t, max_dist=50, ratio=0.0, cross_check=False):
    q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
    oq = np.zeros(len(q), np.int32); ot = np.zeros(len(q), np.int32); od = np.zeros(len(q), np.int32)
    f = lib().ora_match_bf
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    n = f(_p(q), len(q), _p(t), len(t), int(max_dist), float(ratio), int(cross_check), _p(oq), _p(ot), _p(od))
    return oq[:n].copy(), ot[:n].copy(), od[:n].copy()


def match_stereo(pyr_l, pyr_r, p, kl, dl, kr, dr, fxb, baseline):
    L = p.num_levels
    keep = [np.ascontiguousarray(a, np.uint8) for a in list(pyr_l) + list(pyr_r)]
    pl = (C.c_void_p * L)(*[a.ctypes.data for a in keep[:L]])
    pr = (C.c_void_p * L)(*[a.ctypes.data for a in keep[L:]])
    lw = (C.c_int * L)(*[a.shape[1] for a in keep[:L]]); lh = (C.c_int * L)(*[a.shape[0] for a in keep[:L]])
    kl = np.ascontiguousarray(kl, KP_DTYPE); kr = np.ascontiguousarray(kr, KP_DTYPE)
    dl = np.ascontiguousarray(dl, np.uint8); dr = np.ascontiguousarray(dr, np.uint8)
    xr = np.zeros(len(kl), np.float32); dep = np.zeros(len(kl), np.float32); bi = np.zeros(len(kl), np.int32)
    f = lib().ora_match_stereo
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    n = f(pl, pr, lw, lh, C.byref(p), _p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr),
          float(fxb), float(baseline), _p(xr), _p(dep), _p(bi))
    return xr, dep, bi, n


def ba_cam(cam, robust=True):
    return BaCam(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["fxb"],
                 np.sqrt(5.991) if robust else 0.0, np.sqrt(7.815) if robust else 0.0)


def ba_obs(prob):
    o = np.zeros(len(prob["obs_pose"]), OBS_DTYPE)
    o["pose"] = prob["obs_pose"]; o["point"] = prob["obs_point"]
    o["u"] = prob["obs_uvr"][:, 0]; o["v"] = prob["obs_uvr"][:, 1]; o["ur"] = prob["obs_uvr"][:, 2]
    o["inv_sigma2"] = prob["obs_inv_sigma2"]
    return o


def ba_optimize(poses, fixed, points, obs, cam, robust=True, iters=10, active=None):
    poses = np.ascontiguousarray(poses, np.float64).copy(); points = np.ascontiguousarray(points, np.float64).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8); obs = np.ascontiguousarray(obs, OBS_DTYPE)
    log = np.zeros(iters, LOG_DTYPE)
    c = ba_cam(cam)
    act = np.ascontiguousarray(active, np.uint8) if active is not None else None
    n = lib().ora_ba_optimize(_p(poses), _p(fixed), len(poses), _p(points), len(points), _p(obs), _p(act),
                              len(obs), C.byref(c), int(robust), int(iters), _p(log))
    return poses, points, log[:n].copy()


def ba_local(poses, fixed, points, obs, cam, first=5, second=10):
    poses = np.ascontiguousarray(poses, np.float64).copy(); points = np.ascontiguousarray(points, np.float64).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8); obs = np.ascontiguousarray(obs, OBS_DTYPE)
    out = np.zeros(len(obs), np.uint8)
    c = ba_cam(cam)
    lib().ora_ba_local(_p(poses), _p(fixed), len(poses), _p(points), len(points), _p(obs), len(obs),
                       C.byref(c), int(first), int(second), _p(out))
    return poses, points, out


def ba_chi2(poses, points, obs, cam):
    poses = np.ascontiguousarray(poses, np.float64); points = np.ascontiguousarray(points, np.float64)
    obs = np.ascontiguousarray(obs, OBS_DTYPE)
    chi = np.zeros(len(obs)); pos = np.zeros(len(obs), np.uint8)
    c = ba_cam(cam)
    lib().ora_ba_chi2(_p(poses), _p(points), _p(obs), len(obs), C.byref(c), _p(chi), _p(pos))
    return chi, pos


def pose_optimize(pose7, points, obs, cam):
    pose = np.ascontiguousarray(pose7, np.float64).copy(); points = np.ascontiguousarray(points, np.float64)
    obs = np.ascontiguousarray(obs, OBS_DTYPE)
    out = np.zeros(len(obs), np.uint8)
    c = ba_cam(cam)
    n = lib().ora_pose_optimize(_p(pose), _p(points), _p(obs), len(obs), C.byref(c), _p(out))
    return pose, out, n


# ---- Sim3 pose graph -------------------------------------------------------------------------
SIM3_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("meas", "<f8", (8,))])


def sim3_edges(ei, ej, meas):
    e = np.zeros(len(ei), SIM3_EDGE_DTYPE)
    e["i"] = ei; e["j"] = ej; e["meas"] = meas
    return e


def _sim3_unary(fn, a, n_out):
    a = np.ascontiguousarray(a, np.float64); out = np.zeros(n_out)
    fn(_p(a), _p(out))
    return out


def sim3_exp(update7):
    return _sim3_unary(lib().ora_sim3_exp, update7, 8)


def sim3_log(s):
    return _sim3_unary(lib().ora_sim3_log, s, 7)


def sim3_inv(s):
    return _sim3_unary(lib().ora_sim3_inv, s, 8)


def sim3_mul(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64); out = np.zeros(8)
    lib().ora_sim3_mul(_p(a), _p(b), _p(out))
    return out


def sim3_graph_chi2(verts, edges):
    verts = np.ascontiguousarray(verts, np.float64); edges = np.ascontiguousarray(edges, SIM3_EDGE_DTYPE)
    f = lib().ora_sim3_graph_chi2; f.restype = C.c_double
    return f(_p(verts), _p(edges), len(edges))


def sim3_graph_optimize(verts, fixed, edges, fix_scale=True, iters=50):
    verts = np.ascontiguousarray(verts, np.float64).copy(); fixed = np.ascontiguousarray(fixed, np.uint8)
    edges = np.ascontiguousarray(edges, SIM3_EDGE_DTYPE)
    log = np.zeros(iters, LOG_DTYPE)
    n = lib().ora_sim3_graph_optimize(_p(verts), _p(fixed), len(verts), _p(edges), len(edges), int(fix_scale), int(iters), _p(log))
    return verts, log[:n].copy()


SIM3_PAIR_DTYPE = np.dtype([("p1c", "<f8", (3,)), ("p2c", "<f8", (3,)), ("obs1", "<f8", (2,)), ("obs2", "<f8", (2,)),
                            ("inv_sigma2_1", "<f8"), ("inv_sigma2_2", "<f8")])


def sim3_pairs(prob):
    p = np.zeros(len(prob["p1c"]), SIM3_PAIR_DTYPE)
    for k in ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        p[k] = prob[k]
    return p


def sim3_transform_optimize(s12, pairs, cam1, cam2, chi_sq=10.0, fix_scale=True):
    s = np.ascontiguousarray(s12, np.float64).copy(); pairs = np.ascontiguousarray(pairs, SIM3_PAIR_DTYPE)
    c1 = np.ascontiguousarray(cam1, np.float64); c2 = np.ascontiguousarray(cam2, np.float64)
    inl = np.zeros(len(pairs), np.uint8)
    f = lib().ora_sim3_transform_optimize
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
    n = f(_p(s), _p(pairs), len(pairs), _p(c1), _p(c2), float(chi_sq), int(fix_scale), _p(inl))
    return s, inl, n


PROJ_QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("x_right", "<f4"), ("radius", "<f4"), ("min_level", "<i4"), ("max_level", "<i4")])


def match_projection(kp, desc, stereo_xr, width, height, queries, q_desc, hamming_thr=100, lowe_ratio=0.8, taken=None):
    kp = np.ascontiguousarray(kp, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE); qd = np.ascontiguousarray(q_desc, np.uint8)
    sx = np.ascontiguousarray(stereo_xr, np.float32) if stereo_xr is not None else None
    t = np.ascontiguousarray(taken, np.uint8).copy() if taken is not None else None
    idx = np.full(max(len(q), 1), -1, np.int32); dist = np.zeros(max(len(q), 1), np.int32)
    f = lib().ora_match_projection
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    n = f(_p(kp), _p(desc), _p(sx), len(kp), width, height, _p(q), _p(qd), len(q), int(hamming_thr), float(lowe_ratio), _p(t), _p(idx), _p(dist))
    return idx[:len(q)].copy(), dist[:len(q)].copy(), n


def match_orientation_filter(angle_q, angle_t, match_idx):
    aq = np.ascontiguousarray(angle_q, np.float32); at = np.ascontiguousarray(angle_t, np.float32)
    m = np.ascontiguousarray(match_idx, np.int32).copy()
    n = lib().ora_match_orientation_filter(_p(aq), _p(at), _p(m), len(m))
    return m, n


def match_fuse(kp, desc, stereo_xr, width, height, inv_level_sigma_sq, queries, q_desc, hamming_thr=50):
    kp = np.ascontiguousarray(kp, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE); qd = np.ascontiguousarray(q_desc, np.uint8)
    sx = np.ascontiguousarray(stereo_xr, np.float32) if stereo_xr is not None else None
    isq = np.ascontiguousarray(inv_level_sigma_sq, np.float32)
    idx = np.full(max(len(q), 1), -1, np.int32); dist = np.zeros(max(len(q), 1), np.int32)
    f = lib().ora_match_fuse
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    n = f(_p(kp), _p(desc), _p(sx), len(kp), width, height, _p(isq), _p(q), _p(qd), len(q), int(hamming_thr), _p(idx), _p(dist))
    return idx[:len(q)].copy(), dist[:len(q)].copy(), n


def match_area(kp2, desc2, width, height, queries, q_desc, hamming_thr=50, lowe_ratio=0.9):
    kp2 = np.ascontiguousarray(kp2, KP_DTYPE); desc2 = np.ascontiguousarray(desc2, np.uint8)
    q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE); qd = np.ascontiguousarray(q_desc, np.uint8)
    idx = np.full(max(len(q), 1), -1, np.int32)
    f = lib().ora_match_area
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    n = f(_p(kp2), _p(desc2), len(kp2), width, height, _p(q), _p(qd), len(q), int(hamming_thr), float(lowe_ratio), _p(idx))
    return idx[:len(q)].copy(), n


# ---- bag of words (ora_bow.c; [UPSTREAM] DBoW2 TemplatedVocabulary, openvslam match::bow_tree) -----------------------------------
def bow_transform(vocab, desc, levels_up=4):
    """vocab: dict(k, L, parent, desc, weight, is_leaf) with the nodes in DBoW2 file order; returns word id, word weight, node id"""
    d = np.ascontiguousarray(desc, np.uint8); n = len(d)
    parent = np.ascontiguousarray(vocab["parent"], np.int32); nd = np.ascontiguousarray(vocab["desc"], np.uint8)
    wt = np.ascontiguousarray(vocab["weight"], np.float32); leaf = np.ascontiguousarray(vocab["is_leaf"], np.uint8)
    w = np.zeros(max(n, 1), np.int32); ww = np.zeros(max(n, 1), np.float32); node = np.zeros(max(n, 1), np.int32)
    f = lib().ora_bow_transform
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    nw = f(_p(parent), _p(nd), _p(wt), _p(leaf), len(parent), int(vocab["L"]), _p(d), n, int(levels_up), _p(w), _p(ww), _p(node))
    assert nw >= 0
    return w[:n], ww[:n], node[:n]


def bow_tree_match(q_desc, q_node, t_desc, t_node, hamming_thr=50, lowe_ratio=0.75, t_taken=None):
    qd = np.ascontiguousarray(q_desc, np.uint8); qn = np.ascontiguousarray(q_node, np.int32)
    td = np.ascontiguousarray(t_desc, np.uint8); tn = np.ascontiguousarray(t_node, np.int32)
    tk = np.ascontiguousarray(t_taken, np.uint8) if t_taken is not None else None
    idx = np.full(max(len(qn), 1), -1, np.int32); dist = np.zeros(max(len(qn), 1), np.int32)
    f = lib().ora_bow_tree_match
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    n = f(_p(qd), _p(qn), len(qn), _p(td), _p(tn), len(tn), _p(tk), int(hamming_thr), float(lowe_ratio), _p(idx), _p(dist))
    return idx[:len(qn)], dist[:len(qn)], n


def bow_vector(word_id, word_weight):
    """BowVector of DBoW2 with TF_IDF weighting and L1 scoring: the weights of a word add up, then the vector is L1-normalised;
    returns (sorted word ids, values)"""
    acc = {}
    for w, x in zip(word_id, word_weight):
        if x > 0:
            acc[int(w)] = acc.get(int(w), 0.0) + float(x)
    ids = np.array(sorted(acc), np.int32)
    val = np.array([acc[i] for i in ids], np.float64)
    s = np.abs(val).sum()
    return ids, (val / s if s > 0 else val)


def bow_score_l1(a, b):
    """DBoW2 L1Scoring::score: 1 - 0.5 |a - b|_1 over the common words' contribution (-sum(|ai - bi| - |ai| - |bi|) / 2)"""
    ia, va = a; ib, vb = b
    common, xa, xb = np.intersect1d(ia, ib, return_indices=True)
    if len(common) == 0:
        return 0.0
    s = np.sum(np.abs(va[xa] - vb[xb]) - np.abs(va[xa]) - np.abs(vb[xb]))
    return float(-s / 2.0)
