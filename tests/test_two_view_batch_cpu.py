"""CPU tests of the two-view initialiser's batch side: the fixed-size estimators of csrc/two_view_math.h against
LpSlam::homography_from_matches / fundamental_from_matches, the sample table and the RANSAC loop replayed in numpy against the batch's
CPU definition, the "none" answers, and two_view_initialize composed of its four steps against the recorded goldens.  [UPSTREAM]
initialize::perspective.  Comparisons are bit for bit: the functions are host code of one library and perform the same operations in
the same order; the numpy replay performs them one rounding at a time (elementwise products and sums, no fused operation)."""
import ctypes as C
import os

import numpy as np
import pytest

import solver_cases as S
import two_view_cases as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_solvers.npz")


@pytest.fixture(scope="module")
def hip():
    from lpslam_amd import _build, hip
    _build.host_library()
    return hip


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _models(lib, x1, x2):
    """homography_from_matches / fundamental_from_matches at a run-time count"""
    f = lib.lpslam_two_view_models_host
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]; f.restype = None
    H = np.zeros(9); F = np.zeros(9)
    f(_p(np.ascontiguousarray(x1)), _p(np.ascontiguousarray(x2)), len(x1), _p(H), _p(F))
    return H.reshape(3, 3), F.reshape(3, 3)


# ---- the operations of csrc/two_view_math.h in numpy / Python floats, one rounding each --------------------------------------------
def _normalize(p):
    n = len(p)
    mx = my = 0.0
    for x, y in p:
        mx += x; my += y
    mx /= float(n); my /= float(n)
    out = np.column_stack([p[:, 0] - mx, p[:, 1] - my])
    dx = dy = 0.0
    for x, y in out:
        dx += abs(x); dy += abs(y)
    dx /= float(n); dy /= float(n)
    with np.errstate(all="ignore"):
        sx, sy = np.float64(1.0) / np.float64(dx), np.float64(1.0) / np.float64(dy)
        out = np.column_stack([out[:, 0] * sx, out[:, 1] * sy])
        return out, np.array([sx, 0, -mx * sx, 0, sy, -my * sy, 0, 0, 1], np.float64)


def _mul(a, b):
    r = np.zeros(9)
    for i in range(3):
        for j in range(3):
            r[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j]
    return r


def _det(a):
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6])


def _inverse(a):
    i = np.float64(1.0) / _det(a)
    return np.array([(a[4] * a[8] - a[5] * a[7]) * i, (a[2] * a[7] - a[1] * a[8]) * i, (a[1] * a[5] - a[2] * a[4]) * i,
                     (a[5] * a[6] - a[3] * a[8]) * i, (a[0] * a[8] - a[2] * a[6]) * i, (a[2] * a[3] - a[0] * a[5]) * i,
                     (a[3] * a[7] - a[4] * a[6]) * i, (a[1] * a[6] - a[0] * a[7]) * i, (a[0] * a[4] - a[1] * a[3]) * i])


def _ordered_sum(c1, add1, c2, add2):
    score = 0.0
    for a, fa, b, fb in zip(c1.tolist(), add1.tolist(), c2.tolist(), add2.tolist()):
        if fa:
            score += a
        if fb:
            score += b
    return score


def _score_h(H21, H12, p1, p2, sigma):
    th, inv_s2 = 5.991, 1.0 / (sigma * sigma)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    w = 1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8])
    x, y = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w, (H12[3] * u2 + H12[4] * v2 + H12[5]) * w
    c1 = ((u1 - x) * (u1 - x) + (v1 - y) * (v1 - y)) * inv_s2
    w = 1.0 / (H21[6] * u1 + H21[7] * v1 + H21[8])
    x, y = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w, (H21[3] * u1 + H21[4] * v1 + H21[5]) * w
    c2 = ((u2 - x) * (u2 - x) + (v2 - y) * (v2 - y)) * inv_s2
    out1, out2 = c1 > th, c2 > th
    return _ordered_sum(th - c1, ~out1, th - c2, ~out2), ~(out1 | out2)


def _score_f(F, p1, p2, sigma):
    th, ths, inv_s2 = 3.841, 5.991, 1.0 / (sigma * sigma)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    a, b, c = F[0] * u1 + F[1] * v1 + F[2], F[3] * u1 + F[4] * v1 + F[5], F[6] * u1 + F[7] * v1 + F[8]
    num = a * u2 + b * v2 + c
    c1 = num * num / (a * a + b * b) * inv_s2
    a, b, c = F[0] * u2 + F[3] * v2 + F[6], F[1] * u2 + F[4] * v2 + F[7], F[2] * u2 + F[5] * v2 + F[8]
    num = a * u1 + b * v1 + c
    c2 = num * num / (a * a + b * b) * inv_s2
    out1, out2 = c1 > th, c2 > th
    return _ordered_sum(ths - c1, ~out1, ths - c2, ~out2), ~(out1 | out2)


def _replay(hip, s, sigma, iterations, seed):
    """the RANSAC loop of two_view_initialize over the sample table: per model (iteration, score, matrix, flags)"""
    p1, p2 = s["p1"], s["p2"]
    n = len(p1)
    none = (-1, 0.0, np.zeros(9), np.zeros(n, bool))
    if n < 8:
        return none, none
    table = hip.two_view_sample_table(n, iterations, seed)
    n1, T1 = _normalize(p1)
    n2, T2 = _normalize(p2)
    with np.errstate(all="ignore"):
        T2inv, T2t = _inverse(T2), T2.reshape(3, 3).T.ravel()
        best_h, best_f = (-1, -1.0, None, None), (-1, -1.0, None, None)
        for it, row in enumerate(table):
            Hn, Fn = hip.two_view_models8_host(n1[row], n2[row])
            H21, F21 = _mul(_mul(T2inv, Hn.ravel()), T1), _mul(_mul(T2t, Fn.ravel()), T1)
            if abs(_det(H21)) > 1e-300:
                sc, fl = _score_h(H21, _inverse(H21), p1, p2, sigma)
                if sc > best_h[1]:
                    best_h = (it, sc, H21, fl)
            sc, fl = _score_f(F21, p1, p2, sigma)
            if sc > best_f[1]:
                best_f = (it, sc, F21, fl)
    return (best_h if best_h[0] >= 0 else none), (best_f if best_f[0] >= 0 else none)


def _assert_model(got, s_index, m, want, off):
    best, score, model, fh, ff = got
    it, sc, M, fl = want
    assert best[s_index, m] == it, (s_index, m, best[s_index], it)
    assert np.float64(score[s_index, m]).tobytes() == np.float64(sc).tobytes(), (s_index, m, score[s_index, m], sc)
    assert model[s_index, m].tobytes() == np.ascontiguousarray(M, np.float64).tobytes(), (s_index, m)
    assert np.array_equal((fh, ff)[m][off[s_index]:off[s_index + 1]].astype(bool), fl), (s_index, m)


def test_the_estimators_at_eight_are_the_run_time_estimators_bit_for_bit(hip):
    lib = hip.host_lib()
    for i in range(300):
        s = T.scene(8, 2000 + i, planar=(i % 3 == 0), outliers=(0.25 if i % 5 == 0 else 0.0))
        n1, _ = _normalize(s["p1"]); n2, _ = _normalize(s["p2"])
        H8, F8 = hip.two_view_models8_host(n1, n2)
        H, F = _models(lib, n1, n2)
        assert H8.tobytes() == H.tobytes() and F8.tobytes() == F.tobytes(), i
        assert np.isfinite(H).all() and np.isfinite(F).all() and abs(np.linalg.norm(H) - 1) < 1e-9
        assert abs(np.linalg.det(F)) < 1e-9                                # rank 2
    c = T.collinear8()
    H8, F8 = hip.two_view_models8_host(c["p1"], c["p2"])
    H, F = _models(lib, c["p1"], c["p2"])
    assert H8.tobytes() == H.tobytes() and F8.tobytes() == F.tobytes()


@pytest.mark.parametrize("iterations", [1, 100])
@pytest.mark.parametrize("seed", [0, T.SEED])
@pytest.mark.parametrize("n", [8, 9, 37, 300])
def test_the_sample_table_replayed_in_numpy_gives_the_loops_winners(hip, n, seed, iterations):
    s = T.general(n, 40 + n, 0.3 if n >= 37 else 0.0)
    off, p1, p2 = T.concat([s])
    got = hip.two_view_ransac_batch_host(off, p1, p2, 1.0, iterations, seed)
    table = hip.two_view_sample_table(n, iterations, seed)
    assert table.shape == (iterations, 8) and all(len(set(r)) == 8 and min(r) >= 0 and max(r) < n for r in table.tolist())
    if seed == 0:                                                          # seed 0 draws what seed 1 draws
        assert np.array_equal(table, hip.two_view_sample_table(n, iterations, 1))
    want_h, want_f = _replay(hip, s, 1.0, iterations, seed)
    _assert_model(got, 0, 0, want_h, off)
    _assert_model(got, 0, 1, want_f, off)
    if n == 300 and iterations == 100:                                     # the loop finds the planted motion: the inliers are the matches not replaced
        assert want_f[0] >= 0 and (want_f[3] & ~s["bad"]).sum() > 0.8 * (~s["bad"]).sum() and (want_f[3] & s["bad"]).sum() <= 0.1 * s["bad"].sum()


def test_sets_too_small_empty_and_degenerate_answer_none_and_leave_their_neighbours_alone(hip):
    a, b = T.general(37, 3, 0.3), T.general(65, 6, 0.3)
    sets = [a, T.first(a, 7), T.first(a, 0), T.one_point(20), b]
    off, p1, p2 = T.concat(sets)
    best, score, model, fh, ff = got = hip.two_view_ransac_batch_host(off, p1, p2, 1.0, 100, T.SEED)
    for i in (1, 2, 3):
        assert (best[i] == -1).all() and (score[i] == 0).all() and not model[i].any(), i
        assert not fh[off[i]:off[i + 1]].any() and not ff[off[i]:off[i + 1]].any()
    for i in (0, 4):
        o1, q1, q2 = T.concat([sets[i]])
        alone = hip.two_view_ransac_batch_host(o1, q1, q2, 1.0, 100, T.SEED)
        assert (alone[0][0] >= 0).all()
        assert np.array_equal(best[i], alone[0][0]) and score[i].tobytes() == alone[1][0].tobytes() and model[i].tobytes() == alone[2][0].tobytes()
        assert np.array_equal(fh[off[i]:off[i + 1]], alone[3]) and np.array_equal(ff[off[i]:off[i + 1]], alone[4])
    # offsets that do not start at 0: the first set is skipped, the flags stay indexed like the matches
    part = hip.two_view_ransac_batch_host(off[3:], p1, p2, 1.0, 100, T.SEED)
    assert np.array_equal(part[0], best[3:]) and part[2].tobytes() == model[3:].tobytes() and np.array_equal(part[3][off[4]:], fh[off[4]:])
    # the refusals of the device call
    for kw in (dict(iterations=0), dict(iterations=hip.TWO_VIEW_MAX_ITERATIONS + 1), dict(sigma=0.0), dict(sigma=float("nan")), dict(sigma=-1.0)):
        with pytest.raises(hip.LpslamHipError):
            hip.two_view_ransac_batch_host(off, p1, p2, **kw)
    with pytest.raises(hip.LpslamHipError):
        hip.two_view_ransac_batch_host(np.array([0, 20, 10], np.int32), p1, p2)
    assert len(hip.two_view_ransac_batch_host(np.zeros(1, np.int32), np.zeros((0, 2)), np.zeros((0, 2)))[0]) == 0


def _initialize(lib, name, K, kp_ref, kp_cur, matches, sigma, iterations, seed):
    n = len(matches)
    o = dict(ok=np.zeros(1, np.int32), R=np.zeros(9), t=np.zeros(3), H=np.zeros(9), F=np.zeros(9), scores=np.zeros(2), parallax_deg=np.zeros(1),
             model=np.zeros(1, np.int32), inlier=np.zeros(max(n, 1), np.uint8), triangulated=np.zeros(max(n, 1), np.uint8), points=np.zeros((max(n, 1), 3)))
    f = getattr(lib, name)
    f.restype = C.c_int
    steps = name.endswith("_steps")
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_uint32] + [C.c_void_p] * (11 if steps else 10)
    calls = np.zeros(2, np.int32)
    extra = [_p(calls)] if steps else []
    o["ok"][0] = f(_p(np.ascontiguousarray(K)), _p(kp_ref), _p(kp_cur), _p(matches), n, sigma, iterations, seed, _p(o["R"]), _p(o["t"]), _p(o["H"]), _p(o["F"]),
                   _p(o["scores"]), _p(o["parallax_deg"]), _p(o["model"]), _p(o["inlier"]), _p(o["triangulated"]), _p(o["points"]), *extra)
    return o, calls


def test_the_four_steps_through_the_hook_return_the_recorded_goldens(hip):
    lib = hip.host_lib()
    mine = [c for c in S.load(GOLDEN) if c[0] == "two_view"]
    assert len(mine) >= 2
    for _, tag, args, a, want in mine:
        got, calls = _initialize(lib, "lpslam_two_view_initialize_steps", a["K"], a["kp_ref"], a["kp_cur"], a["matches"], args["sigma"], args["iterations"], args["seed"])
        assert calls[0] >= 1 and calls[1] == 0, tag
        for name, w in want.items():
            g = np.ascontiguousarray(got[name])[:len(w)] if name in ("inlier", "triangulated", "points") else np.ascontiguousarray(got[name])
            if name == "parallax_deg":
                assert abs(g[0] - w[0]) <= 1e-12 * abs(w[0]), (tag, g[0], w[0])
            else:
                assert g.tobytes() == w.tobytes(), (tag, name)


@pytest.mark.parametrize("name,model,ok", [("general", 1, True), ("planar", 0, True), ("rotation", 0, False), ("out30", 1, None), ("out60", 1, None), ("one_point", -1, False),
                                           ("collinear", None, False), ("seven", -1, False)])
def test_the_four_steps_through_the_hook_are_two_view_initialize(hip, name, model, ok):
    """every scene of tests/two_view_cases.py: the function with its own steps and with the steps handed in return the same bytes, and
    the scene is what its name says (which model wins, whether a map comes out)"""
    lib = hip.host_lib()
    s = dict(general=T.general(), planar=T.planar(), rotation=T.rotation(), out30=T.general(300, 12, 0.3), out60=T.general(300, 13, 0.6), one_point=T.one_point(),
             collinear=T.collinear8(), seven=T.first(T.general(), 7))[name]
    kp_ref, kp_cur, matches = T.as_keypoints(s)
    a, _ = _initialize(lib, "lpslam_two_view_initialize", T.K, kp_ref, kp_cur, matches, 1.0, 100, 12345)
    b, calls = _initialize(lib, "lpslam_two_view_initialize_steps", T.K, kp_ref, kp_cur, matches, 1.0, 100, 12345)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (name, k)
    assert calls[1] == 0 and (name != "seven" or calls[0] == 0)
    if model is not None:
        assert a["model"][0] == model, (name, a["model"], a["scores"])
    if ok is not None:
        assert bool(a["ok"][0]) == ok, name
    if ok:
        assert calls[0] == 2                                               # the RANSAC loop and the pose check
    if name == "rotation":
        assert a["parallax_deg"][0] < 1.0
    # sets without a winner in step 1 have no score after step 2 either
    off, p1, p2 = T.concat([s])
    best, score, mod, fh, ff = hip.two_view_ransac_batch_host(off, p1, p2, 1.0, 100, 12345)
    if name in ("one_point", "seven"):
        assert (best == -1).all() and not a["scores"].any()
    else:
        assert (best[0] >= 0).any()


def test_check_poses_host_is_the_pose_check_of_two_view_initialize(hip):
    """the planted motion among wrong ones: codes, points and the parallax that two_view_initialize reports for the winner"""
    s = T.general(300, 2)
    kp_ref, kp_cur, matches = T.as_keypoints(s)
    a, _ = _initialize(hip.host_lib(), "lpslam_two_view_initialize", T.K, kp_ref, kp_cur, matches, 1.0, 100, 12345)
    assert a["ok"][0] and a["model"][0] == 1
    R = np.stack([a["R"].reshape(3, 3)] * 2); t = np.stack([a["t"], -a["t"]])
    X, cosp, code = hip.two_view_check_poses_host(R, t, T.K, s["p1"], s["p2"], a["inlier"][:300], 4.0)
    tri = a["triangulated"][:300].astype(bool)
    assert np.array_equal(code[0] == 2, tri) and X[0][tri].tobytes() == a["points"][:300][tri].tobytes()
    assert np.isnan(X[0][code[0] == 0]).all() and (cosp[0][code[0] == 0] == 0).all() and not (code[0][a["inlier"][:300] == 0]).any()
    cs = np.sort(cosp[0][code[0] > 0])
    assert abs(np.degrees(np.arccos(min(1.0, cs[min(50, len(cs) - 1)]))) - a["parallax_deg"][0]) < 1e-9
    # t reversed: every point comes out mirrored, behind both cameras, with the same parallax (degrees here, far from the 0.99998 exemption)
    assert not code[1].any() and np.isnan(X[1]).all()
    with pytest.raises(hip.LpslamHipError):
        hip.two_view_check_poses_host(np.tile(np.eye(3), (9, 1, 1)), np.zeros((9, 3)), T.K, s["p1"], s["p2"], a["inlier"][:300], 4.0)
