"""CPU tests of the triangulation step between keyframes: the host forms of lpslam_amd/csrc/triangulate_math.h
against tests/triangulate_ref.py on the planted pairs and sets of tests/triangulate_cases.py, the tracker option's range, the
neighbour list and the baseline gate, and the stand-alone sanitizer program tests/cpp/triangulate_host_main.cpp."""
import os
import subprocess

import numpy as np
import pytest

import triangulate_cases as tc
import triangulate_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest relative distance between the reference's SVD triangulation and its own Jacobi-on-A^T A restatement over the planted
# code-1 pairs, measured (7.88e-14 over 500 pairs) and rounded up; the code under test gets four times that, for the contraction a
# compiler may apply.  Codes 2 and 3 are a back-projection: 1e-12.
SVD_JACOBI_DEVIATION = 8.0e-14
TOL_TRIANGULATED = 4.0 * SVD_JACOBI_DEVIATION
TOL_BACK_PROJECTED = 1e-12
WANTED_REASONS = {"ok1", "ok2", "ok3", "parallax", "cos<=0", "depth1", "depth2", "reproj1", "reproj2", "reproj1_stereo", "reproj2_stereo", "ratio_low", "ratio_high"}


@pytest.fixture(scope="module")
def mgr(hiplib):
    from lpslam_amd import _build, manager
    _build.host_library()
    manager.load()
    return manager


def check_planted_pairs():
    """what both the CPU and the GPU test first establish about the planted set; returns the references"""
    refs = tc.pair_reference()
    every = [r for g in refs for r in g["svd"]]
    assert 1900 <= len(every) <= 2100
    assert {r["reason"] for r in every} == WANTED_REASONS                    # every code and every rejection is reached
    excluded = sum(r["margin"] < 1e-9 for r in every)
    assert excluded == 0                                                     # no tested quantity within 1e-9 (relative) of its bound
    assert min(r["parallax_deg"] for r in every if r["code"] == 1) >= 1.0
    # a rejected view sees the other kind of bound too: with and without the right-image term, in either view
    measured, n = tc.svd_jacobi_deviation()
    print("SVD against Jacobi on A^T A: %.3e over %d triangulated pairs" % (measured, n))
    assert n >= 400 and measured <= 1e-9 and measured <= SVD_JACOBI_DEVIATION
    return refs


def assert_pairs(group, refs, code, X):
    want = np.array([r["code"] for r in refs["svd"]])
    assert np.array_equal(code, want), (group["name"], np.flatnonzero(code != want)[:10])
    assert np.isnan(X[code == 0]).all()
    worst = {1: 0.0, 2: 0.0, 3: 0.0}
    for k, r in enumerate(refs["svd"]):
        if r["code"]:
            worst[r["code"]] = max(worst[r["code"]], float(np.linalg.norm(X[k] - r["X"]) / np.linalg.norm(r["X"])))
    print("%-16s relative distance from the reference: code 1 %.2e, code 2 %.2e, code 3 %.2e" % (group["name"], worst[1], worst[2], worst[3]))
    assert worst[1] <= TOL_TRIANGULATED and worst[2] <= TOL_BACK_PROJECTED and worst[3] <= TOL_BACK_PROJECTED, (group["name"], worst)


def test_host_pairs_match_reference(mgr):
    refs = check_planted_pairs()
    for g, r in zip(tc.planted_pairs(), refs):
        code, X = mgr.tri_pair_host(g["cam"].as6(), tc.SCALE, g["pose1"], g["pose2"], g["k1"], g["k2"])
        assert_pairs(g, r, code, X)


HOST_SHAPES = [(0, 65, 1), (65, 0, 1), (1, 1, 1), (63, 64, 3), (64, 65, 3), (65, 63, 1), (257, 257, 3)]


def host_lists(mgr, cam, q, s, q_depth=None):
    return mgr.tri_candidates_host(cam.as6(), tc.SCALE, tc.to_tri_keypoints(q["kp"], depth=q_depth), q["desc"], q["group"],
                                   tc.to_tri_keypoints(s["kpts"], s["x_right"], s["depth"]), s["desc"], s["group"], s["F"], s["epipole"])


@pytest.mark.parametrize("groups", ["zero", "vocab"])
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_host_candidate_lists_match_reference(mgr, shape, groups):
    cam, q, sets = tc.planted_sets(*shape, groups=groups)
    for s, (j, dist, count) in zip(sets, tc.reference_lists(cam, q, sets)):
        hj, hd, hc, keys = host_lists(mgr, cam, q, s)
        assert np.array_equal(hc, count) and np.array_equal(hj, j) and np.array_equal(hd, dist)
        match, rank, exhausted = mgr.tri_replay_host(keys, hc, len(s["kpts"]))
        rm, rr, re_ = tr.replay(j, count, len(s["kpts"]))
        assert np.array_equal(match, rm) and np.array_equal(rank, rr) and exhausted == re_


def test_planted_edge_cases_are_there_and_agree(mgr):
    cam, q, sets = tc.planted_sets(257, 257, 3, groups="vocab", degenerate=(1,), no_epipole=(2,))
    ref = tc.reference_lists(cam, q, sets)
    for s, (j, dist, count) in zip(sets, ref):
        hj, hd, hc, _ = host_lists(mgr, cam, q, s)
        assert np.array_equal(hc, count) and np.array_equal(hj, j) and np.array_equal(hd, dist)
    j, dist, count = ref[0]
    assert count.max() > tr.LISTED and (j[count > tr.LISTED] >= 0).all()        # more passed than are listed: the count says so
    ties = [(i, r) for i in range(len(j)) for r in range(tr.LISTED - 1) if j[i, r + 1] >= 0 and dist[i, r] == dist[i, r + 1]]
    assert ties and all(j[i, r] < j[i, r + 1] for i, r in ties)                 # equal distances: the lower index first
    assert (count[q["group"] < 0] == 0).all() and (q["group"] < 0).any()
    assert ref[1][2].sum() == 0                                                 # the degenerate line passes nothing
    # the epipole rule: the same set without an epipole, and with stereo keypoints, lets the keypoints next to it through
    s0 = dict(sets[0]); s0["epipole"] = None
    assert host_lists(mgr, cam, q, s0)[2].sum() > count.sum()
    cam_s, q_s, sets_s = tc.planted_sets(257, 257, 1, groups="vocab", target_stereo=True)
    js, ds, cs = tc.reference_lists(cam_s, q_s, sets_s)[0]
    hj, hd, hc, _ = host_lists(mgr, cam_s, q_s, sets_s[0])
    assert np.array_equal(hc, cs) and np.array_equal(hj, js)
    mono = dict(sets_s[0]); mono["depth"] = None; mono["x_right"] = None
    assert tc.reference_lists(cam_s, q_s, [mono])[0][2].sum() < cs.sum()
    # a stereo QUERY switches the rule off as well
    depth_q = np.full(len(q_s["kp"]), 6.0, np.float32)
    jq, dq, cq = tc.reference_lists(cam_s, q_s, [mono], q_depth=depth_q)[0]
    hj, hd, hc, _ = host_lists(mgr, cam_s, q_s, mono, q_depth=depth_q)
    assert np.array_equal(hc, cq) and np.array_equal(hj, jq) and cq.sum() > tc.reference_lists(cam_s, q_s, [mono])[0][2].sum()


def test_replay_exhausts_a_list_whose_candidates_are_taken():
    """nine queries with the same eight candidates and a count above eight: the ninth finds its list used up"""
    j = np.tile(np.arange(8, dtype=np.int32), (9, 1)); count = np.full(9, 12, np.int32)
    match, rank, exhausted = tr.replay(j, count, 20)
    assert list(match) == list(range(8)) + [-1] and exhausted == 1
    count[8] = 8                                                                 # everything that passed is listed: not counted
    assert tr.replay(j, count, 20)[2] == 0


def test_replay_host_form(mgr):
    j = np.tile(np.arange(8, dtype=np.int64), (9, 1)); keys = ((np.arange(8, dtype=np.uint64) + np.uint64(3)) << np.uint64(32)) | j.astype(np.uint64)
    count = np.full(9, 12, np.int32)
    match, rank, exhausted = mgr.tri_replay_host(keys, count, 20)
    assert list(match) == list(range(8)) + [-1] and list(rank) == list(range(8)) + [-1] and exhausted == 1
    skip = np.zeros(9, np.uint8); skip[0] = 1                                    # a query that is not served leaves its candidate to the next
    match, rank, exhausted = mgr.tri_replay_host(keys, count, 20, skip)
    assert list(match) == [-1] + list(range(8)) and exhausted == 0


def test_epipolar_geometry_of_the_tracker(mgr):
    cam = tc.CAM_MONO
    for s in range(6):
        pose = tc.neighbour_pose(s)
        F, ep = mgr.tri_epipolar(cam.as6(), tc.ORIGIN, pose)
        Fr, epr = tr.epipolar(cam, tc.ORIGIN, pose)
        assert np.abs(F - Fr).max() <= 1e-12 * np.abs(Fr).max() and np.allclose(ep, epr, rtol=1e-12)
        X = np.array([[0.4, -0.3, 6.0], [-1.0, 0.5, 9.0]])
        u1, v1, _ = tr.project(cam, tc.ORIGIN, X); u2, v2, _ = tr.project(cam, pose, X)
        for k in range(2):
            l = F @ np.array([u1[k], v1[k], 1.0])
            assert abs(l @ np.array([u2[k], v2[k], 1.0])) / np.hypot(l[0], l[1]) < 1e-9      # x_n^T F x_c = 0, in pixels
    sideways = tr.look_pose([0.5, 0.0, 0.0])                                     # c's centre has z = 0 in n's frame
    assert mgr.tri_epipolar(cam.as6(), tc.ORIGIN, sideways)[1] is None and tr.epipolar(cam, tc.ORIGIN, sideways)[1] is None


def test_option_range(mgr):
    assert all(mgr.tri_option_ok(n) for n in (0, 1, 10, 20, 32))
    assert not any(mgr.tri_option_ok(n) for n in (-1, 33, 100, -2 ** 31))


def test_neighbour_list_and_baseline_gate_on_a_hand_built_map(mgr):
    """six keyframes on a line 0.1 m apart, the new one (c = 6) at 0.6 m; its covisible list is [1, 3, 4]"""
    cov = [1, 3, 4]
    assert mgr.tri_neighbour_list(cov, -1, 10) == [1, 3, 4]                       # stereo: the list as it is
    assert mgr.tri_neighbour_list(cov, 5, 10) == [5, 1, 3, 4]                     # monocular: the previous keyframe in front
    assert mgr.tri_neighbour_list(cov, 3, 10) == [1, 3, 4]                        # ... unless it is there already
    assert mgr.tri_neighbour_list(cov, 5, 3) == [5, 1, 3] and mgr.tri_neighbour_list(cov, -1, 2) == [1, 3]
    assert mgr.tri_neighbour_list([], 5, 20) == [5] and mgr.tri_neighbour_list([], -1, 20) == []
    poses = [tr.look_pose([0.1 * k, 0.0, 0.0], yaw=0.03 * k) for k in range(7)]
    # stereo: the true baseline 0.12 m -- keyframe 5 (0.1 m away) is skipped, keyframe 4 (0.2 m) is served
    assert not mgr.tri_baseline_accepts(poses[6], poses[5], 0.12) and mgr.tri_baseline_accepts(poses[6], poses[4], 0.12)
    assert mgr.tri_baseline_accepts(poses[6], poses[4], 0.2 - 1e-9) and not mgr.tri_baseline_accepts(poses[6], poses[4], 0.2 + 1e-9)
    # monocular: baselineDistThresh x the median depth of the neighbour's landmarks (the lower median of an even count)
    assert mgr.tri_median_depth([4.0, 9.0, 2.0]) == 4.0 and mgr.tri_median_depth([4.0, 9.0, 2.0, 7.0]) == 4.0 and mgr.tri_median_depth([]) == -1.0
    median = mgr.tri_median_depth([3.0, 5.0, 8.0])
    assert mgr.tri_baseline_accepts(poses[6], poses[4], 0.02 * median) and not mgr.tri_baseline_accepts(poses[6], poses[4], 0.1 * median)


def _kp_line(k):
    return "%r %r %d %r %r" % (float(k["x"]), float(k["y"]), int(k["octave"]), float(k["x_right"]), float(k["depth"]))


def test_standalone_sanitizer_program(mgr, tmp_path):
    """tests/cpp/triangulate_host_main.cpp: the host forms in a program of its own, built with -fsanitize=address,undefined, over the
    planted pairs and three planted sets with the reference's answers"""
    cases = tmp_path / "cases.txt"
    refs = tc.pair_reference()
    n_pairs = 0
    with open(cases, "w") as f:
        f.write(" ".join(repr(float(v)) for v in tc.CAM_MONO.as6()) + "\n")
        f.write("%d %s\n" % (len(tc.SCALE), " ".join(repr(float(v)) for v in tc.SCALE)))
        f.write("%r %d\n" % (TOL_TRIANGULATED, len(refs)))
        for g, r in zip(tc.planted_pairs(), refs):
            f.write("%r %s %s %d\n" % (g["cam"].fxb, " ".join(repr(float(v)) for v in g["pose1"]), " ".join(repr(float(v)) for v in g["pose2"]), len(g["k1"])))
            for a, b, w in zip(g["k1"], g["k2"], r["svd"]):
                X = w["X"] if w["code"] else (0.0, 0.0, 0.0)
                f.write("%s %s %d %r %r %r\n" % (_kp_line(a), _kp_line(b), w["code"], float(X[0]), float(X[1]), float(X[2])))
                n_pairs += 1
        cam, q, sets = tc.planted_sets(65, 257, 3, groups="vocab", degenerate=(1,), no_epipole=(2,))
        f.write("%d\n" % len(sets))
        n_lists = 0
        for s, (j, dist, count) in zip(sets, tc.reference_lists(cam, q, sets)):
            ep = s["epipole"]
            f.write("%d %d %d %r %r %s\n" % (len(q["kp"]), len(s["kpts"]), 0 if ep is None else 1, 0.0 if ep is None else float(ep[0]), 0.0 if ep is None else float(ep[1]),
                                              " ".join(repr(float(v)) for v in np.asarray(s["F"]).reshape(9))))
            for kp, desc, grp in ((tc.to_tri_keypoints(q["kp"]), q["desc"], q["group"]), (tc.to_tri_keypoints(s["kpts"]), s["desc"], s["group"])):
                for k, d, g_ in zip(kp, desc, grp):
                    f.write("%s %d %s\n" % (_kp_line(k), int(g_), " ".join(str(int(b)) for b in d)))
            match, rank, exhausted = tr.replay(j, count, len(s["kpts"]))
            for i in range(len(j)):
                keys = [(int(dist[i, r]) << 32) | int(j[i, r]) if j[i, r] >= 0 else 2 ** 64 - 1 for r in range(tr.LISTED)]
                f.write("%d %d %d %s\n" % (int(count[i]), int(match[i]), int(rank[i]), " ".join(str(k) for k in keys)))
                n_lists += 1
            f.write("%d\n" % exhausted)
    exe = tmp_path / "triangulate_host_main"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "triangulate_host_main.cpp")])
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pairs ok %d" % n_pairs in out.stdout and "lists ok %d" % n_lists in out.stdout, out.stdout
