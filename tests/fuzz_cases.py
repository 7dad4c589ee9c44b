"""Seeded random parity cases shared by tests/test_fuzz_gpu.py (bounded slices inside `-m gpu`) and the open-ended sweeps
tools/fuzz_parity.py / fuzz_ba.py / fuzz_pose.py / fuzz_sim3.py / fuzz_match.py.  Every case is a function of (seed, case index) alone: a failing case can be
re-run by its number.  Each `*_case` returns (ok, tag): the HIP path through the C ABI against the CPU oracle, bit for bit for
the front end and the matchers, within the tolerances of tests/test_ba_gpu.py for the optimisers (tests/sim3_cases.py for Sim3)."""
import numpy as np

import match_cases
import sim3_cases
from lpslam_amd import hip, synth

ROT_TOL, TRANS_TOL, CHI_RTOL = 1e-4, 1e-3, 1e-9


def _rng(seed, case):
    return np.random.default_rng([int(seed), int(case)])


def frontend_case(O, seed, case):
    """Random image size (every 7th very wide, every 11th very tall: many quad-tree roots, the 1531 x 97 kind), keypoint budget,
    level count, scale factor, FAST thresholds, image kind and mapping reserve (> 0: the queued kernels); extraction, brute-force
    and stereo matching against the oracle."""
    rng = _rng(seed, case)
    w = int(rng.integers(96, 900)); h = int(rng.integers(96, 600))
    if case % 7 == 3: w, h = int(rng.integers(700, 1600)), int(rng.integers(96, 170))
    if case % 11 == 5: w, h = int(rng.integers(96, 170)), int(rng.integers(500, 1000))
    levels = int(rng.integers(1, 9))
    scale = float(rng.choice([1.1, 1.2, 1.2, 1.3, 1.5, 2.0]))
    while levels > 1 and min(w, h) / scale ** (levels - 1) < 64: levels -= 1
    kpts = int(rng.integers(20, 1500))
    ini = int(rng.integers(5, 40)); mn = int(rng.integers(2, ini + 1))
    kind = int(rng.integers(0, 3))
    if kind == 0: img = synth.random_image(w, h, seed=int(rng.integers(1 << 30)))
    elif kind == 1: img = rng.integers(0, 256, (h, w)).astype(np.uint8)                 # white noise: corners everywhere
    else:
        img = synth.random_image(w, h, seed=int(rng.integers(1 << 30))); img[:, : w // 3] = 77   # a flat third: empty cells, min-threshold retries
    reserve = int(rng.choice([0, 4, 8, 16]))
    tag = "case %d: %dx%d levels %d scale %.1f kpts %d thr %d/%d kind %d reserve %d" % (case, w, h, levels, scale, kpts, ini, mn, kind, reserve)
    p = O.params(kpts, scale, levels, ini, mn)
    okp, od, occ, opyr = O.extract(img, p, True)
    ctx = hip.Context(w, h, kpts, scale, levels, ini, mn, max_images=2)
    try:
        if reserve: ctx.set_mapping_reserve(reserve)
        right_img = np.roll(img, -3, axis=1)
        ctx.upload(0, img); ctx.upload(1, right_img); ctx.extract(2)
        bad = [("pyramid %d" % l) for l in range(levels) if not np.array_equal(ctx.pyramid_level(0, l), opyr[l])]
        bad += [("fast %d" % l) for l in range(levels) if not np.array_equal(O.fast_level(opyr[l], ini, mn), ctx.candidates(0, l))]
        gkp, gd = ctx.keypoints(0)
        if not (len(gkp) == len(okp) and all(np.array_equal(okp[f], gkp[f]) for f in okp.dtype.names)): bad.append("keypoints")
        elif not np.array_equal(od, gd): bad.append("descriptors")
        rkp, rd, _, rpyr = O.extract(right_img, p, True)
        kp1, d1 = ctx.keypoints(1)
        if not (len(kp1) == len(rkp) and all(np.array_equal(rkp[f], kp1[f]) for f in rkp.dtype.names) and np.array_equal(rd, d1)): bad.append("right image")
        if len(gkp) and len(kp1):
            ctx.match_bf(0, 1)
            gq, gt, gdist = ctx.bf_matches(0, 1, 64, 0.8, True)
            oq, ot, odist = O.match_bf(od, rd, 64, 0.8, True)
            if not (np.array_equal(gq, oq) and np.array_equal(gt, ot) and np.array_equal(gdist, odist)): bad.append("bf")
        fxb, base = 40.0 * w / 640.0, 0.1
        if len(okp) and len(rkp):
            oxr, odep, obi, _ = O.match_stereo(opyr, rpyr, p, okp, od, rkp, rd, fxb, base)
            ctx.match_stereo(0, 1, fxb, base)
            gxr, gdep, gbi = ctx.stereo(0)
            if not (np.array_equal(gxr, oxr) and np.array_equal(gdep, odep) and np.array_equal(gbi, obi)): bad.append("stereo")
    finally:
        ctx.close()
    return not bad, tag + "  -> %d keypoints%s" % (len(okp), ("  failed: " + ",".join(bad)) if bad else "")


def _rot_err(q1, q2):
    return 2 * np.arccos(np.clip(np.abs(np.sum(q1 * q2, axis=1)), 0, 1))


def ba_case(O, ctx, seed, case, max_points=1500):
    """Random window (2 .. 51 keyframes), observation count, monocular share, inactive share, noise (rejected trials), robust on /
    off, duplicates, shuffled caller order, fixed-keyframe patterns; two thirds with tracks as a tracker makes them (band path)."""
    rng = _rng(seed, case)
    n_kf = int(rng.integers(2, 52)); n_pts = int(rng.integers(20, max_points))
    n_obs = int(min(n_kf * n_pts, rng.integers(2 * n_pts, 8 * n_pts + 1)))
    robust = bool(rng.integers(0, 2)); iters = int(rng.integers(1, 12))
    noise = float(rng.choice([1.0, 1.0, 3.0, 8.0]))
    tracks = "contiguous" if rng.integers(0, 3) else "random"
    prob = synth.ba_problem(n_kf, n_pts, n_obs, 640, 480, seq_id=int(rng.integers(1000)), pose_noise=(0.01 * noise, 0.05 * noise), point_noise=0.05 * noise,
                            tracks=tracks, top_up=bool(rng.integers(0, 2)))
    m = len(prob["obs_pose"])
    if rng.integers(0, 4) == 0:                                       # landmarks seen twice by a keyframe
        dup = rng.choice(m, max(1, m // 50), replace=False)
        for key in ("obs_pose", "obs_point", "obs_uvr", "obs_inv_sigma2"): prob[key] = np.concatenate([prob[key], prob[key][dup]])
        prob["obs_uvr"][m:, :2] += rng.normal(0, 0.3, (len(dup), 2)); m = len(prob["obs_pose"])
    if rng.integers(0, 3) == 0:                                       # caller order shuffled
        perm = rng.permutation(m)
        for key in ("obs_pose", "obs_point", "obs_uvr", "obs_inv_sigma2"): prob[key] = prob[key][perm]
    if rng.integers(0, 2): prob["obs_uvr"][rng.random(m) < 0.3, 2] = -1.0
    active = None
    if rng.integers(0, 2): active = (rng.random(m) > 0.15).astype(np.uint8)
    fx = int(rng.integers(0, 4))
    if fx == 0: prob["fixed"][rng.random(n_kf) < 0.3] = 1
    elif fx == 1: prob["fixed"][:int(rng.integers(1, max(2, n_kf // 2)))] = 1      # a tracker's window: the oldest observers are fixed
    elif fx == 2: prob["fixed"][:] = 0; prob["fixed"][int(rng.integers(0, n_kf))] = 1
    tag = "case %d: %s %d KF (%d free) %d pts %d obs robust %d iters %d noise %.0f" % (case, tracks, n_kf, int((prob["fixed"] == 0).sum()), n_pts, m, robust, iters, noise)
    obs = O.ba_obs(prob)
    op, ox, olog = O.ba_optimize(prob["poses"], prob["fixed"], prob["points"], obs, prob["cam"], robust, iters, active)
    ba = hip.BundleAdjuster(ctx, prob["poses"], prob["fixed"], prob["points"], hip.ba_obs_array(prob), prob["cam"])
    try:
        if active is not None: ba.set_active(active)
        glog = ba.optimize(robust, iters); gp, gx = ba.state()
        tag += " [%s %d]" % ba.solver()
    finally:
        ba.close()
    checks = {"len": len(glog) == len(olog)}
    if checks["len"]:
        checks.update(chi_before=np.allclose(glog["chi2_before"], olog["chi2_before"], rtol=CHI_RTOL),
                      chi_after=np.allclose(glog["chi2_after"], olog["chi2_after"], rtol=CHI_RTOL),
                      trials=np.array_equal(glog["trials"], olog["trials"]), status=np.array_equal(glog["status"], olog["status"]),
                      lam=np.allclose(glog["lambda"], olog["lambda"], rtol=1e-6),
                      rot=_rot_err(gp[:, :4], op[:, :4]).max() < ROT_TOL, trans=np.abs(gp[:, 4:] - op[:, 4:]).max() < TRANS_TOL,
                      pts=np.abs(gx - ox).max() < TRANS_TOL)
    ok = all(checks.values())
    if not ok:
        tag += "  failed: " + ",".join(k for k, v in checks.items() if not v)
    return ok, tag + "  trials %s" % (list(glog["trials"]),)


POSE_SIZES = [0, 1, 4, 5, 6, 30, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 2600, 2700, 2800, 3500]


def pose_case(O, ctx, seed, case):
    """lpslam_hip_pose_optimize against the oracle's pose_optimize: observation counts 0 ... beyond what the kernel keeps in LDS (the
    size classes first, then random), mono / stereo mixes, gross outliers, start poses off the truth.  A classification can sit on its
    threshold: a handful of flipped observations is tolerated when the poses agree to 1e-6 / 1e-5 m.  Returns (ok, tag, |dq|, |dt|)."""
    rng = _rng(seed, case)
    n = int(POSE_SIZES[case % len(POSE_SIZES)] if case < 2 * len(POSE_SIZES) else rng.integers(0, 1500))
    cam = dict(synth.intrinsics(640, 480)); cam_stereo = rng.random() < 0.7
    if not cam_stereo: cam["fxb"] = 0.0
    pts = np.stack([rng.uniform(-4, 4, max(n, 1)), rng.uniform(-3, 3, max(n, 1)), rng.uniform(2, 20, max(n, 1))], axis=1)
    yaw = rng.normal(0, 0.02); q = np.array([np.cos(yaw / 2), 0, np.sin(yaw / 2), 0]); t = rng.normal(0, 0.05, 3)
    R = np.array([[1 - 2 * q[2] ** 2, 0, 2 * q[0] * q[2]], [0, 1, 0], [-2 * q[0] * q[2], 0, 1 - 2 * q[2] ** 2]])
    pc = pts @ R.T + t
    obs = np.zeros(n, hip.BA_OBS_DTYPE)
    obs["point"] = np.arange(n)
    obs["u"] = cam["fx"] * pc[:n, 0] / pc[:n, 2] + cam["cx"] + rng.normal(0, 0.5, n)
    obs["v"] = cam["fy"] * pc[:n, 1] / pc[:n, 2] + cam["cy"] + rng.normal(0, 0.5, n)
    stereo = (rng.random(n) < 0.6) & cam_stereo
    obs["ur"] = np.where(stereo, obs["u"] - cam["fxb"] / pc[:n, 2] + rng.normal(0, 0.5, n), -1.0)
    obs["inv_sigma2"] = 1.0 / (1.2 ** (2 * rng.integers(0, 4, n)))
    out_idx = rng.random(n) < rng.choice([0.0, 0.1, 0.3])
    obs["v"][out_idx] += rng.choice([-1, 1], out_idx.sum()) * rng.uniform(15, 60, out_idx.sum())
    start = np.concatenate([[1, 0, 0, 0], rng.normal(0, 0.02, 3)])
    oobs = np.zeros(n, O.OBS_DTYPE)
    for f in oobs.dtype.names: oobs[f] = obs[f]
    opose, oout, oin = O.pose_optimize(start, pts, oobs, cam)
    kpose, kout, kin = hip.pose_optimize(ctx, start, pts, obs, cam)
    dr = float(np.abs(kpose[:4] - opose[:4]).max()); dt = float(np.abs(kpose[4:] - opose[4:]).max())
    same = kin == oin and np.array_equal(kout, oout.astype(bool))
    flips = int(np.sum(kout != oout.astype(bool)))
    ok = (same or flips <= max(1, n // 200)) and dr < 1e-6 and dt < 1e-5
    tag = "case %d: n %d stereo %s inliers %d / %d flips %d |dq| %.2e |dt| %.2e passes %d" % (case, n, cam_stereo, kin, oin, flips, dr, dt, ctx.pose_optimize_passes())
    return ok, tag, dr, dt


def sim3_case(O, ctx, seed, case):
    """lpslam_hip_sim3_* on an irregular pose graph (sim3_cases.irregular_graph: reversed and duplicated edges, a hub, fixed vertices
    anywhere in the numbering): 2 ... 70 vertices, 1 ... 3 of them fixed, the scale fixed or free, with or without scale drift; 12
    iterations on both sides, per-edge chi2, the logs over the oracle's converging prefix, final vertices, fixed vertices and fixed
    scales bit for bit.  The prefix is as long as the draw makes it: small graphs converge in two steps.  Where the oracle itself is
    not steady under a one-ulp change of its input (sim3_cases.oracle_wobble: most large graphs with the scale free), the logs are
    compared over the first iteration only and the final vertices not at all; the tag says so."""
    rng = _rng(seed, case)
    n = int(rng.integers(2, 71)); n_fixed = int(rng.integers(1, min(3, n - 1) + 1))
    fix_scale = bool(rng.integers(0, 2)); drift_scale = float(rng.choice([0.0, 0.01]))
    p = sim3_cases.irregular_graph(n, int(rng.integers(1 << 30)), n_fixed, fix_scale, drift_scale)
    steady = sim3_cases.oracle_is_steady(O, p, 12, trials=8)
    checks, info = sim3_cases.compare_graph(hip, O, ctx, p, 12, min_prefix=0, first_step_only=not steady)
    n_free = n - n_fixed
    nb, need = sim3_cases.panel_shape(n_free)
    tag = "case %d: n %d n_free %d nb %d need %d edges %d fix_scale %d drift_scale %g prefix %d%s" % (case, n, n_free, nb, need, info["n_edges"], fix_scale, drift_scale, info["prefix"], "" if steady else " (oracle unsteady)")
    ok = all(checks.values())
    if not ok:
        tag += "  failed: " + ",".join(k for k, v in checks.items() if not v)
    return ok, tag + "  |dq| %.1e |dt| %.1e trials %s" % (info["rot_dev"], info["trans_dev"], list(info["lg"]["trials"]))


WINDOW_LOG = {}      # (seed, case) -> what window_case saw: policy, skipped, the oracle's match count, the library's rescan count


def window_draw(O, seed, case):
    """The inputs of window_case, from the oracle alone: image size, level count, keypoint budget, image kind, frame 1 = frame 0 rolled by
    a few pixels and its right image, the matcher policy and its queries.  None when frame 0 has no keypoints."""
    rng = np.random.default_rng([int(seed), int(case), 8])
    w = int(rng.choice([320, 376, 640, 752, 333])); h = int(rng.choice([240, 480, 251]))
    levels = int(rng.integers(1, 9))
    while levels > 1 and min(w, h) / 1.2 ** (levels - 1) < 64: levels -= 1
    kpts = int(rng.integers(50, 1501))
    kind = int(rng.integers(0, 2))
    img0 = rng.integers(0, 256, (h, w)).astype(np.uint8) if kind == 0 else synth.random_image(w, h, seed=int(rng.integers(1 << 30)))
    img1 = np.roll(img0, (int(rng.integers(-4, 5)), int(rng.integers(-6, 7))), axis=(0, 1))
    right = np.roll(img1, -3, axis=1)
    ties = rng.random() < 0.4
    policy = match_cases.POLICIES[int(rng.integers(0, 3))]
    nq_draw = rng.choice([1, 3, 4, 5, 64, 200, -1], p=[.05, .05, .1, .1, .2, .2, .3])
    thr = int(rng.choice([50, 100, 256, 30, 0], p=[.3, .3, .2, .15, .05]))
    ratio = float(rng.choice([0.8, 0.9, 1.0, 0.6, 0.0], p=[.3, .3, .2, .15, .05]))
    use_stereo = bool(rng.integers(0, 2))
    taken_density = float(rng.choice([0.1, 0.5, 1.0])) if (policy == "projection" and rng.integers(0, 2)) else None
    p = O.params(kpts, 1.2, levels)
    kp0, d0, _, _ = O.extract(img0, p)
    tag = "case %d: %dx%d levels %d kpts %d kind %d ties %d %s thr %d ratio %.1f stereo %d taken %s" % (case, w, h, levels, kpts, kind, ties, policy, thr, ratio, use_stereo, taken_density)
    if len(kp0) == 0: return None, tag
    nq = len(kp0) if nq_draw < 0 else int(nq_draw)
    src = rng.integers(0, len(kp0), nq)
    sig = 1.0 if policy == "fuse" else 4.0
    near = rng.random(nq) < 0.8
    x = np.where(near, kp0["x"][src] + rng.normal(0, sig, nq), rng.uniform(-50, w + 50, nq))
    y = np.where(near, kp0["y"][src] + rng.normal(0, sig, nq), rng.uniform(-50, h + 50, nq))
    radius = np.exp(rng.uniform(np.log(4.0), np.log(300.0), nq))
    special = rng.random(nq) < 0.1
    radius = np.where(special, rng.choice([0.0, -5.0, 4000.0], nq), radius)
    open_levels = rng.random(nq) < 0.5
    lo = np.where(open_levels, -1, rng.integers(-1, levels + 1, nq)); hi = np.where(open_levels, -1, rng.integers(-1, levels + 1, nq))
    xr = np.where(rng.random(nq) < 0.5, x - 3.0 + rng.normal(0, 1.0, nq), -1.0)
    q = match_cases.queries(x, y, radius, lo, hi, xr)
    qd = d0[src].copy()
    proto = rng.integers(0, 256, (4, 32)).astype(np.uint8)
    if ties: qd[rng.random(nq) < 0.3] = proto[0]
    return dict(w=w, h=h, levels=levels, kpts=kpts, p=p, img1=img1, right=right, ties=ties, proto=proto, policy=policy, q=q, qd=qd, thr=thr, ratio=ratio,
                use_stereo=use_stereo, taken_density=taken_density, rng=rng), tag


def window_finish(d, n_kp, desc):
    """what depends on the matched frame's own keypoint count: the planted descriptors (30 % of the frame copies of four prototypes) and
    the `taken` mask"""
    rng = d["rng"]
    if d["ties"]:
        desc = desc.copy()
        planted = rng.random(n_kp) < 0.3
        desc[planted] = d["proto"][rng.integers(0, 4, int(planted.sum()))]
    taken = (rng.random(n_kp) < d["taken_density"]).astype(np.uint8) if d["taken_density"] is not None else None
    return desc, taken


def window_case(O, seed, case):
    """lpslam_hip_match_projection / _fuse / _area against the oracle's matchers, bit for bit (tests/match_cases.py): random image size
    (widths 376 and 752 among them: cell columns a float product misplaces), 1 ... 8 levels, 50 ... 1500 keypoints, white noise or a
    synthetic scene; the matched frame is frame 0 rolled by a few pixels, its right image that rolled by 3; in 40 % of the cases 30 %
    of the frame's descriptors are copies of four prototypes (ties, rescans).  1, 3, 4, 5, 64, 200 or as many queries as frame 0 has
    keypoints: 80 % near a keypoint of frame 0, the rest anywhere in the image grown by 50 px; radius 4 ... 300 log-uniform, one in
    ten 0, -5 or 4000; level bounds open or anything in -1 ... L, inverted pairs included; x_right on half the queries; thresholds
    and ratios at their ends (0, 256; 0.0, 1.0) now and then; a `taken` mask of density 0.1 / 0.5 / 1.0 in half the projection
    cases; the stereo column in half the cases.  A case whose frame has no keypoints is skipped.  Records itself in WINDOW_LOG."""
    d, tag = window_draw(O, seed, case)
    if d is None:
        WINDOW_LOG[(seed, case)] = dict(policy=None, skipped=True, matches=0, rescans=0)
        return True, tag + "  -> skipped (no keypoints)"
    ctx = hip.Context(d["w"], d["h"], d["kpts"], 1.2, d["levels"], max_images=2)
    try:
        fr, bad = match_cases.load_frame(O, ctx, d["p"], 0, d["img1"], 1, d["right"], 40.0 * d["w"] / 640.0, 0.1)
        if len(fr.kp) == 0:
            WINDOW_LOG[(seed, case)] = dict(policy=None, skipped=True, matches=0, rescans=0)
            return not bad, tag + "  -> skipped (no keypoints)" + ("  failed: " + ",".join(bad) if bad else "")
        desc, taken = window_finish(d, len(fr.kp), fr.desc)
        if d["ties"]: fr.set_descriptors(desc)
        use_stereo = d["use_stereo"] and fr.xr is not None
        why, (oi, od, on), rescans = match_cases.compare(O, fr, d["policy"], d["q"], d["qd"], d["thr"], d["ratio"], taken, use_stereo)
        if why: bad.append(why)
    finally:
        ctx.close()
    WINDOW_LOG[(seed, case)] = dict(policy=d["policy"], skipped=False, matches=int(on), rescans=int(rescans))
    return not bad, tag + "  -> %d keypoints, %d queries, %d matches, %d rescans%s" % (len(fr.kp), len(d["q"]), on, rescans, ("  failed: " + "; ".join(bad)) if bad else "")
