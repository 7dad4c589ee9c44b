"""Windows for the tests of the bundle adjuster's build (tests/test_ba_ref_cpu.py, tests/test_ba_build_gpu.py, tools/build_accuracy.py),
each small and named after what it pins.  Camera synth.intrinsics(640, 480); landmarks 2-20 m in front of the LAST keyframe (make() adds the window's
forward travel to every depth; mono_mix draws 8-20 m so that its landmark 1, at 2.3 m, holds the maximum of diag H_ll), keyframes one
frame apart (synth.StereoSequence.pose); measurements are exact projections plus noise, free keyframes and landmarks start perturbed -- the recipe
of test_ba_schur_parts_gpu.window.  numpy only.

    tiny         3 keyframes, the middle one fixed, 5 stereo landmarks seen by all (dim 12, padded 32)
    mono_mix     6 keyframes, first and last fixed, 40 landmarks, about half of the observations mono, order shuffled; landmark 0 has a
                 single mono observation, landmark 1 is seen by the two fixed keyframes only (and holds the maximum of diag H_ll), free
                 keyframe 4 has no observation
    huber_edges  4 keyframes, first and last fixed, 12 landmarks seen by all; observations planted at chi2 = delta^2 (1 -+ 1e-3), mono and stereo (PLANTED)
    inactive     mono_mix with a mask that drops about a third: all of landmark 5, all of keyframe 3
    slices_256   10 keyframes (0 fixed), free keyframe k sees the first c_k of 1025 landmarks, c = 0, 1, 63, 64, 65, 511, 512, 513, 1025;
    slices_257   the fixed keyframe sees 62 / 63, which makes the total 11 x 256 / one more
    pairs        4 free keyframes + 1 fixed; landmarks grouped by the two free keyframes that see them: lists of 0, 1, 31, 32, 33, 64 terms
                 off the diagonal, 32, 65, 97, 128 on it
    dupes        keyframe 1 observes landmark 3 twice (lpslam_hip_ba_create takes such a window: a case, not a refusal test)
    parts_129    4 keyframes that all see every one of n landmarks: two and three parts of k_ba_schur, a ragged last round
    parts_257
    wide         64 free keyframes and 2 fixed (7 and 40), four frames apart, 600 landmarks with random tracks of 2-5 keyframes
    band         12 keyframes, first and last fixed, every landmark seen by 2-4 consecutive ones
    batch40      BATCH40: 40 windows of the tiny and pairs kind, other seeds
"""
import functools

import numpy as np

import ba_ref
from lpslam_amd import synth

W, H = 640, 480
BAND_MAX_HBW, BAND_MAX_DIM = 9, 304          # csrc/ba_band.inl: BD_MAXHBW, bc_fits
SLICE_COUNTS = (0, 1, 63, 64, 65, 511, 512, 513, 1025)
PAIR_TERMS = {(0, 1): 0, (0, 2): 1, (0, 3): 31, (1, 2): 32, (1, 3): 33, (2, 3): 64}


def _rng(*key):
    return np.random.Generator(np.random.PCG64([synth.SEED_BASE + 4242] + [int(k) for k in key]))


def make(n_kf, fixed, n_pts, pairs, seed, mono=None, shuffle=False, depth=(2.0, 20.0), stride=1):
    """The problem dictionary of synth.ba_problem for the (keyframe, landmark) pairs given; `mono`: mask over the pairs."""
    rng = _rng(seed)
    k = synth.intrinsics(W, H)
    seq = synth.StereoSequence(W, H, 0, n_points=1)
    Rs, ts = zip(*[seq.pose(stride * i) for i in range(n_kf)])
    ahead = 0.05 * stride * (n_kf - 1)                                   # the last keyframe still has every landmark >= depth[0] in front of it
    z = rng.uniform(depth[0], depth[1], n_pts) + ahead
    lat = depth[0] / (depth[0] + ahead)
    X = np.stack([z * rng.uniform(-0.5, 0.5, n_pts) * lat, z * rng.uniform(-0.38, 0.38, n_pts) * lat, z], axis=1)
    obs = np.asarray(pairs, np.int64).reshape(-1, 2)
    mono = np.zeros(len(obs), bool) if mono is None else np.asarray(mono, bool)
    if shuffle:
        order = rng.permutation(len(obs))
        obs, mono = obs[order], mono[order]
    uv = np.zeros((len(obs), 3))
    for i in range(n_kf):
        m = obs[:, 0] == i
        pc = X[obs[m, 1]] @ Rs[i].T + ts[i]
        u = k["fx"] * pc[:, 0] / pc[:, 2] + k["cx"]
        uv[m] = np.stack([u, k["fy"] * pc[:, 1] / pc[:, 2] + k["cy"], u - k["fxb"] / pc[:, 2]], axis=1)
    sigma = 1.2 ** rng.integers(0, 8, len(obs))
    meas = uv + rng.normal(0, 1.0, (len(obs), 3)) * sigma[:, None]
    assert (meas[:, 2] > 0).all()                                   # a negative right coordinate means "mono" to the library
    meas[mono, 2] = -1.0
    fx = np.zeros(n_kf, np.uint8); fx[list(fixed)] = 1
    poses_gt = np.array([np.concatenate([synth.rot_to_quat(Rs[i]), ts[i]]) for i in range(n_kf)])
    poses = poses_gt.copy()
    for i in range(n_kf):
        if not fx[i]:
            dR = synth._small_rot(rng.normal(0, 0.01, 3))
            poses[i] = np.concatenate([synth.rot_to_quat(dR @ Rs[i]), dR @ ts[i] + rng.normal(0, 0.05, 3)])
    return dict(poses=poses, poses_gt=poses_gt, points=X + rng.normal(0, 0.05, (n_pts, 3)), points_gt=X, fixed=fx,
                obs_pose=obs[:, 0].astype(np.int32), obs_point=obs[:, 1].astype(np.int32), obs_uvr=meas.astype(np.float64),
                obs_inv_sigma2=(1.0 / sigma ** 2).astype(np.float64), cam=dict(fx=k["fx"], fy=k["fy"], cx=k["cx"], cy=k["cy"], fxb=k["fxb"]))


def all_see(n_kf, n_pts):
    return [(f, j) for j in range(n_pts) for f in range(n_kf)]


def tiny(seed=1):
    return make(3, [1], 5, all_see(3, 5), seed)


def mono_mix(seed=2):
    rng = _rng(seed, 1)
    seen = (0, 1, 2, 3, 5)                                       # keyframe 4 is free and sees nothing
    pairs = [(1, 0), (0, 1), (5, 1)]
    for j in range(2, 40):
        pairs += [(int(f), j) for f in np.sort(rng.choice(seen, rng.integers(2, 6), replace=False))]
    mono = rng.random(len(pairs)) < 0.5
    mono[0] = True; mono[1:3] = False
    pr = make(6, [0, 5], 40, pairs, seed, mono, shuffle=True, depth=(8.0, 20.0))
    # landmark 1 close to the cameras, with unit weights: the largest diagonal entry of H_ll belongs to it
    k = pr["cam"]
    X = np.array([0.1, -0.1, 2.3])
    pr["points_gt"][1] = X; pr["points"][1] = X + np.array([0.002, -0.002, 0.004])
    for o in np.nonzero(pr["obs_point"] == 1)[0]:
        q, t = pr["poses"][pr["obs_pose"][o], :4], pr["poses"][pr["obs_pose"][o], 4:]
        pc = ba_ref._rot(q[None].astype(np.float64), np.float64)[0] @ X + t
        u = k["fx"] * pc[0] / pc[2] + k["cx"]
        pr["obs_uvr"][o] = [u + 0.3, k["fy"] * pc[1] / pc[2] + k["cy"] - 0.2, u - k["fxb"] / pc[2] + 0.1]
        pr["obs_inv_sigma2"][o] = 1.0
    return pr


INACTIVE_LANDMARK, INACTIVE_KEYFRAME = 5, 3


def inactive_mask(pr, seed=3):
    rng = _rng(seed, 2)
    act = rng.random(len(pr["obs_pose"])) > 0.2
    act[(pr["obs_point"] == INACTIVE_LANDMARK) | (pr["obs_pose"] == INACTIVE_KEYFRAME)] = False
    act[pr["obs_point"] <= 1] = True                             # (the single mono observation and the fixed-only landmark stay)
    return act.astype(np.uint8)


# (observation index, mono, side): side -1 sits at delta^2 (1 - 1e-3), +1 at delta^2 (1 + 1e-3)
PLANTED = ((1, True, -1), (5, True, +1), (10, False, -1), (14, False, +1), (22, True, +1), (26, False, -1))


def huber_edges(seed=14):
    n_kf, n_pts = 4, 12
    pairs = all_see(n_kf, n_pts)
    mono = np.zeros(len(pairs), bool)
    for o, m, _ in PLANTED:
        mono[o] = m
    pr = make(n_kf, [0, 3], n_pts, pairs, seed, mono)          # (a second fixed keyframe: the census' step bar)
    LD = ba_ref.LD
    for o, m, side in PLANTED:
        assert pr["fixed"][pr["obs_pose"][o]] == 0
        pr["obs_inv_sigma2"][o] = 1.0
        target = np.sqrt(LD(ba_ref.CHI2_MONO if m else ba_ref.CHI2_STEREO) * (1 + LD(side) * LD(1e-3)))
        e, _, _, _, _ = ba_ref.residuals(pr, pr["poses"], pr["points"], LD)
        proj = pr["obs_uvr"][o].astype(LD) - e[o]                # the projection in long double
        d = np.array([0.6, -0.64, 0.0 if m else 0.48], LD)
        d = d / np.sqrt((d * d).sum())
        new = (proj + target * d).astype(np.float64)
        pr["obs_uvr"][o] = [new[0], new[1], -1.0 if m else new[2]]
    return pr


def slices(fixed_sees, seed=5):
    pairs = [(0, j) for j in range(fixed_sees)]
    for kf, c in enumerate(SLICE_COUNTS):
        pairs += [(kf + 1, j) for j in range(c)]
    return make(10, [0], 1025, pairs, seed)


def pairs_window(seed=6):
    pairs, j = [], 0
    for (a, b), n in PAIR_TERMS.items():
        for _ in range(n):
            pairs += [(a + 1, j), (b + 1, j)] + ([(0, j)] if j % 2 == 0 else [])      # keyframe 0 is the fixed one
            j += 1
    return make(5, [0], j, pairs, seed)


DUPE_KEYFRAME, DUPE_LANDMARK = 1, 3


def dupes(seed=7):
    pr = make(4, [0], 10, all_see(4, 10) + [(DUPE_KEYFRAME, DUPE_LANDMARK)], seed)
    return pr


def parts(n, seed=8):
    return make(4, [0], n, all_see(4, n), seed + n)


def wide(seed=9):
    rng = _rng(seed, 1)
    pairs = []
    for j in range(600):
        pairs += [(int(f), j) for f in np.sort(rng.choice(66, rng.integers(2, 6), replace=False))]
    return make(66, [7, 40], 600, pairs, seed, stride=4)       # (keyframes four frames apart: the parallax the census' step bar needs)


def band(seed=30):
    rng = _rng(seed, 1)
    pairs = []
    for j in range(120):
        n = int(rng.integers(2, 5)); f0 = int(rng.integers(0, 12 - n + 1))
        pairs += [(f, j) for f in range(f0, f0 + n)]
    return make(12, [0, 11], 120, pairs, seed)                 # (a second fixed keyframe: the census' step bar)


BUILDERS = {"tiny": tiny, "mono_mix": mono_mix, "huber_edges": huber_edges, "inactive": mono_mix,
            "slices_256": lambda: slices(62), "slices_257": lambda: slices(63), "pairs": pairs_window, "dupes": dupes,
            "parts_129": lambda: parts(129), "parts_257": lambda: parts(257), "wide": wide, "band": band}
NAMES = tuple(BUILDERS)
STEP_API = tuple(n for n in NAMES if n != "band")                 # 4a: every case but band and batch40
PRODUCT = ("tiny", "mono_mix", "inactive", "pairs", "parts_129", "parts_257", "wide", "band")      # 4b
# seeds from 100 on; of the tiny kind (3 keyframes, 5 landmarks) only the draws whose derived step bar meets the census' 1e-6 are taken
TINY_SEEDS = (109, 114, 115, 123, 140, 144, 151, 153, 154, 157, 163, 173, 175, 176, 181, 183, 185, 197, 198, 201)
BATCH40 = tuple(("tiny", TINY_SEEDS[i // 2]) if i % 2 == 0 else ("pairs", 100 + i // 2) for i in range(40))


@functools.lru_cache(maxsize=None)
def problem(name):
    pr = BUILDERS[name]()
    for v in pr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def batch_problem(i):
    kind, seed = BATCH40[i]
    return tiny(seed) if kind == "tiny" else pairs_window(seed)


@functools.lru_cache(maxsize=None)
def mask(name):
    return inactive_mask(problem(name)) if name == "inactive" else None


@functools.lru_cache(maxsize=None)
def reference(name, robust=True, dt=ba_ref.LD):
    """(lin, red, st) of the case's first trial, computed once"""
    pr = batch_problem(int(name[1:])) if name.startswith("#") else problem(name)
    return ba_ref.first_trial(pr, robust, None if name.startswith("#") else mask(name), dt)


# ---- what the structure implies ---------------------------------------------------------------------------------------------
def free_span(pr):
    slot, _ = ba_ref.slots(pr)
    sl = slot[pr["obs_pose"]]
    free = sl >= 0
    lo = np.full(len(pr["points"]), 1 << 30); hi = np.full(len(pr["points"]), -1)
    np.minimum.at(lo, pr["obs_point"][free], sl[free]); np.maximum.at(hi, pr["obs_point"][free], sl[free])
    return int((hi - lo)[hi >= 0].max()) if (hi >= 0).any() else 0


def implied_solver(pr):
    """what lpslam_hip_ba_create chooses: the band path when no landmark spans more than 9 free slots and the system has at most 304 unknowns"""
    dim = 6 * int((pr["fixed"] == 0).sum())
    span = free_span(pr)
    return ("band", span) if 0 < dim <= BAND_MAX_DIM and span <= BAND_MAX_HBW and len(pr["obs_pose"]) else ("dense", -1)


def pair_terms(pr, active=None):
    """terms of every pose-block pair list, free keyframes i x k, counted on the CPU"""
    free = np.nonzero(pr["fixed"] == 0)[0]
    A = np.zeros((len(pr["poses"]), len(pr["points"])), np.int64)
    act = np.ones(len(pr["obs_pose"]), bool) if active is None else np.asarray(active, bool)
    np.add.at(A, (pr["obs_pose"][act], pr["obs_point"][act]), 1)
    return A[free] @ A[free].T


# ---- the bars (tests/test_ba_build_gpu.py states them) ----------------------------------------------------------------------
U = 2.0 ** -53


def entry_terms(lin, red):
    """terms behind every entry of S (its pair list's; a diagonal block adds the keyframe's observation count) and of rhs"""
    t = red["terms"].astype(np.float64) + np.diag(lin["obs_count"].astype(np.float64))
    return np.kron(t, np.ones((6, 6))), np.repeat(np.diag(t), 6)


def rel_err(x, ref, T):
    """max |x - ref| / T over the entries with T > 0, in long double; entries with T == 0 must be exact zeros"""
    x, ref, T = np.asarray(x, ba_ref.LD), np.asarray(ref, ba_ref.LD), np.asarray(T, ba_ref.LD)
    pos = T > 0
    exact = bool((x[~pos] == 0).all())
    return (float((np.abs(x - ref)[pos] / T[pos]).max()) if pos.any() else 0.0), exact


def step_scales(st, lin):
    """||step||_inf of rotation, translation and points"""
    xp = np.asarray(st["xp"], np.float64).reshape(-1, 6)
    return (float(np.abs(xp[:, :3]).max()) if len(xp) else 0.0, float(np.abs(xp[:, 3:]).max()) if len(xp) else 0.0, float(np.abs(st["xl"]).max()))


def derived(T, t, c):
    """(t + c) 2^-53 T"""
    return U * (np.asarray(t, np.float64) + c) * np.asarray(T, np.float64)


def system_bars(lin, red, c):
    """The derived bars of every entry of S and of rhs: (t + c) kappa_l 2^-53 T with kappa_l taken to 1 on the parts of T that
    (H_ll + lam I)^-1 does not multiply -- H_pp in S; b_p and b_l's own rounding in the rhs, where kappa_l stays on the product with |b_l|
    itself.  T = S_pp_abs + S_sc_abs (rhs alike), so no entry's bar is larger than (t + c) kappa_l 2^-53 T."""
    tS, tr = entry_terms(lin, red)
    k = max(red["kappa_l"], 1.0)
    bS = derived(red["S_pp_abs"] + k * red["S_sc_abs"], tS, c)
    br = derived(red["rhs_pp_abs"] + red["rhs_sc_abs"] + k * red["rhs_sc_k"], tr, c)
    return bS, br


def lin_bars(lin, c):
    """b_p, diag H_pp, chi2, max diag H_ll: (t + c) 2^-53 T; t = the keyframe's observations, all active ones for chi2, the landmark's for
    the maximum (no more than the number of keyframes: that is used)"""
    t = np.repeat(lin["obs_count"].astype(np.float64), 6)
    n_act = float(lin["act"].sum())
    return dict(bp=derived(lin["bp_abs"], t, c), hpp=derived(lin["hpp_diag_abs"], t, c),
                chi2=float(derived(lin["chi2_abs"], n_act, c)), max_ll=float(derived(lin["max_ll_abs"], len(lin["slot"]), c)))


def step_bars(lin, red, st, c):
    """kappa_2(S + lambda I) ((the bars of S and rhs relative to their norms) + n 2^-53) ||step||_inf, for rotation, translation, points"""
    bS, br = system_bars(lin, red, c)
    A = red["S"].astype(np.float64) + float(red["lam"]) * np.eye(lin["dim"])
    rhs = red["rhs"].astype(np.float64)
    rel = np.linalg.norm(bS, 2) / np.linalg.norm(A, 2) + np.linalg.norm(br) / max(np.linalg.norm(rhs), 1e-300) + lin["dim"] * U
    plain = [st["kappa_s"] * rel * s for s in step_scales(st, lin)]
    # The same first-order bound in the variables y = D^1/2 x, D = diag(S + lambda I), read back entry by entry: |dx_i| <= ||dy||_2 / sqrt(d_i).
    # A keyframe without observations has lambda alone on its block and kappa_2 of the unscaled matrix measures that gap of scales
    # (7e4 in mono_mix and slices), not how the step reacts; each bar is the smaller of the two bounds.
    d = np.sqrt(np.diag(A))
    xp = st["xp"].astype(np.float64)
    As = A / np.outer(d, d)
    rels = np.linalg.norm(bS / np.outer(d, d), 2) / np.linalg.norm(As, 2) + np.linalg.norm(br / d) / max(np.linalg.norm(rhs / d), 1e-300) + lin["dim"] * U
    dx = np.linalg.cond(As) * rels * np.linalg.norm(d * xp) / d
    dxb = dx.reshape(-1, 6)
    rot, tr = min(plain[0], float(dxb[:, :3].max())), min(plain[1], float(dxb[:, 3:].max()))
    # points: x_l = (H_ll + lambda I)^-1 (b_l - W^T x_p) takes the poses' bar through |H^-1 W^T| and its own rounding through kappa_l
    pts = plain[2]
    if len(dx):
        both = np.minimum(dx, np.repeat([[plain[0]] * 3 + [plain[1]] * 3], len(dxb), 0).reshape(-1))
        sl = lin["slot"]
        pr_pose, pr_point = lin["obs_pose"], lin["obs_point"]
        fr = (sl[pr_pose] >= 0) & lin["act"]
        G = np.abs(np.einsum("nij,nkj->nik", red["Hinv"][pr_point[fr]], lin["W"][fr]).astype(np.float64))      # 3 x 6 per observation
        acc = np.zeros((len(lin["points"]), 3))
        np.add.at(acc, pr_point[fr], np.einsum("nik,nk->ni", G, both.reshape(-1, 6)[sl[pr_pose[fr]]]))
        own = red["kappa_l"] * (c + len(sl)) * U * np.abs(st["xl"].astype(np.float64))
        pts = min(pts, float((acc + own).max()))
    return rot, tr, pts


def state_errors(poses, points, ref_poses, ref_points, free):
    """(rotation in rad, translation, points): largest distance of the free poses' and the points' entries"""
    q, r = np.asarray(poses, ba_ref.LD)[free, :4], np.asarray(ref_poses, ba_ref.LD)[free, :4]
    sgn = np.sign((q * r).sum(1))[:, None]
    rot = float(2 * np.abs(q - sgn * r).max()) if len(q) else 0.0
    tr = float(np.abs(np.asarray(poses, ba_ref.LD)[free, 4:] - np.asarray(ref_poses, ba_ref.LD)[free, 4:]).max()) if len(q) else 0.0
    return rot, tr, float(np.abs(np.asarray(points, ba_ref.LD) - np.asarray(ref_points, ba_ref.LD)).max())
