"""The part size k_ba_schur cuts a dense window's pose-block pair lists by (csrc/ba.hip schur_parts, chosen per window by
k_bs_blkscan): every boundary of the cut, a window whose capacity binds, the same bytes alone / in a batch / twice,
batch-built windows, and the choice surviving graph replays with rejected trials.  Tolerances are those of test_ba_gpu.py: chi2
trajectory relative 1e-9, identical trials / status, lambda relative 1e-6, poses within 1e-4 rad / 1e-3 m of the CPU oracle."""
import numpy as np
import pytest

from lpslam_amd import synth

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL, CHI_RTOL = 1e-4, 1e-3, 1e-9
SPLIT = 8                                                   # leading pose-side workgroups per keyframe (csrc/ba.hip)
CANDIDATES = (128, 160, 192, 224)                           # part sizes with at most 8 parts; else 256 with at most 4
ITERS = 3
# terms of every pair list of the small windows (4 keyframes, 1 fixed, every landmark seen by all): one part | exactly one part |
# two parts | two full parts | three parts | more than 8 parts' worth: the cap, with a ragged last round
BOUNDARY_TERMS = (127, 128, 129, 256, 257, 8 * 128 + 1)
CAPACITY_WINDOW = (40, 1400, 18)                            # keyframes, landmarks, random observers of each


def rot_err(q1, q2):
    return 2 * np.arccos(np.clip(np.abs(np.sum(q1 * q2, axis=1)), 0, 1))


def window(n_kf, n_pts, observers=None, seed=0):
    """Keyframes one frame apart, landmarks every keyframe can see; each observed by all keyframes or by `observers` random ones.
    The same dictionary synth.ba_problem returns."""
    rng = np.random.Generator(np.random.PCG64([synth.SEED_BASE + seed, 11]))
    w, h = 640, 480
    k = synth.intrinsics(w, h)
    seq = synth.StereoSequence(w, h, seed, n_points=1)
    Rs, ts = zip(*[seq.pose(i) for i in range(n_kf)])
    cand = np.stack([rng.uniform(-12, 12, n_pts * 8), rng.uniform(-4, 4, n_pts * 8), rng.uniform(4.0, 30.0, n_pts * 8)], axis=1)
    vis = np.ones(len(cand), bool)
    uvs = np.zeros((len(cand), n_kf, 3))
    for i in range(n_kf):
        pc = cand @ Rs[i].T + ts[i]
        z = pc[:, 2]
        zs = np.where(z > 0.5, z, 0.5)
        u = k["fx"] * pc[:, 0] / zs + k["cx"]; v = k["fy"] * pc[:, 1] / zs + k["cy"]
        vis &= (z > 1.0) & (z < 40.0) & (u >= 20) & (u < w - 20) & (v >= 20) & (v < h - 20)
        uvs[:, i] = np.stack([u, v, u - k["fxb"] / zs], axis=1)
    good = np.nonzero(vis)[0][:n_pts]
    assert len(good) == n_pts, "not enough landmarks every keyframe sees: %d" % len(good)
    if observers is None:
        pairs = [(f, j) for j in range(n_pts) for f in range(n_kf)]
    else:
        pairs = [(f, j) for j in range(n_pts) for f in np.sort(rng.choice(n_kf, observers, replace=False))]
    obs = np.array(pairs)
    sigma = 1.2 ** rng.integers(0, 8, len(obs))
    meas = uvs[good[obs[:, 1]], obs[:, 0]] + rng.normal(0, 1.0, (len(obs), 3)) * sigma[:, None]
    poses_gt = np.array([np.concatenate([synth.rot_to_quat(Rs[i]), ts[i]]) for i in range(n_kf)])
    poses = poses_gt.copy()
    for i in range(1, n_kf):
        dR = synth._small_rot(rng.normal(0, 0.01, 3))
        poses[i] = np.concatenate([synth.rot_to_quat(dR @ Rs[i]), dR @ ts[i] + rng.normal(0, 0.05, 3)])
    fixed = np.zeros(n_kf, np.uint8); fixed[0] = 1
    return dict(poses=poses, points=cand[good] + rng.normal(0, 0.05, (n_pts, 3)), fixed=fixed,
                obs_pose=obs[:, 0].astype(np.int32), obs_point=obs[:, 1].astype(np.int32), obs_uvr=meas.astype(np.float64),
                obs_inv_sigma2=(1.0 / sigma ** 2).astype(np.float64), cam=dict(fx=k["fx"], fy=k["fy"], cx=k["cx"], cy=k["cy"], fxb=k["fxb"]))


def pair_terms(pr):
    """terms of every pose-block pair list (free keyframes i <= k), counted on the CPU"""
    free = np.nonzero(pr["fixed"] == 0)[0]
    A = np.zeros((len(pr["poses"]), len(pr["points"])), np.int64)
    np.add.at(A, (pr["obs_pose"], pr["obs_point"]), 1)
    cnt = A[free] @ A[free].T
    return cnt[np.triu_indices(len(free))]


def further_parts(terms, part):
    limit = 4 if part >= 256 else 8
    return int(sum(min(-(-int(n) // part), limit) - 1 for n in terms if n > part))


def rule(terms, capacity):
    """the smallest candidate whose further parts fit the capacity, else 256"""
    for part in CANDIDATES:
        if further_parts(terms, part) <= capacity:
            return part
    return 256


@pytest.fixture(scope="module")
def ctx(hiplib):
    return hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)


@pytest.fixture(scope="module")
def windows():
    w = {("all", n): window(4, n, None, seed=n) for n in BOUNDARY_TERMS}
    w[("capacity",)] = window(*CAPACITY_WINDOW, seed=7)
    return w


@pytest.fixture(scope="module")
def oracle_results(oracle, windows):
    """every window's CPU solve, computed once"""
    return {key: oracle.ba_optimize(pr["poses"], pr["fixed"], pr["points"], oracle.ba_obs(pr), pr["cam"], True, ITERS) for key, pr in windows.items()}


def _make(hiplib, ctx, pr, build=True):
    """the window on the dense path (four keyframes that all see every landmark are block-banded and would take the band path)"""
    ba = hiplib.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hiplib.ba_obs_array(pr), pr["cam"], build=build)
    if build:
        ba.set_solver("dense")
    return ba


def _against(ores, glog, gp, gx):
    op, ox, olog = ores
    assert len(glog) == len(olog)
    assert np.allclose(glog["chi2_before"], olog["chi2_before"], rtol=CHI_RTOL)
    assert np.allclose(glog["chi2_after"], olog["chi2_after"], rtol=CHI_RTOL)
    assert np.array_equal(glog["trials"], olog["trials"]) and np.array_equal(glog["status"], olog["status"])
    assert np.allclose(glog["lambda"], olog["lambda"], rtol=1e-6)
    assert rot_err(gp[:, :4], op[:, :4]).max() < ROT_TOL and np.abs(gp[:, 4:] - op[:, 4:]).max() < TRANS_TOL
    assert np.abs(gx - ox).max() < TRANS_TOL


@pytest.mark.parametrize("n", BOUNDARY_TERMS)
def test_parts_at_every_boundary(hiplib, ctx, windows, oracle_results, n):
    pr = windows[("all", n)]
    terms = pair_terms(pr)
    assert len(terms) == 6 and (terms == n).all(), "every list of the window is meant to hold %d terms" % n
    ba = _make(hiplib, ctx, pr)
    assert ba.solver()[0] == "dense"
    part, capacity = ba.schur_part()
    assert capacity >= further_parts(terms, 128), "a small window is not meant to meet the capacity"
    assert part == 128
    glog = ba.optimize(True, ITERS)
    _against(oracle_results[("all", n)], glog, *ba.state())
    ba.close()


def test_capacity_binds(hiplib, ctx, windows, oracle_results):
    pr = windows[("capacity",)]
    terms = pair_terms(pr)
    ba = _make(hiplib, ctx, pr)
    assert ba.solver()[0] == "dense"
    part, capacity = ba.schur_part()
    assert further_parts(terms, 128) > capacity > 0, "the window is meant to have more further parts at 128 (%d) than fit (%d)" % (further_parts(terms, 128), capacity)
    assert part == rule(terms, capacity) and part > 128
    assert part == 256 or further_parts(terms, part) <= capacity      # the launch stays one generation of workgroups
    glog = ba.optimize(True, ITERS)
    _against(oracle_results[("capacity",)], glog, *ba.state())
    ba.close()


@pytest.mark.parametrize("key", [("all", n) for n in BOUNDARY_TERMS] + [("capacity",)], ids=lambda k: "-".join(str(x) for x in k))
def test_same_bytes_alone_in_a_batch_and_twice(hiplib, ctx, windows, key):
    pr = windows[key]
    ba = _make(hiplib, ctx, pr)
    part = ba.schur_part()[0]
    glog = ba.optimize(True, ITERS)
    gp, gx = ba.state()
    ba.reset()
    again = ba.optimize(True, ITERS)
    ap, ax = ba.state()
    assert again.tobytes() == glog.tobytes() and ap.tobytes() == gp.tobytes() and ax.tobytes() == gx.tobytes()
    mates = [windows[("all", 129 if key != ("all", 129) else 127)], windows[("all", 257 if key != ("all", 257) else 256)]]
    batch = [_make(hiplib, ctx, mates[0]), _make(hiplib, ctx, pr), _make(hiplib, ctx, mates[1])]
    assert batch[1].schur_part()[0] == part
    logs = hiplib.ba_optimize_batch(batch, True, ITERS)
    bp, bx = batch[1].state()
    assert logs[1].tobytes() == glog.tobytes() and bp.tobytes() == gp.tobytes() and bx.tobytes() == gx.tobytes()
    for b in batch + [ba]:
        b.close()


def test_batch_built_windows_get_the_part_of_single_builds(hiplib, ctx, windows, oracle_results):
    """Windows whose structure is built by one lpslam_hip_ba_build_batch of several.  The first plan was that they keep 256; then
    tests/test_ba_gpu.py::test_batched_build_equals_single_builds, which asks a batch-built window for the bytes of the same window
    built alone, cannot hold (two cuts sum S in two groupings), and it is the older promise.  So a batch-built window reports the
    part size, and gives the bytes, of the same window built alone -- the boundary windows 128, the window whose capacity binds its
    larger size -- and follows the oracle."""
    keys = [("all", 257), ("capacity",), ("all", 8 * 128 + 1)]
    bas = [_make(hiplib, ctx, windows[k], build=False) for k in keys]
    hiplib.ba_build_batch(bas)
    for ba, k in zip(bas, keys):
        ba.set_solver("dense")
        alone = _make(hiplib, ctx, windows[k])
        assert ba.schur_part() == alone.schur_part() and (ba.schur_part()[0] == 128) == (k != ("capacity",))
        glog = ba.optimize(True, ITERS)
        gp, gx = ba.state()
        alog = alone.optimize(True, ITERS)
        ap, ax = alone.state()
        assert alog.tobytes() == glog.tobytes() and ap.tobytes() == gp.tobytes() and ax.tobytes() == gx.tobytes()
        _against(oracle_results[k], glog, gp, gx)
        ba.close(); alone.close()


def test_rejected_trials_keep_the_part_choice(hiplib, oracle):
    """A window whose fifth iteration rejects trials (lambda-only units), its lists of up to ~150 terms cut at 128, through
    optimize_begin / optimize_end until the launch graph is replayed: the part size is chosen once by the build, and every round
    gives the first round's bytes and follows the oracle."""
    pr = synth.ba_problem(6, 150, 800, 640, 480, seq_id=46, pose_noise=(0.5, 3.0), point_noise=3.0)
    iters = 10
    assert pair_terms(pr).max() > 128
    own = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)
    ba = _make(hiplib, own, pr)
    part = ba.schur_part()[0]
    assert part == 128
    before = own.ba_counters()["replays"]
    rounds = []
    for _ in range(4):
        ba.reset()
        ba.optimize_begin(True, iters)
        log = ba.optimize_end()
        rounds.append((log,) + ba.state())
    assert own.ba_counters()["replays"] - before >= 2, "the later rounds were meant to replay the captured graph"
    assert ba.schur_part()[0] == part
    first = rounds[0]
    assert first[0]["trials"].max() > 1
    _against(oracle.ba_optimize(pr["poses"], pr["fixed"], pr["points"], oracle.ba_obs(pr), pr["cam"], True, iters), *first)
    for log, p, x in rounds[1:]:
        assert log.tobytes() == first[0].tobytes() and p.tobytes() == first[1].tobytes() and x.tobytes() == first[2].tobytes()
    ba.close(); own.close()
