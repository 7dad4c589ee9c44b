"""The bundle adjuster at its solver and capacity limits (FP64, against the CPU oracle with the tolerances of test_ba_gpu.py).

Which kernels solve a problem depends on its size: the one-launch update (k_ba_update) takes at most UPD_MAXP = 320 keyframes,
a landmark-major block holds 256 CSR entries unless one landmark has more, the band path needs a block half-bandwidth <= 9 and
dim <= 304, k_chol_wg needs dim + 1 <= 304, a call runs at most 64 iterations.  Every test here sits on or next to one of those
limits and asserts the path it took as well as the numbers, so that it cannot pass by taking the path next to the one it is about."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from lpslam_amd import synth
from test_ba_gpu import CHI_RTOL, ROT_TOL, TRANS_TOL, _compare, rot_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS_KEYS = ("obs_pose", "obs_point", "obs_uvr", "obs_inv_sigma2")


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(640, 480, 500, 1.2, 4, max_images=1)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _close_problems(request):
    """every problem a test creates on the module's context is destroyed when the test ends, whether or not it passed"""
    c = request.getfixturevalue("ctx") if "ctx" in request.fixturenames else None
    before = set(c._children) if c is not None else set()
    yield
    if c is not None:
        for child in list(c._children):
            if child not in before:
                child.close()


# ---- problems -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _global(n_kf, tracks="random"):
    """a global-BA-sized map (BASELINE config 5's landmarks and observations) with n_kf keyframes; callers copy before changing it"""
    return synth.ba_problem(n_kf, 30000, 240000, 1920, 1080, seq_id=2, kf_stride=2, tracks=tracks)


def _copy(prob):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in prob.items()}


def _quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _add_heavy_landmarks(prob, counts, seed):
    """`counts[i]` more observations of the i-th most observed landmark, each by a keyframe that already sees it (repeated (keyframe,
    landmark) pairs, the landmark's span of keyframes unchanged), projected from the ground truth with fresh pixel noise"""
    rng = np.random.default_rng(seed)
    cam = prob["cam"]
    deg = np.bincount(prob["obs_point"], minlength=len(prob["points"]))
    heavy = np.argsort(-deg, kind="stable")[:len(counts)]
    add = {k: [] for k in OBS_KEYS}
    for j, n in zip(heavy, counts):
        kfs = rng.choice(prob["obs_pose"][prob["obs_point"] == j], n)
        for f in kfs:
            pc = _quat_to_rot(prob["poses_gt"][f, :4]) @ prob["points_gt"][j] + prob["poses_gt"][f, 4:]
            u = cam["fx"] * pc[0] / pc[2] + cam["cx"]
            v = cam["fy"] * pc[1] / pc[2] + cam["cy"]
            add["obs_uvr"].append(np.array([u, v, u - cam["fxb"] / pc[2]]) + rng.normal(0, 1.0, 3))
            add["obs_pose"].append(f); add["obs_point"].append(j); add["obs_inv_sigma2"].append(1.0)
    out = _copy(prob)
    for k in OBS_KEYS:
        out[k] = np.concatenate([prob[k], np.asarray(add[k], prob[k].dtype).reshape((-1,) + prob[k].shape[1:])])
    assert np.bincount(out["obs_point"]).max() > 256
    return out


def _free_spans(prob):
    """first / last FREE keyframe slot of every landmark that has an observation by a free keyframe"""
    free = prob["fixed"] == 0
    slot = np.where(free, np.cumsum(free) - 1, -1)
    s = slot[prob["obs_pose"]]
    keep = s >= 0
    j, s = prob["obs_point"][keep], s[keep]
    lo = np.full(len(prob["points"]), 1 << 30); hi = np.full(len(prob["points"]), -1)
    np.minimum.at(lo, j, s); np.maximum.at(hi, j, s)
    seen = hi >= 0
    return lo[seen], hi[seen], np.nonzero(seen)[0]


def _half_bandwidth(prob):
    """block half-bandwidth of the reduced system: the widest span of free slots a landmark covers"""
    lo, hi, _ = _free_spans(prob)
    return int((hi - lo).max())


def _band_groups(prob, gmax, maxkf=10):
    """landmark groups of the band path: landmarks by (first free slot, id), cut at gmax landmarks or a window of maxkf keyframes"""
    lo, hi, _ = _free_spans(prob)
    order = np.lexsort((np.arange(len(lo)), lo))
    groups, q = 0, 0
    while q < len(order):
        f0, last, cnt = lo[order[q]], lo[order[q]], 0
        while q + cnt < len(order) and cnt < gmax:
            l2 = max(last, hi[order[q + cnt]])
            if l2 - f0 + 1 > maxkf:
                break
            last = l2; cnt += 1
        groups += 1; q += cnt
    return groups


# ---- checks ---------------------------------------------------------------------------------------------------------------

_ORACLE = {}


def _oracle_opt(oracle, key, prob, robust, iters, active=None):
    """oracle.ba_optimize; with a `key` (a name for the problem, not for a run of it) computed once per (key, robust, iters) --
    the global-size problems take seconds in the oracle.  A keyed run has every observation active."""
    if key is None:
        return oracle.ba_optimize(prob["poses"], prob["fixed"], prob["points"], oracle.ba_obs(prob), prob["cam"], robust, iters, active)
    assert active is None
    full = (key, bool(robust), int(iters))
    if full not in _ORACLE:
        _ORACLE[full] = oracle.ba_optimize(prob["poses"], prob["fixed"], prob["points"], oracle.ba_obs(prob), prob["cam"], robust, iters)
    return _ORACLE[full]


def _check(glog, gp, gx, want):
    op, ox, olog = want
    assert len(glog) == len(olog)
    # relative tolerances only: np.allclose's default atol of 1e-8 would accept any lambda once it has fallen below it (~1e-29
    # after 64 accepted iterations), and any chi2 of a problem that fits to that level
    assert np.allclose(glog["chi2_before"], olog["chi2_before"], rtol=CHI_RTOL, atol=0)
    assert np.allclose(glog["chi2_after"], olog["chi2_after"], rtol=CHI_RTOL, atol=0)
    assert np.array_equal(glog["trials"], olog["trials"]) and np.array_equal(glog["status"], olog["status"])
    assert np.allclose(glog["lambda"], olog["lambda"], rtol=1e-6, atol=0)
    assert rot_err(gp[:, :4], op[:, :4]).max() < ROT_TOL and np.abs(gp[:, 4:] - op[:, 4:]).max() < TRANS_TOL
    assert len(gx) == 0 or np.abs(gx - ox).max() < TRANS_TOL


def _make(hiplib, ctx, prob, solver=None):
    b = hiplib.BundleAdjuster(ctx, prob["poses"], prob["fixed"], prob["points"], hiplib.ba_obs_array(prob), prob["cam"])
    if solver:
        b.set_solver(solver)
    return b


def _update_path(hiplib, ctx, prob, robust=True, iters=3, solver=None, active=None):
    """launches of (k_ba_update, k_ba_backsub, k_ba_trial) in a profiled run of a separate problem object"""
    b = _make(hiplib, ctx, prob, solver)
    try:
        if active is not None:
            b.set_active(active)
        prof, _, _ = b.optimize_profiled(robust, iters)
    finally:
        b.close()
    return tuple(prof.get(k, (0.0, 0, 0))[1] for k in ("k_ba_update", "k_ba_backsub", "k_ba_trial"))


def _one_pass(path):
    return path[0] > 0 and path[1] == 0


def _two_launch(path):
    return path[0] == 0 and path[1] > 0 and path[2] > 0


def _run_child(tmp_path, which, env_extra, timeout=420):
    """_child_main(which) in a fresh process (the switches below are read once per process); its results come back as an .npz"""
    out = str(tmp_path / ("%s.npz" % which))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from lpslam_amd import _build, hip\n_build.hip_library(); hip.load()\n"
            "import test_ba_limits_gpu as t\n"
            "t._child_main(hip, %r, %r)\n"
            "print('VARIANT-OK')\n") % (ROOT, os.path.join(ROOT, "tests"), which, out)
    env = dict(os.environ); env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "VARIANT-OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    return dict(np.load(out)), r.stderr


# ---- 1. either side of UPD_MAXP ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kf,tracks", [(320, "random"), (321, "random"), (321, "contiguous")])
def test_either_side_of_the_one_launch_update_limit(hiplib, oracle, ctx, n_kf, tracks):
    """320 keyframes are the most k_ba_update holds (UPD_MAXP): that map takes the one-launch update, 321 the two-launch form
    (k_ba_backsub + k_ba_trial) with free keyframes -- what every global BA of a larger map runs.  10 iterations against the oracle."""
    prob = _global(n_kf, tracks)
    assert abs(len(prob["obs_pose"]) - 240000) <= 0.05 * 240000
    path = _update_path(hiplib, ctx, prob)
    assert _one_pass(path) if n_kf <= 320 else _two_launch(path), path
    ba = _make(hiplib, ctx, prob)
    assert ba.solver() == ("dense", -1)
    glog = ba.optimize(True, 10)
    gp, gx = ba.state()
    _check(glog, gp, gx, _oracle_opt(oracle, (n_kf, tracks), prob, True, 10))
    assert len(glog) == 10 and glog["chi2_after"][-1] < glog["chi2_before"][0]
    assert ba.timeouts() == (0, 0)
    ba.close()


# ---- 2. the two-launch form forced on the windows that normally take the one-launch update ------------------------------------

def _small_cases():
    """(name, problem, kind, robust, iters, active, solver): windows that take k_ba_update by default"""
    dense = synth.ba_problem(12, 600, 4000, 640, 480, seq_id=21)
    band = synth.ba_problem(14, 500, 2600, 640, 480, seq_id=6, tracks="contiguous")
    rejected = synth.ba_problem(6, 150, 800, 640, 480, seq_id=46, pose_noise=(0.5, 3.0), point_noise=3.0)
    mono = synth.ba_problem(7, 200, 1100, 640, 480, seq_id=3)
    mono["obs_uvr"][::3, 2] = -1.0
    active = np.ones(len(mono["obs_pose"]), np.uint8); active[::5] = 0
    local = synth.ba_problem(8, 300, 1800, 640, 480, seq_id=9)
    local["obs_uvr"][np.arange(0, len(local["obs_pose"]), 29), 0] += 35.0
    heavy = _add_heavy_landmarks(synth.ba_problem(9, 300, 2000, 640, 480, seq_id=31), (257, 600), seed=3)
    return [("dense", dense, "opt", True, 8, None, "dense"), ("band", band, "opt", True, 8, None, None),
            ("rejected", rejected, "opt", True, 10, None, None), ("mono", mono, "opt", True, 6, active, None),
            ("local", local, "local", True, 5, None, None), ("heavy", heavy, "opt", True, 8, None, "dense")]


def _run_small_cases(hiplib, ctx):
    res = {}
    for name, prob, kind, robust, iters, active, solver in _small_cases():
        b = _make(hiplib, ctx, prob, solver)
        if active is not None:
            b.set_active(active)
        if kind == "local":
            res[name + "_out"] = b.local(5, 10)
        else:
            res[name + "_log"] = b.optimize(robust, iters)
        res[name + "_poses"], res[name + "_points"] = b.state()
        res[name + "_path"] = np.array(_update_path(hiplib, ctx, prob, robust, iters, solver, active))
        res[name + "_solver"] = np.array(b.solver()[0])
        res[name + "_timeouts"] = np.array(b.timeouts())
        b.close()
    return res


def _child_main(hiplib, which, out):
    ctx = hiplib.Context(640, 480, 500, 1.2, 4, max_images=1)
    if which == "two_launch":
        res = _run_small_cases(hiplib, ctx)
    else:
        res = {}
        for name, prob in _group_cases():
            b = _make(hiplib, ctx, prob)
            res[name + "_log"] = b.optimize(True, 8)
            res[name + "_poses"], res[name + "_points"] = b.state()
            res[name + "_solver"] = np.array(b.solver())
            b.close()
    ctx.close()
    np.savez(out, **res)


def test_forced_two_launch_update_matches_the_oracle_and_the_one_launch_form(hiplib, oracle, ctx, tmp_path):
    """LPSLAM_HIP_BA_TWO_LAUNCH_UPDATE=1 (read once per process, so in a child process) sends the windows that normally take
    k_ba_update through k_ba_backsub + k_ba_trial: dense, band, rejected trials, mono + inactive observations, the local flow with
    outliers and a window with landmarks of more than 256 observations.  Each follows the oracle, and the two forms agree to rounding
    (they sum in different orders, so not to the bit): the same LM decisions; chi2 and lambda within 1e-13 relative, poses within
    1e-12, landmarks within 5e-11 (measured on an MI355X: 1.5e-14, 4.3e-14 and 6.8e-12 at most)."""
    want = _run_small_cases(hiplib, ctx)
    got, _ = _run_child(tmp_path, "two_launch", {"LPSLAM_HIP_BA_TWO_LAUNCH_UPDATE": "1"})
    for name, prob, kind, robust, iters, active, solver in _small_cases():
        assert _one_pass(tuple(want[name + "_path"])), (name, want[name + "_path"])
        assert _two_launch(tuple(got[name + "_path"])), (name, got[name + "_path"])
        assert str(got[name + "_solver"]) == str(want[name + "_solver"]), name
        assert name != "band" or str(got[name + "_solver"]) == "band"
        assert tuple(got[name + "_timeouts"]) == (0, 0) and tuple(want[name + "_timeouts"]) == (0, 0)
        gp, gx = got[name + "_poses"], got[name + "_points"]
        wp, wx = want[name + "_poses"], want[name + "_points"]
        if kind == "local":
            obs = oracle.ba_obs(prob)
            op, ox, oout = oracle.ba_local(prob["poses"], prob["fixed"], prob["points"], obs, prob["cam"], 5, 10)
            assert np.array_equal(got[name + "_out"], oout) and np.array_equal(want[name + "_out"], oout), name
            assert rot_err(gp[:, :4], op[:, :4]).max() < ROT_TOL and np.abs(gp[:, 4:] - op[:, 4:]).max() < TRANS_TOL
            assert np.abs(gx - ox).max() < TRANS_TOL, name
        else:
            glog, wlog = got[name + "_log"], want[name + "_log"]
            _check(glog, gp, gx, _oracle_opt(oracle, None, prob, robust, iters, active))
            assert np.array_equal(glog["trials"], wlog["trials"]) and np.array_equal(glog["status"], wlog["status"]), name
            assert np.allclose(glog["chi2_after"], wlog["chi2_after"], rtol=1e-13, atol=0), (name, glog["chi2_after"] / wlog["chi2_after"] - 1)
            assert np.allclose(glog["lambda"], wlog["lambda"], rtol=1e-13, atol=0), name
        assert np.abs(gp - wp).max() <= 1e-12 and np.abs(gx - wx).max() <= 5e-11, (name, np.abs(gp - wp).max(), np.abs(gx - wx).max())


# ---- 3. landmarks with more than 256 observations -------------------------------------------------------------------------

def test_landmarks_with_more_than_256_observations(hiplib, oracle, ctx):
    """A landmark-major block holds more than 256 CSR entries when one landmark has more: the update walks them in further chunks.
    A dense window and a band window (one-launch update) and the 321-keyframe map (two-launch form), each with landmarks of
    257..600 observations, against the oracle."""
    dense = _add_heavy_landmarks(synth.ba_problem(9, 300, 2000, 640, 480, seq_id=31), (257, 600, 300), seed=1)
    band0 = synth.ba_problem(14, 500, 2600, 640, 480, seq_id=6, tracks="contiguous")
    band = _add_heavy_landmarks(band0, (257, 512, 513), seed=2)
    assert _half_bandwidth(band) == _half_bandwidth(band0) <= 9
    for prob, solver, iters in ((dense, "dense", 8), (band, None, 8)):
        assert np.bincount(prob["obs_point"]).max() > 256
        assert _one_pass(_update_path(hiplib, ctx, prob, solver=solver))
        if solver:
            ba = _make(hiplib, ctx, prob, solver)
            glog = ba.optimize(True, iters)
            gp, gx = ba.state()
            _check(glog, gp, gx, _oracle_opt(oracle, None, prob, True, iters))
        else:
            ba, _, _, _ = _compare(hiplib, oracle, ctx, prob, True, iters)
            assert ba.solver() == ("band", _half_bandwidth(prob))
        assert ba.timeouts() == (0, 0)
        ba.close()
    big = _add_heavy_landmarks(_global(321), (257, 400, 600), seed=4)
    assert _two_launch(_update_path(hiplib, ctx, big))
    ba = _make(hiplib, ctx, big)
    glog = ba.optimize(True, 10)
    gp, gx = ba.state()
    _check(glog, gp, gx, _oracle_opt(oracle, ("heavy", 321), big, True, 10))
    ba.close()


# ---- 4. band limits -------------------------------------------------------------------------------------------------------

def test_band_half_bandwidth_limit(hiplib, oracle, ctx):
    """Tracks of 10 keyframes give a widest span of 9 free slots: the band path, ("band", 9); of 11, a span of 10: the dense path.
    The span is computed from the observations, not assumed."""
    at = synth.ba_problem(20, 600, 6000, 640, 480, seq_id=60, tracks="contiguous")
    over = synth.ba_problem(20, 600, 6600, 640, 480, seq_id=60, tracks="contiguous")
    assert _half_bandwidth(at) == 9 and _half_bandwidth(over) == 10
    ba, _, _, _ = _compare(hiplib, oracle, ctx, at, True, 8)
    assert ba.solver() == ("band", 9)
    ba.close()
    ba, _, _, _ = _compare(hiplib, oracle, ctx, over, True, 8)
    assert ba.solver() == ("dense", -1)
    with pytest.raises(hiplib.LpslamHipError):
        ba.set_solver("band")
    ba.close()
    # a fixed keyframe inside the window takes no slot: the same tracks span one slot less across it
    fx = synth.ba_problem(20, 600, 6600, 640, 480, seq_id=61, tracks="contiguous")
    assert _half_bandwidth(fx) == 10
    fx["fixed"][:] = 0; fx["fixed"][[0, 10]] = 1
    hb = _half_bandwidth(fx)
    assert hb <= 9, hb
    ba, _, _, _ = _compare(hiplib, oracle, ctx, fx, True, 8)
    assert ba.solver() == ("band", hb)
    ba.close()


def test_band_dimension_limit(hiplib, oracle, ctx):
    """51 keyframes, one fixed: dim 300 <= 304, the band path; 52 keyframes: dim 306, the dense path whatever the bandwidth."""
    for n_kf, want in ((51, "band"), (52, "dense")):
        prob = synth.ba_problem(n_kf, 5000, 40000, 1280, 720, seq_id=n_kf, tracks="contiguous", top_up=True)
        hb = _half_bandwidth(prob)
        assert hb <= 9 and int((prob["fixed"] == 0).sum()) * 6 == 6 * (n_kf - 1)
        ba, _, _, glog = _compare(hiplib, oracle, ctx, prob, True, 8)
        assert ba.solver() == ((want, hb) if want == "band" else ("dense", -1))
        if want == "dense":
            with pytest.raises(hiplib.LpslamHipError):
                ba.set_solver("band")
        assert ba.timeouts() == (0, 0)
        ba.close()


def _group_cases():
    return [("hbw9", synth.ba_problem(20, 600, 6000, 640, 480, seq_id=60, tracks="contiguous")),
            ("dim300", synth.ba_problem(51, 5000, 40000, 1280, 720, seq_id=51, tracks="contiguous", top_up=True)),
            ("heavy", _add_heavy_landmarks(synth.ba_problem(14, 500, 2600, 640, 480, seq_id=6, tracks="contiguous"), (257, 512), seed=2))]


@pytest.mark.parametrize("group", [4, 64])
def test_band_group_size_limits(hiplib, oracle, tmp_path, group):
    """LPSLAM_HIP_BA_GROUP (landmarks per k_schur_group workgroup, 4..64; read once per process) at both ends: the windows are cut
    into the groups the plan promises (the creation trace says how many) and follow the oracle."""
    got, err = _run_child(tmp_path, "group%d" % group, {"LPSLAM_HIP_BA_GROUP": str(group), "LPSLAM_HIP_BA_TRACE": "1"})
    traced = [int(line.split(" groups")[0].rsplit(" ", 1)[1]) for line in err.splitlines() if "[lpslam_hip_ba_create]" in line and "-> band" in line]
    cases = _group_cases()
    # one creation per case, in order: the trace's i-th band line is the i-th case's plan
    assert traced == [_band_groups(prob, group) for _, prob in cases], traced
    for name, prob in cases:
        solver, hbw = got[name + "_solver"]
        assert str(solver) == "band" and int(hbw) == _half_bandwidth(prob), (name, solver, hbw)
        assert _band_groups(prob, group) != _band_groups(prob, 32), name          # the switch changed the cut
        _check(got[name + "_log"], got[name + "_poses"], got[name + "_points"], _oracle_opt(oracle, None, prob, True, 8))


# ---- 5. dense panels and the single-workgroup factorisation -------------------------------------------------------------

@pytest.mark.parametrize("n_free", [5, 6, 16, 21, 22, 32, 48])
def test_dense_panel_edges(hiplib, oracle, ctx, n_free):
    """dims 30 / 36 / 96 / 126 / 132 / 192 / 288: below, on and above 32-column panel edges of the dense factorisation (single
    problems: the panel-pair chain, never k_chol_wg)."""
    prob = synth.ba_problem(n_free + 1, 40 * (n_free + 1), 300 * (n_free + 1), 640, 480, seq_id=300 + n_free)
    assert int((prob["fixed"] == 0).sum()) == n_free
    before = ctx.ba_wg_factorisations()
    ba = _make(hiplib, ctx, prob, "dense")
    assert ba.solver()[0] == "dense"
    prof, _, dim = ba.optimize_profiled(True, 3)
    assert dim == 6 * n_free and _one_pass(tuple(prof.get(k, (0, 0, 0))[1] for k in ("k_ba_update", "k_ba_backsub", "k_ba_trial")))
    ba.reset()
    glog = ba.optimize(True, 8)
    gp, gx = ba.state()
    _check(glog, gp, gx, _oracle_opt(oracle, None, prob, True, 8))
    assert ctx.ba_wg_factorisations() == before
    ba.close()


def test_single_workgroup_factorisation_limit_in_a_batch(hiplib, oracle):
    """A batch of 40 dense problems of dims 300 (dim + 1 = 301 <= 304: k_chol_wg) and 306 (the panel-pair chain beside it); a batch
    of 40 dim-306 problems alone runs no k_chol_wg, so the factorisations counted for the mixed batch are the dim-300 ones.  Every
    problem matches its single solve within rounding, one of each dim the oracle."""
    c = hiplib.Context(640, 480, 500, 1.2, 4, max_images=1)
    probs = {nf: [synth.ba_problem(nf + 1, 2500, 16000, 640, 480, seq_id=400 + 10 * nf + i) for i in range(10)] for nf in (50, 51)}
    make = lambda pr: _make(hiplib, c, pr, "dense")
    iters = 6
    singles = {}
    for nf, ps in probs.items():
        for i, pr in enumerate(ps):
            one = make(pr)
            singles[(nf, i)] = (one.optimize(True, iters),) + one.state()
            one.close()
    assert c.ba_wg_factorisations() == 0
    items = [(nf, i) for nf in (50, 51) for i in range(10)] * 2
    batch = [make(probs[nf][i]) for nf, i in items]
    logs = hiplib.ba_optimize_batch(batch, True, iters)
    assert c.ba_wg_factorisations() >= iters, "the dim-300 problems were meant to go through k_chol_wg"
    for (nf, i), b, lg in zip(items, batch, logs):
        wl, wp, wx = singles[(nf, i)]
        gp, gx = b.state()
        assert len(wl) == len(lg) and np.allclose(wl["chi2_after"], lg["chi2_after"], rtol=1e-10) and np.array_equal(wl["trials"], lg["trials"])
        assert np.abs(wp - gp).max() < 1e-8 and np.abs(wx - gx).max() < 1e-8, (nf, i)
    for nf in (50, 51):
        pr = probs[nf][0]
        lg = logs[items.index((nf, 0))]
        gp, gx = batch[items.index((nf, 0))].state()
        _check(lg, gp, gx, _oracle_opt(oracle, None, pr, True, iters))
    for b in batch:
        b.close()
    big = [make(probs[51][i % 10]) for i in range(40)]
    before = c.ba_wg_factorisations()
    logs = hiplib.ba_optimize_batch(big, True, iters)
    assert c.ba_wg_factorisations() == before, "dim 306 does not fit k_chol_wg"
    for i, (b, lg) in enumerate(zip(big, logs)):
        wl, wp, wx = singles[(51, i % 10)]
        gp, gx = b.state()
        assert np.allclose(wl["chi2_after"], lg["chi2_after"], rtol=1e-10) and np.abs(wp - gp).max() < 1e-8, i
        b.close()
    c.close()


# ---- 6. mixed batch -------------------------------------------------------------------------------------------------------

def test_mixed_batch_of_every_update_form(hiplib, oracle, ctx):
    """One batch with a one-launch window, a structure-only window (no free keyframe), a window without landmarks, a band window
    and the 321-keyframe map (both without k_ba_update): k_ba_update runs beside k_ba_backsub + k_ba_trial, which skip the problems
    it took.  Below 40 problems there is no k_chol_wg, so every problem gives the bytes of its single solve; each follows the oracle."""
    one_pass = synth.ba_problem(12, 600, 4000, 640, 480, seq_id=21)
    structure = synth.ba_problem(4, 60, 200, 640, 480, seq_id=8)
    structure["fixed"][:] = 1
    base = synth.ba_problem(5, 80, 320, 640, 480, seq_id=22)
    no_lm = dict(base, points=np.zeros((0, 3)), points_gt=np.zeros((0, 3)), **{k: base[k][:0] for k in OBS_KEYS})
    band = synth.ba_problem(14, 500, 2600, 640, 480, seq_id=6, tracks="contiguous")
    big = _global(321)
    probs = [("one_pass", one_pass, "one"), ("structure", structure, "two"), ("no_landmarks", no_lm, "two"),
             ("band", band, "one"), ("global321", big, "two")]
    iters = 10
    for name, pr, form in probs:
        path = _update_path(hiplib, ctx, pr)
        assert (_one_pass(path) if form == "one" else path[0] == 0 and path[1] > 0), (name, path)
    batch = [_make(hiplib, ctx, pr) for _, pr, _ in probs]
    assert [b.solver()[0] for b in batch] == ["dense", "dense", "dense", "band", "dense"]
    logs = hiplib.ba_optimize_batch(batch, True, iters)
    for (name, pr, _), b, lg in zip(probs, batch, logs):
        one = _make(hiplib, ctx, pr)
        wl = one.optimize(True, iters)
        wp, wx = one.state()
        gp, gx = b.state()
        assert wl.tobytes() == lg.tobytes() and np.array_equal(wp, gp) and np.array_equal(wx, gx), name
        one.close()
        _check(lg, gp, gx, _oracle_opt(oracle, (321, "random") if name == "global321" else None, pr, True, iters))
    assert np.array_equal(batch[1].state()[0], structure["poses"]) and np.array_equal(batch[2].state()[0], base["poses"])
    assert logs[2]["chi2_after"][-1] == 0.0
    assert all(b.timeouts() == (0, 0) for b in batch)
    for b in batch:
        b.close()


# ---- 7. iteration cap -----------------------------------------------------------------------------------------------------

def test_iteration_cap(hiplib, oracle, ctx):
    """MAX_LOG = 64: optimize(robust, 64) runs and logs all 64 iterations (a dense and a band window that are still descending at
    the end -- chi2 falls by more than 8e-9 relative per iteration, so no decision is left to rounding); 65 is refused by optimize,
    optimize_begin and the batch call, and the problem stays usable."""
    for prob in (synth.ba_problem(12, 600, 4000, 640, 480, seq_id=21), synth.ba_problem(14, 500, 2600, 640, 480, seq_id=6, tracks="contiguous")):
        ba = _make(hiplib, ctx, prob)
        glog = ba.optimize(True, 64)
        gp, gx = ba.state()
        _check(glog, gp, gx, _oracle_opt(oracle, None, prob, True, 64))
        assert len(glog) == 64 and np.all(glog["status"] == 0)
        with pytest.raises(hiplib.LpslamHipError):
            ba.optimize(True, 65)
        with pytest.raises(hiplib.LpslamHipError):
            ba.optimize_begin(True, 65)
        with pytest.raises(hiplib.LpslamHipError):
            hiplib.ba_optimize_batch([ba], True, 65)
        assert np.array_equal(ba.state()[0], gp)                 # refused before anything ran
        ba.reset()
        again = ba.optimize(True, 64)
        ap, ax = ba.state()
        assert again.tobytes() == glog.tobytes() and np.array_equal(ap, gp) and np.array_equal(ax, gx)
        ba.close()
