"""The reference of the build tests (tests/ba_ref.py) tied to things that are not the kernel, and the cases (tests/build_cases.py) held to
what they claim.  No GPU.

  against FakeStepBA    the float64 reference equals the test double's reduced buffer, scalars and one step_solve / step_end to relative 1e-12
                        (stereo only, every observation active: all the double covers)
  Jacobians             A and B equal central differences of the reference's own residual under oplus, relative 1e-7, in long double
  against the oracle    chi2 to relative 1e-12; poses and points behind the first iteration within M max(e_host, 2^-53) of the long-double
                        reference (e_host: the float64 reference's distance from it, M of tests/build_runner.py); lambda to 1e-9
  census                every case is what build_cases' docstring says, rho of the first trial > 0.1, the derived step bar <= 1e-6 rad / m
  sensitivity           six planted defects of the reference move a checked quantity by more than 100 x what the GPU tests allow"""
import numpy as np
import pytest

import ba_ref
import build_cases as bc
import build_runner as br
from _fake_ba import FakeStepBA

LD = ba_ref.LD


def close(a, b, rtol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= rtol * max(np.abs(b).max(), 1e-300)


# ---- FakeStepBA ---------------------------------------------------------------------------------------------------------------
def test_float64_reference_equals_the_step_double():
    pr = bc.make(4, [0, 3], 60, bc.all_see(4, 60), 77)
    lin, red, st = ba_ref.first_trial(pr, True, None, np.float64)
    fake = FakeStepBA(pr)
    fake.step_begin(True, True)
    S, rhs, bp, hd, tail = fake._sections()
    d = fake.dim
    assert d == lin["dim"] == 12
    assert close(bp[:d], lin["bp"], 1e-12) and close(hd[:d], lin["hpp_diag"], 1e-12) and close(tail[0], lin["chi2"], 1e-12)
    assert close(fake.scal[4], lin["max_ll"], 1e-12)
    fake.step_lambda0()
    assert close(fake.lam, lin["lam0"], 1e-12)
    fake.step_begin(True, False)
    assert close(S[:d, :d], red["S"], 1e-12) and close(rhs[:d], red["rhs"], 1e-12)
    fake.step_solve()
    assert close(fake.scal[1], st["chi_trial"], 1e-12) and close(fake.scal[2], st["scale_l"], 1e-12) and close(fake.scal[3], st["scale_p"], 1e-12)
    accepted, finished = fake.step_end()
    assert accepted == st["accepted"] and finished
    assert close(fake.lam, st["lam_next"], 1e-12)
    poses, points = fake.state()
    assert close(poses, st["poses"], 1e-12) and close(points, st["points"], 1e-12)


# ---- Jacobians ----------------------------------------------------------------------------------------------------------------
def test_jacobians_equal_central_differences():
    pr = bc.problem("mono_mix")
    e, pc, R, mono, _ = ba_ref.residuals(pr, pr["poses"], pr["points"], LD)
    A, B = ba_ref.jacobians(pr, pc, R, mono, LD)
    assert mono.any() and (~mono).any()
    h = LD(1e-7)
    for k in range(6):
        d = np.zeros(6, LD); d[k] = h
        plus = np.array([ba_ref.oplus(p, d) for p in pr["poses"]]); minus = np.array([ba_ref.oplus(p, -d) for p in pr["poses"]])
        num = (ba_ref.residuals(pr, plus, pr["points"], LD)[0] - ba_ref.residuals(pr, minus, pr["points"], LD)[0]) / (2 * h)
        scale = np.abs(B).max(axis=(1, 2))
        assert (np.abs(num - B[:, :, k]).max(1) <= 1e-7 * scale).all(), "B, column %d" % k
    for k in range(3):
        dx = np.zeros(3, LD); dx[k] = h
        num = (ba_ref.residuals(pr, pr["poses"], pr["points"].astype(LD) + dx, LD)[0] - ba_ref.residuals(pr, pr["poses"], pr["points"].astype(LD) - dx, LD)[0]) / (2 * h)
        scale = np.abs(A).max(axis=(1, 2))
        assert (np.abs(num - A[:, :, k]).max(1) <= 1e-7 * scale).all(), "A, column %d" % k
    assert not A[mono, 2].any() and not B[mono, 2].any() and not e[mono, 2].any()


# ---- the compiled CPU oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.NAMES)
def test_chi2_equals_the_oracle(oracle, name):
    pr = bc.problem(name)
    lin = bc.reference(name)[0]
    chi, _ = oracle.ba_chi2(pr["poses"], pr["points"], oracle.ba_obs(pr), pr["cam"])
    assert close(chi.sum(), lin["chi"].sum(), 1e-12)
    own = lin["chi"] + 2 * pr["obs_inv_sigma2"] * (np.abs(lin["e"]) * lin["e_abs"]).sum(1)       # an observation's chi2 moves with its residual's rounding
    assert (np.abs(chi - lin["chi"]) <= 1e-12 * own).all()


@pytest.mark.parametrize("name", bc.NAMES)
def test_first_iteration_equals_the_oracle(oracle, name):
    pr, mask = bc.problem(name), bc.mask(name)
    lin, red, st = bc.reference(name)
    l64, r64, s64 = bc.reference(name, True, np.float64)
    op, ox, olog = oracle.ba_optimize(pr["poses"], pr["fixed"], pr["points"], oracle.ba_obs(pr), pr["cam"], True, 1, active=mask)
    assert len(olog) == 1 and olog["trials"][0] == 1 and st["accepted"], "a case whose first trial the oracle rejects"
    free = pr["fixed"] == 0
    dev = bc.state_errors(op, ox, st["poses"], st["points"], free)
    host = bc.state_errors(s64["poses"], s64["points"], st["poses"], st["points"], free)
    for q, sc in enumerate(bc.step_scales(st, lin)):
        print(name, q, "oracle %.3e host %.3e" % (dev[q] / sc, host[q] / sc))
        assert dev[q] / sc <= br.M * max(host[q] / sc, bc.U), (name, q)
    assert abs(olog["lambda"][0] - float(st["lam_next"])) <= 1e-9 * float(st["lam_next"])
    assert close(olog["chi2_before"][0], lin["chi2"], 1e-12)
    assert op[~free].tobytes() == np.ascontiguousarray(pr["poses"])[~free].tobytes()


# ---- census -------------------------------------------------------------------------------------------------------------------
def counts(pr):
    return np.bincount(pr["obs_pose"], minlength=len(pr["poses"]))


@pytest.mark.parametrize("name", bc.NAMES)
def test_every_case_steps_well_inside_its_decision(name):
    lin, red, st = bc.reference(name)
    assert st["accepted"] and float(st["rho"]) > 0.1
    bars = bc.step_bars(lin, red, st, br.C)
    print(name, bars)
    assert max(bars) <= 1e-6, "the derived step bar is meant to be a hundredth of what the older tests allow"
    assert bc.implied_solver(bc.problem(name))[0] == ("dense" if name == "wide" else "band")


def test_tiny():
    pr = bc.problem("tiny")
    assert list(pr["fixed"]) == [0, 1, 0] and list(counts(pr)) == [5, 5, 5] and (pr["obs_uvr"][:, 2] >= 0).all()
    assert bc.reference("tiny")[0]["dim"] == 12 and ((12 + 1 + 31) // 32) * 32 == 32


def test_mono_mix_and_inactive():
    pr = bc.problem("mono_mix")
    lin, red, st = bc.reference("mono_mix")
    mono = pr["obs_uvr"][:, 2] < 0
    assert list(pr["fixed"]) == [1, 0, 0, 0, 0, 1] and len(pr["points"]) == 40
    assert 0.4 < mono.mean() < 0.6
    assert not np.array_equal(pr["obs_point"], np.sort(pr["obs_point"])), "observation order is meant to be shuffled"
    o0 = np.nonzero(pr["obs_point"] == 0)[0]
    assert len(o0) == 1 and mono[o0[0]] and pr["fixed"][pr["obs_pose"][o0[0]]] == 0
    assert pr["fixed"][pr["obs_pose"][pr["obs_point"] == 1]].all() and (pr["obs_point"] == 1).sum() == 2
    dll = np.einsum("jii->ji", lin["Hll"])
    assert int(np.argmax(dll.max(1))) == 1 and float(lin["max_ll"]) > 1.5 * float(np.delete(dll, 1, 0).max())
    assert counts(pr)[4] == 0
    blk = red["S"][18:24]
    assert not blk.any() and not red["S"][:, 18:24].any() and not red["S_abs"][18:24].any()
    # inactive
    m = bc.mask("inactive").astype(bool)
    assert 0.25 < 1 - m.mean() < 0.45
    assert not m[pr["obs_point"] == bc.INACTIVE_LANDMARK].any() and not m[pr["obs_pose"] == bc.INACTIVE_KEYFRAME].any()
    li, ri, _ = bc.reference("inactive")
    assert not li["Hll"][bc.INACTIVE_LANDMARK].any() and li["obs_count"][2] == 0 and not ri["S"][12:18].any()
    assert np.array_equal(ri["terms"], bc.pair_terms(pr, m))


def test_huber_edges():
    pr = bc.problem("huber_edges")
    lin = bc.reference("huber_edges")[0]
    for o, m, side in bc.PLANTED:
        d2 = LD(ba_ref.CHI2_MONO if m else ba_ref.CHI2_STEREO)
        assert (pr["obs_uvr"][o, 2] < 0) == m and pr["fixed"][pr["obs_pose"][o]] == 0
        assert abs(float(lin["chi"][o] / d2) - (1 + side * 1e-3)) < 1e-9, (o, float(lin["chi"][o] / d2))
        assert bool(lin["on_lin"][o]) == (side > 0)
    assert not bc.reference("huber_edges", False)[0]["on_lin"].any()
    assert {(m, s) for _, m, s in bc.PLANTED} == {(True, -1), (True, 1), (False, -1), (False, 1)}


@pytest.mark.parametrize("name,total", [("slices_256", 11 * 256), ("slices_257", 11 * 256 + 1)])
def test_slices(name, total):
    pr = bc.problem(name)
    c = counts(pr)
    assert tuple(c[1:]) == bc.SLICE_COUNTS and len(pr["obs_pose"]) == total and list(pr["fixed"]) == [1] + [0] * 9
    for kf in range(10):
        assert np.array_equal(np.sort(pr["obs_point"][pr["obs_pose"] == kf]), np.arange(c[kf]))
    track = np.bincount(pr["obs_point"], minlength=1025)
    assert set(track % 4) == {0, 1, 2, 3} and track.min() >= 1


def test_pairs_dupes_parts():
    pr = bc.problem("pairs")
    t = bc.pair_terms(pr)
    for (a, b), n in bc.PAIR_TERMS.items():
        assert t[a, b] == t[b, a] == n
    assert list(np.diag(t)) == [32, 65, 97, 128]
    red = bc.reference("pairs")[1]
    assert np.array_equal(red["terms"], t) and not red["S"][0:6, 6:12].any() and not red["S_abs"][0:6, 6:12].any()
    pr = bc.problem("dupes")
    twice = (pr["obs_pose"] == bc.DUPE_KEYFRAME) & (pr["obs_point"] == bc.DUPE_LANDMARK)
    assert twice.sum() == 2 and bc.pair_terms(pr)[0, 0] == 10 + 3          # 9 single terms and the 2 x 2 of the duplicate
    for n in (129, 257):
        pr = bc.problem("parts_%d" % n)
        assert (bc.pair_terms(pr) == n).all() and bc.pair_terms(pr).shape == (3, 3)


def test_wide_band_batch():
    pr = bc.problem("wide")
    assert (pr["fixed"] == 0).sum() == 64 and list(np.nonzero(pr["fixed"])[0]) == [7, 40] and len(pr["points"]) == 600
    track = np.bincount(pr["obs_point"], minlength=600)
    assert track.min() == 2 and track.max() == 5 and counts(pr).min() > 0
    assert ((6 * 64 + 1 + 31) // 32) * 32 == 416
    pr = bc.problem("band")
    assert bc.implied_solver(pr) == ("band", 3) and len(pr["poses"]) == 12
    assert len(bc.BATCH40) == 40 and {k for k, _ in bc.BATCH40} == {"tiny", "pairs"} and len(set(bc.BATCH40)) == 40
    for i in range(len(bc.BATCH40)):
        lin, red, st = bc.reference("#%d" % i)
        assert st["accepted"] and float(st["rho"]) > 0.1 and lin["dim"] == (12 if i % 2 == 0 else 24), i
        assert max(bc.step_bars(lin, red, st, br.C)) <= 1e-6, i


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
def allowed(ref, host, T, bar):
    """what the GPU tests allow an entry to move by: the larger of the derived bar and the regression bar"""
    e_host, _ = bc.rel_err(host, ref, T)
    return np.maximum(np.asarray(bar, np.float64), br.M * max(e_host, bc.U) * np.asarray(T, np.float64))


def moved(name, mutate, robust=True):
    """the largest |mutated - reference| / allowed over the quantities test_ba_build_gpu.py checks at lambda_0"""
    pr, mask = bc.problem(name), bc.mask(name)
    lin, red, _ = bc.reference(name, robust)
    l64, r64, _ = bc.reference(name, robust, np.float64)
    lm = ba_ref.linearize(pr, robust, mask, LD, mutate=mutate)
    rm = ba_ref.reduce(pr, lm, lin["lam0"], mutate)
    bS, brhs = bc.system_bars(lin, red, br.C)
    lb = bc.lin_bars(lin, br.C)
    out = {}
    for q, x, ref, host, T, bar in (("S", rm["S"], red["S"], r64["S"], red["S_abs"], bS), ("rhs", rm["rhs"], red["rhs"], r64["rhs"], red["rhs_abs"], brhs),
                                    ("b_p", lm["bp"], lin["bp"], l64["bp"], lin["bp_abs"], lb["bp"]), ("diag H_pp", lm["hpp_diag"], lin["hpp_diag"], l64["hpp_diag"], lin["hpp_diag_abs"], lb["hpp"]),
                                    ("chi2", [lm["chi2"]], [lin["chi2"]], [l64["chi2"]], [lin["chi2_abs"]], [lb["chi2"]])):
        a = allowed(ref, host, T, bar)
        pos = a > 0
        diff = np.abs(np.asarray(x, LD) - np.asarray(ref, LD)).astype(np.float64)
        out[q] = float((diff[pos] / a[pos]).max()) if pos.any() else 0.0
        if (diff[~pos] > 0).any():
            out[q] = np.inf                                 # an entry that must be exactly zero moved
    return out


def free_pair(pr, shared=True):
    """two observations of one landmark by two different free keyframes"""
    slot = ba_ref.slots(pr)[0][pr["obs_pose"]]
    for j in range(len(pr["points"])):
        ks = np.nonzero((pr["obs_point"] == j) & (slot >= 0))[0]
        if len(ks) >= 2 and slot[ks[0]] != slot[ks[-1]]:
            return int(ks[0]), int(ks[-1])
    raise AssertionError("no landmark with two free keyframes")


@pytest.mark.parametrize("name", ["pairs", "parts_257", "wide", "slices_257"])
def test_a_dropped_pair_term_shows(name):
    m = moved(name, {"drop_w": free_pair(bc.problem(name))})
    print(name, m)
    assert m["S"] > 100 and m["rhs"] == 0 and m["b_p"] == 0


def test_a_huber_edge_with_unit_weight_shows():
    for o, mono, side in bc.PLANTED:
        m = moved("huber_edges", {"huber_unit": o})
        print(o, side, m)
        if side > 0:
            assert m["S"] > 100 and m["diag H_pp"] > 100 and m["b_p"] > 100
        else:
            assert max(m.values()) == 0, "below the threshold the weight is 1 already"


def test_a_leaking_mono_row_shows():
    pr = bc.problem("mono_mix")
    slot = ba_ref.slots(pr)[0][pr["obs_pose"]]
    k = int(np.nonzero((pr["obs_uvr"][:, 2] < 0) & (slot >= 0) & (pr["obs_point"] > 1))[0][0])
    m = moved("mono_mix", {"mono_row3": k})
    print(m)
    assert m["S"] > 100 and m["diag H_pp"] > 100


@pytest.mark.parametrize("name", ["tiny", "wide", "parts_257"])
def test_lambda_left_out_of_one_landmark_shows(name):
    pr = bc.problem(name)
    l = int(pr["obs_point"][free_pair(pr)[0]])
    m = moved(name, {"no_lambda": l})
    print(name, m)
    assert m["S"] > 100 or m["rhs"] > 100


def test_a_counted_inactive_observation_shows():
    pr, mask = bc.problem("inactive"), bc.mask("inactive")
    slot = ba_ref.slots(pr)[0][pr["obs_pose"]]
    k = int(np.nonzero((mask == 0) & (slot >= 0))[0][0])
    m = moved("inactive", {"count_inactive": k})
    print(m)
    assert m["chi2"] > 100 and m["b_p"] > 100 and m["S"] > 100


def test_the_duplicates_cross_term_in_the_rhs_shows():
    pr = bc.problem("dupes")
    a, b = np.nonzero((pr["obs_pose"] == bc.DUPE_KEYFRAME) & (pr["obs_point"] == bc.DUPE_LANDMARK))[0]
    m = moved("dupes", {"dupe_cross": (int(a), int(b))})
    print(m)
    assert m["rhs"] > 100 and m["S"] == 0
