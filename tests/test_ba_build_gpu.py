"""The build of the bundle adjuster's reduced system and its first Levenberg step held to a reference of the same operation: the
long-double restatement tests/ba_ref.py on the windows of tests/build_cases.py (tests/test_ba_ref_cpu.py ties that reference to the step
double, to central differences and to the CPU oracle, and holds the cases to what they claim).

  a. through the step API (dense solver): b_p, diag H_pp, chi2, max diag H_ll behind step_begin(robust, first); S (both triangles, every
     entry), rhs, the padding and lambda_0 (build_runner's docstring says how) behind step_lambda0 + step_begin; the same again behind one step_solve / step_end, at the state
     the device accepted (read back, so the second comparison starts from the device's own numbers) or at the grown lambda.  That solve
     factored S in place: every block is rewritten, and blocks the reference has as zero -- the empty pair list, the keyframe without
     observations -- are exactly 0.0.
  b. one optimize(robust, 1) on the product paths -- the solver the structure implies and, where that is the band solver, the dense one
     too; a batch-built window; 40 windows through ba_optimize_batch and k_chol_wg: free poses and points, fixed poses byte for byte,
     chi2 before and after, one trial, accepted, lambda.

Two bars on every compared entry (tests/test_ba_solve_gpu.py's pair).

Derived, nothing measured in it:  |dev - ref| <= (t + c) kappa_l 2^-53 T entry by entry, T the companion of absolute values of ba_ref,
t the terms of the entry's pair list (+ the keyframe's observations on a diagonal block), kappa_l the largest kappa_2(H_ll + lambda I).
Inside T, kappa_l is taken to 1 on the parts (H_ll + lambda I)^-1 does not multiply (build_cases.system_bars), which only tightens the bar.
b_p, diag H_pp, chi2 and max diag H_ll: the same with kappa_l = 1.  The step: kappa_2(S + lambda_0 I) (the bars of S and rhs relative to
their norms + n 2^-53) ||step||_inf for rotation, translation and points apart, or the same first-order bound in Jacobi-scaled variables
where that is smaller (build_cases.step_bars), + 4 x 2^-53 |value| for the stored state; the census holds it to 1e-6 rad / m.

  One departure from "every lowest-level product by its absolute value", in T and therefore in both bars: where the residual e = obs -
  projection enters a sum (b_p, b_l, rhs, chi2) its companion is |obs| + |projection|, not |e| (ba_ref's docstring: T of b_p grows 40 to 550
  times, T of chi2 about 300 times).  The cancellation is the operation's own: a float64 residual is wrong by a few 2^-53 of |projection|,
  hundreds of 2^-53 of |e|, and no data-independent c covers that against |e|.  S, diag H_pp and max diag H_ll are not touched by it.

  c = 128, counted in roundings of relative size 2^-53 on the longest chain behind one term Y W^T of an entry (fast_rcp / fast_rsqrt:
  1.4e-16 = 1.3 of them):  quat_to_rot 7 (norm 4, rsqrt 1.3, scaling 1, an entry 4 of which 3 overlap) -> camera point +4 = 11 -> 1 / z
  +1.3 -> an entry of A or B at most +6 (four factors, a sum, 1 + .) = 18.3;  W = B^T (w A): +4 = 22.3, twice in a term = 44.6;  an entry
  of H_ll 2 x 18.3 + 3 = 39.6 and point_hinv's cofactor, determinant, reciprocal and product +9 = 48.6;  Y = W H^-1 +3, Y W^T +3:
  99.2 -- rounded up to 128 for the sum over a landmark's observations (at most 10 here) and the Huber weight's own chain (rsqrt and two
  products).  The t terms of a list add t.

Regression:  e_dev <= M max(e_host, 2^-53), e = max |x - ref| / T (states: / ||step||_inf), e_host from the float64 run of the reference
on the same input.  M = 64 (build_runner.M): the smallest power of two >= 2 x the largest ratio e_dev / e_host measured on an MI355X over
every case, 20.69 (build_runner.MEASURED_RATIO; profiles/build_accuracy.txt, tools/build_accuracy.py; DESIGN.md "Accuracy of the window
build"): max diag H_ll of `pairs`, one number whose float64 error happens to be 1.7e-16; the next largest ratio is 3.77.  The factor 2 is
what a re-ordered sum may move an error by."""
import numpy as np
import pytest

import build_cases as bc
import build_runner as br

pytestmark = pytest.mark.gpu

M, MEASURED_RATIO, C = br.M, br.MEASURED_RATIO, br.C

PRODUCT = [(n, s) for n in bc.PRODUCT for s in ("auto", "dense")]


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)
    yield c
    c.close()


def check(rows):
    print("\n" + br.HEADER)
    for r in rows:
        print(br.format_row(r))
    for r in rows:
        where = (r["case"], r["stage"], r["qty"], r["path"])
        assert r["finite"], where
        assert r["exact"], "an entry the reference has as exactly zero is not 0.0 on the device %s" % (where,)
        assert r["worst"] <= 1.0, "|dev - ref| is %.3g x the derived bar %s" % (r["worst"], where)
        assert r["e_dev"] <= M * max(r["e_host"], bc.U), "e_dev %.3g is %.1f x the host's %s" % (r["e_dev"], r["ratio"], where)


STEP_CASES = [(n, True) for n in bc.STEP_API] + [("huber_edges", False)]


@pytest.mark.parametrize("name,robust", STEP_CASES, ids=[n + ("" if r else "-plain") for n, r in STEP_CASES])
def test_reduced_buffer_through_the_step_api(hiplib, ctx, name, robust):
    rows, f = br.step_api(hiplib, ctx, name, robust)
    print(f)
    assert f["solver"][0] == "dense", "the step API works on the dense reduced buffer"
    assert f["solver_before"][0] == bc.implied_solver(bc.problem(name))[0]
    check(rows)
    assert f["padding_first"], "outside the corner: zeros, the zero rhs row, identity rows below it"
    assert f["padding_second"], "outside the corner behind a solve: zeros right of it, identity rows below the rhs row"
    assert f["accepted"] == f["ref_accepted"]
    assert abs(f["lam"] - f["lam_ref"]) <= br.LAMBDA_RTOL * f["lam_ref"], "lambda behind the first trial: lambda_0 times g2o's factor"
    assert f["lam_factor_ok"], "lambda / lambda_0 is neither g2o's factor of an accepted trial nor the doubling of a rejected one"


def _product(hiplib, ctx, name, solver, **kw):
    implied = bc.implied_solver(bc.problem(name))
    rows, f = br.product(hiplib, ctx, name, solver, **kw)
    print(f)
    assert f["solver"] == (implied if solver == "auto" else ("dense", implied[1]))
    check(rows)
    assert f["n_log"] == 1 and f["trials"] == 1 and f["ref_accepted"] and f["moved"]
    assert f["fixed_bytes"], "a fixed pose changed"
    assert abs(f["lam"] - f["lam_ref"]) <= br.LAMBDA_RTOL * f["lam_ref"]


@pytest.mark.parametrize("name,solver", [(n, s) for n, s in PRODUCT if s == "auto" or bc.implied_solver(bc.problem(n))[0] == "band"], ids=lambda x: str(x))
def test_first_iteration_on_the_product_paths(hiplib, ctx, name, solver):
    _product(hiplib, ctx, name, solver)


def test_first_iteration_of_a_batch_built_window(hiplib, ctx):
    _product(hiplib, ctx, "mono_mix", "auto", batch_build=True)
    _product(hiplib, ctx, "mono_mix", "dense", batch_build=True)


def test_first_iteration_of_forty_windows_in_one_batch(hiplib, ctx):
    each, launches = br.batch40(hiplib, ctx)
    assert launches == 1, "the batch did not go through k_chol_wg"
    for rows, f in each:
        check(rows)
        assert f["n_log"] == 1 and f["trials"] == 1 and f["ref_accepted"] and f["fixed_bytes"] and f["moved"]
        assert abs(f["lam"] - f["lam_ref"]) <= br.LAMBDA_RTOL * f["lam_ref"]
