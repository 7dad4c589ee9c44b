"""Device side of the build tests (tests/test_ba_build_gpu.py, tools/build_accuracy.py): a case's window on the device, the reduced buffer
read through the step API at its two states, one optimize() iteration on the product paths, and the rows of figures both are judged by.

A row compares one quantity of one case:  e = max |x - ref| / T over its entries (T: the companion of absolute values, or ||step||_inf
for a state), e_dev for the device and e_host for the float64 run of the reference, ratio = e_dev / max(e_host, 2^-53), worst =
max |x_dev - ref| / derived bar (<= 1 passes), exact = "entries whose companion is zero are exactly 0.0".

lambda_0 cannot be read by itself: lpslam_hip_ba_status reports lambda only behind a step_end, which has already multiplied it.  It is held
three ways: S and rhs at lambda_0 carry it in every (H_ll + lambda_0 I)^-1; the lambda behind the first trial equals the reference's
lambda_0 times g2o's factor to LAMBDA_RTOL; and that factor lies in [1/3, 2/3] behind an accepted trial and is 2 behind a rejected one
(facts["lam_factor_ok"], as solve_runner.real_case asserts)."""
import numpy as np

import ba_ref
import build_cases as bc
import solve_runner as sr

LD = ba_ref.LD
C = 128                          # the constant of the derived bar (counted in tests/test_ba_build_gpu.py)
M = 64                           # the margin of the regression bar: the smallest power of two >= 2 x MEASURED_RATIO
MEASURED_RATIO = 20.69           # the largest e_dev / max(e_host, 2^-53) on an MI355X (profiles/build_accuracy.txt): pairs, max diag H_ll
LAMBDA_RTOL = 1e-9


def make_ba(hip, ctx, pr, mask=None, solver="auto", build=True):
    ba = hip.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hip.ba_obs_array(pr), pr["cam"], build=build)
    if build:
        finish(ba, mask, solver)
    return ba


def finish(ba, mask, solver):
    if solver != "auto":
        ba.set_solver(solver)
    if mask is not None:
        ba.set_active(mask)


def read_buffers(ba, dim):
    ptr, red_n = ba.reduced_buffer()
    n = sr.padded_dim(red_n)
    h = sr.device_read(ba.lib, ptr, red_n)
    scal = sr.device_read(ba.lib, ba.scalar_buffer()[0], 8)
    return dict(n=n, P=h[:n * n].reshape(n, n).copy(), S=h[:n * n].reshape(n, n)[:dim, :dim].copy(), rhs=h[n * n:n * n + dim].copy(),
                bp=h[n * n + n:n * n + n + dim].copy(), hpp=h[n * n + 2 * n:n * n + 2 * n + dim].copy(), chi2=float(h[n * n + 3 * n]),
                max_ll=float(scal[4]), tails=(h[n * n + dim:n * n + n], h[n * n + n + dim:n * n + 2 * n], h[n * n + 2 * n + dim:n * n + 3 * n]))


def row(case, stage, qty, dev, ref, host, T, bar, terms, kappa, path, dim):
    dev, ref, host = np.asarray(dev, LD), np.asarray(ref, LD), np.asarray(host, LD)
    T = np.broadcast_to(np.asarray(T, LD), ref.shape); bar = np.broadcast_to(np.asarray(bar, LD), ref.shape)
    e_dev, exact = bc.rel_err(dev, ref, T)
    e_host, _ = bc.rel_err(host, ref, T)
    pos = T > 0
    worst = float((np.abs(dev - ref)[pos] / bar[pos]).max()) if pos.any() else 0.0
    return dict(case=case, stage=stage, qty=qty, dim=dim, terms=int(np.max(terms)), kappa=float(kappa), e_host=e_host, e_dev=e_dev,
                ratio=e_dev / max(e_host, bc.U), worst=worst, exact=exact, path=path, finite=bool(np.isfinite(np.asarray(dev, np.float64)).all()))


HEADER = "case               stage    quantity       dim  terms     kappa      e_host       e_dev     ratio  e_dev/bar  path"


def format_row(r):
    return "%-18s %-8s %-12s %5d %6d %9.3g  %10.3e  %10.3e  %8.2f  %9.2e  %s%s" % (
        r["case"], r["stage"], r["qty"], r["dim"], r["terms"], r["kappa"], r["e_host"], r["e_dev"], r["ratio"], r["worst"], r["path"], "" if r["exact"] else "  NOT-EXACT-ZERO")


def lin_rows(case, stage, buf, lin, l64, path):
    b = bc.lin_bars(lin, C)
    t = int(lin["obs_count"].max()) if len(lin["obs_count"]) else 0
    d = lin["dim"]
    return [row(case, stage, "b_p", buf["bp"], lin["bp"], l64["bp"], lin["bp_abs"], b["bp"], t, 1, path, d),
            row(case, stage, "diag H_pp", buf["hpp"], lin["hpp_diag"], l64["hpp_diag"], lin["hpp_diag_abs"], b["hpp"], t, 1, path, d),
            row(case, stage, "chi2", [buf["chi2"]], [lin["chi2"]], [l64["chi2"]], [lin["chi2_abs"]], [b["chi2"]], int(lin["act"].sum()), 1, path, d),
            row(case, stage, "max H_ll", [buf["max_ll"]], [lin["max_ll"]], [l64["max_ll"]], [lin["max_ll_abs"]], [b["max_ll"]], len(lin["slot"]), 1, path, d)]


def red_rows(case, stage, buf, lin, red, r64, path):
    bS, br = bc.system_bars(lin, red, C)
    tS, tr = bc.entry_terms(lin, red)
    d = lin["dim"]
    return [row(case, stage, "S", buf["S"], red["S"], r64["S"], red["S_abs"], bS, tS.max() if d else 0, red["kappa_l"], path, d),
            row(case, stage, "rhs", buf["rhs"], red["rhs"], r64["rhs"], red["rhs_abs"], br, tr.max() if d else 0, red["kappa_l"], path, d)]


def padding_ok(buf, dim, solved):
    """outside the dim x dim corner: zero right of it, identity rows below row `dim`.  Row `dim` is the factorisation's rhs row: zero before
    the first solve; behind one it holds what k_chol_prep and the solve put there -- the working rhs left of the diagonal (not compared),
    1e200 on the diagonal, zeros right of it"""
    P, n = buf["P"], buf["n"]
    ok = not P[:dim, dim:].any()
    below = P[dim + 1:, :]
    ok = ok and np.array_equal(below, np.eye(n)[dim + 1:, :])
    if solved:
        ok = ok and P[dim, dim] == 1e200 and not P[dim, dim + 1:].any() and bool(np.isfinite(P[dim, :dim]).all())
    else:
        ok = ok and not P[dim, :].any()
    return bool(ok) and not any(t.any() for t in buf["tails"])


def step_api(hip, ctx, name, robust=True):
    """4a: the reduced buffer at the first trial's lambda_0 and again behind one solve.  Returns (rows, facts)."""
    pr, mask = bc.problem(name), bc.mask(name)
    lin, red, st = bc.reference(name, robust)
    l64, r64, s64 = bc.reference(name, robust, np.float64)
    dim = lin["dim"]
    case = name + ("" if robust else "/plain")
    ba = make_ba(hip, ctx, pr, mask, "auto")
    facts = dict(solver_before=ba.solver())
    ba.step_begin(robust, True)
    rows = lin_rows(case, "first", read_buffers(ba, dim), lin, l64, "k_ba_lin + k_ba_point_sum")
    ba.step_lambda0()
    ba.step_begin(robust, False)
    buf = read_buffers(ba, dim)
    facts["solver"] = ba.solver()
    rows += red_rows(case, "lambda0", buf, lin, red, r64, "k_ba_schur") + lin_rows(case, "lambda0", buf, lin, l64, "k_ba_schur")[:3]
    facts["padding_first"] = padding_ok(buf, dim, False)
    ba.step_solve()
    accepted, finished = ba.step_end()
    lam = ba.status()["lam"]
    lam0 = float(lin["lam0"])
    facts.update(accepted=accepted, ref_accepted=st["accepted"], lam=lam, lam_ref=float(st["lam_next"]),
                 lam_factor_ok=bool(1 / 3 - 1e-9 <= lam / lam0 <= 2 / 3 + 1e-9) if accepted else abs(lam - 2 * lam0) <= LAMBDA_RTOL * lam0)
    if accepted:
        poses, points = ba.state()
        lin2 = ba_ref.linearize(pr, robust, mask, LD, poses, points)
        l642 = ba_ref.linearize(pr, robust, mask, np.float64, poses, points)
    else:
        lin2, l642 = lin, l64
    red2, r642 = ba_ref.reduce(pr, lin2, LD(lam)), ba_ref.reduce(pr, l642, np.float64(lam))
    ba.step_begin(robust, False)
    buf2 = read_buffers(ba, dim)
    rows += red_rows(case, "second", buf2, lin2, red2, r642, "k_ba_schur") + lin_rows(case, "second", buf2, lin2, l642, "k_ba_schur")[:3]
    facts["padding_second"] = padding_ok(buf2, dim, True)
    ba.close()
    return rows, facts


def trial_gradient_bar(pr, robust, mask, st, bars):
    """what the step's bars may move the trial's chi2 by: 2 (|b_p| . bar + |b_l| . bar) at the trial state, and that state's own chi2 bar"""
    lt = ba_ref.linearize(pr, robust, mask, LD, st["poses"].astype(np.float64), st["points"].astype(np.float64))
    g = 2.0 * (float(np.abs(lt["bp"]).reshape(-1, 6)[:, :3].sum()) * bars[0] + float(np.abs(lt["bp"]).reshape(-1, 6)[:, 3:].sum()) * bars[1] + float(np.abs(lt["bl"]).sum()) * bars[2])
    return g + bc.lin_bars(lt, C)["chi2"], float(lt["chi2_abs"])


def product_rows(case, pr, mask, robust, ref, ref64, log, poses, points, path):
    """4b: the state, chi2 and lambda behind optimize(robust, 1) against the reference's first iteration"""
    lin, red, st = ref
    l64, r64, s64 = ref64
    free = pr["fixed"] == 0
    bars = bc.step_bars(lin, red, st, C)
    scales = bc.step_scales(st, lin)
    dev = bc.state_errors(poses, points, st["poses"], st["points"], free)
    host = bc.state_errors(s64["poses"], s64["points"], st["poses"], st["points"], free)
    store = 4 * bc.U * np.array([1.0, float(np.abs(st["poses"][:, 4:]).max()), float(np.abs(st["points"]).max())])
    rows = []
    for q, (nm, sc) in enumerate(zip(("rotation", "translation", "points"), scales)):
        r = dict(case=case, stage="iter1", qty=nm, dim=lin["dim"], terms=int(red["terms"].max()) if lin["dim"] else 0, kappa=st["kappa_s"], e_host=host[q] / sc, e_dev=dev[q] / sc,
                 worst=dev[q] / (bars[q] + store[q]), exact=True, path=path, finite=bool(np.isfinite(poses).all() and np.isfinite(points).all()))
        r["ratio"] = r["e_dev"] / max(r["e_host"], bc.U)
        rows.append(r)
    d = lin["dim"]
    rows.append(row(case, "iter1", "chi2_bef", [log["chi2_before"][0]], [lin["chi2"]], [l64["chi2"]], [lin["chi2_abs"]], [bc.lin_bars(lin, C)["chi2"]], int(lin["act"].sum()), 1, path, d))
    gbar, gabs = trial_gradient_bar(pr, robust, mask, st, bars)
    rows.append(row(case, "iter1", "chi2_aft", [log["chi2_after"][0]], [st["chi_trial"]], [s64["chi_trial"]], [gabs], [gbar], int(lin["act"].sum()), st["kappa_s"], path, d))
    facts = dict(trials=int(log["trials"][0]), n_log=len(log), lam=float(log["lambda"][0]), lam_ref=float(st["lam_next"]), ref_accepted=st["accepted"],
                 fixed_bytes=poses[~free].tobytes() == np.ascontiguousarray(pr["poses"], np.float64)[~free].tobytes(),
                 moved=poses[free].tobytes() != np.ascontiguousarray(pr["poses"], np.float64)[free].tobytes())
    return rows, facts


def product(hip, ctx, name, solver, robust=True, batch_build=False):
    pr, mask = bc.problem(name), bc.mask(name)
    if batch_build:
        mate = bc.problem("pairs")
        bas = [make_ba(hip, ctx, pr, build=False), make_ba(hip, ctx, mate, build=False)]
        hip.ba_build_batch(bas)
        finish(bas[0], mask, solver)
        ba = bas[0]
        bas[1].close()
    else:
        ba = make_ba(hip, ctx, pr, mask, solver)
    sv = ba.solver()
    log = ba.optimize(robust, 1)
    poses, points = ba.state()
    ba.close()
    path = "optimize / %s%s" % ("k_chol_band hbw %d" % sv[1] if sv[0] == "band" else "dense", ", batch-built" if batch_build else "")
    rows, facts = product_rows(name, pr, mask, robust, bc.reference(name, robust), bc.reference(name, robust, np.float64), log, poses, points, path)
    facts["solver"] = sv
    return rows, facts


def batch40(hip, ctx, robust=True):
    """40 small windows through ba_optimize_batch(iters=1) on the dense solver: one k_chol_wg launch"""
    prs = [bc.batch_problem(i) for i in range(len(bc.BATCH40))]
    bas = [make_ba(hip, ctx, pr, None, "dense") for pr in prs]
    before = ctx.ba_wg_factorisations()
    logs = hip.ba_optimize_batch(bas, robust, 1)
    launches = ctx.ba_wg_factorisations() - before
    out = []
    for i, (pr, ba, log) in enumerate(zip(prs, bas, logs)):
        poses, points = ba.state()
        ba.close()
        out.append(product_rows("batch40#%d" % i, pr, None, robust, bc.reference("#%d" % i, robust), bc.reference("#%d" % i, robust, np.float64), log, poses, points, "optimize_batch / k_chol_wg"))
    return out, launches
