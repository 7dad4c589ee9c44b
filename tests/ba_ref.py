"""One Levenberg trial of the SE3 bundle adjuster restated in numpy, in np.longdouble (dtype=np.float64 runs the identical code in
double: its distance from the long-double result is the "host error" of the build tests).  Stands on its own; takes the problem
dictionary of synth.ba_problem / hiplib.ba_obs_array.

    lin = linearize(pr, robust, active)        per observation e, chi2, weight, rho, A (landmark), B (pose, rotation first); the sums
                                               H_ll, b_l, H_pp, b_p, W, chi2, max diag H_ll, lambda_0 -- and their companions of
                                               absolute values (`*_abs`)
    red = reduce(pr, lin, lam)                 S = H_pp - sum W (H_ll + lam I)^-1 W^T (no lambda on the pose diagonal), rhs, companions
                                               S_abs, rhs_abs, the largest kappa_2(H_ll + lam I), the pair-list term counts
    st  = step(pr, lin, red, robust)           x_p = (S + lam I)^-1 rhs refined in the working precision, x_l, the trial state (g2o's
                                               SE3 oplus), its chi2, rho, the accept decision and the next lambda
    first_trial(pr, ...)                       the three in a row at lambda_0

Companions of absolute values: every lowest-level product replaced by its absolute value, |B|^T w |B| + |W| |H^-1| |W|^T entrywise.
One departure from that definition, stated here because every bar of the build tests inherits it: the residual e = obs - projection is a
difference of numbers a few hundred times its size, so wherever e enters a sum (b_l, b_p, rhs, chi2) its companion is e_abs = |obs| +
|projection|, not |e|.  That makes T of b_p 40 to 550 times, and T of chi2 about 300 times, what "every product by its absolute value"
alone gives; without it a float64 evaluation of the residual does not fit a bar of the form k 2^-53 T with a data-independent k.  S,
diag H_pp and max diag H_ll hold no residual and take the plain definition.  A Huber weight's own dependence on the residual has no
companion: it stays inside the constant c of the bars (build_cases.system_bars / lin_bars / step_bars).

`mutate` (tests/test_ba_ref_cpu.py, sensitivity): a dictionary that plants one defect -- see MUTATIONS."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs an extended np.longdouble (x87: 64-bit significand)"

CHI2_MONO, CHI2_STEREO = 5.991, 7.815
MUTATIONS = ("drop_w",          # (a, b): the term of observations a, b (one landmark, two free keyframes) left out of their pair list, both triangles
             "huber_unit",      # k: observation k keeps weight inv_sigma2 whatever its chi2
             "mono_row3",       # k: the third Jacobian row of mono observation k is not zeroed
             "no_lambda",       # l: (H_ll + lam I)^-1 of landmark l without lam
             "count_inactive",  # k: observation k counts although the mask switches it off
             "dupe_cross")      # (a, b): the cross term Y_a b_l of duplicates a, b counted into the rhs once more


def _rot(q, dt):
    """rotation matrices of the quaternions (n x 4, w first), normalised as the kernels do"""
    q = q / np.sqrt((q * q).sum(1))[:, None]
    w, x, y, z = q.T
    one, two = dt(1), dt(2)
    R = np.empty((len(q), 3, 3), dt)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - w * z); R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y); R[:, 2, 1] = two * (y * z + w * x); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def _cam(pr, dt):
    return {k: dt(pr["cam"][k]) for k in ("fx", "fy", "cx", "cy", "fxb")}


def residuals(pr, poses, points, dt=LD):
    """e (n x 3, third entry 0 at mono observations), the camera-frame points, the rotations and e_abs = |obs| + |projection|"""
    c = _cam(pr, dt)
    op, ol = pr["obs_pose"], pr["obs_point"]
    uvr = pr["obs_uvr"].astype(dt)
    R = _rot(np.asarray(poses, dt)[:, :4], dt)[op]
    pc = np.einsum("nij,nj->ni", R, np.asarray(points, dt)[ol]) + np.asarray(poses, dt)[op, 4:]
    x, y, z = pc.T
    u = c["fx"] * x / z + c["cx"]; v = c["fy"] * y / z + c["cy"]; ur = u - c["fxb"] / z
    mono = pr["obs_uvr"][:, 2] < 0
    e = np.stack([uvr[:, 0] - u, uvr[:, 1] - v, np.where(mono, dt(0), uvr[:, 2] - ur)], axis=1)
    e_abs = np.stack([np.abs(uvr[:, 0]) + np.abs(c["fx"] * x / z) + c["cx"], np.abs(uvr[:, 1]) + np.abs(c["fy"] * y / z) + c["cy"],
                      np.where(mono, dt(0), np.abs(uvr[:, 2]) + np.abs(c["fx"] * x / z) + c["cx"] + np.abs(c["fxb"] / z))], axis=1)
    return e, pc, R, mono, e_abs


def weights(pr, e, mono, robust, dt=LD):
    """chi2 = inv_sigma2 |e|^2, the Huber weight and rho of every observation (delta^2 = 5.991 mono, 7.815 stereo)"""
    om = pr["obs_inv_sigma2"].astype(dt)
    chi = om * (e * e).sum(1)
    d2 = np.where(mono, dt(CHI2_MONO), dt(CHI2_STEREO))
    # the kernels and the oracle carry delta = sqrt(5.991) as a double and square it again: the threshold is that product
    delta = np.sqrt(d2.astype(np.float64)).astype(dt)
    dsqr = delta * delta
    lin = (chi > dsqr) & bool(robust)
    sq = np.sqrt(np.where(lin, chi, dt(1)))
    w = np.where(lin, om * delta / sq, om)
    rho = np.where(lin, dt(2) * sq * delta - dsqr, chi)
    return chi, w, rho, lin


def jacobians(pr, pc, R, mono, dt=LD, keep_row3=None):
    c = _cam(pr, dt)
    x, y, z = pc.T
    z2 = z * z
    n = len(z)
    A = np.zeros((n, 3, 3), dt); B = np.zeros((n, 3, 6), dt)
    A[:, 0] = -c["fx"] * R[:, 0] / z[:, None] + c["fx"] * (x / z2)[:, None] * R[:, 2]
    A[:, 1] = -c["fy"] * R[:, 1] / z[:, None] + c["fy"] * (y / z2)[:, None] * R[:, 2]
    A[:, 2] = A[:, 0] - c["fxb"] * R[:, 2] / z2[:, None]
    B[:, 0, 0] = x * y / z2 * c["fx"]; B[:, 0, 1] = -(dt(1) + x * x / z2) * c["fx"]; B[:, 0, 2] = y / z * c["fx"]
    B[:, 0, 3] = -c["fx"] / z; B[:, 0, 5] = x / z2 * c["fx"]
    B[:, 1, 0] = (dt(1) + y * y / z2) * c["fy"]; B[:, 1, 1] = -x * y / z2 * c["fy"]; B[:, 1, 2] = -x / z * c["fy"]
    B[:, 1, 4] = -c["fy"] / z; B[:, 1, 5] = y / z2 * c["fy"]
    B[:, 2, 0] = B[:, 0, 0] - c["fxb"] * y / z2; B[:, 2, 1] = B[:, 0, 1] + c["fxb"] * x / z2; B[:, 2, 2] = B[:, 0, 2]
    B[:, 2, 3] = B[:, 0, 3]; B[:, 2, 5] = B[:, 0, 5] - c["fxb"] / z2
    zero = mono.copy()
    if keep_row3 is not None:
        zero[keep_row3] = False
    A[zero, 2] = 0; B[zero, 2] = 0
    return A, B


def slots(pr):
    free = pr["fixed"] == 0
    slot = np.cumsum(free) - 1
    slot[~free] = -1
    return slot, int(free.sum())


def _scatter(shape, idx, vals, dt):
    out = np.zeros(shape, dt)
    np.add.at(out, idx, vals)
    return out


def linearize(pr, robust=True, active=None, dt=LD, poses=None, points=None, mutate=None):
    mutate = mutate or {}
    poses = pr["poses"] if poses is None else poses
    points = pr["points"] if points is None else points
    n_obs, n_pts = len(pr["obs_pose"]), len(points)
    act = np.ones(n_obs, bool) if active is None else np.asarray(active).astype(bool).copy()
    if "count_inactive" in mutate:
        act[mutate["count_inactive"]] = True
    e, pc, R, mono, e_abs = residuals(pr, poses, points, dt)
    chi, w, rho, on_lin = weights(pr, e, mono, robust, dt)
    if "huber_unit" in mutate:
        w[mutate["huber_unit"]] = dt(pr["obs_inv_sigma2"][mutate["huber_unit"]])
    A, B = jacobians(pr, pc, R, mono, dt, mutate.get("mono_row3"))
    wa = np.where(act, w, dt(0))
    slot, n_free = slots(pr)
    sl = slot[pr["obs_pose"]]
    fr = sl >= 0
    ol = pr["obs_point"]
    aA, aB = np.abs(A), np.abs(B)
    we = wa[:, None] * e

    def sums(JL, JR, wt, shape, idx, m):
        return _scatter(shape, idx[m], np.einsum("nri,n,nrj->nij", JL[m], wt[m], JR[m]), dt)

    def vsum(J, wt, vec, shape, idx, m):
        return _scatter(shape, idx[m], np.einsum("nri,nr->ni", J[m], wt[m, None] * vec[m]), dt)
    every = np.ones(n_obs, bool)
    Hll = sums(A, A, wa, (n_pts, 3, 3), ol, every); bl = -vsum(A, wa, e, (n_pts, 3), ol, every)
    Hll_abs = sums(aA, aA, wa, (n_pts, 3, 3), ol, every); bl_abs = vsum(aA, wa, e_abs, (n_pts, 3), ol, every)
    Hpp = sums(B, B, wa, (n_free, 6, 6), sl, fr); bp = -vsum(B, wa, e, (n_free, 6), sl, fr)
    Hpp_abs = sums(aB, aB, wa, (n_free, 6, 6), sl, fr); bp_abs = vsum(aB, wa, e_abs, (n_free, 6), sl, fr)
    W = np.einsum("nri,n,nrj->nij", B, np.where(fr, wa, dt(0)), A)                     # 6 x 3 per observation; zero at fixed keyframes
    chi2 = np.where(act, rho, dt(0)).sum()
    chi2_abs = (np.where(act, rho, dt(0)) + 2 * np.where(act, pr["obs_inv_sigma2"].astype(dt), dt(0)) * (np.abs(e) * e_abs).sum(1)).sum()
    dll = np.einsum("jii->ji", Hll)
    max_ll = dll.max() if n_pts else dt(0)
    where_ll = np.unravel_index(int(np.argmax(dll)), dll.shape) if n_pts else (0, 0)
    dpp = np.einsum("sii->si", Hpp).reshape(-1)
    max_pp = np.abs(dpp).max() if n_free else dt(0)
    lam0 = dt(1e-5) * max(max_pp, max_ll if n_pts else dt(0))
    cnt = np.bincount(pr["obs_pose"][act], minlength=len(pr["poses"]))
    return dict(dt=dt, e=e, e_abs=e_abs, chi=chi, w=w, rho=rho, on_lin=on_lin, mono=mono, act=act, A=A, B=B, slot=slot, n_free=n_free, dim=6 * n_free,
                Hll=Hll, bl=bl, Hpp=Hpp, bp=bp.reshape(-1), W=W, chi2=chi2, max_ll=max_ll, max_ll_abs=Hll_abs[where_ll[0], where_ll[1], where_ll[1]] if n_pts else dt(0),
                lam0=lam0, Hll_abs=Hll_abs, bl_abs=bl_abs, Hpp_abs=Hpp_abs, bp_abs=bp_abs.reshape(-1), chi2_abs=chi2_abs,
                hpp_diag=dpp, hpp_diag_abs=np.einsum("sii->si", Hpp_abs).reshape(-1), obs_count=cnt[pr["fixed"] == 0], poses=np.asarray(poses), points=np.asarray(points), obs_pose=pr["obs_pose"], obs_point=pr["obs_point"])


def inv3(H, dt):
    """inverse of symmetric 3 x 3 matrices by cofactors (the working precision throughout)"""
    a, b, c, d, e, f = H[:, 0, 0], H[:, 0, 1], H[:, 0, 2], H[:, 1, 1], H[:, 1, 2], H[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * c00 + b * c01 + c * c02
    ok = np.abs(det) > 0
    idt = np.where(ok, dt(1) / np.where(ok, det, dt(1)), dt(0))
    out = np.empty_like(H)
    out[:, 0, 0] = c00 * idt; out[:, 0, 1] = out[:, 1, 0] = c01 * idt; out[:, 0, 2] = out[:, 2, 0] = c02 * idt
    out[:, 1, 1] = (a * f - c * c) * idt; out[:, 1, 2] = out[:, 2, 1] = (b * c - a * e) * idt; out[:, 2, 2] = (a * d - b * b) * idt
    return out


def pair_index(pr, lin):
    """(a, b): every ordered pair of active observations of free keyframes that share a landmark (a == b and duplicates included)"""
    ks = np.nonzero(lin["act"] & (lin["slot"][pr["obs_pose"]] >= 0))[0]
    ks = ks[np.argsort(pr["obs_point"][ks], kind="stable")]
    lm = pr["obs_point"][ks]
    starts = np.r_[0, np.nonzero(np.diff(lm))[0] + 1, len(ks)] if len(ks) else np.array([0])
    pa, pb = [], []
    for s, t in zip(starts[:-1], starts[1:]):
        g = ks[s:t]
        pa.append(np.repeat(g, len(g))); pb.append(np.tile(g, len(g)))
    if not pa:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(pa), np.concatenate(pb)


def reduce(pr, lin, lam, mutate=None):
    mutate = mutate or {}
    dt = lin["dt"]
    lam = dt(lam)
    nf, dim = lin["n_free"], lin["dim"]
    sl = lin["slot"][pr["obs_pose"]]
    ol = pr["obs_point"]
    Hd = lin["Hll"] + lam * np.eye(3, dtype=dt)
    if "no_lambda" in mutate:
        Hd[mutate["no_lambda"]] = lin["Hll"][mutate["no_lambda"]]
    Hinv = inv3(Hd, dt)
    ev = np.linalg.eigvalsh(Hd.astype(np.float64)) if len(Hd) else np.ones((1, 3))
    seen = np.zeros(len(Hd), bool); seen[ol[lin["act"]]] = True
    kap = np.abs(ev).max(1) / np.maximum(np.abs(ev).min(1), 1e-300)
    kappa_l = float(kap[seen].max()) if seen.any() else 1.0
    a, b = pair_index(pr, lin)
    if "drop_w" in mutate:
        da, db = mutate["drop_w"]
        keep = ~(((a == da) & (b == db)) | ((a == db) & (b == da)))
        a, b = a[keep], b[keep]
    W, aW, aH = lin["W"], np.abs(lin["W"]), np.abs(Hinv)
    eye = np.eye(nf, dtype=dt)[:, None, :, None]

    def blockdiag(Hb):                                     # [slot, r, slot, c]
        return np.ascontiguousarray(Hb[:, :, None, :] * eye) if nf else np.zeros((0, 6, 0, 6), dt)

    def schur(Wl, Hi, Wr, bvec):
        Y = np.einsum("nij,njk->nik", Wl[a], Hi[ol[a]])
        blk = _scatter((nf, nf, 6, 6), (sl[a], sl[b]), np.einsum("nik,njk->nij", Y, Wr[b]), dt)
        d = a == b                                          # the rhs takes an observation's own term: Y_a b_l
        vec = _scatter((nf, 6), sl[a[d]], np.einsum("nik,nk->ni", Y[d], bvec[ol[a[d]]]), dt)
        return blk.transpose(0, 2, 1, 3).reshape(dim, dim), vec.reshape(-1)
    Ss, rs = schur(W, Hinv, W, lin["bl"])
    Sa, ra = schur(aW, aH, aW, lin["bl_abs"])
    _, rk = schur(aW, aH, aW, np.abs(lin["bl"]))          # what an error of (H_ll + lam I)^-1 is multiplied by in the rhs
    S = blockdiag(lin["Hpp"]).reshape(dim, dim) - Ss
    rhs = lin["bp"] - rs
    S_pp_abs = blockdiag(lin["Hpp_abs"]).reshape(dim, dim)
    S_abs = S_pp_abs + Sa
    rhs_abs = lin["bp_abs"] + ra
    if "dupe_cross" in mutate:
        da, db = mutate["dupe_cross"]
        rhs[6 * sl[da]:6 * sl[da] + 6] -= (W[da] @ Hinv[ol[da]]) @ lin["bl"][ol[db]]
    terms = np.zeros((nf, nf), np.int64)
    np.add.at(terms, (sl[a], sl[b]), 1)
    return dict(S=S, rhs=rhs, S_abs=S_abs, rhs_abs=rhs_abs, S_pp_abs=S_pp_abs, S_sc_abs=Sa, rhs_pp_abs=lin["bp_abs"], rhs_sc_abs=ra, rhs_sc_k=rk, Hinv=Hinv, kappa_l=kappa_l, terms=terms, lam=lam)


def solve_refined(A, b, dt, steps=40):
    """x with A x = b: a float64 Cholesky solve refined with residuals in dt until the correction stops shrinking"""
    n = len(b)
    if n == 0:
        return np.zeros(0, dt)
    A64 = A.astype(np.float64)
    L = np.linalg.cholesky(A64)

    def sub(r):
        return np.linalg.solve(L.T, np.linalg.solve(L, r))
    x = sub(b.astype(np.float64)).astype(dt)
    last = np.inf
    for _ in range(steps):
        r = b - A @ x
        s = float(np.abs(r).max())
        if s == 0.0:
            break
        d = sub((r / dt(s)).astype(np.float64)).astype(dt) * dt(s)
        size = float(np.abs(d).max())
        if not size < 0.5 * last:
            break
        x = x + d
        last = size
    return x


def oplus(pose, d, dt=LD):
    """exp([omega, upsilon]) * pose, g2o's SE3Quat::exp with its small-angle branch (theta < 1e-5)"""
    pose, d = np.asarray(pose, dt), np.asarray(d, dt)
    w = d[:3]
    th = np.sqrt((w * w).sum())
    Wm = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)
    if th < 1e-5:
        a, b, c = dt(1), dt(0.5), dt(1) / dt(6)
        qe = np.r_[dt(1), dt(0.5) * w]
    else:
        a, b, c = np.sin(th) / th, (dt(1) - np.cos(th)) / (th * th), (th - np.sin(th)) / (th * th * th)
        qe = np.r_[np.cos(th / 2), np.sin(th / 2) / th * w]
    I = np.eye(3, dtype=dt)
    Re = I + a * Wm + b * (Wm @ Wm)
    V = I + b * Wm + c * (Wm @ Wm)
    q = pose[:4]
    qn = np.r_[qe[0] * q[0] - qe[1:] @ q[1:], qe[0] * q[1:] + q[0] * qe[1:] + np.cross(qe[1:], q[1:])]
    return np.r_[qn / np.sqrt((qn * qn).sum()), V @ d[3:] + Re @ pose[4:]]


def step(pr, lin, red, robust=True):
    dt = lin["dt"]
    lam, dim, nf = red["lam"], lin["dim"], lin["n_free"]
    A = red["S"] + lam * np.eye(dim, dtype=dt)
    xp = solve_refined(A, red["rhs"], dt)
    kappa_s = float(np.linalg.cond(A.astype(np.float64))) if dim else 1.0
    sl = lin["slot"][pr["obs_pose"]]
    ol = pr["obs_point"]
    fr = (sl >= 0) & lin["act"]
    wx = _scatter((len(lin["points"]), 3), ol[fr], np.einsum("nij,ni->nj", lin["W"][fr], xp.reshape(nf, 6)[sl[fr]]), dt)
    xl = np.einsum("nij,nj->ni", red["Hinv"], lin["bl"] - wx)
    poses = np.asarray(lin["poses"], dt).copy()
    for i in np.nonzero(lin["slot"] >= 0)[0]:
        poses[i] = oplus(poses[i], xp[6 * lin["slot"][i]:6 * lin["slot"][i] + 6], dt)
    points = np.asarray(lin["points"], dt) + xl
    e, _, _, mono, _ = residuals(pr, poses, points, dt)
    _, _, rho_obs, _ = weights(pr, e, mono, robust, dt)
    chi_trial = np.where(lin["act"], rho_obs, dt(0)).sum()
    scale_l = (xl * (lam * xl + lin["bl"])).sum()
    scale_p = (xp * (lam * xp + lin["bp"])).sum()
    rho = (lin["chi2"] - chi_trial) / (scale_l + scale_p + dt(1e-3))
    accepted = bool(rho > 0 and np.isfinite(chi_trial))
    if accepted:
        t = dt(2) * rho - dt(1)
        alpha = min(dt(1) - t * t * t, dt(2) / dt(3))
        lam_next = lam * max(dt(1) / dt(3), alpha)
    else:
        lam_next = lam * dt(2)
    return dict(xp=xp, xl=xl, poses=poses, points=points, chi_trial=chi_trial, rho=rho, accepted=accepted, lam_next=lam_next, kappa_s=kappa_s,
                scale_l=scale_l, scale_p=scale_p)


def first_trial(pr, robust=True, active=None, dt=LD, mutate=None):
    lin = linearize(pr, robust, active, dt, mutate=mutate)
    red = reduce(pr, lin, lin["lam0"], mutate)
    st = step(pr, lin, red, robust)
    return lin, red, st
