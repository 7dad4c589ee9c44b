#!/usr/bin/env python3
"""Generates tests/golden/g20_solvers.npz: the host library's small solvers, recorded bit for bit through their C shims
(lpslam_sym_eigen, lpslam_epnp_solve, lpslam_pnp_solve_ransac, lpslam_sim3_solve_ransac, lpslam_two_view_initialize) over seeded
inputs at the smallest shapes where two copies of one algorithm could diverge.  tests/test_solvers_golden_cpu.py replays the
fixture and compares the bytes; tests/solver_cases.py holds the calls and the file layout.

  sym_eigen     n = 3, 4, 9, 12: random SPD matrices, diagonal matrices with two and with all eigenvalues equal and in descending
                order (the tie rule and every move of the sort), the zero matrix, a rank-1 matrix
  epnp          n = 3 (refused), 4, 5, 6, 37, 300: planted poses without noise and with 0.5 px of it; coplanar and collinear sets
                (refused); at least one set whose first landmark lands behind the camera before the sign rule (found with the
                numpy restatement, which the product follows operation by operation)
  pnp_ransac    n = 3, 4, 5, 37, 300 x seeds 0, 0x9E3779B9 x 1, 7, 100 iterations x 0 % and 60 % outliers; the tags say what
                became of the refit, and both outcomes (kept, rejected) are present
  sim3_ransac   n = 2 (refused), 3, 50 with fix_scale 0 and 1
  two_view      the general and the planar scene of tests/test_two_view_cpu.py (parallax far from the acceptance threshold)

Everything but two_view's parallax_deg (acos) is + - * / sqrt under -ffp-contract=off: the same bits on every machine.
Usage: python tools/make_golden_solvers.py      (deterministic)
"""
import ctypes as C
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_cases as P                   # noqa: E402
import solver_cases as S                # noqa: E402
import test_two_view_cpu as T           # noqa: E402
from oracle import two_view as TV       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g20_solvers.npz")
CAM = P.CAM
c64 = lambda a: np.ascontiguousarray(a, np.float64)


def eigen_cases():
    for n in (3, 4, 9, 12):
        for seed in range(3):
            a = np.random.default_rng(100 * n + seed).normal(size=(n, n))
            yield "spd seed %d" % seed, n, a @ a.T
        two = np.arange(n, 0, -1, dtype=float); two[0] = two[n - 1] = 0.5        # the equal pair first and last, the rest descending
        yield "diagonal, two equal", n, np.diag(two)
        yield "diagonal, all equal", n, np.diag(np.full(n, 2.5))
        yield "diagonal, descending", n, np.diag(np.arange(n, 0, -1, dtype=float))
        yield "zero", n, np.zeros((n, n))
        v = np.random.default_rng(7 + n).normal(size=n)
        yield "rank 1", n, np.outer(v, v)


def posed(n, noise, seed):
    """n landmarks in front of a seeded pose, exact projections plus Gaussian noise"""
    rng = np.random.default_rng(seed)
    r = P.rot(rng.normal(size=3), rng.uniform(0.2, 1.2)); t = rng.normal(0, 1.0, 3)
    xc = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(3, 12, n)])
    pw = (xc - t) @ r
    uv = np.column_stack([CAM[0] * xc[:, 0] / xc[:, 2] + CAM[2], CAM[1] * xc[:, 1] / xc[:, 2] + CAM[3]]) + rng.normal(0, noise, (n, 2))
    return c64(pw), c64(uv)


def epnp_cases():
    pw, uv = posed(3, 0.0, 1)
    yield "three matches (refused)", pw, uv
    for n in (4, 5, 6, 37, 300):
        for noise in (0.0, 0.5):
            for seed in range(2 if n == 300 else 4):
                pw, uv = posed(n, noise, 1000 * n + 10 * seed + (1 if noise else 0))
                yield "planted, noise %.1f px, seed %d" % (noise, seed), pw, uv
    for n in (4, 40):
        s = P.coplanar(n, 3)
        yield "coplanar (refused)", s["pw"], s["obs"]
    for n in (4, 6):
        s = P.coplanar(n, 3)
        yield "collinear (refused)", c64(np.column_stack([np.linspace(-1.0, 2.0, n) ** 3, np.full(n, 0.75), np.full(n, 1.5)])), s["obs"]


def sign_flips(pw, uv):
    """how many of the restatement's three guesses put the first landmark behind the camera before the sign rule"""
    flips = []
    horn = TV._horn_jacobi

    def spy(pc, pw_):
        f = sys._getframe(1).f_locals
        flips.append(bool(f["al"][0] @ f["ccs"][:, 2] < 0))
        return horn(pc, pw_)
    TV._horn_jacobi = spy
    try:
        TV.epnp_solve(pw, uv, CAM)
    finally:
        TV._horn_jacobi = horn
    return sum(flips)


def refit_outcome(lib, s, iterations, seed, out):
    """what pnp_solve_ransac's refit did, replayed through the shims: 'none' (no pose), 'unsolved', 'kept' or 'rejected'"""
    n = len(s["w"])
    if out["count"][0] == 0:
        return "none"
    table = np.zeros((iterations, 4), np.int32)
    assert lib.lpslam_pnp_sample_table(n, iterations, C.c_uint32(seed), table.ctypes.data_as(C.c_void_p)) == 1

    def solve(rows):
        o = S.run(lib, "epnp", {"n": int(len(s["pw"][rows]))}, dict(pw=c64(s["pw"][rows]), uv=c64(s["obs"][rows]), cam=CAM))
        return (o["R"], o["t"]) if o["ok"][0] else None

    def inliers(R, t):
        X, obs = s["pw"], s["obs"]
        xc = R[0] * X[:, 0] + R[1] * X[:, 1] + R[2] * X[:, 2] + t[0]; yc = R[3] * X[:, 0] + R[4] * X[:, 1] + R[5] * X[:, 2] + t[1]
        z = R[6] * X[:, 0] + R[7] * X[:, 1] + R[8] * X[:, 2] + t[2]
        with np.errstate(all="ignore"):
            du = CAM[0] * xc / z + CAM[2] - obs[:, 0]; dv = CAM[1] * yc / z + CAM[3] - obs[:, 1]
            return (z > 0) & ((du * du + dv * dv) * s["w"] < 5.991)
    best, flags = 0, None
    for row in table:
        h = solve(row)
        if h is not None and inliers(*h).sum() > best:
            flags = inliers(*h); best = int(flags.sum())
    assert best >= 4
    h = solve(flags)
    if h is None:
        assert out["count"][0] == best
        return "unsolved"
    count = int(inliers(*h).sum())
    assert out["count"][0] == (count if count >= best else best)
    return "kept" if count >= best else "rejected"


def ransac_cases():
    for n in (3, 4, 5, 37, 300):
        for share in (0.0, 0.6):
            s = P.planted(n, share, 40 + n)
            for seed in (0, P.SEED):
                for iterations in (1, 7, 100):
                    yield n, share, s, seed, iterations


def sim3_cases():
    for n in (2, 3, 50):
        for fix_scale in (0, 1):
            for seed in range(3):
                rng = np.random.default_rng(500 + 10 * n + seed)
                s_true = 1.0 if fix_scale else 1.37
                x2 = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)])
                r = P.rot([0.2, 1.0, -0.1], 0.4); t = np.array([0.8, -0.1, 0.3])
                x1 = s_true * (x2 @ r.T) + t
                proj = lambda x: np.column_stack([CAM[0] * x[:, 0] / x[:, 2] + CAM[2], CAM[1] * x[:, 1] / x[:, 2] + CAM[3]])
                obs1 = proj(x1) + rng.normal(0, 0.3, (n, 2)); obs2 = proj(x2) + rng.normal(0, 0.3, (n, 2))
                x1n = x1 + rng.normal(0, 0.01, x1.shape)
                if n == 50:
                    bad = rng.random(n) < 0.3
                    x1n[bad] += rng.normal(0, 1.5, (int(bad.sum()), 3))
                w = 1.0 / (1.2 ** rng.integers(0, 4, n)) ** 2
                yield n, fix_scale, seed, dict(p1c=c64(x1n), p2c=c64(x2), obs1=c64(obs1), obs2=c64(obs2), is1=c64(w), is2=c64(w[::-1]), cam=CAM)


def main():
    from lpslam_amd import _build
    lib = C.CDLL(_build.host_library())
    cases = []
    for tag, n, a in eigen_cases():
        cases.append(("sym_eigen", "n %d, %s" % (n, tag), {"n": n}, dict(A=c64(a))))
    flipped = 0
    for tag, pw, uv in epnp_cases():
        n = len(pw)
        k = sign_flips(pw, uv) if n >= 4 and "refused" not in tag else 0
        flipped += k > 0
        cases.append(("epnp", "n %d, %s, %d guesses with the first landmark behind the camera" % (n, tag, k), {"n": n}, dict(pw=pw, uv=uv, cam=CAM)))
    assert flipped >= 1
    for n, share, s, seed, iterations in ransac_cases():
        cases.append(("pnp_ransac", "n %d, %d %% outliers" % (n, round(100 * share)), {"n": n, "iterations": iterations, "seed": int(seed)},
                      dict(pw=c64(s["pw"]), obs=c64(s["obs"]), w=c64(s["w"]), cam=CAM)))
    for n, fix_scale, seed, arrays in sim3_cases():
        cases.append(("sim3_ransac", "n %d, data seed %d" % (n, seed), {"n": n, "fix_scale": fix_scale, "iterations": 50, "seed": int(P.SEED)}, arrays))
    for name, sc in (("general", T.scene(seed=2)), ("planar", T.scene(planar=True, seed=21, r=T._rot([0.1, 1.0, 0.2], 0.14), t=[-0.6, -0.34, 0.14], slope=(1.16, -0.82)))):
        kp_ref, kp_cur, matches = sc[:3]
        cases.append(("two_view", name + " scene", {"n": len(matches), "sigma": 1.0, "iterations": 100, "seed": 12345},
                      dict(K=T.K, kp_ref=np.ascontiguousarray(kp_ref, np.float32), kp_cur=np.ascontiguousarray(kp_cur, np.float32), matches=np.ascontiguousarray(matches, np.int32))))
    outputs = [S.run(lib, fn, args, arrays) for fn, _, args, arrays in cases]
    # what the fixture must hold
    refits = {}
    for i, ((fn, tag, args, arrays), out) in enumerate(zip(cases, outputs)):
        if fn == "epnp":
            assert bool(out["ok"][0]) == ("refused" not in tag), tag
        if fn == "pnp_ransac":
            s = dict(pw=arrays["pw"], obs=arrays["obs"], w=arrays["w"])
            what = refit_outcome(lib, s, args["iterations"], args["seed"], out) if args["n"] >= 4 else "none"
            refits[what] = refits.get(what, 0) + 1
            cases[i] = (fn, tag + ", refit " + what, args, arrays)
        if fn == "sim3_ransac":
            assert (out["count"][0] > 0) == (args["n"] >= 3), tag
        if fn == "two_view":
            assert out["ok"][0] == 1 and out["parallax_deg"][0] > 2.0, (tag, out["parallax_deg"])      # the threshold is 1 degree
    assert refits.get("kept", 0) >= 1 and refits.get("rejected", 0) >= 1, refits
    S.save(OUT, cases, outputs)
    print(os.path.basename(OUT), os.path.getsize(OUT), "bytes,", len(cases), "cases; refits", refits, "; epnp sets with a sign flip", flipped)


if __name__ == "__main__":
    main()
