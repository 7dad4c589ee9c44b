"""Device side of the solver-level tests (tests/test_ba_solve_gpu.py, tools/solve_accuracy.py): problems that lend their reduced
buffers to lpslam_hip_ba_debug_solve, the reduced systems of real windows read through the step API, and the accuracy figures."""
import ctypes as C
import math

import numpy as np

import solve_cases as sc
from lpslam_amd import synth

CW_MIN_BATCH = 40                    # LPSLAM_HIP_CW_MIN_BATCH (include/lpslam_hip.h): batches from here on take k_chol_wg
CHAIN, WG = "k_chol_pair + k_chol_xsolve", "k_chol_wg"
REAL_KINDS = ("random", "mono", "empty-kf")


class Holders:
    """Built problems with the dense solver, by dimension.  Their observations do not matter; they are never optimised."""

    def __init__(self, hiplib, ctx):
        self.hip, self.ctx, self.pool = hiplib, ctx, {}

    def take(self, dim, k=1):
        assert dim % 6 == 0
        have = self.pool.setdefault(dim, [])
        if len(have) < k:
            free = dim // 6
            n_pts = max(40, free + 1)
            pr = synth.ba_problem(free + 1, n_pts, 3 * n_pts, 640, 480, seq_id=900 + free)
            obs = self.hip.ba_obs_array(pr)
            while len(have) < k:
                ba = self.hip.BundleAdjuster(self.ctx, pr["poses"], pr["fixed"], pr["points"], obs, pr["cam"])
                ba.set_solver("dense")
                have.append(ba)
        return have[:k]

    def drop(self, dim):
        for ba in self.pool.pop(dim, []):
            ba.close()

    def close(self):
        for dim in list(self.pool):
            self.drop(dim)

    # ---- the three ways a system is solved ----
    def solve(self, problems, cases):
        xs, flags = self.hip.ba_debug_solve(problems, [c["A"] for c in cases], [c["b"] for c in cases])
        return xs, [int(f) for f in flags]

    def alone(self, case, which=0):
        """one problem: the panel-pair chain"""
        xs, flags = self.solve([self.take(case["n"], which + 1)[which]], [case])
        return xs[0], flags[0]

    def wg_batch(self, cases):
        """CW_MIN_BATCH problems (the cases, repeated until the batch is full), every one of them small: k_chol_wg.  Returns the
        results of the cases' first copies and whether the context counted a k_chol_wg launch."""
        assert 0 < len(cases) <= CW_MIN_BATCH and all(c["n"] <= sc.WG_MAX_DIM for c in cases)
        full = [cases[i % len(cases)] for i in range(CW_MIN_BATCH)]
        return self.batch(full, len(cases))

    def batch(self, full, keep=None):
        used, probs = {}, []
        for c in full:
            i = used.get(c["n"], 0); used[c["n"]] = i + 1
            probs.append(self.take(c["n"], i + 1)[i])
        before = self.ctx.ba_wg_factorisations()
        xs, flags = self.solve(probs, full)
        keep = len(full) if keep is None else keep
        return xs[:keep], flags[:keep], self.ctx.ba_wg_factorisations() - before


# ---- band windows -------------------------------------------------------------------------------------------------------------
BAND = "k_chol_band"


def free_span(pr):
    """the widest span of free slots a landmark covers: the block half-bandwidth lpslam_hip_ba_create finds"""
    slot = np.cumsum(pr["fixed"] == 0) - 1
    sl = np.where(pr["fixed"][pr["obs_pose"]] == 0, slot[pr["obs_pose"]], -1)
    free = sl >= 0
    lo = np.full(len(pr["points"]), 1 << 30); hi = np.full(len(pr["points"]), -1)
    np.minimum.at(lo, pr["obs_point"][free], sl[free]); np.maximum.at(hi, pr["obs_point"][free], sl[free])
    return int((hi - lo)[hi >= 0].max())


def band_window(free, hbw, n_pts=None, seq=0):
    """a synth.ba_problem window of `free` free keyframes with contiguous tracks whose landmarks span exactly `hbw` free slots at most:
    the track cap is hbw + 2 keyframes (the fixed first keyframe may be one of them), and what a landmark has beyond hbw slots behind
    its first free one is dropped"""
    assert 0 <= hbw <= min(9, free - 1)
    n_kf = free + 1
    n_pts = n_pts or max(60, 6 * n_kf)
    pr = synth.ba_problem(n_kf, n_pts, max(3, hbw + 2) * n_pts, 640, 480, seq_id=800 + free + 100 * hbw + seq, tracks="contiguous")
    slot = np.cumsum(pr["fixed"] == 0) - 1
    sl = np.where(pr["fixed"][pr["obs_pose"]] == 0, slot[pr["obs_pose"]], -1)
    lo = np.full(n_pts, 1 << 30)
    np.minimum.at(lo, pr["obs_point"][sl >= 0], sl[sl >= 0])
    keep = (sl < 0) | (sl <= lo[pr["obs_point"]] + hbw)
    for k in ("obs_pose", "obs_point", "obs_uvr", "obs_inv_sigma2"):
        pr[k] = pr[k][keep]
    assert free_span(pr) == hbw, (free, hbw, free_span(pr))
    return pr


class BandHolders:
    """Built problems that stay on the band solver, by (dimension, block half-bandwidth).  They are never optimised."""

    def __init__(self, hiplib, ctx):
        self.hip, self.ctx, self.pool = hiplib, ctx, {}

    def take(self, dim, k=1, hbw=None):
        assert dim % 6 == 0
        free = dim // 6
        hbw = min(9, free - 1) if hbw is None else hbw
        have = self.pool.setdefault((dim, hbw), [])
        if len(have) < k:
            pr = band_window(free, hbw)
            obs = self.hip.ba_obs_array(pr)
            while len(have) < k:
                ba = self.hip.BundleAdjuster(self.ctx, pr["poses"], pr["fixed"], pr["points"], obs, pr["cam"])
                assert ba.solver() == ("band", hbw), (dim, ba.solver())
                have.append(ba)
        return have[:k]

    def close(self):
        for key in list(self.pool):
            for ba in self.pool.pop(key):
                ba.close()

    def holder_for(self, case, which=0):
        """a holder whose band takes the case: 6 hbw + 5 >= w"""
        hbw = -(-(case["w"] - 5) // 6)
        assert 6 * hbw + 5 >= case["w"]
        return self.take(case["n"], which + 1, hbw)[which]

    def solve(self, problems, cases):
        xs, flags = self.hip.ba_debug_solve(problems, [c["A"] for c in cases], [c["b"] for c in cases])
        return xs, [int(f) for f in flags]

    def alone(self, case, which=0):
        xs, flags = self.solve([self.holder_for(case, which)], [case])
        return xs[0], flags[0]

    def batch(self, cases):
        """every case on a holder of its own, in one call"""
        used, probs = {}, []
        for c in cases:
            i = used.get(c["n"], 0); used[c["n"]] = i + 1
            probs.append(self.holder_for(c, i))
        return self.solve(probs, cases)


def real_band_case(hiplib, ctx, free, hbw):
    """S + lambda_0 I and rhs of the first LM trial of a contiguous-track window, read as real_case reads them (dense solver, step API);
    the dense kernel's S is exactly zero outside the block band: the pair lists have no list there"""
    n_kf = free + 1
    pr = band_window(free, hbw, n_pts=max(150, 8 * n_kf), seq=50)
    ba = hiplib.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hiplib.ba_obs_array(pr), pr["cam"])
    assert ba.solver() == ("band", hbw)
    ba.set_solver("dense")
    S, rhs, lam0, _ = first_trial_system(ba, 6 * free)
    ba.close()
    blk = np.arange(6 * free) // 6
    outside = np.abs(blk[:, None] - blk[None, :]) > hbw
    assert not S[outside].any(), "the dense Schur complement of a band window has entries outside the block band"
    A = np.tril(S) + np.tril(S, -1).T
    A[np.arange(len(A)), np.arange(len(A))] += lam0
    c = sc.case_from(A, rhs, "real-band%d" % hbw)
    c["w"] = 6 * hbw + 5
    assert sc.half_bandwidth(A) <= c["w"]
    return c


REAL_BAND = ((9, 3), (30, 9), (50, 9))          # (free keyframes, block half-bandwidth)


# ---- real windows -----------------------------------------------------------------------------------------------------------
def real_window(kind, free):
    """a synth.ba_problem window with `free` free keyframes: random tracks; the same kind with monocular observations only; one
    whose last keyframe has no observation at all"""
    seq = 700 + free + 1000 * REAL_KINDS.index(kind)
    n_kf = free + 1 - (1 if kind == "empty-kf" and free > 1 else 0)
    n_pts = max(150, 8 * n_kf)
    pr = synth.ba_problem(n_kf, n_pts, 5 * n_pts, 640, 480, seq_id=seq)
    if kind == "mono":
        pr["obs_uvr"] = pr["obs_uvr"].copy(); pr["obs_uvr"][:, 2] = -1.0
    if kind == "empty-kf" and free > 1:
        last = pr["poses"][-1].copy(); last[4:] += 0.3
        pr["poses"] = np.vstack([pr["poses"], last]); pr["poses_gt"] = np.vstack([pr["poses_gt"], last])
        pr["fixed"] = np.append(pr["fixed"], np.uint8(0))
    assert int((pr["fixed"] == 0).sum()) == free
    return pr


def _memcpy(lib):
    # through the library's own handle: the HIP runtime it is linked against, whatever else is loaded
    f = lib.hipMemcpy
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return f


def device_read(lib, ptr, n):
    """n doubles of device memory (the step API has synchronised the stream that wrote them)"""
    buf = np.zeros(int(n))
    assert _memcpy(lib)(buf.ctypes.data, ptr, buf.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return buf


def device_write(lib, ptr, values):
    buf = np.ascontiguousarray(values, np.float64)
    assert _memcpy(lib)(ptr, buf.ctypes.data, buf.nbytes, 1) == 0          # hipMemcpyHostToDevice


def padded_dim(red_n):
    """the reduced buffer holds S (n x n) | rhs | b_p | diag H_pp (n each) | 8 scalars"""
    n = (math.isqrt(4 * red_n - 23) - 3) // 2
    assert n * n + 3 * n + 8 == red_n
    return n


def first_trial_system(ba, dim, robust=True):
    """The first LM trial of a window brought to the point in front of its solve, as dist_ba.PartitionedBA does on one rank.
    Returns (S as the device holds it: the dim x dim corner of the reduced buffer, rhs, lambda_0, the padded dimension).
    lambda_0 is what lm_begin sets, 1e-5 max(max diag H_pp, max diag H_ll): status() reports lambda only behind a step_end."""
    ba.step_begin(robust, True)
    ba.step_lambda0()
    ba.step_begin(robust, False)
    ptr, red_n = ba.reduced_buffer()
    n = padded_dim(red_n)
    sp, _ = ba.scalar_buffer()
    h = device_read(ba.lib, ptr, red_n)
    S = h[:n * n].reshape(n, n)[:dim, :dim].copy()
    rhs = h[n * n:n * n + dim].copy()
    hpp = h[n * n + 2 * n:n * n + 2 * n + dim]
    max_ll = float(device_read(ba.lib, sp, 8)[4]) if ba.n_points else 0.0
    lam0 = 1e-5 * max(max_ll, float(np.abs(hpp).max()))
    return S, rhs, lam0, n


def read_S(ba, n):
    """the padded n x n matrix of the reduced buffer"""
    return device_read(ba.lib, ba.reduced_buffer()[0], n * n).reshape(n, n)


def real_case(hiplib, ctx, kind, free):
    pr = real_window(kind, free)
    ba = hiplib.BundleAdjuster(ctx, pr["poses"], pr["fixed"], pr["points"], hiplib.ba_obs_array(pr), pr["cam"])
    ba.set_solver("dense")
    S, rhs, lam0, _ = first_trial_system(ba, 6 * free)
    # the trial itself, for lambda: g2o multiplies lambda_0 by a factor in [1/3, 2/3] behind an accepted trial and by 2 behind a rejected one
    ba.step_solve()
    accepted, _ = ba.step_end()
    lam = ba.status()["lam"]
    ba.close()
    assert (1 / 3 - 1e-12 <= lam / lam0 <= 2 / 3 + 1e-12) if accepted else lam == 2 * lam0, (lam, lam0, accepted)
    A = np.tril(S) + np.tril(S, -1).T                   # the lower triangle (k_ba_schur sums the two triangles apart: they differ in the last bits)
    assert np.allclose(A, S, rtol=0, atol=1e-12 * np.abs(S).max())
    A[np.arange(len(A)), np.arange(len(A))] += lam0
    return sc.case_from(A, rhs, "real-" + kind)


# ---- figures ----------------------------------------------------------------------------------------------------------------
def row(case, x, kernel):
    e = sc.forward_error(x, case["x"])
    return dict(dim=case["n"], family=case["family"], kappa=case["kappa"], e_host=case["e_host"], e_dev=e,
                ratio=e / max(case["e_host"], sc.U), bound=sc.bound(case), kernel=kernel)


def format_row(r):
    return "%5d  %-12s %10.3e  %10.3e  %10.3e  %8.2f  %10.3e  %s" % (r["dim"], r["family"], r["kappa"], r["e_host"], r["e_dev"], r["ratio"], r["bound"], r["kernel"])


HEADER = "  dim  family          kappa_2      e_host       e_dev     ratio   n k 2^-53  kernel"
