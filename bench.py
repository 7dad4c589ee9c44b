#!/usr/bin/env python3
"""bench.py -- throughput of the lpslam hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1] + configs[2], the configuration the metric is quoted on): ONE SLAM session per GPU,
1280x720 stereo, 2000 keypoints / image, 8 pyramid levels, a 300-frame synthetic sequence of which a
ring of RESIDENT frames lives in HBM.  One "step" = 16 stereo frames in one launch (frames_per_launch 16):
    ORB extraction of 32 images, 16 stereo matches, 16 temporal brute-force matches (2000 x 2000, frame k vs k-1),
    + the local bundle adjustment of every keyframe among them (every 6th frame: 2.67 per step on average): a FRESH
      problem each time -- lpslam_hip_ba_create (structure phase, g2o's buildStructure, inside the timed region),
      10 LM iterations with Huber, destroy -- 50 keyframes / 5000 landmarks / ~39k stereo observations.
The bundle adjustments run on their own stream and host thread beside the front end, as the reference's mapping thread
runs beside tracking; a session's windows are solved one after the other (they depend on each other).
value = frames/s over the whole job (all ranks); N > 1 runs one independent session per GPU (replicas, no data-path
collective, "weak" scaling).  A plain run sets up, warms up, times the K steps and prints the headline line.  With --full
the line also carries the roofline of the kernel with the largest share of GPU time (every timed kernel is a candidate:
HIP events on the stream the kernel runs on), the PCIe-inclusive and contiguous-track legs, the extras and the CPU oracle
on a bounded sample.  --dump-outputs DIR writes what the timed path computed in its last step (dump_outputs below).
"""
import argparse
import json
import os
import sys
import threading
import time, tempfile

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

W, H, KPTS, LEVELS = 1280, 720, 2000, 8
FRAMES_PER_STEP = 16          # batched mode, B = 16 frames per launch
KF_INTERVAL = 6               # keyframe every 6th frame
RESIDENT = 48                 # stereo frames of the sequence resident in HBM (3 steps of 16; the ring is re-walked)
BA_KF, BA_PTS, BA_OBS, BA_ITERS = 50, 5000, 40000, 10
BA_VARIANTS = 4               # distinct windows (problem seeds) the keyframes rotate through
# compute units of every XCD the front end's extraction kernels leave to the mapping solves that run beside them
# (lpslam_hip_set_mapping_reserve: kept in software by persistent work-queue grids since round 4, no CU-masked stream).  The
# front-end-only and batched extras run with 0.
MAPPING_RESERVE = int(os.environ.get("LPSLAM_BENCH_RESERVE", "16"))
HBM_PEAK_GBS = 8000.0         # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s spec, 6.29 measured copy)
FP64_PEAK_TFLOPS = 78.6       # MI355X FP64 matrix = vector peak (MI355X_MICROARCH.md / SURVEY.md 8(d))
INT_PEAK_TOPS = 39.3          # 256 CU x 64 lanes x 2.4 GHz int32 VALU ops (matching)

# timer slots of the front-end stages
T_PYR, T_FAST, T_DIST, T_DESC, T_STEREO, T_BF = range(6)
FE_STAGES = ["pyramid", "fast", "distribute", "describe", "stereo", "bf"]
FE_KERNEL = {"pyramid": "k_pyr_bands", "fast": "k_fast_cells", "distribute": "k_distribute", "describe": "k_describe",
             "stereo": "k_stereo", "bf": "k_bf_knn2"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)          # (20 steps were 72 ms of timed region: differences below 3 % drowned in it)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=FRAMES_PER_STEP, help="stereo frames per step (per launch)")
    ap.add_argument("--full", action="store_true", help="after the timed steps, everything else the benchmark measures: PCIe-inclusive and "
                    "contiguous-track legs, instrumented passes and rooflines, extras, CPU baseline, partitioned global BA (N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write what the timed path computed in its last step as DIR/<name>.npy")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline leg")
    ap.add_argument("--no-ba", action="store_true", help="front end only (BASELINE configs[1])")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)            # internal: an extra that needs a process of its own (tracker_multi)
    ap.add_argument("--device", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the untimed extras (latency mode, batched sessions, trackers, global BA): profiling runs")
    return ap.parse_args()


class Workload:
    """One SLAM session: a ring of resident stereo frames + the windows its keyframes trigger."""

    def __init__(self, device, seq_id, frames, with_ba=True, resident=RESIDENT):
        from lpslam_amd import hip, synth
        self.hip, self.synth = hip, synth
        self.F = frames
        self.R = max(resident // frames, 1) * frames           # ring length: a whole number of steps
        self.k = synth.intrinsics(W, H)
        self.ctx = hip.Context(W, H, KPTS, 1.2, LEVELS, max_images=2 * self.R, device=device)
        seq = synth.StereoSequence(W, H, seq_id)
        # the sequence's frames live in page-locked host memory of the context (what a capture layer fills): the PCIe-inclusive
        # leg copies every frame it extracts from there, on the context's copy stream
        self.host_frames = [tuple(self.ctx.host_frame(img) for img in seq.frame(i)) for i in range(self.R)]
        for i, (l, r) in enumerate(self.host_frames):
            self.ctx.upload(2 * i, l); self.ctx.upload(2 * i + 1, r)
        self.with_ba = with_ba
        self.frame_counter = 0          # frames fed so far (front-end thread)
        self.kf_counter = 0             # keyframes solved so far (BA thread)
        self.last_windows = []          # (poses, landmarks, LM log) of the last windows run_steps(..., keep=n) solved
        if with_ba:
            # two kinds of window (synth.ba_problem): "random" -- every landmark keeps a random 8-9 of the ~50 keyframes that see it, the
            # reduced system is dense: the stress case and the headline of rounds 1-3 -- and "contiguous" -- a landmark is seen by a run
            # of neighbouring keyframes, as a tracker produces them: block-banded reduced system, the band path (ba_band.inl).
            # Both at SURVEY 8(d) config 3's size: 50 KF / 5000 landmarks / 40 000 +- 2 % observations (top_up).  A kind is generated
            # when it is first used: the timed loop runs "random", only --full also runs "contiguous".
            self.seq_id = seq_id
            self.prob_sets, self.obs_sets = {}, {}
            self.set_tracks("random")
        self.ctx.sync()

    def set_tracks(self, kind):
        if kind not in self.prob_sets:
            self.prob_sets[kind] = [self.synth.ba_problem(BA_KF, BA_PTS, BA_OBS, W, H, self.seq_id * BA_VARIANTS + v, tracks=kind, top_up=True)
                                    for v in range(BA_VARIANTS)]
            self.obs_sets[kind] = [self.hip.ba_obs_array(p) for p in self.prob_sets[kind]]
        self.tracks = kind
        self.probs, self.obs = self.prob_sets[kind], self.obs_sets[kind]
        self.n_obs = int(np.mean([len(o) for o in self.obs]))

    # ---- front end: one launch sequence for the F frames of step `s` (ring position)
    def front_end(self, s):
        c, F = self.ctx, self.F
        f0 = (s * F) % self.R
        c.extract_range(2 * f0, 2 * F)
        c.match_stereo_strided(2 * f0, 2 * f0 + 1, 2, F, self.k["fxb"], self.k["baseline"])
        if F > 1:
            c.match_bf_strided(2 * f0 + 2, 2 * f0, 2, F - 1)
        c.match_bf(2 * f0, 2 * ((f0 - 1) % self.R))          # first frame of this step against the last frame before it

    def upload_step(self, s):
        """the 2 F images of step `s` from page-locked host memory into their ring slots: asynchronous, on the copy stream, ordered
        behind whatever the context has been given so far (lpslam_hip_upload_images_async); the step's extraction waits for it"""
        f0 = (s * self.F) % self.R
        self.ctx.upload_async(2 * f0, [img for fr in self.host_frames[f0:f0 + self.F] for img in fr])

    def keyframes_of_step(self, s):
        g0 = s * self.F
        return sum(1 for g in range(g0, g0 + self.F) if g % KF_INTERVAL == 0)

    def new_problem(self, v, build=True):
        p = self.probs[v % BA_VARIANTS]
        return self.hip.BundleAdjuster(self.ctx, p["poses"], p["fixed"], p["points"], self.obs[v % BA_VARIANTS], p["cam"], build=build)

    def bundle_adjust_fresh(self):
        """what a keyframe costs the mapping side, unpipelined: structure phase + 10 LM iterations + read-back + release"""
        v = self.kf_counter
        ba = self.new_problem(v)
        self.kf_counter += 1
        log = ba.optimize(True, BA_ITERS)
        ba.state()
        ba.close()
        return log

    def bundle_adjust_pipelined(self, n_kf, keep=0):
        """The mapping thread as a pipeline: the structure of window k+1 (upload + device-side build, asynchronous on its own stream)
        is set up while window k is being solved; when k is done its poses / landmarks are read back and window k+1 receives its
        values (lpslam_hip_ba_set_state) -- in a tracker the observations the previous solve classified as outliers would be masked
        with set_active at the same point.  Every window is still created, solved, read back and released inside the timed region.
        The read-back and LM log of the last `keep` windows are kept in self.last_windows."""
        self.last_windows = []
        if n_kf <= 0:
            return
        def start(ba, v):
            p = self.probs[v % BA_VARIANTS]
            ba.set_state(p["poses"], p["points"])
            ba.optimize_begin(True, BA_ITERS)
        cur = self.new_problem(self.kf_counter)
        start(cur, self.kf_counter)
        for i in range(n_kf):
            self.kf_counter += 1
            nxt = self.new_problem(self.kf_counter) if i + 1 < n_kf else None     # builds beside the running solve
            log = cur.optimize_end()
            if nxt is not None:
                start(nxt, self.kf_counter)                  # the next solve is on its way before the finished one is read back
            poses, points = cur.state()
            if i >= n_kf - keep:
                self.last_windows.append((poses, points, log))
            cur.close()
            cur = nxt

    def front_end_steps(self, first_step, k, upload):
        """resident: the frames are in HBM already.  upload: every step's frames come over PCIe inside the loop -- the copies of step
        s + 2 are enqueued (copy stream) before the kernels of step s, so they run beside the kernels of two steps"""
        ahead = self.R // self.F - 1                     # steps of the ring that may be in flight beside the one being extracted (2)
        if upload:
            for s in range(first_step, min(first_step + ahead, first_step + k)):
                self.upload_step(s)
        for s in range(first_step, first_step + k):
            if upload and s + ahead < first_step + k:
                self.upload_step(s + ahead)              # overwrites the ring position of step s - 1: ordered behind its kernels
            self.front_end(s)

    def run_steps(self, first_step, k, upload=False):
        """k steps: the front end on this thread, the keyframes' bundle adjustments on a second one (own stream); the windows of
        the last step stay in self.last_windows"""
        if not self.with_ba:
            self.front_end_steps(first_step, k, upload)
            self.ctx.sync()
            return
        err = []
        n_kf = sum(self.keyframes_of_step(s) for s in range(first_step, first_step + k))
        n_last = self.keyframes_of_step(first_step + k - 1) if k > 0 else 0

        def ba_loop():
            try:
                self.bundle_adjust_pipelined(n_kf, keep=n_last)
            except Exception as e:      # noqa: BLE001
                err.append(e)
        th = threading.Thread(target=ba_loop)
        th.start()
        self.front_end_steps(first_step, k, upload)
        self.ctx.sync()
        th.join()
        if err:
            raise err[0]

    # ---- instrumented pass: HIP events around every front-end stage on the context stream
    def front_end_timed(self):
        c, F = self.ctx, self.F
        for slot, stage in ((T_PYR, "pyramid"), (T_FAST, "fast"), (T_DIST, "distribute"), (T_DESC, "describe")):
            c.timer_begin(slot); c.stage(stage, 2 * F); c.timer_end(slot)
        c.timer_begin(T_STEREO); c.match_stereo_strided(0, 1, 2, F, self.k["fxb"], self.k["baseline"]); c.timer_end(T_STEREO)
        c.timer_begin(T_BF)
        if F > 1:
            c.match_bf_strided(2, 0, 2, F - 1)
        c.match_bf(0, 2 * F - 2)
        c.timer_end(T_BF)
        c.sync()
        return [c.timer_ms(s) for s in range(len(FE_STAGES))]

    # ---- algorithmic work per step
    def level_pixels(self):
        return [w * h for w, h in zip(self.ctx.level_w, self.ctx.level_h)]

    def extract_bytes(self):
        """B_img = (P - P_7) + (P - P_0) + P + 2P + 2 K 31^2 + 60 K per image (17 236 083 B at 1280x720 / 2000)."""
        P = self.level_pixels(); Ps = sum(P)
        return 2 * self.F * ((Ps - P[-1]) + (Ps - P[0]) + Ps + 2 * Ps + 2 * KPTS * 31 * 31 + 60 * KPTS)

    def stage_work(self):
        """algorithmic work of one launch of each front-end stage: (amount, unit, bound, peak)"""
        P = self.level_pixels(); Ps = sum(P); n_img = 2 * self.F; K = KPTS
        return {
            "pyramid": (n_img * ((Ps - P[-1]) + (Ps - P[0])), "B", "hbm", HBM_PEAK_GBS * 1e9),
            "fast": (n_img * Ps, "B", "hbm", HBM_PEAK_GBS * 1e9),
            "distribute": (None, "B", "hbm", HBM_PEAK_GBS * 1e9),          # 4 B x candidates: data dependent, filled in by the caller
            "describe": (n_img * (2 * K * 31 * 31 + K * 60), "B", "hbm", HBM_PEAK_GBS * 1e9),
            "stereo": (None, "B", "hbm", HBM_PEAK_GBS * 1e9),
            "bf": (self.F * 2 * K * K * 8, "op", "valu", INT_PEAK_TOPS * 1e12),   # xor + popcount per 32-bit word pair
        }


def ba_flops(prob, dim, block_half_bandwidth=-1):
    """linearise ~520 FLOP/obs, Schur sum_j(216 n_j^2 + 108 n_j + 50), Cholesky dim^3/3, back-sub + chi2 ~150 FLOP/obs.
    A block-banded system (half-bandwidth hb = 6 w + 5 scalars): band Cholesky n (hb^2 + 3 hb) + the two substitutions 4 n hb."""
    n_obs = len(prob["obs_pose"])
    nj = np.bincount(prob["obs_point"], minlength=len(prob["points"])).astype(np.float64)
    schur = float((216 * nj * nj + 108 * nj + 50).sum())
    n = dim + 1                      # the rhs rides along as one more row
    if block_half_bandwidth >= 0:
        hb = 6.0 * block_half_bandwidth + 5.0
        chol = dim * (hb * hb + 3.0 * hb) + 4.0 * dim * hb
    else:
        chol = n ** 3 / 3.0 + 2.0 * n * n
    return {"linearise": 520.0 * n_obs, "schur": schur, "cholesky": chol, "backsub": 150.0 * n_obs}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(wl, step, out_dir):
    """What the timed path computed in its last step `step`, as a caller of it receives it, one float32 / float64 .npy file per array:
    keypoints (x, y, size, angle, response, octave, class_id) and descriptors (32 bytes as values) of the step's 2F images, left and
    right of every frame in turn, concatenated (`keypoint_counts`: per image); the stereo matches of its F left images (x_right,
    depth, index of the right keypoint) and their temporal brute-force matches (best index, best and second distance); the poses,
    landmarks and LM log (chi2_before, chi2_after, lambda, trials, status; NaN past the last iteration) of the windows solved for
    the step's keyframes.  Over DUMP_LIMIT_BYTES in all, every array keeps the same fixed, seeded sample of its rows."""
    c, F = wl.ctx, wl.F
    f0 = (step * F) % wl.R
    images = range(2 * f0, 2 * f0 + 2 * F)
    lefts = range(2 * f0, 2 * f0 + 2 * F, 2)
    kps, descs = zip(*[c.keypoints(i) for i in images])
    stereo = [c.stereo(i) for i in lefts]
    bf = [c.bf_knn2(i) for i in lefts]
    kp_all = np.concatenate(kps)
    out = {
        "keypoint_counts": np.array([len(k) for k in kps], np.float64),
        "keypoints": np.stack([kp_all[f].astype(np.float32) for f in kp_all.dtype.names], axis=1),
        "descriptors": np.concatenate(descs).astype(np.float32),
        "stereo_x_right": np.concatenate([s[0] for s in stereo]).astype(np.float32),
        "stereo_depth": np.concatenate([s[1] for s in stereo]).astype(np.float32),
        "stereo_index": np.concatenate([s[2] for s in stereo]).astype(np.float64),
        "bf_knn2": np.stack([np.concatenate([b[j] for b in bf]) for j in range(3)], axis=1).astype(np.float64),
    }
    if wl.with_ba:
        logs = np.full((len(wl.last_windows), BA_ITERS, 5), np.nan)
        for w, (_, _, log) in enumerate(wl.last_windows):
            logs[w, :len(log)] = np.stack([log[f].astype(np.float64) for f in log.dtype.names], axis=1)
        out["ba_poses"] = np.array([p for p, _, _ in wl.last_windows], np.float64).reshape(-1, BA_KF, 7)
        out["ba_points"] = np.array([x for _, x, _ in wl.last_windows], np.float64).reshape(-1, BA_PTS, 3)
        out["ba_log"] = logs
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        frac = DUMP_LIMIT_BYTES / total
        for name, a in out.items():
            m = int(len(a) * frac)
            out[name] = a[np.sort(np.random.default_rng(0).choice(len(a), m, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU baseline: the oracle (CPU restatement of the OpenVSLAM / g2o algorithms) on a bounded sample of the same workload
# ---------------------------------------------------------------------------------------------------------------------------------
def _cpu_frames(O, synth, n):
    seq = synth.StereoSequence(W, H, 0)
    return [seq.frame(i) for i in range(n)]


def _cpu_front_end(O, p, k, frames):
    prev = None
    for l, r in frames:
        kl, dl, _, pl = O.extract(l, p, True)
        kr, dr, _, pr = O.extract(r, p, True)
        O.match_stereo(pl, pr, p, kl, dl, kr, dr, k["fxb"], k["baseline"])
        O.match_bf_knn2(dl, prev if prev is not None else dl)
        prev = dl


def front_end_valu_issue():
    """The bound the extraction kernels run against, profile-derived like `traffic`: vector-instruction issue, priced against the MEASURED
    ceiling.  tools/dev/valu_issue_bench.hip (profiles/r05_valu_issue.txt): a gfx950 compute unit issues 1.75 wave64 instructions of
    the 32-bit encoded kind (VOP1 / VOP2) and 0.96 of the wide kinds (VOP3 / VOP3P) per shader-clock cycle, at 2.15 - 2.40 GHz under
    load; a kernel's ceiling is the harmonic mix over its (static) instruction mix (tools/valu_mix.py).  floor_us = SQ_INSTS_VALU per
    launch / (compute units x clock x ceiling), from the newest profiles/<tag>_pmc.json and the kernel statistics of the same tag."""
    try:
        import csv
        pdir = os.path.join(ROOT, "profiles")
        tags = sorted(f[:-len("_pmc.json")] for f in os.listdir(pdir) if f.endswith("_pmc.json") and os.path.exists(os.path.join(pdir, f[:-len("_pmc.json")] + "_bench_kernel_stats.csv")))
        mixes = sorted(f for f in os.listdir(pdir) if f.endswith("_valu_mix.json"))
        if not tags or not mixes:
            return None
        tag = tags[-1]
        pmc = json.load(open(os.path.join(pdir, tag + "_pmc.json")))
        mix = json.load(open(os.path.join(pdir, mixes[-1])))
        kern = pmc.get("kernels", pmc)
        dur = {}
        for r in csv.DictReader(open(os.path.join(pdir, tag + "_bench_kernel_stats.csv"))):
            dur[r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].replace("<true>", "").replace("<false>", "")] = float(r["AverageNs"]) / 1e3
        clock_ghz = 2.3
        out = {"source": "profiles/%s_pmc.json + _bench_kernel_stats.csv; ceilings: profiles/%s (rates measured: profiles/r05_valu_issue.txt)" % (tag, mixes[-1]), "clock_GHz": clock_ghz,
               "measured_issue_rates_per_cu_cycle": mix.get("rates_per_cu_cycle"),
               "note": "floor_us = SQ_INSTS_VALU per launch / (compute units x clock x measured issue ceiling of the kernel's instruction mix); the direct kernels use 256 compute units, the queued (_q) ones of the timed loop 128"}
        for name in ("k_fast_cells", "k_describe", "k_fast_cells_q", "k_describe_q"):
            v = kern.get(name)
            m = mix["kernels"].get(name)
            if v and m and "SQ_INSTS_VALU" in v and name in dur:
                cus = 128 if name.endswith("_q") else 256
                n = v["SQ_INSTS_VALU"]["mean_per_launch"]
                floor_us = n / (cus * clock_ghz * 1e3 * m["issue_ceiling_per_cu_cycle"])
                out[name] = {"valu_instructions_per_launch": int(n), "issue_ceiling_per_cu_cycle": m["issue_ceiling_per_cu_cycle"], "issued_per_cu_cycle": round(n / (cus * clock_ghz * 1e3 * dur[name]), 3),
                             "floor_us": round(floor_us, 1), "measured_us": round(dur[name], 1), "frac": round(floor_us / dur[name], 3)}
        return out
    except Exception as e:      # noqa: BLE001 -- profile-derived decoration only
        return {"error": str(e)}


def cpu_baseline():
    """Legs: (1) one thread, -O3 (the reference builds with BUILD_WITH_MARCH_NATIVE=OFF); (2) one thread,
    -march=native; (3) the reference's own threading: left / right extraction on two threads, local BA on a third; (4) all host
    cores, -march=native: independent frames and windows in parallel (ctypes releases the GIL).  Bounded: ~20 s of CPU in all."""
    from oracle import oracle as O
    from lpslam_amd import synth
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    n_visible = ncpu
    try:        # the cores this job may actually use: the cgroup's CPU quota where there is one, else the one-GPU share of the box (16)
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        ncpu = min(ncpu, max(1, int(int(quota) / int(period)))) if quota != "max" else min(ncpu, 16)
    except (OSError, ValueError):
        ncpu = min(ncpu, 16)
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip(); break
    except OSError:
        pass
    p = O.params(KPTS, 1.2, LEVELS)
    k = synth.intrinsics(W, H)
    frames = _cpu_frames(O, synth, 8)
    prob = synth.ba_problem(BA_KF, BA_PTS, BA_OBS, W, H, 0)
    obs = O.ba_obs(prob)

    def ba_once():
        O.ba_optimize(prob["poses"], prob["fixed"], prob["points"], obs, prob["cam"], True, BA_ITERS)

    def single(n_frames):
        t0 = time.perf_counter(); _cpu_front_end(O, p, k, frames[:n_frames]); t_front = (time.perf_counter() - t0) / n_frames
        t0 = time.perf_counter(); ba_once(); t_ba = time.perf_counter() - t0
        return t_front, t_ba

    legs = {}
    t_front, t_ba = single(6)
    legs["1_thread_O3"] = {"value": round(1.0 / (t_front + t_ba / KF_INTERVAL), 3), "unit": "frames/s", "cores": 1, "flags": "-O3",
                           "front_end_ms_per_frame": round(1e3 * t_front, 2), "ba_ms_per_iter": round(1e3 * t_ba / BA_ITERS, 3)}
    # the reference's own threading: left / right extraction on two threads (the std::async pair of
    # src/Trackers/OpenVSLAMStereoTracker.cpp:199-213), the local BA on a third (OpenVSLAM's mapping thread)
    t0 = time.perf_counter()
    th_ba = threading.Thread(target=ba_once); th_ba.start()
    prev = None
    for l, r in frames[:KF_INTERVAL]:
        res = {}
        th_r = threading.Thread(target=lambda: res.__setitem__("r", O.extract(r, p, True))); th_r.start()
        kl, dl, _, pl = O.extract(l, p, True)
        th_r.join()
        kr, dr, _, pr = res["r"]
        O.match_stereo(pl, pr, p, kl, dl, kr, dr, k["fxb"], k["baseline"])
        O.match_bf_knn2(dl, prev if prev is not None else dl)
        prev = dl
    th_ba.join()
    legs["3_threads_reference_threading_O3"] = {"value": round(KF_INTERVAL / (time.perf_counter() - t0), 3), "unit": "frames/s", "cores": 3, "flags": "-O3"}
    native_ok = True
    try:
        O.use_native_build(True)
    except Exception as e:      # noqa: BLE001 -- no compiler on the box: the default build stays
        native_ok = False
        legs["native_build_error"] = str(e)[:200]
    flags = "-O3 -march=native" if native_ok else "-O3"
    t_front_n, t_ba_n = single(6)
    legs["1_thread_native"] = {"value": round(1.0 / (t_front_n + t_ba_n / KF_INTERVAL), 3), "unit": "frames/s", "cores": 1, "flags": flags,
                               "front_end_ms_per_frame": round(1e3 * t_front_n, 2), "ba_ms_per_iter": round(1e3 * t_ba_n / BA_ITERS, 3)}
    # all cores: every thread runs whole keyframe intervals (6 frames + 1 window) of its own -- independent sequences in parallel
    n_thr = max(ncpu, 1)
    t0 = time.perf_counter()
    ths = [threading.Thread(target=lambda: (_cpu_front_end(O, p, k, frames[:KF_INTERVAL]), ba_once())) for _ in range(n_thr)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    t_all = time.perf_counter() - t0
    best = {"value": round(n_thr * KF_INTERVAL / t_all, 3), "unit": "frames/s", "cores": n_thr, "kind": "port", "flags": flags,
            "sample": "%d threads, each one keyframe interval of the workload (6 stereo frames: extract L+R, stereo match, 2000x2000 BF; one local BA of "
                      "%d LM iterations); CPU restatement of the OpenVSLAM / g2o algorithms, not OpenVSLAM itself" % (n_thr, BA_ITERS),
            "host": {"nproc": n_visible, "cores_used": ncpu, "cpu_model": model}}
    O.use_native_build(False)
    return best, legs


# ---------------------------------------------------------------------------------------------------------------------------------
def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks ourselves, exactly as the driver does
    (torch.distributed.run, one process per GPU, rendezvous on 127.0.0.1), as a CHILD process -- nothing in this process has
    touched torch or the GPU yet -- and leave with its exit code.  The ranks print the JSON line (rank 0) to our stdout."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def tracker_multi_child(device):
    """N sessions through the drop-in API at once: N LpSlamManager instances in ONE process on one GPU -- what BASELINE configs[3] runs per
    device when a node serves more sequences than it has GPUs, and the reference's deployment unit (one manager, one worker thread, one
    frame in flight per sequence: /root/reference/src/Manager/SlamManager.cpp:54-61,191-201).  Every manager has its own context, streams
    and worker; a feeder thread per manager enqueues its 120 frames; results are counted by the library's compiled callback.
    Aggregate = all results / wall time from the first enqueue to the last result.  Prints one JSON object."""
    from lpslam_amd import hip, manager, synth, _build
    hip.set_flat_priorities(True)                 # many sessions in one process: every stream at the default priority (lpslam_hip.h), before the first stream exists
    _build.host_library()
    k = synth.intrinsics(W, H)
    seq_t = synth.StereoSequence(W, H, 4)
    tr_frames = [seq_t.frame(i) for i in range(120)]

    def run(n_mgr, frames):
        mgs = []
        for i in range(n_mgr):
            mg = manager.Manager()
            for num in (0, 1):
                c = manager.default_camera()
                c.camera_number = num; c.f_x = k["fx"]; c.f_y = k["fy"]; c.c_x = k["cx"]; c.c_y = k["cy"]
                c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = k["fxb"]
                mg.set_camera(c)
            mg.add_tracker("VSLAMStereo", '{"cameraSetup": "stereo", "slamKeypoints": %d, "numLevels": %d, "keyframeInterval": %d, "device": %d}' % (KPTS, LEVELS, KF_INTERVAL, device))
            mg.count_results(); mg.provide_odometry(native=True)
            mg.start()
            mgs.append(mg)

        def feed(mg):
            for i, (l, r) in enumerate(frames):
                mg.add_stereo((i + 1) * 40_000_000, l, r)
        feeders = [threading.Thread(target=feed, args=(mg,)) for mg in mgs]
        t2 = time.perf_counter()
        for th in feeders:
            th.start()
        want = n_mgr * len(frames)
        while sum(mg.result_counts()[0] for mg in mgs) < want and time.perf_counter() - t2 < 120:
            time.sleep(0.001)
        t_all = time.perf_counter() - t2
        for th in feeders:
            th.join()
        counts = [mg.result_counts() for mg in mgs]
        for mg in mgs:
            mg.stop()
        return {"frames": int(sum(c[0] for c in counts)), "valid": int(sum(c[1] for c in counts)),
                "aggregate_frames_per_s": round(sum(c[0] for c in counts) / t_all, 1), "per_manager_frames_per_s": round(sum(c[0] for c in counts) / t_all / n_mgr, 1)}
    run(1, tr_frames[:30])                       # untimed: code objects, page-locked staging and the allocator's pools of a new process
    tm = {}
    for n_mgr in (8, 16):
        before = (hip.shared_launch_counters(device), hip.shared_front_end_counters(device), hip.shared_solve_counters(device))
        tm["managers_%d" % n_mgr] = run(n_mgr, tr_frames)
        after = (hip.shared_launch_counters(device), hip.shared_front_end_counters(device), hip.shared_solve_counters(device))
        # what the sessions shared: requests per launch of the window matchers + pose optimisers, of the front-end chains, of the windows' solves
        tm["managers_%d" % n_mgr]["requests_per_shared_launch"] = {name: round((a[1] - b[1]) / max(a[0] - b[0], 1), 2)
                                                                   for name, b, a in zip(("match_and_pose", "front_end", "local_ba"), before, after)}
    tm["note"] = ("a process of its own, as a server of many sessions runs; N LpSlamManager instances (each a session of the device's pool with its own worker, prefetch and mapping "
                  "threads) fed 120 stereo frames each by N threads; the sessions' pending front ends, window matchers, pose optimisations and local bundle adjustments go out as shared "
                  "launches on four role streams (lpslam_amd/csrc/share.hip); compiled odometry and result callbacks; one untimed 30-frame session first")
    print(json.dumps(tm))


def main():
    args = parse()
    if args.child == "tracker_multi":
        return tracker_multi_child(args.device)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    use_dist = world > 1 or os.environ.get("LPSLAM_BENCH_FORCE_DIST") == "1"      # the second: one-rank rehearsal of the N > 1 code path
    if use_dist:
        import torch            # noqa: F401  (before the HIP library: both must share one HIP runtime, torch's loads first)
        import torch.distributed  # noqa: F401
    from lpslam_amd import hip
    ndev = hip.device_count()
    if ndev < 1:
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    device = local_rank % ndev
    backend = os.environ.get("LPSLAM_BENCH_BACKEND", "nccl")      # "nccl" is RCCL on ROCm; "gloo" only for single-GPU rehearsals
    if world > ndev and backend == "nccl":
        raise SystemExit("bench.py --gpus %d: only %d HIP device(s) visible (one rank per GPU over RCCL; LPSLAM_BENCH_BACKEND=gloo "
                         "rehearses several ranks on one GPU)" % (world, ndev))
    if use_dist:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(device)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group(backend=backend)

    wl = Workload(device, rank, args.frames, with_ba=not args.no_ba)
    F = args.frames

    def sync_tensor(values, op=None):
        import torch
        t = torch.tensor(values, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=op or dist.ReduceOp.SUM)
        if backend == "nccl":
            torch.cuda.synchronize()
        return t

    def barrier():
        wl.ctx.sync()
        if dist is not None:
            sync_tensor([0.0])

    if wl.with_ba and MAPPING_RESERVE:
        try:
            wl.ctx.set_mapping_reserve(MAPPING_RESERVE)
        except Exception as e:      # noqa: BLE001  (a runtime without CU masks: run without the reserve and say so)
            print("mapping reserve not available: %s" % e, file=sys.stderr)
            globals()["MAPPING_RESERVE"] = 0
    wl.run_steps(0, args.warmup)
    barrier()
    t0 = time.perf_counter()
    wl.run_steps(args.warmup, args.steps)
    elapsed = time.perf_counter() - t0
    barrier()
    if dist is not None:
        elapsed = float(sync_tensor([elapsed], dist.ReduceOp.MAX).item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(wl, args.warmup + args.steps - 1, args.dump_outputs)
    n_kf_timed = sum(wl.keyframes_of_step(s) for s in range(args.warmup, args.warmup + args.steps)) if wl.with_ba else 0
    kf_per_step = n_kf_timed / max(args.steps, 1)
    frames_total = world * F * args.steps
    value = frames_total / elapsed
    head = {
        "metric": "frames/sec (ORB+match+local-BA), 1280x720 stereo",
        "value": round(value, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u8 front end / f64 BA", "data": "synthetic",
        "config": {"workload": "configs[1]+configs[2]: one session, 1280x720 stereo, 2000 kpts, 8 levels; step = %d stereo frames in one launch "
                               "(extract L+R, stereo match, 2000x2000 BF temporal match; ring of %d resident frames of the 300-frame sequence) + a fresh "
                               "50-KF/5k-landmark/%d-obs local BA (create + %d LM iterations + destroy) per keyframe (every %dth frame)"
                               % (F, wl.R, wl.n_obs if wl.with_ba else 0, BA_ITERS, KF_INTERVAL),
                   "frames_per_step": F, "frames_per_launch": F, "keyframes_per_step": round(kf_per_step, 3), "replicas": world, "parallelism": "replicas x%d" % world,
                   "mapping_reserve_cus_per_xcd": MAPPING_RESERVE if wl.with_ba else 0,
                   "ba_tracks": "random (dense reduced system; pair lists + panel-pair chain)"},
    }
    if not args.full:
        # a plain run: the headline line and nothing else
        if rank == 0:
            print(json.dumps(head), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    # the same K steps once more with every frame coming over PCIe inside the loop (page-locked host frames -> copy stream): the
    # PCIe-inclusive rate, reported beside `value` (which is quoted with the inputs resident, as the bench contract says)
    wl.run_steps(max(args.warmup - 1, 0), 1, upload=True)
    barrier()
    t0 = time.perf_counter()
    wl.run_steps(args.warmup, args.steps, upload=True)          # the same step indices: the same ring positions and keyframes
    elapsed_pcie = time.perf_counter() - t0
    barrier()
    if dist is not None:
        elapsed_pcie = float(sync_tensor([elapsed_pcie], dist.ReduceOp.MAX).item())
    # the same K steps with the keyframes' windows as a tracker makes them (contiguous tracks: block-banded reduced system, band path)
    elapsed_contig = None
    if wl.with_ba:
        wl.set_tracks("contiguous")
        wl.run_steps(max(args.warmup - 2, 0), min(2, args.warmup))
        barrier()
        t0 = time.perf_counter()
        wl.run_steps(args.warmup, args.steps)
        elapsed_contig = time.perf_counter() - t0
        barrier()
        if dist is not None:
            elapsed_contig = float(sync_tensor([elapsed_contig], dist.ReduceOp.MAX).item())
        wl.set_tracks("random")

    out = None
    if rank == 0:
        # ---- instrumented passes, outside the timed region: HIP events on the streams the kernels run on
        n_inst = max(3, min(args.steps, 10))
        fe_ms = np.mean([wl.front_end_timed() for _ in range(n_inst)], axis=0)        # as in the timed loop: under the mapping reserve
        fe_ms_free = fe_ms
        if wl.with_ba and MAPPING_RESERVE:
            # the front-end kernels on the whole chip (what their roofline is priced on); the timed loop gives them 256 - 8 r CUs
            wl.ctx.sync(); wl.ctx.set_mapping_reserve(0)
            fe_ms_free = np.mean([wl.front_end_timed() for _ in range(n_inst)], axis=0)
            wl.ctx.sync(); wl.ctx.set_mapping_reserve(MAPPING_RESERVE)
        def profile_ba():
            """set-up alone, HIP-event time per kernel of a solve, a keyframe's solve unpipelined and in the mapping pipeline (current track kind)"""
            ts = []
            for v in range(6):      # set-up alone: create until the structure is ready on the device (a state read synchronises)
                t1 = time.perf_counter(); b = wl.new_problem(v); b.state(); ts.append(1e3 * (time.perf_counter() - t1)); b.close()
            setup_ms = float(np.median(ts[1:]))
            acc, iters_done, dim, solver = {}, 0, 0, None
            for v in range(n_inst):
                b = wl.new_problem(v)
                solver = b.solver()
                prof, iters_done, dim = b.optimize_profiled(True, BA_ITERS)
                b.close()
                for name, (ms, marks, per) in prof.items():
                    a = acc.setdefault(name, [0.0, 0, per]); a[0] += ms; a[1] += marks
            prof = {n: {"ms_per_solve": a[0] / n_inst, "marks_per_solve": a[1] / n_inst, "launches_per_mark": a[2]} for n, a in acc.items()}
            ts = []
            for v in range(n_inst):
                t1 = time.perf_counter(); wl.bundle_adjust_fresh(); ts.append(1e3 * (time.perf_counter() - t1))
            total_ms = float(np.median(ts))
            # wall time of the graph-replayed solve alone (what the timed loop runs): optimize(10) on a resident problem, reset in between
            b = wl.new_problem(0); b.optimize(True, BA_ITERS); tw = []
            for _ in range(max(n_inst, 5)):
                b.reset(); b.state()
                t1 = time.perf_counter(); b.optimize(True, BA_ITERS); tw.append(1e3 * (time.perf_counter() - t1))
            b.close()
            profile_ba.wall_ms_per_iter = float(np.median(tw)) / BA_ITERS
            t1 = time.perf_counter(); wl.bundle_adjust_pipelined(8); pipe_ms = 1e3 * (time.perf_counter() - t1) / 8
            return prof, setup_ms, total_ms, iters_done, dim, pipe_ms, solver
        ba_prof, ba_setup_ms, ba_total_ms, ba_iters_done, ba_dim, ba_pipe_ms, ba_solver = None, None, None, 0, 0, None, None
        if wl.with_ba:
            ba_prof, ba_setup_ms, ba_total_ms, ba_iters_done, ba_dim, ba_pipe_ms, ba_solver = profile_ba()

        # ---- GPU time per step by kernel: the dominant one gets the roofline
        per_step = {FE_KERNEL[n]: float(ms) for n, ms in zip(FE_STAGES, fe_ms)}
        if ba_prof:
            for n, d in ba_prof.items():
                per_step["k_chol_factor" if n == "chol" else n] = d["ms_per_solve"] * kf_per_step
        dom = max(per_step, key=per_step.get)
        work = wl.stage_work()
        flops = ba_flops(wl.probs[0], ba_dim) if wl.with_ba else None
        roof = None
        if dom == "k_chol_factor":
            d = ba_prof["chol"]
            launches = d["marks_per_solve"] * d["launches_per_mark"]          # kernel launches per solve
            avg_ms = d["ms_per_solve"] / max(launches, 1)
            fl_per_launch = flops["cholesky"] * d["marks_per_solve"] / max(launches, 1)
            ach = fl_per_launch / (avg_ms * 1e-3) / 1e12
            roof = {"bound": "mfma", "kernel": hip.ba_factor_kernel_name(ba_dim, ba_solver is not None and ba_solver[0] == "band"), "launches_per_step": round(launches * kf_per_step, 2),
                    "achieved": round(ach, 4), "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / FP64_PEAK_TFLOPS, 6),
                    "algorithmic_flops_per_launch": int(fl_per_launch), "algorithmic_bytes_per_launch": int(8 * (ba_dim + 1) ** 2 * d["marks_per_solve"] / max(launches, 1)),
                    "avg_launch_us": round(1e3 * avg_ms, 3), "traffic": None,
                    "note": "FP64 dense factorisation of the %d x %d reduced system (n^3/3 + 2 n^2 FLOP per factorisation, SURVEY 8(d)) over the "
                            "launches of one factorisation; latency bound (serial panel chain), see DESIGN.md section 5" % (ba_dim + 1, ba_dim + 1)}
        elif dom in ("k_ba_schur", "k_ba_point_sum", "k_ba_backsub", "k_ba_trial", "k_ba_update", "k_ba_lin", "k_chol_xsolve"):
            d = ba_prof[dom]
            avg_ms = d["ms_per_solve"] / max(d["marks_per_solve"], 1)
            n_obs = len(wl.probs[0]["obs_pose"])
            nj = np.bincount(wl.probs[0]["obs_point"], minlength=len(wl.probs[0]["points"])).astype(np.float64)
            terms = float((nj * (nj + 1) / 2).sum())
            bytes_per_launch = {"k_ba_schur": 336.0 * terms, "k_ba_point_sum": 72.0 * n_obs, "k_ba_backsub": 144.0 * n_obs + 8.0 * (ba_dim + 1) ** 2,
                                "k_ba_trial": (64.0 + 40 + 144 + 72) * n_obs, "k_ba_update": (144.0 + 40 + 144 + 64) * n_obs, "k_ba_lin": (40.0 + 144 + 72) * n_obs, "k_chol_xsolve": 8.0 * (ba_dim + 1) ** 2}[dom]
            ach = bytes_per_launch / (avg_ms * 1e-3) / 1e9
            roof = {"bound": "hbm", "kernel": dom, "launches_per_step": round(d["marks_per_solve"] * kf_per_step, 2), "achieved": round(ach, 2), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5), "algorithmic_bytes_per_launch": int(bytes_per_launch), "avg_launch_us": round(1e3 * avg_ms, 3), "traffic": None}
        else:
            stage = [n for n in FE_STAGES if FE_KERNEL[n] == dom][0]
            amount, unit, bound, peak = work[stage]
            ms = per_step[dom]
            if amount is None:
                amount = 0
            if bound == "hbm":
                ach = amount / (ms * 1e-3) / 1e9
                roof = {"bound": "hbm", "kernel": dom, "launches_per_step": 1, "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(ach / HBM_PEAK_GBS, 5), "algorithmic_bytes_per_launch": int(amount), "avg_launch_us": round(1e3 * ms, 3), "traffic": None}
            else:
                ach = amount / (ms * 1e-3) / 1e12
                roof = {"bound": "valu", "kernel": dom, "launches_per_step": 2, "achieved": round(ach, 3), "peak": INT_PEAK_TOPS, "unit": "Tint32op/s",
                        "frac": round(ach / INT_PEAK_TOPS, 5), "algorithmic_ops_per_step": int(amount), "avg_ms_per_step": round(ms, 4), "traffic": None}
        # HBM traffic of the dominant kernel from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate runs
        # of this command, tools/refresh_profiles.sh -> profiles/<round>_pmc.json); profile-derived, not measured in this run
        try:
            pmc_files = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_pmc.json"))
            pmc = json.load(open(os.path.join(ROOT, "profiles", pmc_files[-1])))
            kn = roof["kernel"]
            if kn in pmc["kernels"] and pmc.get("frames_per_launch", 6) == F:
                e = pmc["kernels"][kn]
                roof["traffic"] = int(round(1024.0 * (e["FETCH_SIZE"]["mean_per_launch"] + e["WRITE_SIZE"]["mean_per_launch"])))
                hb = e.get("hbm_bytes_per_launch")
                if hb:          # the guide's gfx950 rule: FETCH_SIZE x 2 for reads of 16 B per lane (tools/pmc_wrap.py names the class per kernel)
                    roof["traffic_corrected"] = hb["corrected"]
                    roof["traffic_fetch_correction"] = hb["fetch_correction"]
                alg = roof.get("algorithmic_bytes_per_launch")
                if alg:
                    roof["traffic_over_algorithmic"] = round(roof.get("traffic_corrected", roof["traffic"]) / alg, 3)
                roof["traffic_source"] = "profiles/" + pmc_files[-1] + " (FETCH_SIZE + WRITE_SIZE per launch from separate --pmc passes; see DESIGN.md section 6)"
        except (OSError, KeyError, ValueError, IndexError):
            pass

        pcie_fps = frames_total / elapsed_pcie
        fe_extract_ms = float(fe_ms[T_PYR] + fe_ms[T_FAST] + fe_ms[T_DIST] + fe_ms[T_DESC])
        fe_extract_free_ms = float(fe_ms_free[T_PYR] + fe_ms_free[T_FAST] + fe_ms_free[T_DIST] + fe_ms_free[T_DESC])
        out = dict(head)
        out.update({
            "ba_ms_per_iter": round(sum(d["ms_per_solve"] for d in ba_prof.values()) / max(ba_iters_done, 1), 4) if ba_prof else None,      # event sum: every launch with the gap in front of it
            "ba_wall_ms_per_iter": round(profile_ba.wall_ms_per_iter, 4) if ba_prof else None,      # optimize(10) by graph replay, wall / 10
            "ba_setup_ms": round(ba_setup_ms, 4) if ba_setup_ms is not None else None,
            "ba_ms_per_keyframe": round(ba_total_ms, 4) if ba_total_ms is not None else None,
            "ba_ms_per_keyframe_pipelined": round(ba_pipe_ms, 4) if ba_pipe_ms is not None else None,
            "roofline": roof,
            # HIP-event time between consecutive launches of an event-instrumented solve / front-end pass (each entry includes the gap in
            # front of its kernel: the BA entries sum to more than the graph-replayed solve of the timed loop takes)
            "gpu_ms_per_step_by_kernel": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])},
            "gpu_ms_per_step_by_kernel_note": "event-instrumented passes outside the timed region, launch gaps included; not a decomposition of ms_per_step",
            "ba_kernel_us_per_iteration": {("k_chol_factor" if n == "chol" else n): round(1e3 * d["ms_per_solve"] / max(ba_iters_done, 1), 2) for n, d in ba_prof.items()} if ba_prof else None,
            # SURVEY.md 8(d) whole-extraction figure: B_img = pyramid + FAST + blur + patches + outputs per image, over the
            # summed time of the four extraction kernels (the blur's 2P bytes are part of B_img although it is fused away here)
            "front_end_roofline": {"algorithmic_bytes_per_step": int(wl.extract_bytes()), "extract_ms_per_step": round(fe_extract_free_ms, 4),
                                   "achieved": round(wl.extract_bytes() / (fe_extract_free_ms * 1e-3) / 1e9, 1), "unit": "GB/s",
                                   "frac": round(wl.extract_bytes() / (fe_extract_free_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                                   "extract_ms_per_step_under_mapping_reserve": round(fe_extract_ms, 4),
                                   "note": "the four extraction kernels on all 256 CUs; in the timed loop they run on 256 - 8 x mapping_reserve CUs beside the mapping solves",
                                   "valu_issue": front_end_valu_issue()},
            "value_upload_inclusive": round(pcie_fps, 2),          # the same K steps with every extracted frame copied over PCIe inside the loop (below)
            "pcie_inclusive_frames_per_s": round(pcie_fps, 2),
            "pcie_inclusive": {"frames_per_s": round(pcie_fps, 2), "ms_per_step": round(1e3 * elapsed_pcie / args.steps, 4), "ratio_to_value": round(pcie_fps / value, 4),
                               "host_bytes_per_step": 2 * F * W * H,
                               "note": "the same K timed steps with every extracted frame copied from page-locked host memory inside the loop "
                                       "(lpslam_hip_upload_images_async: copy stream, step s+1 copied beside the kernels of step s)"},
        })
        if flops:
            tot = sum(flops.values())
            it_ms = sum(d["ms_per_solve"] for d in ba_prof.values()) / max(ba_iters_done, 1)
            out["ba_roofline"] = {"flop_per_iteration": int(tot), "ms_per_iteration": round(it_ms, 4), "achieved_TFLOPs": round(tot / (it_ms * 1e-3) / 1e12, 4),
                                  "frac_of_fp64_peak": round(tot / (it_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, 5)}
        if wl.with_ba and elapsed_contig is not None:
            # the same workload with windows as a tracker makes them: contiguous tracks, block-banded reduced system (ba_band.inl)
            wl.set_tracks("contiguous")
            c_prof, c_setup, c_total, c_iters, c_dim, c_pipe, c_solver = profile_ba()
            c_flops = ba_flops(wl.probs[0], c_dim, c_solver[1] if c_solver[0] == "band" else -1)
            c_it_ms = sum(d["ms_per_solve"] for d in c_prof.values()) / max(c_iters, 1)
            c_tot = sum(c_flops.values())
            dchol = c_prof["chol"]
            chol_us = 1e3 * dchol["ms_per_solve"] / max(dchol["marks_per_solve"] * dchol["launches_per_mark"], 1)
            out["value_contiguous"] = round(frames_total / elapsed_contig, 2)
            out["contiguous"] = {
                "frames_per_s": round(frames_total / elapsed_contig, 2), "ms_per_step": round(1e3 * elapsed_contig / args.steps, 4),
                "observations": wl.n_obs, "solver": c_solver[0], "block_half_bandwidth": c_solver[1],
                "ba_ms_per_iter": round(c_it_ms, 4), "ba_wall_ms_per_iter": round(profile_ba.wall_ms_per_iter, 4), "ba_setup_ms": round(c_setup, 4), "ba_ms_per_keyframe": round(c_total, 4), "ba_ms_per_keyframe_pipelined": round(c_pipe, 4),
                "ba_kernel_us_per_iteration": {("k_chol_factor" if n == "chol" else n): round(1e3 * d["ms_per_solve"] / max(c_iters, 1), 2) for n, d in c_prof.items()},
                "ba_roofline": {"flop_per_iteration": int(c_tot), "achieved_TFLOPs": round(c_tot / (c_it_ms * 1e-3) / 1e12, 4), "frac_of_fp64_peak": round(c_tot / (c_it_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, 5)},
                "factor_roofline": {"bound": "mfma", "kernel": hip.ba_factor_kernel_name(c_dim, c_solver[0] == "band"), "avg_launch_us": round(chol_us, 3),
                                    "algorithmic_flops_per_launch": int(c_flops["cholesky"]), "achieved": round(c_flops["cholesky"] / (chol_us * 1e-6) / 1e12, 5), "peak": FP64_PEAK_TFLOPS,
                                    "unit": "TFLOP/s", "frac": round(c_flops["cholesky"] / (chol_us * 1e-6) / 1e12 / FP64_PEAK_TFLOPS, 6),
                                    "note": "band Cholesky + both substitutions of the %d x %d system, half-bandwidth %d: %d 16-column strips factored from both ends by two workgroups, "
                                            "a serial chain of %d strips (latency bound: 2.3 us per strip, 1.15 of it the pivot chain)"
                                            % (c_dim, c_dim, 6 * max(c_solver[1], 0) + 5, (c_dim + 15) // 16, (c_dim + 15) // 16 - (((c_dim + 15) // 16 - 5) // 2 if (c_dim + 15) // 16 >= 12 else 0))},
                "note": "windows with contiguous tracks (synth.ba_problem tracks='contiguous'): landmark-group Schur complement on the FP64 matrix cores + band Cholesky; "
                        "`value` above is the random-track workload of rounds 1-3"}
            wl.set_tracks("random")

    # ---- extras, outside the timed region; the scaling runs (N > 1) print the timed line only
    if rank == 0 and not args.no_extras and world == 1:
        extras = {}
        skip = set(filter(None, os.environ.get("LPSLAM_BENCH_SKIP", "").split(",")))      # development: extras to leave out
        n_fe = max(3, min(args.steps, 10))
        wl.ctx.sync()
        wl.ctx.set_mapping_reserve(0)                    # the front end alone / a GPU-filling batch of sessions: nothing to make room for
        t2 = time.perf_counter()
        for s in range(n_fe):
            wl.front_end(s)
        wl.ctx.sync()
        fe_batched = n_fe * F / (time.perf_counter() - t2)
        lat = []
        for _ in range(20):
            t2 = time.perf_counter()
            wl.ctx.extract(2)
            wl.ctx.match_stereo_strided(0, 1, 2, 1, wl.k["fxb"], wl.k["baseline"])
            wl.ctx.match_bf(0, 2)
            wl.ctx.sync()
            lat.append(1e3 * (time.perf_counter() - t2))
        extras["front_end"] = {"batched_frames_per_s": round(fe_batched, 1), "frames_per_launch": F,
                               "single_frame_latency_ms": round(float(np.median(lat)), 4)}
        # K0 on-device undistort / rectify: remaps of a staged raw frame, 8 B per pixel algorithmic
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        for eye in (0, 1):
            wl.ctx.set_rectify_map(eye, xx * 0.97 + 15 + 3 * np.sin(yy / 50), yy * 0.97 + 9 + 3 * np.cos(xx / 70))
        wl.ctx.upload_raw(0, 0, wl.host_frames[0][0])
        for i in range(2 * F):
            wl.ctx.remap_staged(i, i & 1)
        wl.ctx.sync(); t2 = time.perf_counter()
        for _ in range(10):
            for i in range(2 * F):
                wl.ctx.remap_staged(i, i & 1)
        wl.ctx.sync()
        t_rm = (time.perf_counter() - t2) / (10 * 2 * F)
        extras["remap"] = {"us_per_image": round(1e6 * t_rm, 2), "algorithmic_GBps": round(8.0 * W * H / t_rm / 1e9, 1)}
        for i in range(F):          # restore the resident frames
            l, r = wl.host_frames[i]
            wl.ctx.upload(2 * i, l); wl.ctx.upload(2 * i + 1, r)
        # ---- S independent sessions served by the one GPU (north star: "batched sequences"): every session's frames go through the
        # front end, the windows of all sessions are solved as ONE batch per keyframe round (lpslam_hip_ba_optimize_batch: one launch
        # chain, blockIdx.y = session), fresh problems every round (create inside the loop)
        if wl.with_ba and "multi_session" not in skip:
            try:
                S = 16
                rounds = int(os.environ.get("LPSLAM_BENCH_MS_ROUNDS", "4"))
                fe_ctx = wl.ctx                                  # the sessions' frames: the resident ring, KF_INTERVAL frames per session and round

                from concurrent.futures import ThreadPoolExecutor
                creators = ThreadPoolExecutor(8)                 # every session has a mapping thread of its own: the windows are set up side by side

                ahead = ThreadPoolExecutor(1)                    # sets the NEXT round's windows up beside the running batch (the single-session pipeline, 16 wide)

                def make_all(v0):
                    # the host half of every window on the sessions' own threads, the device half of all sixteen as one launch chain
                    bas = list(creators.map(lambda v: wl.new_problem(v, build=False), range(v0, v0 + S)))
                    hip.ba_build_batch(bas)
                    return bas

                def session_rounds(n_rounds):
                    """every round: the windows built beside the previous round's solve receive their values (set_state: what the solve
                    before them produced), are solved as one batch, read back and released"""
                    fut = ahead.submit(make_all, 0)
                    for r in range(n_rounds):
                        ta = time.perf_counter()
                        bas = fut.result()
                        tb = time.perf_counter()
                        if r + 1 < n_rounds:
                            fut = ahead.submit(make_all, (r + 1) * S)
                        ps = [wl.probs[(r * S + i) % BA_VARIANTS] for i in range(S)]
                        hip.ba_set_state_batch(bas, [p["poses"] for p in ps], [p["points"] for p in ps])
                        tc = time.perf_counter()
                        hip.ba_optimize_batch(bas, True, BA_ITERS)
                        td = time.perf_counter()
                        hip.ba_state_batch(bas)
                        for b in bas:
                            b.close()
                        if os.environ.get("LPSLAM_BENCH_ROUND_TRACE"):
                            print("round %d: waited for the windows %.3f ms, set_state %.3f, batch %.3f, state + close %.3f" % (r, 1e3 * (tb - ta), 1e3 * (tc - tb), 1e3 * (td - tc), 1e3 * (time.perf_counter() - td)), file=sys.stderr)

                def fe_round():
                    n_frames = S * KF_INTERVAL                  # 96 stereo frames per round, in launches of the ring's size
                    done = 0
                    while done < n_frames:
                        n = min(wl.R, n_frames - done)
                        fe_ctx.extract_range(0, 2 * n)
                        fe_ctx.match_stereo_strided(0, 1, 2, n, wl.k["fxb"], wl.k["baseline"])
                        fe_ctx.match_bf_strided(2, 0, 2, n - 1)
                        done += n
                    fe_ctx.sync()
                ms_reserve = int(os.environ.get("LPSLAM_BENCH_MS_RESERVE", "8"))       # the sessions' front ends leave 8 compute units of every XCD to the batch of windows (measured 0 / 8 / 16: 11.7-12.4 k / 12.5-12.9 k / 11.3-12.2 k frames/s, contiguous)
                wl.ctx.set_mapping_reserve(ms_reserve)
                for kind, key in (("random", "multi_session"), ("contiguous", "multi_session_contiguous")):
                    wl.set_tracks(kind)
                    session_rounds(2); fe_round()          # two rounds: the pipeline holds two sets of windows, their blocks come from the cache afterwards
                    t2 = time.perf_counter()
                    th = threading.Thread(target=lambda: session_rounds(rounds))
                    th.start()
                    for _ in range(rounds):
                        fe_round()
                    th.join()
                    t_ms = time.perf_counter() - t2
                    t3 = time.perf_counter()
                    session_rounds(rounds)
                    t_ba_only = (time.perf_counter() - t3) / rounds
                    fl = out["ba_roofline"]["flop_per_iteration"] if kind == "random" and "ba_roofline" in out else (out["contiguous"]["ba_roofline"]["flop_per_iteration"] if "contiguous" in out else None)
                    extras[key] = {"sessions_per_gpu": S, "tracks": kind, "frames_per_s": round(rounds * S * KF_INTERVAL / t_ms, 1),
                                   "batched_ba_ms_per_round": round(1e3 * t_ba_only, 3), "ba_windows_per_s": round(S / t_ba_only, 1),
                                   # the batch's arithmetic against the FP64 matrix-core peak: S windows x BA_ITERS iterations of the
                                   # per-iteration flop count above, over the whole round (create + solve + read-back + destroy)
                                   "ba_roofline": ({"TFLOPs": round(S * BA_ITERS * fl / t_ba_only / 1e12, 3), "frac_of_fp64_peak": round(S * BA_ITERS * fl / t_ba_only / 1e12 / FP64_PEAK_TFLOPS, 5)} if fl else None),
                                   "note": "16 sessions, 6 stereo frames + 1 fresh local BA each per round; the windows of a round are prepared on 8 host threads beside the previous round's solve (every session has its mapping thread; lpslam_hip_ba_prepare enqueues nothing) and built by ONE launch chain (lpslam_hip_ba_build_batch), receive their values (one lpslam_hip_ba_set_state_batch call), are solved by one lpslam_hip_ba_optimize_batch call, read back (one lpslam_hip_ba_get_batch call) and released; the front ends leave %d compute units per XCD to the batch" % ms_reserve}
                wl.set_tracks("random")
                wl.ctx.set_mapping_reserve(0)
                creators.shutdown(); ahead.shutdown()
            except Exception as e:      # noqa: BLE001
                extras["multi_session"] = {"error": str(e)}
        # the integrated path: the same sequence through the drop-in boundary (LpSlamManager -> stereo tracker: upload, extract,
        # stereo + projection matching, one-launch pose optimiser, keyframe every 6th frame with a windowed local BA).  One untimed
        # session of 30 frames first (the timed loop above never ran the tracker's kernels: code objects, page-locked staging and
        # the allocator's pools are cold for the first frames of a process), then 120 frames timed from the first enqueue to the last
        # result; `steady_frames_per_s` is the same run without its first 20 frames (a new session's own first-frame allocations).
        try:
            from lpslam_amd import manager, _build
            _build.host_library()
            seq_t = wl.synth.StereoSequence(W, H, 4)
            tr_frames = [seq_t.frame(i) for i in range(120)]

            def tracker_session(frames, extra_cfg=""):
                mg = manager.Manager()
                for num in (0, 1):
                    c = manager.default_camera()
                    c.camera_number = num; c.f_x = wl.k["fx"]; c.f_y = wl.k["fy"]; c.c_x = wl.k["cx"]; c.c_y = wl.k["cy"]
                    c.resolution_x = W; c.resolution_y = H; c.focal_x_baseline = wl.k["fxb"]
                    mg.set_camera(c)
                mg.add_tracker("VSLAMStereo", '{"cameraSetup": "stereo", "slamKeypoints": %d, "numLevels": %d, "keyframeInterval": %d, "device": %d%s}' % (KPTS, LEVELS, KF_INTERVAL, device, extra_cfg))
                arrivals = []
                mg.collect_results(on_result=lambda: arrivals.append(time.perf_counter()))
                mg.provide_odometry(native=True)           # the library's compiled identity-odometry callback: no interpreter (and no wait for its lock) on the worker thread
                log = os.path.join(tempfile.mkdtemp(prefix="lpslam_bench_"), "slam.log")
                mg.log_to_file(log)
                mg.start()
                t2 = time.perf_counter()
                for i, (l, r) in enumerate(frames):
                    mg.add_stereo((i + 1) * 40_000_000, l, r)
                while len(mg.results) < len(frames) and time.perf_counter() - t2 < 60:
                    time.sleep(0.0005)
                t_all = time.perf_counter() - t2
                st = mg.status()
                mg.stop()
                return mg, t_all, st, arrivals, manager.Manager.statistics(log)

            tracker_session(tr_frames[:30])
            runs = [tracker_session(tr_frames) for _ in range(3)]       # three sessions over the same 120 frames: the median one is reported
            runs.sort(key=lambda r: r[1])
            mg, t_tr, st_tr, arrivals, tstats = runs[1]
            steady = (len(arrivals) - 21) / (arrivals[-1] - arrivals[20]) if len(arrivals) > 40 else None
            extras["tracker"] = {"frames": len(mg.results), "valid": int(sum(r["valid"] for r in mg.results)), "frames_per_s": round(len(mg.results) / t_tr, 1),
                                 "frames_per_s_of_the_three_sessions": [round(len(r[0].results) / r[1], 1) for r in runs],
                                 "steady_frames_per_s": round(steady, 1) if steady else None,
                                 "last_frame_ms": round(1e3 * st_tr.frame_time, 3), "key_frames": int(st_tr.key_frames),
                                 "ms_per_frame_in_tracker": tstats.get("ms_per_frame"), "ms_pose_optimiser": tstats.get("ms_dev_pose"),
                                 "ms_matchers": tstats.get("ms_dev_match"), "ms_frame_read_back": tstats.get("ms_dev_get"),
                                 "warm_up": "one untimed 30-frame session in this process"}
            # the same session with a vocabulary, as the reference always runs (vocabFile; the committed 1000-word test vocabulary: BoW vector of
            # every keyframe, loop candidates from the BoW database, all candidates matched under the vocabulary's nodes in one call)
            vocab = os.path.join(ROOT, "tests", "golden", "vocab_k10_L3.dbow2")
            if os.path.exists(vocab):
                mgv, t_v, st_v, _, vstats = tracker_session(tr_frames, ', "vocabFile": "%s"' % vocab)
                extras["tracker"]["with_vocabulary"] = {"frames_per_s": round(len(mgv.results) / t_v, 1), "valid": int(sum(r["valid"] for r in mgv.results)), "key_frames": int(st_v.key_frames),
                                                        "ms_per_frame_in_tracker": vstats.get("ms_per_frame"), "ms_kf_insert": vstats.get("ms_kf_insert"), "ms_kf_loop": vstats.get("ms_kf_loop"),
                                                        "vocabulary": "tests/golden/vocab_k10_L3.dbow2 (k = 10, L = 3, 1000 words)"}
        except Exception as e:      # noqa: BLE001 -- an extra must not take the benchmark line down
            extras["tracker"] = {"error": str(e)}
        # N sessions through the drop-in API at once: N LpSlamManager instances in this process on this GPU -- what BASELINE configs[3]
        # runs per device when a node serves more sequences than it has GPUs, and the reference's deployment unit (one manager, one worker
        # thread, one frame in flight per sequence: /root/reference/src/Manager/SlamManager.cpp:54-61,191-201).  Every manager has its own
        # context, streams and worker; a feeder thread per manager enqueues its 120 frames; results are counted by the library's compiled
        # callback.  Aggregate = all results / wall time from the first enqueue to the last result.
        if "tracker_multi" not in skip and "tracker" not in skip:
            # A process that serves many sessions runs with every stream at the default priority from its first stream on
            # (lpslam_hip_set_flat_priorities); this process has created high-priority mapping streams for the numbers
            # above, and ONE such stream ever created halves the aggregate (3600 -> 2000 frames/s at 8 managers, tools/dev_tracker_multi.py
            # WITH_BA=1): the managers run in a child process of their own, as such a server would be.
            try:
                import subprocess
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "tracker_multi", "--device", str(device)], capture_output=True, text=True, timeout=600)
                line = [l for l in r.stdout.splitlines() if l.startswith("{")]
                extras["tracker_multi"] = json.loads(line[-1]) if r.returncode == 0 and line else {"error": "child process: rc %d, %s" % (r.returncode, r.stderr.strip()[-300:])}
            except Exception as e:      # noqa: BLE001
                extras["tracker_multi"] = {"error": str(e)}
        # the monocular tracker on the same boundary: two-view initialisation, then tracking with triangulated keyframes
        try:
            mg = manager.Manager()
            c = manager.default_camera()
            c.camera_number = 0; c.f_x = wl.k["fx"]; c.f_y = wl.k["fy"]; c.c_x = wl.k["cx"]; c.c_y = wl.k["cy"]; c.resolution_x = W; c.resolution_y = H
            mg.set_camera(c)
            mg.add_tracker("VSLAMMono", '{"cameraSetup": "monocular", "slamKeypoints": %d, "numLevels": 3, "keyframeInterval": %d, "device": %d}' % (KPTS, KF_INTERVAL, device))
            mg.collect_results(); mg.provide_odometry()
            mg.start()
            walls = wl.synth.WallSequence(W, H, 4, step=0.05)
            mono_frames = [walls.frame(i) for i in range(30)]
            t2 = time.perf_counter()
            for i, img in enumerate(mono_frames):
                mg.add_image((i + 1) * 40_000_000, img)
            while len(mg.results) < len(mono_frames) and time.perf_counter() - t2 < 60:
                time.sleep(0.0005)
            t_tr = time.perf_counter() - t2
            st_tr = mg.status()
            mg.stop()
            extras["tracker_mono"] = {"frames": len(mg.results), "valid": int(sum(r["valid"] for r in mg.results)),
                                      "frames_per_s": round(len(mg.results) / t_tr, 1), "key_frames": int(st_tr.key_frames), "landmarks": int(st_tr.feature_points)}
        except Exception as e:      # noqa: BLE001
            extras["tracker_mono"] = {"error": str(e)}
        # BASELINE configs[4]'s global BA on ONE GPU (all landmarks on this rank; the partitioned solve adds one all-reduce of
        # the reduced system per trial): 200 keyframes, 30 k landmarks, ~240 k observations, 10 LM iterations
        try:
            gprob = wl.synth.ba_problem(200, 30000, 240000, 1920, 1080, seq_id=2, kf_stride=2)
            gobs = wl.hip.ba_obs_array(gprob)
            t2 = time.perf_counter()
            gba = wl.hip.BundleAdjuster(wl.ctx, gprob["poses"], gprob["fixed"], gprob["points"], gobs, gprob["cam"])
            gba.state(); t_gsetup = time.perf_counter() - t2
            gba.optimize(True, 2); gba.reset()
            t2 = time.perf_counter(); glog2 = gba.optimize(True, BA_ITERS); t_g = time.perf_counter() - t2
            extras["global_ba"] = {"keyframes": 200, "landmarks": 30000, "observations": int(gba.n_obs), "ms_per_iter": round(1e3 * t_g / max(len(glog2), 1), 4),
                                   "setup_ms": round(1e3 * t_gsetup, 3), "chi2_first": float(glog2["chi2_before"][0]), "chi2_last": float(glog2["chi2_after"][-1])}
            gba.close()
        except Exception as e:      # noqa: BLE001
            extras["global_ba"] = {"error": str(e)}
        pg = wl.synth.pose_graph_problem(200, 0)
        graph = wl.hip.PoseGraph(wl.ctx, pg["verts"], pg["fixed"], wl.hip.sim3_edges(pg["edge_i"], pg["edge_j"], pg["meas"]), True)
        graph.optimize(2)
        t2 = time.perf_counter(); glog = graph.optimize(10); t_pg = time.perf_counter() - t2
        extras["pose_graph"] = {"keyframes": 200, "edges": int(len(pg["edge_i"])), "ms_per_iter": round(1e3 * t_pg / max(len(glog), 1), 4)}
        graph.close()
        out.update(extras)
        # the driver's record keeps the NAMES of the first 20 extra keys in alphabetical order: the figures the review follows most
        # closely once more under keys that sort first
        out["a_value_contiguous"] = out.get("value_contiguous")
        out["a_value_upload_inclusive"] = out.get("value_upload_inclusive")
        out["a_tracker"] = {k: extras.get("tracker", {}).get(k) for k in ("frames_per_s", "steady_frames_per_s", "ms_per_frame_in_tracker", "ms_pose_optimiser")}
        out["a_tracker_multi"] = {k: (v.get("aggregate_frames_per_s") if isinstance(v, dict) else None) for k, v in extras.get("tracker_multi", {}).items() if k.startswith("managers_")}
        out["a_multi_session"] = {k: extras.get(k, {}).get("frames_per_s") for k in ("multi_session", "multi_session_contiguous")}

    if rank == 0 and world == 1 and not args.no_cpu:
        best, legs = cpu_baseline()
        out["cpu_baseline"] = best
        out["cpu_baseline_legs"] = legs
        best["note"] = ("unoptimised scalar restatement of the OpenVSLAM / g2o algorithms (the oracle), not OpenVSLAM: front end ~%d ms per stereo frame on one thread, "
                        "several times what an OpenCV-SIMD ORB extractor needs; a reported baseline, not the target" % round(legs["1_thread_native"]["front_end_ms_per_frame"]))
        out["gpu_over_cpu"] = {"ratio": round(out["value"] / best["value"], 2), "cpu_leg": "%d threads, -O3 -march=native, oracle port" % best["cores"],
                               "ratio_vs_1_thread": round(out["value"] / legs["1_thread_native"]["value"], 1)}

    # ---- N > 1, outside the timed region: BASELINE configs[4], the landmark-partitioned global BA over all ranks with the C++ RCCL
    # driver (lpslam_hip_ba_optimize_partitioned: packed-triangle all-reduce on the problem's stream).  A watchdog prints the timed
    # line and leaves with a NON-ZERO status if the section does not finish (the measured headline is kept, the run is not green).
    if dist is not None and rank == 0 and backend != "nccl":
        # rehearsal (gloo): the partitioned global BA is not run, but what its all-reduce would move is known from the sizes alone
        n = 6 * 199
        out["global_ba_partitioned"] = {"ranks": world, "skipped": "rehearsal backend %s" % backend,
                                        "allreduce_bytes_per_trial": int(8 * (n * (n + 1) // 2 + 3 * 1216 + 8)),
                                        "allreduce_calls": "2 + 2 x trials (packed system; trial chi2 + scale; once: diagonal SUM and MAX)"}
    if dist is not None and not args.no_extras and backend == "nccl":
        done_flag = threading.Event()

        def watchdog():
            if not done_flag.wait(150.0):
                if rank == 0:
                    out["global_ba_partitioned"] = {"error": "timed out"}
                    print(json.dumps(out), flush=True)
                os._exit(3)         # every rank: a hung collective must not read as a green run
        threading.Thread(target=watchdog, daemon=True).start()
        try:
            from lpslam_amd.dist_ba import shard_problem
            uid = [hip.RcclComm.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            comm = hip.RcclComm(uid[0], world, rank)
            gprob = wl.synth.ba_problem(200, 30000, 240000, 1920, 1080, seq_id=2, kf_stride=2)
            shard = shard_problem(gprob, rank, world)
            gba = hip.BundleAdjuster(wl.ctx, shard["poses"], shard["fixed"], shard["points"], hip.ba_obs_array(shard), shard["cam"])
            gba.optimize_partitioned(comm, True, 2)
            gba.reset()
            barrier()
            t2 = time.perf_counter(); glog = gba.optimize_partitioned(comm, True, BA_ITERS); t_g = time.perf_counter() - t2
            t_g = float(sync_tensor([t_g], dist.ReduceOp.MAX).item())
            if rank == 0:
                n = 6 * 199
                out["global_ba_partitioned"] = {"ranks": world, "keyframes": 200, "landmarks": 30000, "observations": int(len(gprob["obs_pose"])),
                                                "iterations": int(len(glog)), "ms_per_iter": round(1e3 * t_g / max(len(glog), 1), 4),
                                                "allreduce_bytes_per_trial": int(8 * (n * (n + 1) // 2 + 3 * 1216 + 8)),
                                                "chi2_first": float(glog["chi2_before"][0]), "chi2_last": float(glog["chi2_after"][-1]),
                                                "driver": "lpslam_hip_ba_optimize_partitioned (C++, RCCL on the problem's stream)"}
            gba.close(); comm.close()
        except Exception as e:      # noqa: BLE001
            if rank == 0:
                out["global_ba_partitioned"] = {"error": str(e)[:300]}
        done_flag.set()

    if rank == 0:
        print(json.dumps(out), flush=True)
        # (stderr, one line, last: whatever keeps only the tail of the run's output keeps this)
        print("BENCH SUMMARY value=%s contiguous=%s upload_inclusive=%s ba_ms_per_iter=%s/%s tracker=%s tracker_multi=%s multi_session=%s roofline_frac=%s" % (
            out.get("value"), out.get("value_contiguous"), out.get("value_upload_inclusive"), out.get("ba_ms_per_iter"), (out.get("contiguous") or {}).get("ba_ms_per_iter"),
            (out.get("a_tracker") or {}).get("frames_per_s"), out.get("a_tracker_multi"), out.get("a_multi_session"), (out.get("roofline") or {}).get("frac")), file=sys.stderr, flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
