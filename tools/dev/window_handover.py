"""development: the hand-over between two windows of the pipelined mapping loop, driven as bench.py's bundle_adjust_pipelined drives it
(50 keyframes / 5000 landmarks / 40 000 observations, random tracks): host clocks at entry and exit of optimize_end, set_state and
optimize_begin, wall time per keyframe, and the calling thread's CPU time per keyframe (what a polled wait costs)"""
import sys, os, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lpslam_amd import hip, synth
ctx = hip.Context(1280, 720, 2000, 1.2, 8, max_images=2)
probs = [synth.ba_problem(50, 5000, 40000, 1280, 720, seq_id=s, tracks="random", top_up=True) for s in range(4)]
obs = [hip.ba_obs_array(p) for p in probs]
def new(v):
    p = probs[v % 4]
    return hip.BundleAdjuster(ctx, p["poses"], p["fixed"], p["points"], obs[v % 4], p["cam"])
def start(ba, v, T=None):
    p = probs[v % 4]
    t0 = time.perf_counter(); ba.set_state(p["poses"], p["points"]); t1 = time.perf_counter(); ba.optimize_begin(True, 10); t2 = time.perf_counter()
    if T is not None:
        T["set_state"].append(t1 - t0); T["begin"].append(t2 - t1)
def run(n_kf, T):
    cur = new(0); start(cur, 0)
    t_all, c_all = time.perf_counter(), time.thread_time()
    for i in range(n_kf):
        t = time.perf_counter(); nxt = new(i + 1) if i + 1 < n_kf else None; T["new"].append(time.perf_counter() - t)
        t = time.perf_counter(); cur.optimize_end(); T["end"].append(time.perf_counter() - t)
        if nxt is not None:
            start(nxt, i + 1, T)
        t = time.perf_counter(); cur.state(); T["state"].append(time.perf_counter() - t)
        t = time.perf_counter(); cur.close(); T["close"].append(time.perf_counter() - t)
        cur = nxt
    return (time.perf_counter() - t_all) / n_kf, (time.thread_time() - c_all) / n_kf
keys = ("new", "end", "set_state", "begin", "state", "close")
run(20, {k: [] for k in keys})                      # graphs captured, page-locked blocks and code objects in place
for rep in range(3):
    T = {k: [] for k in keys}
    wall, cpu = run(60, T)
    print("per keyframe %.1f us wall, %.1f us CPU of the calling thread | median us: " % (1e6 * wall, 1e6 * cpu) + ", ".join("%s %.1f" % (k, 1e6 * statistics.median(T[k])) for k in keys)
          + " | mean us: " + ", ".join("%s %.1f" % (k, 1e6 * statistics.mean(T[k])) for k in keys))
print("graph replays %d" % ctx.ba_graph_replays())
ctx.close()
