"""development: the benchmark's window (50 keyframes / 5000 landmarks / 40 000 observations, random tracks) solved a few times with plain
optimize() calls, to be run under `rocprofv3 --kernel-trace` (graph replay is off under the profiler, so every launch is in the trace);
tools/dev/window_chain_summary.py turns the trace into per-launch figures of the panel chain"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lpslam_amd import hip, synth
ctx = hip.Context(1280, 720, 2000, 1.2, 8, max_images=2)
p = synth.ba_problem(50, 5000, 40000, 1280, 720, seq_id=0, tracks="random", top_up=True)
ba = hip.BundleAdjuster(ctx, p["poses"], p["fixed"], p["points"], hip.ba_obs_array(p), p["cam"])
for _ in range(6):
    ba.reset()
    log = ba.optimize(True, 10)
print("solver %s, %d iterations, trials %s, chi2 %.6f" % (ba.solver()[0], len(log), log["trials"].tolist(), log["chi2_after"][-1]))
ba.close(); ctx.close()
