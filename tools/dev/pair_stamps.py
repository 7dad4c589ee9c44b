"""development: shader-clock stamps inside k_chol_pair (build with LPSLAM_HIP_EXTRA_FLAGS=-DLPSLAM_PAIR_STAMPS) for the diagonal
workgroup, the first row workgroup and the first Minv workgroup of each of the five launches of the benchmark's window (50 keyframes /
5000 landmarks / 40 000 observations, random tracks).  Cycles from kernel entry; the stamps of the last factorisation of the run.
Every stamped workgroup's entry and exit are also given on the diagonal workgroup's clock (cycles from ITS entry).  Measured on an
MI355X: the shader clocks of different compute units do not share an origin, whether the chain is pinned to one XCD
or spread, so these offsets show which workgroups sit on one clock (entries a few cycles apart), not which one ends the launch.
usage: pair_stamps.py [RESERVE]      CUs of every XCD of the mapping reserve (default 0: pinned chain; 1-8: spread over the XCDs)"""
import sys, os, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from lpslam_amd import hip, synth
SLOTS = 24
NAMES = {1: "blocks in LDS", 2: "after step 1", 3: "2a start", 4: "2a strip A done", 5: "2a wait over", 6: "2a written out",
         7: "2b start", 8: "2b strip A done", 9: "2b wait over", 10: "2b written out", 11: "after step 2", 12: "after step 3 (left)",
         13: "4 start", 14: "4 strip A done", 15: "4 wait over", 16: "4 written out", 17: "w2 announced", 18: "w3 announced",
         19: "w2 2c done", 20: "w3 2c done", 21: "step 2's stores issued", 23: "exit"}
ctx = hip.Context(1280, 720, 2000, 1.2, 8, max_images=2)
reserve = int(sys.argv[1]) if len(sys.argv) > 1 else 0
ctx.set_mapping_reserve(reserve)
print("mapping reserve %d CUs per XCD: the chain is %s" % (reserve, "spread over the XCDs" if 0 < reserve <= 8 else "pinned to one XCD"))
p = synth.ba_problem(50, 5000, 40000, 1280, 720, seq_id=0, tracks="random", top_up=True)
ba = hip.BundleAdjuster(ctx, p["poses"], p["fixed"], p["points"], hip.ba_obs_array(p), p["cam"])
for _ in range(3):
    ba.reset()
    ba.optimize(True, 10)
buf = np.zeros(8 * 3 * SLOTS, dtype=np.uint64)
rc = ctx.lib.lpslam_hip_debug_pair_stamps(buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size))
assert rc == 0, rc
st = buf.reshape(8, 3, SLOTS).astype(np.int64)
for m in range(5):
    for kind, kname in enumerate(("diagonal", "row", "Minv")):
        s = st[m, kind]
        if s[0] == 0:
            continue
        rel = {k: int(s[k] - s[0]) for k in NAMES if s[k] != 0 and s[k] >= s[0]}
        print("m=%d %-8s " % (m, kname) + " | ".join("%s %d" % (NAMES[k], rel[k]) for k in sorted(rel, key=lambda k: rel[k])))
        waits = ["%s %d" % (n, int(s[b] - s[a])) for n, a, b in (("2a", 4, 5), ("2b", 8, 9), ("4", 14, 15)) if s[a] and s[b]]
        print("             wait at the announcement, cycles: " + ", ".join(waits))
        if st[m, 0, 0] != 0:
            print("             on the diagonal workgroup's clock: entry %+d, exit %d" % (int(s[0] - st[m, 0, 0]), int(s[23] - st[m, 0, 0])))
ba.close(); ctx.close()
