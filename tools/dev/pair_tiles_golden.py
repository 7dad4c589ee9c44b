"""development: the stored arrays of tests/test_ba_pair_tiles_gpu.py -- poses and points of its nine windows after three LM iterations
of the dense solver, as the library in use gives them on an MI355X.  They are meant to come from the PARENT commit's library (build
that commit elsewhere and name its liblpslam_hip.so in LPSLAM_HIP_LIB), so that the test compares this commit's bytes with the parent's.
usage: pair_tiles_golden.py [OUT_DIR]      (default tests/golden/pair_tiles)"""
import sys, os, importlib.util
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from lpslam_amd import hip
spec = importlib.util.spec_from_file_location("pair_tiles_cases", os.path.join(ROOT, "tests", "test_ba_pair_tiles_gpu.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)                                  # the windows and the solver setting: one copy, the test's
out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN_DIR
os.makedirs(out, exist_ok=True)
hip.load()
print("library:", hip.LIB_PATH)
ctx = hip.Context(320, 240, 400, 1.2, 4, max_images=1)
for free, nb, need in T.CASES:
    ba = T.make(hip, ctx, T.window(free))
    log = ba.optimize(True, T.ITERS)
    poses, points = ba.state()
    np.save(os.path.join(out, "poses_%d.npy" % free), poses)
    np.save(os.path.join(out, "points_%d.npy" % free), points)
    print("free %2d  nb %d  last column %2d  solver %s  trials %s  chi2 %.9f" % (free, nb, need, ba.solver()[0], log["trials"].tolist(), log["chi2_after"][-1]))
    ba.close()
ctx.close()
