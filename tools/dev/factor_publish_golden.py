"""development: the stored arrays of tests/test_ba_factor_publish_gpu.py -- x_p and the pivot flag of its systems, each solved through
lpslam_hip_ba_debug_solve on a fresh problem, as the library in use gives them on an MI355X.  They are meant to come from the PARENT
commit's library (build that commit elsewhere and name its liblpslam_hip.so in LPSLAM_HIP_LIB), so that the test compares this commit's
bytes with the parent's.
usage: factor_publish_golden.py [OUT.npz]      (default tests/golden/factor_publish/parent.npz)"""
import sys, os, importlib.util
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))            # solve_cases, solve_runner
import numpy as np
from lpslam_amd import hip
spec = importlib.util.spec_from_file_location("factor_publish_cases", os.path.join(ROOT, "tests", "test_ba_factor_publish_gpu.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)                                  # the dimensions and the systems: one copy, the test's
out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
os.makedirs(os.path.dirname(out), exist_ok=True)
hip.load()
print("library:", hip.LIB_PATH)
ctx = hip.Context(320, 240, 400, 1.2, 4, max_images=1)
keys = [(dim, f) for dim in T.DIMS for f in T.FAMILIES]
arrays = {}
for (dim, f), (x, flag) in zip(keys, T.solve_fresh(hip, ctx, [T.system(*k) for k in keys])):
    arrays["x_" + T.key(dim, f)] = x
    arrays["flag_" + T.key(dim, f)] = np.int32(flag)
    print("dim %3d  %-8s flag %d  |x|_inf %.17g" % (dim, f, flag, np.abs(x).max()))
np.savez(out, **arrays)
print("%s: %d bytes" % (out, os.path.getsize(out)))
ctx.close()
