#!/usr/bin/env python3
"""Open-ended fuzz of the window matchers (lpslam_hip_match_projection / _fuse / _area) against the oracle's (GPU box): random image
sizes, level counts, keypoint budgets, planted descriptor ties, query counts, windows, level bounds, thresholds, `taken` masks.  The
cases are tests/fuzz_cases.py's (a bounded slice runs inside `-m gpu`: tests/test_fuzz_gpu.py).  usage: fuzz_match.py [cases] [seed] [first_case]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O                                      # noqa: E402
import fuzz_cases                                                   # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
first = int(sys.argv[3]) if len(sys.argv) > 3 else 0
O.build()
bad = 0
t0 = time.time()
for case in range(first, first + cases):
    ok, tag = fuzz_cases.window_case(O, seed, case)
    if not ok:
        bad += 1; print("BAD  " + tag, flush=True)
    elif case % 20 == 0:
        print("ok   " + tag, flush=True)
log = [e for (s, c), e in fuzz_cases.WINDOW_LOG.items() if s == seed]
print("%d cases, %d bad, %d skipped, %d with matches, %d rescans, %.1f s" % (cases, bad, sum(e["skipped"] for e in log), sum(e["matches"] > 0 for e in log),
                                                                           sum(e["rescans"] for e in log), time.time() - t0))
sys.exit(1 if bad else 0)
