#!/usr/bin/env python3
"""Generates tests/golden/g10_sim3_probes.npz: 45 Sim3 log / exp probes on both sides of every branch of g2o's Sim3::log
(tests/sim3_cases.py: theta in PROBE_THETA x sigma in PROBE_SIGMA, seeded axes and translations).

  u        45 x 7   the updates (theta axis, upsilon, sigma)
  theta    45       the theta class of each probe
  M        45 x 8   oracle.sim3_exp(u)
  chi2_mp  45       |log M|^2 by mpmath at 50 digits (sim3_cases.mp_sim3_log_chi2), rounded to double

The probes stop at theta = 3.14: beyond it the log is ill-conditioned (at pi - 1e-6 the oracle's own round trip is off by 1e-4
to 2e-3), which is no property of the kernel.  The GPU tests read the fixture and never import mpmath; tests/test_sim3_ref_cpu.py
regenerates it where mpmath is installed.
Usage: python tools/make_golden_sim3.py      (deterministic; needs mpmath)
"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O          # noqa: E402
import sim3_cases                       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g10_sim3_probes.npz")


def main():
    O.build()
    u, theta = sim3_cases.probe_updates()
    M = np.array([O.sim3_exp(x) for x in u])
    chi2_mp = np.array([sim3_cases.mp_sim3_log_chi2(m) for m in M])
    np.savez_compressed(OUT, u=u, theta=theta, M=M, chi2_mp=chi2_mp)
    print(os.path.basename(OUT), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
