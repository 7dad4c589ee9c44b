#!/usr/bin/env python3
"""The accuracy table of the dense window solve ("Accuracy of the dense window solve"; profiles/solve_accuracy.txt): every case
of tests/solve_cases.py and the reduced systems of real windows through lpslam_hip_ba_debug_solve, alone (panel-pair chain) and in a
batch of 40 (k_chol_wg), against the exact or refined solution and against a plain float64 Cholesky solve on the host.

    python tools/solve_accuracy.py [OUT]          # on the MI355X; prints the table, writes it to OUT when given
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import solve_cases as sc          # noqa: E402
import solve_runner as sr         # noqa: E402
from lpslam_amd import hip        # noqa: E402


def main():
    hip.load()
    ctx = hip.Context(320, 240, 400, 1.2, 4, max_images=1)
    holders = sr.Holders(hip, ctx)
    rows = []
    for n in sc.DIMS:
        cases = list(sc.synthetic_cases(n))
        if n in sc.WIDE_DIMS:
            cases += [sr.real_case(hip, ctx, kind, n // 6) for kind in sr.REAL_KINDS]
        for c in cases:
            x, flag = holders.alone(c)
            assert flag == 0, (n, c["family"])
            rows.append(sr.row(c, x, sr.CHAIN))
        if n <= sc.WG_MAX_DIM:
            xs, flags, launches = holders.wg_batch(cases)
            assert launches == 1 and not any(flags)
            rows += [sr.row(c, x, sr.WG) for c, x in zip(cases, xs)]
        holders.drop(n)
    holders.close(); ctx.close()
    worst = max(rows, key=lambda r: r["ratio"])
    m = 2
    while m < 2 * worst["ratio"]:
        m *= 2
    lines = ["# forward error of the dense window solve on an MI355X: e = ||x - x*||_inf / ||x*||_inf, ratio = e_dev / max(e_host, 2^-53)",
             "# e_host: float64 Cholesky and two substitutions on the host; the bound every solver must meet is n kappa_2 2^-53",
             sr.HEADER] + [sr.format_row(r) for r in rows]
    lines += ["# largest ratio %.2f (dim %d, %s, %s); largest e_dev / bound %.3g" % (worst["ratio"], worst["dim"], worst["family"], worst["kernel"], max(r["e_dev"] / r["bound"] for r in rows)),
              "# M = smallest power of two >= 2 x largest ratio = %d" % m]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
