#!/usr/bin/env python3
"""The accuracy table of the dense window solve ("Accuracy of the dense window solve"; profiles/solve_accuracy.txt): every case
of tests/solve_cases.py and the reduced systems of real windows through lpslam_hip_ba_debug_solve, alone (panel-pair chain) and in a
batch of 40 (k_chol_wg), against the exact or refined solution and against a plain float64 Cholesky solve on the host.

    python tools/solve_accuracy.py [OUT]          # on the MI355X; prints the table, writes it to OUT when given
    python tools/solve_accuracy.py band [OUT]     # the banded window solve, k_chol_band (profiles/solve_accuracy_band.txt)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import solve_cases as sc          # noqa: E402
import solve_runner as sr         # noqa: E402
from lpslam_amd import hip        # noqa: E402


def write(lines, rows, name, out):
    worst = max(rows, key=lambda r: r["ratio"])
    m = 2
    while m < 2 * worst["ratio"]:
        m *= 2
    lines = lines + [sr.HEADER] + [sr.format_row(r) for r in rows]
    lines += ["# largest ratio %.2f (dim %d, %s, %s); largest e_dev / bound %.3g" % (worst["ratio"], worst["dim"], worst["family"], worst["kernel"], max(r["e_dev"] / r["bound"] for r in rows)),
              "# %s = smallest power of two >= 2 x largest ratio = %d" % (name, m)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)


def band(out):
    """every positive definite band case (full width, the narrow bands, the real band windows, the partners of the pivot cases)"""
    hip.load()
    ctx = hip.Context(320, 240, 400, 1.2, 4, max_images=1)
    holders = sr.BandHolders(hip, ctx)
    real = {6 * free: (free, hbw) for free, hbw in sr.REAL_BAND}
    cases = []
    for n in sc.BAND_DIMS:
        cases += sc.band_cases(n)
        if n in real:
            cases.append(sr.real_band_case(hip, ctx, *real[n]))
    for w, n in sc.BAND_NARROW:
        cases += sc.narrow_band_cases(n, w)
    cases += [sc.notpd_band(n, p)[0] for n, p, _ in sc.BAND_NOTPD_TOP] + [sc.notpd_band(n, q, True)[0] for n, q, _ in sc.BAND_NOTPD_BOTTOM]
    rows = []
    for c in cases:
        x, flag = holders.alone(c)
        assert flag == 0, (c["n"], c["family"])
        r = sr.row(c, x, "%s w=%d" % (sr.BAND, c["w"]))
        rows.append(r)
    holders.close(); ctx.close()
    write(["# forward error of the banded window solve (k_chol_band) on an MI355X: e = ||x - x*||_inf / ||x*||_inf, ratio = e_dev / max(e_host, 2^-53)",
           "# e_host: float64 Cholesky and two substitutions on the host; the bound every solver must meet is n kappa_2 2^-53; w: scalar half-bandwidth"],
          rows, "M_band", out)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "band":
        return band(sys.argv[2] if len(sys.argv) > 2 else None)
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
    write(["# forward error of the dense window solve on an MI355X: e = ||x - x*||_inf / ||x*||_inf, ratio = e_dev / max(e_host, 2^-53)",
           "# e_host: float64 Cholesky and two substitutions on the host; the bound every solver must meet is n kappa_2 2^-53"],
          rows, "M", sys.argv[1] if len(sys.argv) > 1 else None)


if __name__ == "__main__":
    main()
