#!/usr/bin/env python3
"""The accuracy table of the window build ("Accuracy of the window build"; profiles/build_accuracy.txt): every case of
tests/build_cases.py through the step API (the reduced buffer at lambda_0 and again behind one solve) and through one optimize()
iteration on the product paths, against the long-double reference of tests/ba_ref.py and against its float64 run.

    python tools/build_accuracy.py [OUT]          # on the MI355X; prints the table, writes it to OUT when given
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import build_cases as bc          # noqa: E402
import build_runner as br         # noqa: E402
from lpslam_amd import hip        # noqa: E402

PRODUCT = [(n, s) for n in bc.PRODUCT for s in (("auto", "dense") if bc.implied_solver(bc.problem(n))[0] == "band" else ("auto",))]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    hip.load()
    ctx = hip.Context(320, 240, 400, 1.2, 4, max_images=1)
    rows, notes = [], []
    for name in bc.STEP_API:
        for robust in ((True, False) if name == "huber_edges" else (True,)):
            r, f = br.step_api(hip, ctx, name, robust)
            rows += r
            notes.append("# %s%s: accepted %s (reference %s), lambda %.17g (reference %.17g), padding exact %s / %s" % (
                name, "" if robust else "/plain", f["accepted"], f["ref_accepted"], f["lam"], f["lam_ref"], f["padding_first"], f["padding_second"]))
    for name, solver in PRODUCT:
        r, f = br.product(hip, ctx, name, solver)
        rows += r
        notes.append("# %s on %s: trials %d, lambda %.17g (reference %.17g), fixed poses kept %s" % (name, f["solver"], f["trials"], f["lam"], f["lam_ref"], f["fixed_bytes"]))
    r, f = br.product(hip, ctx, "mono_mix", "auto", batch_build=True)
    rows += r
    each, launches = br.batch40(hip, ctx)
    worst = {}
    for r, f in each:                                     # 40 windows: the worst row of every quantity
        for x in r:
            if x["qty"] not in worst or x["ratio"] > worst[x["qty"]]["ratio"]:
                worst[x["qty"]] = x
    rows += list(worst.values())
    notes.append("# batch40: k_chol_wg launches %d, trials %s" % (launches, sorted(set(f["trials"] for _, f in each))))
    ctx.close()
    top = max(rows, key=lambda x: x["ratio"])
    m = 2
    while m < 2 * top["ratio"]:
        m *= 2
    lines = ["# accuracy of the window build on an MI355X: e = max |x - x*| / T over a quantity's entries (T: its companion of absolute values; ||step||_inf for a state),",
             "# ratio = e_dev / max(e_host, 2^-53) with e_host from the float64 run of the reference; e_dev/bar: the largest |x - x*| over the derived bar (t + c) kappa_l 2^-53 T, c = %d" % br.C,
             br.HEADER] + [br.format_row(x) for x in rows] + notes
    lines += ["# largest ratio %.2f (%s, %s, %s); largest e_dev / bar %.3g; every exact-zero entry exact: %s" % (
        top["ratio"], top["case"], top["stage"], top["qty"], max(x["worst"] for x in rows), all(x["exact"] for x in rows)),
        "# M = smallest power of two >= 2 x largest ratio = %d" % m]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
