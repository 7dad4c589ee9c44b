"""development: from a rocprofv3 kernel_trace.csv of tools/dev/window_chain_trace.py, the duration of k_chol_pair by its position m in the
factorisation (the launches of one factorisation follow each other; `per` of them, 5 for the benchmark's window) and of the unit's
other kernels; the first solve of the trace (code objects, cold caches) is left out"""
import csv, collections, re, statistics, sys
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
per = int(sys.argv[2]) if len(sys.argv) > 2 else 5
skip_units = int(sys.argv[3]) if len(sys.argv) > 3 else 10
by = collections.defaultdict(list)
n_pair = 0
for r in rows:
    m = re.search(r"(k_[a-z_0-9]+)", r["Kernel_Name"])
    if not m:
        continue
    name, d = m.group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if name == "k_chol_pair":
        unit, pos = divmod(n_pair, per)
        n_pair += 1
        if unit >= skip_units:
            by["k_chol_pair m=%d" % pos].append(d)
    elif n_pair >= skip_units * per:
        by[name].append(d)
print("%d k_chol_pair launches, %d units counted" % (n_pair, n_pair // per - skip_units))
for k in sorted(by):
    v = by[k]
    print("%-22s %5d launches: mean %7.2f median %7.2f min %7.2f max %7.2f us" % (k, len(v), statistics.mean(v), statistics.median(v), min(v), max(v)))
