"""development: k_ba_schur's workgroups on the benchmark's window, one launch taken apart (build with
LPSLAM_HIP_EXTRA_FLAGS=-DLPSLAM_SCHUR_STAMPS).  Per workgroup: the 32-term rounds it runs (from the pair lists, rebuilt here on the
CPU the way lpslam_hip_ba_prepare / k_bs_blkscan lay the launch out), start, first round in LDS, end of the loop, end -- grouped by
round count, then the workgroups that end last.
usage: schur_parts_stamps.py <repository root> <part> <max parts> [out file]     (part 0: ask the library, lpslam_hip_ba_get_schur_part)"""
import sys, os, ctypes as C
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
from lpslam_amd import hip, synth
part, maxp = int(sys.argv[2]), int(sys.argv[3])
out = open(sys.argv[4], "w") if len(sys.argv) > 4 else sys.stdout
SPLIT = 8
ctx = hip.Context(1280, 720, 2000, 1.2, 8, max_images=2)
prob = synth.ba_problem(50, 5000, 40000, 1280, 720, seq_id=0, tracks="random", top_up=True)
ba = hip.BundleAdjuster(ctx, prob["poses"], prob["fixed"], prob["points"], hip.ba_obs_array(prob), prob["cam"])
asked = part == 0
if asked:
    part, cap = ba.schur_part()
    maxp = 4 if part >= 256 else 8
    print("library: part %d, capacity %d" % (part, cap), file=out)
obs = hip.ba_obs_array(prob)
n_poses, n_points = len(prob["poses"]), len(prob["points"])
free = [i for i in range(n_poses) if not prob["fixed"][i]]
N = len(free)
A = np.zeros((n_poses, n_points), np.int64)
np.add.at(A, (obs["pose"], obs["point"]), 1)
Af = A[free]
cnt = Af @ Af.T                                              # terms of pair (i, k)
kf_obs = A.sum(axis=1)
def parts_of(n, part=part, maxp=maxp):
    return 1 if n <= part else min((n + part - 1) // part, maxp)
blocks = [(i, k) for i in range(N) for k in range(i, N)]
terms = [int(cnt[i, k]) for i, k in blocks]
table = [(b, q) for b, n in enumerate(terms) for q in range(1, parts_of(n))]
# what lpslam_hip_ba_prepare lays out: the stretch in front of the pairs and the XCD tiles
first_part = int(os.environ.get("EFIRST_PART", 128 if asked else part))      # (a library that chooses the part size lays the stretch out for the smallest)
efirst = min(sum(parts_of(int(kf_obs[p]), first_part, 4 if first_part >= 256 else 8) - 1 for p in free) + 32, 4095)
lead = n_poses * SPLIT
grp = lambda i: min(3, i * 4 // max(N, 1))
tile = [[6, 0, 1, 2], [0, 6, 3, 4], [1, 3, 7, 5], [2, 4, 5, 7]]
of_xcd = [[] for _ in range(8)]
for dpass in (True, False):
    for b, (i, k) in enumerate(blocks):
        if (i == k) == dpass:
            of_xcd[tile[grp(i)][grp(k)] if N >= 16 else b & 7].append(b)
at = [0] * 8
perm = []
for w in range(len(blocks)):
    x = (lead + efirst + w) & 7
    if at[x] >= len(of_xcd[x]):
        x = max(range(8), key=lambda y: (len(of_xcd[y]) - at[y], -y))
    perm.append(of_xcd[x][at[x]]); at[x] += 1
def rounds_of(b, q):
    chunks = (terms[b] + 31) // 32
    p = parts_of(terms[b])
    return len(range(q, chunks, p))
ba.reset(); ba.optimize(True, 3)
for rep in range(2):
    ba.reset(); ba.optimize(True, 3)
    buf = np.zeros(8 * 8192, dtype=np.uint64)
    ctx.lib.lpslam_hip_debug_schur_stamps(buf.ctypes.data_as(C.c_void_p), buf.size)
    st = buf.reshape(-1, 8).astype(np.int64)
    t0 = st[st[:, 0] > 0][:, 0].min()
    rows = []                                                # (workgroup, kind, rounds, start, first round, loop end, end)
    for w in range(lead, lead + efirst + len(blocks) + max(len(table) - efirst, 0)):
        bx = w - lead
        if efirst <= bx < efirst + len(blocks):
            b, q, kind = perm[bx - efirst], 0, "part 0"
        else:
            e = bx if bx < efirst else bx - len(blocks)
            if e >= len(table): continue
            (b, q), kind = table[e], "further"
        i, k = blocks[b]
        kind += " diag" if i == k else ""
        s = st[w]
        if s[1] < s[0] or s[0] < t0: continue               # (a stale record of an earlier launch)
        rows.append((w, kind, rounds_of(b, q), (s[0] - t0) * 0.01, (s[5] - t0) * 0.01, (s[6] - t0) * 0.01, (s[1] - t0) * 0.01))
    ld = st[:lead]; ld = ld[(ld[:, 1] >= ld[:, 0]) & (ld[:, 0] >= t0)]
    end_all = max(r[6] for r in rows)
    print("launch %d: part %d (at most %d), %d pair workgroups + %d leading, first stretch %d; launch ends %.2f us after its first workgroup starts"
          % (rep, part, maxp, len(rows), lead, efirst, end_all), file=out)
    if len(ld):
        print("  leading (pose side): start %.2f .. %.2f, end %.2f .. %.2f" % ((ld[:, 0].min() - t0) * 0.01, (ld[:, 0].max() - t0) * 0.01, (ld[:, 1].min() - t0) * 0.01, (ld[:, 1].max() - t0) * 0.01), file=out)
    print("  rounds  workgroups  start min/mean/max      first round in LDS (after start) mean   per round mean   end mean / max", file=out)
    for r in sorted(set(x[2] for x in rows)):
        a = np.array([x[3:] for x in rows if x[2] == r])
        per = ((a[:, 2] - a[:, 1]) / max(r, 1)).mean()
        print("  %6d  %10d  %5.2f / %5.2f / %5.2f   %5.2f                                   %5.2f            %5.2f / %5.2f"
              % (r, len(a), a[:, 0].min(), a[:, 0].mean(), a[:, 0].max(), (a[:, 1] - a[:, 0]).mean(), per, a[:, 3].mean(), a[:, 3].max()), file=out)
    print("  the 12 workgroups that end last:", file=out)
    for x in sorted(rows, key=lambda x: -x[6])[:12]:
        print("    workgroup %5d  %-14s rounds %d  start %5.2f  first round %5.2f  loop end %5.2f  end %5.2f" % x, file=out)
    late = [x for x in rows if x[3] > 3.0]
    print("  workgroups that start later than 3 us: %d (latest %.2f us)" % (len(late), max([x[3] for x in rows])), file=out)
ba.close(); ctx.close()
