#!/usr/bin/env python3
"""Times the whole-map place ranking, lpslam_hip_rank_stored, against the same ranking done with the calls that existed before it:
lpslam_hip_match_bf_stored in chunks of 48 sets (its pair list and page-locked block are sized for 48), votes counted on the host.
Stored sets of {100, 1000, 3000} x {1200, 2000} descriptors against a query slot of as many; each timing is a median of wall clocks
around calls that return only after their kernels completed (both wait on a completion flag), after a warm-up and a device sync.

Beside both: the pair-count floor, one Hamming distance per pair = 8 v_xor_b32 (32-bit encoding, 1.75 per CU and cycle) + 8
v_bcnt_u32_b32 (VOP3, 0.96) per 64 pairs = 12.9 CU-cycles, on 256 CUs at 2.3 GHz; and the static instruction mix of
k_rank_votes's unrolled step from the gfx950 assembly (same two classes, DPP forms counted as wide): the kernel's own issue ceiling.

usage: time_place_rank.py [--reps N] [--sizes 100,1000,3000] [--desc 1200,2000] [--out FILE]      (--mix-only: no GPU)"""
import argparse, json, os, re, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_E32, RATE_WIDE, CUS, GHZ = 1.75, 0.96, 256, 2.3
FLOOR_CYC_PER_64 = 8 / RATE_E32 + 8 / RATE_WIDE


def kernel_mix():
    """instructions of k_rank_votes per 64 pairs by class: (e32, wide, s_nop) over the unrolled 64-step body"""
    with tempfile.TemporaryDirectory() as td:
        s_path = os.path.join(td, "m.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                               "-o", s_path, os.path.join(ROOT, "lpslam_amd", "csrc", "match.hip")], stderr=subprocess.DEVNULL)
        text = open(s_path).read()
    i = text.index("k_rank_votes"); i = text.index(":", text.index("\n_Z", i - 200))
    body = text[i:text.index(".Lfunc_end", i)].split("\n")
    # the fully unrolled chunk: the longest run of lines between two loop labels
    blocks, cur = [], []
    for ln in body:
        if re.match(r"^\.LBB\d+_\d+:", ln):
            blocks.append(cur); cur = []
        else:
            cur.append(ln.strip())
    blocks.append(cur)
    blk = max(blocks, key=lambda b: sum(t.startswith("v_bcnt") for t in b))
    steps = sum(t.startswith("v_bcnt") for t in blk) / 8
    e32 = wide = nop = 0
    for t in blk:
        op = t.split()[0] if t else ""
        if op.startswith("v_") and op not in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32"):
            if op.endswith("_e32") and "f64" not in op and "dpp" not in t.split()[0]:
                e32 += 1
            else:
                wide += 1
        elif op == "s_nop":
            nop += 1
    return {"steps_in_block": steps, "e32_per_step": e32 / steps, "wide_per_step": wide / steps, "s_nop_per_step": nop / steps,
            "cu_cycles_per_64_pairs": (e32 / RATE_E32 + wide / RATE_WIDE) / steps, "floor_cu_cycles_per_64_pairs": FLOOR_CYC_PER_64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="100,1000,3000")
    ap.add_argument("--desc", default="1200,2000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mix-only", action="store_true")
    a = ap.parse_args()
    mix = kernel_mix()
    res = {"mix": mix, "rows": []}
    print("k_rank_votes static mix per 64 pairs: %.1f e32 + %.1f wide (+%.1f s_nop) -> %.1f CU-cycles; pair floor %.1f -> floor share %.2f"
          % (mix["e32_per_step"], mix["wide_per_step"], mix["s_nop_per_step"], mix["cu_cycles_per_64_pairs"], FLOOR_CYC_PER_64,
             FLOOR_CYC_PER_64 / mix["cu_cycles_per_64_pairs"]), flush=True)
    if not a.mix_only:
        from lpslam_amd import _build, hip
        _build.hip_library()
        ctx = hip.Context(1280, 720, 2100, 1.2, 8, max_images=2)
        rng = np.random.default_rng(1)
        print("%6s %5s %12s %12s %12s %9s %11s" % ("sets", "desc", "rank ms", "chunked ms", "floor ms", "speed-up", "floor share"), flush=True)
        for nd in [int(x) for x in a.desc.split(",")]:
            q = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
            ctx.set_descriptors(0, q)
            stored = 0
            for n_sets in sorted(int(x) for x in a.sizes.split(",")):
                for k in range(stored, n_sets):       # a growing map: 1/3 of each set is a noisy copy of query descriptors
                    d = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
                    m = nd // 3
                    d[:m] = q[rng.choice(nd, m, replace=False)] ^ (rng.random((m, 32)) < 0.03).astype(np.uint8)
                    ctx.desc_store_put(k, d)
                    ctx.desc_store_mask(k, (rng.random(nd) < 0.8).astype(np.uint8))
                stored = n_sets
                keys = np.arange(n_sets, dtype=np.int32)
                ctx.rank_stored(0, None, 50, 0.75, 8); ctx.sync()
                t_rank = []
                for _ in range(a.reps):
                    t0 = time.perf_counter(); ctx.rank_stored(0, None, 50, 0.75, 8); t_rank.append(time.perf_counter() - t0)
                t_chunk = []
                for _ in range(max(1, min(a.reps, 3))):
                    ctx.sync(); t0 = time.perf_counter()
                    votes = np.zeros(n_sets, np.int64)
                    for i in range(0, n_sets, 48):
                        for j, (mq, mt, md) in enumerate(ctx.match_bf_stored(0, keys[i:i + 48], 50, 0.75, True)):
                            votes[i + j] = len(mt)      # (the mask lookup of the real ranking left out: the host side is flattered)
                    order = np.lexsort((keys, -votes))[:8]
                    t_chunk.append(time.perf_counter() - t0)
                pairs = float(n_sets) * nd * nd
                floor_ms = pairs / 64 * FLOOR_CYC_PER_64 / (CUS * GHZ * 1e9) * 1e3
                r, c = float(np.median(t_rank)) * 1e3, float(np.median(t_chunk)) * 1e3
                row = {"sets": n_sets, "desc": nd, "rank_ms": r, "chunked_ms": c, "floor_ms": floor_ms, "speedup": c / r, "floor_share": floor_ms / r}
                res["rows"].append(row)
                print("%6d %5d %12.3f %12.3f %12.3f %9.1f %11.2f" % (n_sets, nd, r, c, floor_ms, c / r, floor_ms / r), flush=True)
            for k in range(stored):
                ctx.desc_store_drop(k)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
