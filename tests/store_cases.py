"""Planted cases and references for the descriptor store, lpslam_hip_match_bf_stored (k_bf_knn2_pairs, k_runs_to_host) and
lpslam_hip_rank_stored (k_rank_votes, k_rank_topk): tests/test_store_ref_cpu.py and tests/test_store_planted_gpu.py iterate over
the same lists.  No GPU import here.

Distances are exact: flip(desc, k, rng) inverts exactly k distinct bits, base queries are uniform random 32-byte descriptors whose
mutual nearest-neighbour distance is far above the planted ones (2000 of them: at least 87), so planted distances of 60 or less
decide every match of a case.

Two references.  reference_matches / reference_votes / reference_rank are the oracle's C code (oracle.match_bf) and plain
counting / sorting; numpy_knn2 / numpy_matches restate the forward / reverse 2-NN and the filter in numpy (xor + popcount table,
first minimum, float32 ratio test, initial best and second distance 257) for the CPU test alone.

A Case carries its query descriptors, its stored sets and masks, the calls to make (`combos` for match_bf_stored, `ranks` for
rank_stored) and `props`, the planted properties as tuples the CPU test asserts on the reference itself:
  ("knn", key, query, best_idx, best_dist, second_dist)       forward 2-NN of `query` in set `key`
  ("rev", key, train, query)                                  reverse best (first minimum) of train descriptor `train`
  ("match", key, max_dist, ratio, cross, query, train)        `query` is matched to `train`; train -1: it has no match
  ("count", key, max_dist, ratio, cross, n)                   number of matches ("count_min": at least n)
  ("votes", key, max_dist, ratio, n)                          cross-checked, mask-passing matches
  ("votes_min", key, max_dist, ratio, n)                      at least n of them
  ("vote_in", key, max_dist, ratio, lo, hi)                   at least one of them has its train index in [lo, hi)
  ("f32", ratio, second, best, rejected)                      float32: ratio * second < best
"""
import functools

import numpy as np

from oracle import oracle as O

MAX_DIST, RATIO = 50, 0.75
SLOTS = 2124                      # descriptor slots of the tests' context (1280 x 720, 2100 keypoints, 8 levels)
BF_TILE, RK_PASS = 1024, 256      # LDS tile of both kernels; queries per pass of k_rank_votes


def flip(desc, k, rng):
    """`desc` with exactly k distinct bits inverted: Hamming distance k"""
    bits = rng.choice(256, int(k), replace=False)
    out = np.array(desc, np.uint8, copy=True)
    np.bitwise_xor.at(out, bits >> 3, (1 << (bits & 7)).astype(np.uint8))
    return out


def rand_desc(rng, n):
    return rng.integers(0, 256, (int(n), 32), dtype=np.uint8)


# ---- reference 1: the oracle ---------------------------------------------------------------------------------------------------
def reference_matches(q, t, max_dist, ratio, cross):
    return O.match_bf(q, t, max_dist, ratio, cross)


def reference_votes(q, sets, masks, max_dist, ratio):
    votes = {}
    for key, t in sets.items():
        mt = O.match_bf(q, t, max_dist, ratio, True)[1]
        m = masks.get(key)
        votes[key] = len(mt) if m is None else int(np.count_nonzero(m[mt]))
    return votes


def reference_rank(votes_by_key, top_k):
    order = sorted((k for k, v in votes_by_key.items() if v >= 1), key=lambda k: (-votes_by_key[k], k))[:top_k]
    return np.array(order, np.int32), np.array([votes_by_key[k] for k in order], np.int32)


# ---- reference 2: numpy ----------------------------------------------------------------------------------------------------------
_POP16 = np.array([bin(i).count("1") for i in range(256)], np.uint8)
_POP16 = (_POP16[:, None] + _POP16[None, :]).reshape(-1)          # popcount of a 16-bit word


def numpy_knn2(q, t, rows=128):
    """forward (best index, best distance, second distance) of every q in t and the reverse best index of every t in q, from one
    distance matrix: argmin takes the first minimum; nothing found: index -1, distances 257"""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    bi = np.full(nq, -1, np.int32); bd = np.full(nq, 257, np.int32); sd = np.full(nq, 257, np.int32)
    rbi = np.full(nt, -1, np.int32); rbd = np.full(nt, 257, np.int32)
    if nq == 0 or nt == 0:
        return bi, bd, sd, rbi
    qw, tw = q.view(np.uint16), t.view(np.uint16)
    for i0 in range(0, nq, rows):
        i1 = min(i0 + rows, nq)
        d = np.zeros((i1 - i0, nt), np.int32)
        for w in range(16):
            d += _POP16[qw[i0:i1, w, None] ^ tw[None, :, w]]
        r = np.arange(i1 - i0)
        bi[i0:i1] = d.argmin(1); bd[i0:i1] = d[r, bi[i0:i1]]
        col = d.argmin(0); cd = d[col, np.arange(nt)]             # reverse: this chunk's first minimum, kept if strictly smaller
        better = cd < rbd
        rbi[better] = col[better] + i0; rbd[better] = cd[better]
        d[r, bi[i0:i1]] = 257
        sd[i0:i1] = d.min(1)
    return bi, bd, sd, rbi


def numpy_matches(q, t, max_dist, ratio, cross, knn=None):
    bi, bd, sd, rbi = knn if knn is not None else numpy_knn2(q, t)
    keep = bi >= 0
    keep &= ~(bd > max_dist)
    if np.float32(ratio) > 0:
        keep &= ~(np.float32(ratio) * sd.astype(np.float32) < bd.astype(np.float32))
    if cross and len(rbi):
        keep &= rbi[np.maximum(bi, 0)] == np.arange(len(bi))
    i = np.flatnonzero(keep).astype(np.int32)
    return i, bi[i], bd[i]


# ---- cases -----------------------------------------------------------------------------------------------------------------------
BOTH = ((MAX_DIST, 0.0, False), (MAX_DIST, RATIO, True))


class Case:
    def __init__(self, name, q, sets, masks=None, combos=BOTH, ranks=((MAX_DIST, 0.0, 8), (MAX_DIST, RATIO, 8)), props=()):
        self.name, self.q, self.sets, self.masks = name, q, sets, masks or {}
        self.combos, self.ranks, self.props = tuple(combos), tuple(ranks), list(props)

    def __repr__(self):
        return self.name


def _rng(name, *more):
    return np.random.default_rng([sum(ord(c) * (i + 1) for i, c in enumerate(name))] + [int(m) for m in more])


def flipped_subset(rng, q, nt, frac=0.6, max_flip=40):
    """nt train descriptors: bit-flipped copies of a random subset of q (exact distances 0..max_flip) plus random fillers, shuffled"""
    k = min(int(round(min(nt, len(q)) * frac)) if nt > 1 else 1, nt, len(q))
    src = rng.choice(len(q), k, replace=False)
    base = [flip(q[i], rng.integers(0, max_flip + 1), rng) for i in src]
    d = np.concatenate([np.array(base, np.uint8).reshape(-1, 32), rand_desc(rng, nt - k)])
    return d[rng.permutation(nt)]


# a. structural sizes: query count -> train sizes of the sets stored for ONE call (nt_max differs from most sets' nt; 0 = empty set;
#    3000 is larger than the context's slot count)
SIZE_GROUPS = ((1, (1, 63, 1025)), (16, (64, 0, 2048)), (17, (65, 257, 3000)), (255, (255, 1023)), (256, (256, 1024, 0)),
               (257, (257, 2049)), (2124, (3000, 1, 1025, 0, 2048, 64)))


@functools.lru_cache(None)
def size_cases():
    cases = []
    for nq, sizes in SIZE_GROUPS:
        rng = _rng("sizes", nq)
        q = rand_desc(rng, nq)
        sets = {int(key): flipped_subset(rng, q, nt) for key, nt in zip(rng.choice(np.arange(-999, 9999), len(sizes), replace=False), sizes)}
        big = max(sets, key=lambda k: len(sets[k]))
        props = [("count_min", big, MAX_DIST, 0.0, False, (min(nq, len(sets[big])) + 2) // 3)]
        cases.append(Case("sizes_nq%d" % nq, q, sets, combos=BOTH, ranks=(), props=props))
    return cases


# b. more than 48 keys in one call (the device block and the page-locked block are pre-sized for 48 sets)
@functools.lru_cache(None)
def many_keys_case():
    rng = _rng("many")
    q = rand_desc(rng, 300)
    keys = rng.choice(np.arange(-5000, 100000), 120, replace=False)
    sets = {int(k): flipped_subset(rng, q, int(rng.integers(5, 301))) for k in keys}
    return Case("many_keys_120", q, sets, combos=BOTH, ranks=((MAX_DIST, RATIO, 256),),
                props=[("count_min", int(k), MAX_DIST, 0.0, False, 1) for k in keys[:5]])


# c. forward ties: identical train descriptors at the merges of bf_knn2_body -- the 64-descriptor sub-range, the 256-descriptor
#    wavefront share and the 1024-descriptor tile --; query 0 equals them, query 1 is one bit off, query 2 four bits off a second tie
FORWARD_TIES = (("sub_range", 130, (63, 64)), ("wavefront", 300, (255, 256)), ("tile", 1100, (1023, 1024)),
                ("across_tile", 1100, (5, 1030)), ("first_last", 2049, (0, 2048)), ("three_tiles", 2100, (1023, 1024, 2048)))


@functools.lru_cache(None)
def forward_tie_cases():
    cases = []
    for name, nt, tied in FORWARD_TIES:
        rng = _rng("fwd" + name)
        q = rand_desc(rng, 8); t = rand_desc(rng, nt)
        t[list(tied)] = q[0]
        q[1] = flip(q[0], 1, rng)
        first = tied[0]
        only_first = np.ones(nt, np.uint8); only_first[first] = 0            # the winner masked out: no vote
        not_rest = np.ones(nt, np.uint8); not_rest[list(tied[1:])] = 0       # the losers masked out: the vote stays
        # the second distance of a tied query is the tie's distance.  Query 1 (best 1, second 1) fails the ratio test for that reason
        # alone when the cross check is off; set 8 holds the same tie of a descriptor no query equals, query 2 is 4 bits off it and owns
        # it: best 4, second 4 -- its vote exists at ratio 0 and must not exist at ratio 0.75
        near = rand_desc(rng, 1)[0]
        t2 = rand_desc(rng, nt); t2[list(tied)] = near
        q[2] = flip(near, 4, rng)
        sets, masks = {7: t, -2: t, 30: t, 8: t2}, {-2: only_first, 30: not_rest}
        props = [("knn", 7, 0, first, 0, 0), ("knn", 7, 1, first, 1, 1), ("knn", 8, 2, first, 4, 4),
                 ("f32", RATIO, 1, 1, True), ("f32", RATIO, 4, 4, True),
                 ("match", 7, MAX_DIST, 0.0, False, 0, first), ("match", 7, MAX_DIST, 0.0, False, 1, first),
                 ("match", 7, MAX_DIST, RATIO, False, 0, first), ("match", 7, MAX_DIST, RATIO, False, 1, -1),
                 ("match", 7, MAX_DIST, RATIO, True, 0, first), ("match", 7, MAX_DIST, RATIO, True, 1, -1),
                 ("match", 7, MAX_DIST, 0.0, True, 1, -1),                   # one bit off: the train descriptor belongs to query 0
                 ("match", 8, MAX_DIST, 0.0, True, 2, first), ("match", 8, MAX_DIST, RATIO, False, 2, -1), ("match", 8, MAX_DIST, RATIO, True, 2, -1),
                 ("votes", 7, MAX_DIST, 0.0, 1), ("votes", -2, MAX_DIST, 0.0, 0), ("votes", 30, MAX_DIST, 0.0, 1), ("votes", 8, MAX_DIST, 0.0, 1),
                 ("votes", 7, MAX_DIST, RATIO, 1), ("votes", -2, MAX_DIST, RATIO, 0), ("votes", 30, MAX_DIST, RATIO, 1), ("votes", 8, MAX_DIST, RATIO, 0)]
        cases.append(Case("fwd_tie_" + name, q, sets, masks, combos=BOTH + ((MAX_DIST, 0.0, True), (MAX_DIST, RATIO, False)), props=props))
    return cases


# d. reverse ties: the train descriptor at index `at` of a set of nt has the listed (query, distance) neighbours among 320 queries;
#    the owner is the smallest distance, then the smallest query index: neighbouring lanes, two wavefronts, two passes of
#    k_rank_votes (256 queries per pass), the pass edge itself
REVERSE_TIES = (("lanes", ((3, 7), (4, 7)), 100, 40), ("wavefronts", ((3, 7), (67, 7)), 1100, 1050), ("passes", ((3, 7), (300, 7)), 100, 99),
                ("pass_edge", ((255, 7), (256, 7)), 65, 64), ("four", ((3, 7), (4, 7), (67, 7), (300, 7)), 2049, 2048),
                ("closer_later", ((3, 7), (300, 6)), 100, 0))


@functools.lru_cache(None)
def reverse_tie_cases():
    cases = []
    for name, near, nt, at in REVERSE_TIES:
        rng = _rng("rev" + name)
        q = rand_desc(rng, 320); t = rand_desc(rng, nt)
        for qi, d in near:
            q[qi] = flip(t[at], d, rng)
        owner = min(near, key=lambda qd: (qd[1], qd[0]))[0]
        props = [("rev", 11, at, owner), ("votes", 11, MAX_DIST, 0.0, 1), ("votes", 11, MAX_DIST, RATIO, 1)]
        for qi, d in near:
            props += [("knn", 11, qi, at, d, None), ("match", 11, MAX_DIST, 0.0, False, qi, at),
                      ("match", 11, MAX_DIST, RATIO, True, qi, at if qi == owner else -1)]
        cases.append(Case("rev_tie_" + name, q, {11: t}, props=props))
    return cases


# e. thresholds exactly on their edge, and the case one step past it
@functools.lru_cache(None)
def threshold_cases():
    cases = []
    rng = _rng("max_dist_edge")
    q = rand_desc(rng, 8)
    t = np.concatenate([[flip(q[0], 50, rng)], [flip(q[1], 51, rng)], rand_desc(rng, 10)])
    cases.append(Case("max_dist_edge", q, {4: t}, combos=((50, 0.0, False), (50, 0.0, True), (51, 0.0, True)), ranks=((50, 0.0, 8), (51, 0.0, 8)),
                      props=[("knn", 4, 0, 0, 50, None), ("knn", 4, 1, 1, 51, None), ("match", 4, 50, 0.0, False, 0, 0), ("match", 4, 50, 0.0, False, 1, -1),
                             ("match", 4, 51, 0.0, True, 1, 1), ("votes", 4, 50, 0.0, 1), ("votes", 4, 51, 0.0, 2)]))

    rng = _rng("ratio_edge")
    q = rand_desc(rng, 8)
    t = np.concatenate([[flip(q[0], 30, rng)], [flip(q[0], 40, rng)], [flip(q[1], 30, rng)], [flip(q[1], 39, rng)], rand_desc(rng, 10)])
    cases.append(Case("ratio_edge", q, {4: t}, combos=((50, 0.75, False), (50, 0.75, True), (50, 0.0, True)), ranks=((50, 0.75, 8), (50, 0.0, 8)),
                      props=[("knn", 4, 0, 0, 30, 40), ("knn", 4, 1, 2, 30, 39), ("f32", 0.75, 40, 30, False), ("f32", 0.75, 39, 30, True),
                             ("match", 4, 50, 0.75, False, 0, 0), ("match", 4, 50, 0.75, False, 1, -1), ("match", 4, 50, 0.75, True, 0, 0),
                             ("match", 4, 50, 0.0, True, 1, 2), ("votes", 4, 50, 0.75, 1), ("votes", 4, 50, 0.0, 2)]))

    # one descriptor: the second distance stays 257 (0.9f * 257 = 231.3 keeps best 231 and rejects 232; a sentinel of 256 would reject 231)
    rng = _rng("single_descriptor")
    q = rand_desc(rng, 8); t = rand_desc(rng, 1)
    q[0] = flip(t[0], 10, rng); q[2] = flip(t[0], 231, rng); q[3] = flip(t[0], 232, rng); q[4] = flip(t[0], 256, rng)
    cases.append(Case("single_descriptor", q, {4: t}, combos=((50, 0.75, False), (50, 0.75, True), (256, 0.9, False), (256, 0.0, False), (256, 0.75, True)),
                      ranks=((50, 0.75, 8), (256, 0.0, 8), (256, 0.9, 1)),
                      props=[("knn", 4, 0, 0, 10, 257), ("knn", 4, 2, 0, 231, 257), ("knn", 4, 3, 0, 232, 257), ("knn", 4, 4, 0, 256, 257),
                             ("f32", 0.9, 257, 231, False), ("f32", 0.9, 257, 232, True), ("f32", 0.9, 256, 231, True),
                             ("match", 4, 50, 0.75, False, 0, 0), ("match", 4, 256, 0.9, False, 2, 0), ("match", 4, 256, 0.9, False, 3, -1),
                             ("match", 4, 256, 0.0, False, 4, 0), ("count", 4, 256, 0.0, False, 8), ("rev", 4, 0, 0),
                             ("votes", 4, 50, 0.75, 1), ("votes", 4, 256, 0.0, 1)]))

    # max_dist 256 with ratio 0: nothing is filtered, every query has a match; cross-checked, every train descriptor owns one query at most
    rng = _rng("max_dist_256")
    q = rand_desc(rng, 40); t = rand_desc(rng, 70)
    t[69] = ~q[5]                                                    # distance 256 is still a distance: query 5 against its complement
    cases.append(Case("max_dist_256", q, {4: t, 5: t[69:]}, combos=((256, 0.0, False), (256, 0.0, True)), ranks=((256, 0.0, 8),),
                      props=[("count", 4, 256, 0.0, False, 40), ("count", 5, 256, 0.0, False, 40), ("knn", 5, 5, 0, 256, 257), ("match", 5, 256, 0.0, False, 5, 0),
                             ("votes", 5, 256, 0.0, 1)]))

    # masks: zero on exactly the winning train descriptors, zero on everything else, non-zero bytes that are 2 and 255
    rng = _rng("masks")
    q = rand_desc(rng, 60); t = rand_desc(rng, 120)
    win = np.sort(rng.choice(120, 20, replace=False))
    for j, at in enumerate(win):
        t[at] = flip(q[j], rng.integers(0, 21), rng)
    no_winner = np.ones(120, np.uint8); no_winner[win] = 0
    only_winners = np.zeros(120, np.uint8); only_winners[win] = 1
    odd = np.zeros(120, np.uint8); odd[win[0::2]] = 2; odd[win[1::2]] = 255
    half = np.zeros(120, np.uint8); half[win[:10:2]] = 2; half[win[1:10:2]] = 255; half[np.setdiff1d(np.arange(120), win)] = 255
    cases.append(Case("masks", q, {1: t, 2: t, 3: t, 4: t, 5: t}, {2: no_winner, 3: only_winners, 4: odd, 5: half}, combos=((MAX_DIST, RATIO, True),),
                      props=[("count", 1, MAX_DIST, RATIO, True, 20)] + [("votes", k, MAX_DIST, r, v) for r in (0.0, RATIO) for k, v in ((1, 20), (2, 0), (3, 20), (4, 20), (5, 10))]))
    return cases


# f. planted votes for k_rank_topk.  A set made of m exact copies of distinct query descriptors plus 0..3 random fillers scores m at
#    max_dist 10: the library holds one such set per (m, fillers), set i of a pattern stores VOTE_LIB[votes[i]][i % 4].
TOPK_MAX_DIST, TOPK_NQ, TOPK_MAX_VOTE = 10, 16, 8


@functools.lru_cache(None)
def vote_library():
    rng = _rng("vote_library")
    q = rand_desc(rng, TOPK_NQ)
    lib = {}
    for m in range(TOPK_MAX_VOTE + 1):
        for f in range(4):
            d = np.concatenate([q[rng.choice(TOPK_NQ, m, replace=False)], rand_desc(rng, f)])
            lib[(m, f)] = d[rng.permutation(m + f)]
    return q, lib


def topk_keys(n):
    """ascending keys of a pattern's n sets (index order on the device = key order), negative ones included"""
    return (np.arange(n, dtype=np.int64) * 3 - 1000 + (np.arange(n) % 2)).astype(np.int32)


# tied block at the K-th place: (top_k, sets above the block, index step between the block's members, where the cut falls).  The cut
# is the index of the first member of the block that is NOT taken; a thread of k_rank_topk owns the chunk [tid * per, tid * per + per),
# per = ceil(n / 1024), a wavefront 64 chunks.
TOPK_CUTS = ((8, 3, 1, "inside_chunk"), (8, 3, 1, "chunk_edge"), (8, 3, 1, "wave_edge"), (8, 0, 1, "first_at_0"), (8, 3, 1, "last_at_end"),
             (256, 40, 1, "inside_chunk"), (256, 40, 3, "chunk_edge"), (256, 40, 1, "wave_edge"), (256, 0, 2, "first_at_0"), (256, 40, 3, "last_at_end"),
             (1, 0, 1, "wave_edge"), (1, 0, 1, "last_at_end"))
TOPK_SIZES = (1, 1023, 1024, 1025, 4097)


def topk_cut_index(n, top_k, high, step, where):
    """(start of the tied block, number of members, cut index) of one TOPK_CUTS row at n sets"""
    per = (n + 1023) // 1024
    need, extra = top_k - high, 5
    members = need + extra
    if where == "first_at_0":
        start = 0
    elif where == "last_at_end":
        start = n - 1 - step * (members - 1)
    else:
        unit = 64 * per if where == "wave_edge" else per
        cut = -(-(step * need + 1) // unit) * unit                 # the first multiple of the unit that leaves room for the taken members
        if where == "chunk_edge" and cut % (64 * per) == 0:
            cut += per
        if where == "inside_chunk":
            cut += 1 if per > 1 else 0                             # (per == 1: every index is a chunk edge)
        start = cut - step * need
    return start, members, start + step * need


@functools.lru_cache(None)
def topk_patterns(n):
    """[(name, top_ks, votes[n])] for n stored sets"""
    pats = [("all_equal", (1, 8, 256), np.full(n, 3, np.int32)), ("all_zero", (1, 8, 256), np.zeros(n, np.int32))]
    few = np.zeros(n, np.int32)
    idx = np.unique([0, n // 3, n // 2, (2 * n) // 3, n - 1])
    few[idx] = np.array([2, 1, 2, 7, 1])[:len(idx)]
    pats.append(("few_nonzero", (8, 256) if n > 1 else (1, 8, 256), few))
    if n < 1023:
        return pats
    for top_k, high, step, where in TOPK_CUTS:
        start, members, cut = topk_cut_index(n, top_k, high, step, where)
        rng = _rng("topk" + where, n, top_k)
        votes = rng.integers(0, 4, n).astype(np.int32)             # below the block: 0..3
        block = start + step * np.arange(members)
        assert block[0] >= 0 and block[-1] < n
        votes[block] = 4
        outside = np.setdiff1d(np.arange(n), np.arange(block[0], block[-1] + 1))
        inside = np.setdiff1d(np.arange(block[0], block[-1] + 1), block)      # (between the members when step > 1)
        pool = np.concatenate([outside, inside])
        votes[rng.choice(pool, high, replace=False)] = rng.integers(5, TOPK_MAX_VOTE + 1, high)
        pats.append(("cut_%s_k%d" % (where, top_k), (top_k,), votes))
    return pats


# g. LDS regimes of rank_stored: 32 KB tile + 4 (nt_max + nq) + 4 bytes of dynamic LDS.  2000 queries: 6191 is the largest set at
#    64 KB, 6192 the first above it, 30767 the largest at 160 KB, 30768 is refused.  The companions run in the same launch (same LDS
#    size) and end in a partial 64-descriptor chunk of 1 and of 63 in every regime.
LDS_NQ = 2000
LDS_CASES = (("below_64k", (6191, 1025, 2111)), ("above_64k", (6192, 4097, 5055)), ("well_above_64k", (12000, 4097, 5055)), ("at_160k", (30767, 63, 4097)))
LDS_REFUSED_NT = 30768


def rk_lds_bytes(nt_max, nq):
    return 32 * 1024 + 4 * nt_max + 4 * nq + 4


def planted_big_set(rng, q, nt, n_plant=300):
    """nt descriptors with flipped copies of queries spread over the whole set, its last 64-descriptor chunk and its last index included;
    returns (set, mask, lo): the mask keeps the last chunk [lo, nt) and four fifths of the rest"""
    t = rand_desc(rng, nt)
    lo = (nt - 1) // 64 * 64
    n_plant = min(n_plant, nt, len(q))
    at = np.unique(np.concatenate([np.linspace(0, nt - 1, n_plant).astype(np.int64), np.arange(lo, nt)[-8:], [nt - 1]]))
    src = rng.choice(len(q), len(at), replace=len(at) > len(q))
    for a, s in zip(at, src):
        t[a] = flip(q[s], rng.integers(0, 45), rng)
    t[nt - 1] = q[src[-1]]                                          # an exact copy at the very last index
    mask = rng.choice(np.array([0, 1, 2, 255, 1], np.uint8), nt)
    mask[lo:] = 255
    return t, mask, lo


@functools.lru_cache(None)
def lds_case(name):
    sizes = dict(LDS_CASES)[name]
    rng = _rng("lds" + name)
    q = rand_desc(rng, LDS_NQ)
    sets, masks, props = {}, {}, []
    for key, nt in zip((20, -7, 33), sizes):
        sets[key], masks[key], lo = planted_big_set(rng, q, nt)
        props += [("votes_min", key, MAX_DIST, RATIO, min(100, nt // 4)), ("vote_in", key, MAX_DIST, RATIO, lo, nt), ("vote_in", key, MAX_DIST, RATIO, 0, 64)]
        if nt > BF_TILE:
            props.append(("vote_in", key, MAX_DIST, RATIO, BF_TILE, min(2 * BF_TILE, nt)))
    del masks[-7]                                                    # one companion without a mask
    return Case("lds_" + name, q, sets, masks, combos=(), ranks=((MAX_DIST, RATIO, 8),), props=props)


# h. match_bf_descriptors / match_bf_strided at multi-tile sizes
MULTI_TILE = ((1025, 2049), (2124, 2124))


@functools.lru_cache(None)
def multi_tile_case(nq, nt):
    rng = _rng("multi", nq, nt)
    q = rand_desc(rng, nq)
    t = flipped_subset(rng, q, nt)
    t[1030] = t[5]; q[0] = t[5]; t[1024] = t[1023]; q[1] = t[1023]; q[2] = flip(t[5], 1, rng)     # ties over the first tile edge
    return Case("multi_tile_%dx%d" % (nq, nt), q, {0: t}, combos=BOTH, ranks=(),
                props=[("knn", 0, 0, 5, 0, 0), ("knn", 0, 1, 1023, 0, 0), ("knn", 0, 2, 5, 1, 1), ("count_min", 0, MAX_DIST, 0.0, False, nq // 3)])


def planted_cases():
    """every case whose planted properties the CPU test asserts (the large LDS cases are built on demand: lds_case)"""
    return size_cases() + [many_keys_case()] + forward_tie_cases() + reverse_tie_cases() + threshold_cases() + [multi_tile_case(*s) for s in MULTI_TILE]


# ---- the planted properties, asserted on a reference ------------------------------------------------------------------------------
def check_props(case, knn2, matches):
    """asserts every planted property of `case` on a reference: knn2(q, t) -> (bi, bd, sd, rbi), matches(q, t, max_dist, ratio, cross) -> (mq, mt, md)"""
    memo = {}

    def knn2_of(key):
        if ("knn", key) not in memo:
            memo[("knn", key)] = knn2(case.q, case.sets[key])
        return memo[("knn", key)]

    def matches_of(key, *call):
        if (key,) + call not in memo:
            memo[(key,) + call] = matches(case.q, case.sets[key], *call)
        return memo[(key,) + call]

    for p in case.props:
        kind = p[0]
        if kind == "f32":
            _, ratio, second, best, rejected = p
            assert bool(np.float32(ratio) * np.float32(second) < np.float32(best)) == rejected, (case, p)
            continue
        if kind == "knn":
            _, _, qi, idx, dist, second = p
            bi, bd, sd, _ = knn2_of(p[1])
            assert bi[qi] == idx and bd[qi] == dist, (case, p, bi[qi], bd[qi])
            assert second is None or sd[qi] == second, (case, p, sd[qi])
        elif kind == "rev":
            assert knn2_of(p[1])[3][p[2]] == p[3], (case, p)
        elif kind == "match":
            _, _, max_dist, ratio, cross, qi, ti = p
            mq, mt, _ = matches_of(p[1], max_dist, ratio, cross)
            got = mt[mq == qi]
            assert (len(got) == 0) if ti < 0 else (len(got) == 1 and got[0] == ti), (case, p, got)
        elif kind in ("count", "count_min"):
            _, _, max_dist, ratio, cross, n = p
            got = len(matches_of(p[1], max_dist, ratio, cross)[0])
            assert got == n if kind == "count" else got >= n, (case, p, got)
        else:
            _, key, max_dist, ratio = p[:4]
            mt = matches_of(key, max_dist, ratio, True)[1]
            m = case.masks.get(key)
            voted = mt if m is None else mt[m[mt] != 0]
            if kind == "votes":
                assert len(voted) == p[4], (case, p, len(voted))
            elif kind == "votes_min":
                assert len(voted) >= p[4], (case, p, len(voted))
            elif kind == "vote_in":
                assert np.any((voted >= p[4]) & (voted < p[5])), (case, p)
            else:
                raise AssertionError("unknown property %r" % (p,))


def oracle_knn2(q, t):
    return O.match_bf_knn2(q, t) + (O.match_bf_knn2(t, q)[0],)
