"""GPU parity tests of the bag-of-words kernels through the C ABI against the CPU oracle: the tree walk (word, weight, node per
keypoint: array_equal) and match::bow_tree (match indices and distances: array_equal, ties and taken targets included)."""
import numpy as np
import pytest

from bow_util import LEVELS_UP, VOCAB_CASES, levels_up_of, make_vocab, read_vocab, vocab_case, walk_case, walk_numpy
from lpslam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(hiplib):
    v = read_vocab()
    ctx = hiplib.Context(640, 480, 1000, 1.2, 4, max_images=2)
    voc = hiplib.Vocabulary(ctx, v["k"], v["L"], v["parent"], v["desc"], v["weight"], v["is_leaf"])
    assert (voc.k, voc.L, voc.n_nodes, voc.n_words) == (10, 3, len(v["parent"]), 1000)
    return v, ctx, voc


def test_transform_parity_on_extracted_keypoints(hiplib, oracle, setup):
    v, ctx, voc = setup
    seq = synth.StereoSequence(640, 480, 4, n_points=6000)
    l, r = seq.frame(3)
    ctx.upload(0, l); ctx.upload(1, r)
    ctx.extract(2)
    for slot in (0, 1):
        _, desc = ctx.keypoints(slot)
        assert len(desc) > 500
        for lu in (0, 1, 2, 4):
            w, ww, nd = voc.transform(slot, lu)
            ow, oww, ond = oracle.bow_transform(v, desc, lu)
            assert np.array_equal(w, ow) and np.array_equal(ww, oww) and np.array_equal(nd, ond), (slot, lu)
    # descriptors from host memory, some of them exactly on tree nodes (ties between children)
    rng = np.random.default_rng(3)
    d = rng.integers(0, 256, (777, 32), dtype=np.uint8)
    d[:100] = v["desc"][rng.integers(0, len(v["desc"]), 100)]
    w, ww, nd = voc.transform_host(d, 1)
    ow, oww, ond = oracle.bow_transform(v, d, 1)
    assert np.array_equal(w, ow) and np.array_equal(ww, oww) and np.array_equal(nd, ond)


def test_vocabulary_arguments_are_checked(hiplib, setup):
    v, ctx, _ = setup
    bad_parent = v["parent"].copy(); bad_parent[5] = 900                      # a parent that does not precede its child
    with pytest.raises(hiplib.LpslamHipError):
        hiplib.Vocabulary(ctx, 10, 3, bad_parent, v["desc"], v["weight"], v["is_leaf"])
    bad_leaf = v["is_leaf"].copy(); bad_leaf[0] = 1                            # node 1 has children
    with pytest.raises(hiplib.LpslamHipError):
        hiplib.Vocabulary(ctx, 10, 3, v["parent"], v["desc"], v["weight"], bad_leaf)


@pytest.mark.parametrize("levels_up,ratio,thr", [(1, 0.75, 50), (2, 0.9, 50), (3, 1.0, 100), (0, 0.6, 30)])
def test_bow_tree_match_parity(hiplib, oracle, setup, levels_up, ratio, thr):
    """two consecutive frames: keypoints of the first (a third of them switched off, as keypoints without a landmark are) against
    the second's; with levels_up = 3 the node is the root (L = 3): every query scans every target, lists get exhausted and the
    single-query rescans run"""
    v, ctx, voc = setup
    seq = synth.StereoSequence(640, 480, 4, n_points=6000)
    ctx.upload(0, seq.frame(5)[0]); ctx.upload(1, seq.frame(6)[0])
    ctx.extract(2)
    _, da = ctx.keypoints(0); _, db = ctx.keypoints(1)
    rng = np.random.default_rng(11)
    db = db.copy(); db[40:60] = db[20:40]                                       # duplicated descriptors: ties between targets
    _, _, na = voc.transform_host(da, levels_up); _, _, nb = voc.transform_host(db, levels_up)
    na = na.copy(); na[rng.random(len(na)) < 0.33] = -1
    taken = (rng.random(len(db)) < 0.1).astype(np.uint8)
    gi, gd, gn = hiplib.match_bow_tree(ctx, da, na, db, nb, thr, ratio, taken)
    oi, od, on = oracle.bow_tree_match(da, na, db, nb, thr, ratio, taken)
    assert gn == on and on > 50 and np.array_equal(gi, oi) and np.array_equal(gd[gi >= 0], od[oi >= 0])
    assert np.all(gi[na < 0] == -1) and not np.any(taken[gi[gi >= 0]])
    m = gi[gi >= 0]
    assert len(np.unique(m)) == len(m)                                          # a target is matched once


def test_bow_tree_match_of_several_sets_in_one_call(hiplib, oracle, setup):
    """one keyframe's descriptors against five target sets (different frames, ragged sizes, an empty set, a set without a node in common,
    one with a `taken` mask) in ONE call: every set's result is that of the single-set call and of the oracle"""
    v, ctx, voc = setup
    seq = synth.StereoSequence(640, 480, 4, n_points=6000)
    ctx.upload(0, seq.frame(5)[0])
    ctx.extract(1)
    _, da = ctx.keypoints(0)
    rng = np.random.default_rng(3)
    _, _, na = voc.transform_host(da, 1)
    na = na.copy(); na[rng.random(len(na)) < 0.3] = -1
    tds, tns, tks = [], [], []
    for i, fr in enumerate((6, 7, 9)):
        ctx.upload(1, seq.frame(fr)[0]); ctx.extract_range(1, 1)
        _, db = ctx.keypoints(1)
        db = db[: len(db) - 37 * i].copy()
        _, _, nb = voc.transform_host(db, 1)
        tds.append(db); tns.append(nb.copy()); tks.append((rng.random(len(db)) < 0.1).astype(np.uint8) if i == 1 else None)
    tds.append(np.zeros((0, 32), np.uint8)); tns.append(np.zeros(0, np.int32)); tks.append(None)                 # an empty set
    tds.append(tds[0].copy()); tns.append(np.full(len(tns[0]), -1, np.int32)); tks.append(None)                  # no target is under a node
    multi = hiplib.match_bow_tree_multi(ctx, da, na, tds, tns, 50, 0.75, tks)
    assert len(multi) == 5
    total = 0
    for (gi, gd, gn), td, tn, tk in zip(multi, tds, tns, tks):
        si, sd, sn = hiplib.match_bow_tree(ctx, da, na, td, tn, 50, 0.75, tk) if len(td) else (np.full(len(na), -1, np.int32), None, 0)
        assert gn == sn and np.array_equal(gi, si)
        if len(td):
            oi, od, on = oracle.bow_tree_match(da, na, td, tn, 50, 0.75, tk if tk is not None else np.zeros(len(td), np.uint8))
            assert gn == on and np.array_equal(gi, oi) and np.array_equal(gd[gi >= 0], od[oi >= 0])
        total += gn
    assert total > 100 and multi[3][2] == 0 and multi[4][2] == 0


# ---- the tree walk on generated vocabularies --------------------------------------------------------------------------------------
# k_bow_transform16 gives sixteen lanes to a descriptor; lane `sub` takes children sub, sub + 16, ...  The committed vocabulary (k = 10,
# L = 3, perfectly balanced) never makes a lane take a second child, never ends a walk above level L and never leaves the node id 0.
#   k2_L6, k3_L6            the production depth; 2 and 3 of the sixteen lanes busy
#   k16_L2, k17_L2, k33_L2  exactly one trip of the child loop, one child into the second trip, one into the third
#   k10_L4                  one level deeper than the committed file at the product's k (11110 nodes)
#   ragged                  declared k = 20, L = 5: 1 .. 20 children per node, words at every depth from 1 to 5, duplicated siblings
#   leaf_at_1               a word directly under the root
@pytest.fixture(scope="module")
def small_ctx(hiplib):
    ctx = hiplib.Context(320, 240, 400, 1.2, 4, max_images=2)
    yield ctx
    ctx.close()


def _device_vocab(hiplib, ctx, v):
    return hiplib.Vocabulary(ctx, v["k"], v["L"], v["parent"], v["desc"], v["weight"], v["is_leaf"])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", list(VOCAB_CASES))
def test_transform_on_generated_vocabularies(hiplib, oracle, small_ctx, case):
    """word id, weight and node id of 300 descriptors against the oracle AND the numpy walk, with the node level below, at and above
    the root.  The ragged case's input conditions (words above level L - 1 for a fifth of the descriptors, a fifth at depth L, exact
    sibling ties, single-child nodes) are asserted here on the reference and in tests/test_bow_cpu.py."""
    v, desc = vocab_case(case)
    voc = _device_vocab(hiplib, small_ctx, v)
    try:
        assert (voc.k, voc.L, voc.n_nodes, voc.n_words) == (v["k"], v["L"], len(v["parent"]), int(v["is_leaf"].sum()))
        for lu in LEVELS_UP:
            levels_up = levels_up_of(lu, v["L"])
            got = voc.transform_host(desc, levels_up)
            (want, st) = walk_case(case, levels_up)
            assert _same(got, oracle.bow_transform(v, desc, levels_up)), (case, lu, "oracle")
            assert _same(got, want), (case, lu, "numpy walk")
            if case == "ragged" and levels_up == 1:
                n, L = len(desc), v["L"]
                assert (st["depth"] < L - 1).sum() >= n // 5 and (st["depth"] == L).sum() >= n // 5
                assert st["tie"].sum() >= 20 and st["single"].sum() >= 20
                assert np.all(got[2][st["depth"] < L - 1] == 0) and np.all(got[2][st["depth"] >= L - 1] > 0)
            if case == "leaf_at_1":
                assert (st["depth"] == 1).sum() >= 10 and np.all(got[0][st["depth"] == 1] == 0)      # the root's third child is word 0
    finally:
        voc.close()


def test_transform_tie_break_takes_the_first_child(hiplib, oracle, small_ctx):
    """one level, 40 children: lane `sub` holds orders sub, sub + 16 and sub + 32.  Equal children: 17 = 2 (the lower order on the
    HIGHER lane), 19 = 3 (the same lane, two trips), 36 = 20 (the same lane, second and third trip), 39 = 0 (first and last child)."""
    rng = np.random.default_rng(31)
    v = make_vocab(rng, 40, 1, flip=0.5)
    assert len(v["parent"]) == 40 and v["is_leaf"].all()
    for later, first in ((17, 2), (19, 3), (36, 20), (39, 0)):
        v["desc"][later] = v["desc"][first]
    q = v["desc"][[2, 3, 20, 0, 17, 19, 36, 39, 5, 38]]
    voc = _device_vocab(hiplib, small_ctx, v)
    try:
        for lu in (0, 1):
            w, ww, nd = voc.transform_host(q, lu)
            assert w.tolist() == [2, 3, 20, 0, 2, 3, 20, 0, 5, 38], lu
            assert np.array_equal(ww, v["weight"][w]) and nd.tolist() == ([w_ + 1 for w_ in w.tolist()] if lu == 0 else [0] * 10)
            assert _same((w, ww, nd), oracle.bow_transform(v, q, lu)) and _same((w, ww, nd), walk_numpy(v, q, lu))
    finally:
        voc.close()


def test_transform_descriptor_counts(hiplib, oracle):
    """counts around the sixteen-lane group (16 descriptors a wavefront quarter) and the 256-thread workgroup (16 descriptors each):
    partly filled groups and workgroups.  One fresh context, ascending counts and then a small one again: the page-locked result
    block grows and is then reused at a smaller size."""
    v, _ = vocab_case("ragged")
    rng = np.random.default_rng(32)
    pool = rng.integers(0, 256, (4097, 32), dtype=np.uint8)
    pool[::3] = v["desc"][rng.integers(0, len(v["desc"]), len(pool[::3]))]
    want = oracle.bow_transform(v, pool, 1)
    ctx = hiplib.Context(320, 240, 400, 1.2, 4, max_images=2)
    voc = _device_vocab(hiplib, ctx, v)
    try:
        for n in (1, 15, 16, 17, 255, 256, 257, 4097, 8):
            d = pool[4097 - n:]                                                  # the tail: a count's first descriptor is not the last count's
            got = voc.transform_host(d, 1)
            assert len(got[0]) == n and _same(got, [x[4097 - n:] for x in want]), n
        assert all(len(x) == 0 for x in voc.transform_host(np.zeros((0, 32), np.uint8), 1))
    finally:
        voc.close(); ctx.close()


def test_transform_of_a_device_slot(hiplib, oracle, small_ctx):
    """descriptors already on the device (the count is read there): the same result as for descriptors from host memory"""
    v, desc = vocab_case("ragged")
    voc = _device_vocab(hiplib, small_ctx, v)
    try:
        n = 299                                                                  # 18 groups of sixteen and 11 lanes' worth
        assert n % 16 and n <= small_ctx.max_kp
        small_ctx.set_descriptors(0, desc[:n])
        for lu in (0, 1, 5):
            got = voc.transform(0, lu)
            assert len(got[0]) == n and _same(got, voc.transform_host(desc[:n], lu)) and _same(got, oracle.bow_transform(v, desc[:n], lu)), lu
        small_ctx.set_descriptors(1, desc[:7])
        assert len(voc.transform(1, 1)[0]) == 7 and len(voc.transform(0, 1)[0]) == n
        small_ctx.set_descriptors(0, np.zeros((0, 32), np.uint8))
        got = voc.transform(0, 1)
        assert [len(x) for x in got] == [0, 0, 0]
    finally:
        voc.close()


def test_child_count_guard_uses_the_real_widest_node(hiplib, oracle, small_ctx):
    """the child order has 16 bits in the kernel's key.  What the file DECLARES as k says nothing about the tree: one that declares
    k = 10 and has a node with 65536 children is refused; with 65535 children it works, up to the last child"""
    rng = np.random.default_rng(33)
    big = make_vocab(rng, 10, 1, branch=lambda r, d: 65536, flip=0.5)
    assert big["k"] == 10 and len(big["parent"]) == 65536 and big["is_leaf"].all()
    with pytest.raises(hiplib.LpslamHipError):
        voc = _device_vocab(hiplib, small_ctx, big)
        try:
            voc.transform_host(big["desc"][:4], 0)                               # (a library that refuses at the first transform)
        finally:
            voc.close()
    v = {f: (x[:65535] if isinstance(x, np.ndarray) else x) for f, x in big.items()}
    d = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    d[:20] = v["desc"][rng.integers(0, 65535, 20)]
    d[20] = d[63] = v["desc"][65534]
    voc = _device_vocab(hiplib, small_ctx, v)
    try:
        assert voc.n_words == 65535
        got = voc.transform_host(d, 0)
        assert _same(got, oracle.bow_transform(v, d, 0)) and _same(got, walk_numpy(v, d, 0))
        assert got[0][20] == 65534 and got[0][63] == 65534 and got[2][20] == 65535
    finally:
        voc.close()


# ---- match::bow_tree at planted segment shapes --------------------------------------------------------------------------------------
# bow_topk_body: one wavefront per query over the targets of its node (64 lanes, four candidates kept per lane and per query), the host
# replays the order-dependent part over those lists and scans again for one query where its list was eaten (`m < 2 && cnt > 4`).
SEGMENTS = (1, 2, 4, 5, 63, 64, 65, 255, 256, 257, 1000)


def _noisy(rng, d, bits):
    """copies of the descriptors d with `bits` distinct bits flipped"""
    out = d.copy().reshape(-1, 32)
    for row in out:
        for b in rng.choice(256, bits, replace=False):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _planted(seed=41):
    """one node per segment size (ids not contiguous, up to 1 000 000), three queries each and four for the last: nq is no multiple of
    4; a node with queries only, one with targets only, queries and targets without a node; both sides shuffled"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(999_999, len(SEGMENTS) + 1, replace=False)).tolist() + [1_000_000]
    only_q, only_t = ids.pop(3), ids.pop(7)
    td, tn, qd, qn = [], [], [], []
    for node, size in zip(ids, SEGMENTS):
        t = rng.integers(0, 256, (size, 32), dtype=np.uint8)
        td.append(t); tn += [node] * size
        nq = 4 if size == SEGMENTS[-1] else 3
        qd.append(_noisy(rng, t[rng.integers(0, size, nq)], 10)); qn += [node] * nq
    td.append(rng.integers(0, 256, (30, 32), dtype=np.uint8)); tn += [only_t] * 10 + [-1] * 20
    qd.append(rng.integers(0, 256, (7, 32), dtype=np.uint8)); qn += [only_q] * 3 + [-1] * 4
    td, qd, tn, qn = np.concatenate(td), np.concatenate(qd), np.array(tn, np.int32), np.array(qn, np.int32)
    pt, pq = rng.permutation(len(tn)), rng.permutation(len(qn))
    return qd[pq], qn[pq], td[pt], tn[pt], only_q


def _match_both(hiplib, oracle, ctx, qd, qn, td, tn, thr, ratio, taken=None):
    gi, gd, gn = hiplib.match_bow_tree(ctx, qd, qn, td, tn, thr, ratio, taken)
    oi, od, on = oracle.bow_tree_match(qd, qn, td, tn, thr, ratio, taken)
    assert gn == on and np.array_equal(gi, oi) and np.array_equal(gd[gi >= 0], od[oi >= 0])
    assert gn == (gi >= 0).sum() and len(np.unique(gi[gi >= 0])) == gn
    return gi, gd, gn


def test_bow_tree_match_segment_sizes(hiplib, oracle, small_ctx):
    qd, qn, td, tn, only_q = _planted()
    assert len(qn) == 41 and (qn >= 0).sum() == 37 and tn.max() == 1_000_000 and (tn < 0).any() and (qn < 0).any()
    for thr, ratio in ((50, 0.9), (256, 1.0), (10, 0.6)):
        gi, gd, gn = _match_both(hiplib, oracle, small_ctx, qd, qn, td, tn, thr, ratio)
        assert np.all(gi[(qn < 0) | (qn == only_q)] == -1)
        assert np.all(tn[gi[gi >= 0]] == qn[gi >= 0])                            # a match stays under its node
        if thr >= 50:
            assert gn >= len(qn) // 2


def test_bow_tree_match_of_equal_descriptors(hiplib, oracle, small_ctx):
    """300 identical targets under one node: every distance ties, the position (target index order) decides"""
    rng = np.random.default_rng(42)
    one = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    td = np.repeat(one, 300, axis=0); tn = np.full(300, 77, np.int32); qn = np.full(5, 77, np.int32)
    near = np.repeat(_noisy(rng, one, 10), 5, axis=0)                              # ten bits from every target
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, np.repeat(one, 5, axis=0), qn, td, tn, 0, 1.0)
    assert gi.tolist() == [0, 1, 2, 3, 4] and gd.tolist() == [0] * 5
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, near, qn, td, tn, 10, 1.0)
    assert gi.tolist() == [0, 1, 2, 3, 4] and gd.tolist() == [10] * 5
    # best == second: nothing passes a ratio below 1 ...
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, near, qn, td, tn, 256, 0.9)
    assert gn == 0 and gi.tolist() == [-1] * 5
    # ... unless both are 0: upstream rejects on `ratio * second < best`, and 0.9 * 0 is not below 0
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, np.repeat(one, 5, axis=0), qn, td, tn, 256, 0.9)
    assert gi.tolist() == [0, 1, 2, 3, 4]


def test_bow_tree_match_rescan_is_needed_and_runs(hiplib, oracle, small_ctx):
    """12 identical queries, 40 targets at 1, 2, ..., 40 bits from them: every query's list of four is targets 0 .. 3, so from the
    fifth query on a match exists only through the single-query re-scan (without it four queries would match)"""
    rng = np.random.default_rng(43)
    one = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    td = np.concatenate([_noisy(rng, one, b) for b in range(1, 41)])
    tn = np.full(40, 123456, np.int32); qn = np.full(12, 123456, np.int32)
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, np.repeat(one, 12, axis=0), qn, td, tn, 256, 1.0)
    assert gn == 12 and gi.tolist() == list(range(12)) and gd.tolist() == list(range(1, 13))


def test_bow_tree_match_four_nearest_targets_on_one_lane(hiplib, oracle, small_ctx):
    """One query and 64 * 4 + 1 = 257 targets under one node: lane l of the query's wavefront meets targets l, l + 64, l + 128, ...
    The four nearest (8, 9, 10 and 11 bits from the query, every other target 60) are targets 5, 69, 133 and 197 -- all lane 5 -- so
    the wavefront's four answers are one lane's whole list, popped four times.  8 against 9 fails a ratio of 0.8, 8 against a lost
    second (60) would pass; with the successive bests marked taken every entry becomes the head in turn, and only 11 against 60
    passes."""
    rng = np.random.default_rng(46)
    one = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    best4 = [5, 69, 133, 197]
    td = _noisy(rng, np.repeat(one, 257, axis=0), 60)
    for r, t in enumerate(best4):
        td[t] = _noisy(rng, one, 8 + r)
    tn = np.full(257, 31, np.int32); qn = np.full(1, 31, np.int32)
    for stage in range(5):
        taken = np.zeros(257, np.uint8); taken[best4[:stage]] = 1
        gi, gd, gn = _match_both(hiplib, oracle, small_ctx, one, qn, td, tn, 256, 0.8, taken if stage else None)
        assert gi.tolist() == ([best4[3]] if stage == 3 else [-1]), (stage, gi)        # 8 : 9, 9 : 10, 10 : 11 fail, 11 : 60 passes, 60 : 60 fails
        gi, gd, gn = _match_both(hiplib, oracle, small_ctx, one, qn, td, tn, 256, 1.0, taken if stage else None)
        if stage < 4:
            assert gi.tolist() == [best4[stage]] and gd.tolist() == [8 + stage], (stage, gi, gd)
        else:
            assert gn == 1 and gd.tolist() == [60] and gi[0] not in best4


def test_bow_tree_match_taken_masks(hiplib, oracle, small_ctx):
    rng = np.random.default_rng(44)
    td = rng.integers(0, 256, (6, 32), dtype=np.uint8); tn = np.full(6, 9, np.int32)
    qd = _noisy(rng, td[[1, 4, 4]], 5); qn = np.full(3, 9, np.int32)
    gi, _, gn = _match_both(hiplib, oracle, small_ctx, qd, qn, td, tn, 256, 1.0, np.ones(6, np.uint8))
    assert gn == 0 and gi.tolist() == [-1, -1, -1]                               # every target was taken beforehand
    taken = np.ones(6, np.uint8); taken[4] = 0                                   # one free target: one candidate, no second, no re-scan
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, qd, qn, td, tn, 256, 1.0, taken)
    assert gi.tolist() == [4, -1, -1] and gd[0] > 5                              # the first query has it (second = 256), the others nothing
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, qd[1:], qn[1:], td, tn, 4, 1.0, taken)
    assert gn == 0                                                               # five bits away, threshold four
    gi, gd, gn = _match_both(hiplib, oracle, small_ctx, qd[1:], qn[1:], td, tn, 5, 1.0, taken)
    assert gi.tolist() == [4, -1] and gd[0] == 5


def test_bow_tree_match_planted_sets_in_one_call(hiplib, oracle, small_ctx):
    """the planted set, an empty set and the planted set with a `taken` mask in one call: each as the single-set call gives it"""
    qd, qn, td, tn, _ = _planted()
    rng = np.random.default_rng(45)
    taken = (rng.random(len(tn)) < 0.5).astype(np.uint8)
    tds = [td, np.zeros((0, 32), np.uint8), td]; tns = [tn, np.zeros(0, np.int32), tn]; tks = [None, None, taken]
    multi = hiplib.match_bow_tree_multi(small_ctx, qd, qn, tds, tns, 50, 0.9, tks)
    assert len(multi) == 3 and multi[1][2] == 0 and np.all(multi[1][0] == -1)
    for s in (0, 2):
        si, sd, sn = _match_both(hiplib, oracle, small_ctx, qd, qn, tds[s], tns[s], 50, 0.9, tks[s])
        gi, gd, gn = multi[s]
        assert gn == sn and np.array_equal(gi, si) and np.array_equal(gd[gi >= 0], sd[si >= 0])
    assert multi[0][2] >= len(qn) // 2 and 0 < multi[2][2] and not np.any(taken[multi[2][0][multi[2][0] >= 0]])
    assert not np.array_equal(multi[0][0], multi[2][0])                          # the mask changed something
