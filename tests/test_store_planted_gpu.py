"""The descriptor store, lpslam_hip_match_bf_stored (k_bf_knn2_pairs with per-pair sizes and the reverse pair, k_runs_to_host) and
lpslam_hip_rank_stored (k_rank_votes, k_rank_topk) against the CPU oracle on the planted cases of tests/store_cases.py: structural
sizes around the 64 / 256 / 1024-descriptor merges, sets larger than the slot count, more than 48 keys in a call, forward and reverse
ties, thresholds on their edge, masks, the tie cut of the top K, and the dynamic-LDS regimes of k_rank_votes up to its refusal.

Every comparison is exact (integers) and every expectation comes from store_cases (oracle.match_bf, counting, sorting): no device
call produces one.  The keys=None form of rank_stored is compared with the same reference as the explicit-keys form.
tests/test_store_ref_cpu.py asserts, without a GPU, that each case really has the property it is named for."""
import ctypes as C

import numpy as np
import pytest

import store_cases as sc

pytestmark = pytest.mark.gpu

ERR_CAPACITY = 3


@pytest.fixture(scope="module")
def ctx(hiplib):
    """2100 keypoints / 8 levels: 2124 descriptor slots per image"""
    c = hiplib.Context(1280, 720, 2100, 1.2, 8, max_images=4)
    assert c.max_kp == sc.SLOTS
    yield c
    c.close()


def _put(ctx, case):
    for key, t in case.sets.items():
        ctx.desc_store_put(key, t)
        if key in case.masks:
            ctx.desc_store_mask(key, case.masks[key])


def _drop(ctx, keys):
    for k in keys:
        ctx.desc_store_drop(int(k))


def _assert_rank(ctx, slot, keys, votes, max_dist, ratio, top_k, what):
    want_k, want_v = sc.reference_rank(votes, top_k)
    got_k, got_v = ctx.rank_stored(slot, keys, max_dist, ratio, top_k)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v), (what, "keys", got_k[:8], got_v[:8], want_k[:8], want_v[:8])
    all_k, all_v = ctx.rank_stored(slot, None, max_dist, ratio, top_k)           # keys == NULL: every stored set
    assert np.array_equal(all_k, want_k) and np.array_equal(all_v, want_v), (what, "all", all_k[:8], all_v[:8], want_k[:8], want_v[:8])


def run_case(ctx, case, rng=None):
    """stores the case's sets, makes its calls, compares each with the oracle, drops the sets"""
    ctx.set_descriptors(0, case.q)
    keys = list(case.sets)
    if rng is not None:
        keys = [keys[i] for i in rng.permutation(len(keys))]
    try:
        _put(ctx, case)
        for max_dist, ratio, cross in case.combos:
            got = ctx.match_bf_stored(0, keys, max_dist, ratio, cross)
            assert len(got) == len(keys)
            for key, g in zip(keys, got):
                want = sc.reference_matches(case.q, case.sets[key], max_dist, ratio, cross)
                for name, a, b in zip(("query", "train", "distance"), g, want):
                    assert np.array_equal(a, b), (case, key, len(case.sets[key]), max_dist, ratio, cross, name)
        for max_dist, ratio, top_k in case.ranks:
            votes = sc.reference_votes(case.q, case.sets, case.masks, max_dist, ratio)
            _assert_rank(ctx, 0, keys, votes, max_dist, ratio, top_k, (case, max_dist, ratio, top_k))
    finally:
        _drop(ctx, case.sets)


@pytest.mark.parametrize("case", sc.size_cases(), ids=repr)
def test_stored_sets_at_structural_sizes(ctx, case):
    """a: several sets of different sizes in one call (nt_max differs from most sets' nt, empty sets, 3000 > the slot count)"""
    run_case(ctx, case)


def test_more_than_48_keys_in_one_call(ctx):
    """b: 120 sets of 5 to 300 descriptors, keys in shuffled order: both blocks of match_bf_stored grow past their 48-set size"""
    run_case(ctx, sc.many_keys_case(), np.random.default_rng(2))


@pytest.mark.parametrize("case", sc.forward_tie_cases(), ids=repr)
def test_forward_ties_first_index_wins(ctx, case):
    """c: identical train descriptors across the sub-range, wavefront and tile merges; masks tell the winner from the losers in the
    votes; the second distance of a tied query is the tie's distance: only that makes the ratio test reject queries 1 and 2"""
    run_case(ctx, case)


@pytest.mark.parametrize("case", sc.reverse_tie_cases(), ids=repr)
def test_reverse_ties_smallest_query_owns(ctx, case):
    """d: one train descriptor equidistant from queries in neighbouring lanes, two wavefronts, two passes of k_rank_votes"""
    run_case(ctx, case)


@pytest.mark.parametrize("case", sc.threshold_cases(), ids=repr)
def test_thresholds_on_their_edge(ctx, case):
    """e: best == max_dist, ratio * second == best in float32, second = 257 for a single descriptor, max_dist 256, masks"""
    run_case(ctx, case)


@pytest.mark.parametrize("n", sc.TOPK_SIZES)
def test_topk_cut_of_planted_votes(ctx, n):
    """f: n sets with planted vote counts (store_cases.vote_library), keys shuffled and partly negative; the tie cut at the K-th place
    inside a thread's chunk, on a chunk edge, on a wavefront edge, with the block at index 0 and at n - 1"""
    q, lib = sc.vote_library()
    ctx.set_descriptors(0, q)
    keys = sc.topk_keys(n)
    shuffled = keys[np.random.default_rng(n).permutation(n)]
    stored = {}
    try:
        for name, top_ks, votes in sc.topk_patterns(n):
            for i, v in enumerate(votes.tolist()):
                if stored.get(i) != v:                                     # (a put replaces the set under its key)
                    ctx.desc_store_put(int(keys[i]), lib[(v, i % 4)]); stored[i] = v
            by_key = dict(zip(keys.tolist(), votes.tolist()))
            for top_k in top_ks:
                _assert_rank(ctx, 0, shuffled, by_key, sc.TOPK_MAX_DIST, sc.RATIO, top_k, (n, name, top_k))
    finally:
        _drop(ctx, keys)


@pytest.mark.parametrize("name", [name for name, _ in sc.LDS_CASES])
def test_rank_lds_regimes(ctx, name):
    """g: 2000 queries, largest set 6191 (64 KB of dynamic LDS), 6192 (the first above), 12000, 30767 (160 KB); votes come from
    every tile and from the last, partial chunk of each set"""
    run_case(ctx, sc.lds_case(name))


def test_rank_refuses_one_past_the_lds_limit(ctx):
    """g: nq + nt_max = 32768 needs 160 KB + 4 bytes: the capacity error, n_out 0, outputs untouched, the store intact"""
    case = sc.lds_case("below_64k")
    rng = np.random.default_rng(9)
    too_big = sc.rand_desc(rng, sc.LDS_REFUSED_NT)
    ctx.set_descriptors(0, case.q)
    try:
        _put(ctx, case)
        ctx.desc_store_put(77, too_big)
        keys = np.array(list(case.sets) + [77], np.int32)
        ok = np.full(8, -12345, np.int32); ov = np.full(8, -12345, np.int32); n = C.c_int32(99)
        # the wrapper raises on an error code and owns its output arrays; the entry point through a prototype of the test's own
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
        f = proto(("lpslam_hip_rank_stored", ctx.lib))
        for kk, nk in ((keys.ctypes.data_as(C.c_void_p), len(keys)), (None, 0)):
            n.value = 99
            rc = f(ctx.h, 0, kk, nk, sc.MAX_DIST, sc.RATIO, 8, ok.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == ERR_CAPACITY and n.value == 0
            assert np.all(ok == -12345) and np.all(ov == -12345)
        # the refused call changed nothing: the in-range sets still rank as the reference says, the big one still matches as a set
        votes = sc.reference_votes(case.q, case.sets, case.masks, sc.MAX_DIST, sc.RATIO)
        want_k, want_v = sc.reference_rank(votes, 8)
        got_k, got_v = ctx.rank_stored(0, list(case.sets), sc.MAX_DIST, sc.RATIO, 8)
        assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)
        ctx.desc_store_drop(77)
        all_k, all_v = ctx.rank_stored(0, None, sc.MAX_DIST, sc.RATIO, 8)
        assert np.array_equal(all_k, want_k) and np.array_equal(all_v, want_v)
    finally:
        _drop(ctx, list(case.sets) + [77])


@pytest.mark.parametrize("nq,nt", sc.MULTI_TILE)
def test_descriptors_and_strided_at_multi_tile_sizes(ctx, nq, nt):
    """h: match_bf_descriptors (k_bf_knn2 both ways + k_words_to_host) and match_bf_strided over two pairs, train sets of more than
    one and more than two LDS tiles, against the oracle"""
    case = sc.multi_tile_case(nq, nt)
    q, t = case.q, case.sets[0]
    ctx.set_descriptors(0, q)
    for max_dist, ratio, cross in case.combos:
        got = ctx.match_bf_descriptors(0, 1, t, max_dist, ratio, cross)
        want = sc.reference_matches(q, t, max_dist, ratio, cross)
        for name, a, b in zip(("query", "train", "distance"), got, want):
            assert np.array_equal(a, b), (case, max_dist, ratio, cross, name)
    # strided: pairs (0, 2) and (1, 3) in one launch, the second pair the first one mirrored
    ctx.set_descriptors(1, t[:sc.SLOTS]); ctx.set_descriptors(2, t[:sc.SLOTS]); ctx.set_descriptors(3, q)
    ctx.match_bf_strided(0, 2, 1, 2)
    for slot, (a, b) in ((0, (q, t[:sc.SLOTS])), (1, (t[:sc.SLOTS], q))):
        for name, g, o in zip(("best_idx", "best_dist", "second_dist"), ctx.bf_knn2(slot), sc.O.match_bf_knn2(a, b)):
            assert np.array_equal(g, o), (case, slot, name)
