"""The planted cases of tests/store_cases.py, checked without a GPU: the two references -- the oracle's C code and the numpy
restatement -- agree exactly on every case, and every planted property (a tie and who wins it, a threshold on its edge and the
neighbour one step past it, a vote count, where the cut of a tied block falls) holds on the reference itself, so a case cannot
silently miss the edge tests/test_store_planted_gpu.py runs it for."""
import numpy as np
import pytest

import store_cases as sc


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", sc.planted_cases(), ids=repr)
def test_references_agree_and_properties_hold(case):
    for key, t in case.sets.items():
        knn = sc.numpy_knn2(case.q, t)
        assert _same(sc.oracle_knn2(case.q, t), knn), (case, key)
        calls = set(case.combos) | {(md, r, True) for md, r, _ in case.ranks}
        for max_dist, ratio, cross in sorted(calls):
            assert _same(sc.reference_matches(case.q, t, max_dist, ratio, cross), sc.numpy_matches(case.q, t, max_dist, ratio, cross, knn)), (case, key, max_dist, ratio, cross)
    sc.check_props(case, sc.oracle_knn2, sc.reference_matches)
    sc.check_props(case, sc.numpy_knn2, sc.numpy_matches)


def test_flip_is_exact():
    rng = np.random.default_rng(1)
    d = sc.rand_desc(rng, 1)[0]
    for k in (0, 1, 8, 50, 231, 256):
        f = sc.flip(d, k, rng)
        assert int(np.unpackbits(f ^ d).sum()) == k
    q = sc.rand_desc(rng, 2000)                                          # the planted distances (60 at most) dominate
    bi, bd, sd, _ = sc.numpy_knn2(q, q)
    assert np.array_equal(bi, np.arange(2000)) and sd.min() >= 87


def test_size_groups_cover_the_structural_sizes():
    assert {nq for nq, _ in sc.SIZE_GROUPS} == {1, 16, 17, 255, 256, 257, 2124}
    assert {nt for _, sizes in sc.SIZE_GROUPS for nt in sizes} - {0} == {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 3000}
    assert max(nt for _, sizes in sc.SIZE_GROUPS for nt in sizes) > sc.SLOTS
    assert all(len({len(t) for t in c.sets.values()}) > 1 for c in sc.size_cases())          # nt_max differs from most sets' nt
    assert len(sc.many_keys_case().sets) > 48


def test_tie_tables_sit_on_the_merge_boundaries():
    tied = {t for _, _, t in sc.FORWARD_TIES}
    assert {(63, 64), (255, 256), (1023, 1024), (5, 1030), (1023, 1024, 2048)} <= tied
    assert any(t[0] == 0 and t[1] == nt - 1 for _, nt, t in sc.FORWARD_TIES)
    pairs = {tuple(q for q, _ in near) for _, near, _, _ in sc.REVERSE_TIES}
    assert {(3, 4), (3, 67), (3, 300), (255, 256)} <= pairs
    for a, b in ((3, 67), (3, 300), (255, 256)):
        assert a // 64 != b // 64                                          # two wavefronts
    assert 3 // sc.RK_PASS != 300 // sc.RK_PASS and 255 // sc.RK_PASS != 256 // sc.RK_PASS      # two passes of k_rank_votes


def test_vote_library_scores_its_planted_votes():
    q, lib = sc.vote_library()
    for ratio in (0.0, sc.RATIO):
        votes = sc.reference_votes(q, lib, {}, sc.TOPK_MAX_DIST, ratio)
        assert all(votes[(m, f)] == m for m, f in lib), votes
    for (m, f), d in lib.items():
        assert len(d) == m + f and len(sc.numpy_matches(q, d, sc.TOPK_MAX_DIST, sc.RATIO, True)[0]) == m


@pytest.mark.parametrize("n", sc.TOPK_SIZES)
def test_topk_patterns_cut_where_planted(n):
    keys = sc.topk_keys(n)
    assert np.all(np.diff(keys) > 0) and keys[0] < 0
    per = (n + 1023) // 1024
    pats = dict((name, (top_ks, votes)) for name, top_ks, votes in sc.topk_patterns(n))
    assert len(pats) == (3 if n == 1 else 3 + len(sc.TOPK_CUTS))
    for name, (top_ks, votes) in pats.items():
        assert len(votes) == n and votes.min() >= 0 and votes.max() <= sc.TOPK_MAX_VOTE
        by_key = dict(zip(keys.tolist(), votes.tolist()))
        for top_k in top_ks:
            rk, rv = sc.reference_rank(by_key, top_k)
            assert len(rk) == min(top_k, int(np.count_nonzero(votes)))
            assert np.all(np.diff(rv) <= 0) and np.all((np.diff(rv) < 0) | (np.diff(rk) > 0))
    assert np.count_nonzero(pats["all_zero"][1]) == 0 and len(set(pats["all_equal"][1].tolist())) == 1
    assert 0 < np.count_nonzero(pats["few_nonzero"][1]) < 8
    if n == 1:
        return
    for top_k, high, step, where in sc.TOPK_CUTS:
        top_ks, votes = pats["cut_%s_k%d" % (where, top_k)]
        start, members, cut = sc.topk_cut_index(n, top_k, high, step, where)
        block = start + step * np.arange(members)
        assert np.array_equal(np.flatnonzero(votes == 4), block) and np.count_nonzero(votes > 4) == high
        rk, rv = sc.reference_rank(dict(zip(keys.tolist(), votes.tolist())), top_k)
        taken = np.sort(np.searchsorted(keys, rk[rv == 4]))
        # the first `need` members of the block are taken, the cut index is the first member that is not
        assert np.array_equal(taken, block[:top_k - high]) and block[top_k - high] == cut and len(rk) == top_k and np.count_nonzero(rv > 4) == high
        if where == "inside_chunk":
            assert per == 1 or cut % per != 0
        elif where == "chunk_edge":
            assert cut % per == 0 and cut % (64 * per) != 0
        elif where == "wave_edge":
            assert cut % (64 * per) == 0
        elif where == "first_at_0":
            assert block[0] == 0
        else:
            assert block[-1] == n - 1


def test_lds_regimes_sit_on_their_lines():
    nq = sc.LDS_NQ
    big = {name: sizes[0] for name, sizes in sc.LDS_CASES}
    assert sc.rk_lds_bytes(big["below_64k"], nq) == 64 * 1024 and sc.rk_lds_bytes(big["above_64k"], nq) == 64 * 1024 + 4
    assert 64 * 1024 < sc.rk_lds_bytes(big["well_above_64k"], nq) < 160 * 1024
    assert sc.rk_lds_bytes(big["at_160k"], nq) == 160 * 1024 and nq + big["at_160k"] == 32767
    assert sc.rk_lds_bytes(sc.LDS_REFUSED_NT, nq) == 160 * 1024 + 4 and nq + sc.LDS_REFUSED_NT == 32768
    for _, sizes in sc.LDS_CASES:
        assert {1, 63} <= {nt % 64 for nt in sizes}


@pytest.mark.parametrize("name", [name for name, _ in sc.LDS_CASES])
def test_lds_cases_vote_in_every_tile(name):
    """the big sets: the two references agree (the 2-NN in full, the filtered matches at the call's thresholds) and the planted copies
    give votes in the first chunk, the second tile and the last, partial chunk"""
    case = sc.lds_case(name)
    for key, t in case.sets.items():
        knn = sc.numpy_knn2(case.q, t)
        assert _same(sc.oracle_knn2(case.q, t), knn), (case, key)
        for max_dist, ratio, _ in case.ranks:
            assert _same(sc.reference_matches(case.q, t, max_dist, ratio, True), sc.numpy_matches(case.q, t, max_dist, ratio, True, knn)), (case, key)
    sc.check_props(case, sc.oracle_knn2, sc.reference_matches)
