"""lpslam_hip_rank_stored: whole-map place ranking on the device.  votes(k) is the number of matches
lpslam_hip_match_bf_stored(query, {k}, max_dist, ratio, cross_check=1) reports whose train keypoint passes k's mask; the result is the
top K keys by (votes desc, key asc).  The reference here is exactly that: match_bf_stored in chunks of <= 48 sets and numpy counting."""
import numpy as np
import pytest

import store_cases

pytestmark = pytest.mark.gpu

MAX_DIST, RATIO = 50, 0.75


@pytest.fixture(scope="module")
def ctx(hiplib):
    """2100 keypoints / 8 levels: 2124 descriptor slots per image, room for 2000-descriptor query slots"""
    c = hiplib.Context(1280, 720, 2100, 1.2, 8, max_images=2)
    yield c
    c.close()


def _clear(ctx, keys):
    for k in keys:
        ctx.desc_store_drop(int(k))


def _reference(ctx, query, keys, masks, top_k, max_dist=MAX_DIST, ratio=RATIO):
    votes = {}
    keys = [int(k) for k in keys]
    for i in range(0, len(keys), 48):
        chunk = keys[i:i + 48]
        for k, (mq, mt, md) in zip(chunk, ctx.match_bf_stored(query, chunk, max_dist, ratio, True)):
            m = masks.get(k)
            votes[k] = len(mt) if m is None else int(np.count_nonzero(m[mt]))
    order = sorted((k for k in keys if votes[k] >= 1), key=lambda k: (-votes[k], k))[:top_k]
    return np.array(order, np.int32), np.array([votes[k] for k in order], np.int32), votes


def _make_map(ctx, rng, q, n_sets, nd, twins=0):
    """stored sets: bit-flipped subsets of the query descriptors plus random fillers, random masks (none, partial, all zero),
    `twins` sets stored twice under another key (equal votes: the key decides)"""
    flips = (rng.random((4096, 32)) < 0.04).astype(np.uint8) << rng.integers(0, 8, (4096, 32)).astype(np.uint8)
    keys = rng.choice(np.arange(-5000, 100000), n_sets, replace=False).astype(np.int32)
    masks, sets = {}, {}
    for i, key in enumerate(keys):
        key = int(key)
        if twins and i >= n_sets - twins:
            src = int(keys[i - twins])
            sets[key] = sets[src]
            if src in masks:
                masks[key] = masks[src]
        else:
            nt = int(rng.integers(nd // 2, nd + 1)) if i % 7 else nd
            frac = rng.random() * 0.6
            k = min(int(nt * frac), nd)
            base = q[rng.choice(nd, k, replace=False)] ^ flips[rng.integers(0, 4096, k)]
            d = np.concatenate([base, rng.integers(0, 256, (nt - k, 32), dtype=np.uint8)])
            sets[key] = d[rng.permutation(nt)]
            r = rng.random()
            if r < 0.6:
                masks[key] = (rng.random(nt) < 0.8).astype(np.uint8)
            elif r < 0.65:
                masks[key] = np.zeros(nt, np.uint8)
        ctx.desc_store_put(key, sets[key])
        if key in masks:
            ctx.desc_store_mask(key, masks[key])
    return keys, masks, sets


@pytest.mark.parametrize("nd", [1200, 2000])
@pytest.mark.parametrize("n_sets", [1, 47, 48, 49, 1000, 3000])
def test_rank_equals_chunked_matching(ctx, n_sets, nd):
    rng = np.random.default_rng(n_sets * 31 + nd)
    q = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
    ctx.set_descriptors(0, q)
    keys, masks, _ = _make_map(ctx, rng, q, n_sets, nd, twins=min(4, n_sets // 8))
    try:
        for top_k in (8, 256, 1):
            want_k, want_v, votes = _reference(ctx, 0, keys, masks, top_k)
            got_k, got_v = ctx.rank_stored(0, keys, MAX_DIST, RATIO, top_k)
            assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v), (top_k, got_k[:8], want_k[:8])
            all_k, all_v = ctx.rank_stored(0, None, MAX_DIST, RATIO, top_k)       # keys == NULL: every stored set
            assert np.array_equal(all_k, want_k) and np.array_equal(all_v, want_v)
        if n_sets >= 47:
            assert sum(v > 0 for v in votes.values()) > n_sets // 3       # the case is not trivially empty
    finally:
        _clear(ctx, keys)


def test_rank_other_thresholds_and_key_order(ctx):
    """another max_dist / ratio (ratio 0 disables the test), keys listed in any order"""
    rng = np.random.default_rng(5)
    nd = 700
    q = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
    ctx.set_descriptors(1, q)
    keys, masks, sets = _make_map(ctx, rng, q, 130, nd, twins=10)
    try:
        for max_dist, ratio in ((80, 0.0), (30, 0.9), (256, 0.75)):
            want_k, want_v, votes = _reference(ctx, 1, keys, masks, 40, max_dist, ratio)
            assert votes == store_cases.reference_votes(q, sets, masks, max_dist, ratio)       # the chunked device reference against the CPU oracle
            got_k, got_v = ctx.rank_stored(1, keys[::-1], max_dist, ratio, 40)
            assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v), (max_dist, ratio)
    finally:
        _clear(ctx, keys)


def test_rank_ties_are_ordered_by_key(ctx):
    """identical sets under many keys: equal votes, key ascending, and the cut at top_k takes the smallest keys"""
    rng = np.random.default_rng(11)
    q = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    ctx.set_descriptors(0, q)
    d = q[:300] ^ (rng.random((300, 32)) < 0.03).astype(np.uint8)
    keys = [90, -3, 7, 1000, 45, 2, 61, 13, 8, 5]
    for k in keys:
        ctx.desc_store_put(k, d)
    ctx.desc_store_put(500, d[:150])                                   # fewer votes, below the tied block
    try:
        got_k, got_v = ctx.rank_stored(0, None, MAX_DIST, RATIO, 4)
        assert list(got_k) == [-3, 2, 5, 7] and len(set(got_v.tolist())) == 1 and got_v[0] > 150
        got_k, got_v = ctx.rank_stored(0, None, MAX_DIST, RATIO, 11)
        assert list(got_k) == sorted(keys) + [500] and got_v[-1] < got_v[0]
        want_k, want_v, _ = _reference(ctx, 0, keys + [500], {}, 11)
        assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)
    finally:
        _clear(ctx, keys + [500])


def test_rank_empty_sets_slot_and_masks(ctx):
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    ctx.set_descriptors(0, q)
    ctx.desc_store_put(1, np.zeros((0, 32), np.uint8))                 # empty set: 0 votes
    ctx.desc_store_mask(1, np.zeros(0, np.uint8))
    ctx.desc_store_put(2, q[:200])
    ctx.desc_store_put(3, q[:250])
    ctx.desc_store_mask(3, np.zeros(250, np.uint8))                    # all-zero mask: 0 votes
    try:
        got_k, got_v = ctx.rank_stored(0, [1, 2, 3], MAX_DIST, RATIO, 8)
        assert list(got_k) == [2] and list(got_v) == [200]
        ctx.desc_store_put(3, q[:250])                                   # a put clears the mask
        got_k, got_v = ctx.rank_stored(0, [1, 2, 3], MAX_DIST, RATIO, 8)
        assert list(got_k) == [3, 2] and list(got_v) == [250, 200]
        half = np.zeros(250, np.uint8); half[::2] = 1
        ctx.desc_store_mask(3, half)
        got_k, got_v = ctx.rank_stored(0, [1, 2, 3], MAX_DIST, RATIO, 8)
        assert list(got_k) == [2, 3] and list(got_v) == [200, 125]
        ctx.set_descriptors(0, np.zeros((0, 32), np.uint8))              # empty query slot: nothing has a vote
        got_k, got_v = ctx.rank_stored(0, [1, 2, 3], MAX_DIST, RATIO, 8)
        assert len(got_k) == 0 and len(got_v) == 0
        assert len(ctx.rank_stored(0, [], MAX_DIST, RATIO, 8)[0]) == 0
    finally:
        _clear(ctx, [1, 2, 3])


def test_rank_invalid_arguments(ctx, hiplib):
    rng = np.random.default_rng(4)
    q = rng.integers(0, 256, (100, 32), dtype=np.uint8)
    ctx.set_descriptors(0, q)
    ctx.desc_store_put(10, q[:50]); ctx.desc_store_put(11, q[50:])
    try:
        bad = [lambda: ctx.rank_stored(0, [10, 12], MAX_DIST, RATIO, 8),          # unknown key
               lambda: ctx.rank_stored(0, [10, 11, 10], MAX_DIST, RATIO, 8),      # duplicate key
               lambda: ctx.rank_stored(0, [10, 11], MAX_DIST, RATIO, 0),          # top_k outside 1..256
               lambda: ctx.rank_stored(0, None, MAX_DIST, RATIO, 257),
               lambda: ctx.desc_store_mask(10, np.ones(49, np.uint8)),            # mask length is not the set's
               lambda: ctx.desc_store_mask(12, np.ones(50, np.uint8))]            # mask of an unknown key
        for call in bad:
            with pytest.raises(hiplib.LpslamHipError, match="error 1:"):
                call()
        got_k, got_v = ctx.rank_stored(0, [10, 11], MAX_DIST, RATIO, 256)
        assert list(got_k) == [10, 11] and list(got_v) == [50, 50]
    finally:
        _clear(ctx, [10, 11])
