"""The page-locked staging block of a context (h_match, lp_match_staging) changing hands: the window matchers, the vocabulary walk, the
bag-of-words matcher, the brute-force matchers and the pose optimiser all stage their inputs and receive their results in ONE block per
context, each with a layout, a done flag and a growth policy of its own.  The other tests exercise one user per context, or users of
one size; here every user runs inside one context, once with the block growing under them (calls ordered by rising need) and once
with the block at its final size from the first call on (the reverse order, on a second context), then a second time on the first
context.  It is the same kernel on the same inputs every time: the three result sets must be equal element for element."""
import numpy as np
import pytest

import bow_util
import match_cases as M
from lpslam_amd import synth

pytestmark = pytest.mark.gpu

W, H, KPTS, LEVELS = 320, 240, 400, 4


def _load(hiplib, oracle):
    """the stereo pair of test_window_match_gpu.py's `small` fixture in a context of its own: frame 0 in slots 0 / 1, frame 1 in 2 / 3"""
    seq = synth.StereoSequence(W, H, 5)
    l0, r0 = seq.frame(0); l1, r1 = seq.frame(1)
    k = synth.intrinsics(W, H)
    ctx = hiplib.Context(W, H, KPTS, 1.2, LEVELS, max_images=4)
    p = oracle.params(KPTS, 1.2, LEVELS)
    f0, bad0 = M.load_frame(oracle, ctx, p, 0, l0, 1, r0, k["fxb"], k["baseline"])
    f1, bad1 = M.load_frame(oracle, ctx, p, 2, l1, 3, r1, k["fxb"], k["baseline"])
    assert not (bad0 + bad1), (bad0, bad1)
    return ctx, f0, f1


def _al(x):
    return (x + 63) & ~63


def _calls(hiplib, f0, f1, S):
    """[(name, staging bytes the call needs, run(ctx, f1 of that context, vocabulary of that context) -> tuple of arrays / numbers,
    the oracle's arguments for a window-matcher call or None)], inputs fixed here once.  The needs restate the size expressions of the
    library: match.hip (window_match, the two brute-force entry points), bow.hip (bow_transform_device, lpslam_hip_match_bow_tree_multi),
    pose_opt.hip (the all-in-LDS block); S = slots per image."""
    rng = np.random.default_rng(23)
    nk0, nk1 = len(f0.kp), len(f1.kp)
    out = []

    # pose optimiser, 16 observations: header 128 | packed observations (7 doubles) | outlier bytes
    n = 16
    cam = dict(synth.intrinsics(640, 480))
    pts = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(2, 20, n)], axis=1)
    obs = np.zeros(n, hiplib.BA_OBS_DTYPE)
    obs["point"] = np.arange(n)
    obs["u"] = cam["fx"] * pts[:, 0] / pts[:, 2] + cam["cx"] + rng.normal(0, 0.5, n)
    obs["v"] = cam["fy"] * pts[:, 1] / pts[:, 2] + cam["cy"] + rng.normal(0, 0.5, n)
    obs["ur"] = np.where(rng.random(n) < 0.6, obs["u"] - cam["fxb"] / pts[:, 2], -1.0)
    obs["inv_sigma2"] = 1.0
    start = np.concatenate([[1, 0, 0, 0], rng.normal(0, 0.02, 3)])
    out.append(("pose_optimize, 16 observations", 128 + n * 56 + n,
                lambda c, fr, voc: hiplib.pose_optimize(c, start, pts, obs, cam), None))

    # window matcher: keys 32 | query 24 | descriptor 32 | count 4 per query, 64 (ids, done flag), best-so-far 2 per slot
    def window_need(nq): return nq * (32 + 24 + 32 + 4) + 64 + 2 * S
    src = rng.permutation(nk0)[:8]
    q8 = M.queries(f0.kp["x"][src] + rng.normal(0, 4, 8), f0.kp["y"][src] + rng.normal(0, 4, 8), 15.0 * np.float32(1.2) ** f0.kp["octave"][src])
    qd8 = f0.desc[src].copy()
    out.append(("match_projection, 8 queries", window_need(8), lambda c, fr, voc: M.run_gpu(fr, "projection", q8, qd8, 100, 0.9),
                (q8, qd8, 100, 0.9)))
    q_all = M.queries(f0.kp["x"] + rng.normal(0, 4, nk0), f0.kp["y"] + rng.normal(0, 4, nk0), 15.0 * np.float32(1.2) ** f0.kp["octave"])
    qd_all = f0.desc.copy()
    taken = np.zeros(nk1, np.uint8); taken[::5] = 1
    out.append(("match_projection, every keypoint of frame 0, taken mask", window_need(nk0),
                lambda c, fr, voc: M.run_gpu(fr, "projection", q_all, qd_all, 100, 0.9, taken), (q_all, qd_all, 100, 0.9, taken)))

    # vocabulary walk over a slot: 64 (done flag, count) | word ids | weights | node ids, one each per slot
    out.append(("Vocabulary.transform", 64 + 3 * 4 * S, lambda c, fr, voc: voc.transform(fr.slot, 2), None))

    # bag-of-words matcher, one set; every descriptor has a node: query descriptors | segments, target descriptors, taken | set table |
    # keys, counts | ids
    vocab = _vocab()
    qn = bow_util.walk_numpy(vocab, f0.desc, 2)[2]; tn = bow_util.walk_numpy(vocab, f1.desc, 2)[2]
    assert (qn > 0).all() and (tn > 0).all() and len(np.intersect1d(qn, tn)) > 1
    bow_need = _al(nk0 * 32) + _al(nk0 * 8) + _al(nk1 * 32) + _al(nk1) + _al(32) + _al(nk0 * 32) + _al(nk0 * 4) + 64
    out.append(("match_bow_tree, one set", bow_need, lambda c, fr, voc: hiplib.match_bow_tree(c, f0.desc, qn, f1.desc, tn, 60, 0.9), None))

    # brute force against descriptors from the host, cross-checked: 16 words | 3 per query | 1 per train descriptor.  (Slot 1, the right
    # image of frame 0, is the scratch slot.)  lpslam_hip_get_bf_matches on the same pair is the filter's third caller: the same matches
    def bf_descriptors(c, fr, voc):
        got = c.match_bf_descriptors(fr.slot, 1, f0.desc, 60, 0.9, True)
        ref = c.bf_matches(fr.slot, 1, 60, 0.9, True)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "match_bf_descriptors and bf_matches differ"
        return got
    out.append(("match_bf_descriptors, cross-checked", 4 * (16 + 3 * nk1 + nk0), bf_descriptors, None))

    # brute force against the two stored sets (_run), one of them empty: 64 | pair list (40 each) | run list (16 each), to 64 | 16 words,
    # 3 per query and set, 1 per stored descriptor
    def bf_stored(c, fr, voc):
        r = c.match_bf_stored(fr.slot, [7, 9], 60, 0.9, True)
        assert len(r[1][0]) == 0
        return r[0] + r[1]
    out.append(("match_bf_stored, two keys", _al(64 + 4 * 40 + 4 * 16) + 4 * (16 + 2 * 3 * nk1 + nk0), bf_stored, None))

    out.sort(key=lambda e: e[1])
    # place ranking keeps a page-locked block of its own: it shares the done-flag protocol and the arrival counter of the brute-force
    # matchers, not the block -- last in the list
    out.append(("rank_stored", 0, lambda c, fr, voc: c.rank_stored(fr.slot, None, 60, 0.9, 4), None))
    return out


def _vocab():
    return bow_util.make_vocab(np.random.default_rng(5), 6, 3, flip=0.25)


def _flat(r):
    """a call's result as a tuple of (dtype, shape, bytes) / numbers: equality is element for element, floats bit for bit"""
    return tuple((a.dtype.str, a.shape, a.tobytes()) if isinstance(a, np.ndarray) else a for a in r)


def _run(hiplib, ctx, f0, fr, calls):
    """a context's vocabulary and stored descriptor sets (neither touches the staging block), then the calls in the order given"""
    v = _vocab()
    voc = hiplib.Vocabulary(ctx, v["k"], v["L"], v["parent"], v["desc"], v["weight"], v["is_leaf"])
    ctx.desc_store_put(7, f0.desc); ctx.desc_store_put(9, np.zeros((0, 32), np.uint8))
    return {name: fn(ctx, fr, voc) for name, need, fn, _ in calls}, voc


def test_the_staging_block_changes_hands_and_regrows(hiplib, oracle):
    ctx_a, f0, f1a = _load(hiplib, oracle)
    ctx_b, _, f1b = _load(hiplib, oracle)
    try:
        calls = _calls(hiplib, f0, f1a, ctx_a.max_kp)
        needs = [c[1] for c in calls[:-1]]
        assert needs == sorted(needs) and len(set(needs)) == len(needs), needs
        assert calls[0][0].startswith("pose_optimize") and needs[0] < 2048 and needs[-1] > 16 * needs[0]       # grows from the first call to the last kind
        fwd, voc_a = _run(hiplib, ctx_a, f0, f1a, calls)                 # A: the block regrows under the first call of each larger user
        rev, voc_b = _run(hiplib, ctx_b, f0, f1b, calls[::-1])           # B: at its final size from the first call on
        again = {name: fn(ctx_a, f1a, voc_a) for name, need, fn, _ in calls}
        for name in fwd:
            assert _flat(fwd[name]) == _flat(rev[name]), "%s: growing block and full-size block differ" % name
            assert _flat(fwd[name]) == _flat(again[name]), "%s: first and second run on one context differ" % name
        # the two window-matcher calls against the oracle, exactly (match_cases.compare's checks)
        for name, _, _, oracle_args in calls:
            if oracle_args is None: continue
            gi, gd, gn, _ = fwd[name]
            oi, od, on = M.run_oracle(oracle, f1a, "projection", *oracle_args)
            assert np.array_equal(gi, oi) and gn == on == int((gi >= 0).sum()) and np.array_equal(gd[gi >= 0], od[oi >= 0]), name
            assert on > (4 if "8 queries" in name else 50), (name, on)
        assert fwd["pose_optimize, 16 observations"][2] >= 8 and len(fwd["Vocabulary.transform"][0]) == len(f1a.kp)
        assert fwd["match_bow_tree, one set"][2] > 20 and len(fwd["match_bf_descriptors, cross-checked"][0]) > 20
        assert len(fwd["match_bf_stored, two keys"][0]) > 20 and list(fwd["rank_stored"][0]) == [7]
    finally:
        ctx_a.close(); ctx_b.close()
