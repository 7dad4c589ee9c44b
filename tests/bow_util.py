"""Test helpers of the bag-of-words tests: the reader of a DBoW2 binary vocabulary (the layout tools/train_vocabulary.py writes and
lpslam_amd/host/bow.cpp reads), a seeded generator of vocabulary trees of any shape (ragged ones as DBoW2's training leaves them), the
brute-force numpy walk both the oracle and the device kernel are held against, and the table of generated trees the CPU and the GPU
tests share."""
import functools
import os
import struct

import numpy as np

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_k10_L3.dbow2")


def read_vocab(path=VOCAB):
    raw = open(path, "rb").read()
    n, size, k, L, scoring, weighting = struct.unpack_from("<6I", raw, 0)
    assert size == 41
    n = (len(raw) - 24) // 41            # the header counts the records, or the records and the root (DBoW2): the file decides
    rec = np.frombuffer(raw, np.uint8, n * 41, 24).reshape(n, 41)
    return dict(k=k, L=L, parent=rec[:, :4].copy().view("<u4").reshape(n).astype(np.int32), desc=rec[:, 4:36].copy(),
                weight=rec[:, 36:40].copy().view("<f4").reshape(n), is_leaf=rec[:, 40].copy())


def make_vocab(rng, k, L, branch=None, stop=0.0, dup=0.0, flip=0.12):
    """A vocabulary tree in memory, the dict read_vocab() returns: nodes 1-based in file order (a node's children are consecutive, a
    parent precedes its children, as DBoW2 creates them), `k` and `L` what the file would declare.
    branch(rng, depth)  number of children of a node at `depth` (the root: 0); default k.  0 makes the node a leaf.
    stop                probability that a node at depth 1 .. L - 1 is a leaf
    dup                 probability that a child's descriptor is a copy of an earlier sibling's (an exact tie for a query on it)
    flip                a child's descriptor is its parent's with every bit flipped with this probability (the root's is random), so a
                        query copied from a deep node does walk down to it and meets the ties there; 0.5 = independent descriptors
    Weights are random float32, about one in ten exactly 0.0 (a word every training image contains has idf 0)."""
    parent, desc = [], []
    queue = [(0, 0, rng.integers(0, 256, 32, dtype=np.uint8))]         # node id, depth, descriptor
    n = 0
    while queue:
        node, d, nd = queue.pop(0)
        if d >= L or (d >= 1 and rng.random() < stop):
            continue
        nc = int(branch(rng, d)) if branch else k
        if nc <= 0:
            continue
        ch = nd[None, :] ^ np.packbits(rng.random((nc, 256)) < flip, axis=1)
        for j in np.flatnonzero(rng.random(nc) < dup):
            if j > 0:
                ch[j] = ch[rng.integers(0, j)]
        parent.append(np.full(nc, node, np.int32)); desc.append(ch)
        if d + 1 < L:
            queue.extend((n + 1 + j, d + 1, ch[j]) for j in range(nc))
        n += nc
    parent = np.concatenate(parent); desc = np.concatenate(desc)
    weight = rng.random(n).astype(np.float32)
    weight[rng.random(n) < 0.1] = 0.0
    is_leaf = (np.bincount(parent, minlength=n + 1)[1:] == 0).astype(np.uint8)
    return dict(k=int(k), L=int(L), parent=parent, desc=desc, weight=weight, is_leaf=is_leaf)


_POPCOUNT = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)


def walk_numpy(vocab, desc, levels_up, stats=None):
    """[UPSTREAM] DBoW2 TemplatedVocabulary::transform, restated as plainly as numpy allows: from the root to the child with the smallest
    Hamming distance (argmin: the first one on a tie) until a leaf; the word is the leaf's rank among the leaves in file order, the node
    id the node passed at level L - levels_up (0 when the walk never is at that level).  The children of a node are read off `parent`
    itself, not off a start/list table as the oracle and the device library build one.
    stats (a dict) receives per descriptor: `depth` of its leaf, `tie` (the smallest distance was shared by two children at some
    level), `single` (it passed a node with one child)."""
    parent, node_desc, is_leaf = vocab["parent"], vocab["desc"], vocab["is_leaf"]
    word_of = np.cumsum(is_leaf) - 1
    kids = {}
    n = len(desc)
    word = np.zeros(n, np.int32); weight = np.zeros(n, np.float32); nid = np.zeros(n, np.int32)
    depth = np.zeros(n, np.int32); tie = np.zeros(n, bool); single = np.zeros(n, bool)
    for f in range(n):
        cur, level = 0, 0
        while cur == 0 or not is_leaf[cur - 1]:
            level += 1
            if cur not in kids:
                kids[cur] = np.flatnonzero(parent == cur) + 1
            ch = kids[cur]
            ds = _POPCOUNT[node_desc[ch - 1] ^ desc[f]].sum(1)
            j = int(np.argmin(ds))
            tie[f] |= int((ds == ds[j]).sum()) > 1
            single[f] |= len(ch) == 1
            cur = int(ch[j])
            if level == vocab["L"] - levels_up:
                nid[f] = cur
        word[f] = word_of[cur - 1]; weight[f] = vocab["weight"][cur - 1]; depth[f] = level
    if stats is not None:
        stats.update(depth=depth, tie=tie, single=single)
    return word, weight, nid


def _ragged_branch(rng, depth):
    """the root is full (20); below it a quarter of the nodes have one child, the others 1 .. 20"""
    if depth == 0:
        return 20
    return 1 if rng.random() < 0.25 else int(rng.integers(1, 21))


def _leaf_at_1_branch():
    seen = [0]

    def branch(rng, depth):
        if depth == 1:
            seen[0] += 1
            return 0 if seen[0] == 3 else 5                              # the root's third child (order 2) is a word itself
        return 5
    return branch


# name -> (seed, k, L, further arguments of make_vocab).  What each one reaches in k_bow_transform16 is in tests/test_bow_gpu.py.
VOCAB_CASES = {
    "k2_L6": (21, 2, 6, {}),
    "k3_L6": (22, 3, 6, {}),
    "k16_L2": (23, 16, 2, {}),
    "k17_L2": (24, 17, 2, {}),
    "k33_L2": (25, 33, 2, {}),
    "k10_L4": (26, 10, 4, {}),
    "ragged": (27, 20, 5, dict(branch=_ragged_branch, stop=0.3, dup=0.2)),
    "leaf_at_1": (28, 5, 3, dict(branch=None)),
}
LEVELS_UP = ("0", "1", "L-1", "L", "L+2")


def levels_up_of(name, L):
    return {"0": 0, "1": 1, "L-1": L - 1, "L": L, "L+2": L + 2}[name]


@functools.lru_cache(maxsize=None)
def vocab_case(name):
    """the generated tree `name` and its 300 descriptors -- a third copies of node descriptors, a third random, a third near a node --
    built once per process and read-only"""
    seed, k, L, kw = VOCAB_CASES[name]
    kw = dict(kw)
    if name == "leaf_at_1":
        kw["branch"] = _leaf_at_1_branch()
    rng = np.random.default_rng(seed)
    v = make_vocab(rng, k, L, **kw)
    desc = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    desc[:100] = v["desc"][rng.integers(0, len(v["desc"]), 100)]
    desc[200:] = v["desc"][rng.integers(0, len(v["desc"]), 100)] ^ np.packbits(rng.random((100, 256)) < 0.05, axis=1)   # near a node
    for a in list(v.values()) + [desc]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v, desc


@functools.lru_cache(maxsize=None)
def walk_case(name, levels_up):
    """walk_numpy of the case's descriptors, computed once and shared by the CPU and the GPU tests; the arrays are read-only"""
    v, desc = vocab_case(name)
    stats = {}
    out = walk_numpy(v, desc, levels_up, stats)
    for a in out + tuple(stats.values()):
        a.setflags(write=False)
    return out, stats
