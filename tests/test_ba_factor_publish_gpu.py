"""What k_chol_pair still publishes of the factor: Ldiag and Lsub have one reader, k_chol_xsolve, which takes the rhs row
out of the system's LAST panel column, so the diagonal workgroup stores that row of the column's diagonal block (and, for the second
column of a pair, L_j1,j) in the system's last launch and nothing in any other.  Everything else of those arrays keeps what an earlier
solve or the allocation left there.  No arithmetic changed, so x_p keeps the parent commit's bytes.

Systems go through lpslam_hip_ba_debug_solve (tests/solve_runner.py); per dimension the `known` system and the k = 6 ladder of
tests/solve_cases.py.  dim = 6 x free keyframes, nb = ceil((dim + 1) / 32) panel columns, need = dim - 32 (nb - 1) real columns in
the last one:

     dim  nb  launches                                  need
       6   1  `single` at m = 0                            6
      30   1  `single` at m = 0                           30
      36   2  pair, the rhs row in j1                      4
      48   2  pair, the rhs row in j1                     16
      54   2  pair, the rhs row in j1                     22
      66   3  pair + `single` with a previous pair         2
      96   4  two pairs, the last column is the rhs row    0
     102   4  two pairs                                    6
     132   5  pair, pair, `single` with a previous pair    4
     294  10  the benchmark's window                       6
     306  10  above k_chol_wg's limit                     18
     600  19  nine pairs and a `single`                   24

1. x_p and the pivot flag of a fresh problem are, byte for byte, those the parent commit's library gave through the same hook on an
   MI355X (tests/golden/factor_publish/parent.npz, written by tools/dev/factor_publish_golden.py).
2. A problem that has solved another system of its dimension before gives the bytes of a fresh one, in both orders: a block that is
   read but no longer written would come from the earlier solve.  And both give the stored bytes: where a block is written by NO
   solve, a fresh and a used problem read the same thing, whatever the allocation held, and agree with each other (seen with the
   publication of the pair launches taken out: dims 96 - 306 got zeroed pages and equal, wrong bytes).
3. Systems of different length in one call: the chain runs the longest system's launches, a shorter system's last column lies in an
   earlier one.  Each gets the bytes it gets alone.
4. A pivot <= 0 in a first column of a pair, in a second column, in the last column, and in the first panel of the benchmark's
   dimension raises the flag and gives the zero step; the next positive definite solve on that problem gives the fresh bytes."""
import os

import numpy as np
import pytest

import solve_cases as sc
import solve_runner as sr

pytestmark = pytest.mark.gpu

NB = 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_publish", "parent.npz")
# dim, nb, need
CASES = [(6, 1, 6), (30, 1, 30), (36, 2, 4), (48, 2, 16), (54, 2, 22), (66, 3, 2), (96, 4, 0), (102, 4, 6), (132, 5, 4), (294, 10, 6),
         (306, 10, 18), (600, 19, 24)]
DIMS = [c[0] for c in CASES]
FAMILIES = ("known", "ladder6")
MIXED = ((36, 66, 132, 294), (96, 102))
# dim, failing pivot, where.  nb = 2 / 4 / 5 / 10 for dim 54 / 102 / 132 / 294.
NOTPD = ((54, 5, "first column of the only pair"),
         (102, 40, "second column of the first pair: not the last column"),
         (102, 90, "first column of the last pair"),
         (54, 50, "last column, second of a pair"),
         (132, 129, "last column, `single`"),
         (294, 10, "first panel of the benchmark's dimension"),
         (294, 200, "first column of its fourth pair"),
         (294, 250, "second column of its fourth pair"))
ZERO_PIVOT = sc.ZERO_PIVOT


def system(dim, family):
    return sc.known(dim) if family == "known" else sc.ladder(dim, 6)


def key(dim, family):
    return "%s_%d" % (family, dim)


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = hiplib.Context(320, 240, 400, 1.2, 4, max_images=1)
    yield c
    c.close()


def solve_fresh(hiplib, ctx, cases):
    """every case on a problem of its own that has solved nothing before: [(x, flag)]"""
    out = []
    for c in cases:
        h = sr.Holders(hiplib, ctx)
        out.append(h.alone(c))
        h.close()
    return out


@pytest.fixture(scope="module")
def fresh(hiplib, ctx):
    """(dim, family) -> (x_p, flag) of a fresh problem: the reference of every test here, computed once"""
    keys = [(dim, f) for dim in DIMS for f in FAMILIES]
    return dict(zip(keys, solve_fresh(hiplib, ctx, [system(*k) for k in keys])))


@pytest.fixture(scope="module")
def holders(hiplib, ctx):
    h = sr.Holders(hiplib, ctx)
    yield h
    h.close()


@pytest.mark.parametrize("dim,nb,need", CASES, ids=["dim%d" % d for d in DIMS])
def test_bytes_of_the_parent_commit(fresh, dim, nb, need):
    assert dim % 6 == 0 and (dim + 1 + NB - 1) // NB == nb and dim - NB * (nb - 1) == need
    stored = np.load(GOLDEN)
    for f in FAMILIES:
        x, flag = fresh[dim, f]
        px, pflag = stored["x_" + key(dim, f)], int(stored["flag_" + key(dim, f)])
        assert flag == pflag == 0
        assert x.dtype == px.dtype and x.shape == px.shape == (dim,) and x.tobytes() == px.tobytes(), (dim, f)


@pytest.mark.parametrize("dim", DIMS, ids=["dim%d" % d for d in DIMS])
def test_stale_blocks_are_never_read(hiplib, ctx, fresh, dim):
    a, b = system(dim, "known"), system(dim, "ladder6")
    (xa, _), (xb, _) = fresh[dim, "known"], fresh[dim, "ladder6"]
    assert xa.tobytes() != xb.tobytes(), "the two systems are meant to differ"
    stored = np.load(GOLDEN)
    pa, pb = stored["x_" + key(dim, "known")], stored["x_" + key(dim, "ladder6")]
    h = sr.Holders(hiplib, ctx)
    for c, want, parent, what in ((a, xa, pa, "first solve"), (b, xb, pb, "B behind A"), (a, xa, pa, "A behind B")):
        x, flag = h.alone(c)
        assert flag == 0 and x.tobytes() == want.tobytes(), (dim, what, "differs from a fresh problem")
        assert x.tobytes() == parent.tobytes(), (dim, what, "differs from the parent commit's bytes")
    h.close()


@pytest.mark.parametrize("dims", MIXED, ids=["-".join(str(d) for d in m) for m in MIXED])
def test_batches_of_mixed_length(holders, fresh, dims):
    for f in FAMILIES:
        xs, flags, wg_launches = holders.batch([system(d, f) for d in dims])
        assert wg_launches == 0, "a batch this small takes the panel-pair chain"
        for d, x, flag in zip(dims, xs, flags):
            assert flag == 0 and x.tobytes() == fresh[d, f][0].tobytes(), (d, f)
    # the shorter systems first, the longest first: the order in the batch does not matter
    xs, flags, _ = holders.batch([system(d, "known") for d in reversed(dims)])
    for d, x in zip(reversed(dims), xs):
        assert x.tobytes() == fresh[d, "known"][0].tobytes(), d


def _flag_then_clean(hiplib, ctx, holders, good, bad, where):
    (x_fresh, flag_fresh), = solve_fresh(hiplib, ctx, [good])
    assert flag_fresh == 0 and good["pd"] and not bad["pd"]
    xb, flag = holders.alone(bad)
    assert flag == 1, where
    assert np.isfinite(xb).all() and not xb.any(), "a flagged solve gives the zero step"
    x, flag = holders.alone(good)
    assert flag == 0 and x.tobytes() == x_fresh.tobytes(), where
    assert sr.row(good, x, sr.CHAIN)["e_dev"] <= sc.bound(good)


@pytest.mark.parametrize("n,p,where", NOTPD, ids=["%d-p%d" % (n, p) for n, p, _ in NOTPD])
def test_pivot_flag(hiplib, ctx, holders, n, p, where):
    good, bad = sc.notpd(n, p)
    assert sc.first_failing_pivot(bad["A"]) // NB == p // NB, "the failing pivot lies in the panel the case is about"
    _flag_then_clean(hiplib, ctx, holders, good, bad, where)


@pytest.mark.parametrize("n,p", ZERO_PIVOT)
def test_zero_pivot(hiplib, ctx, holders, n, p):
    _flag_then_clean(hiplib, ctx, holders, sc.ladder(n, 2), sc.zero_pivot(n, p), "zero pivot %d of %d" % (p, n))
