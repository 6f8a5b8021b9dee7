"""GPU tests of the cold-path prefix scans (csrc/rb2_scan.h) on their own, through rb2_hip_scan_check / HipBwt.scan_check: every operation
in every form the engine instantiates, in place on the device, against a model on the host -- cumsum for the sums, a saturating cumsum
in Python ints for the sums that stop at 2^62, maximum.accumulate for the running maximum.  Everything is compared exactly: the items,
out[n], the separate total word and, in the three-launch form, the prefix of every block.  The sizes are those at which the code takes
another path: around a wave, a block of threads, a block of the scan (S items), and 256 S + 1 items, the smallest size at which the one
block that scans the blocks' totals takes a second turn."""
from itertools import accumulate

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SAT = 1 << 62
U64 = (1 << 64) - 1
MULTI_SIZES = ["0", "1", "63", "64", "65", "255", "256", "257", "S-1", "S", "S+1", "3*S+5", "256*S+1"]
BLOCK_SIZES = ["0", "1", "T-1", "T", "T+1", "3*T+5"]


@pytest.fixture(scope="module")
def g(hip):
    g = hip.HipBwt(0)
    yield g
    g.close()


def excl(op, x):
    """e[i] = the items in front of i taken together, i = 0 .. n (e[n]: all of them), whatever the op: Python ints or uint64"""
    if op == "sat":
        return [0] + list(accumulate(np.minimum(x, np.uint64(SAT)).tolist(), lambda a, b: min(a + b, SAT)))
    if op == "max":
        return np.concatenate([np.zeros(1, np.uint64), np.maximum.accumulate(x)]) if len(x) else np.zeros(1, np.uint64)
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(x, dtype=np.uint64)])


def check(g, op, form, x, what):
    x = np.asarray(x, np.uint64)
    n = len(x)
    out, parts, tot, per = g.scan_check(op, form, x)
    e = np.array(excl(op, x), np.uint64)
    want = e[1:] if op == "max" else e[:n]                         # the maximum is inclusive, the sums are exclusive
    bad = np.flatnonzero(out[:n] != want)
    assert len(bad) == 0, (op, form, n, what, "first wrong item", int(bad[0]), int(out[bad[0]]), int(want[bad[0]]))
    assert int(out[n]) == int(e[n]), (op, form, n, what, "out[n]", int(out[n]), int(e[n]))
    assert tot == int(e[n]), (op, form, n, what, "total", tot, int(e[n]))
    if form == "multi":
        assert len(parts) == (n + per - 1) // per
        assert np.array_equal(parts, e[0:n:per]), (op, n, what, "block prefixes")


def singles(n, places):
    """one item that is not zero, at each of the places inside the array"""
    for p in sorted(set(p for p in places if 0 <= p < n)):
        x = np.zeros(n, np.uint64)
        x[p] = 7
        yield x, "only item %d" % p


def common(rng, n, top, places):
    yield rng.integers(0, top, n, dtype=np.uint64), "random below %d" % top
    yield np.zeros(n, np.uint64), "zeros"
    yield from singles(n, places)


@pytest.fixture(scope="module")
def S(g):
    return g.scan_check("add64", "multi", [])[3]


@pytest.mark.parametrize("size", MULTI_SIZES)
@pytest.mark.parametrize("op", ["add32", "add64", "sat", "max"])
def test_three_launch_scan(g, S, op, size):
    n = eval(size, {"S": S})
    rng = np.random.default_rng(n + 1)
    per = S // 256                                                 # items of a thread, side by side
    edges = [0, n - 1, 63, 64, 256, S - 1, S] if n <= 3 * S + 5 else [0, n - 1, 256 * S - 1, 256 * S]
    # add32: totals below 2^32 (2^20 items below 1000); add64 and sat: carries out of the low word; max: values that need all 64 bits
    top = {"add32": 1000, "add64": 1 << 40, "sat": 1 << 40, "max": 1 << 63}[op]
    for x, what in common(rng, n, top, edges):
        check(g, op, "multi", x, what)
    if op == "sat":
        # the cap is first reached at item b, in front of which a makes the sum 2^62 - 2: inside the items of one thread, in another lane of
        # the wave, in another wave, in another block (the top kernel), in another turn of the top kernel; small items everywhere else
        scopes = {"thread": (3, 5), "lanes": (3, 5 * per + 2), "waves": (3, 2 * 64 * per + 7), "blocks": (3, 2 * S + 3), "turns": (3, 256 * S)}
        bigs = [1, SAT - 1, SAT, 1 << 63, U64]                     # (1: the sum is exactly 2^62 - 1 behind b and reaches the cap at the next 1)
        if n > 3 * S + 5:
            scopes = {k: scopes[k] for k in ("blocks", "turns")}   # (the others are the business of the smaller sizes)
            bigs = [SAT - 1, U64]
        for name, (a, b) in scopes.items():
            for big in bigs:
                if b >= n:
                    continue
                x = rng.integers(0, 2, n, dtype=np.uint64)
                x[:b] = 0
                x[a], x[b] = SAT - 2, big
                check(g, op, "multi", x, "cap across %s, item %d = %d" % (name, b, big))
        if n > 0:
            x = np.full(n, U64, np.uint64)                             # every item counts as 2^62
            check(g, op, "multi", x, "all 2^64 - 1")
    if op == "max" and n > 0:
        for p, where in ((min(5, n - 1), "first"), (n - 1 - min(3, n - 1), "last")):
            x = rng.integers(0, 1 << 40, n, dtype=np.uint64)       # not monotone
            x[p] = U64 if where == "first" else 1 << 50
            check(g, op, "multi", x, "maximum in the %s block" % where)


@pytest.mark.parametrize("size", BLOCK_SIZES)
@pytest.mark.parametrize("form", ["block256", "block1024"])
def test_one_block_scan(g, form, size):
    T = g.scan_check("add64", form, [])[3]
    assert T == int(form[5:])
    n = eval(size, {"T": T})
    rng = np.random.default_rng(n + 2)
    for x, what in common(rng, n, 1 << 40, [0, n - 1, 63, 64, T - 1, T, 3 * T]):
        check(g, "add64", form, x, what)
