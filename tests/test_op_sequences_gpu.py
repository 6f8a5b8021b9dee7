"""Mixed operation sequences on one handle against the CPU model of tests/op_sequences.py: every way an rb2_hip_t changes its rows (host,
prefetched, registered and device inserts, delete, merge, the loaders, reset), with the host-side state that must follow them -- the sampled
suffix array and the remembered .fmd SIZE (index_rows_change), the host mirror of the ropes, the sparse flags, the steady / lean / forked
round state, the prefetch bookkeeping -- compared exactly after every step.

Random scripts come from op_sequences.script (what they contain is asserted on the CPU, tests/test_op_sequences_ref.py); a failure prints the
script as data and the step.  The pinned scripts below are written out by hand; each exists for one thing and asserts that it happened."""
import numpy as np
import pytest

import helpers as H
import merge_ref as MR
import op_sequences as S
import test_steady_round_gpu as ST
from test_lean_count_gpu import TAIL3
from test_merge_gpu import _long_reads
from test_query_gpu import _Env
from test_query_layouts_gpu import FORCED

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "sparse": FORCED, "dense": {"RB2_SPARSE_LAMBDA": "0"}}


def maker(hip, so, env):
    """the environment is read when a handle is created: it is set around that, as tools/fuzz_parity.py and check_job do"""
    def make():
        with _Env(**env):
            return hip.HipBwt(so)
    return make


def fixed(n, length, seed, both=0):
    return {"kind": "fixed", "seed": seed, "n": n, "both": both, "len": length, "dup": 0}


# ---- random scripts -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so,profile,seed", S.gpu_cases())
def test_random_script(hip, so, profile, seed):
    S.run(S.script(seed, so, profile), maker(hip, so, ENVS[profile]))


# ---- steady, lean and forked rounds behind a delete, a load, a merge and a reset ---------------------------------------------------------

def round_stats(g):
    return {"steady": g.steady_stats()["prep_skipped"], "lean": g.lean_stats()["rounds"], "forked": g.lean_fork_stats()["forked"],
            "verified": g.lean_count_stats()["verified"]}


def copies_of_indexed(r, seed, n_new=1100, n_old=300):
    """a batch in the manner of test_steady_round_gpu.with_a_duplicate: new reads of 24 symbols, one of them twice, and copies of strings the
    index holds, so that intervals stay non-empty to the last round"""
    rng = np.random.RandomState(seed)
    codes = H.splitmix_bases(n_new, 24, seed=seed)
    codes[n_new - 100] = codes[37]
    w = r.m.walks()
    reads = list(codes) + [w[i][::-1].copy() for i in rng.randint(0, len(w), size=n_old)]
    return H.encode_batch([reads[i] for i in rng.permutation(len(reads))])


@pytest.mark.parametrize("so,verify", [(1, False), (0, False), (1, True)])
def test_steady_after_everything(hip, so, verify):
    """Batches that go steady, lean and forked (1025 .. 1500 distinct reads, the shapes of test_steady_round_gpu.py) behind each of: a delete of
    a quarter of the strings, load_fmd, a merge, reset -- and behind every one of them a batch whose strings copy indexed ones.  RB2_TS_MAX=0 as in
    test_lean_fork_gpu.py: with so few tiles the counting tail is the one-launch form otherwise, which is never counted lean from A or forked.
    verify: every lean count is run both ways (RB2_LEAN_VERIFY=1; such rounds are never forked) and must not differ"""
    env = dict(ST.K1, **dict(ST.DENSE, **TAIL3))
    if verify:
        env.update(RB2_STEADY_LEAN="2", RB2_LEAN_VERIFY="1")
    lean_batches = [H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=300 + 1025)), H.encode_batch(ST.mixed_lengths()),
                    H.encode_batch_fixed(H.splitmix_bases(1500, 24, seed=91)), H.encode_batch_fixed(H.splitmix_bases(1301, 24, seed=92)),
                    H.encode_batch_fixed(H.splitmix_bases(1025, 24, seed=93))]
    sc = {"seed": 11, "so": so, "sides": [fixed(1200, 24, 61), fixed(1100, 24, 62)], "buffers": {"lean%d" % i: b for i, b in enumerate(lean_batches)}, "ops": []}
    r = S.Runner(sc, maker(hip, so, env))

    def step(op):
        sc["ops"].append(op)
        r.step(op)

    try:
        step({"op": "insert_host", "batch": "lean0", "lazy": 0})
        behind = [lambda: {"op": "delete", "ids": np.random.RandomState(3).choice(r.m.n, size=r.m.n // 4, replace=False).tolist()},
                  lambda: {"op": "load_fmd", "k": 0},
                  lambda: {"op": "merge_from", "k": 1, "batch_bytes": r.side(1).rows // 4},
                  lambda: {"op": "reset"}]
        for i, what in enumerate(behind):
            step(what())
            before = round_stats(r.g)
            step({"op": "insert_host", "batch": "lean%d" % (i + 1), "lazy": 0})
            after = round_stats(r.g)
            assert after["steady"] > before["steady"] and after["lean"] > before["lean"], (sc["ops"][-2]["op"], before, after)
            if verify:
                assert after["verified"] > before["verified"], (sc["ops"][-2]["op"], before, after)
            else:
                assert after["forked"] > before["forked"], (sc["ops"][-2]["op"], before, after)
            sc["buffers"]["dup%d" % i] = copies_of_indexed(r, 70 + i)
            step({"op": "insert_host", "batch": "dup%d" % i, "lazy": 0})
            sc["buffers"]["dup%db" % i] = copies_of_indexed(r, 80 + i, 1025, 200)
            step({"op": "insert_host", "batch": "dup%db" % i, "lazy": 1, "full": 1})
        cnt = r.g.lean_count_stats()
        assert cnt["mismatches"] == 0, cnt
        assert (cnt["verified"] > 0) == verify and (r.g.lean_fork_stats()["on"] == 1) == (not verify), (cnt, r.g.lean_fork_stats())
    finally:
        r.close()


# ---- a sparse index that is only asked, inserted into and merged into stays sparse ------------------------------------------------------

def test_sparse_stays_sparse(hip):
    so = 1
    bufs = {"mixed": H.encode_batch(MR.mixed_reads(150, 41)), "src": H.encode_batch(MR.mixed_reads(120, 42) + _long_reads(7, 8))}
    bufs.update({"long%d" % i: H.encode_batch(_long_reads(20 + i, 8)) for i in range(6)})
    sc = {"seed": 12, "so": so, "sides": ["src"], "buffers": bufs, "ops": []}
    r = S.Runner(sc, maker(hip, so, FORCED))

    def step(op, sparse=None):
        sc["ops"].append(op)
        r.step(op)
        if sparse is not None:
            assert r.g.layout_stats()["sparse_now"] is sparse, (op["op"], r.g.layout_stats())

    try:
        step({"op": "insert_host", "batch": "mixed", "lazy": 1})
        k = 0
        while not r.g.layout_stats()["sparse_now"]:
            assert k < 3, "three batches of long reads in place and the index is not sparse"
            step({"op": "insert_host", "batch": "long%d" % k, "lazy": 1})
            k += 1
        # the quiet stretch: nothing here may settle the index
        step({"op": "insert_dev", "batch": "long3", "misalign": 1}, sparse=True)
        step({"op": "ssa_build", "step": 3}, sparse=True)
        step({"op": "reserve", "bytes": 1 << 16, "strings": 100, "symbols": 0}, sparse=True)     # (its quiet checks are the queries, locate among them)
        step({"op": "insert_host", "batch": "long4", "lazy": 0}, sparse=True)
        step({"op": "delete", "ids": []}, sparse=True)                # (the quiet checks unpack; deleting nothing changes nothing)
        assert r.g.layout_stats()["sparse_rounds"] > 0
        src = r.source(0)
        assert src.layout_stats()["sparse_now"], "the source of the merge is not sparse"
        step({"op": "merge_from", "k": 0, "batch_bytes": r.side(0).rows // 4})
        assert src.layout_stats()["sparse_now"]
        step({"op": "insert_host", "batch": "long5", "lazy": 1})
        step({"op": "ssa_build", "step": 4}, sparse=True)
        step({"op": "settle"}, sparse=False)                          # valid and right behind the change of layout: step() compared locate with the model
        assert r.g.ssa_info()["valid"] and r.ssa
        step({"op": "delete", "ids": np.random.RandomState(4).choice(r.m.n, size=r.m.n // 3, replace=False).tolist(), "full": 1}, sparse=False)
    finally:
        r.close()


# ---- all ten prefetch plans in a row on one handle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("so,lazy,reg", [(0, 1, 0), (1, 0, 0), (2, 1, 1), (0, 0, 1)])
def test_prefetch_plans(hip, so, lazy, reg):
    rng = np.random.RandomState(40 + so)
    sc = {"seed": 13, "so": so, "sides": [S.batch_spec(rng, dup=False)], "ops": []}
    r = S.Runner(sc, maker(hip, so, {}))

    def step(op):
        sc["ops"].append(op)
        r.step(op)

    try:
        step({"op": "insert_host", "batch": S.batch_spec(rng, dup=False), "lazy": lazy})
        mids = [lambda: {"op": "delete", "ids": rng.choice(r.m.n, size=r.m.n // 3, replace=False).tolist()}, lambda: {"op": "load_fmd", "k": 0}, lambda: {"op": "reset"}]
        for plan in list(S.PLANS) + [10, 10]:
            op = {"op": "insert_prefetched", "batch": S.batch_spec(rng), "plan": plan, "lazy": lazy, "reg": reg}
            if plan in S.NEEDS_AUX:
                op["aux"] = S.batch_spec(rng)
                if plan == 6:
                    op["aux"]["n"] += 100
            if plan == 10:
                op["mid"] = mids.pop(0)()
            if plan in (5, 10):
                op["full"] = 1
            step(op)
        assert r.grown == 1 and r.steps == 13
        r.full_checks(r.steps)
    finally:
        r.close()


# ---- pieces of more than two superblocks each -------------------------------------------------------------------------------------------

def test_medium_pieces(hip):
    so = 2
    leaf = hip.HipBwt.layout()["leaf_syms"]
    bufs = {"first": H.encode_batch_fixed(H.splitmix_bases(7500, 100, seed=77), True, True), "more": H.encode_batch_fixed(H.splitmix_bases(700, 100, seed=78), True, True)}
    sc = {"seed": 14, "so": so, "sides": [], "buffers": bufs, "ops": []}
    r = S.Runner(sc, maker(hip, so, {}))

    def step(op):
        sc["ops"].append(op)
        r.step(op)
        assert leaf == 1024 and r.m.cnt[1:5, 1:5].min() > 2 * 32 * leaf, r.m.cnt     # every piece (b,x), b, x in A..T, exceeds two superblocks

    try:
        step({"op": "insert_host", "batch": "first", "lazy": 1})
        step({"op": "ssa_build", "step": 5})
        step({"op": "delete", "ids": np.flatnonzero(np.random.RandomState(1).rand(r.m.n) < 0.25).tolist(), "full": 1})
        step({"op": "insert_prefetched", "batch": "more", "plan": 2, "lazy": 1, "reg": 1})
        step({"op": "save_then_load_self", "full": 1})
        assert r.fulls == [2, 4] and r.row_changes == [0, 2, 3, 4]
    finally:
        r.close()


# ---- to the empty index and back ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 2])
def test_empty_and_back(hip, so):
    rng = np.random.RandomState(50 + so)
    sc = {"seed": 15, "so": so, "sides": [None], "ops": []}
    r = S.Runner(sc, maker(hip, so, {}))

    def step(op):
        sc["ops"].append(op)
        r.step(op)

    try:
        r.quiet_checks(99)                                          # 1. a fresh handle
        r.full_checks(99)                                           # 2. save_fmd
        assert r.old_size == S.EMPTY_FMD
        step({"op": "load_fmd", "k": 0})                            # 3. that image (the full check held it equal to the model's)
        step({"op": "insert_host", "batch": S.batch_spec(rng), "lazy": 1})                        # 4.
        step({"op": "delete", "ids": list(range(r.m.n))})           # 5.
        assert r.m.rows == 0
        step({"op": "ssa_build", "step": 2, "full": 1})             # 6. save_fmd: 216 bytes again, fetched with the SIZE of before
        assert r.old_size == S.EMPTY_FMD
        step({"op": "insert_dev", "batch": S.batch_spec(rng), "misalign": 0})                     # 7.
        step({"op": "reset"})                                       # 8.
        step({"op": "load_ropes", "k": 0})                          # 9. empty streams
        step({"op": "insert_prefetched", "batch": S.batch_spec(rng), "plan": 1, "lazy": 0, "reg": 0, "full": 1})   # 10.
        assert r.m.rows > 0
    finally:
        r.close()
