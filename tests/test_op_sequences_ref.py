"""CPU checks of tests/op_sequences.py: the model against routes that do not go through its rebuild, and what the generator must put into
the scripts tests/test_op_sequences_gpu.py runs (caps, not measurements: when one fails, the generator's weights change, not the condition)."""
from collections import Counter

import numpy as np
import pytest

import delete_ref as D
import helpers as H
import op_sequences as S

REF_SEEDS = [(so, S.PROFILES[k % 3], 100 + k) for so in (0, 1, 2) for k in range(14)][:40]       # 40 seeds across the three orders

_ran = {}


def ran(so, profile, seed):
    """(script, the null runner after it): each script is generated and run once"""
    key = (so, profile, seed)
    if key not in _ran:
        sc = S.script(seed, so, profile)
        _ran[key] = (sc, S.run(sc))
    return _ran[key]


def gpu_scripts():
    return [ran(*c) for c in S.gpu_cases()]


# ---- the model against an independent route ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so,profile,seed", REF_SEEDS)
def test_model_against_a_plain_list(so, profile, seed):
    sc, r = ran(so, profile, seed)
    assert r.steps == len(sc["ops"]) and 12 <= r.steps <= 16
    walked = sorted(w[::-1].tobytes() for w in r.m.walks())
    assert walked == sorted(s.tobytes() for s in r.plain)           # the multiset, in every order
    if so == 0:                                                     # input order: one oracle batch of the surviving strings in id order
        o = H.Oracle(0)
        if r.plain:
            o.insert_multi(H.encode_batch(r.plain, True, False))
        bwt = o.bwt()
        o.close()
        assert np.array_equal(bwt, r.m.bwt)
        assert all(np.array_equal(w[::-1], s) for w, s in zip(r.m.walks(), r.plain))


@pytest.mark.parametrize("so", [0, 1, 2])
def test_rebuild_is_the_incremental_oracle(so):
    """three batches one by one into the model, and into one oracle that keeps its state"""
    rng = np.random.RandomState(5 + so)
    m, o = S.Model(so), H.Oracle(so)
    for _ in range(3):
        buf = S.make_batch(S.batch_spec(rng), m.walks())
        delta = m.insert(buf)
        before = o.counts()
        o.insert_multi(buf)
        assert np.array_equal(o.bwt(), m.bwt) and np.array_equal(o.counts(), m.cnt) and np.array_equal(o.counts() - before, delta)
    o.close()
    ids = rng.choice(m.n, size=m.n // 3, replace=False)
    want, rows = D.delete(m.bwt, ids)
    assert m.delete(ids) == rows and np.array_equal(m.bwt, want)     # the rebuild from the survivors is the BWT minus the rows of the walks


def test_helpers():
    buf = H.encode_batch([[1, 2, 3], [], [4]], True, True)
    assert [s.tolist() for s in S.strings_of(buf)] == [[1, 2, 3], [2, 3, 4], [], [], [4], [1]]
    assert S.cut_at_sentinel(buf, 1) == 4 and S.cut_at_sentinel(buf, 5) == 8 and S.cut_at_sentinel(buf, len(buf)) == len(buf)
    other = S.other_content(buf)
    assert len(other) == len(buf) and np.array_equal(other == 0, buf == 0) and not np.array_equal(other, buf)
    assert S.Model(0).image().shape == (S.EMPTY_FMD,)


# ---- conditions on the generator, over the seeds the GPU test uses ----------------------------------------------------------------------

def test_every_operation_and_every_plan_occurs():
    kinds, plans = Counter(), Counter()
    for sc, _ in gpu_scripts():
        for op in sc["ops"]:
            kinds[op["op"]] += 1
            if op["op"] == "insert_prefetched":
                plans[op["plan"]] += 1
    assert all(kinds[k] >= 3 for k in S.KINDS), kinds
    assert all(plans[p] >= 1 for p in S.PLANS), plans


def test_every_script_changes_rows_under_a_valid_array():
    for sc, r in gpu_scripts():
        assert r.rows_changed_while_valid >= 1, S.show(sc)


def test_every_script_has_two_full_checks_around_a_row_change():
    for sc, r in gpu_scripts():
        assert any(a < c <= b for a, b in zip(r.fulls, r.fulls[1:]) for c in r.row_changes), S.show(sc)
        ops = sc["ops"]
        assert any(op["op"] == "ssa_build" and op.get("full") for op in ops) and any(op["op"] == "ssa_drop" and op.get("full") for op in ops), S.show(sc)
        assert ops[-1].get("full")


def test_deletes_are_followed_by_inserts():
    n = followed = 0
    for sc, _ in gpu_scripts():
        ops = sc["ops"]
        for i, op in enumerate(ops):
            if op["op"] == "delete":
                n += 1
                followed += int(i + 1 < len(ops) and ops[i + 1]["op"] in S.INSERTS)
    assert n >= 18 and 3 * followed >= n, (n, followed)


def test_an_insert_follows_reset_delete_all_and_a_load_in_every_order():
    for so in (0, 1, 2):
        seen = set()
        for sc, _ in gpu_scripts():
            if sc["so"] != so:
                continue
            r = S.Runner(dict(sc, ops=[]))
            ops = sc["ops"]
            for i, op in enumerate(ops):
                n = r.m.n
                r.step(op)
                if i + 1 < len(ops) and ops[i + 1]["op"] in S.INSERTS:
                    if op["op"] == "reset":
                        seen.add("reset")
                    elif op["op"] == "delete" and n and len(set(op["ids"])) == n:
                        seen.add("delete all")
                    elif op["op"] in ("load_ropes", "load_fmd", "save_then_load_self"):
                        seen.add("load")
        assert seen == {"reset", "delete all", "load"}, (so, seen)


def test_no_index_exceeds_the_cap():
    for sc, r in gpu_scripts():
        assert r.max_rows <= S.MAX_ROWS, (r.max_rows, S.show(sc))


def test_a_script_is_its_seed():
    a, b = S.script(7, 1, "sparse"), S.script(7, 1, "sparse")
    assert a == b and S.show(a) == S.show(b) and "insert" in S.show(a, 3)
