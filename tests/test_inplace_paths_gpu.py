"""In-place (sparse) rounds under every fallback knob of the engine, and void rounds taken back from deep behind queued rounds.

One engine queues in-place rounds without waiting for their verdict.  A void round (a leaf that cannot take its inserts) sets
ctl->overflow, every kernel queued behind it returns at once, and the host rewinds its own bookkeeping when it finds out
(insert_dev: descriptor / array parity, n_sparse_rounds, known_ae, the ne snapshot ring).  Every case here
compares the device index with the oracle -- count matrix after every batch, all six ropes -- and asserts through
layout_stats() / rewind_stats() that the path it is named for ran.

Fixtures (forced sparse: RB2_SPARSE_LAMBDA=1e18 RB2_SPARSE_MAXPEN=0):
  a  2000 x 120 bp, then 5000 identical strings: every in-place round of the second batch is void
  b  a, then 3000 x 150 bp; run under RB2_TS_MAX=2, so that the counting tail is k_tscan1-3 + k_tfix and k_setup rides on k_tfix
  c  long reads (1.5-2.6 kbp, runs of N, both strands) and short repetitive ones in three batches: leaf splits and re-spreads
  d  six fuzz jobs of one to three batches of 1-4000 strings (test_sparse_forced_fuzz's shapes, fixed seed)
String tiles (512 strings) per batch: a 4 and 10, c 1, d 1-8 -- counts that are no multiple of RB2_TS_BLOCKS = 2 or 3, and below it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

FORCED = dict(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0")
NE_RING = 32                                    # rb2_device.h NE_RING


class Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- fixtures: a list of jobs, each a list of batch buffers (one handle per job) ---------------------------------------

def _dups(n_sym):
    return ([1, 2, 3, 4] * (n_sym // 4 + 1))[:n_sym]


def fixture_a(dup_len=40):
    return [[H.encode_batch_fixed(H.splitmix_bases(2000, 120, seed=9)), H.encode_batch([_dups(dup_len)] * 5000)]]


def fixture_b(dup_len=40):
    return [fixture_a(dup_len)[0] + [H.encode_batch_fixed(H.splitmix_bases(3000, 150, seed=10))]]


def fixture_c():
    rng = np.random.RandomState(3)
    reads = []
    for _ in range(120):
        r = list(rng.randint(1, 5, size=int(rng.randint(1500, 2600))))
        for _ in range(int(rng.randint(0, 3))):                     # 0-2 runs of N per read
            at, n = int(rng.randint(0, len(r) - 1)), int(rng.randint(1, 300))
            r[at:at + n] = [5] * len(r[at:at + n])
        reads.append(np.array(r, np.uint8))
    reads += H.repetitive_reads(100, seed=71, max_len=40)
    return [[H.encode_batch(part, True, True) for part in (reads[:50], reads[50:100], reads[100:])]]


def fixture_d():
    rng = np.random.RandomState(4242)
    jobs = []
    for _ in range(6):
        batches = []
        for _ in range(int(rng.randint(1, 4))):
            n = int(rng.choice([1, 2, 63, 65, 300, 513, 1500, 4000]))
            pool = [list(rng.randint(1, 5, size=rng.randint(1, 30))) for _ in range(5)]
            reads = []
            for _ in range(n):
                L = int(rng.choice([0, 1, 5, 17, 40, 120]))
                r = (pool[rng.randint(5)] * 8)[:L] if rng.rand() < 0.3 else list(rng.randint(1, 5, size=L))
                reads.append([int(x) for x in r])
            batches.append(H.encode_batch(reads, True, rng.rand() < 0.25))
        jobs.append(batches)
    return jobs


FIXTURES = {"a": fixture_a, "b": fixture_b, "c": fixture_c, "d": fixture_d,
            "a101": lambda: fixture_a(101), "b101": lambda: fixture_b(101)}
_jobs, _want = {}, {}


def jobs_of(fx):
    if fx not in _jobs:
        _jobs[fx] = FIXTURES[fx]()
    return _jobs[fx]


def oracle_of(fx, so):
    """per job: (count matrix after every batch, the six ropes at the end) -- the oracle runs once per fixture and order"""
    if (fx, so) not in _want:
        out = []
        for job in jobs_of(fx):
            o = H.Oracle(so)
            cnt = []
            for buf in job:
                o.insert_multi(buf)
                cnt.append(o.counts().copy())
            out.append((cnt, o.ropes()))
            o.close()
        _want[(fx, so)] = out
    return _want[(fx, so)]


def run_dev(hip, fx, so, env):
    """every job of fixture fx on a fresh handle under env (kept set for the whole run: some knobs are read per round); compared
    with the oracle batch by batch; returns the summed layout / rewind statistics and the rope hashes of the last job"""
    want = oracle_of(fx, so)
    st, rw, hashes = {}, {"rewinds": 0, "rounds_taken_back": 0, "deepest": 0, "even_depth": 0}, None
    with Env(**env):
        for j, (job, (cnt, ropes)) in enumerate(zip(jobs_of(fx), want)):
            dev = hip.HipBwt(so)
            for i, buf in enumerate(job):
                dev.insert_multi(buf)
                assert np.array_equal(dev.counts(), cnt[i]), "%s so %d %s: count matrix after batch %d of job %d" % (fx, so, env, i, j)
            for b in range(6):
                got = dev.rope(b)
                assert len(got) == len(ropes[b]) and np.array_equal(got, ropes[b]), \
                    "%s so %d %s: rope %d of job %d differs at %s" % (fx, so, env, b, j, np.flatnonzero(got[:len(ropes[b])] != ropes[b][:len(got)])[:5])
            s, r = dev.layout_stats(), dev.rewind_stats()
            hashes = dev.rope_hashes()
            dev.close()
            for k, v in s.items():
                if k != "sparse_now":
                    st[k] = st.get(k, 0) + v
            for k in ("rewinds", "rounds_taken_back", "even_depth"):
                rw[k] += r[k]
            rw["deepest"] = max(rw["deepest"], r["deepest"])
    return st, rw, hashes


def check_rewinds_match_voids(st, rw, lazy, what):
    """one engine, lazy verdicts: every void round is found by the host after it queued rounds behind it and is taken back from
    there (insert_dev); with RB2_LAZY_VERDICT=0 the host waits for each verdict, nothing is ever queued behind a void round"""
    if lazy:
        assert rw["rewinds"] == st["void_rounds"], what
        assert rw["rounds_taken_back"] >= rw["rewinds"] and rw["deepest"] >= (1 if rw["rewinds"] else 0), what
    else:
        assert rw["rewinds"] == 0 and rw["rounds_taken_back"] == 0, what


# ---- 1. every fallback knob, every order, on the void / split / fuzz fixtures ------------------------------------------

KNOBS = {
    "lazy_verdict0": {"RB2_LAZY_VERDICT": "0"},
    "run_ahead1": {"RB2_RUN_AHEAD": "1"},
    "run_ahead2": {"RB2_RUN_AHEAD": "2"},
    "run_ahead64": {"RB2_RUN_AHEAD": "64"},             # (also case 3: default polling, deep run-ahead; the depth is only reported)
    "dir_ride0": {"RB2_DIR_RIDE": "0"},
    "ts_blocks1": {"RB2_TS_BLOCKS": "1"},
    "ts_blocks2": {"RB2_TS_BLOCKS": "2"},
    "ts_blocks3": {"RB2_TS_BLOCKS": "3"},
    "leaf_pipe0": {"RB2_LEAF_PIPE": "0"},               # one wave per four work orders (plain k_merge_leaf grid)
    "leaf_pipe4": {"RB2_LEAF_PIPE": "4"},               # 16 waves, one per work list: long grid-stride walks at test size
}


@pytest.mark.parametrize("fx", ["a", "b", "c", "d"])
@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_knob_matrix(hip, knob, so, fx):
    env = dict(FORCED, **KNOBS[knob])
    if fx == "b":
        env["RB2_TS_MAX"] = "2"
    st, rw, _ = run_dev(hip, fx, so, env)
    what = "%s so %d %s: %s %s" % (fx, so, knob, st, rw)
    assert st["sparse_rounds"] > 0, what
    check_rewinds_match_voids(st, rw, knob != "lazy_verdict0", what)
    if fx in ("a", "b"):
        assert st["void_rounds"] > 0, what
    if fx == "c":
        assert st["leaf_splits"] > 0 and st["respreads"] > 0, what


# ---- 2. deep rewinds: the host learns of a void round only when it drains (RB2_VERDICT_POLL=0) -----------------------------
# With the poll off the host queues every round up to the end of the batch behind a void one.  Void rounds come every other round
# (void, dense redo, one dense back-off round, retry), from round 0 in the first batch (120 symbols, while the index is small) and
# from round 8 in the second (behind the dense head of RB2_SPARSE_HEAD rounds), so the depth of a rewind has the parity of the
# batch's strings plus one: 120 and 101 symbols give both parities.  The first rewinds of each batch are 90-120 rounds deep.

@pytest.mark.parametrize("fx", ["a101", "b101"])
@pytest.mark.parametrize("ahead", [None, "64"])
@pytest.mark.parametrize("so", [0, 1, 2])
def test_deep_rewinds(hip, so, ahead, fx):
    env = dict(FORCED, RB2_VERDICT_POLL="0")
    if ahead:
        env["RB2_RUN_AHEAD"] = ahead
    if fx == "b101":
        env["RB2_TS_MAX"] = "2"
    st, rw, _ = run_dev(hip, fx, so, env)
    what = "%s so %d run-ahead %s: %s %s" % (fx, so, ahead, st, rw)
    assert st["void_rounds"] > 0 and st["sparse_rounds"] > 0, what
    check_rewinds_match_voids(st, rw, True, what)
    assert rw["deepest"] > NE_RING, what                             # the ne snapshot ring wrapped behind the void round
    assert rw["even_depth"] > 0, what                                # rewinds that keep the descriptor / array sides
    assert rw["rewinds"] - rw["even_depth"] > 0, what                # ... and rewinds that flip them back


@pytest.mark.parametrize("so", [0, 1, 2])
def test_widening_drain_finds_a_pending_void(hip, so):
    """RB2_POS_WIDEN_AT=12 widens the positions before round 12 of every batch; the drain in front of the widening finds the void
    round queued at 8 (or 0 in the first batch) and the host rewinds there, then widens when it comes to round 12 again"""
    env = dict(FORCED, RB2_VERDICT_POLL="0", RB2_POS_WIDEN_AT="12")
    st, rw, _ = run_dev(hip, "a101", so, env)
    what = "so %d: %s %s" % (so, st, rw)
    assert st["void_rounds"] > 0, what
    check_rewinds_match_voids(st, rw, True, what)


# ---- 4. the knobs together: the configuration of rounds 4-5 -------------------------------------------------------------

@pytest.mark.parametrize("so", [0, 1, 2])
def test_round4_knobs_combined_bit_identical(hip, so):
    old = dict(RB2_LAZY_VERDICT="0", RB2_DIR_RIDE="0", RB2_TS_BLOCKS="1", RB2_LEAF_PIPE="0")
    st0, rw0, h0 = run_dev(hip, "c", so, dict(FORCED))
    st1, rw1, h1 = run_dev(hip, "c", so, dict(FORCED, **old))
    what = "so %d: default %s %s / combined %s %s" % (so, st0, rw0, st1, rw1)
    assert h0 == h1, what
    assert st1["sparse_rounds"] > 0 and st1["leaf_splits"] > 0, what
    check_rewinds_match_voids(st1, rw1, False, what)


# ---- 5. pools that grow by hipMalloc + copy (RB2_NO_VMM=1, read once per process: a child of its own) -----------------------

_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import helpers as H
import test_inplace_paths_gpu as T
import ropebwt2_amd as R
out = {}
def check(tag, so, bufs, env):
    o = H.Oracle(so)
    with T.Env(**env):
        dev = R.HipBwt(so)
        for i, b in enumerate(bufs):
            o.insert_multi(b); dev.insert_multi(b)
            assert np.array_equal(dev.counts(), o.counts()), (tag, i)
    for b in range(6):
        assert np.array_equal(dev.rope(b), o.rope(b)), (tag, b)
    out[tag] = dev.layout_stats()
    dev.close(); o.close()
big = H.encode_batch_fixed(H.splitmix_bases(40000, 100, seed=21))
check("sparse", 1, T.fixture_c()[0] + [big], T.FORCED)                 # re-layouts size their target pools (grown, not copied)
check("dense", 2, [H.encode_batch_fixed(H.splitmix_bases(2000, 100, seed=20)), big], {})   # a dense batch grows its pool keeping the index (copy)
print("STATS " + json.dumps(out))
"""


def test_pools_grow_without_vmm(hip):
    here = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD % {"root": os.path.dirname(here), "tests": here}
    env = dict(os.environ, RB2_NO_VMM="1")
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-1500:])
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("STATS ")]
    assert line, p.stdout.decode()[-500:]
    st = json.loads(line[0][6:])
    assert st["sparse"]["relayouts"] >= 1 and st["sparse"]["sparse_rounds"] > 0, st
