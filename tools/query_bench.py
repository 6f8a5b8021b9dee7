"""Throughput of the FM-index query kernels (k_bsearch, k_extend, k_extract; csrc/rb2_query.h) on a configs[1]-sized index.

Builds the first configs[1] batch on the device (40.8 M x 101 bp synthetic reads, RLO by default, the generator of
tests/test_hip_parity.py::test_full_batch_properties), then times, after a warm-up, with a host clock around a synchronise:
  - backward_search_dev on P patterns of length 20, 32 and 64: substrings of the reads (hits) and uniform random patterns (mostly misses);
  - extend (host variant) on P bi-intervals;
  - extract (host variant) on R rows;
  - the baseline: the same backward search composed from rb2_hip_rank_batch calls (what a user could do before), on fewer patterns;
  - smem (--only smem, or after the others): smem_dev on P reads of 101 bp with 2 % substituted bases against an index of the same reads
    built with BOTH strands, and its baseline, the same algorithm driven from the host with one rb2_hip_extend call per step for a
    sample of the queries in lock step (composed_smem), reported per query.
For each case: queries/s, LF steps/s (one step = the ranks at both ends of an interval, or one LF of a walk), the bytes a step touches
by the layout, and steps/s x bytes against the 8 TB/s HBM peak.  One JSON document on stdout and in --out.

    python tools/query_bench.py --out profiles/query_bench.json [--so 1] [--patterns 4000000] [--rows 1000000] [--only smem] [--fmd PATH]
With --fmd the index is not built but loaded from an .fmd file (rb2_hip_load_fmd, from a file image in host memory): the document then
records the load -- file bytes, seconds (first load and the median of three more), GB of file per second -- and the smem cases, which
need an index of their own reads, are left out.  "hits" are then hits only if the file holds the reads of the generator.
With --only smem and an --out file that exists, the smem cases replace those of the file and the rest of it stays.
With --locate only the sampled suffix array is measured, on the index of the first cases (single strand), and stored under "locate" in
the --out file, whose other entries stay: rb2_hip_ssa_build at log2_step 3, 5 and 7 (seconds, LF steps per second -- one step per row of
the index --, bytes held), and at each step locate_dev for the intervals of P substring patterns of length 20 and 64 with max_hits 16
(hits per second).
With --overlap only the suffix-prefix overlap query is measured and stored under "overlap" in the --out file, whose other entries stay:
on the index of the first cases (single strand), overlap_dev on P whole reads of the index at min_ovlp 1 and 20 (queries, LF steps --
one per rank pair -- and records per second, with the fastest and slowest of the three runs) and backward_search_dev on the same reads
in the same run; then, on an index of both strands, the baseline a user could compose before: every suffix of a read a pattern of its
own, count(revcomp(suffix) + $) through rb2_hip_backward_search, against rb2_hip_overlap on the same few thousand reads.
With --delete FRACTION only string deletion is measured and appended to "delete" in the --out file, whose other entries stay: on the
index of the first cases, rb2_hip_delete_strings of a seeded random FRACTION of the strings -- seconds of the call (host clock: it returns
when the new index is in place), pool bytes read plus written per second (the leaves read and the leaves written once each, and all the
traffic of the passes: the planes read twice, the marks, the zeroed destination), and the share of the source groups that took the fast
path (a shift, no compress).  The same run times what a user could do before: rb2_hip_reset, then one insert of the survivors, whose
text is put on the device outside the timed region.  In input order (--so 0) the survivors are the same strings and the two indexes are
compared by their checksums; in the other orders an id is no read number, so the rebuild takes a random subset of the reads of the same size.
With --contained only the duplicate / containment query is measured and appended to "contained" in the --out file, whose other entries
stay: contained_dev over every string of the default index (unique reads) and of an index of reads drawn from one genome at 30x (equal
start positions give real copies), with the early exit and with RB2_CONTAIN_EARLY=0 -- strings and LF steps per second, the mean steps
per string and the share of every flag.  On a sample of the strings the same run times rb2_hip_contained through host buffers against what
a user could compose before, rb2_hip_extract of the sample followed by rb2_hip_backward_search of the extracted strings, and compares
the occurrences the two report.
With --irreducible only the irreducible-overlap query is measured and stored under "irreducible" in the --out file, whose other entries
stay: an index of both strands of reads drawn from one genome at 30x, in input order, after reduce(pairs=True); irreducible_dev over
--irreducible-queries reads of the index (their text read back with extract) at --irreducible-min-ovlp, max_ext = read length - min_ovlp
-- queries per second, median of three after a warm-up with the fastest and the slowest beside it, rank pairs per second from a lower
bound of the steps (the call does not report the steps of a query: the search takes one per symbol, every entry of the root one, and
a record of extension e at least e more), records per query and the share of the overlap records of the same reads (rb2_hip_overlap,
lengths below the read's own) that survive.  On 4000 reads the same run times what a user could compose before -- overlaps(), extract of
every neighbour, and the pruning on the host (tests/irreducible_ref.py: edges_by_composition) -- against irreducible(pairs=True), and
compares the edge sets (equals_fused).
With --unitigs only the unitig calls are measured and stored under "unitigs" in the --out file, whose other entries stay: the index of
--irreducible (both strands of reads drawn from one genome at 30x, input order, after reduce(pairs=True); --reads, default 1 000 000);
its edges come from rb2_hip_irreducible over every string and rb2_hip_string_ids, put together with numpy (not timed: HipBwt.edges
walks Python lists).  unitig_chains_dev and unitig_text_dev (canonical, caps from a sizing call that is timed by itself) are timed
separately -- host clock round a synchronise, median of three after a warm-up -- and reported with the chains, the longest chain, the
doublings queued, the total text and the LF steps per second (one step per symbol written).  The composition it replaces is timed on a
sample the host can follow: the first --unitig-sample vertices of the longest chain and the edges among them -- the Python chain walk
of tests/unitig_ref.py (chains) plus extract() of every read of the sample and the gluing of texts() -- against unitig_chains and
unitig_text (host buffers, min_reads=2) on the same edges; the texts are compared (equals_fused).
With --graph only rb2_hip_string_graph is measured and stored under "string_graph" in the --out file, whose other entries stay: the index of
--unitigs (--reads, default 1 000 000) with its suffix array; (a) string_graph_dev over every string -- sources and edges per second, median
of three after a warm-up with the fastest and the slowest beside it; (b) HipBwt.edges() on the first --unitig-sample strings against
string_graph on the same strings (host buffers; the rows are compared: equals_fused); (c) irreducible_dev alone on the same strings, their
texts already on the device, against string_graph_dev measured next to it: what unpacking, counting, scanning and emitting cost on top.
With --clean only rb2_hip_graph_clean_dev is measured and stored under "clean" in the --out file, whose other entries stay: a synthetic edge
list that needs no index (tests/graph_clean_ref.py backbone: both strands of --reads reads, default 1 000 000, a one-read tip every 50 reads
and a one-read bubble every 70), the call's seconds (median of three after a warm-up) and seconds per round, and unitig_chains_dev on the
same list, which every round contains (clean_case).
With --merge only rb2_hip_unpack_dev and rb2_hip_merge are measured and stored under "merge" in the --out file, whose other entries stay:
symbols per second of unpack_dev in both directions against rb2_hip_extract of the same strings (max_len = the read length), and the merge
of an index of a quarter as many other reads into the benchmark index against extract + a host pass + rb2_hip_insert_multi from the host
buffer into an identical index (merge_case).
With --approx-ed only the approximate search with insertions and deletions is measured and stored under "approx_ed" in the --out file, whose
other entries stay: on the index of the first cases, --approx-ed-queries reads of the index with 0, 1 and 2 planted edits -- one substitution,
one deleted base, one inserted base in turn, never at the two end positions -- through approx_ed_dev at max_ed = planted (--approx-steps is
its max_steps), queries per second, median of three after a warm-up with the fastest and the slowest run beside it.  Next to each the same
reads with as many planted substitutions through approx_dev at max_mm = planted: what a step cost before the column.
With --correct only the read correction is measured and stored under "correct" in the --out file, whose other entries stay: on the index of
the first cases (single strand, unique reads: min_occ = 1), correct_dev on --correct-reads reads of the index with 0, 1 and 2 planted
substitutions in turn (k = --correct-k, max_fix 8, the default max_probes) -- reads per second, median of three after a warm-up with the
fastest and the slowest beside it, probes per second from a lower bound (the call does not report the probes of a read: L - k + 1 for its
profile), the reads restored.  The baseline is what could be composed before: the profile alone, count() on the host-sliced k-mers of
--correct-sample of the same reads, which must name the same reads as untouched (no weak position <=> cnt == 0 and weak == 0: equals_fused).
Then correct_into of the whole index into an empty one, timed the same way (the destination reset outside the timed region).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ropebwt2_amd import HipBwt  # noqa: E402
from ropebwt2_amd.hipbwt import pack_patterns  # noqa: E402
import helpers as H  # noqa: E402

HBM_PEAK = 8.0e12
LEAF_BYTES, META_BYTES, SB_BYTES = 384, 16, 32      # per rank: three leaf lines, the LeafMeta, the SbRec (the SbBase records stay in cache)
RANK_BYTES = LEAF_BYTES + META_BYTES + SB_BYTES


def timed(fn, sync, reps=3):
    fn(); sync()                                     # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def hit_patterns(n, L, n_reads, seed):
    rng = np.random.RandomState(seed)
    pool_reads = min(n_reads, 200_000)
    reads = H.splitmix_bases(pool_reads, 101, seed=42)
    out = np.empty((n, L), np.uint8)
    for i0 in range(0, n, 250_000):                  # (chunks: the index arrays are 8 bytes per symbol)
        k = min(250_000, n - i0)
        ri = rng.randint(0, pool_reads, size=k)
        st = rng.randint(0, 101 - L + 1, size=k)
        out[i0:i0 + k] = reads[ri[:, None], st[:, None] + np.arange(L)[None, :]]
    return out


def row_case(name, n, sec, steps, rank_per_step):
    bps = RANK_BYTES * rank_per_step
    return {"case": name, "queries": int(n), "seconds": sec, "queries_per_s": n / sec, "lf_steps": int(steps), "lf_steps_per_s": steps / sec,
            "bytes_per_step": bps, "touched_bytes_per_s": steps / sec * bps, "fraction_of_hbm_peak": steps / sec * bps / HBM_PEAK}


def composed_search(g, counts, pats):
    """backward search through rb2_hip_rank_batch: per step, the rows of both ends go to their ropes, six rank_batch calls"""
    C = np.concatenate([[0], np.cumsum(counts.sum(1))[:5]]).astype(np.int64)     # rows in front of each rope
    rope_end = np.concatenate([C[1:], [counts.sum()]])
    before = np.zeros((6, 6), np.int64)                                            # symbols of the ropes in front of rope b
    before[1:] = np.cumsum(counts, 0)[:5]
    n, L = pats.shape
    lo = np.zeros(n, np.int64); hi = np.full(n, int(counts.sum()), np.int64); m = np.zeros(n, np.int64); live = np.ones(n, bool)
    for j in range(L - 1, -1, -1):
        idx = np.flatnonzero(live)
        if len(idx) == 0:
            break
        c = pats[idx, j].astype(np.int64)
        x = np.concatenate([lo[idx], hi[idx]]); cc = np.concatenate([c, c])
        b = np.minimum(np.searchsorted(rope_end, x, side="right"), 5)
        occ = np.zeros(len(x), np.int64)
        for r in range(6):
            k = np.flatnonzero(b == r)
            if len(k):
                rk = g.rank_batch(r, x[k] - C[r])
                occ[k] = before[r, cc[k]] + rk[np.arange(len(k)), cc[k]]
        nl, nh = C[c] + occ[:len(idx)], C[c] + occ[len(idx):]
        ok = nl < nh
        lo[idx[ok]] = nl[ok]; hi[idx[ok]] = nh[ok]; m[idx[ok]] += 1
        live[idx[~ok]] = False
    return lo, hi, m


def composed_smem(g, counts, qs, min_len=1, min_occ=1):
    """k_smem's algorithm driven from the host for all the queries qs (n, L) in lock step: per step ONE rb2_hip_extend call for the
    queries that have a step to take.  The state of a query is (xf, xo, sz) with xf the end the next step ranks, so every step is a
    backward extension of (xf, xo, sz) whichever way the query is going.  Returns the records per query, the steps and the calls."""
    n, L = qs.shape
    C = np.concatenate([[0], np.cumsum(counts.sum(1))]).astype(np.int64)
    idx = np.arange(n)
    p = np.zeros(n, np.int64); s = np.zeros(n, np.int64); e = np.zeros(n, np.int64)
    st = np.zeros((n, 3), np.int64)
    back = np.zeros(n, bool); walking = np.zeros(n, bool)
    recs = [[] for _ in range(n)]
    steps = calls = 0
    while True:
        fresh = np.flatnonzero(~walking & (p < L))                    # start from the bi-interval of q[p], or skip p
        if len(fresh) == 0 and not walking.any():
            break
        if len(fresh):
            c0 = qs[fresh, p[fresh]].astype(np.int64)
            ok = c0 < 5
            cc = np.where(ok, c0, 0)
            sz = np.where(ok, C[cc + 1] - C[cc], 0)
            go = sz >= min_occ
            p[fresh[~go]] += 1
            f = fresh[go]
            st[f, 0] = C[cc[go]]; st[f, 1] = C[5 - cc[go]]; st[f, 2] = sz[go]
            s[f] = p[f]; e[f] = p[f] + 1; back[f] = True; walking[f] = True
        w = np.flatnonzero(walking)
        if len(w) == 0:
            continue
        j = np.where(back[w], s[w] - 1, e[w])
        inside = (j >= 0) & (j < L)
        c = np.where(inside, qs[w, np.clip(j, 0, L - 1)], 0).astype(np.int64)
        stop = (c < 1) | (c > 4)
        k = np.flatnonzero(~stop)
        if len(k):
            a = np.where(back[w[k]], c[k], 5 - c[k])
            ok6 = g.extend(st[w[k]], 1)
            calls += 1; steps += len(k)
            nx = ok6[np.arange(len(k)), a]
            good = nx[:, 2] >= min_occ
            stop[k[~good]] = True
            wk = w[k[good]]
            st[wk] = nx[good]
            bk = back[wk]
            s[wk[bk]] -= 1; e[wk[~bk]] += 1
        ws = w[stop]
        turn = ws[back[ws]]
        st[turn, 0], st[turn, 1] = st[turn, 1].copy(), st[turn, 0].copy()
        done = ws[~back[ws]]
        back[turn] = False
        for i in done:
            if e[i] - s[i] >= min_len:
                recs[i].append([s[i], e[i], st[i, 1], st[i, 0], st[i, 2]])
        p[done] = e[done]; walking[done] = False
    return recs, steps, calls


def smem_steps(qs, mem, cnt):
    """extension steps k_smem took (min_len = 1, min_occ = 1, no N, every symbol present in the index), from its records: for an SMEM
    [s, e) found from position p (the end of the one before): p - s backward steps and one that failed unless s == 0, e - p - 1 forward
    steps and one that failed unless e == L"""
    n, L = qs.shape
    k = np.arange(mem.shape[1])[None, :] < cnt[:, None]
    s, e = mem[:, :, 0], mem[:, :, 1]
    p = np.concatenate([np.zeros((n, 1), np.int64), e[:, :-1]], 1)
    return int(((e - s - 1 + (s > 0) + (e < L)) * k).sum()), p


def smem_case(a, res):
    L = 101
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    g = HipBwt(a.so)
    buf = g.dev_alloc(2 * n * (L + 1))
    t = time.perf_counter()
    g.synth_reads(buf, 0, n, L, seed=42, strand=1)                  # every read followed by its reverse complement
    g.insert_multi_dev(buf, 2 * n * (L + 1))
    g.sync()
    counts = g.counts()
    build_s = time.perf_counter() - t
    g.dev_free(buf)
    print("smem: index of %d reads x 2 strands built in %.1f s" % (n, build_s), file=sys.stderr, flush=True)
    P, M = a.patterns, 16
    rng = np.random.RandomState(11)
    qs = hit_patterns(P, L, n, 101)
    sub = rng.rand(P, L) < 0.02                                     # 2 % substitutions: another base, never the same
    qs[sub] = 1 + (qs[sub] - 1 + rng.randint(1, 4, size=int(sub.sum()))) % 4
    flat = np.ascontiguousarray(qs.reshape(-1)); off = np.arange(P + 1, dtype=np.int64) * L
    dq, do, dm, dc = g.dev_alloc(len(flat)), g.dev_alloc(8 * (P + 1)), g.dev_alloc(40 * M * P), g.dev_alloc(8 * P)
    g.L.rb2_hip_memcpy(g.h, dq, flat.ctypes.data, len(flat), 0)
    g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
    sec = timed(lambda: g.smem_dev(P, dq, do, dm, dc, 1, 1, M), g.sync)
    mem = np.zeros((P, M, 5), np.int64); cnt = np.zeros(P, np.int64)
    g.L.rb2_hip_memcpy(g.h, mem.ctypes.data, dm, mem.nbytes, 1)
    g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, dc, 8 * P, 1)
    for q in (dq, do, dm, dc):
        g.dev_free(q)
    assert cnt.min() >= 0, int(cnt.min())
    trunc = int((cnt > M).sum())
    print("smem: %d queries in %.3f s" % (P, sec), file=sys.stderr, flush=True)
    # the steps are counted from the records, so they need all of them: a sample of the queries again with room for every SMEM
    ns, M2 = min(P, a.step_queries), 128
    st2, mem2, cnt2 = g.smem_raw(list(qs[:ns]), 1, 1, M2)
    assert np.array_equal(cnt2, cnt[:ns]) and cnt2.max() <= M2, int(cnt2.max())
    assert all(np.array_equal(mem2[i, :min(cnt2[i], M)], mem[i, :min(cnt2[i], M)]) for i in range(0, ns, 97))
    steps_s, _ = smem_steps(qs[:ns], mem2, cnt2)
    steps = int(round(steps_s / ns * P))
    row = row_case("smem_dev 101 bp reads, 2 %% substitutions, min_len=1 min_occ=1 max_mems=%d (both strands indexed)" % M, P, sec, steps, 2)
    row.update({"measured": True, "lf_steps_counted_on_queries": ns, "lf_steps_are": "counted on the first %d queries, scaled to %d" % (ns, P),
                "queries_with_more_than_max_mems": trunc, "smems": int(cnt.sum()), "smems_per_query": float(cnt.mean()),
                "mean_smem_length": float((mem2[:, :, 1] - mem2[:, :, 0]).sum() / max(cnt2.sum(), 1)),
                "index": {"reads": n, "strands": 2, "symbols": int(counts.sum()), "build_seconds": build_s, "layout": g.layout_stats()}})
    nb = min(a.baseline_queries, ns)
    t = time.perf_counter()
    recs, bsteps, calls = composed_smem(g, counts, qs[:nb])
    bsec = time.perf_counter() - t
    same = all(len(r) == cnt2[i] and np.array_equal(np.array(r, np.int64).reshape(-1, 5), mem2[i, :cnt2[i]]) for i, r in enumerate(recs))
    fsteps, _ = smem_steps(qs[:nb], mem2[:nb], cnt2[:nb])
    brow = row_case("baseline: the same SMEM algorithm driven from the host, one rb2_hip_extend call per step, %d queries in lock step" % nb, nb, bsec, bsteps, 2)
    brow.update({"measured": True, "extend_calls": calls, "equals_fused": bool(same), "steps_equal_fused_count": bool(bsteps == fsteps), "seconds_per_query": bsec / nb})
    host = timed(lambda: g.smem_raw(list(qs[:nb]), 1, 1, M), lambda: None, reps=1)
    hrow = row_case("smem (host buffers), the baseline's %d queries" % nb, nb, host, fsteps, 2)
    hrow["measured"] = True
    g.close()
    res["cases"] = [c for c in res["cases"] if "smem" not in c["case"].lower()] + [row, brow, hrow]


def locate_case(a, res):
    L = 101
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    g.dev_free(p)
    N = int(g.counts().sum())
    P, M = a.patterns, 16
    ivs = {}
    for Lp in (20, 64):                                              # the intervals of substrings of the reads, kept on the device
        pats = hit_patterns(P, Lp, n, Lp)
        flat = np.ascontiguousarray(pats.reshape(-1)); off = np.arange(P + 1, dtype=np.int64) * Lp
        dp, do, dq = g.dev_alloc(len(flat)), g.dev_alloc(8 * (P + 1)), g.dev_alloc(24 * P)
        g.L.rb2_hip_memcpy(g.h, dp, flat.ctypes.data, len(flat), 0)
        g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
        g.backward_search_dev(P, dp, do, dq)
        out = np.zeros((P, 3), np.int64)
        g.L.rb2_hip_memcpy(g.h, out.ctypes.data, dq, 24 * P, 1)
        for q in (dp, do, dq):
            g.dev_free(q)
        assert (out[:, 2] == Lp).all()
        ivs[Lp] = np.ascontiguousarray(out[:, :2])
    d_iv, d_hit, d_cnt = g.dev_alloc(16 * P), g.dev_alloc(16 * M * P), g.dev_alloc(8 * P)
    rows = []
    for s in (3, 5, 7):
        sec = timed(lambda: g.build_ssa(s), lambda: None)           # (rb2_hip_ssa_build synchronises before it returns)
        inf = g.ssa_info()
        row = {"case": "ssa_build log2_step=%d" % s, "seconds": sec, "lf_steps": N, "lf_steps_per_s": N / sec, "samples": inf["samples"],
               "device_bytes": inf["device_bytes"], "bytes_per_row": inf["device_bytes"] / N, "measured": True, "locate": []}
        print("locate: built step %d in %.3f s" % (s, sec), file=sys.stderr, flush=True)
        for Lp in (20, 64):
            g.L.rb2_hip_memcpy(g.h, d_iv, ivs[Lp].ctypes.data, 16 * P, 0)
            lsec = timed(lambda: g.locate_dev(P, d_iv, d_hit, d_cnt, M), g.sync)
            cnt = np.zeros(P, np.int64)
            g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, d_cnt, 8 * P, 1)
            assert np.array_equal(cnt, ivs[Lp][:, 1] - ivs[Lp][:, 0])
            hits = int(np.minimum(cnt, M).sum())
            row["locate"].append({"case": "locate_dev, intervals of %d substrings of length %d, max_hits=%d" % (P, Lp, M), "intervals": P, "slots": P * M,
                                  "hits": hits, "intervals_with_more_than_max_hits": int((cnt > M).sum()), "seconds": lsec, "hits_per_s": hits / lsec,
                                  "intervals_per_s": P / lsec, "measured": True})
        rows.append(row)
    for q in (d_iv, d_hit, d_cnt):
        g.dev_free(q)
    res["locate"] = {"index": {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": N, "strands": 1, "layout": g.layout_stats()}, "cases": rows}
    g.close()


def spread(fn, sync, reps=3):
    """timed(), with the fastest and the slowest run beside the median"""
    fn(); sync()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def overlap_case(a, res):
    L, M = 101, 24
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    P = a.patterns
    qs = hit_patterns(P, L, n, 101)                                 # whole reads of the index
    flat = np.ascontiguousarray(qs.reshape(-1)); off = np.arange(P + 1, dtype=np.int64) * L
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    g.dev_free(p)
    N = int(g.counts().sum())
    dq, do, dr, dc, db = g.dev_alloc(len(flat)), g.dev_alloc(8 * (P + 1)), g.dev_alloc(24 * M * P), g.dev_alloc(8 * P), g.dev_alloc(24 * P)
    g.L.rb2_hip_memcpy(g.h, dq, flat.ctypes.data, len(flat), 0)
    g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
    rows = []

    def bsearch():
        sec, lo, hi = spread(lambda: g.backward_search_dev(P, dq, do, db), g.sync)
        out = np.zeros((P, 3), np.int64)
        g.L.rb2_hip_memcpy(g.h, out.ctypes.data, db, 24 * P, 1)
        assert (out[:, 2] == L).all()                               # reads of the index: every step succeeds, L rank pairs each
        row = row_case("backward_search_dev on the same %d reads" % P, P, sec, P * L, 2)
        row.update({"measured": True, "lf_steps_per_s_slowest": P * L / hi, "lf_steps_per_s_fastest": P * L / lo})
        return row
    rows.append(bsearch())
    for min_ovlp in (1, 20):
        sec, lo, hi = spread(lambda: g.overlap_dev(P, dq, do, dr, dc, min_ovlp, M), g.sync)
        cnt = np.zeros(P, np.int64)
        g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, dc, 8 * P, 1)
        assert cnt.min() >= 1                                       # a read of the index finds itself
        recs = int(cnt.sum())
        row = row_case("overlap_dev, %d reads of the index (101 bp), min_ovlp=%d max_recs=%d" % (P, min_ovlp, M), P, sec, P * L, 2)
        row.update({"measured": True, "lf_steps_are": "rank pairs: one per symbol of a read, every suffix of which occurs", "lf_steps_per_s_slowest": P * L / hi,
                    "lf_steps_per_s_fastest": P * L / lo, "records": recs, "records_per_s": recs / sec, "records_per_query": recs / P,
                    "queries_with_more_than_max_recs": int((cnt > M).sum())})
        rows.append(row)
        print("overlap: min_ovlp %d: %d queries in %.3f s" % (min_ovlp, P, sec), file=sys.stderr, flush=True)
    rows.append(bsearch())                                          # once more behind the overlap runs: the drift of the run itself
    rows[-1]["case"] += " (again, after the overlap runs)"
    for q in (dq, do, dr, dc, db):
        g.dev_free(q)
    index = {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": N, "strands": 1, "layout": g.layout_stats()}
    g.close()
    # the baseline needs the strings that END in a pattern: on an index of both strands those are the strings that start with its reverse complement
    g = HipBwt(a.so)
    buf = g.dev_alloc(2 * n * (L + 1))
    g.synth_reads(buf, 0, n, L, seed=42, strand=1)
    g.insert_multi_dev(buf, 2 * n * (L + 1))
    g.sync()
    g.dev_free(buf)
    nb, min_ovlp = min(a.baseline_queries // 5, P), 20                # (4000 reads by default: 82 patterns each)
    comp = np.array([0, 4, 3, 2, 1, 5], np.uint8)
    pats = [np.concatenate([comp[q[L - l:][::-1]], [0]]).astype(np.uint8) for q in qs[:nb] for l in range(min_ovlp, L + 1)]
    pat, poff = pack_patterns(pats)
    out = np.zeros((len(pats), 3), np.int64)
    bsec = timed(lambda: g.L.rb2_hip_backward_search(g.h, len(pats), pat.ctypes.data, poff.ctypes.data, out.ctypes.data), lambda: None)
    lens = np.diff(poff)
    ends = np.where(out[:, 2] == lens, out[:, 1] - out[:, 0], 0).reshape(nb, L - min_ovlp + 1)
    got = [None]

    def fused():
        got[0] = g.overlap_raw(list(qs[:nb]), min_ovlp, L - min_ovlp + 1)
    fsec = timed(fused, lambda: None)
    _, rec, cnt = got[0]
    mine = np.zeros_like(ends)
    k = np.arange(rec.shape[1])[None, :] < cnt[:, None]
    mine[np.nonzero(k)[0], rec[:, :, 0][k] - min_ovlp] = (rec[:, :, 2] - rec[:, :, 1])[k]
    brow = row_case("baseline: one pattern per suffix, count(revcomp(suffix) + $) through rb2_hip_backward_search (host buffers), %d reads, min_ovlp=%d, both strands indexed"
                    % (nb, min_ovlp), nb, bsec, int(np.minimum(out[:, 2] + 1, lens).sum()), 2)
    brow.update({"measured": True, "patterns": len(pats), "pattern_bytes": int(len(pat)), "equals_fused": bool(np.array_equal(ends, mine)), "seconds_per_query": bsec / nb})
    frow = row_case("overlap (host buffers), the baseline's %d reads, min_ovlp=%d" % (nb, min_ovlp), nb, fsec, nb * L, 2)
    frow.update({"measured": True, "records": int(cnt.sum()), "seconds_per_query": fsec / nb})
    g.close()
    res["overlap"] = {"index": index, "cases": rows + [brow, frow]}


def approx_case(a, res):
    """reads of the index with 0 .. max_mm planted substitutions through approx_dev: queries per second, and rank pairs per second from a
    lower bound of the steps (the call does not report the steps a query took: a query that finds its read again ranks every position
    once for the piece bound and once along the path of the match, 2 L pairs, and whatever it backtracks through on top)"""
    L, M = 101, 16
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    P = a.approx_queries
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    g.dev_free(p)
    index = {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": int(g.counts().sum()), "strands": 1, "layout": g.layout_stats()}
    rng = np.random.RandomState(11)
    rows = []
    do, dr, dc = g.dev_alloc(8 * (P + 1)), g.dev_alloc(32 * M * P), g.dev_alloc(8 * P)
    off = np.arange(P + 1, dtype=np.int64) * L
    g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
    for max_mm, planted in ((0, 0), (1, 1), (2, 2), (2, 0), (3, 3)):
        qs = hit_patterns(P, L, n, 101).copy()
        for _ in range(planted):                                    # (two may fall on one position: then fewer are planted)
            at = rng.randint(L, size=P)
            qs[np.arange(P), at] = 1 + (qs[np.arange(P), at] + rng.randint(3, size=P)) % 4
        flat = np.ascontiguousarray(qs.reshape(-1))
        dq = g.dev_alloc(len(flat))
        g.L.rb2_hip_memcpy(g.h, dq, flat.ctypes.data, len(flat), 0)
        sec, lo, hi = spread(lambda: g.approx_dev(P, dq, do, dr, dc, max_mm, 1, a.approx_steps, M), g.sync)
        cnt = np.zeros(P, np.int64)
        g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, dc, 8 * P, 1)
        g.dev_free(dq)
        assert (cnt != -1).all() and (planted > max_mm or ((cnt >= 1) | (cnt <= -2)).all())      # the read itself is within reach, unless the steps ran out
        least = int(2 * L * ((cnt >= 1) | (cnt <= -3)).sum() + (cnt == 0).sum())
        row = {"case": "approx_dev, %d reads of the index (%d bp) with %d planted substitutions, max_mm=%d min_occ=1 max_steps=%d max_recs=%d" % (P, L, planted, max_mm, a.approx_steps, M),
               "measured": True, "queries": P, "seconds": sec, "seconds_fastest": lo, "seconds_slowest": hi, "queries_per_s": P / sec,
               "rank_pairs_at_least": least, "rank_pairs_per_s_at_least": least / sec, "matches": int(np.maximum(cnt, 0).sum()),
               "queries_with_a_match": int((cnt >= 1).sum()), "queries_out_of_steps": int((cnt <= -2).sum()), "queries_with_more_than_max_recs": int((cnt > M).sum())}
        rows.append(row)
        print("approx: max_mm %d, %d planted: %d queries in %.3f s" % (max_mm, planted, P, sec), file=sys.stderr, flush=True)
    for q in (do, dr, dc):
        g.dev_free(q)
    g.close()
    res["approx"] = {"index": index, "cases": rows}


def plant_edits(rng, reads, planted):
    """reads (P, L) with `planted` edits each -- one substitution, one deleted base, one inserted base in turn, read i starting the turn at
    kind i % 3, never at the two end positions: (the queries concatenated, their P + 1 offsets).  The reads of one turn stay together, so
    the queries come out in three groups of one length each"""
    flat, lens = [], []
    for r in range(3):
        q = reads[r::3].copy()
        for j in range(planted):
            n, m = q.shape
            kind = (r + j) % 3
            if kind == 0:                                            # another symbol at 1 .. m - 2
                at = rng.randint(1, m - 1, size=n)
                q[np.arange(n), at] = 1 + (q[np.arange(n), at] + rng.randint(3, size=n)) % 4
            elif kind == 1:                                          # the symbol at 1 .. m - 2 deleted
                keep = np.ones((n, m), bool)
                keep[np.arange(n), rng.randint(1, m - 1, size=n)] = False
                q = q[keep].reshape(n, m - 1)
            else:                                                    # a symbol inserted in front of 1 .. m - 1
                new = np.zeros((n, m + 1), bool)
                new[np.arange(n), rng.randint(1, m, size=n)] = True
                t = np.empty((n, m + 1), np.uint8)
                t[~new] = q.reshape(-1)
                t[new] = rng.randint(1, 5, size=n)
                q = t
        flat.append(q.reshape(-1))
        lens.append(np.full(len(q), q.shape[1], np.int64))
    return np.ascontiguousarray(np.concatenate(flat)), np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)


def approx_ed_case(a, res):
    """reads of the index with 0, 1, 2 planted edits (plant_edits) through approx_ed_dev at max_ed = planted: queries per second.  Next to
    each, the same reads with as many planted substitutions only (never at the ends either) through approx_dev at max_mm = planted, on the
    same index with the same budget: what a step cost before the column.  Neither call reports its steps; the records are counted"""
    L, M = 101, 16
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    P = a.approx_ed_queries
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    g.dev_free(p)
    index = {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": int(g.counts().sum()), "strands": 1, "layout": g.layout_stats()}
    rng = np.random.RandomState(13)
    reads = hit_patterns(P, L, n, 101)
    rows = []
    do, dr, dc = g.dev_alloc(8 * (P + 1)), g.dev_alloc(32 * M * P), g.dev_alloc(8 * P)

    def run(call, flat, off, k):
        dq = g.dev_alloc(len(flat))
        g.L.rb2_hip_memcpy(g.h, dq, flat.ctypes.data, len(flat), 0)
        g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
        sec, lo, hi = spread(lambda: call(P, dq, do, dr, dc, k, 1, a.approx_steps, M), g.sync)
        cnt = np.zeros(P, np.int64)
        g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, dc, 8 * P, 1)
        g.dev_free(dq)
        assert (cnt != -1).all() and ((cnt >= 1) | (cnt <= -2)).all()                             # the read itself is within reach, unless the steps ran out
        return {"queries": P, "seconds": sec, "seconds_fastest": lo, "seconds_slowest": hi, "queries_per_s": P / sec, "matches": int(np.maximum(cnt, 0).sum()),
                "queries_with_a_match": int((cnt >= 1).sum()), "queries_out_of_steps": int((cnt <= -2).sum()), "queries_with_more_than_max_recs": int((cnt > M).sum())}

    for planted in (0, 1, 2):
        flat, off = plant_edits(rng, reads, planted)
        ed = run(g.approx_ed_dev, flat, off, planted)
        subs = reads.copy()
        for _ in range(planted):                                    # (two may fall on one position: then fewer are planted)
            at = rng.randint(1, L - 1, size=P)
            subs[np.arange(P), at] = 1 + (subs[np.arange(P), at] + rng.randint(3, size=P)) % 4
        mm = run(g.approx_dev, np.ascontiguousarray(subs.reshape(-1)), np.arange(P + 1, dtype=np.int64) * L, planted)
        rows.append({"case": "%d reads of the index (%d bp), %d planted: approx_ed_dev on edits (substitution, deletion, insertion in turn) at max_ed=%d, approx_dev on substitutions at "
                             "max_mm=%d; min_occ=1 max_steps=%d max_recs=%d" % (P, L, planted, planted, planted, a.approx_steps, M),
                     "measured": True, "planted": planted, "approx_ed_dev": ed, "approx_dev": mm, "seconds_ratio": ed["seconds"] / mm["seconds"]})
        print("approx_ed: %d planted: %d queries in %.3f s (approx_dev on substitutions: %.3f s)" % (planted, P, ed["seconds"], mm["seconds"]), file=sys.stderr, flush=True)
    for q in (do, dr, dc):
        g.dev_free(q)
    g.close()
    res["approx_ed"] = {"index": index, "cases": rows}


def composed_kmers(g, lo, hi, code, l0, k, min_occ):
    """the k-mers that end in the l0-mer `code` with interval [lo, hi), level by level from the host: one extend call per level"""
    code = np.array([code], np.uint64); ik = np.array([[lo, 0, hi - lo]], np.int64)
    calls = items = 0
    for l in range(l0, k):
        ok = g.extend(ik, 1)[:, 1:5]                                 # (n, 4, 3): the left extensions by A C G T
        calls += 1; items += len(ik)
        live = ok[:, :, 2] >= min_occ
        code = (code[:, None] | (np.arange(4, dtype=np.uint64)[None, :] << np.uint64(2 * l)))[live]
        ik = np.ascontiguousarray(ok[live])
        ik[:, 1] = 0
    return code, ik[:, 0], ik[:, 0] + ik[:, 2], calls, items


def kmers_case(a, res):
    L = 101
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    g.dev_free(p)
    N = int(g.counts().sum())
    P, Lp = a.patterns, 32
    pats = hit_patterns(P, Lp, n, Lp)
    flat = np.ascontiguousarray(pats.reshape(-1)); off = np.arange(P + 1, dtype=np.int64) * Lp
    dp, do, dq = g.dev_alloc(len(flat)), g.dev_alloc(8 * (P + 1)), g.dev_alloc(24 * P)
    g.L.rb2_hip_memcpy(g.h, dp, flat.ctypes.data, len(flat), 0)
    g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)

    def bsearch(tag):
        sec, lo, hi = spread(lambda: g.backward_search_dev(P, dp, do, dq), g.sync)
        row = row_case("backward_search_dev L=%d hits, %d patterns%s" % (Lp, P, tag), P, sec, P * Lp, 2)
        row.update({"measured": True, "lf_steps_per_s_slowest": P * Lp / hi, "lf_steps_per_s_fastest": P * Lp / lo})
        return row
    rows = [bsearch("")]
    for k in (21, 31):
        for min_occ in (1, 2):
            items = 1 + sum(g.kmers_raw(l, min_occ, False, 0, 0)[0] for l in range(1, k))          # the l-mers the walk ranks, l < k
            got = [None]

            def spectrum():
                got[0] = g.kmers_raw(k, min_occ, False, 0, 256)
            sec, lo, hi = spread(spectrum, lambda: None)
            found, _, hist, info = got[0]
            base = {"k": k, "min_occ": min_occ, "kmers": found, "expanded_items": items, "launches": int(info[0]), "largest_segment": int(info[1]),
                    "segments_alive": int(info[2]), "measured": True}
            row = dict(base, case="kmers k=%d min_occ=%d, spectrum only (256 bins)" % (k, min_occ), seconds=sec, kmers_per_s=found / sec,
                       expanded_items_per_s=items / sec, expanded_items_per_s_slowest=items / hi, expanded_items_per_s_fastest=items / lo, spectrum_head=hist[:8].tolist())
            rows.append(row)
            print("kmers: k %d min_occ %d: %d k-mers, %d items, spectrum in %.3f s" % (k, min_occ, found, items, sec), file=sys.stderr, flush=True)
            cap = min(found, a.kmer_recs)

            def records():
                got[0] = g.kmers_raw(k, min_occ, False, cap, 0)
            sec, lo, hi = spread(records, lambda: None)
            assert got[0][0] == found
            rows.append(dict(base, case="kmers k=%d min_occ=%d, records to host (max_recs %d)" % (k, min_occ, cap), seconds=sec, records=cap, kmers_per_s=found / sec,
                             records_per_s=cap / sec, expanded_items_per_s=items / sec, expanded_items_per_s_slowest=items / hi, expanded_items_per_s_fastest=items / lo))
    rows.append(bsearch(" (again, after the k-mer runs)"))
    # the baseline: the k-mers that end in one 8-mer, from the host level by level, against the fused records with that ending
    k, min_occ, l0 = 21, 2, 8
    tail = pats[0, :l0]
    tcode = int(sum((int(c) - 1) << (2 * (l0 - 1 - i)) for i, c in enumerate(tail)))
    blo, bhi, bm = g.backward_search([tail])
    assert bm[0] == l0
    t = time.perf_counter()
    ccode, clo, chi, calls, citems = composed_kmers(g, int(blo[0]), int(bhi[0]), tcode, l0, k, min_occ)
    bsec = time.perf_counter() - t
    found = g.kmers_raw(k, min_occ, False, 0, 0)[0]
    same = None
    if found <= a.kmer_recs:
        _, rec, _, _ = g.kmers_raw(k, min_occ, False, found, 0)
        mine = rec[(rec[:, 0].astype(np.uint64) & np.uint64(4 ** l0 - 1)) == np.uint64(tcode)]
        mine = mine[np.argsort(mine[:, 1])]
        o = np.argsort(clo)
        same = bool(len(mine) == len(ccode) and np.array_equal(mine[:, 0].astype(np.uint64), ccode[o]) and np.array_equal(mine[:, 1], clo[o]) and np.array_equal(mine[:, 2], chi[o]))
    rows.append({"case": "baseline: the k-mers ending in one %d-mer (k=%d, min_occ=%d) from the host, one rb2_hip_extend call per level" % (l0, k, min_occ), "seconds": bsec,
                 "extend_calls": calls, "expanded_items": citems, "expanded_items_per_s": citems / bsec, "kmers": int(len(ccode)), "equals_fused": same, "measured": True})
    for q in (dp, do, dq):
        g.dev_free(q)
    res["kmers"] = {"index": {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": N, "strands": 1, "layout": g.layout_stats()}, "cases": rows}
    g.close()


def delete_case(a, res):
    L = 101
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    nb = n * (L + 1)
    g = HipBwt(a.so)
    p = g.dev_alloc(nb)
    t = time.perf_counter()
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, nb)
    g.sync()
    build_s = time.perf_counter() - t
    symbols = int(g.counts().sum())
    keep = np.random.RandomState(17).rand(n) >= a.delete
    ids = np.flatnonzero(~keep)
    t = time.perf_counter()
    rows = g.delete(ids)
    sec = time.perf_counter() - t
    st = g.delete_stats()
    hashes = g.rope_hashes() if a.so == 0 else None
    pool = (st["leaves_read"] + st["leaves_written"]) * LEAF_BYTES
    traffic = st["leaves_read"] * (2 * LEAF_BYTES + 3 * 128 + 12 + 12) + st["leaves_written"] * 2 * LEAF_BYTES   # planes twice, marks zeroed + read twice, kept counts and bases; zeroed + written
    case = {"fraction": a.delete, "sorting_order": a.so, "reads": n, "symbols": symbols, "build_seconds": build_s, "ids": int(len(ids)), "rows_removed": rows,
            "seconds": sec, "pool_bytes": pool, "pool_bytes_per_s": pool / sec, "traffic_bytes": traffic, "traffic_bytes_per_s": traffic / sec,
            "fraction_of_hbm_peak": traffic / sec / HBM_PEAK, "groups": st["groups"], "groups_compressed": st["groups_compressed"],
            "fast_path_share": 1.0 - st["groups_compressed"] / max(st["groups"], 1), "measured": True}
    # what a user could do before: reset, insert the survivors again (their text already on the device)
    host = np.empty(nb, np.uint8)
    g.synth_reads(p, 0, n, L, seed=42)
    g.sync()
    g.L.rb2_hip_memcpy(g.h, host.ctypes.data, p, nb, 1)
    surv = np.ascontiguousarray(host.reshape(n, L + 1)[keep]).reshape(-1)
    del host
    g.L.rb2_hip_memcpy(g.h, p, surv.ctypes.data, len(surv), 0)
    g.sync()
    t = time.perf_counter()
    g.reset()
    g.insert_multi_dev(p, len(surv))
    g.sync()
    alt = time.perf_counter() - t
    case["rebuild_seconds"] = alt
    case["rebuild_over_delete"] = alt / sec
    case["rebuild_same_strings"] = a.so == 0
    case["rebuild_equals_delete"] = (g.rope_hashes() == hashes) if a.so == 0 else None
    g.dev_free(p)
    g.close()
    res.setdefault("delete", []).append(case)


def contained_case(a, res):
    L = 101
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    nb = n * (L + 1)
    for name, glen in (("default: unique reads", 0), ("reads of one genome at 30x", n * L // 30)):
        g = HipBwt(a.so)
        p = g.dev_alloc(nb)
        t = time.perf_counter()
        g.synth_reads(p, 0, n, L, seed=42, genome_len=glen)
        g.insert_multi_dev(p, nb)
        g.sync()
        build_s = time.perf_counter() - t
        g.dev_free(p)
        case = {"index": name, "reads": n, "read_len": L, "genome_len": glen, "sorting_order": a.so, "symbols": int(g.counts().sum()), "build_seconds": build_s,
                "layout": g.layout_stats(), "runs": [], "measured": True}
        print("contained: %s built in %.1f s" % (name, build_s), file=sys.stderr, flush=True)
        d_rec = g.dev_alloc(40 * n)
        rec = np.zeros((n, 5), np.int64)
        full_occ = None
        for early in (1, 0):
            os.environ["RB2_CONTAIN_EARLY"] = str(early)
            sec = timed(lambda: g.contained_dev(n, None, d_rec), g.sync, reps=3 if early else 1)
            g.L.rb2_hip_memcpy(g.h, rec.ctypes.data, d_rec, rec.nbytes, 1)
            steps = int(rec[:, 4].sum())
            share = np.bincount(np.clip(rec[:, 0], -2, 4) + 2, minlength=7) / n
            case["runs"].append({"early_exit": bool(early), "seconds": sec, "strings_per_s": n / sec, "lf_steps": steps, "lf_steps_per_s": steps / sec,
                                 "ranks_per_s_at_most": 4 * steps / sec, "mean_walked": steps / n,
                                 "flag_share": {str(f): float(share[f + 2]) for f in (0, 1, 2, 3, 4, -1, -2)}})
            print("contained: early exit %d: %.3f s" % (early, sec), file=sys.stderr, flush=True)
            if not early:
                full_occ = rec[:, 1].copy()
        g.dev_free(d_rec)
        os.environ.pop("RB2_CONTAIN_EARLY", None)
        # the composition the call replaces, through the host, on a sample: extract, then backward_search of what came out
        m = min(a.contained_sample, n)
        ids = np.sort(np.random.RandomState(5).choice(n, size=m, replace=False)).astype(np.int64)
        out3 = np.zeros((m, 3), np.int64)

        def composed():
            _, txt, ln = g.extract_raw(ids, L)
            off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
            flat = np.ascontiguousarray(txt.reshape(-1)) if (ln == L).all() else np.ascontiguousarray(np.concatenate([txt[i, :ln[i]] for i in range(m)]))
            g.L.rb2_hip_backward_search(g.h, m, flat.ctypes.data, off.ctypes.data, out3.ctypes.data)
        csec = timed(composed, lambda: None)
        got = {}

        def fused():
            got["rec"] = g.contained_raw(ids)
        fsec = timed(fused, lambda: None)
        os.environ["RB2_CONTAIN_EARLY"] = "0"
        fsec0 = timed(fused, lambda: None)
        os.environ.pop("RB2_CONTAIN_EARLY", None)
        case["sample"] = {"strings": m, "composed_extract_then_backward_search_seconds": csec, "contained_host_seconds": fsec,
                          "contained_host_seconds_no_early_exit": fsec0, "composed_over_fused": csec / fsec, "composed_over_fused_no_early_exit": csec / fsec0,
                          "equals_fused": bool(np.array_equal(out3[:, 1] - out3[:, 0], full_occ[ids]) and np.array_equal(got["rec"][:, 1], full_occ[ids])),
                          "note": "the composition yields occ alone; n_equal and rank would take an overlap call more"}
        g.close()
        res.setdefault("contained", []).append(case)


def irreducible_case(a, res):
    import irreducible_ref as IR
    L, M = 101, 4
    n = a.reads or 4_000_000
    min_ovlp = a.irreducible_min_ovlp
    max_ext = L - min_ovlp                                          # reads of one length: a neighbour leaves the read by L - l symbols
    g = HipBwt(0)                                                   # input order: strings 2i and 2i + 1 are a read and its reverse complement
    nb = 2 * n * (L + 1)
    p = g.dev_alloc(nb)
    t = time.perf_counter()
    g.synth_reads(p, 0, n, L, seed=42, strand=1, genome_len=n * L // 30)
    g.insert_multi_dev(p, nb)
    g.sync()
    build_s = time.perf_counter() - t
    g.dev_free(p)
    t = time.perf_counter()
    gone = g.reduce(pairs=True)
    reduce_s = time.perf_counter() - t
    left = int(g.counts()[:, 0].sum())
    index = {"reads": n, "read_len": L, "genome_len": n * L // 30, "strands": 2, "sorting_order": 0, "build_seconds": build_s, "reduce_pairs_seconds": reduce_s,
             "strings_removed": int(len(gone)), "strings": left, "symbols": int(g.counts().sum()), "layout": g.layout_stats()}
    print("irreducible: index of %d strings built in %.1f s, reduced in %.1f s" % (left, build_s, reduce_s), file=sys.stderr, flush=True)
    P = min(a.irreducible_queries, left)
    ids = np.sort(np.random.RandomState(5).choice(left, size=P, replace=False)).astype(np.int64)
    _, txt, ln = g.extract_raw(ids, L)
    assert (ln == L).all()
    flat = np.ascontiguousarray(txt.reshape(-1)); off = np.arange(P + 1, dtype=np.int64) * L
    dq, do, dr, dc, dv = g.dev_alloc(len(flat)), g.dev_alloc(8 * (P + 1)), g.dev_alloc(32 * M * P), g.dev_alloc(8 * P), g.dev_alloc(24 * (max_ext + 1) * P)
    g.L.rb2_hip_memcpy(g.h, dq, flat.ctypes.data, len(flat), 0)
    g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
    sec, lo, hi = spread(lambda: g.irreducible_dev(P, dq, do, dr, dc, L, min_ovlp, max_ext, a.irreducible_steps, M), g.sync)
    cnt = np.zeros(P, np.int64); rec = np.zeros((P, M, 4), np.int64)
    g.L.rb2_hip_memcpy(g.h, cnt.ctypes.data, dc, 8 * P, 1)
    g.L.rb2_hip_memcpy(g.h, rec.ctypes.data, dr, rec.nbytes, 1)
    osec, _, _ = spread(lambda: g.overlap_dev(P, dq, do, dv, dc, min_ovlp, max_ext + 1), g.sync)
    ocnt = np.zeros(P, np.int64)
    g.L.rb2_hip_memcpy(g.h, ocnt.ctypes.data, dc, 8 * P, 1)
    for q in (dq, do, dr, dc, dv):
        g.dev_free(q)
    assert (cnt != -1).all() and (ocnt >= 1).all()                  # a read of the index finds itself at its full length: that record is no candidate
    found = np.where(cnt <= -2, -2 - cnt, cnt)
    live = np.arange(M)[None, :] < np.minimum(found, M)[:, None]
    least = int(P * L + (ocnt - 1).sum() + rec[:, :, 1][live].sum())
    row = {"case": "irreducible_dev, %d reads of the index (%d bp), min_ovlp=%d max_ext=%d max_steps=%d max_recs=%d" % (P, L, min_ovlp, max_ext, a.irreducible_steps, M),
           "measured": True, "queries": P, "seconds": sec, "seconds_fastest": lo, "seconds_slowest": hi, "queries_per_s": P / sec,
           "rank_pairs_at_least": least, "rank_pairs_per_s_at_least": least / sec, "records": int(found.sum()), "records_per_query": float(found.sum() / P),
           "queries_out_of_steps": int((cnt <= -2).sum()), "queries_with_more_than_max_recs": int((found > M).sum()),
           "overlap_records_below_full_length": int((ocnt - 1).sum()), "share_of_overlap_records_that_survive": float(found.sum() / max((ocnt - 1).sum(), 1)),
           "overlap_dev_seconds_same_reads": osec}
    print("irreducible: %d queries in %.3f s" % (P, sec), file=sys.stderr, flush=True)
    # the composition it replaces, on few reads: overlaps, the text of every neighbour, the pruning on the host
    g.build_ssa(5)
    nq = min(a.baseline_queries // 5, P)                            # (4000 reads by default)
    qs = list(txt[:nq])
    got = {}

    def composed():
        ov = g.overlaps(qs, min_ovlp, max_hits=64)
        ov = [[(k, l) for k, l in o if l < L] for o in ov]
        need = np.unique(np.array([k for o in ov for k, _ in o], np.int64))
        texts = dict(zip(need.tolist(), g.extract(need, L)))
        got["composed"] = [sorted(IR.edges_by_composition(texts, o, max_ext)) for o in ov]

    def fused():
        got["fused"] = g.irreducible(qs, min_ovlp, max_ext, max_steps=a.irreducible_steps, max_recs=64, max_hits=64, pairs=True)
    csec = timed(composed, lambda: None, reps=1)
    fsec = timed(fused, lambda: None, reps=1)
    brow = {"case": "baseline: overlaps(), extract of every neighbour, pruning on the host; %d reads" % nq, "measured": True, "queries": nq, "seconds": csec,
            "seconds_per_query": csec / nq, "edges": int(sum(len(e) for e in got["composed"])), "equals_fused": bool(got["composed"] == got["fused"])}
    frow = {"case": "irreducible(pairs=True) (host buffers, string ids resolved), the baseline's %d reads" % nq, "measured": True, "queries": nq, "seconds": fsec,
            "seconds_per_query": fsec / nq, "edges": int(sum(len(e) for e in got["fused"])), "composed_over_fused": csec / fsec}
    g.close()
    res["irreducible"] = {"index": index, "cases": [row, brow, frow]}


def unitig_case(a, res):
    import unitig_ref as U
    L, M = 101, 8
    n = a.reads or 1_000_000
    min_ovlp = a.irreducible_min_ovlp
    g = HipBwt(0)
    nb = 2 * n * (L + 1)
    p = g.dev_alloc(nb)
    g.synth_reads(p, 0, n, L, seed=42, strand=1, genome_len=n * L // 30)
    g.insert_multi_dev(p, nb)
    g.sync()
    g.dev_free(p)
    gone = g.reduce(pairs=True)
    ns = int(g.counts()[:, 0].sum())
    g.build_ssa(5)
    # the edges of every string: irreducible records, their `$` ranges resolved to ids, rows src, dst, l, ext
    t = time.perf_counter()
    _, txt, ln = g.extract_raw(np.arange(ns, dtype=np.int64), L)
    assert (ln == L).all()
    flat = np.ascontiguousarray(txt.reshape(-1)); off = np.arange(ns + 1, dtype=np.int64) * L
    rec = np.zeros((ns, M, 4), np.int64); cnt = np.zeros(ns, np.int64)
    g.L.rb2_hip_irreducible(g.h, ns, flat.ctypes.data, off.ctypes.data, min_ovlp, L - min_ovlp, a.irreducible_steps, M, rec.ctypes.data, cnt.ctypes.data)
    assert (cnt != -1).all()
    found = np.where(cnt <= -2, -2 - cnt, cnt)                      # (a read out of steps or of slots keeps the records it has: the graph is what it is)
    live = np.arange(M)[None, :] < np.minimum(found, M)[:, None]
    who, recs = np.nonzero(live)[0], rec[live]
    H8 = 8
    _, ids, n_ids = g.string_ids_raw(recs[:, 2:], H8)
    hit = np.arange(H8)[None, :] < np.minimum(n_ids, H8)[:, None]
    rows = np.nonzero(hit)[0]
    edges = np.ascontiguousarray(np.stack([who[rows], ids[hit] ^ 1, recs[rows, 0], recs[rows, 1]], 1).astype(np.int64))
    m = len(edges)
    edges_s = time.perf_counter() - t
    del txt, flat, rec
    index = {"reads": n, "read_len": L, "genome_len": n * L // 30, "strands": 2, "sorting_order": 0, "strings_removed": int(len(gone)), "strings": ns,
             "symbols": int(g.counts().sum()), "min_ovlp": min_ovlp, "edges": m,
             "reads_out_of_steps": int((cnt <= -2).sum()), "reads_with_more_records_than_slots": int((found > M).sum()), "ranges_wider_than_slots": int((n_ids > H8).sum()), "edges_seconds_not_part_of_the_measurement": edges_s, "layout": g.layout_stats()}
    print("unitigs: %d strings, %d edges in %.1f s" % (ns, m, edges_s), file=sys.stderr, flush=True)
    de, dv, di = g.dev_alloc(max(edges.nbytes, 8)), g.dev_alloc(32 * ns), g.dev_alloc(32)
    g.L.rb2_hip_memcpy(g.h, de, edges.ctypes.data, edges.nbytes, 0)
    csec, clo, chi = spread(lambda: g.unitig_chains_dev(ns, m, de, dv, di), g.sync)
    info = np.zeros(4, np.int64); vtx = np.zeros((ns, 4), np.int64)
    g.L.rb2_hip_memcpy(g.h, info.ctypes.data, di, 32, 1)
    g.L.rb2_hip_memcpy(g.h, vtx.ctypes.data, dv, vtx.nbytes, 1)
    K = 0
    while (1 << K) < ns:
        K += 1
    crow = {"case": "unitig_chains_dev, %d vertices, %d edges" % (ns, m), "measured": True, "seconds": csec, "seconds_fastest": clo, "seconds_slowest": chi,
            "vertices_per_s": ns / csec, "chains": int(info[0]), "cycles": int(info[1]), "longest_chain": int(info[2]), "edges_ignored": int(info[3]),
            "doublings_queued": 2 * K, "launches": 2 * K + 5 + -(-m // (1 << 24))}
    got = {}

    def size():
        got["size"] = g.unitig_text_dev(ns, dv, None, None, True, 1, 0, 0)
    ssec, _, _ = spread(size, lambda: None)
    sel, total = int(got["size"][1][0]), int(got["size"][1][1])
    du, dt = g.dev_alloc(max(40 * sel, 8)), g.dev_alloc(max(total, 8))

    def text():
        got["text"] = g.unitig_text_dev(ns, dv, du, dt, True, 1, sel, total)
    tsec, tlo, thi = spread(text, lambda: None)
    stored, tinfo = got["text"]
    urec = np.zeros((sel, 5), np.int64)
    g.L.rb2_hip_memcpy(g.h, urec.ctypes.data, du, urec.nbytes, 1)
    chosen = np.zeros(ns, bool); chosen[urec[:, 0]] = True
    steps_all = int(L * sel * 2 + vtx[chosen[vtx[:, 0]] & (vtx[:, 0] != np.arange(ns)), 3].sum())   # two walks per selected head, ext_in steps for every other vertex of a selected chain
    trow = {"case": "unitig_text_dev canonical=1 min_reads=1, caps from the sizing call", "measured": True, "seconds": tsec, "seconds_fastest": tlo, "seconds_slowest": thi,
            "sizing_call_seconds": ssec, "chains_selected": sel, "chains_stored": int(stored), "total_text": total, "chains_with_a_short_piece": int(tinfo[2]),
            "lf_steps": steps_all, "lf_steps_per_s": steps_all / tsec, "text_bytes_per_s": total / tsec}
    for q in (de, dv, di, du, dt):
        g.dev_free(q)
    print("unitigs: chains %.4f s, text %.4f s" % (csec, tsec), file=sys.stderr, flush=True)
    # the composition on a sample: the first vertices of the longest chain, the edges among them
    h0 = int(vtx[np.argmax(vtx[:, 1]), 0])
    S = min(a.unitig_sample, int(info[2]))
    V = np.sort(np.flatnonzero((vtx[:, 0] == h0) & (vtx[:, 1] < S)))
    inV = np.zeros(ns, bool); inV[V] = True
    sub = np.ascontiguousarray(edges[inV[edges[:, 0]] & inV[edges[:, 1]]])
    loc = sub.copy(); loc[:, 0] = np.searchsorted(V, sub[:, 0]); loc[:, 1] = np.searchsorted(V, sub[:, 1])

    def composed():
        v, _ = U.chains(len(V), loc)
        strings = g.extract(V, L)
        got["composed"] = U.texts(strings, v, False, 2)

    def fused():
        v, _ = g.unitig_chains(sub)
        got["fused"] = g.unitig_text(v, False, 2)
    bsec = timed(composed, lambda: None, reps=1)
    fsec = timed(fused, lambda: None, reps=1)
    cu, ct, _ = got["composed"]
    fu, ft = got["fused"]
    same = bool(np.array_equal(ct, ft) and np.array_equal(V[cu[:, 0]], fu[:, 0]) and np.array_equal(cu[:, 1:], fu[:, 1:]))
    brow = {"case": "baseline: Python chain walk (tests/unitig_ref.py chains) + extract of every read + gluing, the first %d vertices of the longest chain and the %d edges among them" % (len(V), len(sub)),
            "measured": True, "seconds": bsec, "unitigs": int(len(cu)), "text": int(len(ct)), "equals_fused": same}
    frow = {"case": "unitig_chains + unitig_text (host buffers, min_reads=2) on the same edges", "measured": True, "seconds": fsec, "unitigs": int(len(fu)), "text": int(len(ft)),
            "composed_over_fused": bsec / fsec}
    g.close()
    res["unitigs"] = {"index": index, "cases": [crow, trow, brow, frow]}


def clean_case(a, res):
    """--clean: rb2_hip_graph_clean_dev on a synthetic edge list that needs no index (tests/graph_clean_ref.py backbone): both strands of
    --reads reads in a row, a one-read tip every 50 reads and a one-read bubble every 70; beside it unitig_chains_dev on the same list"""
    import graph_clean_ref as GC
    reads = a.reads or 1_000_000
    t0 = time.perf_counter()
    n, edges = GC.backbone(reads, tips=[(i, 1) for i in range(25, reads - 1, 50)], bubbles=[(i, 1, 1) for i in range(35, reads - 2, 70)])
    m = len(edges)
    print("clean: %d vertices, %d rows made in %.1f s" % (n, m, time.perf_counter() - t0), file=sys.stderr, flush=True)
    g = HipBwt(0)
    de, do, dv, di = g.dev_alloc(edges.nbytes), g.dev_alloc(edges.nbytes), g.dev_alloc(32 * n), g.dev_alloc(32)
    g.L.rb2_hip_memcpy(g.h, de, edges.ctypes.data, edges.nbytes, 0)
    got = {}

    def run():
        got["clean"] = g.graph_clean_dev(n, m, de, do, m)
    sec, lo, hi = spread(run, g.sync)
    kept, info = got["clean"]
    rounds = int(info[2])
    csec, clo, chi = spread(lambda: g.unitig_chains_dev(n, m, de, dv, di), g.sync)
    for d in (de, do, dv, di):
        g.dev_free(d)
    g.close()
    row = {"case": "graph_clean_dev max_tip_reads=2 max_bubble_reads=3 pairs=1, %d vertices, %d rows, cap = m" % (n, m), "measured": True, "seconds": sec, "seconds_fastest": lo,
           "seconds_slowest": hi, "rounds": rounds, "seconds_per_round": sec / max(rounds, 1), "rows_kept": int(kept), "tip_rows": int(info[3]), "bubble_rows": int(info[4]),
           "chains_after": int(info[6]), "rows_per_second_per_round": m * max(rounds, 1) / sec}
    crow = {"case": "unitig_chains_dev on the same list (every round contains it)", "measured": True, "seconds": csec, "seconds_fastest": clo, "seconds_slowest": chi}
    res["clean"] = {"list": {"vertices": n, "rows": m, "reads": reads, "tip_every": 50, "bubble_every": 70}, "cases": [row, crow],
                    "round_over_chains": sec / max(rounds, 1) / csec}
    print("clean: %.4f s in %d rounds, chains alone %.4f s" % (sec, rounds, csec), file=sys.stderr, flush=True)


def graph_case(a, res):
    """--graph: rb2_hip_string_graph_dev on the both-strand read index of --unitigs (reduced, suffix array at log2_step 5)"""
    L, M, H8 = 101, 8, 8
    n = a.reads or 1_000_000
    min_ovlp = a.irreducible_min_ovlp
    kw = dict(min_ovlp=min_ovlp, max_ext=L - min_ovlp, max_steps=a.irreducible_steps, max_recs=M, max_hits=H8, pairs=True)
    g = HipBwt(0)
    nb = 2 * n * (L + 1)
    p = g.dev_alloc(nb)
    g.synth_reads(p, 0, n, L, seed=42, strand=1, genome_len=n * L // 30)
    g.insert_multi_dev(p, nb)
    g.sync()
    g.dev_free(p)
    gone = g.reduce(pairs=True)
    ns = int(g.counts()[:, 0].sum())
    g.build_ssa(5)
    # (a) the whole graph: a counting call sizes the rows, the timed calls store them
    m, info = g.string_graph_dev(0, ns, None, 0, **kw)
    de = g.dev_alloc(max(32 * m, 8))
    got = {}

    def full():
        got["full"] = g.string_graph_dev(0, ns, de, m, **kw)
    sec, lo, hi = spread(full, lambda: None)
    m2, info = got["full"]
    assert m2 == m and info[1] == m
    index = {"reads": n, "read_len": L, "genome_len": n * L // 30, "strands": 2, "sorting_order": 0, "strings_removed": int(len(gone)), "strings": ns,
             "symbols": int(g.counts().sum()), "ssa_log2_step": 5, "layout": g.layout_stats()}
    arow = {"case": "(a) string_graph_dev over all %d strings, min_ovlp=%d max_ext=%d max_steps=%d max_recs=%d max_hits=%d pairs=1" % (ns, min_ovlp, L - min_ovlp, a.irreducible_steps, M, H8),
            "measured": True, "sources": ns, "edges": m, "seconds": sec, "seconds_fastest": lo, "seconds_slowest": hi, "sources_per_s": ns / sec, "edges_per_s": m / sec,
            "edge_bytes_per_s": 32 * m / sec, "info": [int(v) for v in info]}
    print("graph: %d sources, %d edges in %.3f s" % (ns, m, sec), file=sys.stderr, flush=True)
    # (c) the glue: the search alone on the same strings, their texts already on the device
    _, txt, ln = g.extract_raw(np.arange(ns, dtype=np.int64), L)
    assert (ln == L).all()
    flat = np.ascontiguousarray(txt.reshape(-1)); off = np.arange(ns + 1, dtype=np.int64) * L
    dq, do, dr, dc = g.dev_alloc(len(flat)), g.dev_alloc(8 * (ns + 1)), g.dev_alloc(32 * M * ns), g.dev_alloc(8 * ns)
    g.L.rb2_hip_memcpy(g.h, dq, flat.ctypes.data, len(flat), 0)
    g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (ns + 1), 0)
    isec, ilo, ihi = spread(lambda: g.irreducible_dev(ns, dq, do, dr, dc, L, min_ovlp, L - min_ovlp, a.irreducible_steps, M), g.sync)
    sec2, lo2, hi2 = spread(full, lambda: None)                       # (again, next to it in time)
    for q in (dq, do, dr, dc, de):
        g.dev_free(q)
    del txt, flat
    crow = {"case": "(c) irreducible_dev alone on the same %d strings, texts resident, against string_graph_dev measured next to it" % ns, "measured": True,
            "irreducible_dev_seconds": isec, "irreducible_dev_fastest": ilo, "irreducible_dev_slowest": ihi,
            "string_graph_dev_seconds": sec2, "string_graph_dev_fastest": lo2, "string_graph_dev_slowest": hi2,
            "glue_seconds": sec2 - isec, "string_graph_over_irreducible": sec2 / isec}
    # (b) against the host composition, on a sample the Python loop can follow
    S = min(a.unitig_sample, ns)

    def composed():
        got["composed"] = g.edges(np.arange(S, dtype=np.int64), **kw)

    def fused():
        got["fused"] = g.string_graph(0, S, **kw)
    bsec = timed(composed, lambda: None, reps=1)                      # (edges() raises when a read of the sample runs out of max_steps: raise --irreducible-steps then)
    fsec, flo, fhi = spread(fused, lambda: None)
    f_edges, f_info = got["fused"]
    same = bool(np.array_equal(f_edges[np.lexsort(f_edges.T[::-1])], got["composed"]))
    brow = {"case": "(b) baseline: HipBwt.edges() (extract, irreducible, string_ids through host buffers, Python tuples), the first %d strings" % S, "measured": True,
            "sources": S, "seconds": bsec, "edges": int(len(got["composed"])), "sources_per_s": S / bsec, "equals_fused": same}
    frow = {"case": "(b) string_graph (host buffers) on the same %d strings" % S, "measured": True, "sources": S, "seconds": fsec, "seconds_fastest": flo, "seconds_slowest": fhi,
            "edges": int(len(f_edges)), "sources_per_s": S / fsec, "info": [int(v) for v in f_info], "composed_over_fused": bsec / fsec}
    g.close()
    res["string_graph"] = {"index": index, "cases": [arow, brow, frow, crow]}


def save_fmd_case(a, res):
    """rb2_hip_save_fmd against the route the host layer offers for the same bytes: rb2_hip_stream_rope of the six ropes into the parallel host
    writer (rb2_fmdp_*, 16 threads) and rb2_fmd_write to /dev/shm.  Warm-up, then the median of three; both routes end synchronised."""
    import ctypes as C
    from ropebwt2_amd.build import lib_path
    L = 101
    n = a.reads or 20_000_000
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    t = time.perf_counter()
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    build_s = time.perf_counter() - t
    g.dev_free(p)
    symbols = int(g.counts().sum())
    W = C.CDLL(lib_path("libropebwt2.so"))
    W.rb2_fmdp_init.restype = C.c_void_p; W.rb2_fmdp_init.argtypes = [C.c_int, C.c_int64]
    W.rb2_fmdp_expect.argtypes = [C.c_void_p, C.c_int64]
    W.rb2_fmdp_finish.restype = C.c_void_p; W.rb2_fmdp_finish.argtypes = [C.c_void_p]
    W.rb2_fmd_write_path.argtypes = [C.c_void_p, C.c_char_p]
    W.rb2_fmd_destroy.argtypes = [C.c_void_p]
    push = C.cast(W.rb2_fmdp_push_runs, C.c_void_p)                # (user, runs, n_bytes): the callback rb2_hip_stream_rope wants
    shm = "/dev/shm/rb2_save_fmd_bench_%d.fmd" % os.getpid()

    def host_route():
        w = W.rb2_fmdp_init(16, 0)
        W.rb2_fmdp_expect(w, symbols)
        for b in range(6):
            g.L.rb2_hip_stream_rope(g.h, b, push, w)
        f = W.rb2_fmdp_finish(w)
        assert W.rb2_fmd_write_path(f, shm.encode()) == 0
        W.rb2_fmd_destroy(f)
    out = {}

    def cold():                                                   # what a caller pays who saves once: the sizing pass, then the pass that writes
        g.L.rb2_hip_ssa_drop(g.h)                                 # (drops the size the handle remembers from the call before; there is no suffix array to free)
        out["img"] = g.save_fmd()

    def warm():                                                   # the size still remembered: the writing pass alone
        out["img"] = g.save_fmd()

    def sizing():
        g.L.rb2_hip_ssa_drop(g.h)
        out["size"] = int(g.L.rb2_hip_save_fmd(g.h, None, 0))
    try:
        cold_s = timed(cold, lambda: None)
        warm_s = timed(warm, lambda: None)
        size_s = timed(sizing, lambda: None)
        file_s = timed(lambda: g.save_fmd(shm), lambda: None)     # no sizing pass, nothing remembered is used
        same_file = bool(np.array_equal(np.fromfile(shm, np.uint8), out["img"]))
        host_s = timed(host_route, lambda: None)
        same = bool(np.array_equal(np.fromfile(shm, np.uint8), out["img"]))
    finally:
        if os.path.exists(shm):
            os.remove(shm)
    size = int(len(out["img"]))
    res["save_fmd"] = {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": symbols, "build_seconds": build_s, "file_bytes": size,
                       "save_fmd_seconds": cold_s, "save_fmd_size_remembered_seconds": warm_s, "sizing_call_seconds": size_s, "save_fmd_file_seconds": file_s,
                       "host_route_seconds": host_s, "host_over_device": host_s / cold_s, "host_over_device_file": host_s / file_s,
                       "images_equal": same, "file_equals_memory": same_file, "file_gb_per_s": size / cold_s / 1e9, "measured": True}
    g.close()


def merge_case(a, res):
    """rb2_hip_unpack_dev and rb2_hip_merge.  Unpack: symbols per second of unpack_dev over the whole index and over
    the first R strings, in both directions, of the host variant and of rb2_hip_extract on the same R strings (max_len = the read length: no
    padding).  Merge: an index of a quarter as many other reads merged into the benchmark index, against what a user could do before --
    rb2_hip_extract of the source's strings, reversing and terminating them on the host, rb2_hip_insert_multi from that host buffer into an
    identical index.  Every figure: the median, the fastest and the slowest of three after a warm-up; each run starts from a rebuilt
    destination (outside the timed region) and ends synchronised."""
    L = 101
    n = a.reads or 20_000_000
    m = n // 4
    R = min(a.rows, n)
    g, src = HipBwt(a.so), HipBwt(a.so)
    p, ps = g.dev_alloc(n * (L + 1)), src.dev_alloc(m * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    src.synth_reads(ps, n, m, L, seed=42)                          # the reads behind those of the destination
    g.sync(); src.sync()

    def rebuild():
        g.reset()
        g.insert_multi_dev(p, n * (L + 1))
        g.sync()
    t = time.perf_counter(); rebuild(); build_s = time.perf_counter() - t
    src.insert_multi_dev(ps, m * (L + 1))
    src.sync()
    src.dev_free(ps)
    symbols = int(g.counts().sum())
    out = {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": symbols, "build_seconds": build_s, "unpack": [], "measured": True}
    stat = lambda ts: {"seconds": float(np.median(ts)), "fastest": float(min(ts)), "slowest": float(max(ts))}
    # ---- unpack
    dt, do = g.dev_alloc(n * (L + 1) + 64), g.dev_alloc(8 * (n + 1))
    rows = np.arange(R, dtype=np.int64)
    for name, k, fn in (("unpack_dev all, text order", n, lambda: g.unpack_dev(0, n, False, n * (L + 1), dt, do)),
                        ("unpack_dev all, reversed", n, lambda: g.unpack_dev(0, n, True, n * (L + 1), dt, do)),
                        ("unpack_dev R, text order", R, lambda: g.unpack_dev(0, R, False, R * (L + 1), dt, do)),
                        ("unpack_dev R, reversed", R, lambda: g.unpack_dev(0, R, True, R * (L + 1), dt, do)),
                        ("unpack (host) R, text order", R, lambda: g.unpack_raw(0, R, False)),
                        ("extract (host) R, max_len = read length", R, lambda: g.extract_raw(rows, L))):
        med, lo, hi = spread(fn, g.sync)
        out["unpack"].append({"name": name, "strings": k, "symbols": k * L, "seconds": med, "fastest": lo, "slowest": hi, "symbols_per_s": k * L / med,
                              "lf_steps_per_s": (1 if "extract" in name else 2) * k * (L + 1) / med})
    u = {c["name"]: c for c in out["unpack"]}
    out["unpack_dev_over_extract"] = u["unpack_dev R, text order"]["symbols_per_s"] / u["extract (host) R, max_len = read length"]["symbols_per_s"]
    out["unpack_host_over_extract"] = u["unpack (host) R, text order"]["symbols_per_s"] / u["extract (host) R, max_len = read length"]["symbols_per_s"]
    g.dev_free(dt); g.dev_free(do)
    # ---- merge
    t_merge, t_extract, t_pack, t_insert, info, hashes = [], [], [], [], None, [None, None]
    for rep in range(4):                                           # the first is the warm-up
        if rep:
            rebuild()
        t = time.perf_counter(); info = g.merge(src); g.sync(); t_merge.append(time.perf_counter() - t)
    hashes[0] = g.rope_hashes()
    for rep in range(4):
        rebuild()
        t0 = time.perf_counter()
        fit, txt, ln = src.extract_raw(np.arange(m, dtype=np.int64), L)
        t1 = time.perf_counter()
        buf = np.zeros((m, L + 1), np.uint8)
        buf[:, :L] = txt[:, ::-1]
        buf = buf.reshape(-1)
        t2 = time.perf_counter()
        g.insert_multi(buf); g.sync()
        t3 = time.perf_counter()
        assert fit == m and (ln == L).all()
        t_extract.append(t1 - t0); t_pack.append(t2 - t1); t_insert.append(t3 - t2)
    hashes[1] = g.rope_hashes()
    path = [x + y + z for x, y, z in zip(t_extract, t_pack, t_insert)]
    out["merge"] = {"src_reads": m, "src_symbols": m * L, "info": list(info), "merge": stat(t_merge[1:]), "extract": stat(t_extract[1:]), "host_pass": stat(t_pack[1:]),
                    "insert_multi_host_buffer": stat(t_insert[1:]), "extract_pack_insert": stat(path[1:]),
                    "insert_over_merge": float(np.median(t_insert[1:]) / np.median(t_merge[1:])), "path_over_merge": float(np.median(path[1:]) / np.median(t_merge[1:])),
                    "same_index": hashes[0] == hashes[1]}
    g.dev_free(p)
    g.close(); src.close()
    res["merge"] = out


def correct_case(a, res):
    """rb2_hip_correct_dev and rb2_hip_correct_into on the index of the first cases; see the module docstring"""
    L, k = 101, a.correct_k
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    P, S = a.correct_reads, a.correct_sample
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    g.dev_free(p)
    probes = HipBwt.correct_default_probes(L, k)
    out = {"index": {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": int(g.counts().sum()), "strands": 1}, "k": k, "min_occ": 1, "max_fix": 8, "max_probes": probes,
           "measured": True}
    rng = np.random.RandomState(13)
    truth = hit_patterns(P, L, n, 101)
    qs = truth.copy()
    planted = np.arange(P) % 3
    for r in (1, 2):                                               # (two may fall on one position: then the second stands)
        who = np.flatnonzero(planted >= r)
        at = rng.randint(L, size=len(who))
        qs[who, at] = 1 + (truth[who, at] + rng.randint(3, size=len(who))) % 4
    flat = np.ascontiguousarray(qs.reshape(-1))
    off = np.arange(P + 1, dtype=np.int64) * L
    dq, do, dt, dc, dw = g.dev_alloc(len(flat)), g.dev_alloc(8 * (P + 1)), g.dev_alloc(len(flat)), g.dev_alloc(8 * P), g.dev_alloc(8 * P)
    g.L.rb2_hip_memcpy(g.h, dq, flat.ctypes.data, len(flat), 0)
    g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
    sec, lo, hi = spread(lambda: g.correct_dev(P, dq, do, P * L, dt, dc, dw, k, 1, 8, probes), g.sync)
    cnt, weak, got = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P * L, np.uint8)
    for d, arr in ((dc, cnt), (dw, weak), (dt, got)):
        g.L.rb2_hip_memcpy(g.h, arr.ctypes.data, d, arr.nbytes, 1)
    for d in (dq, do, dt, dc, dw):
        g.dev_free(d)
    same = (got.reshape(P, L) == truth).all(1)
    least = P * (L - k + 1)
    out["correct_dev"] = {"reads": P, "planted": "0, 1, 2 substitutions in turn", "seconds": sec, "seconds_fastest": lo, "seconds_slowest": hi, "reads_per_s": P / sec,
                          "probes_at_least": least, "probes_per_s_at_least": least / sec, "fixes": int(np.where(cnt <= -2, -2 - cnt, np.maximum(cnt, 0)).sum()),
                          "reads_restored": int(same.sum()), "reads_restored_by_planted": [int(same[planted == r].sum()) for r in range(3)],
                          "reads_over_budget": int((cnt <= -2).sum()), "reads_left_weak": int((weak > 0).sum())}
    print("correct_dev: %d reads in %.3f s" % (P, sec), file=sys.stderr, flush=True)
    # the baseline: the profile alone, by count() on host-sliced k-mers
    S = min(S, P)

    def profile():
        win = np.lib.stride_tricks.sliding_window_view(qs[:S], k, axis=1).reshape(-1, k)
        solid = (g.count(list(win)) >= 1).reshape(S, L - k + 1)
        cover = np.zeros((S, L + 1), np.int64)                     # positions covered by a solid window, by differences
        j = np.arange(L - k + 1)
        np.add.at(cover, (np.nonzero(solid)[0], j[np.nonzero(solid)[1]]), 1)
        np.add.at(cover, (np.nonzero(solid)[0], j[np.nonzero(solid)[1]] + k), -1)
        profile.clean = (np.cumsum(cover, 1)[:, :L] > 0).all(1)
    bsec, blo, bhi = spread(profile, lambda: None)
    out["baseline_profile_by_count"] = {"reads": S, "kmers": S * (L - k + 1), "seconds": bsec, "seconds_fastest": blo, "seconds_slowest": bhi, "reads_per_s": S / bsec,
                                        "equals_fused": bool(np.array_equal(profile.clean, (cnt[:S] == 0) & (weak[:S] == 0))),
                                        "fused_over_baseline_reads_per_s": (P / sec) / (S / bsec)}
    # correct_into: the whole index into an empty one
    dst = HipBwt(a.so)
    ts, info = [], None
    for rep in range(4):                                           # the first is the warm-up
        dst.reset()
        t = time.perf_counter(); info = g.correct_into(dst, k, 1, 8, probes); dst.sync(); ts.append(time.perf_counter() - t)
    med = float(np.median(ts[1:]))
    out["correct_into"] = {"info": info, "seconds": med, "seconds_fastest": float(min(ts[1:])), "seconds_slowest": float(max(ts[1:])), "strings_per_s": n / med,
                           "probes_per_s_at_least": n * (L - k + 1) / med, "same_index": dst.rope_hashes() == g.rope_hashes()}
    dst.close(); g.close()
    res["correct"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--so", type=int, default=1)
    ap.add_argument("--patterns", type=int, default=4_000_000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--baseline-patterns", type=int, default=200_000)
    ap.add_argument("--reads", type=int, default=0, help="reads in the index (default: the configs[1] batch)")
    ap.add_argument("--baseline-queries", type=int, default=20_000, help="queries of the host-driven SMEM baseline")
    ap.add_argument("--step-queries", type=int, default=200_000, help="queries the SMEM extension steps are counted on")
    ap.add_argument("--only", default="", help="'smem': only the smem cases (added to an existing --out file)")
    ap.add_argument("--fmd", default="", help="load the index from this .fmd file instead of building it")
    ap.add_argument("--locate", action="store_true", help="only the sampled suffix array: build and locate rates (added to an existing --out file)")
    ap.add_argument("--overlap", action="store_true", help="only the suffix-prefix overlap query (added to an existing --out file)")
    ap.add_argument("--kmers", action="store_true", help="only the k-mer enumeration (added to an existing --out file)")
    ap.add_argument("--kmer-recs", type=int, default=1 << 26, help="records fetched to host memory at the most (24 bytes each)")
    ap.add_argument("--approx", action="store_true", help="only the approximate search (added to an existing --out file)")
    ap.add_argument("--approx-queries", type=int, default=1_000_000)
    ap.add_argument("--approx-steps", type=int, default=1 << 16, help="max_steps of the approximate search")
    ap.add_argument("--approx-ed", action="store_true", help="only the approximate search with insertions and deletions, beside approx_dev (added to an existing --out file)")
    ap.add_argument("--approx-ed-queries", type=int, default=1_000_000)
    ap.add_argument("--delete", type=float, default=0.0, help="only string deletion: delete this fraction of the strings (appended to an existing --out file)")
    ap.add_argument("--contained", action="store_true", help="only the duplicate / containment query (appended to an existing --out file)")
    ap.add_argument("--contained-sample", type=int, default=1_000_000, help="strings of the sample the composition extract + backward_search is timed on")
    ap.add_argument("--irreducible", action="store_true", help="only the irreducible-overlap query (added to an existing --out file)")
    ap.add_argument("--irreducible-queries", type=int, default=1_000_000)
    ap.add_argument("--irreducible-min-ovlp", type=int, default=40)
    ap.add_argument("--irreducible-steps", type=int, default=1 << 16, help="max_steps of the irreducible-overlap query")
    ap.add_argument("--unitigs", action="store_true", help="only the unitig calls (added to an existing --out file)")
    ap.add_argument("--unitig-sample", type=int, default=20_000, help="vertices of the sample the host composition is timed on")
    ap.add_argument("--save-fmd", action="store_true", help="only the device .fmd encoder against the host writer (added to an existing --out file)")
    ap.add_argument("--merge", action="store_true", help="only unpack and merge (added to an existing --out file)")
    ap.add_argument("--graph", action="store_true", help="only the string graph on the device (added to an existing --out file)")
    ap.add_argument("--clean", action="store_true", help="only tip and bubble removal on a synthetic edge list of --reads reads (added to an existing --out file)")
    ap.add_argument("--correct", action="store_true", help="only the read correction (added to an existing --out file)")
    ap.add_argument("--correct-reads", type=int, default=1_000_000)
    ap.add_argument("--correct-sample", type=int, default=2_000, help="reads of the baseline: the profile by count() on host-sliced k-mers")
    ap.add_argument("--correct-k", type=int, default=21)
    a = ap.parse_args()
    if a.correct:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        correct_case(a, res)
        finish(a, res)
        return
    if a.clean:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        clean_case(a, res)
        finish(a, res)
        return
    if a.graph:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        graph_case(a, res)
        finish(a, res)
        return
    if a.merge:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        merge_case(a, res)
        finish(a, res)
        return
    if a.save_fmd:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        save_fmd_case(a, res)
        finish(a, res)
        return
    if a.unitigs:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        unitig_case(a, res)
        finish(a, res)
        return
    if a.irreducible:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        irreducible_case(a, res)
        finish(a, res)
        return
    if a.contained:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        contained_case(a, res)
        finish(a, res)
        return
    if a.delete > 0:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        delete_case(a, res)
        finish(a, res)
        return
    if a.approx_ed:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        approx_ed_case(a, res)
        finish(a, res)
        return
    if a.approx:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        approx_case(a, res)
        finish(a, res)
        return
    if a.kmers:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        kmers_case(a, res)
        finish(a, res)
        return
    if a.overlap:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        overlap_case(a, res)
        finish(a, res)
        return
    if a.locate:
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        locate_case(a, res)
        finish(a, res)
        return
    if a.only == "smem":
        res = {"cases": []}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        smem_case(a, res)
        finish(a, res)
        return
    L = 101
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    g = HipBwt(a.so)
    load = None
    if a.fmd:
        img = np.fromfile(a.fmd, dtype=np.uint8)
        t = time.perf_counter()
        g.load_fmd(img)
        first = time.perf_counter() - t
        sec = timed(lambda: g.load_fmd(img), lambda: None)
        load = {"file": a.fmd, "file_bytes": int(len(img)), "first_load_seconds": first, "seconds": sec, "file_gb_per_s": len(img) / sec / 1e9, "measured": True}
        build_s = first
        n = int(g.counts()[:, 0].sum())                  # strings in the index
    else:
        p = g.dev_alloc(n * (L + 1))
        t = time.perf_counter()
        g.synth_reads(p, 0, n, L, seed=42)
        g.insert_multi_dev(p, n * (L + 1))
        g.sync()
        build_s = time.perf_counter() - t
        g.dev_free(p)
    counts = g.counts()
    res = {"index": {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": int(counts.sum()), "build_seconds": build_s, "loaded_from_fmd": load,
                     "layout": g.layout_stats()}, "hbm_peak_bytes_per_s": HBM_PEAK,
           "bytes_per_rank": {"leaf_lines": LEAF_BYTES, "leaf_meta": META_BYTES, "sbrec": SB_BYTES}, "cases": []}
    P = a.patterns
    rng = np.random.RandomState(7)
    for Lp in (20, 32, 64):
        for kind in ("hits", "random"):
            pats = hit_patterns(P, Lp, n, Lp) if kind == "hits" else rng.randint(1, 5, size=(P, Lp), dtype=np.uint8)
            flat = np.ascontiguousarray(pats.reshape(-1)); off = np.arange(P + 1, dtype=np.int64) * Lp
            dp, do, dq = g.dev_alloc(len(flat)), g.dev_alloc(8 * (P + 1)), g.dev_alloc(24 * P)
            g.L.rb2_hip_memcpy(g.h, dp, flat.ctypes.data, len(flat), 0)
            g.L.rb2_hip_memcpy(g.h, do, off.ctypes.data, 8 * (P + 1), 0)
            sec = timed(lambda: g.backward_search_dev(P, dp, do, dq), g.sync)
            out = np.zeros((P, 3), np.int64)
            g.L.rb2_hip_memcpy(g.h, out.ctypes.data, dq, 24 * P, 1)
            for q in (dp, do, dq):
                g.dev_free(q)
            m = out[:, 2]
            steps = int(np.minimum(m + 1, Lp).sum())          # successful steps + the one that emptied the interval
            row = row_case("backward_search_dev L=%d %s" % (Lp, kind), P, sec, steps, 2)
            row["full_matches"] = int((m == Lp).sum())
            res["cases"].append(row)
            if Lp == 20 and kind == "hits":
                ik = np.stack([out[:, 0], out[:, 0], out[:, 1] - out[:, 0]], 1)
                res["cases"].append(row_case("extend (host buffers)", P, timed(lambda: g.extend(ik, 1), lambda: None), P, 2))
                nb = min(a.baseline_patterns, P)
                t = time.perf_counter()
                blo, bhi, bm = composed_search(g, counts, pats[:nb])
                bsec = time.perf_counter() - t
                same = bool(np.array_equal(np.stack([blo, bhi, bm], 1), out[:nb]))
                brow = row_case("baseline: backward search composed of rank_batch L=20 hits", nb, bsec, int(np.minimum(bm + 1, Lp).sum()), 2)
                brow["equals_fused"] = same
                res["cases"].append(brow)
                fused_host = timed(lambda: g.backward_search(list(pats[:nb])), lambda: None, reps=1)
                res["cases"].append(row_case("backward_search (host buffers) L=20 hits", nb, fused_host, int(np.minimum(bm + 1, Lp).sum()), 2))
    R = a.rows
    rows = np.random.RandomState(3).randint(0, n, size=R).astype(np.int64)
    fit = [0]

    def ex():
        fit[0], _, ln = g.extract_raw(rows, L)
        ex.ln = ln
    sec = timed(ex, lambda: None)
    res["cases"].append(row_case("extract (host buffers) max_len=101", R, sec, int(ex.ln.sum()) + R, 1))
    res["extract_fitted"] = fit[0]
    g.close()
    if not a.fmd:
        smem_case(a, res)
    finish(a, res)


def finish(a, res):
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
