"""Throughput of the FM-index query kernels (k_bsearch, k_extend, k_extract; csrc/rb2_query.h) on a configs[1]-sized index.

Builds the first configs[1] batch on the device (40.8 M x 101 bp synthetic reads, RLO by default, the generator of
tests/test_hip_parity.py::test_full_batch_properties), then times, after a warm-up, with a host clock around a synchronise:
  - backward_search_dev on P patterns of length 20, 32 and 64: substrings of the reads (hits) and uniform random patterns (mostly misses);
  - extend (host variant) on P bi-intervals;
  - extract (host variant) on R rows;
  - the baseline: the same backward search composed from rb2_hip_rank_batch calls (what a user could do before), on fewer patterns.
For each case: queries/s, LF steps/s (one step = the ranks at both ends of an interval, or one LF of a walk), the bytes a step touches
by the layout, and steps/s x bytes against the 8 TB/s HBM peak.  One JSON document on stdout and in --out.

    python tools/query_bench.py --out profiles/query_bench.json [--so 1] [--patterns 4000000] [--rows 1000000]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--so", type=int, default=1)
    ap.add_argument("--patterns", type=int, default=4_000_000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--baseline-patterns", type=int, default=200_000)
    ap.add_argument("--reads", type=int, default=0, help="reads in the index (default: the configs[1] batch)")
    a = ap.parse_args()
    L = 101
    n = a.reads or -(-(int(4 * 1024 ** 3 * 0.97) + 1) // (L + 1))
    g = HipBwt(a.so)
    p = g.dev_alloc(n * (L + 1))
    t = time.perf_counter()
    g.synth_reads(p, 0, n, L, seed=42)
    g.insert_multi_dev(p, n * (L + 1))
    g.sync()
    build_s = time.perf_counter() - t
    g.dev_free(p)
    counts = g.counts()
    res = {"index": {"reads": n, "read_len": L, "sorting_order": a.so, "symbols": int(counts.sum()), "build_seconds": build_s,
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
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
