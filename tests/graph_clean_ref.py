"""References of rb2_hip_graph_clean (include/rb2_hip.h; kernels in csrc/rb2_clean.h), two that share nothing but the
definitions in the header:

  clean_round(n_str, rows, alive, ...), clean(...)  the model: unitig_ref.chains and flat per-vertex, per-head arrays, the arithmetic
                                                    of the kernels
  brute_clean(...)                                  adjacency lists, paths walked vertex by vertex in the manner of
                                                    unitig_ref.brute_unitigs; knows no vtx

and the inputs of the tests: error_reads(), reads with planted substitutions that make tips and bubbles on the tiles of unitig_ref, and
backbone(), an edge list of both strands with tips and bubbles that needs no index.  Small inputs only.
"""
import numpy as np

import unitig_ref as U

TIP, BUBBLE = 1, 2                                                   # why a row was removed


def _valid(n_str, rows):
    return (rows[:, 0] >= 0) & (rows[:, 0] < n_str) & (rows[:, 1] >= 0) & (rows[:, 1] < n_str) & (rows[:, 3] >= 1)


# ---- the model ----

def clean_round(n_str, rows, alive, max_tip_reads, max_bubble_reads, pairs):
    """one round on the rows rows[alive] (all valid): (m,) uint8, TIP or BUBBLE for the rows this round removes, 0 elsewhere"""
    n, idx = n_str, np.flatnonzero(alive)
    sub = rows[idx]
    src, dst = sub[:, 0], sub[:, 1]
    vtx, _ = U.chains(n, sub)
    head, rank = vtx[:, 0], vtx[:, 1]
    outdeg, indeg = np.bincount(src, minlength=n), np.bincount(dst, minlength=n)
    inedge, outedge = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    inedge[dst] = src                                               # (read only where indeg == 1)
    outedge[src] = dst                                              # (read only where outdeg == 1)
    reads = np.bincount(head, minlength=n)
    minpid = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(minpid, head, np.arange(n, dtype=np.int64) >> pairs)
    tail = np.full(n, -1, np.int64)
    last = rank == reads[head] - 1
    tail[head[last]] = np.flatnonzero(last)
    is_head = (head == np.arange(n)) & (vtx[:, 3] < 1)              # heads of open chains; cycles take no part
    t = np.where(is_head, tail, 0)
    out_tip = is_head & (outdeg[t] == 0) & (indeg >= 1) & (reads <= max_tip_reads)
    in_tip = is_head & (indeg == 0) & (outdeg[t] >= 1) & (reads <= max_tip_reads)
    in_tip_tail = np.zeros(n, bool)
    in_tip_tail[tail[in_tip]] = True
    p, q = np.where(is_head & (indeg == 1), inedge, 0), np.where(is_head, outedge[t], 0)
    q = np.where(q < 0, 0, q)
    arm = is_head & (indeg == 1) & (outdeg[t] == 1) & (outdeg[p] >= 2) & (indeg[q] >= 2)
    lose = np.zeros(n, bool)
    groups = {}
    for h in np.flatnonzero(arm).tolist():
        groups.setdefault((int(p[h]), int(q[h])), []).append(h)
    for hs in groups.values():
        keys = [(int(reads[h]), -int(minpid[h])) for h in hs]
        best = max(keys)
        for h, k in zip(hs, keys):
            lose[h] = reads[h] <= max_bubble_reads and best > k
    lose_tail = np.zeros(n, bool)
    lose_tail[tail[lose]] = True
    anchor_out, anchor_in = np.zeros(n, bool), np.zeros(n, bool)
    anchor_out[src[~out_tip[dst]]] = True                           # has a way out that is no out-tip
    anchor_in[dst[~in_tip_tail[src]]] = True                        # has a way in that is no in-tip
    tip = (out_tip[dst] & anchor_out[src]) | (in_tip_tail[src] & anchor_in[dst])
    bub = lose[dst] | lose_tail[src]
    why = np.zeros(len(rows), np.uint8)
    why[idx] = np.where(tip, TIP, np.where(bub, BUBBLE, 0))
    return why


def clean(n_str, edges, max_tip_reads=2, max_bubble_reads=3, pairs=1, max_rounds=8):
    """(the rows kept (m', 4) int64, info (8,) int64 = m', m', rounds run, tip rows, bubble rows, rows ignored, chains of the rows kept, 0):
    what rb2_hip_graph_clean returns with cap >= m'"""
    rows = np.asarray(edges, np.int64).reshape(-1, 4)
    alive = _valid(n_str, rows)
    ignored, rounds, tips, bubbles = int((~alive).sum()), 0, 0, 0
    while rounds < max_rounds:
        why = clean_round(n_str, rows, alive, max_tip_reads, max_bubble_reads, 1 if pairs else 0)
        rounds += 1
        if not why.any():
            break
        tips, bubbles = tips + int((why == TIP).sum()), bubbles + int((why == BUBBLE).sum())
        alive = alive & (why == 0)
    out = rows[alive].copy()
    return out, np.array([len(out), len(out), rounds, tips, bubbles, ignored, U.chains(n_str, out)[1][0], 0], np.int64)


# ---- brute force: adjacency lists and paths ----

def _paths(n, out, inn):
    """the open paths of the graph, each a list of vertices from its first to its last"""
    def nxt(u):
        return out[u][0][0] if len(out[u]) == 1 and len(inn[out[u][0][0]]) == 1 else None

    def has_prev(v):
        return len(inn[v]) == 1 and len(out[inn[v][0][0]]) == 1

    res = []
    for s in range(n):
        if has_prev(s):
            continue
        path, u = [s], s
        while nxt(u) is not None:
            u = nxt(u)
            path.append(u)
        res.append(path)
    return res


def brute_clean(n_str, edges, max_tip_reads=2, max_bubble_reads=3, pairs=1, max_rounds=8):
    """(the rows kept as a list of tuples in input order, rounds run, tip rows, bubble rows, rows ignored)"""
    rows = [tuple(r) for r in np.asarray(edges, np.int64).reshape(-1, 4).tolist()]
    alive = [e for e, (s, d, _, x) in enumerate(rows) if 0 <= s < n_str and 0 <= d < n_str and x >= 1]
    ignored, rounds, tips, bubbles = len(rows) - len(alive), 0, 0, 0
    sh = 1 if pairs else 0
    while rounds < max_rounds:
        rounds += 1
        out, inn = [[] for _ in range(n_str)], [[] for _ in range(n_str)]
        for e in alive:
            out[rows[e][0]].append((rows[e][1], e))
            inn[rows[e][1]].append((rows[e][0], e))
        paths = _paths(n_str, out, inn)
        short = [c for c in paths if len(c) <= max_tip_reads]
        out_heads = {c[0] for c in short if not out[c[-1]] and inn[c[0]]}
        in_tails = {c[-1] for c in short if not inn[c[0]] and out[c[-1]]}
        gone = {}
        for h in out_heads:
            for p, e in inn[h]:
                if any(d not in out_heads for d, _ in out[p]):
                    gone[e] = TIP
        for t in in_tails:
            for w, e in out[t]:
                if any(s not in in_tails for s, _ in inn[w]):
                    gone[e] = TIP
        arms = {}
        for c in paths:
            if len(inn[c[0]]) == 1 and len(out[c[-1]]) == 1:
                (p, e_in), (q, e_out) = inn[c[0]][0], out[c[-1]][0]
                if len(out[p]) >= 2 and len(inn[q]) >= 2:
                    arms.setdefault((p, q), []).append(((len(c), -min(v >> sh for v in c)), e_in, e_out))
        for group in arms.values():
            for key, e_in, e_out in group:
                if key[0] <= max_bubble_reads and any(k > key for k, _, _ in group):
                    gone.setdefault(e_in, BUBBLE)
                    gone.setdefault(e_out, BUBBLE)
        if not gone:
            break
        tips += sum(1 for w in gone.values() if w == TIP)
        bubbles += sum(1 for w in gone.values() if w == BUBBLE)
        alive = [e for e in alive if e not in gone]
    return [rows[e] for e in alive], rounds, tips, bubbles, ignored


# ---- the inputs ----

def error_reads(reads, n_tip, n_bub, seed):
    """the strings of the reduced index of both strands of reads plus n_tip copies with a substitution 2 .. 8 symbols before their end and
    n_bub copies of reads of >= 57 symbols with a substitution in their middle"""
    r = np.random.RandomState(seed)
    extra = []
    for _ in range(n_tip):
        i = r.randint(5, len(reads) - 5)
        x = reads[i].copy()
        p = len(x) - 1 - r.randint(2, 8)
        x[p] = x[p] % 4 + 1
        extra.append(x)
    long = [k for k in range(5, len(reads) - 5) if len(reads[k]) >= 57]
    for _ in range(n_bub):
        i = long[r.randint(len(long))]
        x = reads[i].copy()
        p = len(x) // 2
        x[p] = x[p] % 4 + 1
        extra.append(x)
    return U.both_strands(U.drop_contained(reads + extra))


def backbone(n, tips=(), bubbles=()):
    """(n_str, edges (m, 4) int64): reads 0 .. n-1 in a row, vertex 2i read i forward and 2i + 1 its reverse complement, i -> i + 1 on the
    forward strand and every row u -> v with its mirror v^1 -> u^1 behind it.  tips: (i, k) hangs k > 0 new reads off read i as a dead
    end that leaves it, k < 0 as one that enters it.  bubbles: (i, span, k) adds an arm of k new reads from read i to read i + span + 1
    beside the span backbone reads between them.  New reads are numbered from n on in the order given"""
    rows, nxt = [], [n]

    def edge(a, b):                                                 # read a -> read b on the forward strand
        u, v = 2 * a, 2 * b
        ext = 5 + (a + 3 * b) % 7
        rows.append((u, v, 50, ext))
        rows.append((v ^ 1, u ^ 1, 50, 11 - ext + 5))

    def fresh(k):
        ids = list(range(nxt[0], nxt[0] + k))
        nxt[0] += k
        return ids

    for i in range(n - 1):
        edge(i, i + 1)
    for i, k in tips:
        ids = fresh(abs(k))
        path = [i] + ids if k > 0 else ids + [i]
        for a, b in zip(path, path[1:]):
            edge(a, b)
    for i, span, k in bubbles:
        path = [i] + fresh(k) + [i + span + 1]
        for a, b in zip(path, path[1:]):
            edge(a, b)
    return 2 * nxt[0], np.array(rows, np.int64).reshape(-1, 4)
