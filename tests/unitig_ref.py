"""References of the unitig calls of include/rb2_hip.h (rb2_hip_unitig_chains, rb2_hip_unitig_text; kernels in csrc/rb2_unitig.h; DESIGN.md
section 20), two that share nothing but the definitions in the header:

  chains(n_str, edges), texts(strings, vtx, ...)  the model of the two calls: dictionaries walked link by link, texts glued from vtx
  brute_unitigs(strings, min_ovlp, ...)           edges from irreducible_ref.brute_irreducible (string slices only), paths walked over
                                                  adjacency lists, texts glued from the strings; knows no vtx

and the inputs of the tests: tile_reads(), reads that tile a random genome (optionally with a planted repeat, optionally circular), and
TILES, the two inputs whose counts test_unitig_ref.py and test_unitig_gpu.py assert.  Small inputs only.
"""
import numpy as np

import irreducible_ref as IR
from query_ref import revcomp

OFF_MAX = 1 << 48                                                    # an off or ext_in beyond this adds no piece (include/rb2_hip.h)


# ---- the model of rb2_hip_unitig_chains ----

def chains(n_str, edges):
    """(vtx (n_str, 4) int64 = head, rank, off, ext_in, info (4,) int64 = chains, cycles, vertices of the longest chain, edges ignored)"""
    edges = np.asarray(edges, np.int64).reshape(-1, 4)
    outdeg, indeg, ignored = {}, {}, 0
    live = []
    for s, d, _, e in edges.tolist():
        if not (0 <= s < n_str and 0 <= d < n_str and e >= 1):
            ignored += 1
            continue
        outdeg[s] = outdeg.get(s, 0) + 1
        indeg[d] = indeg.get(d, 0) + 1
        live.append((s, d, e))
    succ, pred = {}, {}
    for s, d, e in live:
        if outdeg[s] == 1 and indeg[d] == 1:
            succ[s] = (d, e)
            pred[d] = (s, e)
    vtx = np.zeros((n_str, 4), np.int64)
    done = np.zeros(n_str, bool)
    n_chains = n_cycles = longest = 0

    def walk(h, ext_in):
        v, rank, off = h, 0, 0
        vtx[h] = (h, 0, 0, ext_in)
        done[h] = True
        while v in succ and succ[v][0] != h:
            v, e = succ[v]
            rank, off = rank + 1, off + e
            vtx[v] = (h, rank, off, e)
            done[v] = True
        return rank + 1

    for h in range(n_str):                                          # open chains: from the vertices without a predecessor
        if h not in pred:
            longest = max(longest, walk(h, -1))
            n_chains += 1
    for h in range(n_str):                                          # what is left lies on cycles: the first id met is the smallest of its cycle
        if not done[h]:
            longest = max(longest, walk(h, pred[h][1]))
            n_chains += 1
            n_cycles += 1
    return vtx, np.array([n_chains, n_cycles, longest, ignored], np.int64)


# ---- the model of rb2_hip_unitig_text ----

def texts(strings, vtx, canonical=False, min_reads=1, fill=0):
    """(urec (k, 5) int64 = head, n_reads, text_off, text_len, flags of all selected chains, txt uint8 of their total length, info (3,) =
    selected, total, with a short piece).  Positions no piece covers (damaged rows only) hold fill"""
    vtx = np.asarray(vtx, np.int64).reshape(-1, 4)
    n = len(vtx)
    assert n == len(strings)
    members, flags = {}, {}
    for v, (h, rank, off, ext) in enumerate(vtx.tolist()):
        if not 0 <= h < n:
            h = v
            flags[h] = flags.get(h, 0) | 2
        elif h == v and ext >= 1:
            flags[h] = flags.get(h, 0) | 1
        members.setdefault(h, []).append(v)
    urec, parts, toff = [], [], 0
    for h in sorted(members):
        vs = members[h]
        if len(vs) < min_reads or (canonical and min(vs) % 2):
            continue
        head = np.asarray(strings[h], np.uint8)
        pieces, last, fl = [], 0, flags.get(h, 0)
        for v in vs:
            _, _, off, ext = vtx[v].tolist()
            if v == h:
                continue
            if not (0 <= off <= OFF_MAX and 0 <= ext <= OFF_MAX):
                fl |= 2
                continue
            last = max(last, off)
            pieces.append((v, off, ext))
        t = np.full(len(head) + last, fill, np.uint8)
        t[:len(head)] = head
        for v, off, ext in pieces:
            s = np.asarray(strings[v], np.uint8)
            end = len(head) + off
            if ext > len(s):
                fl |= 2
                s = np.concatenate([np.zeros(ext - len(s), np.uint8), s])
            piece = s[len(s) - ext:]
            lo = max(end - ext, 0)
            t[lo:end] = piece[lo - (end - ext):]
        urec.append((h, len(vs), toff, len(t), fl))
        parts.append(t)
        toff += len(t)
    urec = np.array(urec, np.int64).reshape(-1, 5)
    txt = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return urec, txt, np.array([len(urec), toff, int(((urec[:, 4] & 2) != 0).sum())], np.int64)


def unitigs_of(strings, vtx, canonical=True, min_reads=1):
    """what HipBwt.unitigs returns, from the model: [(text bytes, read ids in chain order, circular), ...] by increasing head id"""
    urec, txt, _ = texts(strings, vtx, canonical, min_reads)
    vtx = np.asarray(vtx, np.int64)
    out = []
    for h, k, o, l, fl in urec.tolist():
        vs = np.flatnonzero(vtx[:, 0] == h)
        out.append((txt[o:o + l].tobytes(), vs[np.argsort(vtx[vs, 1])].tolist(), bool(fl & 1)))
    return out


# ---- brute force: string slices and adjacency lists ----

def brute_edges(strings, min_ovlp, max_ext=1000):
    """the rows src, dst, l, ext of HipBwt.edges(pairs=True), sorted: the irreducible neighbours of every string by the definition"""
    return sorted((i, k, l, e) for i, s in enumerate(strings) for k, l, e in (IR.brute_irreducible(strings, s, min_ovlp, max_ext) or ()))


def brute_unitigs(strings, min_ovlp, max_ext=1000, canonical=True, min_reads=1):
    """[(text bytes, read ids in chain order, circular), ...] by increasing head id"""
    n = len(strings)
    out, inn = [[] for _ in range(n)], [[] for _ in range(n)]
    for i, k, _, e in brute_edges(strings, min_ovlp, max_ext):
        out[i].append((k, e))
        inn[k].append(i)

    def nxt(u):
        return out[u][0] if len(out[u]) == 1 and len(inn[out[u][0][0]]) == 1 else None

    def has_prev(v):
        return len(inn[v]) == 1 and len(out[inn[v][0]]) == 1

    seen, res = set(), []
    for s in [v for v in range(n) if not has_prev(v)] + list(range(n)):   # the open paths from their first vertices, then the cycles from their smallest ids
        if s in seen:
            continue
        path, text, u, circ = [s], [np.asarray(strings[s], np.uint8)], s, False
        seen.add(s)
        while True:
            x = nxt(u)
            if x is None:
                break
            if x[0] == s:
                circ = True
                break
            u, e = x
            t = np.asarray(strings[u], np.uint8)
            text.append(t[len(t) - e:])
            path.append(u)
            seen.add(u)
        if len(path) >= min_reads and not (canonical and min(path) % 2):
            res.append((np.concatenate(text).tobytes(), path, circ))
    return sorted(res, key=lambda r: r[1][0])


# ---- the inputs ----

def tile_reads(seed, glen, lo, hi, smax, repeat=None, circular=False):
    """(genome, reads): reads of lo .. hi symbols that start 1 .. smax apart along a random genome; repeat = (a, b, L) copies genome[a:a+L]
    to b first; circular: the reads run on round the end of the genome until a start passes it"""
    r = np.random.RandomState(seed)
    g = r.randint(1, 5, size=glen).astype(np.uint8)
    if repeat:
        a, b, L = repeat
        g[b:b + L] = g[a:a + L]
    reads, p = [], 0
    while True:
        L = r.randint(lo, hi + 1)
        if (p >= glen) if circular else (p + L > glen):
            break
        reads.append(g[(p + np.arange(L)) % glen].copy())
        p += r.randint(1, smax + 1)
    return g, reads


def drop_contained(reads):
    """the reads that are no copy of an earlier read and lie inside no other read or its reverse complement"""
    b = [np.asarray(r, np.uint8).tobytes() for r in reads]
    rc = [revcomp(r).tobytes() for r in reads]
    keep = []
    for i, s in enumerate(b):
        inside = any(j != i and (s in b[j] or s in rc[j]) and (len(b[j]) > len(s) or j < i) for j in range(len(b)))
        if not inside:
            keep.append(reads[i])
    return keep


def both_strands(reads):
    """strings 2i, 2i + 1 = read i and its reverse complement"""
    return [s for r in reads for s in (np.asarray(r, np.uint8), revcomp(r))]


TILE = dict(seed=5, glen=600, lo=40, hi=60, smax=7)
MIN_OVLP, MAX_EXT = 20, 1000
# name: (repeat, strings, edges, chains, the canonical unitigs as (reads, length))
TILES = {"plain": (None, 156, 154, 2, [(78, 600)]),
         "repeat": ((100, 400, 30), 156, 158, 10, [(9, 129), (4, 72), (38, 322), (4, 76), (23, 200)])}


def tile_case(name, circular=False):
    """(genome, the reads as generated, the strings of the reduced index of both strands)"""
    g, reads = tile_reads(repeat=TILES[name][0], circular=circular, **TILE)
    return g, reads, both_strands(drop_contained(reads))
