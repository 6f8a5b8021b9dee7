"""Model-based sequence tests of one handle (tests/test_op_sequences_ref.py, tests/test_op_sequences_gpu.py, tools/fuzz_ops.py).

A script is data: a list of small records, one per operation, applied in lockstep to a CPU model of "the strings an index holds" and to a
handle; after every step the handle is compared with the model, exactly.  The model is the oracle plus the references the suite already
holds against brute force (delete_ref, merge_ref, query_ref, locate_ref, contain_ref, the host .fmd writer): an insert is an oracle rebuild
from the walks of the model's BWT followed by the batch, as tests/test_delete_gpu.py::expect does.

The checks come in two kinds.  The quiet ones are queries and host-side state only: they leave the layout alone (layout_stats() is compared
around them), so a sparse index stays sparse for the next operation.  The full ones download the ropes and encode the .fmd, which settles a
sparse index; they run where a script marks a step with "full", and at its end.

Nothing here needs a GPU: the handle comes from the `make` callable, and without one the runner drives the model alone."""
import json
import os
import tempfile

import numpy as np

import contain_ref as CR
import delete_ref as D
import fmd_save_ref as FS
import helpers as H
import locate_ref as LR
import merge_ref as MR
import query_ref as Q
from ropebwt2_amd.hipbwt import encode_runs

PROFILES = ("default", "sparse", "dense")
INSERTS = ("insert_host", "insert_dev", "insert_prefetched", "insert_registered")
KINDS = INSERTS + ("delete", "merge_from", "load_ropes", "load_fmd", "save_then_load_self", "reset", "ssa_build", "ssa_drop", "reserve", "settle")
PLANS = tuple(range(1, 11))
NEEDS_AUX = (5, 6, 9)
MAX_ROWS = 200000
EMPTY_FMD = 216                                                      # the image of an index without rows (include/rb2_hip.h)
FILL = 0xA5


def counts_of(bwt):
    """the 6 x 6 count matrix of a BWT: [b, a] = the a's in rope b, the rows that begin with b"""
    bwt = np.asarray(bwt, np.uint8)
    cut = np.concatenate([[0], np.cumsum(np.bincount(bwt, minlength=6))])
    return np.array([np.bincount(bwt[cut[b]:cut[b + 1]], minlength=6) for b in range(6)], np.int64)


def strings_of(buf):
    """the strings of an insert buffer in text order, in the order they are inserted"""
    buf = np.asarray(buf, np.uint8)
    ends = np.flatnonzero(buf == 0)
    return [buf[a:b][::-1].copy() for a, b in zip(np.concatenate([[0], ends[:-1] + 1]), ends)]


def cut_at_sentinel(buf, at):
    """the smallest length >= at at which buf may be cut: just behind a sentinel"""
    ends = np.flatnonzero(buf == 0) + 1
    return int(ends[np.searchsorted(ends, max(at, 1))]) if len(ends) else 0


class Model:
    """the BWT and the count matrix of the strings an index must hold"""

    def __init__(self, so):
        self.so = so
        self.bwt = np.zeros(0, np.uint8)
        self.cnt = np.zeros((6, 6), np.int64)
        self._memo = {}

    def _set(self, bwt, cnt=None):
        self.bwt = np.ascontiguousarray(bwt, np.uint8)
        self.cnt = counts_of(self.bwt)
        assert cnt is None or np.array_equal(cnt, self.cnt), "the oracle's count matrix is not that of its BWT"
        self._memo = {}

    def _rebuild(self, bufs):
        o = H.Oracle(self.so)
        for b in bufs:
            if len(b):
                o.insert_multi(b)
        bwt, cnt = o.bwt(), o.counts()
        o.close()
        self._set(bwt, cnt)

    def _cached(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    # -- what the index holds -------------------------------------------------------------------------------------------------------
    @property
    def rows(self):
        return len(self.bwt)

    @property
    def n(self):
        return int(self.cnt[:, 0].sum())

    def walks(self):
        """the strings in id order, last symbol first"""
        return self._cached("walks", lambda: D.walks(self.bwt))

    def buffer(self):
        return D.buffer_of(self.walks())

    def fm(self):
        return self._cached("fm", lambda: Q.FM(self.bwt))

    def ropes(self):
        cut = np.concatenate([[0], np.cumsum(self.cnt.sum(1))])
        return [self.bwt[cut[b]:cut[b + 1]] for b in range(6)]

    def rles(self):
        return [encode_runs(r) for r in self.ropes()]

    def image(self):
        """the .fmd the host writer gives for these ropes"""
        def write():
            fd, path = tempfile.mkstemp(suffix=".fmd")
            os.close(fd)
            try:
                return FS.write_fmd(path, self.rles())
            finally:
                os.unlink(path)
        return self._cached("image", write)

    # -- the operations ---------------------------------------------------------------------------------------------------------------
    def insert(self, buf):
        """returns what the batch adds to the count matrix"""
        before = self.cnt
        self._rebuild([self.buffer(), np.asarray(buf, np.uint8)])
        return self.cnt - before

    def delete(self, ids):
        """returns the rows removed"""
        ids = np.asarray(ids, np.int64).reshape(-1)
        if len(ids) == 0:
            return 0
        rows = D.delete(self.bwt, ids)[1]
        self._rebuild([D.buffer_of(D.survivors(self.bwt, ids))])
        return rows

    def merge(self, other):
        self._rebuild([self.buffer(), other.buffer()])

    def load(self, other):
        self._set(other.bwt.copy())

    def reset(self):
        self._set(np.zeros(0, np.uint8))


# ---- batches: a record that names the reads; copies of indexed strings are drawn from the model when the batch is made -----------------

def batch_spec(rng, dup=True, small=False):
    kind = str(rng.choice(["fixed", "var", "repet"], p=[.35, .35, .3]))
    both = int(rng.rand() < 0.4)
    spec = {"kind": kind, "seed": int(rng.randint(1, 1 << 30)), "n": int(rng.randint(50, 60 if small else 401)), "both": both}
    if kind == "fixed":
        spec["len"] = int(rng.choice([1, 2, 17, 50, 101, 150]))
    elif kind == "repet":
        spec["len"] = int(rng.choice([20, 60, 150]))
        spec["genome"] = max(int(rng.choice([60, 300, 2000])), spec["len"] + 10)
    else:
        spec["len"] = 150
    spec["n"] = max(50, min(spec["n"], 18000 // ((spec["len"] + 1) * (1 + both))))      # (a batch stays below some 18 000 rows)
    spec["dup"] = int(rng.randint(1, 40)) if dup and rng.rand() < 0.6 else 0
    return spec


def make_reads(spec, indexed=()):
    """the reads of a batch in text order; indexed: the walks of the strings the index holds (copies of some of them join the batch)"""
    rng = np.random.RandomState(spec["seed"])
    n, kind = spec["n"], spec["kind"]
    if kind == "fixed":
        reads = list(H.splitmix_bases(n, spec["len"], seed=spec["seed"]))
    elif kind == "repet":
        reads = H.repetitive_reads(n, seed=spec["seed"] % (1 << 20), genome_len=spec["genome"], max_len=spec["len"])
    else:
        lens = rng.choice([0, 1, 3, 30, 90, 150], p=[.05, .1, .1, .3, .35, .1], size=n)
        reads = [rng.randint(1, 6, size=int(l)).astype(np.uint8) for l in lens]
    if spec.get("dup") and len(indexed):
        reads = reads + [np.asarray(indexed[i], np.uint8)[::-1].copy() for i in rng.randint(0, len(indexed), size=spec["dup"])]
    return reads


def make_batch(spec, indexed=()):
    return H.encode_batch(make_reads(spec, indexed), True, bool(spec["both"]))


def other_content(buf):
    """a different batch of the same length with its sentinels in the same places: every ACGT complemented"""
    buf = np.asarray(buf, np.uint8)
    return np.where((buf >= 1) & (buf <= 4), 5 - buf, buf).astype(np.uint8)


# ---- the runner ------------------------------------------------------------------------------------------------------------------------

def show(script, step=None):
    """a script as text that can be pasted into a pinned case"""
    head = {k: v for k, v in script.items() if k not in ("ops", "buffers")}
    lines = ["script = dict(%s, ops=[" % ", ".join("%s=%s" % (k, json.dumps(v)) for k, v in head.items())]
    for i, op in enumerate(script["ops"]):
        lines.append("    %s,%s" % (json.dumps(op), "      # <-- step %d" % i if i == step else ""))
    return "\n".join(lines + ["])"])


class StepFailed(AssertionError):
    pass


class Runner:
    """applies operations to the model and, when make is given, to the handle make() returns; make is called again for the source handle
    of every merge.  The script supplies so, seed, sides (the batch records of the side models) and, for pinned cases, buffers (named
    insert buffers an operation may use in place of a batch record)."""

    def __init__(self, script, make=None):
        self.script = script
        self.so = script["so"]
        self.make = make
        self.m = Model(self.so)
        self.g = make() if make else None
        self.plain = []                                             # the strings by a plain list: text order, id order in input order
        self.sides = {}
        self.srcs = {}
        self.ssa = False                                            # must a sampled suffix array be valid now
        self.old_size = None                                        # SIZE as the previous full check obtained it
        self.grown = 0                                              # how often a prefetch buffer was made to grow
        self.steps = 0
        self.max_rows = 0
        self.rows_changed_while_valid = 0
        self.fulls = []                                             # the steps full checks ran at
        self.row_changes = []                                       # the steps that changed rows

    def close(self):
        for s in self.srcs.values():
            s.close()
        self.srcs = {}
        if self.g is not None:
            self.g.close()
            self.g = None

    # -- the side models and their handles ------------------------------------------------------------------------------------------
    def side_buffer(self, k):
        """the insert buffer of side model k: made from its batch record, a named buffer of a pinned case, or nothing at all (None)"""
        b = self.script["sides"][k]
        if b is None:
            return np.zeros(0, np.uint8)
        return np.ascontiguousarray(self.script["buffers"][b], np.uint8) if isinstance(b, str) else make_batch(b)

    def side(self, k):
        if k not in self.sides:
            m = Model(self.so)
            if len(self.side_buffer(k)):
                m.insert(self.side_buffer(k))
            self.sides[k] = m
        return self.sides[k]

    def source(self, k):
        """a second handle that holds side model k, built in two inserts (so that it may be sparse) and with a sampled suffix array"""
        if k not in self.srcs:
            buf = self.side_buffer(k)
            at = cut_at_sentinel(buf, len(buf) // 2)
            s = self.make()
            for part in (buf[:at], buf[at:]):
                if len(part):
                    s.insert_multi(part)
            s.build_ssa(4)
            self.srcs[k] = s
        return self.srcs[k]

    def buffer_of_op(self, op, key="batch"):
        b = op[key]
        if isinstance(b, str):
            return np.ascontiguousarray(self.script["buffers"][b], np.uint8)
        return make_batch(b, self.m.walks())

    # -- primitive steps on both sides -------------------------------------------------------------------------------------------------
    def _plain_delete(self, ids):
        ids = np.unique(np.asarray(ids, np.int64).reshape(-1))
        if self.so == 0:
            gone = set(ids.tolist())
            self.plain = [s for i, s in enumerate(self.plain) if i not in gone]
        else:                                                       # (a sorted order: the model says which strings the ids name)
            w = self.m.walks()
            gone = {}
            for i in ids.tolist():
                t = w[i][::-1].tobytes()
                gone[t] = gone.get(t, 0) + 1
            keep = []
            for s in self.plain:
                t = s.tobytes()
                if gone.get(t, 0):
                    gone[t] -= 1
                else:
                    keep.append(s)
            assert not any(gone.values()), "the model names a string the plain list does not hold"
            self.plain = keep

    def _insert(self, content, call, host=True):
        """the model takes content; call() hands it to the handle; last_batch_counts() must be the model's delta at once"""
        content = np.ascontiguousarray(content, np.uint8).copy()
        delta = self.m.insert(content)
        self.plain += strings_of(content)
        if self.g is not None:
            call()
            got = self.g.last_batch_counts()
            if host:
                assert got is not None and np.array_equal(got, delta), "last_batch_counts() is not what the batch adds: %s" % (None if got is None else (got - delta).tolist())
            else:
                assert got is None, "last_batch_counts() answers behind a device insert"
        return True

    def _delete(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        self._plain_delete(ids)
        rows = self.m.delete(ids)
        if self.g is not None:
            assert self.g.delete(ids) == rows, "rows removed"
            if len(ids):
                assert self.g.delete_stats()["rows_removed"] == rows
        return len(ids) > 0

    def _load(self, k, how):
        side = self.side(k)
        if self.g is not None:
            if how == "load_ropes":
                self.g.load_ropes(side.rles())
            else:
                assert self.g.load_fmd(side.image()) == side.rows, "symbols loaded"
        self.m.load(side)
        self.plain = [w[::-1].copy() for w in side.walks()]
        return True

    def _reset(self):
        if self.g is not None:
            self.g.reset()
        self.m.reset()
        self.plain = []
        return True

    def _prefetched(self, op):
        """the ten prefetch plans (all on the calling thread): what the handle is told, and what it must hold afterwards"""
        g, plan = self.g, op["plan"]
        s_buf = self.buffer_of_op(op)
        t_buf = self.buffer_of_op(op, "aux") if plan in NEEDS_AUX else None
        ln = len(s_buf)
        cap = max(ln, len(t_buf) if t_buf is not None else 0) + 16
        s = np.zeros(cap, np.uint8)
        s[:ln] = s_buf
        t = None
        if t_buf is not None and plan != 9:
            t = np.zeros(cap + 4096, np.uint8)
            t[:len(t_buf)] = t_buf
        reg = [a for a in (s, t) if a is not None] if op.get("reg") and g is not None else []
        for a in reg:
            assert g.L.rb2_hip_host_register(a.ctypes.data, a.nbytes) == 0, "rb2_hip_host_register"

        def pf(a, n, c):
            if g is not None:
                g.L.rb2_hip_prefetch(g.h, a.ctypes.data, n, c)

        def ins(a, n):
            self._insert(a[:n], lambda: g.L.rb2_hip_insert_multi(g.h, n, a.ctypes.data))

        if g is not None:
            g.set_lazy(op.get("lazy", 1))
        if plan == 1:                                               # everything is over before the insert
            pf(s, ln, ln); ins(s, ln)
        elif plan == 2:                                             # in three parts: pf_done advances
            pf(s, ln // 3, ln); pf(s, 2 * ln // 3, ln); ins(s, ln)
        elif plan == 3:                                             # a capacity below the batch: the second buffer may be too small at the insert
            pf(s, ln // 2, ln // 2); ins(s, ln)
        elif plan == 4:                                             # the second announcement makes the buffer grow: it starts over from byte 0
            self.grown += 1
            pf(s, ln // 4, ln // 4); pf(s, ln // 2, (4 << 20) << self.grown); ins(s, ln)
        elif plan == 5:                                             # another buffer is inserted in between: what was prefetched is overwritten
            pf(s, ln, ln); ins(t, len(t_buf)); ins(s, ln)
        elif plan == 6:                                             # a stale pointer: another, longer buffer was announced
            pf(t, len(t_buf), len(t_buf)); ins(s, ln)
        elif plan == 7:                                             # cancelled, then the same memory holds another batch of the same length
            pf(s, ln, ln)
            if g is not None:
                g.L.rb2_hip_prefetch(g.h, None, 0, 0)
            s[:ln] = other_content(s_buf)
            ins(s, ln)
        elif plan == 8:                                             # more was announced than the insert takes: pf_done > len
            pf(s, ln, ln); ins(s, cut_at_sentinel(s_buf, ln // 2))
        elif plan == 9:                                             # one read buffer for two consecutive batches, each prefetched
            first, second = sorted([s_buf, t_buf], key=len)        # (the longer one second: a pf_done left over from the first would be taken for its head)
            s[:len(first)] = first
            pf(s, len(first), cap); ins(s, len(first))
            s[:len(second)] = second
            pf(s, len(second), cap); ins(s, len(second))
        elif plan == 10:                                            # the rows change between the prefetch and the insert
            pf(s, ln, ln); self._apply(op["mid"]); ins(s, ln)
        else:
            raise ValueError("no prefetch plan %r" % (plan,))
        for a in reg:
            assert g.L.rb2_hip_host_unregister(a.ctypes.data) == 0, "rb2_hip_host_unregister"
        return True

    def _merge(self, op):
        side = self.side(op["k"])
        if self.g is not None:
            src = self.source(op["k"])
            lay = src.layout_stats()
            info = self.g.merge(src, op["batch_bytes"])
            assert info[0] == side.n and info[1] == side.rows - side.n, "merge reports %s" % (info,)
            assert info[2] >= op.get("min_batches", 3) and info[3] <= max(op["batch_bytes"], max(len(w) + 1 for w in side.walks())), "merge reports %s" % (info,)
            assert src.layout_stats() == lay, "the source of a merge changed its layout"
            assert src.ssa_info()["valid"], "the source of a merge lost its sampled suffix array"
            txt, off = src.unpack_raw()
            wt, wo = MR.unpack(side.bwt)
            assert np.array_equal(off, wo) and np.array_equal(txt, wt), "the source of a merge holds other strings"
            assert src.layout_stats() == lay
        self.m.merge(side)
        self.plain += [w[::-1].copy() for w in side.walks()]
        return True

    def _apply(self, op):
        """-> did the rows change (or may the call count as a change of rows: a load of the same rows does)"""
        k, g = op["op"], self.g
        if k == "insert_host":
            buf = self.buffer_of_op(op)
            if g is not None:
                g.set_lazy(op.get("lazy", 1))
            return self._insert(buf, lambda: g.insert_multi(buf))
        if k == "insert_registered":
            buf = self.buffer_of_op(op)

            def call():
                assert g.L.rb2_hip_host_register(buf.ctypes.data, buf.nbytes) == 0, "rb2_hip_host_register"
                g.insert_multi(buf)
                assert g.L.rb2_hip_host_unregister(buf.ctypes.data) == 0, "rb2_hip_host_unregister"
            return self._insert(buf, call)
        if k == "insert_dev":
            buf = self.buffer_of_op(op)

            def call():
                p = g.dev_alloc(len(buf) + 128)
                q = p + op["misalign"]                          # (1: not 16-byte aligned, the engine stages it through its own text buffer)
                g.L.rb2_hip_memcpy(g.h, q, buf.ctypes.data, len(buf), 0)
                g.insert_multi_dev(q, len(buf))
                g.dev_free(p)
            return self._insert(buf, call, host=False)
        if k == "insert_prefetched":
            return self._prefetched(op)
        if k == "delete":
            return self._delete(op["ids"])
        if k == "merge_from":
            return self._merge(op)
        if k in ("load_ropes", "load_fmd"):
            return self._load(op["k"], k)
        if k == "save_then_load_self":
            if g is not None:
                img = g.save_fmd()
                assert np.array_equal(img, self.m.image()), "save_fmd() is not the host writer's image"
                assert g.load_fmd(img) == self.m.rows
            return True
        if k == "reset":
            return self._reset()
        if k == "ssa_build":
            if g is not None:
                assert g.build_ssa(op["step"]) == (self.m.rows + (1 << op["step"]) - 1) >> op["step"], "samples"
            return False
        if k == "ssa_drop":
            if g is not None:
                g.drop_ssa()
            return False
        if k == "reserve":
            if g is not None:
                g.reserve(op["bytes"], op["strings"], op["symbols"])
            return False
        if k == "settle":
            if g is not None:
                g.rope_hashes()
            return False
        raise ValueError("no operation %r" % (k,))

    # -- a step: the operation, then the checks -------------------------------------------------------------------------------------
    def step(self, op):
        i = self.steps
        self.steps += 1
        try:
            was_valid = self.ssa
            changed = self._apply(op)
            k = op["op"]
            if changed:
                self.row_changes.append(i)
                self.rows_changed_while_valid += int(was_valid)
                self.ssa = False
            if k == "ssa_build":
                self.ssa = True
            elif k == "ssa_drop":
                self.ssa = False
            self.max_rows = max(self.max_rows, self.m.rows)
            if self.g is not None:
                if k in ("delete", "load_ropes", "load_fmd", "save_then_load_self", "reset") and changed:
                    assert self.g.layout_stats()["sparse_now"] is False, "sparse behind %s" % k
                self.quiet_checks(i)
            if op.get("full"):
                self.full_checks(i)
        except StepFailed:
            raise
        except AssertionError as e:
            raise StepFailed("step %d, %.200s: %s\n%s" % (i, json.dumps(op), e, show(self.script, i))) from e

    def run(self):
        for op in self.script["ops"]:
            self.step(op)
        if not self.script["ops"] or not self.script["ops"][-1].get("full"):
            self.full_checks(self.steps)
        return self

    def patterns(self, rng, n=64):
        """text-order patterns: substrings of indexed strings, some to the end of the string and closed by `$`, random ones, the empty one"""
        w = self.m.walks()
        pats = [np.zeros(0, np.uint8), np.zeros(1, np.uint8)]
        while len(pats) < n:
            r = rng.rand()
            if len(w) and r < 0.75:
                s = w[rng.randint(len(w))][::-1]
                a = rng.randint(len(s) + 1)
                if r < 0.2:
                    pats.append(np.concatenate([s[a:], [0]]).astype(np.uint8))
                else:
                    p = s[a:a + rng.randint(1, 40)]
                    pats.append(np.concatenate([p, [0]]).astype(np.uint8) if r < 0.3 else p.copy())
            else:
                pats.append(rng.randint(1, 6, size=rng.randint(1, 12)).astype(np.uint8))
        return pats

    def quiet_checks(self, i):
        g, m = self.g, self.m
        rng = np.random.RandomState([self.script.get("seed", 0) & 0x7fffffff, i, 7])
        lay = g.layout_stats()
        assert np.array_equal(g.counts(), m.cnt), "count matrix"
        n = m.n
        assert g._n_strings() == n and len(self.plain) == n, "number of strings"
        fm = m.fm()
        pats = self.patterns(rng)
        want = np.array([fm.backward_search(p) for p in pats], np.int64)
        lo, hi, ml = g.backward_search(pats)
        bad = np.flatnonzero((lo != want[:, 0]) | (hi != want[:, 1]) | (ml != want[:, 2]))
        assert len(bad) == 0, "backward_search of %s: %s, the model has %s" % (pats[bad[0]].tolist(), (lo[bad[0]], hi[bad[0]], ml[bad[0]]), want[bad[0]].tolist())
        w = m.walks()
        if n:
            ids = rng.randint(0, n, size=min(n, 32))
            got = g.extract(ids, max(len(x) for x in w) + 1)
            for k, a in zip(ids.tolist(), got):
                assert a is not None and np.array_equal(a, w[k][::-1]), "extract(%d)" % k
                assert self.so != 0 or np.array_equal(a, self.plain[k]), "string %d is not the %d-th surviving string" % (k, k)
            ids = np.concatenate([rng.randint(0, n, size=min(n, 30)), [-1, n]])
            assert np.array_equal(g.contained_raw(ids), CR.contained(fm, ids)), "contained"
            first = int(rng.randint(0, n))
            cnt = int(rng.randint(0, min(n - first, 200) + 1))
            txt, off = g.unpack_raw(first, cnt)
            wt, wo = MR.pack([x[::-1] for x in w[first:first + cnt]])
            assert np.array_equal(off, wo) and np.array_equal(txt, wt), "unpack(%d, %d)" % (first, cnt)
        else:
            assert g.unpack_raw(0, 0)[1].tolist() == [0] and g.contained_raw([0]).tolist() == [[-1, 0, 0, 0, 0]]
        info = g.ssa_info()
        assert info["valid"] == self.ssa, "sampled suffix array: valid = %s, expected %s" % (info["valid"], self.ssa)
        if self.ssa:
            iv = [(int(a), int(b)) for a, b in want[:, :2] if a >= 0][:12] + [(0, m.rows), (m.rows, m.rows)]
            iv += [tuple(sorted(rng.randint(0, m.rows + 1, size=2).tolist())) for _ in range(2)]
            stored, hit, cnt = g.locate_raw(iv, 8)
            w_stored, w_hit, w_cnt = LR.locate_raw(fm, iv, 8)
            assert stored == w_stored and np.array_equal(cnt, w_cnt) and np.array_equal(hit, w_hit), "locate"
        assert g.ssa_info()["valid"] == self.ssa
        assert g.layout_stats() == lay, "a quiet check changed the layout: %s -> %s" % (lay, g.layout_stats())

    def full_checks(self, i):
        self.fulls.append(i)
        g, m = self.g, self.m
        if g is None:
            return
        try:
            got = g.bwt()
            assert len(got) == len(m.bwt) and np.array_equal(got, m.bwt), \
                "bwt(): %d rows, the model has %d; first differing row: %s" % (len(got), len(m.bwt), np.flatnonzero(got[:len(m.bwt)] != m.bwt[:len(got)])[:1])
            img = m.image()
            new = len(img)
            if self.old_size is not None:                           # the sizing protocol across a change of rows: fetch with the SIZE of before
                old = self.old_size
                buf = np.full(max(old, new) + 64, FILL, np.uint8)
                assert g.L.rb2_hip_save_fmd(g.h, buf.ctypes.data, old) == new, "save_fmd(dst, cap = the SIZE of before) does not return the new SIZE %d" % new
                if new <= old:
                    assert np.array_equal(buf[:new], img), "save_fmd(dst, cap = the SIZE of before): not the new image"
                    assert (buf[new:] == FILL).all(), "save_fmd wrote behind the image"
                else:
                    assert (buf == FILL).all(), "save_fmd wrote into a buffer that is too small"
            self.old_size = int(g.L.rb2_hip_save_fmd(g.h, None, 0))
            assert self.old_size == new, "SIZE %d, the host writer's image has %d bytes" % (self.old_size, new)
            assert np.array_equal(g.save_fmd(), img), "save_fmd() is not the host writer's image"
            assert g.ssa_info()["valid"] == self.ssa, "a full check changed the sampled suffix array"
            assert np.array_equal(g.counts(), m.cnt)
        except AssertionError as e:
            raise StepFailed("full check behind step %d: %s\n%s" % (i, e, show(self.script, i))) from e


def run(script, make=None):
    r = Runner(script, make)
    try:
        return r.run()
    finally:
        r.close()


# ---- the generator ---------------------------------------------------------------------------------------------------------------------

def script(seed, so, profile):
    """12 to 16 operations.  The model runs along, so that ids exist, a row change under a valid array really changes rows and the
    index stays below MAX_ROWS; what every script and the seeds of the GPU test together must contain is asserted in
    tests/test_op_sequences_ref.py."""
    pi = PROFILES.index(profile)
    rng = np.random.RandomState([seed & 0x7fffffff, so, pi, 20])
    sc = {"seed": int(seed), "so": int(so), "profile": profile, "sides": [batch_spec(rng, dup=False) for _ in range(2)], "ops": []}
    r = Runner(sc)
    idx = so * 6 + pi * 2 + seed
    plans = [PLANS[(2 * idx) % 10], PLANS[(2 * idx + 1) % 10]]

    def batch():
        return batch_spec(rng, small=r.m.rows > 110000)

    def ids(how=None):
        n = r.m.n
        how = how or str(rng.choice(["some", "none", "all"], p=[.8, .1, .1]))
        if how == "none" or n == 0:
            return []
        if how == "all":
            return list(range(n))
        x = rng.choice(n, size=max(1, int(n * rng.uniform(0.1, 0.5))), replace=False)
        return np.concatenate([x, x[:max(1, len(x) // 10)]]).tolist()          # (with duplicates)

    def insert(kind=None, plan=None):
        kind = kind or str(rng.choice(INSERTS, p=[.3, .3, .1, .3]))
        op = {"op": kind, "batch": batch()}
        if kind == "insert_host":
            op["lazy"] = int(rng.rand() < 0.6)
        elif kind == "insert_dev":
            op["misalign"] = int(rng.rand() < 0.5)
        elif kind == "insert_prefetched":
            op.update(plan=int(plan or rng.choice(PLANS)), lazy=int(rng.rand() < 0.6), reg=int(rng.rand() < 0.5))
            if op["plan"] in NEEDS_AUX:
                op["aux"] = batch()
                if op["plan"] == 6:
                    op["aux"]["n"] += 100                         # (the other buffer is the longer one, by its strings or not: it is only announced)
            if op["plan"] == 10:
                how = str(rng.choice(["reset", "delete", "load_fmd"]))
                op["mid"] = {"op": "reset"} if how == "reset" else {"op": "delete", "ids": ids("some")} if how == "delete" else {"op": "load_fmd", "k": int(rng.randint(2))}
        return op

    def load():
        how = str(rng.choice(["load_ropes", "load_fmd", "save_then_load_self"], p=[.4, .35, .25]))
        return {"op": how} if how == "save_then_load_self" else {"op": how, "k": int(rng.randint(2))}

    def merge():
        k = int(rng.randint(2))
        return {"op": "merge_from", "k": k, "batch_bytes": max(r.side(k).rows // int(rng.randint(4, 9)), 1)}

    def quiet():
        how = str(rng.choice(["reserve", "settle"], p=[.6, .4]))
        return {"op": "settle"} if how == "settle" else {"op": "reserve", "bytes": int(rng.randint(0, 1 << 20)), "strings": int(rng.randint(0, 5000)), "symbols": int(rng.randint(0, 1 << 21))}

    def ssa():
        return {"op": "ssa_build", "step": int(rng.choice([0, 2, 3, 5]))}

    def change():
        """an operation that changes rows whatever the index holds"""
        how = str(rng.choice(["insert", "delete", "merge", "load", "reset"], p=[.25, .2, .15, .35, .05]))
        if how == "delete" and r.m.n:
            return {"op": "delete", "ids": ids("some")}
        if how == "reset" and r.m.n:
            return {"op": "reset"}
        return merge() if how == "merge" else load() if how == "load" else insert()

    def filler():
        how = str(rng.choice(["insert", "delete", "merge", "load", "reset", "quiet", "ssa_build", "ssa_drop"], p=[.15, .15, .08, .22, .08, .22, .04, .06]))
        if how == "delete":
            return [{"op": "delete", "ids": ids()}] + ([insert] if rng.rand() < 0.5 else [])
        return [{"insert": insert, "merge": merge, "load": load, "reset": lambda: {"op": "reset"}, "quiet": quiet, "ssa_build": ssa, "ssa_drop": lambda: {"op": "ssa_drop"}}[how]()]

    special = (pi + seed) % 3
    segments = [
        lambda: [dict(ssa(), full=1), change],                                                  # a full check right behind ssa_build, then rows change under it
        lambda: [ssa()] + ([quiet()] if rng.rand() < 0.5 else []) + [{"op": "ssa_drop", "full": 1}],
        lambda: [[{"op": "reset"}], [{"op": "delete", "ids": ids("all")}], [load()]][special] + [insert],
        lambda: [insert("insert_prefetched", plans[0])],
        lambda: [insert("insert_prefetched", plans[1])],
        lambda: [{"op": "delete", "ids": ids("some")}, insert],
        lambda: [merge()],
    ]
    order = [segments[j] for j in rng.permutation(len(segments))]
    spare = [int(rng.randint(13, 17)) - 13]                       # operations beyond the segments and the first insert
    fill_at = sorted(rng.randint(0, len(order) + 1, size=3).tolist())

    def emit(ops):
        for op in ops:
            op = op() if callable(op) else op                       # (made when its turn comes: ids and copies are drawn from the index as it is then)
            sc["ops"].append(op)
            r.step(op)

    def fill():
        ops = filler()[:spare[0]]
        spare[0] -= len(ops)
        emit(ops)

    emit([insert()])
    for j, seg in enumerate(order + [None]):
        while fill_at and fill_at[0] == j:
            fill_at.pop(0)
            if spare[0] > 0:
                fill()
        if seg is not None:
            emit(seg())
    sc["ops"][-1]["full"] = 1
    return sc


def gpu_cases():
    """(so, profile, seed) of the random scripts of tests/test_op_sequences_gpu.py"""
    return [(so, profile, seed) for so in (0, 1, 2) for profile in PROFILES for seed in (1, 2)]
