"""child of tests/test_irreducible_gpu.py, with a fatal handler installed that prints the message and leaves with status 7; a stage that
must not be fatal ends with "STAGE OK" and status 0.
  chunk    RB2_QUERY_CHUNK=7 (the host variant stages seven queries at a time, the device variant launches seven at a time) and
           RB2_IRRED_SCRATCH of two rows' worth (two rows take all queries of a launch): the same answers as the model
Every other stage first asks a small index (which must work: "irreducible ok"), then calls both variants with n = 0 and the stage's bad
parameters (which must return: "empty ok"), then makes the one call that must be fatal; a call that returns prints "NOT FATAL".
  ovlp0 ext0 ext8193 steps0 recs0          a parameter of rb2_hip_irreducible outside its range
  dev-len0 dev-len8193 dev-ext0 dev-recs0  the same of rb2_hip_irreducible_dev
  shard                                    a rank of a sharded handle
usage: irreducible_child.py STAGE"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
import irreducible_ref as IR
import query_ref as Q
from ropebwt2_amd.hipbwt import HipBwt, MultiBwt, pack_patterns

#          max_len, min_ovlp, max_ext, max_steps, max_recs
STAGES = {"ovlp0": (40, 0, 4, 100, 4), "ext0": (40, 1, 0, 100, 4), "ext8193": (40, 1, 8193, 100, 4), "steps0": (40, 1, 4, 0, 4), "recs0": (40, 1, 4, 100, 0),
          "dev-len0": (0, 1, 4, 100, 4), "dev-len8193": (8193, 1, 4, 100, 4), "dev-ext0": (40, 1, 0, 100, 4), "dev-recs0": (40, 1, 4, 100, 0),
          "shard": (40, 1, 4, 100, 4)}


def row_bytes(lmax, min_ovlp, max_ext, max_steps):
    """csrc/rb2_query_plan.h: irred_row_bytes(irred_entry_cap(...), max_ext)"""
    cap = max(min(max(lmax - min_ovlp, 0) * (max_ext + 1), max_steps), 1)
    nf = min(cap, max_ext)
    pad = lambda b: (b + 7) // 8 * 8
    return 64 * cap + pad(4 * nf) + pad(2 * cap) + pad(nf)


def chunk(g, reads):
    from test_irreducible_gpu import FILL, _sets, irreducible_dev
    from test_query_gpu import _Env
    fm = Q.FM(g.bwt())
    qs = [np.asarray(r, np.uint8) for r in reads[:50]] + [np.array([1, 0, 2], np.uint8), np.zeros(0, np.uint8), np.array([5], np.uint8)]
    lmax = max(len(q) for q in qs)
    for (min_ovlp, max_ext, max_steps), max_recs in (((1, 4, 1 << 16), 16), ((3, 1000, 1 << 16), 16), ((2, 6, 40), 2)):
        res = [IR.irreducible(fm, q, min_ovlp, max_ext, max_steps) for q in qs]
        want = [None if c == -1 else sorted(r) for r, c, _ in res]
        wcnt = np.array([c for _, c, _ in res], np.int64)
        assert sum(len(w) for w in want if w) > 30 and (wcnt <= -2).any() == (max_steps == 40)
        plain = g.irreducible_raw(qs, min_ovlp, max_ext, max_steps, max_recs)
        with _Env(RB2_QUERY_CHUNK=7, RB2_IRRED_SCRATCH=2 * row_bytes(lmax, min_ovlp, max_ext, max_steps)):
            chunked = g.irreducible_raw(qs, min_ovlp, max_ext, max_steps, max_recs)
            d_rec, d_cnt = irreducible_dev(g, qs, lmax, min_ovlp, max_ext, max_steps, max_recs)
        with _Env(RB2_IRRED_SCRATCH=1):                              # less than one row: one row all the same
            one = g.irreducible_raw(qs, min_ovlp, max_ext, max_steps, max_recs)
        for stored, rec, cnt in (plain, chunked, one, (None, d_rec, d_cnt)):
            assert np.array_equal(cnt, wcnt), (cnt.tolist(), wcnt.tolist())
            have = _sets(rec, cnt, max_recs)
            if max_recs == 16:
                assert have == want
            else:                                                   # cut: distinct true records, as many as there is room for
                assert all(h is None or (len(set(h)) == len(h) == min(len(w), max_recs) and set(h) <= set(w)) for h, w in zip(have, want))
            assert stored is None or stored == sum(len(h) for h in have if h)
        live = np.arange(max_recs)[None, :] < np.array([len(h) if h else 0 for h in _sets(d_rec, d_cnt, max_recs)])[:, None]
        assert (d_rec[~live] == FILL).all() and (plain[1][~live] == 0).all()
    g.close()
    print("STAGE OK")


def main():
    stage = sys.argv[1]
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    g = HipBwt(0)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    reads = H.repetitive_reads(60, seed=9, max_len=30)
    g.insert_multi(H.encode_batch(reads, True, True))
    if stage == "chunk":
        return chunk(g, reads)
    max_len, min_ovlp, max_ext, max_steps, max_recs = STAGES[stage]
    q = max(reads, key=len)
    stored, rec, cnt = g.irreducible_raw([q], 1, 4)
    assert cnt[0] >= 0 and stored == min(cnt[0], 16)
    print("irreducible ok", flush=True)
    qry, off = pack_patterns([q])
    rec, cnt = np.zeros((1, 8, 4), np.int64), np.zeros(1, np.int64)
    args = (min_ovlp, max_ext, max_steps, max_recs, rec.ctypes.data, cnt.ctypes.data)
    h = g.h
    if stage == "shard":
        m = MultiBwt(0, [0, 0])
        h = m.engine(0).h
    else:
        assert g.L.rb2_hip_irreducible(h, 0, qry.ctypes.data, off.ctypes.data, *args) == 0          # n <= 0 returns before the parameters are looked at
        g.L.rb2_hip_irreducible_dev(h, 0, qry.ctypes.data, off.ctypes.data, max_len, *args)
    print("empty ok", flush=True)
    if stage.startswith("dev-"):
        d = g.dev_alloc(4096)                                        # (the check comes before any pointer is used)
        g.L.rb2_hip_irreducible_dev(h, 1, d, d, max_len, min_ovlp, max_ext, max_steps, max_recs, d, d)
    else:
        g.L.rb2_hip_irreducible(h, 1, qry.ctypes.data, off.ctypes.data, *args)
    print("NOT FATAL")


if __name__ == "__main__":
    main()
