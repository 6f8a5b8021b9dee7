"""child of tests/test_overlap_gpu.py, with a fatal handler installed that prints the message and leaves with status 7; a stage that must
not be fatal ends with "STAGE OK" and status 0.
  chunk  the host variants stage three queries / ranges at a time (RB2_QUERY_CHUNK=3) and the device variants launch three at a time: the
         same answers as the model
  nossa  rb2_hip_overlap needs no suffix array; rb2_hip_string_ids without one is fatal
usage: overlap_child.py chunk | nossa"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
import overlap_ref as OR
import query_ref as Q
from ropebwt2_amd.hipbwt import HipBwt
from test_overlap_gpu import FILL, overlap_dev, string_ids_dev
from test_query_gpu import _Env


def main():
    stage = sys.argv[1]
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    reads = H.repetitive_reads(120, seed=51, max_len=30)
    g = HipBwt(0)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    g.insert_multi(H.encode_batch(reads, True, True))
    fm = Q.FM(g.bwt())
    qs = [np.asarray(r, np.uint8) for r in reads[:40]] + [np.array([1, 0, 2], np.uint8), np.zeros(0, np.uint8)]
    if stage == "chunk":
        n = int(fm.C[1])
        g.build_ssa(2)
        rng = np.random.RandomState(6)
        zlo = rng.randint(0, n, size=41)
        zv = np.stack([zlo, np.minimum(zlo + rng.randint(0, 9, size=41), n)], 1)
        zv[17] = (5, 4)
        for max_recs, max_hits in ((30, 8), (2, 3)):
            want = OR.overlap_raw(fm, qs, 1, max_recs)
            w_ids = OR.string_ids_raw(fm, zv, max_hits)
            assert want[0] > 40 and (want[2] > max_recs).any() == (max_recs == 2) and (w_ids[2] > max_hits).any() == (max_hits == 3)
            plain, p_ids = g.overlap_raw(qs, 1, max_recs), g.string_ids_raw(zv, max_hits)
            with _Env(RB2_QUERY_CHUNK=3):
                chunked, c_ids = g.overlap_raw(qs, 1, max_recs), g.string_ids_raw(zv, max_hits)
                d_rec, d_cnt = overlap_dev(g, qs, 1, max_recs)
                d_ids, d_n = string_ids_dev(g, zv, max_hits)
            for got, w in ((plain, want), (chunked, want), (p_ids, w_ids), (c_ids, w_ids)):
                assert got[0] == w[0] and np.array_equal(got[1], w[1]) and np.array_equal(got[2], w[2])
            live = np.arange(max_recs)[None, :] < want[2][:, None]
            assert np.array_equal(d_cnt, want[2]) and np.array_equal(d_rec[live], want[1][live]) and (d_rec[~live] == FILL).all()
            live = np.arange(max_hits)[None, :] < w_ids[2][:, None]
            assert np.array_equal(d_n, w_ids[2]) and np.array_equal(d_ids[live], w_ids[1][live]) and (d_ids[~live] == FILL).all()
        g.close()
        print("STAGE OK")
    elif stage == "nossa":
        print("info", g.ssa_info(), flush=True)
        got, want = g.overlap_raw(qs, 1, 30), OR.overlap_raw(fm, qs, 1, 30)
        assert got[0] == want[0] > 40 and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        print("overlap ok", flush=True)
        g.string_ids_raw([(0, 1)], 1)
        print("NOT FATAL")
    else:
        raise SystemExit("unknown stage " + stage)


if __name__ == "__main__":
    main()
