"""child of tests/test_contain_gpu.py, with a fatal handler installed that prints the message and leaves with status 7; a stage that must
not be fatal ends with "STAGE OK" and status 0.
  chunk  the host variant stages seven ids at a time (RB2_QUERY_CHUNK=7) and the device variant launches seven at a time, with ids and
         without, early exit on and off: the same records as the model
  shard  rb2_hip_contained on a rank of a sharded handle is fatal
usage: contain_child.py chunk | shard"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import contain_ref as CR
import query_ref as Q
from ropebwt2_amd.hipbwt import HipBwt, MultiBwt
from test_contain_gpu import dev_records
from test_query_gpu import _Env


def main():
    stage = sys.argv[1]
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    bufs, bwt = CR.mixed(1, True)
    g = HipBwt(1)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    for b in bufs:
        g.insert_multi(b)
    fm = Q.FM(bwt)
    n = int(fm.C[1])
    assert np.array_equal(g.bwt(), bwt)
    if stage == "chunk":
        ids = np.concatenate([np.random.RandomState(3).randint(0, n, size=60), [-1, n, 0, n - 1]])
        for early in (True, False):
            want, w_ids = CR.contained(fm, early=early), CR.contained(fm, ids, early=early)
            with _Env(RB2_CONTAIN_EARLY=int(early)):
                plain, p_ids = g.contained_raw(), g.contained_raw(ids)
                with _Env(RB2_QUERY_CHUNK=7):
                    chunked, c_ids = g.contained_raw(), g.contained_raw(ids)
                    d_all, d_ids = dev_records(g, n + 3, None), dev_records(g, len(ids), ids)
            for got, w in ((plain, want), (chunked, want), (p_ids, w_ids), (c_ids, w_ids), (d_all[:n], want), (d_ids, w_ids)):
                assert np.array_equal(got, w), early
            assert (d_all[n:] == [-1, 0, 0, 0, 0]).all()
        g.close()
        print("STAGE OK")
    elif stage == "shard":
        assert np.array_equal(g.contained_raw(), CR.contained(fm))
        print("contained ok", flush=True)
        m = MultiBwt(0, [0, 0])
        rec = np.zeros((4, 5), np.int64)
        g.L.rb2_hip_contained(m.engine(0).h, 4, None, rec.ctypes.data)
        print("NOT FATAL")
    else:
        raise SystemExit("unknown stage " + stage)


if __name__ == "__main__":
    main()
