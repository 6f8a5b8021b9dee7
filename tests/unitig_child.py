"""child of tests/test_unitig_gpu.py, with a fatal handler installed that prints the message and leaves with status 7; a stage that must
not be fatal ends with "STAGE OK" and status 0.
  chunk    RB2_QUERY_CHUNK=7: the host variant of the chains stages seven edges at a time, the device variant launches seven at a time;
           the same vtx and info as the model, and the same texts behind them
Every other stage first runs both calls on a small index (which must work: "unitig ok"), then makes the one call that must be fatal; a
call that returns prints "NOT FATAL".
  reads0 nstr nstr-dev capu capt      a parameter of rb2_hip_unitig_text[_dev] outside its range, n_str unequal to the strings of the index
  chains-n chains-m chains-dev-n      the same of rb2_hip_unitig_chains[_dev]
  shard                               rb2_hip_unitig_text on a rank of a sharded handle
usage: unitig_child.py STAGE"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
import unitig_ref as U
from ropebwt2_amd.hipbwt import HipBwt, MultiBwt
from test_query_gpu import _Env


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
    _, reads = U.tile_reads(seed=3, glen=150, lo=20, hi=30, smax=4)
    strings = U.both_strands(U.drop_contained(reads))
    g.insert_multi(H.encode_batch(strings, True, False))
    n = len(strings)
    edges = np.array(U.brute_edges(strings, 10), np.int64).reshape(-1, 4)
    want, winfo = U.chains(n, edges)
    assert len(edges) > 20 and winfo[0] < n
    vtx, info = g.unitig_chains(edges)
    assert np.array_equal(vtx, want) and np.array_equal(info, winfo)
    urec, txt = g.unitig_text(vtx)
    w_urec, w_txt, _ = U.texts(strings, want)
    assert np.array_equal(urec, w_urec) and np.array_equal(txt, w_txt)
    if stage == "chunk":
        from test_unitig_gpu import chains_dev
        with _Env(RB2_QUERY_CHUNK=7):
            vtx, info = g.unitig_chains(edges)
            d_vtx, d_info = chains_dev(g, n, edges)
            urec, txt = g.unitig_text(vtx)
        assert np.array_equal(vtx, want) and np.array_equal(info, winfo) and np.array_equal(d_vtx, want) and np.array_equal(d_info, winfo)
        assert np.array_equal(urec, w_urec) and np.array_equal(txt, w_txt)
        g.close()
        print("STAGE OK")
        return
    print("unitig ok", flush=True)
    inf = np.zeros(4, np.int64)
    urec, txt = np.zeros((n, 5), np.int64), np.zeros(4096, np.uint8)
    text = lambda h, fn, nn, reads, cu, ct: fn(h, nn, vtx.ctypes.data, 0, reads, cu, ct, urec.ctypes.data, txt.ctypes.data, inf.ctypes.data)
    L = g.L
    if stage == "reads0":
        text(g.h, L.rb2_hip_unitig_text, n, 0, n, 4096)
    elif stage == "nstr":
        text(g.h, L.rb2_hip_unitig_text, n - 1, 1, n, 4096)
    elif stage == "nstr-dev":
        d = g.dev_alloc(4096)                                        # (the check comes before any pointer is used)
        L.rb2_hip_unitig_text_dev(g.h, n + 1, d, 0, 1, 0, 0, d, d, inf.ctypes.data)
    elif stage == "capu":
        text(g.h, L.rb2_hip_unitig_text, n, 1, -1, 4096)
    elif stage == "capt":
        text(g.h, L.rb2_hip_unitig_text, n, 1, n, -1)
    elif stage == "chains-n":
        L.rb2_hip_unitig_chains(g.h, -1, len(edges), edges.ctypes.data, vtx.ctypes.data, inf.ctypes.data)
    elif stage == "chains-m":
        L.rb2_hip_unitig_chains(g.h, n, -1, edges.ctypes.data, vtx.ctypes.data, inf.ctypes.data)
    elif stage == "chains-dev-n":
        d = g.dev_alloc(4096)
        L.rb2_hip_unitig_chains_dev(g.h, -1, 0, d, d, d)
    elif stage == "shard":
        m = MultiBwt(0, [0, 0])
        text(m.engine(0).h, L.rb2_hip_unitig_text, 0, 1, 0, 0)
    else:
        raise SystemExit("unknown stage " + stage)
    print("NOT FATAL")


if __name__ == "__main__":
    main()
