"""child of tests/test_graph_gpu.py: one call of rb2_hip_string_graph[_dev] that must fail its validation, with a fatal handler
installed.  The handler prints the message, checks that the index and the caller's buffers are what they were and leaves with status 7;
any other end (a fault, a normal return, a failed check) is the failure the parent looks for.  The validations under test are argument
checks that fire at the top of the call, before any kernel runs, which is why the handler may go on using the handle.
usage: graph_fatal_child.py CASE"""
import ctypes as C
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
from ropebwt2_amd.hipbwt import HipBwt, MultiBwt

GOOD = dict(first=0, n=40, min_ovlp=5, max_ext=40, max_steps=1 << 16, max_recs=16, max_hits=8, pairs=0, cap=64)


def main():
    case = sys.argv[1]
    g = HipBwt(0)
    g.insert_multi(H.encode_batch(H.repetitive_reads(20, seed=21), True, True))      # 40 strings
    if case != "no_ssa":
        g.build_ssa(2)
    if case == "no_ssa_dev":                                        # (built and dropped again)
        g.drop_ssa()
    if case == "odd_pairs":
        g.delete(np.array([39], np.int64))
        g.build_ssa(2)
    hashes, ssa = g.rope_hashes(), g.ssa_info()
    edges = np.full((66, 4), -7, np.int64)
    info = np.full(8, -7, np.int64)
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        try:
            sys.stdout.write("handler: " + msg.decode())
            assert g.rope_hashes() == hashes and g.ssa_info() == ssa
            assert (edges == -7).all() and (info == -7).all()
            print("unchanged ok")
            sys.stdout.flush()
            os._exit(7)
        except BaseException:
            traceback.print_exc()
            sys.stderr.flush()
            sys.stdout.flush()
            os._exit(3)

    cb = CB(handler)
    g.L.rb2_hip_set_fatal_handler(cb, None)

    def call(h=None, dev=False, null=False, **kw):
        a = dict(GOOD, **kw)
        fn = g.L.rb2_hip_string_graph_dev if dev else g.L.rb2_hip_string_graph
        fn(h or g.h, a["first"], a["n"], a["min_ovlp"], a["max_ext"], a["max_steps"], a["max_recs"], a["max_hits"], a["pairs"], a["cap"], None if null else edges.ctypes.data,
           info.ctypes.data)

    if case == "no_ssa":
        call()
    elif case == "no_ssa_dev":                                      # (the device variant checks before it touches edges: a host pointer does no harm)
        call(dev=True)
    elif case == "rank":
        m = MultiBwt(0, [0, 0])
        call(h=m.engine(0).h, n=0)
    elif case == "negative_first":
        call(first=-1, n=3)
    elif case == "negative_n":
        call(n=-1)
    elif case == "range_past_end":
        call(first=30, n=11)
    elif case == "negative_cap":
        call(cap=-1)
    elif case == "null_edges":
        call(null=True)
    elif case == "min_ovlp":
        call(min_ovlp=0)
    elif case == "max_ext_low":
        call(max_ext=0)
    elif case == "max_ext_high":
        call(max_ext=8193)
    elif case == "max_steps":
        call(max_steps=0)
    elif case == "max_recs":
        call(max_recs=0)
    elif case == "max_hits":
        call(max_hits=0)
    elif case == "odd_pairs":
        call(n=39, pairs=1)
    elif case == "dev_max_hits":
        call(dev=True, max_hits=0)
    else:
        raise SystemExit("unknown case " + case)
    print("the call returned")


if __name__ == "__main__":
    main()
