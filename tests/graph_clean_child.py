"""child of tests/test_graph_clean_gpu.py: one call of rb2_hip_graph_clean[_dev] that must fail its validation, with a fatal handler
installed.  The handler prints the message, checks that the caller's buffers are what they were and leaves with status 7; any other end
(a fault, a normal return, a failed check) is the failure the parent looks for.  The validations under test are argument checks that
fire at the top of the call, before any kernel runs, which is why the handler may go on using the handle -- and why the _dev cases may
pass host pointers: nothing reads them.
usage: graph_clean_child.py CASE"""
import ctypes as C
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

from ropebwt2_amd.hipbwt import HipBwt

GOOD = dict(n_str=6, m=5, max_tip_reads=2, max_bubble_reads=3, pairs=1, max_rounds=8, cap=5)


def main():
    case = sys.argv[1]
    g = HipBwt(0)
    edges = np.array([(k, k + 1, 30, 5) for k in range(5)], np.int64)
    before = edges.copy()
    out = np.full((8, 4), -7, np.int64)
    info = np.full(8, -7, np.int64)
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        try:
            sys.stdout.write("handler: " + msg.decode())
            assert np.array_equal(edges, before) and (out == -7).all() and (info == -7).all()
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

    def call(dev=False, e=edges.ctypes.data, o=out.ctypes.data, **kw):
        a = dict(GOOD, **kw)
        fn = g.L.rb2_hip_graph_clean_dev if dev else g.L.rb2_hip_graph_clean
        fn(g.h, a["n_str"], a["m"], e, a["max_tip_reads"], a["max_bubble_reads"], a["pairs"], a["max_rounds"], a["cap"], o, info.ctypes.data)

    if case == "negative_n":
        call(n_str=-1)
    elif case == "negative_m":
        call(m=-1)
    elif case == "negative_cap":
        call(cap=-1)
    elif case == "negative_tip":
        call(max_tip_reads=-1)
    elif case == "negative_bubble":
        call(max_bubble_reads=-1)
    elif case == "max_rounds":
        call(max_rounds=0)
    elif case == "pairs":
        call(pairs=2)
    elif case == "null_edges":
        call(e=None)
    elif case == "null_out":
        call(o=None)
    elif case == "overlap":                                         # out starts inside the last row of edges
        call(o=edges.ctypes.data + 4 * 32 + 8, cap=1)
    elif case == "overlap_front":                                   # edges starts inside out
        call(e=out.ctypes.data + 32, m=2, cap=5)
    elif case == "dev_max_rounds":
        call(dev=True, max_rounds=-3)
    elif case == "dev_overlap":
        call(dev=True, o=edges.ctypes.data, cap=1)
    elif case == "dev_null_out":
        call(dev=True, o=None)
    else:
        raise SystemExit("unknown case " + case)
    print("the call returned")


if __name__ == "__main__":
    main()
