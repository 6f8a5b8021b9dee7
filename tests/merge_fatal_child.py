"""child of tests/test_merge_gpu.py: one call of rb2_hip_unpack or rb2_hip_merge that must fail its validation, with a fatal handler
installed.  The handler prints the message, checks that the indexes are what they were and leaves with status 7; any other end (a fault,
a normal return, a failed check) is the failure the parent looks for.  The validations under test fire at the top of the call, before it
holds or changes anything, which is why the handler may go on using the handles.
usage: merge_fatal_child.py CASE"""
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


def main():
    case = sys.argv[1]
    g, s = HipBwt(1), HipBwt(1)
    g.insert_multi(H.encode_batch(H.repetitive_reads(20, seed=21), True, True))      # 40 strings
    s.insert_multi(H.encode_batch(H.repetitive_reads(10, seed=22), True, True))
    hashes = g.rope_hashes(), s.rope_hashes()
    canary = np.full(4096, 0xAB, np.uint8)
    off = np.full(64, -7, np.int64)
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        try:
            sys.stdout.write("handler: " + msg.decode())
            assert (g.rope_hashes(), s.rope_hashes()) == hashes
            assert (canary == 0xAB).all() and (off == -7).all()
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
    unpack = lambda first, n, cap: g.L.rb2_hip_unpack(g.h, first, n, 0, cap, canary.ctypes.data, off.ctypes.data)
    if case == "range_past_end":
        unpack(30, 11, len(canary))
    elif case == "negative_first":
        unpack(-1, 3, len(canary))
    elif case == "negative_n":
        unpack(0, -1, len(canary))
    elif case == "negative_cap":
        unpack(0, 40, -1)
    elif case == "dst_is_src":
        g.merge(g)
    elif case == "negative_batch":
        g.merge(s, -1)
    elif case in ("rank_dst", "rank_src", "rank_unpack"):
        m = MultiBwt(1, [0, 0])
        if case == "rank_dst":
            g.L.rb2_hip_merge(m.engine(0).h, s.h, 0, None)
        elif case == "rank_src":
            g.L.rb2_hip_merge(g.h, m.engine(0).h, 0, None)
        else:
            g.L.rb2_hip_unpack(m.engine(0).h, 0, 0, 0, 0, None, None)
    else:
        raise SystemExit("unknown case " + case)
    print("the call returned")


if __name__ == "__main__":
    main()
