"""child of tests/test_correct_gpu.py: one call of rb2_hip_correct[_dev] or rb2_hip_correct_into that must fail its validation, with a
fatal handler installed.  The handler prints the message, checks that the indexes and the output buffers are what they were and leaves
with status 7; any other end (a fault, a normal return, a failed check) is the failure the parent looks for.  The validations under test
fire at the top of the call, before it holds or changes anything, which is why the handler may go on using the handles.
usage: correct_fatal_child.py CASE"""
import ctypes as C
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
from ropebwt2_amd.hipbwt import HipBwt, MultiBwt, pack_patterns


def main():
    case = sys.argv[1]
    g, s = HipBwt(0), HipBwt(0)
    g.insert_multi(H.encode_batch(H.repetitive_reads(20, seed=21), True, True))      # 40 strings
    s.insert_multi(H.encode_batch(H.repetitive_reads(10, seed=22), True, True))
    odd = HipBwt(0)
    odd.insert_multi(H.encode_batch(H.repetitive_reads(3, seed=23)))                  # 3 strings
    hashes = g.rope_hashes(), s.rope_hashes(), odd.rope_hashes()
    qry, off = pack_patterns([[1, 2, 3, 4, 1, 2], [2, 2, 1]])
    out = np.full(len(qry), 0xAB, np.uint8)
    cnt, weak = np.full(2, -7, np.int64), np.full(2, -7, np.int64)
    # n = 0 returns before the parameters are looked at
    assert g.L.rb2_hip_correct(g.h, 0, None, None, 0, 0, 0, 0, None, None, None) == 0
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        try:
            sys.stdout.write("handler: " + msg.decode())
            assert (g.rope_hashes(), s.rope_hashes(), odd.rope_hashes()) == hashes
            assert (out == 0xAB).all() and (cnt == -7).all() and (weak == -7).all()
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
    host = lambda h, k, mo, mf, mp: g.L.rb2_hip_correct(h, 2, qry.ctypes.data, off.ctypes.data, k, mo, mf, mp, out.ctypes.data, cnt.ctypes.data, weak.ctypes.data)
    if case == "k0":
        host(g.h, 0, 1, 1, 1)
    elif case == "minocc0":
        host(g.h, 1, 0, 1, 1)
    elif case == "maxfix0":
        host(g.h, 1, 1, 0, 1)
    elif case == "maxprobes0":
        host(g.h, 1, 1, 1, 0)
    elif case in ("dev_k0", "dev_total"):                              # (the pointers are never used: the checks come first)
        d = g.dev_alloc(64)
        g.L.rb2_hip_correct_dev(g.h, 2, d, d, -1 if case == "dev_total" else 9, 0 if case == "dev_k0" else 3, 1, 1, 1, d, d, d)
    elif case == "into_k0":
        s.correct_into(g, 0)
    elif case == "into_maxprobes0":
        s.correct_into(g, 3, max_probes=0)
    elif case == "dst_is_src":
        g.correct_into(g, 3)
    elif case == "negative_batch":
        s.correct_into(g, 3, batch_bytes=-1)
    elif case == "odd_pairs":
        odd.correct_into(g, 3, pairs=True)
    elif case in ("rank", "rank_dst", "rank_src"):
        m = MultiBwt(0, [0, 0])
        if case == "rank":
            host(m.engine(0).h, 3, 1, 1, 1)
        elif case == "rank_dst":
            g.L.rb2_hip_correct_into(m.engine(0).h, s.h, 3, 1, 1, 1, 0, 0, None)
        else:
            g.L.rb2_hip_correct_into(g.h, m.engine(0).h, 3, 1, 1, 1, 0, 0, None)
    else:
        raise SystemExit("unknown case " + case)
    print("the call returned")


if __name__ == "__main__":
    main()
