"""child of tests/test_delete_gpu.py: one call of rb2_hip_delete_strings that must fail its validation, with a fatal handler installed.
The handler prints the message, checks that the index is what it was, makes an in-range call on it and checks the result against the
oracle, and leaves with status 7; any other end (a fault, a normal return, a failed check) is the failure the parent looks for.
The validations under test fire at the top of the call, before it holds or changes anything, which is why the handler may go on using
the handle: that nothing was changed is the property it checks.
usage: delete_fatal_child.py CASE"""
import ctypes as C
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import delete_ref as D
import helpers as H
from ropebwt2_amd.hipbwt import HipBwt, encode_runs


def main():
    case = sys.argv[1]
    so = 1
    buf = H.encode_batch(H.repetitive_reads(20, seed=21), True, True)      # 40 strings
    o = H.Oracle(so)
    o.insert_multi(buf)
    bwt = o.bwt()
    o.close()
    assert D.n_strings(bwt) == 40
    g = HipBwt(so)
    g.insert_multi(buf)
    hashes = g.rope_hashes()
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        try:
            sys.stdout.write("handler: " + msg.decode())
            assert g.rope_hashes() == hashes and np.array_equal(g.bwt(), bwt)
            print("unchanged ok")
            ids = [3, 17, 3, 39]                                            # an in-range call: the hashes are those of the oracle's survivors
            o2 = H.Oracle(so)
            o2.insert_multi(D.buffer_of(D.survivors(bwt, ids)))
            assert g.delete(ids) == D.delete(bwt, ids)[1]
            assert np.array_equal(g.bwt(), o2.bwt())
            g2 = HipBwt(so)
            g2.load_ropes([encode_runs(r) for r in o2.ropes()])
            assert g.rope_hashes() == g2.rope_hashes()
            print("in-range ok")
            sys.stdout.flush()
            os._exit(7)
        except BaseException:
            traceback.print_exc()
            sys.stderr.flush()
            sys.stdout.flush()
            os._exit(3)

    cb = CB(handler)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    if case == "negative_id":
        g.delete([5, -1])
    elif case == "id_is_count":
        g.delete([40])
    elif case == "negative_n":
        ids = np.array([1, 2], np.int64)
        g.L.rb2_hip_delete_strings(g.h, -1, ids.ctypes.data)
    else:
        raise SystemExit("unknown case " + case)
    print("the call returned")


if __name__ == "__main__":
    main()
