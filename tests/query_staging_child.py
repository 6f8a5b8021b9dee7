"""child of tests/test_query_staging_gpu.py, with a fatal handler installed that prints the message and leaves with status 7: what the
query families do with no items and a bad parameter.  rb2_hip_smem returns before it looks at min_occ;
rb2_hip_locate checks max_hits first, so the second call must not come back."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import helpers as H
from ropebwt2_amd.hipbwt import HipBwt
from test_query_staging_gpu import reads


def main():
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    g = HipBwt(0)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    g.insert_multi(H.encode_batch(reads(), True, True))
    g.build_ssa(2)
    print("smem returned", g.L.rb2_hip_smem(g.h, 0, None, None, 1, 0, 4, None, None), flush=True)   # (HipBwt.smem_raw makes no call without queries)
    g.locate_raw([], 0)
    print("NOT FATAL")


if __name__ == "__main__":
    main()
