"""child of tests/test_kmer_gpu.py, with a fatal handler installed that prints the message and leaves with status 7.  Every stage first
enumerates the k-mers of a small index (which must work: "kmers ok"), then makes the one call that must be fatal; a call that returns
prints "NOT FATAL".
  k0 k33 minocc0 negrecs neghist nullrec nullhist   a parameter outside its range
  shard                                              a rank of a sharded handle
usage: kmer_child.py STAGE"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
from ropebwt2_amd.hipbwt import HipBwt, MultiBwt

#          k, min_occ, max_recs, rec, hist_len, hist  (rec / hist: True = a buffer, False = NULL)
STAGES = {"k0": (0, 1, 4, True, 4, True), "k33": (33, 1, 4, True, 4, True), "minocc0": (3, 0, 4, True, 4, True), "negrecs": (3, 1, -1, True, 4, True),
          "neghist": (3, 1, 4, True, -2, True), "nullrec": (3, 1, 4, False, 4, True), "nullhist": (3, 1, 4, True, 4, False), "shard": (3, 1, 4, True, 4, True)}


def main():
    stage = sys.argv[1]
    k, min_occ, max_recs, with_rec, hist_len, with_hist = STAGES[stage]
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    g = HipBwt(0)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    g.insert_multi(H.encode_batch(H.repetitive_reads(60, seed=9, max_len=30), True, True))
    found, rec, hist, info = g.kmers_raw(3, 1, False, 64, 8)
    assert 0 < found <= 64 and hist.sum() == found and info[3] == found
    print("kmers ok", flush=True)
    h = g.h
    if stage == "shard":
        m = MultiBwt(0, [0, 0])
        h = m.engine(0).h
    rec, hist, info = np.zeros((8, 3), np.int64), np.zeros(8, np.int64), np.zeros(4, np.int64)
    g.L.rb2_hip_kmers(h, k, min_occ, 0, max_recs, rec.ctypes.data if with_rec else None, hist_len, hist.ctypes.data if with_hist else None, info.ctypes.data)
    print("NOT FATAL")


if __name__ == "__main__":
    main()
