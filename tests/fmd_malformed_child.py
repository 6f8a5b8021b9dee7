"""child of tests/test_fmd_load_gpu.py: load one malformed .fmd image with a fatal handler installed.  The handler prints the message
and leaves with status 7; any other end (a fault, a normal return) is the failure the parent looks for.
usage: fmd_malformed_child.py CASE FIXTURE"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import fmd_ref
from ropebwt2_amd.hipbwt import HipBwt


def malformed(case, img):
    img = bytearray(img)
    n_bytes = fmd_ref.parse(bytes(img))["n_bytes"]
    if case == "magic":
        img[0:4] = b"RLE\3"
    elif case == "sbits":
        img[4] = 4
    elif case == "truncated":                                   # by one block: the image ends 64 bytes before its stream does
        del img[80 + n_bytes - 64:]
    elif case == "bitflip":                                     # the low bit of the first run's symbol: $ <-> A, C <-> G, T <-> N
        c, l = fmd_ref.block_runs(fmd_ref.parse(bytes(img))["words"], 0)[0]
        y = l.bit_length() - 1
        z = (y + 1).bit_length() - 1
        p = 128 + 2 * z + 1 + y + 2                             # bit of the stream, most significant first; the payload starts at word 2
        img[80 + 8 * (p // 64) + (63 - p % 64) // 8] ^= 1 << ((63 - p % 64) % 8)
    else:
        raise SystemExit("unknown case " + case)
    return bytes(img)


def main():
    case, name = sys.argv[1], sys.argv[2]
    img = malformed(case, fmd_ref.fixture(name)[0])
    g = HipBwt(0)
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    n = g.load_fmd(np.frombuffer(img, np.uint8))
    print("loaded %d symbols" % n)


if __name__ == "__main__":
    main()
