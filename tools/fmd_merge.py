"""Merge .fmd files on the device: the strings of every further file are inserted into the index of the first (rb2_hip_merge).

    python tools/fmd_merge.py OUT.fmd IN1.fmd IN2.fmd [...] [--so N]

IN1 is loaded into one handle, every further file into a second one and merged into the first; the result is written to OUT.fmd
(rb2_hip_save_fmd_file).  --so is the sorting order the strings of IN2 ... are inserted in (0 input order, 1 RLO, 2 RCLO): it must be
the order IN1 was built in, or the result is the BWT of no single order.  One line per input: the `info` of its merge."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ropebwt2_amd import HipBwt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("inputs", nargs="+")
    ap.add_argument("--so", type=int, default=0, choices=(0, 1, 2))
    a = ap.parse_args(argv)
    if len(a.inputs) < 2:
        ap.error("at least two input files")
    dst, src = HipBwt(a.so), HipBwt(a.so)
    print("%s: %d symbols loaded" % (a.inputs[0], dst.load_fmd(a.inputs[0])))
    for path in a.inputs[1:]:
        src.load_fmd(path)
        n, syms, batches, largest = dst.merge(src)
        print("%s: %d strings, %d symbols, %d batches, largest batch %d bytes" % (path, n, syms, batches, largest))
    print("%s: %d bytes" % (a.out, dst.save_fmd(a.out)))
    src.close()
    dst.close()


if __name__ == "__main__":
    main()
