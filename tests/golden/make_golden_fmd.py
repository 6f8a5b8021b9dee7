#!/usr/bin/env python3
"""Generate tests/golden/fmd/*.fmd and *.bwt.gz with the REAL reference (oracle/_ref/ropebwt2, built by oracle/Makefile): for every
input the file `-d` writes and the plain BWT text of the same run (gzip, it is repetitive).  Only data the reference writes is
stored -- never reference source.  Run in the build container:  python tests/golden/make_golden_fmd.py"""
import gzip, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from helpers import GOLDEN_DIR, SYMS, run_ref, lines_from_codes  # noqa

OUT = os.path.join(GOLDEN_DIR, "fmd")


def inputs():
    yield "kat6", "-LR", b"ACGT\nACGA\nTTGA\nNACG\nGATTACA\nCCC\n"
    rng = np.random.RandomState(11)
    yield "rand300", "-LR", lines_from_codes([rng.randint(1, 5, size=rng.randint(1, 41)) for _ in range(300)])
    rng = np.random.RandomState(12)
    genome = rng.randint(1, 5, size=2000).astype(np.uint8)
    yield "cov3000", "-LRs", lines_from_codes([genome[s:s + 60] for s in rng.randint(0, 2000 - 60 + 1, size=3000)])
    yield "longA", "-LR", b"ACGTN\n" + (b"A" * 30000 + b"\n") * 3      # a type-1 header; one run of 90 000 A across ropes $ and A


os.makedirs(OUT, exist_ok=True)
for name, flags, text in inputs():
    fmd = run_ref([flags + "d"], text)
    bwt = run_ref([flags], text)
    open(os.path.join(OUT, name + ".fmd"), "wb").write(fmd)
    with open(os.path.join(OUT, name + ".bwt.gz"), "wb") as fp, gzip.GzipFile(fileobj=fp, mode="wb", mtime=0, filename="") as gz:
        gz.write(bwt)
    print(name, len(fmd), "bytes of .fmd,", len(bwt.strip()), "symbols", file=sys.stderr)
