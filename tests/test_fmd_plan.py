"""The arithmetic of the device .fmd encoder that needs no GPU (csrc/rb2_fmd_plan.h: the code of a run, header type and words, payload
bits, the fit rule as a bisection over the prefix sum of the code widths, the frame rule) against the host writer (csrc/host/fmd.c).
CPU only: tests/fmd_plan_check.cpp builds a serial encoder out of the plan functions alone, links the host writer as the oracle and
compares whole images; it runs as a program of its own, once with -O3 (which adds the stream that crosses a chunk of 2^23 words) and once
under AddressSanitizer + UndefinedBehaviorSanitizer (the plan header and the check program; the writer is linked as the library builds it)."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HOST = os.path.join(CSRC, "host")
INC = os.path.join(H.ROOT, "include")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
PROBES = 70 + 3 * 44                     # every l in 1..70; 2^k - 1, 2^k, 2^k + 1 for k = 7..50


@pytest.mark.parametrize("flags,big", [(["-O3"], True), (SAN, False)], ids=["plain", "sanitized"])
def test_plan_encoder_against_the_host_writer(tmp_path, flags, big):
    exe = str(tmp_path / "fmd_plan_check")
    objs = []
    for c in ("fmd.c", "rle.c"):                                   # the oracle, as the library builds it
        o = str(tmp_path / (c + ".o"))
        subprocess.run(["gcc", "-O2", "-g", "-std=gnu99", "-I" + INC, "-I" + HOST, "-c", os.path.join(HOST, c), "-o", o], check=True)
        objs.append(o)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-I" + INC, "-o", exe, os.path.join(HERE, "fmd_plan_check.cpp")] + objs + ["-lpthread"], check=True)
    p = subprocess.run([exe] + (["big"] if big else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("FMD PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    f = out.split()
    n = {k: int(f[f.index(k) + 1]) for k in ("alone", "ones", "aligned", "wide", "types", "random", "chunk", "transitions", "edges", "events", "undefined", "model_only_w64_at_c64")}
    # A 64-bit code right behind a code that ended on a word boundary makes the writer (and rld0.c:145) shift a word by 64: those streams
    # are encoded by the model and counted, not compared, and what the model met in them counts for no coverage.  They are among the aligned
    # and the wide ones.  A 64-bit code at u == C - 64 > 0 is always such a case (C is a multiple of 64): the program requires that no compared
    # stream holds one and reports how many the model encoded; a 64-bit code that fills a block from u == C - 64 == 0 is compared.
    assert n["alone"] == 1 + 2 * PROBES and n["ones"] == 8 and n["types"] == 6 * 3 + 1 and n["random"] == 1
    assert n["undefined"] == 151 and n["model_only_w64_at_c64"] == 63
    assert n["aligned"] == 97 * PROBES - 10 and n["wide"] == 97 * 7 - 141
    assert n["chunk"] == (1 if big else 0)
    assert n["transitions"] == 9 and n["edges"] == 4 and n["events"] == 5     # all from compared streams: word end, bit before the last, last bit, refused on the last bit, 64 bits at a block's first bit
