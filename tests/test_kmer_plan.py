"""The arithmetic of the k-mer enumeration that needs no GPU (csrc/rb2_kmer_plan.h: the packing of a k-mer and the reverse complement of
a code for k = 1 .. 32, the slices of the depth-first walk, the sizes of its segments, the flush points of the record staging) against
brute force.  CPU only: tests/kmer_plan_check.cpp includes the header and is run as a program of its own, once as the library builds it
and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_kmer_plan_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "kmer_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "kmer_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("KMER PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    codes, slices, launches = (int(out.split()[i]) for i in (3, 5, 7))
    assert codes == 32 * 200 and slices > 1000 and launches > 1000
