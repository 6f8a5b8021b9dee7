"""The batch-cutting arithmetic of rb2_hip_merge that needs no GPU (csrc/rb2_merge_plan.h: the end of the next batch from the block sums
of the offsets and one fetched block; the default budget) against brute force over the whole offset array: a budget of 1, a budget of
one string exactly and minus 1, an oversized string first, last and alone, all-empty strings, the per-batch string limit reached before
the byte budget, and random cases.  CPU only: tests/merge_plan_check.cpp includes the header and is run as a program of its own, once
plain and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_merge_plan_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "merge_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "merge_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("MERGE PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    cases, cuts = (int(out.split()[i]) for i in (4, 6))
    assert cases == 7 * 21 + 4000 and cuts > 20 * cases
