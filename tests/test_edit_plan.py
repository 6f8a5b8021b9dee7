"""The arithmetic of the approximate search with insertions and deletions that needs no GPU (csrc/rb2_edit_plan.h: the packed column, the
terminal and the live test with the piece bound, the rows and stacks of a launch, the split of a call into two launches) against brute
force.  CPU only: tests/edit_plan_check.cpp includes the header and is run as a program of its own, once as the library builds it and once
under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_edit_plan_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "edit_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "edit_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("EDIT PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    launches, columns, searches, matches, pruned = (int(out.split()[i]) for i in (3, 5, 7, 9, 11))
    assert launches > 1000 and columns > 10000 and searches > 3000 and matches > 5000 and pruned > 500
