"""The arithmetic of the approximate search that needs no GPU (csrc/rb2_query_plan.h: the rows and stacks of a launch, the split of a call
into a launch for the short and one for the long queries, the packing of the substitutions, the piece bound) against brute force.  CPU
only: tests/approx_plan_check.cpp includes the header and is run as a program of its own, once as the library builds it and once under
AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_approx_plan_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "approx_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "approx_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("APPROX PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    launches, packings, bounds = (int(out.split()[i]) for i in (3, 5, 7))
    assert launches > 1000 and packings == 2000 and bounds > 1000
