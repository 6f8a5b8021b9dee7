"""The launch arithmetic of the query host layer (csrc/rb2_query_plan.h: the staging budget, record_chunk, split_slots) against brute
force.  CPU only: tests/query_plan_check.cpp includes the header, is built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a
program of its own.  split_slots is checked with launch caps below max_hits too: the engine's own caps (2^24, 2^28) put that branch out
of reach of any test-sized query."""
import os
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))


def test_query_plan_against_brute_force(tmp_path):
    exe = str(tmp_path / "query_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I" + CSRC, "-o", exe, os.path.join(HERE, "query_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    assert int(out.split()[2]) > 9 * 20 * 7                          # (n = 0 makes no call; most of the others make several)
