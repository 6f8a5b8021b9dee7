"""The chunk cutter of rb2_hip_string_graph that needs no GPU (csrc/rb2_graph_plan.h: the strings a chunk may hold, the strings the next
chunk tries, and the cut of the strings tried at the text budget, which the device runs too) driven as the host drives it and held
against brute force: every string in exactly one chunk, every limit respected, an oversized string alone, a record budget below one
string's giving one string per chunk, and random cases.  CPU only: tests/graph_plan_check.cpp includes the header and is run as a
program of its own, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_graph_plan_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "graph_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "graph_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("GRAPH PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    cases, chunks = (int(out.split()[i]) for i in (4, 6))
    assert cases == 19 + 4000 and chunks > 3 * cases
