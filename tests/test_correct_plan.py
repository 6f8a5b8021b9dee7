"""The correction rule and its launch arithmetic without a GPU (csrc/rb2_correct_plan.h: correct_read, the text the kernel k_correct
compiles, and the rows and solid bits of a launch) against a brute force over tiny string sets.  CPU only: tests/correct_plan_check.cpp
includes the header and is run as a program of its own, once as the library builds it and once under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_correct_plan_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "correct_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "correct_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("CORRECT PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    w = out.split()
    reads, runs, budgets, fixed, over = (int(w[w.index(k) + 1]) for k in ("reads", "runs", "budgets", "fixed", "over"))
    assert reads == 240 and runs > 5000 and budgets > 50000 and fixed > 500 and over > 50000
