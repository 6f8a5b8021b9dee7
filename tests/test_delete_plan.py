"""The bit arithmetic of string deletion that needs no GPU (csrc/rb2_delete_plan.h: the bit compress of a group's planes by its kept mask
and the (word, shift, spill word) of a group's kept bits in the destination piece) against brute force.  CPU only:
tests/delete_plan_check.cpp includes the header and is run as a program of its own, once as the library builds it and once under
AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_delete_plan_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "delete_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "delete_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("DELETE PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    masks, splits = (int(out.split()[i]) for i in (4, 6))
    assert masks == 4 + 2 * 64 + 2 * (64 * 63 // 2) + 100000           # 0, ~0, two alternating; <= 2 set or clear bits; random
    assert splits == 5 * 64 * 65 * 3                                   # five group positions x every shift x every count x three planes
