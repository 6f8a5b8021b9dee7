"""CPU tests of the boundary of the irreducible-overlap query: librb2hip.so exports its two entry points and HipBwt has its four methods,
and the arithmetic that sizes the stacks of a launch (csrc/rb2_query_plan.h: the entry cap, the bytes of a row, the rows) holds at its
edges -- tests/irreducible_plan_check.cpp includes the header and runs as a program of its own, once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer.  The fatal argument checks need a handle, and a handle needs a device: they are in
tests/test_irreducible_gpu.py.  No GPU needed."""
import os
import re
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_symbols_and_methods():
    from ropebwt2_amd import HipBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS
    build_all()
    L = load_hip_lib()
    for s in ("rb2_hip_irreducible", "rb2_hip_irreducible_dev"):
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    assert len(L.rb2_hip_irreducible.argtypes) == 10 and len(L.rb2_hip_irreducible_dev.argtypes) == 11
    for m in ("irreducible_raw", "irreducible_dev", "irreducible", "edges"):
        assert callable(getattr(HipBwt, m, None)), m


def test_header_says_whose_ids_the_records_name():
    txt = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    sec = txt[txt.index("irreducible overlaps"):txt.index("rb2_hip_irreducible_dev(")]
    assert "revcomp(T)" in sec and re.search(r"REVERSE COMPLEMENTS", sec) and "rb2_hip_string_ids" in sec
    assert "RB2_IRRED_SCRATCH" in sec and "RB2_IRRED_SCRATCH" in open(os.path.join(H.ROOT, "INTEGRATION.md")).read()


def test_kernel_is_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    assert b"k_irreducible" in open(lib_path("librb2hip.so"), "rb").read()


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_plan_arithmetic(tmp_path, flags):
    exe = str(tmp_path / "irreducible_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "irreducible_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("IRRED PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    caps, rows = (int(out.split()[i]) for i in (3, 5))
    assert caps > 4000 and rows > 500
