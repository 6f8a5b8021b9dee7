"""The host decisions of a dense round that need no GPU (csrc/rb2_round_plan.h: count_plan, merge_plan, the count record, fork_in_force,
lean_stage_in_force) over their whole input space: every 0/1 switch, RB2_STEADY_LEAN 0..2, RB2_LEAN_AUDIT 0, 1, 2 and 8, one engine and a
sharded rank, tiles on both sides of RB2_TS_MAX, the batch's stage-2 counter from 0 to 17, every fact -- against the invariants that the
driver's `internal:` fatals and the audit counter enforce, the audit cadence over 64 consecutive rounds, and named cases that pin the
defaults.  CPU only: tests/round_plan_check.cpp includes the header and is run as a program of its own, once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_round_plan_over_every_switch_and_fact(tmp_path, flags):
    exe = str(tmp_path / "round_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "round_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("ROUND PLAN OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
    points, lean2, forked, lite = (int(out.split()[i]) for i in (4, 6, 8, 10))
    # 2^6 switches x 3 lean x 4 audit x 2 ts_max, x 2 streams x 2^4 facts x 2 engines x 2 tile counts x 18 counter values
    assert points == 64 * 3 * 4 * 2 * 2 * 16 * 2 * 2 * 18
    assert 0 < forked < lean2 < points and lite > 0
