"""kmcp_amd/csrc/recount_rule.hpp in a stand-alone program (tests/recount_rule_check.cpp), built with the address and
undefined-behaviour sanitizers: the elimination in bit masks against the reference's literal double loop on random predicates (one word
and several, the three-target quirk case), the shares of a target's rows summing to 720720 for 1..4096 rows, the tie order, a read's adds
and every verdict of stage 3."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_masks_shares_order_adds_and_verdicts(tmp_path):
    exe = str(tmp_path / "recount_rule_check")
    src = os.path.join(ROOT, "tests", "recount_rule_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
