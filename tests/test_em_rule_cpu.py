"""kmcp_amd/csrc/em_rule.hpp in a stand-alone program (tests/em_rule_check.cpp), built with the address and undefined-behaviour
sanitizers: on random reads the conservation law (an assigned read adds exactly EM_UNIT to match), a target's rows summing to its p, the
two-word bases against unsigned __int128, the placement of the deficit; the roll-up, the loop's ways to stop, the end's order and -F."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shares_bases_rollup_loop_and_end(tmp_path):
    exe = str(tmp_path / "em_rule_check")
    src = os.path.join(ROOT, "tests", "em_rule_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
