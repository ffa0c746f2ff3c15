"""kmcp_amd/csrc/cooccur_rule.hpp in a stand-alone program (tests/cooccur_rule_check.cpp), built with the address and
undefined-behaviour sanitizers: the pair key (symmetric, never 0, round trip), the probe sequence (K7_PROBES distinct slots at table sizes
1, 2, 8 and 2^20), the two-phase count simulated read by read on an 8-slot table (a read is counted completely or not at all), the pairs
of a query and the row cuts of stage 2."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_probes_two_phase_count_and_cuts(tmp_path):
    exe = str(tmp_path / "cooccur_rule_check")
    src = os.path.join(ROOT, "tests", "cooccur_rule_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
