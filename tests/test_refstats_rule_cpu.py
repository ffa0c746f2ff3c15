"""kmcp_amd/csrc/refstats_rule.hpp in a stand-alone program (tests/refstats_rule_check.cpp), built with the address and
undefined-behaviour sanitizers: the per-query counting against a literal count, the row cuts, the roll-up, the verdict at its boundaries
(chunksFrac exactly p) and the mode table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_counting_rollup_verdict_and_modes(tmp_path):
    exe = str(tmp_path / "refstats_rule_check")
    src = os.path.join(ROOT, "tests", "refstats_rule_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
