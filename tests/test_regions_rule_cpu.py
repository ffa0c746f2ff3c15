"""The streaming region merger of kmcp_amd/csrc/regions_rule.hpp in a stand-alone program (tests/regions_rule_check.cpp), built with the
address and undefined-behaviour sanitizers: the same windows in batches cut at every position give the bytes of one batch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batches_cut_anywhere_give_the_same_regions(tmp_path):
    exe = str(tmp_path / "regions_rule_check")
    src = os.path.join(ROOT, "tests", "regions_rule_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
