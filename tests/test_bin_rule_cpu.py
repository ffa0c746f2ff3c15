"""kmcp_amd/csrc/bin_rule.hpp in a stand-alone program (tests/bin_rule_check.cpp), built with the address and undefined-behaviour
sanitizers: the pre-order tables of the pruned tree (parent, last, taxid) over 400 random forests of up to 30 nodes — several roots,
absent, deleted and merged ids, references on leaves and on inner nodes — and chains of depth 41, 48 and 100; bin_lca(min, max) against a
brute-force LCA by ancestor sets for every subset of up to three references; the missing-TaxId refusal; the per-query accumulator."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_preorder_tables_and_lca_of_min_and_max(tmp_path):
    exe = str(tmp_path / "bin_rule_check")
    src = [os.path.join(ROOT, "tests", "bin_rule_check.cpp"), os.path.join(ROOT, "kmcp_amd", "csrc", "taxonomy.cpp")]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe] + src, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "403 cases" in r.stdout and " 0 wrong" in r.stdout, r.stdout
