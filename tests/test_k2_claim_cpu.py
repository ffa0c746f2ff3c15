"""The unit queue of the persistent short-read COBS kernel (kmcp_amd/csrc/k2_claim.hpp) compiled for the host: whatever the number of
units, unit_base, run length, number of claimers and their interleaving, every unit is produced exactly once and in order, and the
pieces of a launch cover the batch once (tests/k2_claim_check.cpp).  The program is built with AddressSanitizer and
UndefinedBehaviorSanitizer and run on its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k2_claims_cover_every_unit_once_in_order(tmp_path):
    exe = str(tmp_path / "k2_claim_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "k2_claim_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
