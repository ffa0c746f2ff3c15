"""Which K1 kernels a batch gets (kmcp_amd/csrc/k1_plan.hpp: the form, its grids, codes read directly or expanded, who drops adjacent
repeats, the layout of the side buffer) compiled for the host: every row of the table in DESIGN.md §4 with the shapes on either side of
its boundaries, the KMCPG_K1_FLAGS bits, and the invariants run_kmers and launch_k1 rely on over a sweep of shapes
(tests/k1_plan_check.cpp).  Which kernels then really run is the GPU suite's part (tests/test_gpu_parity.py forces every form)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k1_plan_rows_boundaries_and_invariants(tmp_path):
    exe = str(tmp_path / "k1_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "k1_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
