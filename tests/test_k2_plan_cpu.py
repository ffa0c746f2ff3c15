"""Which COBS kernels a batch gets (kmcp_amd/csrc/k2_plan.hpp: the lane forms of a row, whether the device is asked for the long
queries, planes, rows per group, the pair and its refusals, block units, the chunked form, and every launch's grid pieces) compiled
for the host: every row of the table in DESIGN.md §4 with the shapes on either side of its boundaries, the grid pieces around
K2_MAX_BLOCKS, and the invariants query_device_after and the launchers rely on over a sweep of shapes (tests/k2_plan_check.cpp).
Which kernels then really run is the GPU suite's part (tests/test_gpu_k2_forms.py runs every form and reads the witness)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k2_plan_rows_boundaries_and_invariants(tmp_path):
    exe = str(tmp_path / "k2_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "k2_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
