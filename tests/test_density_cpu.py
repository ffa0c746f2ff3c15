"""The per-lane pieces of the density kernel (kmcp_amd/csrc/density_core.hpp: the segment rule with its bin and capacity boundaries, the
carry-save walk down a lane's rows, the bit-sliced add of the lanes that share 16 bytes, the expansion of planes to counts) compiled for
the host and run as simulated waves of every lane form against scalar counts of the same bits (tests/density_check.cpp).  The
reference counts the same bits one byte at a time (kmcp/cmd/index-density.go:171-213)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_density_planes_and_flushes_equal_scalar_counts(tmp_path):
    exe = str(tmp_path / "density_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "density_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout and " 0 stores over" in r.stdout, r.stdout
