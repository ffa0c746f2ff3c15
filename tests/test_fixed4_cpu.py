"""The merge order of database sets compiled for the host (kmcp_amd/csrc/k3_set_order.hpp): fixed4 — the integer "%.4f" prints, from
mantissa and exponent alone — against snprintf, with no tolerance; and the set order (the device's second pass and its host twin) against
"print every score with %.4f, parse it back, stable-sort descending over (member, exact K3 order)", which is what kmcp-merge does with the
members' separate results.  The program is tests/fixed4_check.cpp, compiled with g++ as tests/test_k3_keys_cpu.py compiles its check."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097)  # the edges of a wave, of the wave class and of the workgroup class


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fixed4") / "fixed4_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "fixed4_check.cpp")], check=True)
    lib = C.CDLL(so)
    lib.fixed4_sweep.restype = None
    lib.fixed4_sweep.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    lib.set_order_check.restype = C.c_int
    lib.set_order_check.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    return lib


def test_fixed4_prints_what_percent_4f_prints(chk):
    out = (C.c_uint64 * 2)()
    first_bad = C.c_double(-1)
    chk.fixed4_sweep(2026, out, C.byref(first_bad))
    # every c / n for n <= 300, 1000 random c for five larger n, the 20001 half-way cases with both neighbours, 0, 1, 2^-46, 10^6 random doubles
    assert out[0] > 1_100_000
    assert out[1] == 0, f"{out[1]} of {out[0]} values differ from %.4f, the first one is {first_bad.value!r}"


@pytest.mark.parametrize("sort_mode", [0, 1, 2], ids=["qcov", "tcov", "jacc"])
def test_set_order_is_the_merge_order(chk, sort_mode):
    ties = adjacent = mixed = 0
    for m in LENGTHS:
        for seed in range(3):
            t = (C.c_uint64 * 3)()
            bad = chk.set_order_check(sort_mode, m, seed, t)
            assert bad == 0, f"-s mode {sort_mode}, {m} matches, seed {seed}: mismatch mask {bad} (1 two-pass order, 2 host twin, 4 / 8 their mixed-run counts)"
            ties += t[0]
            adjacent += t[1]
            mixed += t[2]
    # the tie rule is exercised: at least a third of the adjacent printed scores are equal, and such runs span members
    assert 3 * ties >= adjacent > 0, (ties, adjacent)
    assert mixed > 100, mixed
