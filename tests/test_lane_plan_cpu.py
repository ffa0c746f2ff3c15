"""The hit-buffer policy of a lane compiled alone (kmcp_amd/csrc/lane_plan.hpp through tests/lane_plan_check.cpp, g++, no GPU): how large the
device hit buffer and the eager copy of a batch are, when a leftover buffer goes back, and how the handle's hits_hint follows the data.
The policy decides whether a batch runs twice.  Properties over a grid, and spot values worked out by hand from the expressions:

  expect   = min(hint n / 1024, 512 n)                      base_cap = 8 n + 1024
  want     = max(base_cap, min(expect + expect / 2, max(base_cap, budget)))
  release  = cap > 16 want and cap > 1 << 20
  first    = min(max(cap kept, want), max(2 n + 1024, min(expect + expect / 4, (32 | 1024) n)))
  hint'    = per_k if per_k > old else old - old / 8 + per_k / 8,   per_k = 1024 cnt / n + 1"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lane_plan") / "lane_plan_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "lane_plan_check.cpp")], check=True)
    lib = C.CDLL(so)
    lib.lp_plan.restype = None
    lib.lp_plan.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    lib.lp_hint.restype = C.c_uint64
    lib.lp_hint.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    return lib


def plan(chk, n, hint, budget, cap, generous=False):
    out = (C.c_uint64 * 4)()
    chk.lp_plan(n, hint, budget, cap, int(generous), out)
    return dict(base_cap=out[0], want=out[1], release=bool(out[2]), first=out[3])


NS = (1, 1023, 1024, 1 << 20)
HINTS = (0, 1, 1024, 1 << 20)
BUDGETS = (0, 20000, 1 << 40)


def test_properties_over_the_grid(chk):
    released = kept = 0
    for n in NS:
        for hint in HINTS:
            for budget in BUDGETS:
                for generous in (False, True):
                    base = plan(chk, n, hint, budget, 0, generous)
                    for cap in (0, base["base_cap"], 17 * base["want"]):
                        h = plan(chk, n, hint, budget, cap, generous)
                        what = (n, hint, budget, cap, generous, h)
                        assert h["base_cap"] == 8 * n + 1024 <= h["want"], what
                        assert (h["base_cap"], h["want"]) == (base["base_cap"], base["want"]), what  # neither depends on the lane's buffer
                        assert h["want"] <= max(h["base_cap"], budget), what  # within the lane's share of the budget
                        assert h["first"] <= max(cap, h["want"]), what
                        assert h["first"] >= min(cap, 2 * n + 1024), what
                        assert h["release"] == (cap > 16 * h["want"] and cap > 1 << 20), what
                        if h["release"]:  # the eager copy is sized for the buffer that will be there
                            assert h["first"] <= h["want"], what
                        released += h["release"]
                        kept += not h["release"]
    assert released and kept


def test_spot_values_worked_out_by_hand(chk):
    # a cold handle, 1024 reads: the plain sizes
    assert plan(chk, 1024, 0, 0, 0) == dict(base_cap=9216, want=9216, release=False, first=3072)
    # 2^20 reads, 2^20 hits per 1024 reads: expect = min(2^30, 512 n = 2^29); want = 1.5 expect; the eager copy stops at 32 per read ...
    assert plan(chk, 1 << 20, 1 << 20, 1 << 40, 0) == dict(base_cap=8389632, want=805306368, release=False, first=33554432)
    # ... and a piece of a large call takes expect + 25 % (below 1024 per read)
    assert plan(chk, 1 << 20, 1 << 20, 1 << 40, 0, True)["first"] == 671088640
    # 1023 reads, one hit per read: expect = 1023, want stays the plain size, first = 2 n + 1024
    assert plan(chk, 1023, 1024, 100, 0) == dict(base_cap=9208, want=9208, release=False, first=3070)
    # the budget caps want (20 000 < 1.5 x 524 288), and first cannot exceed the buffer
    assert plan(chk, 1024, 1 << 20, 20000, 0) == dict(base_cap=9216, want=20000, release=False, first=20000)
    # ... unless the lane already has a larger one
    assert plan(chk, 1024, 1 << 20, 20000, 30000)["first"] == 30000
    assert plan(chk, 1024, 1 << 20, 20000, 40000)["first"] == 32768
    # a leftover buffer: 17 x want of one read is below 2^20 entries and stays; 2^20 + 1 entries go back
    assert plan(chk, 1, 0, 0, 17 * 1032) == dict(base_cap=1032, want=1032, release=False, first=1026)
    assert plan(chk, 1, 0, 0, (1 << 20) + 1) == dict(base_cap=1032, want=1032, release=True, first=1026)
    assert plan(chk, 1, 0, 0, 1 << 20)["release"] is False
    assert plan(chk, 1 << 20, 0, 0, 17 * 8389632) == dict(base_cap=8389632, want=8389632, release=True, first=2098176)
    assert plan(chk, 1 << 20, 0, 0, 16 * 8389632)["release"] is False


def test_hint_rises_at_once_and_decays_by_an_eighth(chk):
    assert chk.lp_hint(0, 5000, 1024) == 5001
    assert chk.lp_hint(8000, 0, 1024) == 7000  # per_k = 1: 8000 - 1000 + 0
    assert chk.lp_hint(5001, 5000, 1024) == 5001  # per_k == old: the decay step, which leaves it where it is
    assert chk.lp_hint(100, 3 << 20, 1 << 20) == 3073  # 3 hits per read
    for n in NS[1:]:
        for old in HINTS + (12345,):
            for cnt in (0, 1, n, 7 * n + 3, 512 * n):
                per_k = cnt * 1024 // n + 1
                want = per_k if per_k > old else old - old // 8 + per_k // 8
                assert chk.lp_hint(old, cnt, n) == want, (old, cnt, n)
                assert chk.lp_hint(old, cnt, n) >= min(old, per_k)
