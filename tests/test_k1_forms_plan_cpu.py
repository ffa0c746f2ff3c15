"""The K1 test plan (tests/k1_forms_plan.py) checked without a GPU, so that tests/test_gpu_k1_forms.py cannot pass vacuously:

  * k1_plan() compiled for the host (tests/k1_forms_print.cpp) gives, for every case's shape, the form, wsz, waves, grid, dynamic LDS and
    the plan bits the table declares;
  * with the oracle alone: every read meant for k1_windows_roll is one it takes (A/C/G/T, >= 1024 windows, longer than max(-u, 512), an
    emission count in (max(-u, 512), 65 536]); every list case leaves exactly what it declares, and 0 < left < n unless it declares 0;
    every -u case has queries on both sides of the bound; every fused-adjacent case has an adjacent repeat across every seam of a read
    (a read that emits one value from end to end, longer than the fused path's bound) or across the mates;
  * ALL_KERNELS is what the cases name, and k1_windows_roll<32, 4> is what no read length reaches."""
import os
import subprocess

import numpy as np
import pytest

from tests import k1_forms_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k1forms") / "k1_forms_print")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "k1_forms_print.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        out = {}
        for ln in r.stdout.splitlines():
            f = ln.split()
            out[f[0]] = dict(form=f[1], wsz=int(f[2]), waves=int(f[3]), grid=int(f[4]), grid2=int(f[5]), lds=int(f[6]), codes_direct=bool(int(f[7])),
                             list_fallback=bool(int(f[8])), adj_done=bool(int(f[9])), segs=int(f[10]), marks=bool(int(f[11])))
        return out
    return run


def test_the_plan_gives_what_the_table_declares(printer):
    got = printer([c.shape_line() for c in P.CASES])
    assert len(got) == len(P.CASES)
    wrong = []
    for c in P.CASES:
        g, e = got[c.id], c.expect
        for key in ("form", "wsz", "waves", "grid", "lds", "codes_direct", "list_fallback", "adj_done"):
            if g[key] != e[key]:
                wrong.append((c.id, key, "plan", g[key], "table", e[key]))
        second = [w for w in e["kernels"] if w[0] in ("k1_seg_roll", "k_unpack2_list") or (e["form"] == "WindowsRoll" and w[0] == "k1_windows_wave")]
        if e["form"] in ("SegRoll2", "WindowsRoll"):
            for w in second:
                if w[3] != g["grid2"]:
                    wrong.append((c.id, w[0], "plan grid2", g["grid2"], "table", w[3]))
        assert (c.left is not None) == (e["form"] in ("SegRoll2", "WindowsRoll")), c.id
        assert ("k_mark_exc" in [w[0] for w in e["kernels"]]) == g["marks"], c.id
    assert not wrong, wrong


def test_unreachable_roll_instantiation(printer):
    """WSZ 32 with KMCPG_WR_WAVES=4: whatever the longest read, the plan halves the waves (or leaves the rolling kernel out)"""
    lens = list(range(2049, 4200, 7)) + [5000, 20000, 62144, 62145, 100000, 191168, 191169, 300000]
    got = printer(["L%d 2 31 15 0 8 %d 256 3 4 0 0 0" % (L, L) for L in lens])
    assert {(g["form"], g["waves"]) for g in got.values()} == {("WindowsRoll", 2), ("WindowsRoll", 1), ("WindowsWave", 0)}
    assert P.UNREACHABLE == (("k1_windows_roll", 32, 4),)
    assert len(P.ALL_KERNELS) == 33 and len(set(P.ALL_KERNELS)) == 33


def test_all_kernels_is_what_the_cases_name():
    assert P.planned_kernels() == P.ALL_KERNELS
    assert len({c.id for c in P.CASES}) == len(P.CASES)


@pytest.fixture(scope="module")
def refs(oracle_lib):
    cache = {}

    def get(c):
        if c.id not in cache:
            cache[c.id] = P.reference(c, oracle_lib)
        return cache[c.id]
    return get


def test_roll_cases_are_not_vacuous(refs):
    n_cases = 0
    for c in P.CASES:
        if c.expect["form"] != "WindowsRoll":
            assert not c.roll_reads, c.id
            continue
        n_cases += 1
        ref = refs(c)
        bound = max(c.u, 512)
        lw = 2 * c.db.k - c.db.ws - 1
        for i in c.roll_reads:
            r, n_emit = c.reads[i], len(ref[i][0])
            assert P.is_acgt(r).all() and len(r) - lw + 1 >= 1024 and len(r) > bound, (c.id, i)
            assert bound < n_emit <= 65536, (c.id, i, n_emit)
        left = P.roll_left(c, ref)
        assert sorted(set(range(len(c.reads))) - set(left)) == sorted(c.roll_reads), (c.id, left)
        assert len(left) == c.left, (c.id, left)
        assert 0 < c.left < len(c.reads) or (c.left == 0 and len(c.reads) == 1), c.id
    assert n_cases >= 14 + 5


def test_segment_list_cases_leave_what_they_declare():
    seen = set()
    for c in P.CASES:
        if c.expect["form"] != "SegRoll2":
            continue
        n_seg = c.expect["grid"]
        left = P.seg_left(c)
        assert left == c.left, (c.id, left)
        assert 0 < left < n_seg or left == 0, c.id
        seen.add((c.codes, left > 0))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_u_cases_have_queries_on_both_sides(refs):
    n_cases = 0
    for c in P.CASES:
        if not c.u_both:
            continue
        n_cases += 1
        raw = np.array([len(a) + len(b) for a, b, _, _ in refs(c)])
        assert c.u < P.BIG and (raw > c.u).any() and ((raw <= c.u) & (raw > 0)).any(), (c.id, raw)
    assert n_cases > 30


def test_fused_adjacent_cases_have_a_repeat_across_the_seams(refs):
    n_cases = 0
    for c in P.CASES:
        fused = c.expect["adj_done"] and c.u < P.BIG
        if c.seam is None:
            continue
        assert fused, c.id
        n_cases += 1
        ref = refs(c)
        bound = max(c.u, 512)
        if c.seam == "read":     # one value from the first window to the last: whatever cuts the windows into tiles, waves or lanes cuts a run
            ok = [i for i, (a, b, _, _) in enumerate(ref) if len(a) > bound and len(a) <= 65536 and (a == a[0]).all()]
            if c.expect["form"] == "WindowsRoll":
                ok = [i for i in ok if i in c.roll_reads]
        else:                    # mate 1's last emission is mate 2's first, in a pair on the fused path
            ok = [i for i, (a, b, _, _) in enumerate(ref) if len(a) and len(b) and a[-1] == b[0] and bound < len(a) + len(b) <= 65536]
        assert ok, c.id
    assert n_cases >= 15


def test_short_mate_cases_cover_the_gate():
    """-m on pairs: mate 2 empty, shorter than k, shorter than -m while mate 1 passes, the other way round, both too short"""
    for c in P.CASES:
        if not (c.expect["form"] == "Short" and c.paired):
            continue
        L = [(len(a), len(b)) for a, b in zip(c.reads, c.reads2)]
        m, k = c.min_qlen, c.db.k
        assert m == 30
        assert any(b == 0 and a >= m for a, b in L) and any(a == 0 and b >= m for a, b in L), c.id
        assert any(a >= m and 0 < b < k for a, b in L) and any(a >= m and b < m for a, b in L) and any(a < m and b >= m for a, b in L), c.id
        assert any(a < m and b < m for a, b in L), c.id
