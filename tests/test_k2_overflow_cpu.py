"""tests/k2_overflow.py without a GPU: the checker of tests/test_gpu_k2_overflow.py against crafted outputs — a correct run passes, every
way of breaking the hit buffer's contract is reported under its own name — and the case table against k2_forms_plan, the rules of
kmcp_amd/csrc/k2_plan.hpp compiled for the host, and the list of cases the three emission sites need."""
import os
import subprocess

import numpy as np
import pytest

from tests import k2_forms_plan as P
from tests import k2_overflow as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOLS, N_READS = 1000, 40


@pytest.fixture(scope="module")
def ref():
    """a list of 3 000 hits of 40 reads over 1 000 columns, with a run of 200 neighbours"""
    rng = np.random.default_rng(7)
    keys = np.unique(np.concatenate([rng.choice(N_READS * NCOLS, 2800, replace=False), 17 * NCOLS + np.arange(200)])).astype(np.int64)
    return keys, rng.integers(1, 255, len(keys)).astype(np.int64)


def _run(ref, cap, seed=1):
    """a correct run: the counter is T, the first min(cap, T) rows hold distinct hits in some order, nothing else is written"""
    keys, cnts = ref
    order = np.random.default_rng(seed).permutation(len(keys))[:min(cap, len(keys))]
    buf = np.full((cap + V.GUARD, 3), V.SENTINEL, dtype=np.uint32)
    buf[:len(order)] = np.stack([keys[order] // NCOLS, keys[order] % NCOLS, cnts[order]], axis=1)
    return len(keys), buf.view(np.int32)  # as the device buffer comes back: int32


def _names(problems):
    return sorted(p.split(":")[0] for p in problems)


@pytest.mark.parametrize("cap", ["0", "1", "64", "T-1", "T", "T+1", "2T"])
def test_a_correct_run_passes(ref, cap):
    T = len(ref[0])
    cap = eval(cap.replace("2T", "2*T"), {"T": T})
    counter, buf = _run(ref, cap)
    assert V.check_run(ref[0], ref[1], NCOLS, cap, counter, buf) == []


def test_a_count_only_call_passes(ref):
    assert V.check_run(ref[0], ref[1], NCOLS, 0, len(ref[0]), np.zeros((0, 3), dtype=np.int32)) == []
    assert _names(V.check_run(ref[0], ref[1], NCOLS, 0, 0, np.zeros((0, 3), dtype=np.int32))) == ["counter"]


# ---- the ways a run can break the contract: each changes a correct run (counter, buf as uint32 [cap + GUARD, 3]) in one place --------------
MUTANTS = {}   # name -> (cap as a function of T, the change -> the counter, what the checker must name)


def mutant(name, want, cap=lambda T: T // 2):
    def register(change):
        MUTANTS[name] = (cap, change, want)
        return change
    return register


@mutant("counter one too small", ["counter"])
def _(ref, T, cap, counter, b):
    return counter - 1


@mutant("counter saturates at cap", ["counter"])
def _(ref, T, cap, counter, b):
    return cap


@mutant("row written at index cap", ["beyond"])
def _(ref, T, cap, counter, b):
    b[cap] = b[0]
    return counter


@mutant("row written at cap + GUARD - 1", ["beyond"])
def _(ref, T, cap, counter, b):
    b[cap + V.GUARD - 1] = b[0]
    return counter


@mutant("hole in the middle", ["hole"])
def _(ref, T, cap, counter, b):
    b[cap // 2] = V.SENTINEL
    return counter


@mutant("hole in the middle of a full list", ["hole", "list"], cap=lambda T: T)
def _(ref, T, cap, counter, b):
    b[cap // 2] = V.SENTINEL
    return counter


@mutant("duplicate entry", ["duplicate"])
def _(ref, T, cap, counter, b):
    b[5] = b[900]
    return counter


@mutant("full list with one hit stored twice", ["duplicate", "list"], cap=lambda T: T)
def _(ref, T, cap, counter, b):
    b[3] = b[4]
    return counter


@mutant("real key, wrong count", ["count"])
def _(ref, T, cap, counter, b):
    b[7, 2] += 1
    return counter


@mutant("tombstone", ["tombstone"])
def _(ref, T, cap, counter, b):
    b[9] = [V.TOMBSTONE, V.TOMBSTONE, 0]
    return counter


@mutant("tuple of a read outside the list", ["foreign"])
def _(ref, T, cap, counter, b):
    b[11, 0] = N_READS
    return counter


@mutant("tuple of a column that is no hit", ["foreign"])
def _(ref, T, cap, counter, b):
    key = int(np.setdiff1d(np.arange(N_READS * NCOLS), ref[0])[0])
    b[11] = [key // NCOLS, key % NCOLS, 3]
    return counter


@mutant("column past the row", ["foreign"])
def _(ref, T, cap, counter, b):
    assert b[11, 0] > 0        # (read - 1, col + ncols) has the key of the real hit it replaces
    b[11] = [b[11, 0] - 1, b[11, 1] + NCOLS, b[11, 2]]
    return counter


@mutant("unused tail touched, cap > T", ["beyond"], cap=lambda T: T + 100)
def _(ref, T, cap, counter, b):
    b[T + 50] = b[0]
    return counter


@mutant("one word of the tail touched", ["beyond"], cap=lambda T: T + 100)
def _(ref, T, cap, counter, b):
    b[T, 2] = 0
    return counter


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_broken_promise_is_named(ref, name):
    cap_of, change, want = MUTANTS[name]
    T = len(ref[0])
    cap = cap_of(T)
    counter, buf = _run(ref, cap)
    counter = change(ref, T, cap, counter, buf.view(np.uint32))
    problems = V.check_run(ref[0], ref[1], NCOLS, cap, counter, buf)
    assert _names(problems) == want, problems


# ---- a CPU model of the emission, and the two ways a kernel could get it wrong --------------------------------------------------------
def _waves(ref, site):
    """the reference cut into the reservations one wave makes: A — up to 16 reads x the 512 columns of a 4-lane unit; B — one read x one
    1-KiB tile; C — 64 consecutive (read, column) words of the count array"""
    keys = ref[0]
    r, c = keys // NCOLS, keys % NCOLS
    wave = {"A": (r // 16) * 64 + c // 512, "B": r * 64 + c // 8192, "C": keys // 64}[site]
    rows = np.stack([r, c, ref[1]], axis=1)
    return [rows[wave == w] for w in np.unique(wave)]


def _emit(waves, cap, seed, count_all=True, guarded=True):
    """one atomicAdd per wave, then `if (idx < cap)` stores, the waves in any order.  count_all=False: the counter advances by what was
    stored; guarded=False: the store is not guarded (rows past the model's buffer are dropped: the model has no memory to corrupt)"""
    buf = np.full((cap + V.GUARD, 3), V.SENTINEL, dtype=np.uint32)
    counter = 0
    for w in np.random.default_rng(seed).permutation(len(waves)):
        base = counter
        counter += len(waves[w]) if count_all else max(0, min(len(waves[w]), cap - base))
        for j, hit in enumerate(waves[w]):
            if base + j < (cap if guarded else len(buf)):
                buf[base + j] = hit
    return counter, buf


@pytest.mark.parametrize("site", ["A", "B", "C"])
def test_the_emission_model_and_its_mutants(ref, site):
    T = len(ref[0])
    waves = _waves(ref, site)
    assert sum(len(w) for w in waves) == T and max(len(w) for w in waves) > 1
    for cap in (0, 1, 65, T // 3 | 1, T - 1, T, T + 1):
        counter, buf = _emit(waves, cap, seed=cap)
        assert V.check_run(ref[0], ref[1], NCOLS, cap, counter, buf) == [], (site, cap)
    for cap in (0, 1, 65, T // 3 | 1, T - 1):
        counter, buf = _emit(waves, cap, seed=cap, count_all=False)
        assert _names(V.check_run(ref[0], ref[1], NCOLS, cap, counter, buf)) == ["counter"], (site, cap)
        counter, buf = _emit(waves, cap, seed=cap, guarded=False)
        assert _names(V.check_run(ref[0], ref[1], NCOLS, cap, counter, buf)) == ["beyond"], (site, cap)


def test_capacities():
    for T in (512, 513, 1999, 1 << 18):
        caps = V.capacities(T)
        assert len(caps) == len(set(caps)) == 25
        assert caps[:2] == [T + 1, T] and caps[-1] == T - 1     # ... so that the rerun with T follows a run that overflowed
        assert {None, 0, 1, 63, 64, 65} <= set(caps)
        odd = [c for c in caps if c is not None and 65 < c < T - 1]
        assert len(odd) == 16 and all(c % 2 for c in odd)
        assert max(np.diff([65] + odd + [T - 1])) <= (T - 66) / 17 + 2   # spread evenly


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def test_batches():
    for name, ns in V.BATCH_N.items():
        stay = [n for n in ns if n <= V.SPLIT_MIN] if name == "8s" else ns     # what the launches that are not chunked meet
        assert P.planes_for(max(stay)) == V.PLANES[name]
        a, b = V.planted(name)
        assert a != b and ns[a] >= 100 and ns[b] >= (16 if name == "8s" else 100)
    for name in ("8", "8s", "10"):
        ns = V.BATCH_N[name]
        assert 36 <= len(ns) <= 44 and len(ns) % 4 != 0
        assert ns.count(130) > len(ns) // 2 and {0, 1, 5, 64, 129, 131, 254} <= set(ns)
    assert max(V.BATCH_N["8"]) == 254 and 400 in V.BATCH_N["8s"] and {255, 1022} <= set(V.BATCH_N["10"])
    short = [n for n in V.BATCH_N["8s"] if n <= V.SPLIT_MIN]
    assert len([n for n in short if n > 0]) >= 4 and V.SPLIT_MIN in short
    ns = V.BATCH_N["16"]
    assert 12 <= len(ns) <= 13 and min(ns) == 1023 and max(ns) == 2048 == P.SPLIT_DEFAULT


def test_case_ids_are_unique():
    ids = [c.id for c in V.CASES]
    assert len(ids) == len(set(ids))
    # database by database: no database is opened twice
    dbs = [c.db for c in V.CASES]
    assert [d for i, d in enumerate(dbs) if i == 0 or dbs[i - 1] != d] == list(dict.fromkeys(dbs))


def test_every_expectation_is_the_plans():
    for c in V.CASES:
        assert c.expect == tuple(P.expect(V.DB[c.db], V.BATCH_N[c.batch], c.env)), c.id
        plain = [f for f in c.expect if f[0] != "split"]
        assert plain and all(f[3] == V.PLANES[c.batch] for f in plain), c.id
        assert any(f[0] == "split" for f in c.expect) == (c.site == "C"), c.id


def test_short_read_knobs_come_with_four_rows():
    """without KMCPG_GROUP_ROWS=4 short_flags is 0 in k2_plan.hpp and a case that sets a KMCPG_K2_ knob runs site A"""
    for c in V.CASES:
        if any(k in c.env for k in V.K2_KNOBS):
            assert c.env.get("KMCPG_GROUP_ROWS") == "4", c.id
        # what k2_plan needs for the short-read unit: a 64-lane class, one hash function, 8 or 10 planes, 4 rows, pruning as it is
        d = V.DB[c.db]
        unit = (c.env.get("KMCPG_GROUP_ROWS") == "4" and d.nh == 1 and ("plain", 64, 0, V.PLANES[c.batch], False, 4) in c.expect and "KMCPG_PRUNE" not in c.env and
                "KMCPG_PRUNE_EVERY" not in c.env and (c.env.get("KMCPG_K2_BLOCK_UNITS", "0") != "0" or c.env.get("KMCPG_K2_EXACT_STOP", "1") != "0"))
        assert unit == (c.site == "B" or (c.site == "C" and c.db == "x2-h1")), c.id
        assert (c.grid is not None) == (c.db in ("x2-h1", "n64f-h1")), c.id
        if unit:
            persist = c.env.get("KMCPG_K2_PERSIST", "1") != "0" and c.env.get("KMCPG_K2_BLOCK_UNITS", "0") == "0"
            wgs = c.env.get("KMCPG_K2_PERSIST_WGS")
            assert c.grid == ((int(wgs) if wgs else "resident") if persist else ("block" if c.env.get("KMCPG_K2_BLOCK_UNITS") == "1" else "piece")), c.id
        else:
            assert c.grid in (None, "piece"), c.id


# the cases the three sites need: (site, database, batch, settings), each met by a case of its own
_GR4 = {"KMCPG_GROUP_ROWS": "4"}
REQUIRED = [("A", dbk, "8", {}) for dbk in ("n4s-h1", "f8-h1", "n16a-h3", "n32a-h1", "n64p-h1", "t3-h1")] + [
    ("A", "n8-h1", "10", _GR4),
    ("A", "x2-h1", "8", dict(_GR4, KMCPG_K2_EXACT_STOP="0", KMCPG_K2_BLOCK_UNITS="0")),
    ("A", "p16-h1", "16", {}),
    ("B", "x2-h1", "8", dict(_GR4, KMCPG_K2_PERSIST="0")),
    ("B", "x2-h1", "10", dict(_GR4, KMCPG_K2_PERSIST="0")),
    ("B", "x2-h1", "8", dict(_GR4, KMCPG_K2_PERSIST="1")),
    ("B", "x2-h1", "8", dict(_GR4, KMCPG_K2_PERSIST="1", KMCPG_K2_PERSIST_WGS="1")),
    ("B", "x2-h1", "8", dict(_GR4, KMCPG_K2_PERSIST="1", KMCPG_K2_PERSIST_WGS="3")),
    ("B", "x2-h1", "8", dict(_GR4, KMCPG_K2_BLOCK_UNITS="1", KMCPG_K2_EXACT_STOP="1")),
    ("B", "x2-h1", "8", dict(_GR4, KMCPG_K2_BLOCK_UNITS="1", KMCPG_K2_EXACT_STOP="0")),
    ("B", "n64f-h1", "8", _GR4),
    ("C", "n8-h1", "8s", {"KMCPG_SPLIT_MIN": "16"}),
    ("C", "n8-h1", "8s", {"KMCPG_SPLIT_MIN": "16", "KMCPG_SPLIT_CHUNK": "64"}),
    ("C", "x2-h1", "8s", dict(_GR4, KMCPG_SPLIT_MIN="16")),
]


def test_every_required_case_has_a_case_of_its_own():
    met = []
    for req in REQUIRED:
        hit = [c.id for c in V.CASES if (c.site, c.db, c.batch, c.env) == req]
        assert len(hit) == 1, (req, hit)
        met += hit
    assert len(set(met)) == len(REQUIRED) == 20
    # the forms the sites are named for
    by = {c.id: c for c in V.CASES}
    assert [by[i].expect for i in met[:6]] == [(("plain", 4, 0, 8, False, 8),), (("plain", 8, 0, 8, False, 8),), (("plain", 16, 0, 8, True, 8),),
                                               (("plain", 32, 0, 8, False, 8),), (("plain", 64, 0, 8, False, 8),),
                                               (("plain", 8, 0, 8, False, 8), ("plain", 32, 0, 8, False, 8), ("plain", 64, 0, 8, False, 8))]
    assert by[met[6]].expect == (("plain", 8, 0, 10, False, 4),)
    assert by[met[7]].expect == (("plain", 64, 0, 8, False, 4),)
    assert by[met[8]].expect == (("pair", 64, 16, 16, False, 8),)
    assert all(by[i].expect == (("plain", 64, 0, V.PLANES[by[i].batch], False, 4),) for i in met[9:17])
    assert by[met[17]].expect == by[met[18]].expect == (("plain", 8, 0, 8, False, 8), ("split", 8, 0, 16, False, 8))
    assert by[met[19]].expect == (("plain", 64, 0, 8, False, 4), ("split", 64, 0, 16, False, 8))
    x2 = V.X2
    assert (x2.cols, x2.blocks, x2.step) == (14973, 3, 4099) and (x2.cols + 7) // 8 == 1872 and x2.stride1 == x2.stridem == 1920 == 1024 + 896
    assert P.lane_classes(1920, 1) == ([64], {64: 2})
    assert "x2" not in [l.name for l in P.LAYOUTS] and "x2-h1" not in P.DB      # the forms test does not get it


def test_the_rules_themselves_launch_what_the_table_expects(tmp_path):
    """kmcp_amd/csrc/k2_plan.hpp compiled for the host (tests/k2_forms_print.cpp) decides every case, as in test_k2_forms_plan_cpu.py"""
    exe = str(tmp_path / "k2_forms_print")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "k2_forms_print.cpp")], check=True)
    lines = []
    for c in V.CASES:
        db, ns = V.DB[c.db], V.BATCH_N[c.batch]
        lay = P.LAYOUT[db.layout]
        split_min = int(c.env.get("KMCPG_SPLIT_MIN", P.SPLIT_DEFAULT))
        longs = [n for n in ns if n > split_min]
        f = [c.id, P.stride_of(db), db.nh, 1 if lay.step == 0 else lay.blocks, 1, 1, -1, len(ns), max(ns), 0, len(longs), max(longs, default=0),
             int("KMCPG_SPLIT_MIN" in c.env), split_min, int("KMCPG_SPLIT_CHUNK" in c.env), int(c.env.get("KMCPG_SPLIT_CHUNK", 0)), 1,
             int("KMCPG_GROUP_ROWS" in c.env), int(c.env.get("KMCPG_GROUP_ROWS", 0)), 1, 1, 1]
        lines.append(" ".join(str(x) for x in f))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(V.CASES)
    for c, ln in zip(V.CASES, out):
        cid, _, _, forms = ln.split()
        got = []
        for f in forms.split(","):
            kind, lpr, lprb, npl, multi, gr = f.split("/")
            got.append((kind, int(lpr), int(lprb), int(npl), bool(int(multi)), int(gr)))
        assert cid == c.id and tuple(sorted(got)) == c.expect, (c.id, got, c.expect)
