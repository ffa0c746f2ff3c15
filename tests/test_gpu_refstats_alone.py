"""K6 alone (kmcp_amd/csrc/k6_refstats.hip), driven through kmcpg_refstats_device on pair lists the test lays out, against the plain
restatement of stage 1 of profile.go (tests/refstats_reference.py stage1) fed the way the TSV route feeds it: one row per pair, its qCov
printed with "%.4f" and parsed back.  Compared: all four counters of every column, the totals, the LEFT bytes (and the guard bytes behind
them), the inputs (unchanged), and the witness: the class each read took, where the adds went.

The table: three columns per target (its chunks); a species joins two neighbouring targets; the last targets lie under no species."""
import os

import numpy as np
import pytest

from tests import k3_cases as K
from tests import refstats_reference as RR

pytestmark = pytest.mark.gpu

GUARD = 64
N_COLS = 600
CAP = 64        # K6_CAP
WG_CAP = 4096   # K3_WG_CAP
FINAL_N = 512
LENGTHS = [0, 1, 2, 4, 5, 63, 64, 65, WG_CAP, WG_CAP + 1]
TARGET = (np.arange(N_COLS) // 3).astype(np.uint32)
SPECIES = np.where(TARGET < 190, TARGET // 2 + 1, 0).astype(np.uint32)


class Tax:
    """the taxonomy behind SPECIES as the restatement asks for it: TaxId of target t = 1000 + t, of species s = s (0: the root)"""

    def resolve(self, t):
        return t

    def known(self, t):
        return True

    def species(self, t):
        return int(SPECIES[3 * (t - 1000)]) if t >= 1000 else t

    def lca(self, a, b):
        if a == b:
            return a
        return self.species(a) if self.species(a) == self.species(b) else 0

    def at_or_below_species(self, t):
        return self.species(t) != 0


TAXIDS = {f"t{t}": 1000 + t for t in range(N_COLS // 3)}


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = K.build_database(oracle_lib, tmp_path_factory.mktemp("k6db"), N_COLS, seed=902)
    with Database.open(d, device=0) as h:
        assert int(h.info.n_cols) == N_COLS
        h.set_profiling(1)
        yield h


def configure(db, species=True, H=0.75, slots=None, wgs=None):
    """the stage set anew (zeroed counters); the two environment knobs are read then"""
    for k, v in (("KMCPG_REFSTATS_SLOTS", slots), ("KMCPG_REFSTATS_WGS", wgs)):
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = str(v)
    try:
        db.set_refstats(TARGET, SPECIES if species else None, hic_min_qcov=H)
    finally:
        os.environ.pop("KMCPG_REFSTATS_SLOTS", None)
        os.environ.pop("KMCPG_REFSTATS_WGS", None)


# ---- segments: columns by pattern (K5's)
def seg_one(rng, m):
    return (3 * 11 + rng.integers(0, 3, size=m)).astype(np.uint32)


def seg_distinct(rng, m):
    return (3 * rng.permutation(200)[:m] + rng.integers(0, 3, size=m)).astype(np.uint32) if m <= 200 else rng.integers(0, N_COLS, size=m).astype(np.uint32)


def seg_aba(rng, m):
    """A B A ...: two targets of one species by turns, the chunk changing; from two pairs on"""
    return np.where(np.arange(m) % 2 == 0, 3 * 4 + np.arange(m) % 3, 3 * 5 + (np.arange(m) // 2) % 3).astype(np.uint32)


def seg_late(rng, m):
    """one target, and the first (and only) rows of three others in the last places"""
    s = np.full(m, 3 * 20, dtype=np.uint32)
    tail = min(3, max(m - 1, 0))
    if tail:
        s[m - tail:] = 3 * np.array([150, 151, 195])[:tail] + 2
    return s


PATTERNS = {"one": seg_one, "distinct": seg_distinct, "aba": seg_aba, "late": seg_late}


class Case:
    def __init__(self, segs, nk=None, counts=None, seed=1, final_n=FINAL_N):
        rng = np.random.default_rng(seed)
        lens = np.array([len(s) for s in segs], dtype=np.int64)
        self.n = len(segs)
        self.final_n = final_n
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        cols = np.concatenate(segs) if lens.sum() else np.zeros(0, dtype=np.uint32)
        self.nk = np.full(self.n, 130, dtype=np.int32) if nk is None else np.asarray(nk, dtype=np.int32)
        self.pairs = np.empty((len(cols), 2), dtype=np.uint32)
        self.pairs[:, 0] = cols
        self.pairs[:, 1] = rng.integers(1, np.repeat(self.nk, lens) + 1) if counts is None else counts


def classify(case, r):
    seg = case.pairs[int(case.offs[r]):int(case.offs[r + 1])]
    if len(seg) == 0:
        return "empty"
    if case.nk[r] > case.final_n or len(seg) > WG_CAP:
        return "left"
    if len(set(TARGET[seg[:, 0]].tolist())) == 1:
        return "single"
    return "wave" if len(seg) <= CAP else "left"


def reference(cases, species, H):
    """the restatement over the TSV the counted reads would print -> (counters [N_COLS, 4], matched, unique, classes per case)"""
    lines, classes = [], []
    for ci, case in enumerate(cases):
        cl = [classify(case, r) for r in range(case.n)]
        classes.append(cl)
        for r in range(case.n):
            if cl[r] in ("empty", "left"):
                continue
            for c, m in case.pairs[int(case.offs[r]):int(case.offs[r + 1])]:
                lines.append("\t".join([f"c{ci}r{r}", "150", str(case.nk[r]), "0", "1", f"t{TARGET[c]}", str(c % 3), "3", "30000", "21", str(m),
                                        "%.4f" % (int(m) / int(case.nk[r])), "0.01", "0.01", "0"]))
    prof, matched, unique = RR.stage1(["\n".join(lines)], max_fpr=1, min_qcov=0, hic_min_qcov=H, level="species" if species else "strain",
                                      taxid_map=TAXIDS, tax=Tax())
    want = np.zeros((N_COLS, 4), dtype=np.uint64)
    for name, t in prof.items():
        base = 3 * int(name[1:])
        for j, l in enumerate((t.rows, t.firsts, t.uniq, t.uniq_hic)):
            want[base:base + 3, j] = np.array(l, dtype=np.uint64)
    return want, matched, unique, classes


def launch(db, name, case, hits=None):
    """one kmcpg_refstats_device call; returns (LEFT bytes, witness, launches)"""
    import torch
    dev = torch.device("cuda", 0)
    n, cap = case.n, len(case.pairs)
    t_pairs = torch.from_numpy(case.pairs.view(np.int64).reshape(-1).copy()).to(dev)
    t_offs = torch.from_numpy(case.offs.view(np.int64).copy()).to(dev)
    t_nk = torch.from_numpy(case.nk).to(dev)
    t_left = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    t_hits = None if hits is None else torch.tensor([hits[0]], dtype=torch.int64, device=dev)
    db.refstats_device(t_pairs.data_ptr(), t_offs.data_ptr(), cap, t_nk.data_ptr(), n, case.final_n, t_left.data_ptr(),
                       d_n_hits=None if hits is None else t_hits.data_ptr(), hit_cap=0 if hits is None else hits[1])
    torch.cuda.synchronize()
    st, launches = db.last_refstats()
    assert np.array_equal(t_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), case.pairs), f"{name}: the pairs were changed"
    assert np.array_equal(t_offs.cpu().numpy().view(np.uint64), case.offs) and np.array_equal(t_nk.cpu().numpy(), case.nk), f"{name}: an input was changed"
    left = t_left.cpu().numpy()
    assert (left[n:] == 0x5A).all(), f"{name}: a byte behind the LEFT bytes was written"
    return left[:n], st, launches


def run(db, name, cases, species=True, H=0.75, **knobs):
    """the cases one after the other into freshly zeroed counters, against the restatement over all of them"""
    from kmcp_amd import lib
    configure(db, species=species, H=H, **knobs)
    want, matched, unique, classes = reference(cases, species, H)
    sts = []
    for case, cl in zip(cases, classes):
        left, st, launches = launch(db, name, case)
        assert left.tolist() == [int(c == "left") for c in cl], f"{name}: the LEFT bytes"
        assert {k: st[k] for k in ("empty", "single", "wave", "left")} == {k: cl.count(k) for k in ("empty", "single", "wave", "left")}, f"{name}: witness {st}"
        assert st["bad_segments"] == 0 and st["skipped"] == 0 and st["spilled_adds"] <= st["global_adds"]
        assert [(l.kernel, l.grid, l.block, l.cls) for l in launches] == ([(lib.K6_REFSTATS, st["grid"], 256, 3)] if case.n else []), name
        assert not case.n or 1 <= st["grid"] <= (case.n + 63) // 64
        sts.append(st)
    got, tot = db.refstats_read(N_COLS)
    g = got.view(np.uint64).reshape(N_COLS, 4)
    bad = np.argwhere(g != want)
    assert len(bad) == 0, f"{name}: column {bad[0][0]} counter {bad[0][1]}: {g[bad[0][0]]}, expected {want[bad[0][0]]}; {len(bad)} differ"
    assert tot == dict(matched_reads=matched, unique_reads=unique, host_reads=0, skipped_launches=0), f"{name}: totals {tot}, expected {matched} / {unique}"
    # every add went somewhere: to a table (and from there to global memory in at most as many adds) or straight to global memory
    total_adds = int(want.sum())
    assert sum(s["lds_adds"] + s["spilled_adds"] for s in sts) == total_adds, name
    return sts, classes, want


def mixed(n_reads, seed):
    rng = np.random.default_rng(seed)
    names = list(PATTERNS)
    segs, nk = [], []
    for r in range(n_reads):
        m = int(rng.choice(LENGTHS[:8] + [3, 7, 33])) if rng.random() < 0.8 else 0
        segs.append(PATTERNS[names[r % 4]](rng, m))
        nk.append(int(rng.choice([130, 130, 130, FINAL_N, FINAL_N + 1])))
    return Case(segs, nk=nk, seed=seed)


# ---- the cases ----
@pytest.mark.parametrize("species", [True, False], ids=["species", "strain"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_segment_lengths(db, pattern, species):
    rng = np.random.default_rng(3)
    _, classes, want = run(db, f"lengths, {pattern}", [Case([PATTERNS[pattern](rng, m) for m in LENGTHS])], species=species)
    if pattern == "one":
        assert classes[0] == ["empty"] + ["single"] * (len(LENGTHS) - 2) + ["left"]
        assert want[33:36, 0].sum() == sum(LENGTHS[:-1]) and want[33:36, 1].sum() == len(LENGTHS) - 2
    else:  # several targets from two pairs on: by the wave up to the cap, LEFT above it
        assert classes[0] == ["empty", "single"] + ["left" if m > CAP else "wave" for m in LENGTHS[2:]]
    if pattern == "aba":  # two targets of one species: unique at level species only
        assert (want[12:18, 2].sum() > 1) == species


# 16 reads = one wave: long segments (the whole wave reduces them — and counts the one-target ones — and hands the result back to the read's
# lane group: the first, the last and inner groups among them), several-target segments the wave counts, one-target segments of a lane
# group and empty reads, side by side
ONE_WAVE = [("aba", 65), ("aba", 40), ("one", 3), ("distinct", 65), ("late", 5), ("one", 0), ("aba", 64), ("one", 130),
            ("distinct", 2), ("late", 65), ("one", 1), ("one", 65), ("distinct", 63), ("one", 64), ("late", 4), ("one", 65)]


@pytest.mark.parametrize("species", [True, False], ids=["species", "strain"])
def test_long_wave_and_single_segments_in_one_wave_then_a_wave_of_one_read(db, species):
    """17 reads: the wave above, and the batch's last read alone in a second wave beside 15 lane groups without a read — long (LEFT,
    single), by the wave, single and empty in turn"""
    rng = np.random.default_rng(17)
    first = [PATTERNS[p](rng, m) for p, m in ONE_WAVE]
    want = ["left", "wave", "single", "left", "wave", "empty", "wave", "single", "wave", "left", "single", "single", "wave", "single", "wave", "single"]
    for (p, m), cls in ((("aba", 65), "left"), (("one", 65), "single"), (("aba", 40), "wave"), (("one", 3), "single"), (("one", 0), "empty")):
        case = Case(first + [PATTERNS[p](rng, m)])
        assert case.n == 17
        sts, classes, _ = run(db, f"one wave and a read, the last one {m} pairs of '{p}'", [case], species=species)
        assert classes[0] == want + [cls] and sts[0]["grid"] == 1


@pytest.mark.parametrize("n_reads", [1, 15, 16, 17, 63, 64, 65])
def test_read_counts(db, n_reads):
    run(db, f"{n_reads} reads", [mixed(n_reads, seed=n_reads)])


def test_a_second_grid_stride_round(db):
    sts, _, _ = run(db, "2 workgroups, 300 reads", [mixed(300, seed=77)], wgs=2)
    assert sts[0]["grid"] == 2  # 5 groups of 64 reads on 2 workgroups: three rounds for the first


def test_nk_at_the_bound_and_qcov_on_both_sides_of_H(db):
    rng = np.random.default_rng(5)
    one = np.array([3 * 7], dtype=np.uint32)
    # (nk, count): 75 / 100 is H itself; 7499 / 10000 one printed digit below; 15000 / 20001 = 0.74996... prints as 0.7500 and passes
    hs = [(100, 75), (10000, 7499), (20001, 15000), (20001, 14999), (130, 130), (130, 1)]
    case = Case([one] * len(hs), nk=[h[0] for h in hs], counts=np.array([h[1] for h in hs], dtype=np.uint32), final_n=20001)
    _, _, want = run(db, "H", [case])
    assert want[21].tolist() == [6, 6, 6, 3]
    segs = [seg_one(rng, 3), seg_one(rng, 3), seg_aba(rng, 6), seg_aba(rng, 6)]
    _, classes, _ = run(db, "final_n", [Case(segs, nk=[FINAL_N, FINAL_N + 1, FINAL_N, FINAL_N + 1])])
    assert classes[0] == ["single", "left", "wave", "left"]


def test_every_read_on_one_column_adds_per_workgroup_not_per_read(db):
    n = 4096
    case = Case([np.array([3 * 50 + 1], dtype=np.uint32)] * n, counts=np.full(n, 120, dtype=np.uint32))
    sts, _, want = run(db, "one column", [case])
    assert want[151].tolist() == [n, n, n, n] and want.sum() == 4 * n
    st = sts[0]
    assert st["spilled_adds"] == 0 and st["lds_adds"] == 4 * n
    assert 0 < st["global_adds"] <= 4 * st["grid"], st


def test_a_table_too_small_spills_and_counts_the_same(db):
    rng = np.random.default_rng(9)
    cases = [Case([seg_distinct(rng, 60) for _ in range(40)] + [seg_one(rng, 9)], seed=9)]
    sts, _, _ = run(db, "2 slots", cases, slots=2)
    assert sts[0]["slots"] == 2 and sts[0]["spilled_adds"] > 0 and sts[0]["lds_adds"] > 0
    sts, _, _ = run(db, "no table", cases, slots=0)
    assert sts[0]["slots"] == 0 and sts[0]["lds_adds"] == 0 and sts[0]["spilled_adds"] == sts[0]["global_adds"] > 0
    sts, _, _ = run(db, "default table", cases)
    assert sts[0]["slots"] == 1024 and sts[0]["spilled_adds"] == 0


def test_two_calls_accumulate_reset_zeroes_and_the_overflow_guard_skips(db):
    a, b = mixed(100, seed=21), mixed(37, seed=22)
    run(db, "two calls", [a, b])
    before, tot = db.refstats_read(N_COLS)
    assert tot["matched_reads"] > 0 and before.view(np.uint64).any()
    # a hit counter above the capacity: the batch will be run again, nothing is counted now
    _, st, _ = launch(db, "guard", a, hits=(1001, 1000))
    assert st["skipped"] == 1 and not any(st[k] for k in ("empty", "single", "wave", "left", "lds_adds", "global_adds"))
    after, tot2 = db.refstats_read(N_COLS)
    assert after.tobytes() == before.tobytes() and tot2 == dict(tot, skipped_launches=1)  # ... and the handle remembers that it skipped one
    # at the capacity it runs
    _, st, _ = launch(db, "guard", a, hits=(1000, 1000))
    assert st["skipped"] == 0 and st["lds_adds"] > 0
    db.refstats_reset()
    zero, tot3 = db.refstats_read(N_COLS)
    assert not zero.view(np.uint64).any() and tot3 == dict(matched_reads=0, unique_reads=0, host_reads=0, skipped_launches=0)


def test_the_stage_off(db):
    import torch

    from kmcp_amd.lib import KmcpGpuError
    z = torch.zeros(8, dtype=torch.int64, device=torch.device("cuda", 0))
    db.set_refstats()
    st, launches = db.last_refstats()
    assert launches == [] and not any(st.values())
    with pytest.raises(KmcpGpuError, match="stage is off"):
        db.refstats_device(z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), 1, FINAL_N, z.data_ptr())
