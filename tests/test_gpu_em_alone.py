"""K9 alone (kmcp_amd/csrc/k9_em.hip): the read log is filled through kmcpg_recount_log_device on pair lists the test lays out (the helpers
of tests/test_gpu_recount_alone.py are imported, the file is not touched), then kmcpg_em_pass / kmcpg_em_read are compared with our rule in
Python integers (tests/em_reference.py) over the reads of every class — all six words of every column for EXACT equality, the totals
and the witness — and the conservation law (every assigned read adds exactly EM_UNIT to match) is asserted on every case.  The two halves
of a pass (the device log and the host log) are compared on a small database searched through the whole pipeline.

The table: three columns per target (its chunks); species: four targets per species, species 0 (none) for the targets from 160 on."""
import os

import numpy as np
import pytest

from tests import em_reference as E
from tests import synth
from tests import test_gpu_recount_alone as R8

pytestmark = pytest.mark.gpu

N_COLS, N_CLASSES, H = R8.N_COLS, R8.N_CLASSES, R8.H
TARGET, SPECIES = R8.TARGET, R8.SPECIES
Case, seg = R8.Case, R8.seg
U = E.EM_UNIT
WORDS = ("match", "uniq", "hic", "single_bases", "bases_lo", "bases_hi")


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = R8.K.build_database(oracle_lib, tmp_path_factory.mktemp("k9db"), N_COLS, seed=905)
    with Database.open(d, device=0) as h:
        assert int(h.info.n_cols) == N_COLS
        h.set_profiling(1)
        yield h


def configure(db, species=True, max_wgs=None, log_bytes=1 << 20):
    """the recount stage set anew (zeroed counters, an empty log); KMCPG_RECOUNT_WGS — the grid's bound, K9's too — is read then"""
    for k in R8.KNOBS + ("KMCPG_EM_SLOTS",):
        os.environ.pop(k, None)
    if max_wgs is not None:
        os.environ["KMCPG_RECOUNT_WGS"] = str(max_wgs)
    try:
        db.set_recount(TARGET, SPECIES if species else None, hic_min_qcov=H, log_bytes=log_bytes)
    finally:
        os.environ.pop("KMCPG_RECOUNT_WGS", None)


def classes_of(est=None, cov=None):
    from kmcp_amd import lib
    c = np.zeros(N_CLASSES, dtype=lib.EM_CLASS_DTYPE)
    c["est"] = 1 if est is None else est
    c["coverage"] = 1.0 if cov is None else cov
    return c


def em(db, classes, level_species=True, slots=None):
    """one kmcpg_em_pass + kmcpg_em_read + kmcpg_last_em"""
    if slots is not None:
        os.environ["KMCPG_EM_SLOTS"] = str(slots)
    try:
        db.em_pass(classes, level_species=level_species)
    finally:
        os.environ.pop("KMCPG_EM_SLOTS", None)
    got, tot = db.em_read()
    st, launches = db.last_em()
    return got, tot, st, launches


def check(db, name, counted, classes, level_species=True, species=True, slots=None):
    """a pass against the Python rule over `counted` = [(case, reads with LEFT byte 0)]; returns (columns, totals, witness)"""
    from kmcp_amd import lib
    got, tot, st, launches = em(db, classes, level_species, slots)
    reads = [(int(case.nk[r]), int(case.qlen[r]), case.rows(r)) for case, rs in counted for r in rs]
    want, wt = E.em_cols(reads, N_COLS, TARGET, SPECIES if species else None, classes["est"], classes["coverage"], H, level_species)
    g = [[int(row[w]) for w in WORDS] for row in got]
    bad = [c for c in range(N_COLS) if g[c] != want[c]]
    assert not bad, f"{name}: column {bad[0]}: {g[bad[0]]}, expected {want[bad[0]]} ({len(bad)} columns differ)"
    assert {k: tot[k] for k in wt} == wt and tot["host_reads"] == 0, f"{name}: totals {tot}, expected {wt}"
    assert int(got["match"].sum()) == tot["assigned_reads"] * U, f"{name}: the conservation law"
    # the witness: the logged reads by the number of their estimated targets
    logged = [(case, r) for case, rs in counted for r in rs if case.classify(r) == "logged"]
    nts = [len({int(TARGET[c]) for c, _ in case.rows(r) if classes["est"][TARGET[c]]}) for case, r in logged]
    assert (st["reads"], st["none"], st["one"], st["split"]) == (len(logged), nts.count(0), nts.count(1), sum(1 for x in nts if x > 1)), f"{name}: witness {st}"
    assert [(l.kernel, l.grid, l.block, l.cls) for l in launches] == ([(lib.K9_EM, st["grid"], 256, 3)] if logged else []), name
    assert (st["grid"] == 0) == (not logged) and st["grid"] <= (len(logged) + 63) // 64
    return got, tot, st


def run(db, name, case, classes=None, level_species=True, species=True, slots=None, max_wgs=None):
    """one case into a freshly set stage, logged, passed over, against the Python rule"""
    configure(db, species=species, max_wgs=max_wgs)
    left, _, _ = R8.launch(db, name, case)
    counted = [r for r in range(case.n) if not left[r] and case.classify(r) != "empty"]
    return check(db, name, [(case, counted)], classes_of() if classes is None else classes, level_species, species, slots) + (counted,)


def mixed_classes(seed):
    """a whitelist with holes and coverages over twelve orders of magnitude"""
    rng = np.random.default_rng(seed)
    return classes_of(est=(rng.random(N_CLASSES) < 0.8).astype(np.uint32), cov=rng.choice([1e-9, 1e-3, 0.25, 1.0, 3.0, 17.25, 1e6], size=N_CLASSES) * rng.uniform(0.5, 2.0, size=N_CLASSES))


# ---- read counts and grid ----
def test_no_reads(db):
    got, tot, st, _ = run(db, "0 reads", Case([]))
    assert st["grid"] == 0 and not got.view(np.uint64).any() and tot["assigned_reads"] == 0
    got, tot, st, _ = run(db, "one empty read", Case([np.zeros((0, 2), dtype=np.uint32)]))
    assert st["reads"] == 0 and not got.view(np.uint64).any()


@pytest.mark.parametrize("n", [1, 16, 17, 65])
def test_read_counts_at_the_wave_and_workgroup_edges(db, n):
    """exactly n logged reads, between reads of one target and empty ones"""
    rng = np.random.default_rng(n)
    segs = []
    for _ in range(n):
        segs += [seg(rng.permutation(40)[:3], counts=rng.choice([90, 100, 130], size=3)), seg([int(rng.integers(0, 200))] * 2), np.zeros((0, 2), dtype=np.uint32)]
    _, tot, st, _ = run(db, f"{n} logged", Case(segs), mixed_classes(n))
    assert st["reads"] == n and st["grid"] == (n + 63) // 64 and tot["assigned_reads"] > 0


def test_1000_reads_on_one_workgroup_take_grid_stride_rounds(db):
    case = R8.mixed(1000, seed=77)
    classes = mixed_classes(77)
    got, tot, st, _ = run(db, "1 workgroup", case, classes, max_wgs=1)
    assert st["grid"] == 1 and st["reads"] > 400 and st["none"] > 0 and st["one"] > 0 and st["split"] > 100
    got2, tot2, st2, _ = run(db, "all workgroups", case, classes)
    assert st2["grid"] > 1 and got2.tobytes() == got.tobytes() and tot2 == tot  # the same inputs, another grid: the same counters


# ---- targets ----
def test_two_targets_64_distinct_targets_and_aba(db):
    rng = np.random.default_rng(1)
    c = classes_of()
    c["coverage"][3], c["coverage"][7] = 3.0, 1.0
    got, tot, _, _ = run(db, "two", Case([seg([7, 3])], qlen=[150]), c)
    assert tot["split_reads"] == 1 and int(got["match"][3 * 7]) == U // 4 and int(got["match"][3 * 3 + 1]) == U - U // 4
    got, tot, st, _ = run(db, "64 distinct", Case([seg(rng.permutation(40).tolist() + list(range(100, 124)), counts=rng.integers(60, 131, size=64))]), mixed_classes(2))
    assert st["split"] == 1 and int((got["match"] > 0).sum()) > 30
    # A B A ...: 32 rows each; p = EM_UNIT / 2 is a multiple of 32, a p that is not follows below
    got, _, _, _ = run(db, "aba", Case([seg([4, 5] * 32, counts=rng.integers(60, 131, size=64))]))
    assert int(got["match"].sum()) == U and int(got["match"][3 * 4:3 * 4 + 3].sum()) == U // 2


def test_no_estimated_target_and_one_among_several(db):
    c = classes_of(est=0)
    got, tot, st, _ = run(db, "none", Case([seg([4, 5, 6])]), c)
    assert st["none"] == 1 and tot["assigned_reads"] == 0 and not got.view(np.uint64).any()
    # one estimated target among several: the unique rule, with qCov on both sides of H (97 / 130 prints 0.7462, 98 / 130 0.7538)
    c["est"][5], c["coverage"][5] = 1, 2.0
    for count, hic in ((97, 0), (98, U)):
        got, tot, st, _ = run(db, f"one of three, {count}", Case([seg([4, 5, 6, 5], counts=[120, count, 120, 110], chunks=[0, 1, 2, 2])], qlen=[151]), c)
        assert st["one"] == 1 and tot["unique_reads"] == 1 and tot["split_reads"] == 0
        assert int(got["match"][16]) == U // 2 == int(got["match"][17]) and int(got["uniq"][16]) == U and int(got["hic"][16]) == hic and int(got["uniq"][17]) == 0
        assert (int(got["bases_hi"][16]) << 32) + int(got["bases_lo"][16]) == 151 * (U // 2) and int(got["single_bases"].sum()) == 0


# ---- shares ----
def test_shares_that_do_not_divide_tiny_coverages_and_the_high_bases_word(db):
    # coverages 1, 1, 15: the quotas are floor(U / 17), floor(U / 17), floor(15 U / 17) and leave a deficit for the first target; the second
    # target has seven rows, which do not divide its quota
    c = classes_of()
    c["coverage"][20], c["coverage"][21], c["coverage"][22] = 1.0, 1.0, 15.0
    got, tot, _, _ = run(db, "m does not divide p", Case([seg([20, 21, 21, 21, 21, 21, 21, 21, 22], chunks=[0, 0, 1, 2, 0, 1, 2, 0, 0])], qlen=[100]), c)
    q = E.quota(1.0, 17.0)
    assert q % 7 != 0 and U - 2 * q - E.quota(15.0, 17.0) > 0, "the case must have a remainder in a target and a deficit"
    assert int(got["match"][3 * 21:3 * 21 + 3].sum()) == q and int(got["match"][3 * 20]) == U - q - E.quota(15.0, 17.0)
    # 1e-9 beside 1e6: the small share is 0, and the deficit goes to the first target — the small one here
    c = classes_of()
    c["coverage"][30], c["coverage"][31] = 1e-9, 1e6
    got, _, _, _ = run(db, "tiny first", Case([seg([30, 31])]), c)
    big = E.quota(1e6, 1e-9 + 1e6)
    assert E.quota(1e-9, 1e-9 + 1e6) == 0 and int(got["match"][90]) == U - big and int(got["match"][94]) == big
    got, _, _, _ = run(db, "tiny second", Case([seg([31, 30])]), c)
    assert int(got["match"][93]) == U and int(got["match"][91]) == 0 and int(got["bases_lo"][91]) == 0
    # qlen 2^31 - 1 reaches the high bases word, in a split read and in a unique one
    got, _, _, _ = run(db, "long", Case([seg([4, 5]), seg([4, 170])], qlen=[2**31 - 1, 2**31 - 1]), classes_of(est=(np.arange(N_CLASSES) < 160).astype(np.uint32)))
    assert int(got["bases_hi"][12]) > 2**29
    total = sum((int(r["bases_hi"]) << 32) + int(r["bases_lo"]) for r in got)
    assert total == 2 * (2**31 - 1) * U


# ---- species and level ----
def test_one_species_against_two_and_strain_level(db):
    # targets 8, 9 (species 3), 12 (species 4), 170 (none)
    same, diff, none = Case([seg([8, 9, 8], counts=[110, 100, 90])]), Case([seg([8, 12])]), Case([seg([170, 171])])
    c = classes_of()
    c["coverage"][8], c["coverage"][9] = 1.0, 3.0
    got, tot, _, _ = run(db, "one species", same, c)
    # 8 has two rows of p = U / 4: its first row adds U / 8 to uniq and hic, 9's row 3 U / 4 (110 / 130 and 100 / 130 are both above H)
    assert tot["split_reads"] == 1 and int(got["uniq"].sum()) == U // 8 + 3 * (U // 4) and int(got["hic"].sum()) == int(got["uniq"].sum())
    for name, case, kw in (("two species", diff, {}), ("species 0", none, {}), ("level strain", same, dict(level_species=False)), ("no table", same, dict(species=False))):
        got, _, _, _ = run(db, name, case, c, **kw)
        assert int(got["uniq"].sum()) == 0 and int(got["match"].sum()) == U


# ---- contention ----
def test_a_hot_column_adds_per_workgroup_not_per_read(db):
    n = 1000
    c = classes_of()
    c["est"][51] = 0  # every read ends on column 150 alone, by the unique rule: match, uniq, hic and both bases words
    case = Case([seg([50, 51])] * n, qlen=[150] * n)
    got, tot, st, _ = run(db, "hot column", case, c, slots=1024)
    assert int(got["match"][150]) == n * U and tot["unique_reads"] == n
    assert st["slots"] == 1024 and st["lds_adds"] == 5 * n and st["spilled_adds"] == 0 and 0 < st["global_adds"] <= 5 * st["grid"], st
    got0, _, st, _ = run(db, "no LDS table", case, c, slots=0)
    assert st["slots"] == 0 and st["lds_adds"] == 0 and st["global_adds"] == st["spilled_adds"] == 5 * n and got0.tobytes() == got.tobytes()


def test_a_2_slot_lds_table_spills_and_counts_the_same(db):
    case = R8.mixed(200, seed=9)
    classes = mixed_classes(9)
    got, tot, st, _ = run(db, "2 slots", case, classes, slots=2)
    assert st["slots"] == 2 and st["spilled_adds"] > 0 and st["lds_adds"] > 0
    got0, tot0, st0, _ = run(db, "1024 slots", case, classes, slots=1024)
    assert st0["spilled_adds"] == 0 and got0.tobytes() == got.tobytes() and tot0 == tot
    got1, tot1, _, _ = run(db, "the default", case, classes)
    assert got1.tobytes() == got.tobytes() and tot1 == tot


# ---- repeatability ----
def test_passes_repeat_other_classes_need_no_new_search_and_the_recount_is_untouched(db):
    from kmcp_amd import lib
    case = R8.mixed(300, seed=5)
    rc, shared = R8.mixed_inputs(6)
    configure(db)
    left, _, _ = R8.launch(db, "log", case)
    counted = [(case, [r for r in range(case.n) if not left[r] and case.classify(r) != "empty"])]
    db.recount_run(rc, R8.pairs_of(shared))
    before, tot_before = db.recount_read()
    a, ta, _ = check(db, "first", counted, mixed_classes(1))
    b, tb, _ = check(db, "second", counted, mixed_classes(1))
    assert a.tobytes() == b.tobytes() and ta == tb and ta["split_reads"] > 50
    c, tc, _ = check(db, "other classes", counted, mixed_classes(2))
    d, td, _ = check(db, "strain level", counted, mixed_classes(1), level_species=False)
    assert len({a.tobytes(), c.tobytes(), d.tobytes()}) == 3
    e, te, _ = check(db, "the first again", counted, mixed_classes(1))
    assert e.tobytes() == a.tobytes() and te == ta
    # the recount's read-out is what it was before the passes, and a new replay gives it again
    after, tot_after = db.recount_read()
    assert after.tobytes() == before.tobytes() and tot_after == tot_before
    db.recount_run(rc, R8.pairs_of(shared))
    again, tot_again = db.recount_read()
    assert again.tobytes() == before.tobytes() and tot_again == tot_before
    f, tf, _ = check(db, "after a replay", counted, mixed_classes(1))
    assert f.tobytes() == a.tobytes()
    assert lib.EM_UNIT == U


# ---- the halves of a pass: the whole pipeline on a small database ----
def test_the_host_half_counts_what_the_device_counts(oracle_lib, tmp_path):
    """six close relatives and two unrelated genomes in two chunks each: most reads hit several of the relatives, the reads of the unrelated
    ones have one target (K8's single rule: on the device route they are counted at once, on the host route by the pass).  The same search with the default log, with a log of 256
    bytes (most multi-target reads are LEFT for want of room and go through the host half) and with KMCPG_RECOUNT_DEVICE=0 (every read
    does) gives the same bytes, and they are the Python rule's over the search's own result"""
    from kmcp_amd import Database, default_params
    rng = np.random.default_rng(92)
    base = synth.random_genomes(1, 6000, seed=93)[0]
    genomes = []
    for i in range(6):
        g = np.frombuffer(base, dtype=np.uint8).copy()
        m = rng.random(len(g)) < 0.01
        g[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(m.sum()))
        genomes.append(g.tobytes())
    genomes += synth.random_genomes(2, 6000, seed=94)
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=2, overlap=150, threads=1)
    reads = synth.sample_reads(genomes, 300, 150, sub_rate=0.0, seed=201, frac_random=0.1)
    p = default_params()
    with Database.open(db_dir, device=0) as h:
        n = int(h.info.n_cols)
        names = [h.col_info(c)[0] for c in range(n)]
        ids = {}
        target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
        species = (target // 3 + 1).astype(np.uint32)
        from kmcp_amd import lib
        classes = np.zeros(len(ids), dtype=lib.EM_CLASS_DTYPE)
        assert len(ids) == 8
        classes["est"], classes["coverage"] = [1, 1, 0, 1, 1, 1, 1, 0], [0.5, 2.0, 1.0, 1e-3, 7.0, 1.0, 1.0, 1.0]
        h.set_recount(target, species, hic_min_qcov=0.9)
        res = h.search_pairs(reads, params=p)
        rows = [(int(res.qkmers[i]), int(res.qlen[i]), [(int(c), int(k)) for c, k in res.read(i).tolist()]) for i in range(len(reads)) if len(res.read(i))]
        want, wt = E.em_cols(rows, n, target, species, classes["est"], classes["coverage"], 0.9, True)
        assert wt["split_reads"] > 100 and wt["unique_reads"] > 10 and wt["assigned_reads"] < len(rows)
        h.em_pass(classes)
        dev, tot = h.em_read()
        assert [[int(r[w]) for w in WORDS] for r in dev] == want and {k: tot[k] for k in wt} == wt and tot["host_reads"] == 0
        assert int(dev["match"].sum()) == tot["assigned_reads"] * U
        st, _ = h.last_em()
        assert st["split"] == wt["split_reads"] and st["reads"] > 0
        # a log of 256 bytes
        h.set_recount(target, species, hic_min_qcov=0.9, log_bytes=256)
        h.search_pairs(reads, params=p)
        h.em_pass(classes)
        small, tot_small = h.em_read()
        rc = np.zeros(len(ids), dtype=lib.RECOUNT_CLASS_DTYPE)
        rc["kept"] = 1
        h.recount_run(rc, np.zeros(0, dtype=lib.COOCCUR_DTYPE))
        assert h.recount_read()[1]["left_full"] > 50
        assert small.tobytes() == dev.tobytes() and tot_small["host_reads"] > 50 and {k: tot_small[k] for k in wt} == wt
        # every read to the host half
        os.environ["KMCPG_RECOUNT_DEVICE"] = "0"
        try:
            h.set_recount(target, species, hic_min_qcov=0.9)
            h.search_pairs(reads, params=p)
        finally:
            os.environ.pop("KMCPG_RECOUNT_DEVICE")
        h.em_pass(classes)
        host, tot_host = h.em_read()
        assert host.tobytes() == dev.tobytes() and tot_host["host_reads"] == tot_host["assigned_reads"] == wt["assigned_reads"] and {k: tot_host[k] for k in wt} == wt
        assert h.last_em()[0]["reads"] == 0
        h.set_recount()
