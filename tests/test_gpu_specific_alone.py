"""K4 alone (kmcp_amd/csrc/k4_specific.hip: k4_verdict, the scan of k3_finalize.hip, k4_compact), driven through
kmcpg_specific_device on pair lists the test lays out and held against plain numpy, bit for bit: the verdict bytes, the new offsets,
the compacted pairs, every word behind the outputs (guard words, and the part of the pair buffer nothing is copied to), the inputs
(unchanged) and the witness — counters equal to numpy's, launches as the launcher makes them.

The tables: three columns per target (its chunks), four targets per species, every seventh target under no species (class 0)."""
import numpy as np
import pytest

from tests import k3_cases as K

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = -0x0123456789ABCDEF
BYTE_SENTINEL = 0xA5
N_COLS = 600
FINAL_N = 512
DROP, KEEP, HOST = 0, 1, 2
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 511, 512, 513, 4096, 4097, 10000]


def tables():
    target = (np.arange(N_COLS) // 3).astype(np.uint32)
    species = np.where(target % 7 == 0, 0, 1000 + target // 4).astype(np.uint32)
    return target, species


TARGET, SPECIES = tables()


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = K.build_database(oracle_lib, tmp_path_factory.mktemp("k4db"), N_COLS, seed=900)
    with Database.open(d, device=0) as h:
        assert int(h.info.n_cols) == N_COLS
        h.set_profiling(1)
        yield h


# ---- segments ----
def cols_of_target(t):
    return np.arange(3 * t, 3 * t + 3)


def targets_of_species(s):
    return [t for t in range(N_COLS // 3) if SPECIES[3 * t] == s]


def segment(rng, m, kind):
    """m columns: 'one' target, several targets of one 'species', 'two' species, one target under 'no-species', 'two-no-species' targets"""
    if m == 0:
        return np.zeros(0, dtype=np.uint32)
    if kind == "one":
        pool = cols_of_target(int(rng.integers(1, 7)))
    elif kind == "no-species":
        pool = cols_of_target(7 * int(rng.integers(0, 5)))
    elif kind == "species":
        ts = targets_of_species(1000 + int(rng.integers(1, 20)))
        pool = np.concatenate([cols_of_target(t) for t in ts])
    elif kind == "two":
        pool = np.concatenate([cols_of_target(9), cols_of_target(30)])
    else:
        assert kind == "two-no-species"
        pool = np.concatenate([cols_of_target(7), cols_of_target(14)])
    seg = pool[rng.integers(0, len(pool), size=m)]
    if kind in ("species", "two", "two-no-species") and m >= 2:  # really more than one target
        seg[0], seg[-1] = pool[0], pool[-1]
    return seg.astype(np.uint32)


class Case:
    def __init__(self, segs, nk=None, seed=1):
        rng = np.random.default_rng(seed)
        lens = np.array([len(s) for s in segs], dtype=np.int64)
        self.n = len(segs)
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        cols = np.concatenate(segs) if len(segs) and lens.sum() else np.zeros(0, dtype=np.uint32)
        self.pairs = np.empty((len(cols), 2), dtype=np.uint32)
        self.pairs[:, 0] = cols
        self.pairs[:, 1] = rng.integers(1, 200, size=len(cols))
        self.nk = np.full(self.n, 130, dtype=np.int32) if nk is None else np.asarray(nk, dtype=np.int32)


def reference(case, level_species, final_n=FINAL_N):
    """verdicts, new offsets, compacted pairs, the witness's counters — one read at a time where reads have pairs, in numpy"""
    lens = np.diff(case.offs.astype(np.int64))
    verdict = np.full(case.n, KEEP, dtype=np.uint8)
    cols = case.pairs[:, 0]
    st = dict(kept=0, dropped=0, host=0, group_segments=0, wave_segments=0, bad_segments=0)
    for r in np.flatnonzero(lens):
        seg = cols[int(case.offs[r]):int(case.offs[r + 1])]
        if case.nk[r] > final_n:
            verdict[r] = HOST
            st["host"] += 1
            continue
        t, s = TARGET[seg], SPECIES[seg]
        keep = t.min() == t.max() or (level_species and s.min() == s.max() and s.min() != 0)
        verdict[r] = KEEP if keep else DROP
        st["kept" if keep else "dropped"] += 1
        st["group_segments" if len(seg) <= 64 else "wave_segments"] += 1
    kept_len = np.where(verdict == DROP, 0, lens)
    out_offs = np.concatenate([[0], np.cumsum(kept_len)]).astype(np.uint64)
    mask = np.repeat(verdict != DROP, lens)
    st["pairs_in"], st["pairs_out"] = int(case.offs[-1]), int(out_offs[-1])
    return verdict, out_offs, case.pairs[mask], st


def run(db, name, case, level_species=True, final_n=FINAL_N, ref=None, profiled=True):
    import torch

    from kmcp_amd import lib
    dev = torch.device("cuda", 0)
    db.set_specific(TARGET, SPECIES if level_species else None)
    if ref is None:
        ref = reference(case, level_species, final_n)
    verdict, out_offs, out_pairs, st = ref
    n, cap = case.n, len(case.pairs)
    t_pairs = torch.from_numpy(case.pairs.view(np.int64).reshape(-1).copy()).to(dev)
    t_offs = torch.from_numpy(case.offs.view(np.int64).copy()).to(dev)
    t_nk = torch.from_numpy(case.nk).to(dev)
    t_out = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    t_oo = torch.full((n + 1 + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    t_v = torch.full((n + GUARD,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    db.specific_device(t_pairs.data_ptr(), t_offs.data_ptr(), cap, t_nk.data_ptr(), n, final_n, t_out.data_ptr(), cap, t_oo.data_ptr(), t_v.data_ptr())
    torch.cuda.synchronize()
    got_st, launches = db.last_specific()
    assert np.array_equal(t_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), case.pairs), f"{name}: the pairs were changed"
    assert np.array_equal(t_offs.cpu().numpy().view(np.uint64), case.offs) and np.array_equal(t_nk.cpu().numpy(), case.nk), f"{name}: an input was changed"
    want_v = np.concatenate([verdict, np.full(GUARD, BYTE_SENTINEL, dtype=np.uint8)])
    got_v = t_v.cpu().numpy()
    bad = np.flatnonzero(got_v != want_v)
    assert len(bad) == 0, f"{name}: verdict of read {bad[0]} (of {n}) is {got_v[bad[0]]}, expected {want_v[bad[0]]}; {len(bad)} differ"
    want_oo = np.concatenate([out_offs.view(np.int64), np.full(GUARD, SENTINEL, dtype=np.int64)])
    got_oo = t_oo.cpu().numpy()
    bad = np.flatnonzero(got_oo != want_oo)
    assert len(bad) == 0, f"{name}: out_offs[{bad[0]}] is {got_oo[bad[0]]}, expected {want_oo[bad[0]]}; {len(bad)} differ"
    want_out = np.full(cap + GUARD, SENTINEL, dtype=np.int64)
    want_out[:len(out_pairs)] = np.ascontiguousarray(out_pairs).view(np.int64).reshape(-1)
    got_out = t_out.cpu().numpy()
    bad = np.flatnonzero(got_out != want_out)
    assert len(bad) == 0, f"{name}: out_pairs[{bad[0]}] is {got_out[bad[0]]:#x}, expected {want_out[bad[0]]:#x}; {len(bad)} differ (kept pairs: {len(out_pairs)} of {cap})"
    assert got_st == st, f"{name}: witness {got_st}, expected {st}"
    waves = (n + 63) // 64
    tiles = (n + 1 + 4095) // 4096
    want_l = [(lib.K4_VERDICT, waves, 256, 3), (lib.K4_SCAN_TILES, tiles, 256, 0), (lib.K4_SCAN_SUMS, 1, 256, 0), (lib.K4_SCAN_ADD, tiles, 256, 0),
              (lib.K4_COMPACT, waves, 256, 3)] if n and profiled else []
    assert [(l.kernel, l.grid, l.block, l.cls) for l in launches] == want_l, name
    return ref


# ---- the cases ----
@pytest.mark.parametrize("level", ["species", "strain"])
def test_segment_lengths(db, level):
    rng = np.random.default_rng(11)
    segs = []
    for kind in ("one", "species", "two", "no-species", "two-no-species"):
        segs += [segment(rng, m, kind) for m in EDGE_LENGTHS]
    case = Case(segs)
    verdict = run(db, f"segment lengths, {level}", case, level == "species")[0]
    per = len(EDGE_LENGTHS)
    long_enough = np.array(EDGE_LENGTHS) >= 2
    assert (verdict[:per] == KEEP).all() and (verdict[3 * per:4 * per] == KEEP).all()  # one target, with or without a species
    assert (verdict[per:2 * per][long_enough] == (KEEP if level == "species" else DROP)).all()  # equal species, unequal targets
    assert (verdict[2 * per:3 * per][long_enough] == DROP).all() and (verdict[4 * per:][long_enough] == DROP).all()  # two species; species 0 twice


@pytest.mark.parametrize("m", [2, 3, 4, 5, 64, 65, 130])
def test_the_one_differing_pair_at_every_position(db, m):
    """m reads of m pairs of one species, the pair of another species at position i in read i — a lane, a loop trip or a butterfly
    step that a reduction drops shows as KEEP; and the same with a second TARGET of the same species (strain level drops it)"""
    rng = np.random.default_rng(m)
    ts = targets_of_species(1003)
    for other, level_species, want in ((cols_of_target(40)[1], True, DROP), (cols_of_target(ts[1])[2], False, DROP), (cols_of_target(ts[1])[2], True, KEEP)):
        segs = []
        for i in range(m):
            seg = cols_of_target(ts[0])[rng.integers(0, 3, size=m)].astype(np.uint32)
            seg[i] = other
            segs.append(seg)
        segs.append(cols_of_target(ts[0])[rng.integers(0, 3, size=m)].astype(np.uint32))  # and none: KEEP
        verdict = run(db, f"differing pair, {m} pairs, other column {other}, species level {level_species}", Case(segs), level_species)[0]
        assert (verdict[:m] == want).all() and verdict[m] == KEEP


def test_species_zero_and_levels(db):
    one_no_species = np.array([21, 22, 23, 21], dtype=np.uint32)          # target 7: species 0, one target
    two_no_species = np.array([21, 42], dtype=np.uint32)                  # targets 7 and 14: species 0 both
    ts = targets_of_species(1002)
    same_species = np.array([3 * ts[0], 3 * ts[1] + 1], dtype=np.uint32)  # equal species, unequal targets
    zero_and_some = np.array([21, 3 * ts[0]], dtype=np.uint32)            # species 0 beside a species
    case = Case([one_no_species, two_no_species, same_species, zero_and_some])
    assert list(run(db, "species 0, species level", case, True)[0]) == [KEEP, DROP, KEEP, DROP]
    assert list(run(db, "species 0, strain level", case, False)[0]) == [KEEP, DROP, DROP, DROP]


def test_queries_above_final_n_are_left_to_the_host(db):
    rng = np.random.default_rng(5)
    segs, nk = [], []
    for kind in ("one", "two", "species"):
        for m in (0, 1, 5, 64, 65, 700):
            for q in (FINAL_N - 1, FINAL_N, FINAL_N + 1, 20000):
                segs.append(segment(rng, m, kind))
                nk.append(q)
    case = Case(segs, nk=nk)
    verdict, out_offs, _, st = run(db, "final_n", case)
    lens = np.diff(case.offs.astype(np.int64))
    above = (np.array(nk) > FINAL_N) & (lens > 0)
    assert (verdict[above] == HOST).all() and not (verdict[~above] == HOST).any() and st["host"] == above.sum()
    assert (np.diff(out_offs.astype(np.int64))[above] == lens[above]).all()  # they keep all their pairs
    other = run(db, "final_n = 1024", case, final_n=1024)[0]
    assert (other[np.array(nk) == 20000][lens[np.array(nk) == 20000] > 0] == HOST).all() and (other[np.array(nk) <= 1024] != HOST).all()


def mostly_short(n_reads, seed, fill=0.4):
    rng = np.random.default_rng(seed)
    kinds = ("one", "species", "two", "no-species", "two-no-species")
    segs = []
    for r in range(n_reads):
        m = 0 if rng.random() > fill else int(rng.choice([1, 2, 3, 7, 33, 64, 65, 90]))
        segs.append(segment(rng, m, kinds[r % 5]))
    return Case(segs, seed=seed)


@pytest.mark.parametrize("n_reads", [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097])
def test_read_counts(db, n_reads):
    case = mostly_short(n_reads, seed=n_reads, fill=0.7)
    run(db, f"{n_reads} reads", case)
    if n_reads in (1, 17):  # the last read has pairs, and then has none
        run(db, f"{n_reads} reads, the last one long", Case([segment(np.random.default_rng(3), 200, "two")] * n_reads))
        run(db, f"{n_reads} reads, all empty", Case([np.zeros(0, dtype=np.uint32)] * n_reads))


# 16 reads = one wave: long segments (the whole wave reduces them and hands the result back to the read's lane group — the first, the last
# and inner groups among them), several-target and one-target segments of a lane group, and empty reads, side by side
ONE_WAVE = [(65, "two"), (2, "species"), (1, "one"), (64, "two"), (130, "one"), (0, "one"), (33, "species"), (65, "species"),
            (5, "two-no-species"), (64, "one"), (3, "no-species"), (65, "one"), (0, "two"), (40, "two"), (1, "no-species"), (65, "two")]


@pytest.mark.parametrize("level", ["species", "strain"])
def test_long_and_small_segments_in_one_wave_then_a_wave_of_one_read(db, level):
    """17 reads: the wave above, and the batch's last read alone in a second wave beside 15 lane groups without a read — long (several
    targets, one target), small (several targets, one target) and empty in turn"""
    rng = np.random.default_rng(17)
    first = [segment(rng, m, kind) for m, kind in ONE_WAVE]
    for m, kind in ((65, "two"), (65, "one"), (40, "two"), (3, "one"), (0, "one")):
        case = Case(first + [segment(rng, m, kind)])
        assert case.n == 17
        verdict, _, _, st = run(db, f"one wave and a read, the last one {m} pairs of '{kind}', {level}", case, level == "species")
        assert st["wave_segments"] == 5 + (m > 64) and st["group_segments"] == 9 + (0 < m <= 64)
        assert verdict[16] == (DROP if kind == "two" else KEEP)
        assert list(verdict[[0, 4, 11, 15]]) == [DROP, KEEP, KEEP, DROP] and verdict[7] == (KEEP if level == "species" else DROP)


MILLION = 256 * 4096 + 1  # 1 048 577 reads: 257 tiles of the scan, the second trip of k3_scan_sums

_million = {}


def million():
    if not _million:
        rng = np.random.default_rng(77)
        lens = np.zeros(MILLION, dtype=np.int64)
        some = rng.choice(MILLION, size=40000, replace=False)
        lens[some] = rng.choice([1, 2, 5, 64, 65, 300], size=len(some))
        lens[[0, MILLION - 1, 4095, 4096, 256 * 4096 - 1, 256 * 4096]] = [3, 2, 66, 1, 4, 70]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        case = Case.__new__(Case)
        case.n, case.offs = MILLION, offs
        total = int(offs[-1])
        # a read's columns: one target, or targets of one species, or two species — by the read's index
        read_of = np.repeat(np.arange(MILLION), lens)
        within = np.arange(total) - np.repeat(offs[:-1].astype(np.int64), lens)
        kind = read_of % 3
        ts = targets_of_species(1005)
        col = np.where(kind == 0, 3 * 11 + within % 3, np.where(kind == 1, 3 * np.array(ts)[within % len(ts)] + within % 2, np.where(within % 2 == 0, 3 * 9, 3 * 30 + 1)))
        case.pairs = np.stack([col, 1 + (np.arange(total) % 97)], axis=1).astype(np.uint32)
        case.nk = np.where(np.arange(MILLION) % 11 == 0, FINAL_N + 1, 130).astype(np.int32)
        _million["case"] = case
        _million["ref"] = vector_reference(case)
    return _million["case"], _million["ref"]


def vector_reference(case, final_n=FINAL_N):
    """`reference` for many reads, with reduceat over the reads that have pairs (species level)"""
    lens = np.diff(case.offs.astype(np.int64))
    has = np.flatnonzero(lens)
    starts = case.offs[:-1].astype(np.int64)[has]
    t, s = TARGET[case.pairs[:, 0]], SPECIES[case.pairs[:, 0]]
    tmin, tmax = np.minimum.reduceat(t, starts), np.maximum.reduceat(t, starts)
    smin, smax = np.minimum.reduceat(s, starts), np.maximum.reduceat(s, starts)
    keep = (tmin == tmax) | ((smin == smax) & (smin != 0))
    host = case.nk[has] > final_n
    verdict = np.full(case.n, KEEP, dtype=np.uint8)
    verdict[has] = np.where(host, HOST, np.where(keep, KEEP, DROP))
    kept_len = np.where(verdict == DROP, 0, lens)
    out_offs = np.concatenate([[0], np.cumsum(kept_len)]).astype(np.uint64)
    judged = ~host
    st = dict(kept=int((keep & judged).sum()), dropped=int((~keep & judged).sum()), host=int(host.sum()),
              group_segments=int((judged & (lens[has] <= 64)).sum()), wave_segments=int((judged & (lens[has] > 64)).sum()), bad_segments=0,
              pairs_in=int(case.offs[-1]), pairs_out=int(out_offs[-1]))
    return verdict, out_offs, case.pairs[np.repeat(verdict != DROP, lens)], st


def test_the_vector_reference_is_the_plain_one():
    """(no GPU work: the two numpy restatements against each other, on a case with every kind of read)"""
    case = mostly_short(3000, seed=9, fill=0.6)
    case.nk[::7] = FINAL_N + 1
    a, b = reference(case, True), vector_reference(case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_a_million_mostly_empty_reads(db):
    case, ref = million()
    st = run(db, f"{MILLION} reads", case, ref=ref)[3]
    assert st["kept"] > 5000 and st["dropped"] > 5000 and st["host"] > 2000 and st["wave_segments"] > 1000


def test_workspace_reuse(db):
    """a large batch, then a small one twice, on one handle: each is right, nothing of the earlier call leaks"""
    case, ref = million()
    run(db, "reuse: a million reads", case, ref=ref)
    small = mostly_short(300, seed=4, fill=0.8)
    a = run(db, "reuse: 300 reads after a million", small)
    b = run(db, "reuse: 300 reads again", small, level_species=False)
    assert a[3]["pairs_in"] == b[3]["pairs_in"] and a[3]["kept"] > b[3]["kept"]


def test_the_stage_off_and_bad_arguments(db):
    import torch

    from kmcp_amd.lib import KmcpGpuError
    dev = torch.device("cuda", 0)
    run(db, "before off", mostly_short(40, seed=2))
    db.set_specific()
    st, launches = db.last_specific()
    assert launches == [] and not any(st.values())
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    with pytest.raises(KmcpGpuError, match="stage is off"):
        db.specific_device(z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), 1, FINAL_N, z.data_ptr(), 1, z.data_ptr(), z.data_ptr())
    with pytest.raises(KmcpGpuError, match="600 columns"):
        db.set_specific(TARGET[:-1], SPECIES[:-1])
    db.set_specific(TARGET, SPECIES)
    with pytest.raises(KmcpGpuError, match="out_cap"):
        db.specific_device(z.data_ptr(), z.data_ptr(), 4, z.data_ptr(), 1, FINAL_N, z.data_ptr(), 3, z.data_ptr(), z.data_ptr())
    db.set_profiling(0)
    try:
        run(db, "no profiling: the counters, no launch records", mostly_short(40, seed=2), profiled=False)
    finally:
        db.set_profiling(1)
