"""The numpy restatement of K3 (tests/k3_cases.py reference) is not trusted on its own word: on metadata-only handles (no GPU) the host
half — kmcpg_finalize on the raw hit list (the round-3 host half), and kmcpg_finalize_grouped on the restatement's own grouping with the
pairs of every segment shuffled (it orders lists that did not come from K3) — must give exactly the restatement's offsets and its
(column, mKmers) per read, for every crafted case of tests/test_gpu_k3_alone.py, every sort mode and the three-member set.

The params leave only -T and the order at work (k3_cases.params_for).  kmcpg_finalize refuses a list with a hit that names no read or
column (K3 counts and drops them): it is given the list without them, and the restatement's `bad` is held against their number."""
import numpy as np
import pytest

from tests import k3_cases as K

MODE_NAMES = ("qcov", "tcov", "jacc", "nosort")


@pytest.fixture(scope="module")
def single_dir(oracle_lib, tmp_path_factory):
    return K.build_database(oracle_lib, tmp_path_factory.mktemp("k3db"), 4200, seed=700)


@pytest.fixture(scope="module")
def single(single_dir):
    from kmcp_amd import Database
    with Database.open(single_dir, device=-1) as db:
        yield db, K.sizes_of(db)


@pytest.fixture(scope="module")
def the_set(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    tmp = tmp_path_factory.mktemp("k3set")
    dirs = [K.build_database(oracle_lib, tmp / f"m{i}", 1500, seed=710 + i) for i in range(3)]
    with Database.open_set(dirs, device=-1) as db:
        yield db, K.sizes_of(db), db.set_info()


def check(db, sizes, name, case, params, bases=None, seed=0):
    ref = K.reference_of(case, sizes, params, bases)
    hits = K.well_formed(case, len(sizes))
    looked_at = min(case.n_hits_word, case.hit_cap)
    tombs = int(np.count_nonzero((hits["read"] == K.NONE) & (hits["col"] == K.NONE)))
    assert ref.bad == looked_at - len(hits)
    qlen = case.nk + 20
    res = db.finalize(hits, case.nk, qlen, params=params)
    got = np.stack([res.matches["col"].astype(np.uint32), res.matches["mkmers"].astype(np.uint32)], axis=1).reshape(-1, 2)
    assert len(ref.pairs) <= len(hits) - tombs
    if params.min_tcov <= 0:
        assert len(ref.pairs) == len(hits) - tombs
    # (the host orders segments of any length: exact equality everywhere)
    exact = ref._replace(classes=(0, 0, 0))
    lens = np.diff(ref.offs.astype(np.int64))
    msg = _difference(name + " finalize", res.offs, got, exact, lens)
    assert msg is None, msg
    grouped = db.finalize_grouped(K.shuffled_segments(ref, np.random.default_rng(seed)), np.concatenate([ref.offs, [np.uint64(0)]]), case.nk, qlen, params=params)
    assert np.array_equal(grouped.offs, res.offs) and grouped.matches.tobytes() == res.matches.tobytes(), name + " finalize_grouped"
    return ref


def _difference(name, offs, pairs, ref, lens):
    if not np.array_equal(np.asarray(offs, dtype=np.uint64), ref.offs):
        r = int(np.flatnonzero(np.asarray(offs, dtype=np.uint64) != ref.offs)[0])
        return f"{name}: offs[{r}] is {int(offs[r])} for {int(ref.offs[r])}"
    diff = np.flatnonzero((pairs != ref.pairs).any(axis=1))
    if len(diff) == 0:
        return None
    i = int(diff[0])
    r = int(np.searchsorted(ref.offs.astype(np.int64), i, side="right")) - 1
    return f"{name}: read {r} ({int(lens[r])} matches) differs at position {i - int(ref.offs[r])}: {pairs[i].tolist()} for {ref.pairs[i].tolist()}"


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_class_edges(single, mode):
    db, sizes = single
    for order in ("runs", "shuffled", "round_robin", "descending"):
        case = K.class_edges(sizes, order)
        ref = check(db, sizes, f"class edges, {order}, {mode}", case, K.params_for(mode))
        lens = np.diff(ref.offs.astype(np.int64))
        assert set(K.EDGE_LENGTHS) <= set(lens.tolist()) and lens[-1] > 0 and ref.classes[1] >= 3 and ref.classes[2] == 1
    ref = check(db, sizes, f"class edges, last read empty, {mode}", K.class_edges(sizes, "runs", last_empty=True), K.params_for(mode))
    assert ref.offs[-1] == ref.offs[-2]


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_runs_and_lanes(single, mode):
    db, sizes = single
    case, breakers = K.runs_and_lanes(sizes)
    assert len(breakers) == 3 and sorted(int(b) % 64 for b in breakers) == [0, 20, 63]
    T = K.tcov_quantile(case, sizes, 1 / 3)
    assert T > 1 / 300
    for t in (0.0, T):
        ref = check(db, sizes, f"runs and lanes, -T {t}, {mode}", case, K.params_for(mode, t))
        assert ref.bad == 12  # four kinds of hits that name no read or column, at three lanes each
        if t:
            assert 0.25 < 1 - len(ref.pairs) / (case.hit_cap - 15) < 0.42
        for name, cut in K.prefixes(case).items():
            check(db, sizes, f"runs and lanes, {name}, -T {t}, {mode}", cut, K.params_for(mode, t))


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_ties_and_the_T_boundary(single, mode):
    db, sizes = single
    case = K.ties(sizes)
    census = K.tie_census(case, sizes)
    assert min(census.values()) >= 20, census
    h, third = case.hits, 1 / 3
    tc = h["count"].astype(np.float64) / sizes[h["col"]].astype(np.float64)
    assert np.count_nonzero(tc == third) >= 50 and np.count_nonzero(tc == 0.05) >= 50
    assert np.count_nonzero((h["count"] == 5) & (sizes[h["col"]] == 100)) and np.count_nonzero((h["count"] == 4) & (sizes[h["col"]] == 81))
    kept = {}
    for t in (0.0, third, float(np.nextafter(third, 1)), float(np.nextafter(third, 0)), 0.05):
        ref = check(db, sizes, f"ties, -T {t!r}, {mode}", case, K.params_for(mode, t))
        kept[t] = len(ref.pairs)
        lens = np.diff(ref.offs.astype(np.int64))
        if t == 0:
            assert ((lens > 1) & (lens <= 512)).sum() >= 5 and (lens > 512).sum() >= 5
    on_third = int(np.count_nonzero(tc == third))
    assert kept[third] == kept[float(np.nextafter(third, 0))] == kept[float(np.nextafter(third, 1))] + on_third  # == -T passes, as the reference's >= does
    assert kept[0.05] == int(np.count_nonzero(tc >= 0.05)) < kept[0.0]


@pytest.mark.parametrize("n_reads", [4094, 4095, 4096, 4097, 8191, 8192, 65535, 256 * 4096 + 5])
def test_many_reads(single, n_reads):
    db, sizes = single
    case = K.many_reads(sizes, n_reads, "runs" if n_reads % 2 else "shuffled")
    for mode in MODE_NAMES if n_reads < 10**6 else ("qcov", "tcov"):
        ref = check(db, sizes, f"{n_reads} reads, {mode}", case, K.params_for(mode))
        lens = np.diff(ref.offs.astype(np.int64))
        assert ref.classes[0] >= 300 and ref.classes[1:] == (4, 1) and lens[-1] == 5
        assert 0.25 < np.count_nonzero(lens) / n_reads < 0.42
        if n_reads > 4097:
            assert lens[4095] == 513 and lens[4096] == 4096
        if n_reads > 10**6:
            assert lens[524288 + 4097] == 2500 and lens[256 * 4096 - 1] == 4097 and lens[256 * 4096] == 1000


def test_many_hits(single):
    db, sizes = single
    case = K.many_hits(sizes)
    assert case.hit_cap > 16384 * 256 and case.hit_cap % 64
    check(db, sizes, "many hits, qcov", case, K.params_for("qcov"))


@pytest.mark.parametrize("mode", ("qcov", "tcov", "jacc"))
def test_set(the_set, mode):
    db, sizes, bases = the_set
    assert len(bases) == 3 and len(sizes) >= 4097
    p = K.params_for(mode)
    for order in ("runs", "shuffled"):
        case = K.class_edges(sizes, order, seed=7, k32=True, big_nk=True)
        ref = check(db, sizes, f"set, class edges, {order}, {mode}", case, p, bases)
        plain = K.reference_of(case, sizes, p)
        short = int(np.count_nonzero((np.diff(ref.offs.astype(np.int64)) >= 2) & (np.diff(ref.offs.astype(np.int64)) <= K.WG_CAP)))
        # many runs of equal printed score span members and are out of member order after the exact sort; some segments have none
        assert ref.mixed_runs >= 500 and 10 <= ref.reordered < short and not np.array_equal(plain.pairs, ref.pairs)
        assert ref.classes == plain.classes and ref.classes[2] == 1 and np.array_equal(ref.offs, plain.offs)
    # the scores the case is there for (sizes as the handle reports them)
    h = case.hits[:case.n_hits_word]
    c, s, nh = h["count"].astype(np.float64), sizes[h["col"]].astype(np.float64), case.nk[h["read"]].astype(np.float64)
    member = np.searchsorted(np.asarray(bases), h["col"], side="right") - 1
    for v in (1 / 32, 3 / 32):
        assert len(set(member[c / s == v].tolist())) == 3, v  # the printed score 0.0312 / 0.0938 in all three members
    score = (c / nh, c / s, c / (nh + s - c))[p.sort_by]
    printed = np.array([float("%.4f" % v) for v in score])
    o = np.lexsort((score, printed, h["read"]))
    near = (h["read"][o][1:] == h["read"][o][:-1]) & (printed[o][1:] == printed[o][:-1]) & (score[o][1:] != score[o][:-1]) & (member[o][1:] != member[o][:-1])
    assert np.count_nonzero(near) >= 20  # scores that differ only beyond the fourth decimal, from different members


def test_one_member_set_is_the_database(single_dir):
    from kmcp_amd import Database
    d = single_dir
    with Database.open(d, device=-1) as db, Database.open_set([d], device=-1) as one:
        sizes = K.sizes_of(db)
        assert np.array_equal(sizes, K.sizes_of(one)) and one.set_info() == [0]
        case = K.class_edges(sizes, "shuffled", seed=9)
        assert case.hits["count"].max() <= 120
        for mode in MODE_NAMES:
            p = K.params_for(mode)
            a, b = db.finalize(case.hits[:case.n_hits_word], case.nk, case.nk + 20, params=p), one.finalize(case.hits[:case.n_hits_word], case.nk, case.nk + 20, params=p)
            assert a.matches.tobytes() == b.matches.tobytes() and np.array_equal(a.offs, b.offs)
            check(one, sizes, f"one-member set, {mode}", case, p)
