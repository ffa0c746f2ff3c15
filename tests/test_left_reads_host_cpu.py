"""The host half of the counting stages (K6, K7, K8) alone: kmcpg_count_left_reads on a metadata-only handle — no GPU — runs the one walk
of the reads a batch's kernels LEFT (kmcp_amd/csrc/finalize.cpp left_reads_host) into the handle's host state, on one list of seven reads:
    0  an empty read                                   4  K3_WG_CAP + 1 pairs in random order: the walk orders them itself
    1  one pair                                        5  exactly K3_WG_CAP pairs in final order: the walk takes them as they are
    2  three pairs, two targets                        6  a read no stage takes
    3  three pairs that all fail -t
What is expected comes from code the walk does not share: every read's final rows from kmcpg_finalize_grouped on the same list, and from
those rows the counters by the plain restatements of the stages' own GPU tests — `reference` of tests/test_gpu_refstats_alone.py (stage 1
of profile.go over the rows as a TSV), `Case.brute` of tests/test_gpu_cooccur_alone.py (the pair count) and `brute` of
tests/test_gpu_recount_alone.py (recount_rule.hpp in Python), imported as they are.  `reference` leaves out the reads its kernel would
leave to the host (above K6_CAP rows with several targets, above K3_WG_CAP rows): the host half takes exactly those, so the two caps are
lifted while it is called here; nothing else of it changes.  The tables are the restatements' own, cut to the database's 12 columns: three
columns per target; K6's species join two neighbouring targets, K8's all four.  Every comparison is exact."""
import os

import numpy as np
import pytest

from tests import test_gpu_cooccur_alone as A7
from tests import test_gpu_recount_alone as A8
from tests import test_gpu_refstats_alone as A6

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "shim", "testdata", "db", "R001")
EINVAL = -1
WG_CAP = 4096  # K3_WG_CAP
H = 0.75
N_READS = 7
EVERY = tuple(range(N_READS))
# the reads each stage takes in the handing-over tests: three different sets, read 6 in none, the read that fails -t in all
MASKS = ((0, 1, 3, 4), (2, 3, 4, 5), (3, 4, 5))
SHARED = {(0, 1): 50, (0, 2): 1, (1, 2): 1, (0, 3): 2}


def classes_of():
    """stage-1 sums that make the correction bite: target 1 beats target 0 where they meet, target 2 holds its own; target 3 was dropped"""
    c = A8.classes_of()
    for t, (kept, reads, ureads) in enumerate([(1, 100, 30), (1, 100, 1000), (1, 100, 60), (0, 100, 50)]):
        c["kept"][t], c["reads"][t], c["ureads"][t] = kept, reads, ureads
    return c


class TheList:
    def __init__(self, db):
        from kmcp_amd import default_params, lib
        rng = np.random.default_rng(31)
        self.n_cols = n_cols = int(db.info.n_cols)
        assert n_cols == 12
        self.params = default_params()
        self.qk = np.array([130, 130, 128, 130, 130, 127, 130], np.int32)
        self.ql = np.array([150, 151, 149, 150, 152, 148, 150], np.int32)
        # short segments arrive in K3's order: descending counts of one query are descending qCov, the default order
        short = {1: [(5, 100)], 2: [(0, 120), (7, 110), (1, 100)], 3: [(2, 60), (9, 50), (4, 40)], 6: [(3, 125), (10, 90)]}
        segs = [np.array(short.get(r, []), np.uint32).reshape(-1, 2) for r in range(N_READS)]
        for r, m in ((4, WG_CAP + 1), (5, WG_CAP)):  # columns and counts as tests/test_finalize_grouped_cpu.py draws them
            segs[r] = np.stack([rng.integers(0, n_cols, size=m), rng.integers(80, 128, size=m)], axis=1).astype(np.uint32)
        # read 5 in final order: what the host half (kmcpg_finalize) makes of its hits, nothing filtered
        hits = np.empty(WG_CAP, dtype=lib.HIT_DTYPE)
        hits["read"], hits["col"], hits["count"] = 0, segs[5][:, 0], segs[5][:, 1]
        ordered = db.finalize(hits, self.qk[5:6], self.ql[5:6], params=default_params(max_fpr=1.0))
        assert len(ordered.matches) == WG_CAP
        segs[5] = np.stack([ordered.matches["col"], ordered.matches["mkmers"]], axis=1).astype(np.uint32)
        self.pairs = np.ascontiguousarray(np.concatenate(segs))
        self.offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
        # the final rows of every read, by code the walk does not share
        fin = db.finalize_grouped(self.pairs, np.concatenate([self.offs, [np.uint64(0)]]), self.qk, self.ql, params=self.params)
        self.rows = [np.stack([fin.read(r)["col"], fin.read(r)["mkmers"]], axis=1).astype(np.uint32).reshape(-1, 2) for r in range(N_READS)]
        assert [len(x) for x in self.rows[:4]] == [0, 1, 3, 0] and len(self.rows[4]) > WG_CAP // 2 and len(self.rows[5]) > WG_CAP // 2 and len(self.rows[6]) == 2
        assert np.array_equal(self.rows[2], segs[2]) and not np.array_equal(self.rows[4], segs[4][:len(self.rows[4])])  # read 4 did need the order
        self._expected = {}

    def left(self, reads):
        m = np.zeros(N_READS, np.uint8)
        m[list(reads)] = 1
        return m

    def rows_of(self, reads):
        return [self.rows[r] if r in reads else np.zeros((0, 2), np.uint32) for r in range(N_READS)]

    def expected(self, taken):
        """(K6's counters [n_cols, 4], K6 matched, unique; K7's pairs; K8's counters, [recounted, unique, corrected]) for the reads each stage takes
        (None: the stage is off)"""
        if taken in self._expected:
            return self._expected[taken]
        k6 = k7 = k8 = None
        if taken[0] is not None:
            rows = self.rows_of(taken[0])
            flat = np.concatenate(rows)
            case = A6.Case([x[:, 0] for x in rows], nk=self.qk, counts=flat[:, 1], final_n=1 << 30)
            caps = A6.WG_CAP, A6.CAP
            A6.WG_CAP = A6.CAP = 1 << 30  # (see the module's text: the host half takes the reads the restatement's kernel would leave)
            try:
                want, matched, unique, _ = A6.reference([case], True, H)
            finally:
                A6.WG_CAP, A6.CAP = caps
            assert not want[self.n_cols:].any()
            k6 = (want[:self.n_cols], matched, unique)
        if taken[1] is not None:
            k7 = dict(A7.Case([x[:, 0] for x in self.rows_of(taken[1])], nk=self.qk).brute(range(N_READS)))
        if taken[2] is not None:
            cnt, tot = A8.brute([(A8.Case(self.rows_of(taken[2]), nk=self.qk, qlen=self.ql), range(N_READS))], classes_of(), SHARED)
            assert not any(any(c) for c in cnt[self.n_cols:])
            k8 = (cnt[:self.n_cols], tot)
        self._expected[taken] = (k6, k7, k8)
        return k6, k7, k8


@pytest.fixture(scope="module")
def db():
    from kmcp_amd import Database
    with Database.open(DB, device=-1) as h:
        yield h


@pytest.fixture(scope="module")
def the_list(db):
    return TheList(db)


def stages_on(db, on=(True, True, True)):
    """the stages set anew (their host state empty), with the tables of the restatements"""
    n = int(db.info.n_cols)
    db.set_refstats(*((A6.TARGET[:n], A6.SPECIES[:n]) if on[0] else ()), hic_min_qcov=H)
    db.set_cooccur(*((A7.TARGET[:n],) if on[1] else ()))
    db.set_recount(*((A8.TARGET[:n], A8.SPECIES[:n]) if on[2] else ()), hic_min_qcov=A8.H)


def count(db, L, masks, **kw):
    db.count_left_reads(L.pairs, L.offs, L.qk, L.ql, params=L.params,
                        **dict(zip(("left_refstats", "left_cooccur", "left_recount"), (None if m is None else L.left(m) for m in masks))), **kw)


def read_outs(db, on=(True, True, True)):
    """everything the three read-outs give, in a form that compares with =="""
    n = int(db.info.n_cols)
    out = []
    if on[0]:
        cols, tot = db.refstats_read(n)
        out.append((cols.view(np.uint64).reshape(n, 4).tolist(), tot))
    if on[1]:
        out.append(A7.table(db))
    if on[2]:
        db.recount_run(classes_of(), A8.pairs_of(SHARED))
        cols, tot = db.recount_read()
        out.append(([[int(x) for x in row] for row in cols.tolist()], tot))
    return out


def check(db, L, taken):
    """the read-outs against the restatements over the reads each stage took; returns the read-outs"""
    on = tuple(t is not None for t in taken)
    k6, k7, k8 = L.expected(taken)
    got = read_outs(db, on)
    it = iter(got)
    if on[0]:
        cols, tot = next(it)
        assert cols == k6[0].tolist(), "K6's counters"
        assert tot == dict(matched_reads=k6[1], unique_reads=k6[2], host_reads=k6[1], skipped_launches=0), tot
    if on[1]:
        table, tot = next(it)
        assert table == k7, "K7's pairs"
        assert tot["host_adds"] == sum(k7.values()) and tot["device_adds"] == 0, tot
    if on[2]:
        cols, tot = next(it)
        assert cols == k8[0], "K8's counters"
        assert [tot["recounted_reads"], tot["unique_reads"], tot["corrected_reads"]] == k8[1], tot
        assert tot["host_reads"] == tot["replayed_reads"] == sum(len(L.rows[r]) > 0 for r in taken[2]) and tot["logged_reads"] == tot["single_reads"] == 0, tot
    return got


def test_the_entry_is_exported_and_wrapped():
    from kmcp_amd import Database, lib
    assert "kmcpg_count_left_reads" in lib.EXPORTS and lib.load().kmcpg_count_left_reads and callable(Database.count_left_reads)


def test_the_sample_exercises_every_rule(db, the_list):
    """the restatements see reads of one and of several targets, under one species and not, and a correction"""
    k6, k7, k8 = the_list.expected((EVERY, EVERY, EVERY))
    assert 0 < k6[2] < k6[1] == 5 and (k6[0] > 0).any()
    assert len(k7) == 6 and max(k7.values()) == 3
    assert k8[1][0] == 5 and k8[1][2] >= 2 and 0 < k8[1][1] < 5 and any(c[0] for c in k8[0])


def test_a_null_mask_means_every_read(db, the_list):
    stages_on(db)
    count(db, the_list, (None, None, None))
    got = check(db, the_list, (EVERY, EVERY, EVERY))
    stages_on(db)
    count(db, the_list, (EVERY, EVERY, EVERY))
    assert read_outs(db) == got


def test_three_masks_hand_each_read_to_the_stages_that_take_it(db, the_list):
    stages_on(db)
    count(db, the_list, MASKS)
    got = check(db, the_list, MASKS)
    # ... which is the sum of three calls with one stage's mask each
    stages_on(db)
    for s in range(3):
        count(db, the_list, tuple(MASKS[s] if i == s else () for i in range(3)))
    assert read_outs(db) == got
    # a second batch adds to the first
    count(db, the_list, ((), (2,), ()))
    assert A7.table(db)[0] == {k: v + (k == (0, 2)) for k, v in got[1][0].items()}


@pytest.mark.parametrize("off", [0, 1, 2])
def test_a_stage_that_is_off_is_left_out_and_its_mask_ignored(db, the_list, off):
    on = tuple(s != off for s in range(3))
    stages_on(db, on)
    count(db, the_list, tuple(EVERY if s == off else MASKS[s] for s in range(3)))
    check(db, the_list, tuple(None if s == off else MASKS[s] for s in range(3)))


def test_bad_lists_are_refused_and_every_stage_off_is_no_work(db, the_list):
    from kmcp_amd import lib
    L = the_list
    good = np.array([[0, 100]], np.uint32)
    qk, ql = np.array([130, 130], np.int32), np.array([150, 150], np.int32)

    def refused(pairs, offs):
        with pytest.raises(lib.KmcpGpuError) as e:
            db.count_left_reads(pairs, np.array(offs, np.uint64), qk, ql)
        assert e.value.code == EINVAL, e.value
        return str(e.value)

    stages_on(db)
    assert "grouped hit list: offsets out of range" in refused(good, [0, 1, 0])   # backwards
    assert "grouped hit list: offsets out of range" in refused(good, [0, 2, 1])   # past the end
    assert "grouped hit list: columns out of range" in refused(np.array([[L.n_cols, 100]], np.uint32), [0, 1, 1])
    assert "read_offs[0] must be 0" in refused(good, [1, 1, 1])
    db.count_left_reads(good, np.array([0, 1, 0], np.uint64), qk, ql, left_refstats=[0, 0], left_cooccur=[0, 0], left_recount=[0, 0])  # (a read nobody takes is not looked at)
    stages_on(db, (False, False, False))
    count(db, L, (None, None, None))
    for read in (lambda: db.refstats_read(L.n_cols), db.cooccur_read, db.recount_read):
        with pytest.raises(lib.KmcpGpuError):
            read()
    stages_on(db)
    assert read_outs(db) == read_outs(db) and not np.array(read_outs(db)[0][0]).any() and read_outs(db)[1][0] == {}
    stages_on(db, (False, False, False))
