"""K8 alone (kmcp_amd/csrc/k8_recount.hip): k8_log driven through kmcpg_recount_log_device on pair lists the test lays out, then
k8_replay through kmcpg_recount_run, against the semantics of kmcp_amd/csrc/recount_rule.hpp restated here in a few lines of Python
(`brute`: the kept rows, the targets by first row, the stable order by printed qCov, the reference's double loop AS WRITTEN, the integer
shares) over exactly the reads with LEFT byte 0.  Compared: all four counters of every column as integers, the totals, the LEFT bytes (and
the guard bytes behind them), the inputs (unchanged), and the witness of both kernels.

The table: three columns per target (its chunks); species: four targets per species, species 0 (none) for the targets from 160 on."""
import os

import numpy as np
import pytest

from tests import k3_cases as K

pytestmark = pytest.mark.gpu

GUARD = 64
N_COLS = 600
N_CLASSES = N_COLS // 3
CAP = 64        # K8_CAP
WG_CAP = 4096   # K3_WG_CAP
FINAL_N = 512
UNIT, BASE = 720720, 65536
H = 0.75
TARGET = (np.arange(N_COLS) // 3).astype(np.uint32)
SPECIES = np.where(TARGET < 160, TARGET // 4 + 1, 0).astype(np.uint32)
KNOBS = ("KMCPG_RECOUNT_SLOTS", "KMCPG_RECOUNT_WGS")


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = K.build_database(oracle_lib, tmp_path_factory.mktemp("k8db"), N_COLS, seed=904)
    with Database.open(d, device=0) as h:
        assert int(h.info.n_cols) == N_COLS
        h.set_profiling(1)
        yield h


def configure(db, log_bytes=1 << 20, slots=None, species=True):
    """the stage set anew (zeroed counters, an empty log); KMCPG_RECOUNT_SLOTS is read then"""
    for k in KNOBS:
        os.environ.pop(k, None)
    if slots is not None:
        os.environ["KMCPG_RECOUNT_SLOTS"] = str(slots)
    try:
        db.set_recount(TARGET, SPECIES if species else None, hic_min_qcov=H, log_bytes=log_bytes)
    finally:
        os.environ.pop("KMCPG_RECOUNT_SLOTS", None)


def classes_of(kept=None, reads=None, ureads=None):
    from kmcp_amd import lib
    c = np.zeros(N_CLASSES, dtype=lib.RECOUNT_CLASS_DTYPE)
    c["kept"] = 1 if kept is None else kept
    c["reads"] = 100 if reads is None else reads
    c["ureads"] = 50 if ureads is None else ureads
    return c


def pairs_of(shared):
    """{(a, b): reads} -> COOCCUR_DTYPE sorted by (class_a, class_b)"""
    from kmcp_amd import lib
    keys = sorted((min(a, b), max(a, b)) for a, b in shared)
    out = np.zeros(len(keys), dtype=lib.COOCCUR_DTYPE)
    for i, (a, b) in enumerate(keys):
        out[i] = (a, b, shared.get((a, b), shared.get((b, a))))
    return out


def seg(targets, counts=None, chunks=None):
    """a read's pairs: one per target in the order given, [(column, count)]"""
    t = np.asarray(targets, dtype=np.int64)
    ch = np.arange(len(t)) % 3 if chunks is None else np.asarray(chunks)
    cn = np.full(len(t), 100) if counts is None else np.asarray(counts)
    return np.stack([3 * t + ch, cn], axis=1).astype(np.uint32)


class Case:
    def __init__(self, segs, nk=None, qlen=None, final_n=FINAL_N):
        self.n = len(segs)
        self.final_n = final_n
        lens = np.array([len(s) for s in segs], dtype=np.int64)
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.pairs = np.concatenate(segs).astype(np.uint32).reshape(-1, 2) if lens.sum() else np.zeros((0, 2), dtype=np.uint32)
        self.nk = np.full(self.n, 130, dtype=np.int32) if nk is None else np.asarray(nk, dtype=np.int32)
        self.qlen = (150 + np.arange(self.n) % 7).astype(np.int32) if qlen is None else np.asarray(qlen, dtype=np.int32)

    def rows(self, r):
        return self.pairs[int(self.offs[r]):int(self.offs[r + 1])]

    def classify(self, r):
        m = len(self.rows(r))
        if m == 0:
            return "empty"
        if self.nk[r] > self.final_n or m > WG_CAP:
            return "left"
        if len(set(TARGET[self.rows(r)[:, 0]].tolist())) == 1:
            return "single"
        return "logged" if m <= CAP else "left"


def qcov(count, nk):
    return float("%.4f" % (float(count) / float(nk)))  # printed_qcov (k3_set_order.hpp): the digits %.4f prints, parsed back


def brute(cases_reads, classes, shared, D=0.05, R=0.05, no_amb_corr=False, level_species=True, species=True):
    """recount_rule.hpp over the given (case, reads): (counters [N_COLS, 4] as Python integers, [recounted, unique, corrected])"""
    cnt = [[0, 0, 0, 0] for _ in range(N_COLS)]
    tot = [0, 0, 0]
    one_minus = 1 - D
    for case, reads in cases_reads:
        for r in reads:
            rows = [(int(c), int(n)) for c, n in case.rows(r) if classes["kept"][TARGET[c]]]
            if not rows:
                continue
            by_target = {}
            for i, (c, _) in enumerate(rows):
                by_target.setdefault(int(TARGET[c]), []).append(i)
            nk, ql = int(case.nk[r]), max(int(case.qlen[r]), 0)
            firstq = {t: qcov(rows[ix[0]][1], nk) for t, ix in by_target.items()}
            order = sorted(by_target, key=lambda t: -firstq[t])  # stable: ties keep the order of the first rows
            dele = [False] * len(order)
            if len(order) > 1 and not no_amb_corr:
                for i in range(len(order) - 1):
                    if dele[i]:
                        continue
                    for j in range(i + 1, len(order)):
                        if dele[j]:
                            continue
                        a, b = order[i], order[j]
                        n = float(shared.get((min(a, b), max(a, b)), 0))
                        if float(classes["reads"][a]) * one_minus >= n and float(classes["ureads"][b]) < float(classes["ureads"][a]) * R:
                            dele[j] = True
                        elif float(classes["reads"][b]) * one_minus >= n and float(classes["ureads"][a]) < float(classes["ureads"][b]) * R:
                            dele[i] = True
            surv = [t for k, t in enumerate(order) if not dele[k]]
            ns = len(surv)
            sp = {int(SPECIES[rows[by_target[t][0]][0]]) if species else 0 for t in surv}
            uniq_first = ns == 1 or (level_species and len(sp) == 1 and 0 not in sp)
            for t in surv:
                m = len(by_target[t])
                for k, i in enumerate(by_target[t]):
                    c, n = rows[i]
                    share = UNIT - (m - 1) * (UNIT // m) if k == 0 else UNIT // m
                    cnt[c][0] += share
                    cnt[c][3] += ql * BASE // (ns * m)
                    if k == 0 and uniq_first:
                        u = UNIT if ns == 1 else share
                        cnt[c][1] += u
                        if qcov(n, nk) >= H:
                            cnt[c][2] += u
            tot[0] += 1
            tot[1] += ns == 1
            tot[2] += any(dele)
    return cnt, tot


def launch(db, name, case, hits=None, max_wgs=0):
    """one kmcpg_recount_log_device call; returns (LEFT bytes, witness, launches)"""
    import torch
    dev = torch.device("cuda", 0)
    n, cap = case.n, len(case.pairs)
    t_pairs = torch.from_numpy(case.pairs.view(np.int64).reshape(-1).copy()).to(dev)
    t_offs = torch.from_numpy(case.offs.view(np.int64).copy()).to(dev)
    t_nk, t_ql = torch.from_numpy(case.nk).to(dev), torch.from_numpy(case.qlen).to(dev)
    t_left = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    t_hits = None if hits is None else torch.tensor([hits[0]], dtype=torch.int64, device=dev)
    db.recount_log_device(t_pairs.data_ptr(), t_offs.data_ptr(), cap, t_nk.data_ptr(), t_ql.data_ptr(), n, case.final_n, t_left.data_ptr(),
                          d_n_hits=None if hits is None else t_hits.data_ptr(), hit_cap=0 if hits is None else hits[1], max_wgs=max_wgs)
    torch.cuda.synchronize()
    st, launches = db.last_recount()
    assert np.array_equal(t_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), case.pairs), f"{name}: the pairs were changed"
    assert np.array_equal(t_offs.cpu().numpy().view(np.uint64), case.offs) and np.array_equal(t_nk.cpu().numpy(), case.nk), f"{name}: an input was changed"
    assert np.array_equal(t_ql.cpu().numpy(), case.qlen), f"{name}: the lengths were changed"
    left = t_left.cpu().numpy()
    assert (left[n:] == 0x5A).all(), f"{name}: a byte behind the LEFT bytes was written"
    return left[:n], st, launches


def check_log(db, name, case, max_wgs=0, full_ok=False):
    """one k8_log launch with its LEFT bytes and witness checked; returns (witness, classes, the reads with LEFT byte 0)"""
    from kmcp_amd import lib
    cl = [case.classify(r) for r in range(case.n)]
    left, st, launches = launch(db, name, case, max_wgs=max_wgs)
    assert set(left.tolist()) <= {0, 1}
    if not full_ok:
        assert left.tolist() == [int(c == "left") for c in cl], f"{name}: the LEFT bytes"
    else:  # a read of the logged class may be LEFT as well (no room); no other class changes
        assert all(left[r] == int(c == "left") for r, c in enumerate(cl) if c != "logged"), f"{name}: the LEFT bytes"
    logged = [r for r in range(case.n) if cl[r] == "logged" and not left[r]]
    n_full = cl.count("logged") - len(logged)
    assert {k: st[k] for k in ("empty", "single", "logged", "left", "left_full")} == dict(empty=cl.count("empty"), single=cl.count("single"), logged=len(logged),
                                                                                          left=cl.count("left") + n_full, left_full=n_full), f"{name}: witness {st}"
    assert (full_ok or n_full == 0) and st["bad_segments"] == 0 and st["skipped"] == 0
    assert [(l.kernel, l.grid, l.block, l.cls) for l in launches if l.kernel == lib.K8_LOG] == ([(lib.K8_LOG, st["grid"], 256, 3)] if case.n else []), name
    assert not case.n or 1 <= st["grid"] <= (case.n + 63) // 64
    # a single-target row adds match and bases, its first row uniq (and hic) too: every add went to LDS or straight to global memory
    singles = [r for r in range(case.n) if cl[r] == "single"]
    n_adds = sum(2 * len(case.rows(r)) + 1 + int(qcov(case.rows(r)[0, 1], case.nk[r]) >= H) - int(case.qlen[r] <= 0) * len(case.rows(r)) for r in singles)
    direct = n_adds - st["lds_adds"]
    assert 0 <= direct <= st["global_adds"] <= max(n_adds, 0) and st["spilled_adds"] == direct, f"{name}: {n_adds} adds, witness {st}"
    return st, cl, [r for r in range(case.n) if cl[r] in ("single", "logged") and not left[r]]


def check_replay(db, name, counted, classes, shared, species=True, **params):
    """kmcpg_recount_run + kmcpg_recount_read against the brute force over `counted` = [(case, reads)]; returns (counters, totals, witness)"""
    from kmcp_amd import lib
    db.recount_run(classes, pairs_of(shared), min_dreads_prop=params.get("D", 0.05), max_mismatch_err=params.get("R", 0.05),
                   no_amb_corr=params.get("no_amb_corr", False), level_species=params.get("level_species", True))
    got, tot = db.recount_read()
    want, wt = brute(counted, classes, shared, species=species, **params)
    g = [[int(x) for x in row] for row in got.tolist()]
    bad = [c for c in range(N_COLS) if g[c] != want[c]]
    assert not bad, f"{name}: column {bad[0]}: {g[bad[0]]}, expected {want[bad[0]]} ({len(bad)} columns differ)"
    assert [tot["recounted_reads"], tot["unique_reads"], tot["corrected_reads"]] == wt, f"{name}: totals {tot}, expected {wt}"
    st, launches = db.last_recount()
    n_multi = sum(1 for case, reads in counted for r in reads if case.classify(r) == "logged")
    assert st["replay_reads"] == tot["logged_reads"] == n_multi and tot["replayed_reads"] == n_multi and tot["host_reads"] == 0
    assert tot["single_reads"] + st["replay_recounted"] == wt[0] and st["replay_corrected"] == wt[2]
    assert [(l.kernel, l.block, l.cls) for l in launches if l.kernel == lib.K8_REPLAY] == ([(lib.K8_REPLAY, 256, 3)] if n_multi else [])
    assert (st["replay_grid"] == 0) == (n_multi == 0) and st["replay_grid"] <= (n_multi + 63) // 64
    assert tot["log_bytes_used"] == st["log_bytes_used"] == 8 * sum(len(case.rows(r)) + 3 for case, reads in counted for r in reads if case.classify(r) == "logged")
    return got, tot, st


def run(db, name, case, classes=None, shared=None, max_wgs=0, species=True, log_bytes=1 << 20, slots=None, **params):
    """one case into a freshly set stage, logged and replayed, against the brute force"""
    configure(db, log_bytes=log_bytes, slots=slots, species=species)
    classes = classes_of() if classes is None else classes
    st, cl, counted = check_log(db, name, case, max_wgs=max_wgs)
    got, tot, rst = check_replay(db, name, [(case, counted)], classes, shared or {}, species=species, **params)
    return st, cl, got, tot, rst


def mixed(n_reads, seed):
    """reads of every class side by side, counts not descending, ties in qCov"""
    rng = np.random.default_rng(seed)
    segs, nk = [], []
    for r in range(n_reads):
        kind = r % 6
        if kind == 0:
            segs.append(np.zeros((0, 2), dtype=np.uint32))
        elif kind == 1:
            m = int(rng.integers(1, 9))
            segs.append(seg([int(rng.integers(0, 200))] * m, counts=rng.integers(60, 131, size=m), chunks=rng.integers(0, 3, size=m)))
        elif kind == 5 and r % 30 == 5:
            segs.append(seg(np.tile(rng.permutation(200)[:2], 33)[:65]))  # 65 pairs, two targets: LEFT
        else:
            m = int(rng.choice([2, 3, 5, 9, 17]))
            t = rng.choice(rng.permutation(40)[:m], size=m + int(rng.integers(0, 4)))
            segs.append(seg(t, counts=rng.choice([70, 90, 90, 100, 104, 130], size=len(t)), chunks=rng.integers(0, 3, size=len(t))))
        nk.append(int(rng.choice([130, 130, 130, FINAL_N, FINAL_N + 1])))
    return Case(segs, nk=nk)


def mixed_inputs(seed):
    """stage-1 sums and a pair list that make the correction bite: a few strong targets, many weak ones, some dropped"""
    rng = np.random.default_rng(seed)
    ureads = rng.choice([0, 1, 2, 40, 400, 4000], size=N_CLASSES)
    c = classes_of(kept=(rng.random(N_CLASSES) < 0.85).astype(np.uint32), reads=ureads + rng.integers(1, 500, size=N_CLASSES), ureads=ureads)
    shared = {(int(a), int(b)): int(rng.choice([1, 5, 50, 3000])) for a in range(40) for b in range(a + 1, 40) if rng.random() < 0.7}
    return c, shared


QUIRK = dict(reads=[100, 100, 100], ureads=[30, 1000, 1])  # b beats a, a beats c; b does not beat c: they share 96 reads, above 95 % of either's


def quirk_inputs():
    c = classes_of()
    for t, (rd, u) in enumerate(zip(QUIRK["reads"], QUIRK["ureads"])):
        c["reads"][10 + t], c["ureads"][10 + t] = rd, u
    return c, {(11, 12): 96, (10, 11): 1, (10, 12): 1}


# ---- the log kernel ----
def test_no_reads_and_one_empty_read(db):
    st, _, got, tot, _ = run(db, "0 reads", Case([]))
    assert st["grid"] == 0 and not got.view(np.uint64).any() and tot["recounted_reads"] == 0
    st, cl, got, tot, _ = run(db, "one empty read", Case([np.zeros((0, 2), dtype=np.uint32)]))
    assert cl == ["empty"] and not got.view(np.uint64).any() and tot["log_bytes_used"] == 0


@pytest.mark.parametrize("m", [1, 17, 65, 4096])
def test_a_single_target_read(db, m):
    rng = np.random.default_rng(m)
    case = Case([seg([11] * m, counts=rng.integers(60, 131, size=m), chunks=rng.integers(0, 3, size=m))], qlen=[151])
    st, cl, got, tot, _ = run(db, f"single {m}", case)
    assert cl == ["single"] and tot["single_reads"] == tot["unique_reads"] == 1 and tot["logged_reads"] == 0
    assert int(got["match"].sum()) == UNIT and int(got["uniq"].sum()) == UNIT  # a target's rows sum to exactly one read, whatever m
    # ... and if stage 1 drops the reference its columns are ignored at read-out
    c = classes_of()
    c["kept"][11] = 0
    got, tot, _ = check_replay(db, "dropped", [(case, [0])], c, {})
    assert not got.view(np.uint64).any() and tot["recounted_reads"] == tot["single_reads"] == 0


def test_every_left_class(db):
    case = Case([seg([4, 5] * 32 + [4]), seg([4, 5]), seg([4, 5]), seg([6] * 3), seg([9] * (WG_CAP + 1)), seg([4, 5] * 32)],
                nk=[130, FINAL_N + 1, FINAL_N, FINAL_N + 1, 130, 130])
    _, cl, _, tot, _ = run(db, "left", case)
    assert cl == ["left", "left", "logged", "left", "left", "logged"] and tot["logged_reads"] == 2


@pytest.mark.parametrize("n_reads", [16, 17, 65])
def test_read_counts_at_the_wave_and_workgroup_edges(db, n_reads):
    classes, shared = mixed_inputs(n_reads)
    st, cl, _, tot, rst = run(db, f"{n_reads} reads", mixed(n_reads, seed=n_reads), classes, shared)
    assert "logged" in cl and "single" in cl and st["grid"] == (n_reads + 63) // 64


def test_1000_reads_on_one_workgroup_take_grid_stride_rounds(db):
    case = mixed(1000, seed=77)
    classes, shared = mixed_inputs(77)
    st, cl, got, tot, rst = run(db, "1 workgroup", case, classes, shared, max_wgs=1)
    assert st["grid"] == 1 and {"empty", "single", "logged", "left"} == set(cl)
    assert tot["corrected_reads"] >= 50 and rst["replay_lookups"] > 0 and tot["unique_reads"] > tot["single_reads"]  # the correction bites
    st2, _, got2, tot2, _ = run(db, "all workgroups", case, classes, shared)
    assert st2["grid"] == 16 and got2.tobytes() == got.tobytes() and tot2 == tot  # the same inputs, another grid: the same counters


def test_the_overflow_guard_skips_two_calls_accumulate_and_reset_zeroes(db):
    a, b = mixed(100, seed=21), mixed(37, seed=22)
    classes, shared = mixed_inputs(21)
    configure(db)
    _, _, ca = check_log(db, "first call", a)
    _, _, cb = check_log(db, "second call", b)
    got, tot, _ = check_replay(db, "two calls", [(a, ca), (b, cb)], classes, shared)
    # a hit counter above the capacity: the batch will be run again, nothing is counted or logged now
    left, st, _ = launch(db, "guard", a, hits=(1001, 1000))
    assert st["skipped"] == 1 and not any(st[k] for k in ("empty", "single", "logged", "left", "lds_adds", "global_adds"))
    got2, tot2, _ = check_replay(db, "after the guard", [(a, ca), (b, cb)], classes, shared)
    assert got2.tobytes() == got.tobytes() and tot2 == dict(tot, skipped_launches=1)
    # at the capacity it runs
    _, st, _ = launch(db, "guard", a, hits=(1000, 1000))
    assert st["skipped"] == 0 and st["logged"] > 0
    check_replay(db, "three calls", [(a, ca), (b, cb), (a, ca)], classes, shared)
    db.recount_reset()
    db.recount_run(classes, pairs_of(shared))
    zero, tot3 = db.recount_read()
    assert not zero.view(np.uint64).any() and not any(v for k, v in tot3.items() if k != "log_bytes")


@pytest.mark.parametrize("k", [3, 10])
def test_a_log_with_room_for_exactly_k_reads(db, k):
    """reads of 2 pairs take 5 words each: k of them are logged whole, the others are LEFT whole and counted as left_full"""
    rng = np.random.default_rng(k)
    case = Case([seg(rng.permutation(40)[:2], counts=rng.choice([90, 100], size=2)) for _ in range(40)] + [seg([7] * 2)] * 5)
    classes, shared = mixed_inputs(5)
    configure(db, log_bytes=8 * 5 * k)
    st, cl, counted = check_log(db, "small log", case, full_ok=True)
    assert st["logged"] == k and st["left_full"] == 40 - k and cl.count("logged") == 40
    got, tot, _ = check_replay(db, "small log", [(case, counted)], classes, shared)
    assert tot["left_full"] == 40 - k and tot["logged_reads"] == k and tot["log_bytes_used"] == tot["log_bytes"] == 40 * k
    # a second launch finds no room at all: every multi-target read is LEFT, the single-target ones are counted again
    st, _, again = check_log(db, "full log", case, full_ok=True)
    assert st["logged"] == 0 and st["left_full"] == 40
    check_replay(db, "full log", [(case, counted), (case, again)], classes, shared)


# ---- the replay ----
def test_two_targets_and_the_three_target_quirk_case(db):
    c = classes_of()
    c["ureads"][3], c["ureads"][7] = 1000, 2
    _, cl, got, tot, rst = run(db, "two", Case([seg([7, 3])]), c, {(3, 7): 1})
    assert cl == ["logged"] and tot["corrected_reads"] == tot["unique_reads"] == 1 and rst["replay_lookups"] == 1
    assert int(got["match"][3 * 3 + 1]) == UNIT and int(got["uniq"][3 * 3 + 1]) == UNIT and int(got["match"][3 * 7]) == 0
    # a (10), b (11), c (12) in qCov order: row a deletes a AND goes on to delete c; an implementation that stops there keeps {b, c}
    c, shared = quirk_inputs()
    _, _, got, tot, _ = run(db, "quirk", Case([seg([10, 11, 12], counts=[120, 110, 100])]), c, shared)
    assert tot["unique_reads"] == tot["corrected_reads"] == 1
    assert [int(got["match"][3 * t + k]) for k, t in enumerate((10, 11, 12))] == [0, UNIT, 0]


def test_64_distinct_targets_aba_and_rows_not_in_qcov_order(db):
    rng = np.random.default_rng(1)
    classes, shared = mixed_inputs(3)
    _, cl, _, tot, rst = run(db, "64 distinct", Case([seg(rng.permutation(40).tolist() + list(range(100, 124)), counts=rng.integers(60, 131, size=64))]), classes, shared)
    assert cl == ["logged"] and tot["corrected_reads"] == 1 and rst["replay_lookups"] >= 63
    _, cl, got, tot, _ = run(db, "aba", Case([seg([4, 5] * 32, counts=rng.integers(60, 131, size=64))]))
    assert cl == ["logged"] and int(got["match"].sum()) == 2 * UNIT  # 32 rows each: 720720 is no multiple of 32, the first rows take the remainder
    c, shared = quirk_inputs()  # the quirk's targets with the strongest row last: the order is by qCov, not by row
    _, _, got, tot, _ = run(db, "reversed", Case([seg([12, 11, 10], counts=[100, 110, 120])]), c, shared)
    assert [int(got["match"][3 * t + k]) for k, t in enumerate((12, 11, 10))] == [0, UNIT, 0]


def test_qcov_ties_keep_the_order_of_the_first_rows(db):
    """x (20), y (21), z (22): y beats x, x beats z, y and z do not beat each other (they share too many reads).  At ONE printed qCov:
    x y z -> {y}; y x z -> {y, z}; z x y -> {y}.  104 / 130 and 103.99.. print alike: 0.8000"""
    c = classes_of()
    for t, u in zip((20, 21, 22), (3, 70, 0)):
        c["ureads"][t] = u
    shared = {(21, 22): 99, (20, 21): 1, (20, 22): 1}
    for order, survivors in (((20, 21, 22), {21}), ((21, 20, 22), {21, 22}), ((22, 20, 21), {21})):
        _, _, got, tot, _ = run(db, f"ties {order}", Case([seg(order, counts=[104, 104, 104])]), c, shared)
        assert {t for t in order if int(got["match"][3 * t:3 * t + 3].sum())} == survivors, order
    _, _, got, _, _ = run(db, "no tie", Case([seg((21, 20, 22), counts=[104, 105, 104])]), c, shared)
    assert {t for t in (20, 21, 22) if int(got["match"][3 * t:3 * t + 3].sum())} == {21}


def test_a_pair_missing_from_the_list_shares_nothing(db):
    c = classes_of()
    c["ureads"][30], c["ureads"][31], c["reads"][30] = 1000, 2, 100
    case = Case([seg([30, 31])])
    _, _, _, tot, _ = run(db, "missing", case, c, {(1, 2): 5})
    assert tot["corrected_reads"] == 1  # shared = 0: nothing protects 31
    _, _, _, tot, _ = run(db, "present", case, c, {(30, 31): 96})
    assert tot["corrected_reads"] == 0  # 95 >= 96 is false
    _, _, _, tot, _ = run(db, "empty list", case, c, {})
    assert tot["corrected_reads"] == 1


def test_survivors_in_one_species_or_not_and_no_amb_corr(db):
    # targets 8, 9 (species 3), 12 (species 4), 170 (none)
    same, diff, none = Case([seg([8, 9, 8], counts=[110, 100, 90])]), Case([seg([8, 12])]), Case([seg([170, 171])])
    _, _, got, tot, _ = run(db, "one species", same)
    assert tot["unique_reads"] == 0 and int(got["uniq"].sum()) == UNIT // 2 + UNIT and int(got["hic"].sum()) == UNIT // 2 + UNIT
    for name, case, kw in (("two species", diff, {}), ("species 0", none, {}), ("level strain", same, dict(level_species=False)), ("no table", same, dict(species=False))):
        _, _, got, _, _ = run(db, name, case, **kw)
        assert int(got["uniq"].sum()) == 0 and int(got["match"].sum()) == 2 * UNIT
    c, shared = quirk_inputs()
    _, _, got, tot, _ = run(db, "no_amb_corr", Case([seg([10, 11, 12], counts=[120, 110, 100])]), c, shared, no_amb_corr=True)
    assert tot["corrected_reads"] == 0 and int(got["match"].sum()) == 3 * UNIT


def test_run_twice_gives_the_same_bytes_and_other_parameters_need_no_new_search(db):
    case = mixed(300, seed=5)
    classes, shared = mixed_inputs(6)
    configure(db)
    _, _, counted = check_log(db, "log", case)
    a, ta, _ = check_replay(db, "first", [(case, counted)], classes, shared)
    b, tb, _ = check_replay(db, "second", [(case, counted)], classes, shared)
    assert a.tobytes() == b.tobytes() and ta == tb and ta["corrected_reads"] > 0
    c, tc, _ = check_replay(db, "other D and R", [(case, counted)], classes, shared, D=0.9, R=0.5)
    d, td, _ = check_replay(db, "no_amb_corr", [(case, counted)], classes, shared, no_amb_corr=True)
    assert len({a.tobytes(), c.tobytes(), d.tobytes()}) == 3 and td["corrected_reads"] == 0
    other, _ = mixed_inputs(9)
    check_replay(db, "other verdicts", [(case, counted)], other, shared)
    e, te, _ = check_replay(db, "the first again", [(case, counted)], classes, shared)
    assert e.tobytes() == a.tobytes() and te == ta


def test_a_hot_column_adds_per_workgroup_not_per_read(db):
    n = 1000
    single = Case([seg([50])] * n, qlen=[150] * n)
    st, _, got, _, _ = run(db, "hot column, single", single)
    assert int(got["match"][150]) == n * UNIT and st["lds_adds"] == 4 * n and st["spilled_adds"] == 0 and 0 < st["global_adds"] <= 4 * st["grid"], st
    st, _, got0, _, _ = run(db, "no LDS table", single, slots=0)
    assert st["slots"] == 0 and st["lds_adds"] == 0 and st["global_adds"] == 4 * n and got0.tobytes() == got.tobytes()
    # the replay: 51 always loses to 50, every read ends on column 150
    c = classes_of()
    c["ureads"][50], c["ureads"][51], c["reads"][50] = 1000, 2, 2 * n
    multi = Case([seg([50, 51])] * n, qlen=[150] * n)
    _, _, got, tot, rst = run(db, "hot column, replay", multi, c, {(50, 51): n})
    assert tot["corrected_reads"] == n and int(got["uniq"][150]) == n * UNIT
    assert rst["replay_lds_adds"] == 4 * n and rst["replay_spilled_adds"] == 0 and 0 < rst["replay_global_adds"] <= 4 * rst["replay_grid"], rst
    _, _, got0, _, rst = run(db, "replay, no LDS table", multi, c, {(50, 51): n}, slots=0)
    assert rst["replay_lds_adds"] == 0 and rst["replay_global_adds"] == 4 * n and got0.tobytes() == got.tobytes()


def test_a_2_slot_lds_table_spills_and_counts_the_same(db):
    case = mixed(200, seed=9)
    classes, shared = mixed_inputs(9)
    st, _, got, tot, rst = run(db, "2 slots", case, classes, shared, slots=2)
    assert st["slots"] == 2 and st["spilled_adds"] > 0 and st["lds_adds"] > 0 and rst["replay_spilled_adds"] > 0 and rst["replay_lds_adds"] > 0
    st0, _, got0, tot0, _ = run(db, "default table", case, classes, shared)
    assert st0["slots"] == 1024 and st0["spilled_adds"] == 0 and got0.tobytes() == got.tobytes() and tot0 == tot


def test_the_stage_off_and_bad_arguments(db):
    import torch

    from kmcp_amd import lib
    from kmcp_amd.lib import KmcpGpuError
    z = torch.zeros(8, dtype=torch.int64, device=torch.device("cuda", 0))
    db.set_recount()
    st, launches = db.last_recount()
    assert launches == [] and not any(st.values())
    with pytest.raises(KmcpGpuError, match="stage is off"):
        db.recount_log_device(z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 1, FINAL_N, z.data_ptr())
    with pytest.raises(KmcpGpuError, match="stage is off"):
        db.recount_run(classes_of(), pairs_of({}))
    with pytest.raises(KmcpGpuError, match="log_bytes"):
        db.set_recount(TARGET, SPECIES, log_bytes=8)
    os.environ["KMCPG_RECOUNT_SLOTS"] = "48"
    try:
        with pytest.raises(KmcpGpuError, match="KMCPG_RECOUNT_SLOTS"):
            db.set_recount(TARGET, SPECIES)
    finally:
        os.environ.pop("KMCPG_RECOUNT_SLOTS")
    configure(db)
    with pytest.raises(KmcpGpuError, match="kmcpg_recount_run first"):
        db.recount_read()
    unsorted = np.array([(3, 4, 1), (1, 2, 1)], dtype=lib.COOCCUR_DTYPE)
    with pytest.raises(KmcpGpuError, match="sorted"):
        db.recount_run(classes_of(), unsorted)
    db.set_recount()
