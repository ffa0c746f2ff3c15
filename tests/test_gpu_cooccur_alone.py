"""K7 alone (kmcp_amd/csrc/k7_cooccur.hip), driven through kmcpg_cooccur_device on pair lists the test lays out, against a brute force:
for every read the device counted (LEFT byte 0), the set of its columns' targets, and one read for every unordered pair of them.
Compared: the pairs and their counts, the totals, the LEFT bytes (and the guard bytes behind them), the inputs (unchanged), and the
witness: the class each read took, the pairs enumerated, where the adds went, the keys claimed.

The table: three columns per target (its chunks)."""
import os
from collections import Counter
from itertools import combinations

import numpy as np
import pytest

from tests import k3_cases as K

pytestmark = pytest.mark.gpu

GUARD = 64
N_COLS = 600
CAP = 64        # K7_CAP
WG_CAP = 4096   # K3_WG_CAP
FINAL_N = 512
TARGET = (np.arange(N_COLS) // 3).astype(np.uint32)
KNOBS = ("KMCPG_COOCCUR_SLOTS", "KMCPG_COOCCUR_WGS")


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = K.build_database(oracle_lib, tmp_path_factory.mktemp("k7db"), N_COLS, seed=903)
    with Database.open(d, device=0) as h:
        assert int(h.info.n_cols) == N_COLS
        h.set_profiling(1)
        yield h


def configure(db, table_slots=1 << 12, slots=None):
    """the stage set anew (an empty table); KMCPG_COOCCUR_SLOTS is read then"""
    for k in KNOBS:
        os.environ.pop(k, None)
    if slots is not None:
        os.environ["KMCPG_COOCCUR_SLOTS"] = str(slots)
    try:
        db.set_cooccur(TARGET, table_slots=table_slots)
    finally:
        os.environ.pop("KMCPG_COOCCUR_SLOTS", None)


def cols_of(targets, rng=None):
    """one column per target, in the order given: the chunk varies"""
    t = np.asarray(targets, dtype=np.uint32)
    chunk = np.arange(len(t)) % 3 if rng is None else rng.integers(0, 3, size=len(t))
    return (3 * t + chunk).astype(np.uint32)


class Case:
    def __init__(self, segs, nk=None, final_n=FINAL_N):
        lens = np.array([len(s) for s in segs], dtype=np.int64)
        self.n = len(segs)
        self.final_n = final_n
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        cols = np.concatenate(segs).astype(np.uint32) if lens.sum() else np.zeros(0, dtype=np.uint32)
        self.nk = np.full(self.n, 130, dtype=np.int32) if nk is None else np.asarray(nk, dtype=np.int32)
        self.pairs = np.empty((len(cols), 2), dtype=np.uint32)
        self.pairs[:, 0] = cols
        self.pairs[:, 1] = 100
        self.targets = [sorted(set(TARGET[self.pairs[int(self.offs[r]):int(self.offs[r + 1]), 0]].tolist())) for r in range(self.n)]

    def classify(self, r):
        m = int(self.offs[r + 1] - self.offs[r])
        if m == 0:
            return "empty"
        if self.nk[r] > self.final_n or m > WG_CAP:
            return "left"
        if len(self.targets[r]) == 1:
            return "single"
        return "wave" if m <= CAP else "left"

    def brute(self, reads):
        """pair -> reads, over the given reads"""
        c = Counter()
        for r in reads:
            c.update(combinations(self.targets[r], 2))
        return c


def launch(db, name, case, hits=None, max_wgs=0):
    """one kmcpg_cooccur_device call; returns (LEFT bytes, witness, launches)"""
    import torch
    dev = torch.device("cuda", 0)
    n, cap = case.n, len(case.pairs)
    t_pairs = torch.from_numpy(case.pairs.view(np.int64).reshape(-1).copy()).to(dev)
    t_offs = torch.from_numpy(case.offs.view(np.int64).copy()).to(dev)
    t_nk = torch.from_numpy(case.nk).to(dev)
    t_left = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    t_hits = None if hits is None else torch.tensor([hits[0]], dtype=torch.int64, device=dev)
    db.cooccur_device(t_pairs.data_ptr(), t_offs.data_ptr(), cap, t_nk.data_ptr(), n, case.final_n, t_left.data_ptr(),
                      d_n_hits=None if hits is None else t_hits.data_ptr(), hit_cap=0 if hits is None else hits[1], max_wgs=max_wgs)
    torch.cuda.synchronize()
    st, launches = db.last_cooccur()
    assert np.array_equal(t_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), case.pairs), f"{name}: the pairs were changed"
    assert np.array_equal(t_offs.cpu().numpy().view(np.uint64), case.offs) and np.array_equal(t_nk.cpu().numpy(), case.nk), f"{name}: an input was changed"
    left = t_left.cpu().numpy()
    assert (left[n:] == 0x5A).all(), f"{name}: a byte behind the LEFT bytes was written"
    return left[:n], st, launches


def table(db):
    got, tot = db.cooccur_read()
    assert (got["class_a"] < got["class_b"]).all()
    keys = list(zip(got["class_a"].tolist(), got["class_b"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and (got["reads"] > 0).all()
    return dict(zip(keys, got["reads"].tolist())), tot


def run(db, name, case, max_wgs=0, full_ok=False, **knobs):
    """one case into a freshly emptied table, against the brute force; returns (witness, classes, the table)"""
    from kmcp_amd import lib
    configure(db, **knobs)
    cl = [case.classify(r) for r in range(case.n)]
    left, st, launches = launch(db, name, case, max_wgs=max_wgs)
    assert set(left.tolist()) <= {0, 1}
    if not full_ok:
        assert left.tolist() == [int(c == "left") for c in cl], f"{name}: the LEFT bytes"
        assert st["left_full"] == 0
    else:  # a read of the wave class may be LEFT as well ("table full"); no other class changes
        assert all(left[r] == int(c == "left") for r, c in enumerate(cl) if c != "wave"), f"{name}: the LEFT bytes"
    counted = [r for r in range(case.n) if cl[r] == "wave" and not left[r]]
    n_full = cl.count("wave") - len(counted)
    assert {k: st[k] for k in ("empty", "single", "wave", "left", "left_full")} == dict(empty=cl.count("empty"), single=cl.count("single"), wave=len(counted),
                                                                                        left=cl.count("left") + n_full, left_full=n_full), f"{name}: witness {st}"
    assert st["bad_segments"] == 0 and st["skipped"] == 0
    assert [(l.kernel, l.grid, l.block, l.cls) for l in launches] == ([(lib.K7_COOCCUR, st["grid"], 256, 3)] if case.n else []), name
    assert not case.n or 1 <= st["grid"] <= (case.n + 63) // 64
    want = case.brute(counted)
    got, tot = table(db)
    assert got == dict(want), f"{name}: {len(got)} pairs, expected {len(want)}"
    n_adds = sum(want.values())
    assert st["pairs"] == n_adds == sum(len(case.targets[r]) * (len(case.targets[r]) - 1) // 2 for r in counted)
    # every add went somewhere: to a workgroup's table (and from there to global memory in at most as many adds) or straight to global memory
    direct = n_adds - st["lds_adds"]
    assert 0 <= direct <= st["global_adds"] <= n_adds and st["spilled_adds"] == (direct if st["slots"] else 0)
    assert st["claimed"] == tot["keys"] >= len(want) and (full_ok or tot["keys"] == len(want))  # (a read that is LEFT keeps the keys it reserved)
    assert tot == dict(multi_reads=len(counted), device_adds=n_adds, host_adds=0, left_full=n_full, host_reads=0, skipped_launches=0,
                       table_slots=knobs.get("table_slots", 1 << 12), keys=tot["keys"], rebuilds=0), f"{name}: totals {tot}"
    return st, cl, got, left


def mixed(n_reads, seed):
    """reads of every class side by side"""
    rng = np.random.default_rng(seed)
    segs, nk = [], []
    for r in range(n_reads):
        kind = r % 6
        if kind == 0:
            segs.append(np.zeros(0, dtype=np.uint32))
        elif kind == 1:
            segs.append(cols_of([int(rng.integers(0, 200))] * int(rng.integers(1, 9)), rng))
        elif kind == 5 and r % 30 == 5:
            segs.append(cols_of(np.tile(rng.permutation(200)[:2], 33)[:65], rng))  # 65 pairs, two targets: LEFT
        else:
            m = int(rng.choice([2, 3, 5, 9, 17]))
            segs.append(cols_of(rng.choice(rng.permutation(40)[:m], size=m + int(rng.integers(0, 4))), rng))  # repeats: chunks of one target
        nk.append(int(rng.choice([130, 130, 130, FINAL_N, FINAL_N + 1])))
    return Case(segs, nk=nk)


# ---- the cases ----
def test_no_reads_and_one_empty_read(db):
    st, _, got, _ = run(db, "0 reads", Case([]))
    assert got == {} and st["grid"] == 0
    st, cl, got, _ = run(db, "one empty read", Case([np.zeros(0, dtype=np.uint32)]))
    assert cl == ["empty"] and got == {} and st["pairs"] == st["claimed"] == 0


def test_a_single_target_read_of_3000_pairs(db):
    st, cl, got, _ = run(db, "single", Case([cols_of([11] * 3000)]))
    assert cl == ["single"] and got == {} and st["claimed"] == 0


def test_two_targets_in_two_pairs(db):
    _, cl, got, _ = run(db, "two", Case([cols_of([7, 3])]))
    assert cl == ["wave"] and got == {(3, 7): 1}


def test_64_pairs_of_64_distinct_targets(db):
    rng = np.random.default_rng(1)
    st, cl, got, _ = run(db, "64 distinct", Case([cols_of(rng.permutation(200)[:64], rng)]))
    assert cl == ["wave"] and st["pairs"] == 2016 == len(got) and set(got.values()) == {1}


def test_64_pairs_alternating_between_two_classes(db):
    st, cl, got, _ = run(db, "aba", Case([cols_of([4, 5] * 32)]))
    assert cl == ["wave"] and got == {(4, 5): 1} and st["pairs"] == 1


def test_65_pairs_with_two_targets_and_too_many_kmers_are_left(db):
    _, cl, got, _ = run(db, "65", Case([cols_of([4, 5] * 32 + [4])]))
    assert cl == ["left"] and got == {}
    _, cl, got, _ = run(db, "final_n", Case([cols_of([4, 5]), cols_of([4, 5]), cols_of([6] * 3)], nk=[FINAL_N + 1, FINAL_N, FINAL_N + 1]))
    assert cl == ["left", "wave", "left"] and got == {(4, 5): 1}
    _, cl, got, _ = run(db, "above K3_WG_CAP", Case([cols_of([9] * (WG_CAP + 1))]))
    assert cl == ["left"] and got == {}


@pytest.mark.parametrize("n_reads", [16, 17, 64, 65])
def test_read_counts_at_the_wave_and_workgroup_edges(db, n_reads):
    st, cl, got, _ = run(db, f"{n_reads} reads", mixed(n_reads, seed=n_reads))
    assert "wave" in cl and got and st["grid"] == (n_reads + 63) // 64


def test_1000_reads_on_one_workgroup_take_grid_stride_rounds(db):
    case = mixed(1000, seed=77)
    st, cl, got, _ = run(db, "1 workgroup", case, max_wgs=1)
    assert st["grid"] == 1 and {"empty", "single", "wave", "left"} == set(cl)
    st2, _, got2, _ = run(db, "all workgroups", case)
    assert st2["grid"] == 16 and got2 == got  # the same inputs, another grid: the same table


def test_a_hot_pair_adds_per_workgroup_not_per_read(db):
    n = 4096
    case = Case([cols_of([50, 20])] * n)
    st, _, got, _ = run(db, "hot pair", case)
    assert got == {(20, 50): n}
    assert st["lds_adds"] == n and st["spilled_adds"] == 0 and 0 < st["global_adds"] <= st["grid"] and st["claimed"] == 1, st
    st, _, got, _ = run(db, "hot pair, no LDS table", case, slots=0)
    assert got == {(20, 50): n}
    assert st["slots"] == 0 and st["lds_adds"] == 0 and st["global_adds"] == n and st["spilled_adds"] == 0 and st["claimed"] == 1, st


def test_more_pairs_in_a_workgroup_than_lds_slots_spill_and_count_the_same(db):
    rng = np.random.default_rng(9)
    case = Case([cols_of(rng.permutation(200)[:12], rng) for _ in range(40)] + [cols_of([1, 2])] * 30)
    st, _, got, _ = run(db, "2 slots", case, slots=2, table_slots=1 << 15)
    assert st["slots"] == 2 and st["spilled_adds"] > 0 and st["lds_adds"] > 0
    st0, _, got0, _ = run(db, "no table", case, slots=0, table_slots=1 << 15)
    assert st0["slots"] == 0 and st0["lds_adds"] == 0 and got0 == got
    std, _, gotd, _ = run(db, "default table", case, table_slots=1 << 15)  # (2 640 pairs in the first workgroup: more than 2 048 slots too)
    assert std["slots"] == 2048 and 0 < std["spilled_adds"] < st["spilled_adds"] and gotd == got
    # 31 pairs in 2 048 slots: none is past the table
    few = Case([cols_of(rng.permutation(200)[:5], rng) for _ in range(3)] + [cols_of([1, 2])] * 30)
    stf, _, _, _ = run(db, "default table, few pairs", few)
    assert stf["spilled_adds"] == 0 and stf["lds_adds"] == stf["pairs"] == 60


def test_a_full_table_counts_a_read_completely_or_leaves_it(db):
    """8 slots, reads of 5 distinct targets (10 pairs each): whichever reads do not fit are LEFT whole.  run() has compared the table with
    the brute force over exactly the reads with left == 0; here: some are left, and device counts + the left reads' = the total"""
    rng = np.random.default_rng(4)
    case = Case([cols_of(rng.permutation(30)[:5], rng) for _ in range(200)] + [cols_of([1, 2])] * 8)
    for slots in (None, 0):
        st, cl, got, left = run(db, "8 slots", case, table_slots=8, full_ok=True, slots=slots)
        assert st["left_full"] > 0 and set(cl) == {"wave"}
        total = Counter(got)
        total.update(case.brute([r for r in range(case.n) if left[r]]))
        assert total == case.brute(range(case.n))
        _, tot = db.cooccur_read()
        assert tot["keys"] <= 8 and tot["left_full"] == st["left_full"] == int(left.sum())


def test_the_overflow_guard_skips_two_calls_accumulate_and_reset_zeroes(db):
    a, b = mixed(100, seed=21), mixed(37, seed=22)
    _, cla, _, _ = run(db, "first call", a)
    launch(db, "second call", b)
    clb = [b.classify(r) for r in range(b.n)]
    want = a.brute([r for r in range(a.n) if cla[r] == "wave"]) + b.brute([r for r in range(b.n) if clb[r] == "wave"])
    before, tot = table(db)
    assert before == dict(want) and tot["multi_reads"] == cla.count("wave") + clb.count("wave")
    # a hit counter above the capacity: the batch will be run again, nothing is counted now
    left, st, _ = launch(db, "guard", a, hits=(1001, 1000))
    assert st["skipped"] == 1 and not any(st[k] for k in ("empty", "single", "wave", "left", "pairs", "lds_adds", "global_adds", "claimed"))
    after, tot2 = table(db)
    assert after == before and tot2 == dict(tot, skipped_launches=1)  # ... and the handle remembers that it skipped one
    # at the capacity it runs
    _, st, _ = launch(db, "guard", a, hits=(1000, 1000))
    assert st["skipped"] == 0 and st["pairs"] > 0
    db.cooccur_reset()
    zero, tot3 = table(db)
    assert zero == {} and not any(v for k, v in tot3.items() if k != "table_slots")


def test_the_same_inputs_twice_give_the_same_sorted_result(db):
    case = mixed(500, seed=5)
    configure(db)
    launch(db, "first", case)
    a, _ = db.cooccur_read()
    configure(db)
    launch(db, "second", case)
    b, _ = db.cooccur_read()
    assert len(a) > 0 and a.tobytes() == b.tobytes()


def test_the_stage_off_and_bad_sizes(db):
    import torch

    from kmcp_amd.lib import KmcpGpuError
    z = torch.zeros(8, dtype=torch.int64, device=torch.device("cuda", 0))
    db.set_cooccur()
    st, launches = db.last_cooccur()
    assert launches == [] and not any(st.values())
    with pytest.raises(KmcpGpuError, match="stage is off"):
        db.cooccur_device(z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), 1, FINAL_N, z.data_ptr())
    with pytest.raises(KmcpGpuError, match="stage is off"):
        db.cooccur_read()
    with pytest.raises(KmcpGpuError, match="power of two"):
        db.set_cooccur(TARGET, table_slots=12)
    os.environ["KMCPG_COOCCUR_SLOTS"] = "48"
    try:
        with pytest.raises(KmcpGpuError, match="KMCPG_COOCCUR_SLOTS"):
            db.set_cooccur(TARGET)
    finally:
        os.environ.pop("KMCPG_COOCCUR_SLOTS")
