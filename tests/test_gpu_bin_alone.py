"""K11 alone (kmcp_amd/csrc/k11_bin.hip), driven through kmcpg_bin_device on K3-form lists and a plan the test lays out, against a brute
force in plain Python: a read's bin is the TaxId of the deepest common member of its whitelisted targets' ancestor sets (the virtual root,
TaxId 0, is in every set; an unknown TaxId has itself and the virtual root).  Every word of the output is checked, the words behind it,
the inputs (unchanged) and the witness.

The crafted taxonomy (TaxIds):  1 -> 10 -> (100 -> (1000, 1001), 101 -> 1002);  1 -> 11 -> 110;  1 -> 5000 -> (5001 -> ... -> 5047, 5100):
a chain of depth 48;  a second real root 2 -> 20;  7777 is in no node table.  No test provokes a fault: offsets outside the buffer are
refused by the kernel's own bounds (counted as bad, treated as empty), and the buffers are allocated in full all the same."""
import numpy as np
import pytest

from tests import k3_cases as K
from tests.binning_cases import preorder

pytestmark = pytest.mark.gpu

N_COLS = 64
GUARD = 16
FILL = 0xA5A5A5A5
NONE, LEFT, NO_NODE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF
FINAL_N = 1000
LDS_NODES = 2048  # common.hpp K11_LDS_NODES
EINVAL = -1

PARENT = {1: 0, 10: 1, 100: 10, 101: 10, 1000: 100, 1001: 100, 1002: 101, 11: 1, 110: 11, 2: 0, 20: 2, 7777: 0, 5000: 1, 5100: 5000}
for _i in range(1, 48):
    PARENT[5000 + _i] = 5000 + _i - 1
# the whitelisted columns: A has three chunks; E sits on an inner node, an ancestor of A's and B's TaxIds; U's TaxId is unknown
COL_TAXID = {0: 1000, 1: 1000, 2: 1000, 3: 1001, 4: 1002, 5: 110, 6: 100, 7: 20, 8: 7777, 9: 5047, 10: 5100}
A, B, C_, D, E, F, U, G, H = 0, 3, 4, 5, 6, 7, 8, 9, 10
OTHERS = np.arange(11, N_COLS)


def ancestors(t, parent):
    out = [t]
    while t != 0:
        t = parent[t]
        out.append(t)
    return out  # deepest first, ends with the virtual root 0


def brute_bin(cols, parent=PARENT):
    ids = sorted({COL_TAXID[int(c)] for c in cols if int(c) in COL_TAXID})
    if not ids:
        return NONE
    sets = [set(ancestors(t, parent)) for t in ids]
    for a in ancestors(ids[0], parent):
        if all(a in s for s in sets):
            return a
    raise AssertionError("no common ancestor")


class Plan:
    def __init__(self, extra=0):
        self.tree = dict(PARENT)
        for i in range(extra):  # leaves nobody matches: they only make the plan larger
            self.tree[90000 + i] = 1 if i % 2 else 5100
        self.parent, self.last, self.taxid, self.num = preorder(self.tree)
        self.node_of_column = np.full(N_COLS, NO_NODE, dtype=np.uint32)
        for c, t in COL_TAXID.items():
            self.node_of_column[c] = self.num[t]
        self.n = len(self.parent)

    def witness(self, segs, nk):
        """what the kernel's counters must say: reads without a bin / of one node / of several / LEFT, and the climb steps"""
        w = dict(no_bin=0, one=0, several=0, left=0, climb_steps=0)
        for cols, k in zip(segs, nk):
            if len(cols) and k > FINAL_N:
                w["left"] += 1
                continue
            nodes = [int(self.node_of_column[c]) for c in cols if self.node_of_column[c] != NO_NODE]
            if not nodes:
                w["no_bin"] += 1
                continue
            lo, hi = min(nodes), max(nodes)
            w["one" if lo == hi else "several"] += 1
            v = lo
            while self.last[v] < hi:
                v = int(self.parent[v])
                w["climb_steps"] += 1
        return w


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = K.build_database(oracle_lib, tmp_path_factory.mktemp("k11db"), N_COLS, seed=1101)
    with Database.open(d, device=0) as h:
        h.set_profiling(1)
        yield h


@pytest.fixture(scope="module")
def small():
    # the crafted tree is what the cases need: a chain of depth 48 below TaxId 1, two real roots and an unknown id under the virtual root
    assert len(ancestors(5047, PARENT)) == 48 + 2 and sorted(t for t, p in PARENT.items() if p == 0) == [1, 2, 7777]
    assert brute_bin([G, H]) == 5000 and brute_bin([A, B]) == 100 and brute_bin([E, 1]) == 100 and brute_bin([U]) == 7777
    assert brute_bin([U, A]) == 0 and brute_bin([F, A]) == 0 and brute_bin([D, B, G]) == 1 and brute_bin([12, 13]) == NONE
    p = Plan()
    assert p.n <= LDS_NODES
    return p


@pytest.fixture(scope="module")
def large():
    p = Plan(extra=3000)
    assert p.n > LDS_NODES
    return p


KINDS = ["none", "one_among", "chunks", "siblings", "anc_desc", "unknown_alone", "unknown_beside", "two_roots", "chain", "ends"]


def segment(kind, m, rng, plan):
    """m columns of the kind; the kinds that need two targets have one where m == 1"""
    if m == 0:
        return np.zeros(0, dtype=np.uint32)
    fill = rng.choice(OTHERS, size=m)
    need = {"none": [], "one_among": [C_], "chunks": [0, 1, 2], "siblings": [A, B], "anc_desc": [E, 1], "unknown_alone": [U], "unknown_beside": [U, A],
            "two_roots": [F, A], "chain": [G, H], "ends": [D, B, G]}[kind]
    if kind == "chunks":
        fill = rng.choice([0, 1, 2], size=m)
    if kind == "ends":
        # the holder of the largest node first, the holder of the smallest last: nothing in between may stand in for them
        by_node = sorted(need, key=lambda c: int(plan.node_of_column[c]))
        seg = fill.copy()
        seg[0] = by_node[-1]
        if m > 1:
            seg[-1] = by_node[0]
        if m > 2:
            seg[m // 2] = by_node[1]
        return seg.astype(np.uint32)
    seg = fill.copy()
    where = rng.choice(m, size=min(m, len(need)), replace=False)
    for w, c in zip(where, need):
        seg[w] = c
    return seg.astype(np.uint32)


def run(db, plan, name, segs, nk, overflow=None, pair_cap=None, offs=None, want=None, bad=0):
    """segs: one array of columns per read; nk: k-mers per read.  overflow: None = no hit counter given, False = a counter at the cap,
    True = above it.  offs / pair_cap / want: for the crafted bad offsets"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(segs)
    lens = np.array([len(s) for s in segs], dtype=np.int64)
    m = int(lens.sum())
    pairs = np.empty((m + 1, 2), dtype=np.uint32)
    pairs[:m, 0] = np.concatenate(segs) if m else []
    pairs[:, 1] = 1 + np.arange(m + 1) % 7
    pairs[m] = (0, 0)
    if offs is None:
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    cap = m if pair_cap is None else pair_cap
    t_pairs = torch.from_numpy(pairs.view(np.int64).reshape(-1).copy()).to(dev)
    t_offs = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    t_nk = torch.from_numpy(np.asarray(nk, dtype=np.int32).copy() if n else np.zeros(1, dtype=np.int32)).to(dev)
    t_bins = torch.from_numpy(np.full(n + GUARD, FILL, dtype=np.uint32).view(np.int32).copy()).to(dev)
    hit_cap = 1000
    t_hits = None if overflow is None else torch.tensor([hit_cap + (1 if overflow else 0)], dtype=torch.int64, device=dev)
    db.bin_device(t_pairs.data_ptr(), t_offs.data_ptr(), cap, t_nk.data_ptr(), n, FINAL_N, t_bins.data_ptr(), None if t_hits is None else t_hits.data_ptr(), hit_cap)
    torch.cuda.synchronize()
    st, launches = db.last_bins()
    assert np.array_equal(t_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), pairs), f"{name}: the pairs were changed"
    assert np.array_equal(t_offs.cpu().numpy().view(np.uint64), offs), f"{name}: the offsets were changed"
    got = t_bins.cpu().numpy().view(np.uint32)
    expect = np.full(n + GUARD, FILL, dtype=np.uint32)
    if overflow:
        wit = dict(no_bin=0, one=0, several=0, left=0, climb_steps=0)
    else:
        if want is None:
            want = [LEFT if len(s) and k > FINAL_N else brute_bin(s, plan.tree) for s, k in zip(segs, nk)]
            wit = plan.witness(segs, nk)
        else:
            wit = None
        expect[:n] = want
    wrong = np.flatnonzero(got != expect)
    assert len(wrong) == 0, f"{name}: bins[{wrong[0]}] is {got[wrong[0]]:#x}, expected {expect[wrong[0]]:#x}; {len(wrong)} differ"
    if wit is not None:
        assert {k: st[k] for k in wit} == wit, f"{name}: witness {st}, expected {wit}"
    assert st["skipped"] == (1 if overflow else 0) and st["bad_segments"] == bad, f"{name}: {st}"
    assert st["in_lds"] == (1 if plan.n <= LDS_NODES else 0), f"{name}: {st}, {plan.n} nodes"
    if n:
        from kmcp_amd import lib
        assert [l.kernel for l in launches] == [lib.K11_BIN] and launches[0].grid == st["grid"] and launches[0].block == 256, f"{name}: launches"
        assert db.last_k11_ms >= 0
    return st


def set_plan(db, plan):
    db.set_binning(plan.node_of_column, plan.parent, plan.last, plan.taxid)


@pytest.mark.parametrize("which", ["small", "large"])
def test_every_kind_at_every_segment_length(db, small, large, which):
    """segments of every length class of the walk (lane group up to 64 pairs, the wave above, K3's unordered ones above 4096), every kind;
    for the kind `ends` also a permutation of the same segment, which must give the same bin"""
    plan = small if which == "small" else large
    set_plan(db, plan)
    rng = np.random.default_rng(11)
    segs, ends = [], []
    for m in [0, 1, 2, 4, 5, 63, 64, 65, 128, 4096, 4097, 5000]:
        for kind in KINDS:
            segs.append(segment(kind, m, rng, plan))
            if kind == "ends":
                ends.append(len(segs) - 1)
                segs.append(rng.permutation(segs[-1]))
    nk = np.full(len(segs), 100)
    st = run(db, plan, f"lengths, {which} plan", segs, nk)
    assert st["several"] > 0 and st["one"] > 0 and st["no_bin"] > 0 and st["climb_steps"] >= 47
    # B, D and G hold the smallest, a middle and the largest node: G stands first and B last, and the permutation has the same bin
    num = [int(plan.node_of_column[c]) for c in (B, D, G)]
    assert num == sorted(num)
    long_ends = [i for i in ends if len(segs[i]) > 2]
    assert len(long_ends) == 9 and all(segs[i][0] == G and segs[i][-1] == B and brute_bin(segs[i]) == brute_bin(segs[i + 1]) == 1 for i in long_ends)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 64, 65, 1000])
def test_read_counts(db, small, n, monkeypatch):
    """the wave and workgroup edges; at 1000 reads three workgroups go round the grid-stride loop; every tenth read with pairs is above the
    -f bound and LEFT, every read without pairs is not"""
    monkeypatch.setenv("KMCPG_BIN_WGS", "3")
    set_plan(db, small)
    rng = np.random.default_rng(n)
    segs = [segment(KINDS[int(rng.integers(len(KINDS)))], int(rng.choice([0, 1, 2, 3, 7, 30, 70])), rng, small) for _ in range(n)]
    nk = np.where(np.arange(n) % 10 == 3, FINAL_N + 1, np.where(np.arange(n) % 10 == 4, FINAL_N, 50))
    st = run(db, small, f"n={n}", segs, nk)
    assert st["grid"] == min(3, (n + 63) // 64)
    if n == 1000:
        assert st["left"] > 50 and st["no_bin"] > 100 and st["several"] > 100
    monkeypatch.delenv("KMCPG_BIN_WGS")
    set_plan(db, small)
    if n:
        assert run(db, small, f"n={n}, the chip's grid", segs, nk)["grid"] == (n + 63) // 64


def test_reads_above_the_bound_are_left(db, small):
    set_plan(db, small)
    segs = [np.array([A], dtype=np.uint32), np.array([], dtype=np.uint32), np.array([A, B] * 40, dtype=np.uint32), np.array([12], dtype=np.uint32), np.array([A], dtype=np.uint32)]
    nk = [FINAL_N + 1, FINAL_N + 1, 2 * FINAL_N, FINAL_N + 1, FINAL_N]
    st = run(db, small, "LEFT", segs, nk, want=[LEFT, NONE, LEFT, LEFT, 1000])
    assert st["left"] == 3 and st["no_bin"] == 1 and st["one"] == 1


@pytest.mark.parametrize("n", [17, 1000])
def test_overflow_guard(db, small, n):
    """*d_n_hits > hit_cap: the batch will be run again — the bins keep their fill; a counter AT the cap is no overflow"""
    set_plan(db, small)
    rng = np.random.default_rng(5)
    segs = [segment(KINDS[i % len(KINDS)], 1 + i % 9, rng, small) for i in range(n)]
    nk = np.full(n, 10)
    run(db, small, f"counter at the cap, n={n}", segs, nk, overflow=False)
    run(db, small, f"overflow, n={n}", segs, nk, overflow=True)


def test_offsets_outside_the_buffer_are_bad_and_empty(db, small):
    set_plan(db, small)
    segs = [np.array([A, B, A], dtype=np.uint32), np.array([A] * 4, dtype=np.uint32), np.array([B] * 5, dtype=np.uint32)]
    # the last segment ends behind pair_cap
    st = run(db, small, "behind the cap", segs, [10, 10, 10], pair_cap=7, want=[100, 1000, NONE], bad=1)
    assert st["no_bin"] == 1
    # offsets that go down: the second read's segment ends before it starts; the third lies inside the buffer
    offs = np.array([0, 3, 2, 12], dtype=np.uint64)
    cols = np.concatenate(segs)
    run(db, small, "offsets that go down", segs, [10, 10, 10], offs=offs, want=[100, NONE, brute_bin(cols[2:12])], bad=1)


def test_refusals(db, small):
    import torch

    from kmcp_amd import lib
    z = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    p = z.data_ptr()

    def refused(fn, word):
        with pytest.raises(lib.KmcpGpuError) as e:
            fn()
        assert e.value.code == EINVAL and word in str(e.value), e.value

    set_plan(db, small)
    refused(lambda: db.bin_device(p, None, 4, p, 1, 10, p), "null")
    refused(lambda: db.bin_device(p, p, 4, p, 1, 10, None), "null")
    # a plan the climb could not rest on
    par, last = small.parent.copy(), small.last.copy()
    par[5] = 5
    refused(lambda: db.set_binning(small.node_of_column, par, small.last, small.taxid), "pre-order")
    last[0] -= 1
    refused(lambda: db.set_binning(small.node_of_column, small.parent, last, small.taxid), "node 0")
    cols = small.node_of_column.copy()
    cols[20] = small.n
    refused(lambda: db.set_binning(cols, small.parent, small.last, small.taxid), "node_of_column[20]")
    refused(lambda: db.set_binning(small.node_of_column[:-1], small.parent, small.last, small.taxid), "n_cols")
    # the refused calls left the plan in place; switched off, the stage says so
    run(db, small, "after the refusals", [np.array([A, B], dtype=np.uint32)], [10])
    db.set_binning()
    refused(lambda: db.bin_device(p, p, 4, p, 1, 10, p), "kmcpg_set_binning")
