"""K10 alone (kmcp_amd/csrc/k10_left.hip: k10_left_mask, the scan of k3_finalize.hip, k4_compact, k10_left_offs), driven through
kmcpg_left_compact_device on K3-form lists the test lays out, against plain numpy: the mask byte of every read, the LEFT offsets and the
compacted pairs (exactly, in order, and every word behind them), the inputs (unchanged), and the witness words.

The reference: mask[r] = OR over the stages whose pointer is given of (left[s][r] != 0) << s; a read with mask != 0 keeps its segment,
every other read has an empty one."""
import numpy as np
import pytest

from tests import k3_cases as K

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = -0x0123456789ABCDEF
MASK_FILL = 0xA5
N_COLS = 64
EINVAL = -1  # KMCPG_EINVAL
SCAN_TILE = 4096  # k3_finalize.hip: SCAN_ITEMS * SCAN_THREADS; the scan runs over n + 1 words, so n = 4096 is the first to cross a tile


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = K.build_database(oracle_lib, tmp_path_factory.mktemp("k10db"), N_COLS, seed=1001)
    with Database.open(d, device=0) as h:
        h.set_profiling(1)
        yield h


class Case:
    """lens: the reads' segment lengths; left: three byte arrays (what the stages wrote); given: which of the three pointers are passed"""

    def __init__(self, lens, left, given=(True, True, True), seed=1):
        rng = np.random.default_rng(seed)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.n = len(self.lens)
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        m = int(self.lens.sum())
        self.pairs = np.empty((m, 2), dtype=np.uint32)
        self.pairs[:, 0] = rng.integers(0, N_COLS, size=m)
        self.pairs[:, 1] = np.arange(1, m + 1)  # every pair is its own: a pair that lands in the wrong place shows
        self.left = [np.asarray(l, dtype=np.uint8) for l in left]
        self.given = given

    def reference(self):
        mask = np.zeros(self.n, dtype=np.uint8)
        for s in range(3):
            if self.given[s]:
                mask |= ((self.left[s] != 0).astype(np.uint8) << s).astype(np.uint8)
        kept = np.where(mask != 0, self.lens, 0)
        offs = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
        pairs = self.pairs[np.repeat(mask != 0, self.lens)]
        return mask, offs, pairs


def run(db, name, case, overflow=None):
    """overflow: None = no hit counter given; False = a counter at the cap (no overflow); True = above it (the guard)"""
    import torch
    dev = torch.device("cuda", 0)
    n, cap = case.n, len(case.pairs)
    t_pairs = torch.from_numpy(np.concatenate([case.pairs.view(np.int64).reshape(-1), np.zeros(1, dtype=np.int64)])).to(dev)
    t_offs = torch.from_numpy(case.offs.view(np.int64).copy()).to(dev)
    t_left = [torch.from_numpy(l.copy()).to(dev) for l in case.left]
    t_mask = torch.full((n + GUARD,), MASK_FILL, dtype=torch.uint8, device=dev)
    t_lp = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    t_lo = torch.full((n + 1 + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    hit_cap = 1000
    t_hits = None if overflow is None else torch.tensor([hit_cap + (1 if overflow else 0)], dtype=torch.int64, device=dev)
    db.left_compact_device(t_pairs.data_ptr(), t_offs.data_ptr(), cap, n, *[t.data_ptr() if g else None for t, g in zip(t_left, case.given)],
                           None if t_hits is None else t_hits.data_ptr(), hit_cap, t_mask.data_ptr(), t_lp.data_ptr(), cap, t_lo.data_ptr())
    torch.cuda.synchronize()
    st, launches = db.last_stats()
    assert np.array_equal(t_pairs.cpu().numpy()[:cap].view(np.uint32).reshape(-1, 2), case.pairs), f"{name}: the pairs were changed"
    assert np.array_equal(t_offs.cpu().numpy().view(np.uint64), case.offs), f"{name}: the offsets were changed"
    for s in range(3):
        assert np.array_equal(t_left[s].cpu().numpy(), case.left[s]), f"{name}: the bytes of stage {s} were changed"
    mask, offs, pairs = case.reference()
    want_mask = np.full(n + GUARD, MASK_FILL, dtype=np.uint8)
    want_lo = np.full(n + 1 + GUARD, SENTINEL, dtype=np.int64)
    want_lp = np.full(cap + GUARD, SENTINEL, dtype=np.int64)
    if overflow:
        want_st = dict(matched_reads=0, left_reads=0, left_pairs=0, bad_segments=0, skipped=1)
    else:
        want_mask[:n] = mask
        want_lo[:n + 1] = offs
        want_lp[:len(pairs)] = np.ascontiguousarray(pairs).view(np.int64).reshape(-1)
        want_st = dict(matched_reads=int((case.lens > 0).sum()), left_reads=int((mask != 0).sum()), left_pairs=len(pairs), bad_segments=0, skipped=0)
    for what, got, want in (("mask", t_mask.cpu().numpy(), want_mask), ("left_offs", t_lo.cpu().numpy(), want_lo), ("left_pairs", t_lp.cpu().numpy(), want_lp)):
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"{name}: {what}[{bad[0]}] is {got[bad[0]]:#x}, expected {want[bad[0]]:#x}; {len(bad)} differ"
    assert {k: st[k] for k in want_st} == want_st, f"{name}: witness {st}, expected {want_st}"
    assert st["n_reads"] == 0 and st["kept_pairs"] == 0 and st["bytes_d2h"] == 0, f"{name}: {st}"
    from kmcp_amd import lib
    assert [l.kernel for l in launches] == [lib.K10_MASK, lib.K4_SCAN_TILES, lib.K4_SCAN_SUMS, lib.K4_SCAN_ADD, lib.K10_COMPACT, lib.K10_OFFS], f"{name}: launches"
    tiles = (n + 1 + SCAN_TILE - 1) // SCAN_TILE
    assert launches[1].grid == tiles and launches[0].grid == (n + 63) // 64, f"{name}: grids {[l.grid for l in launches]}"
    return st


def flags_of(kind, n, rng):
    if kind == "none":
        return [np.zeros(n, dtype=np.uint8)] * 3
    if kind == "all":
        return [np.ones(n, dtype=np.uint8)] * 3
    if kind == "alternating":
        return [(np.arange(n) % 2).astype(np.uint8), np.zeros(n, dtype=np.uint8), (np.arange(n) % 2).astype(np.uint8)]
    return [(rng.integers(0, 4, size=n) == 0).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8) for _ in range(3)]  # any non-zero byte


@pytest.mark.parametrize("kind", ["none", "all", "alternating", "random"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 64, 65, SCAN_TILE])
def test_sizes_and_flags(db, n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    lens = rng.integers(0, 6, size=n)
    st = run(db, f"n={n} {kind}", Case(lens, flags_of(kind, n, rng), seed=n))
    assert (n + 1 + SCAN_TILE - 1) // SCAN_TILE == (2 if n == SCAN_TILE else 1)
    if kind == "none":
        assert st["left_reads"] == 0 and st["left_pairs"] == 0
    if kind == "all":
        assert st["left_reads"] == n and st["left_pairs"] == int(lens.sum())


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_one_stage_only_sets_its_bit(db, stage):
    n = 40
    lens = np.full(n, 3)
    left = [np.zeros(n, dtype=np.uint8) for _ in range(3)]
    left[stage][[0, 7, 16, 39]] = 1
    case = Case(lens, left)
    run(db, f"stage {stage} only", case)
    mask = case.reference()[0]
    assert set(np.unique(mask)) == {0, 1 << stage}


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_a_null_stage_is_not_looked_at(db, stage):
    n = 33
    left = [np.zeros(n, dtype=np.uint8) for _ in range(3)]
    left[stage][:] = 1  # the array says LEFT, the pointer is not passed
    other = (stage + 1) % 3
    left[other][5] = 1
    given = tuple(s != stage for s in range(3))
    st = run(db, f"stage {stage} NULL", Case(np.full(n, 2), left, given))
    assert st["left_reads"] == 1 and st["left_pairs"] == 2


def test_no_stage_given_leaves_nothing(db):
    n = 20
    st = run(db, "all NULL", Case(np.full(n, 4), [np.ones(n, dtype=np.uint8)] * 3, (False, False, False)))
    assert st["left_reads"] == 0


def test_segment_lengths(db):
    """LEFT reads of every length class of the compaction (lane group up to 64 pairs, the wave above) between reads that are not LEFT"""
    lens = []
    flags = []
    for m in [0, 1, 64, 65, 4096, 4097]:
        lens += [m, m, 3]
        flags += [1, 0, 0]
    left = [np.array(flags, dtype=np.uint8), np.zeros(len(flags), dtype=np.uint8), np.zeros(len(flags), dtype=np.uint8)]
    st = run(db, "lengths", Case(lens, left))
    assert st["left_reads"] == 6 and st["left_pairs"] == 0 + 1 + 64 + 65 + 4096 + 4097


@pytest.mark.parametrize("where", ["first", "last", "both"])
@pytest.mark.parametrize("n", [1, 16, 17, 65])
def test_left_read_at_the_ends(db, n, where):
    f = np.zeros(n, dtype=np.uint8)
    if where in ("first", "both"):
        f[0] = 1
    if where in ("last", "both"):
        f[n - 1] = 1
    lens = np.full(n, 70)  # above GROUP_CAP: the wave copies them
    lens[n // 2] = 5
    run(db, f"{where} of {n}", Case(lens, [np.zeros(n, dtype=np.uint8), f, np.zeros(n, dtype=np.uint8)]))


def test_no_pairs_at_all(db):
    run(db, "empty batch of reads", Case(np.zeros(18, dtype=np.int64), [np.ones(18, dtype=np.uint8)] * 3))


@pytest.mark.parametrize("n", [17, SCAN_TILE])
def test_overflow_guard(db, n):
    """*d_n_hits > hit_cap: the batch will be run again — mask, offsets and pairs keep their fill; a counter AT the cap is no overflow"""
    rng = np.random.default_rng(5)
    case = Case(rng.integers(0, 6, size=n), flags_of("all", n, rng))
    run(db, f"counter at the cap, n={n}", case, overflow=False)
    run(db, f"overflow, n={n}", case, overflow=True)


def test_refusals(db):
    import torch

    from kmcp_amd import lib
    z = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    p = z.data_ptr()
    with pytest.raises(lib.KmcpGpuError) as e:
        db.left_compact_device(p, p, 4, 1, p, p, p, None, 0, p, p, 3, p)
    assert e.value.code == EINVAL and "left_cap" in str(e.value)
    with pytest.raises(lib.KmcpGpuError) as e:
        db.left_compact_device(p, None, 4, 1, p, p, p, None, 0, p, p, 4, p)
    assert e.value.code == EINVAL
