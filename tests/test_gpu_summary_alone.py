"""K5 alone (kmcp_amd/csrc/k5_summary.hip: k5_summary, the scan of k3_finalize.hip, k4_compact), driven through kmcpg_summarize_device on
pair lists the test lays out, against the plain restatement of merge-regions.go (tests/regions_reference.py window_summary) fed the way
the TSV route feeds it: every pair's qCov printed with "%.4f" and parsed back.  Compared: n and the 64-bit pattern of the score of every
window, the LEFT flag and what a LEFT record carries, the LEFT pairs and offsets (exactly, in order, and every word behind them), the
inputs (unchanged), and the witness: the class each window took.

The table: three columns per target (its chunks)."""
import numpy as np
import pytest

from tests import k3_cases as K
from tests import regions_reference as RR

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = -0x0123456789ABCDEF
N_COLS = 600
CAP = 64  # K5_CAP
DROP, KEEP, HOST = 0, 1, 2
LENGTHS = [0, 1, 2, 4, 5, 63, 64, 65, CAP, CAP + 1]
TARGET = (np.arange(N_COLS) // 3).astype(np.uint32)


@pytest.fixture(scope="module")
def db(oracle_lib, tmp_path_factory):
    from kmcp_amd import Database
    d = K.build_database(oracle_lib, tmp_path_factory.mktemp("k5db"), N_COLS, seed=901)
    with Database.open(d, device=0) as h:
        assert int(h.info.n_cols) == N_COLS
        h.set_profiling(1)
        h.set_specific(TARGET, None)
        yield h


# ---- segments: columns by pattern
def seg_one(rng, m):
    return (3 * 11 + rng.integers(0, 3, size=m)).astype(np.uint32)


def seg_distinct(rng, m):
    return (3 * rng.permutation(200)[:m] + rng.integers(0, 3, size=m)).astype(np.uint32)


def seg_aba(rng, m):
    """A B A ...: two targets by turns; from two pairs on"""
    return np.where(np.arange(m) % 2 == 0, 3 * 5 + 1, 3 * 9).astype(np.uint32)


def seg_late(rng, m):
    """one target, and the first (and only) rows of three others in the last places"""
    s = np.full(m, 3 * 20, dtype=np.uint32)
    tail = min(3, max(m - 1, 0))
    if tail:
        s[m - tail:] = 3 * np.array([150, 151, 152])[:tail] + 2
    return s


PATTERNS = {"one": seg_one, "distinct": seg_distinct, "aba": seg_aba, "late": seg_late}


class Case:
    def __init__(self, segs, verdicts=None, nk=None, counts=None, seed=1):
        rng = np.random.default_rng(seed)
        lens = np.array([len(s) for s in segs], dtype=np.int64)
        self.n = len(segs)
        self.offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        cols = np.concatenate(segs) if lens.sum() else np.zeros(0, dtype=np.uint32)
        self.nk = np.full(self.n, 130, dtype=np.int32) if nk is None else np.asarray(nk, dtype=np.int32)
        self.pairs = np.empty((len(cols), 2), dtype=np.uint32)
        self.pairs[:, 0] = cols
        self.pairs[:, 1] = rng.integers(1, np.repeat(self.nk, lens) + 1) if counts is None else counts
        self.verdict = np.full(self.n, KEEP, dtype=np.uint8) if verdicts is None else np.asarray(verdicts, dtype=np.uint8)


def reference(case):
    """per window (class, n, score) by the restatement over printed-and-parsed qCov; class: 'empty', 'single', 'wave', 'left'"""
    out = []
    for r in range(case.n):
        seg = case.pairs[int(case.offs[r]):int(case.offs[r + 1])]
        if len(seg) == 0 or case.verdict[r] == DROP:
            out.append(("empty", 0, 0.0))
            continue
        if case.verdict[r] == HOST:
            out.append(("left", len(seg), 0.0))
            continue
        rows = [(int(TARGET[c]), float("%.4f" % (int(m) / int(case.nk[r])))) for c, m in seg]
        n, score = RR.window_summary(rows)
        out.append(("single", 1, score) if n == 1 else ("wave", n, score) if len(seg) <= CAP else ("left", len(seg), 0.0))
    return out


def run(db, name, case, ref=None):
    import torch

    from kmcp_amd import lib
    dev = torch.device("cuda", 0)
    ref = ref or reference(case)
    n, cap = case.n, len(case.pairs)
    t_pairs = torch.from_numpy(case.pairs.view(np.int64).reshape(-1).copy()).to(dev)
    t_offs = torch.from_numpy(case.offs.view(np.int64).copy()).to(dev)
    t_nk = torch.from_numpy(case.nk).to(dev)
    t_v = torch.from_numpy(case.verdict).to(dev)
    t_out = torch.full((2 * (n + GUARD),), SENTINEL, dtype=torch.int64, device=dev)
    t_lp = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    t_lo = torch.full((n + 1 + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    db.summarize_device(t_pairs.data_ptr(), t_offs.data_ptr(), cap, t_v.data_ptr(), t_nk.data_ptr(), n, t_out.data_ptr(), t_lp.data_ptr(), cap, t_lo.data_ptr())
    torch.cuda.synchronize()
    st, launches = db.last_summary()
    assert np.array_equal(t_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), case.pairs), f"{name}: the pairs were changed"
    assert np.array_equal(t_offs.cpu().numpy().view(np.uint64), case.offs) and np.array_equal(t_nk.cpu().numpy(), case.nk), f"{name}: an input was changed"
    raw = t_out.cpu().numpy()
    assert (raw[2 * n:] == SENTINEL).all(), f"{name}: a word behind the summaries was written"
    got = raw[:2 * n].view(lib.SUMMARY_DTYPE)
    left_lens = np.zeros(n, dtype=np.int64)
    for r, (cls, cnt, score) in enumerate(ref):
        g = got[r]
        if cls == "left":
            want_flags = lib.SUMMARY_LEFT | (lib.SUMMARY_HOST if case.verdict[r] == HOST else 0)
            assert (int(g["n_targets"]), int(g["flags"])) == (cnt, want_flags), f"{name}: window {r}: {g}, expected LEFT with {cnt} pairs"
            left_lens[r] = cnt
        else:
            assert int(g["flags"]) == 0 and int(g["n_targets"]) == cnt, f"{name}: window {r} ({cls}): {g}, expected n = {cnt}"
            assert np.float64(g["score"]).view(np.uint64) == np.float64(score).view(np.uint64), f"{name}: window {r} ({cls}, n = {cnt}): score {g['score']!r}, expected {score!r}"
    want_lo = np.concatenate([np.concatenate([[0], np.cumsum(left_lens)]), np.full(GUARD, SENTINEL, dtype=np.int64)])
    got_lo = t_lo.cpu().numpy()
    bad = np.flatnonzero(got_lo != want_lo)
    assert len(bad) == 0, f"{name}: left_offs[{bad[0]}] is {got_lo[bad[0]]}, expected {want_lo[bad[0]]}"
    left_pairs = case.pairs[np.repeat(left_lens > 0, np.diff(case.offs.astype(np.int64)))]
    want_lp = np.full(cap + GUARD, SENTINEL, dtype=np.int64)
    want_lp[:len(left_pairs)] = np.ascontiguousarray(left_pairs).view(np.int64).reshape(-1)
    got_lp = t_lp.cpu().numpy()
    bad = np.flatnonzero(got_lp != want_lp)
    assert len(bad) == 0, f"{name}: left_pairs[{bad[0]}] is {got_lp[bad[0]]:#x}, expected {want_lp[bad[0]]:#x}; {len(bad)} differ"
    classes = [c for c, _, _ in ref]
    want_st = dict(single=classes.count("single"), wave=classes.count("wave"), left=classes.count("left"), empty=classes.count("empty"),
                   left_pairs=int(left_lens.sum()), bytes_d2h=0, bad_segments=0)
    assert st == want_st, f"{name}: witness {st}, expected {want_st}"
    assert st["single"] + st["wave"] + st["left"] + st["empty"] == n
    waves = (n + 63) // 64
    tiles = (n + 1 + 4095) // 4096
    want_l = [(lib.K5_SUMMARY, waves, 256, 3), (lib.K4_SCAN_TILES, tiles, 256, 0), (lib.K4_SCAN_SUMS, 1, 256, 0), (lib.K4_SCAN_ADD, tiles, 256, 0),
              (lib.K5_COMPACT, waves, 256, 3)] if n else []
    assert [(l.kernel, l.grid, l.block, l.cls) for l in launches] == want_l, name
    return ref


def mixed(n_windows, seed):
    rng = np.random.default_rng(seed)
    names = list(PATTERNS)
    segs, verd = [], []
    for r in range(n_windows):
        m = int(rng.choice(LENGTHS + [3, 7, 33])) if rng.random() < 0.8 else 0
        segs.append(PATTERNS[names[r % 4]](rng, m))
        verd.append(rng.choice([KEEP, KEEP, KEEP, DROP, HOST]))
    return Case(segs, verdicts=verd, seed=seed)


# ---- the cases ----
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_segment_lengths(db, pattern):
    rng = np.random.default_rng(3)
    case = Case([PATTERNS[pattern](rng, m) for m in LENGTHS])
    ref = run(db, f"lengths, {pattern}", case)
    classes = [c for c, _, _ in ref]
    if pattern == "one":
        assert classes == ["empty"] + ["single"] * (len(LENGTHS) - 1)
    else:  # several targets from two pairs on: by the wave up to the cap, LEFT above it
        assert classes == ["empty", "single"] + ["left" if m > CAP else "wave" for m in LENGTHS[2:]]
    if pattern == "distinct":
        assert [n for _, n, _ in ref][2:6] == [2, 4, 5, 63]
    if pattern == "late":
        assert [n for _, n, _ in ref][2:7] == [2, 4, 4, 4, 4]


# 16 windows = one wave: long segments (the whole wave reduces them and hands the result back to the window's lane group — the first, the
# last and inner groups among them), several-target segments the wave sums, one-target segments of a lane group and empty windows, side by side
ONE_WAVE = [("aba", 65), ("aba", 40), ("one", 3), ("distinct", 65), ("late", 5), ("one", 0), ("aba", 64), ("one", 130),
            ("distinct", 2), ("late", 65), ("one", 1), ("one", 65), ("distinct", 63), ("one", 64), ("late", 4), ("one", 65)]


def test_long_wave_and_single_segments_in_one_wave_then_a_wave_of_one_window(db):
    """17 windows: the wave above, and the batch's last window alone in a second wave beside 15 lane groups without a window — long
    (LEFT, single), by the wave, single and empty in turn"""
    rng = np.random.default_rng(17)
    first = [PATTERNS[p](rng, m) for p, m in ONE_WAVE]
    want = ["left", "wave", "single", "left", "wave", "empty", "wave", "single", "wave", "left", "single", "single", "wave", "single", "wave", "single"]
    for (p, m), cls in ((("aba", 65), "left"), (("one", 65), "single"), (("aba", 40), "wave"), (("one", 3), "single"), (("one", 0), "empty")):
        case = Case(first + [PATTERNS[p](rng, m)])
        assert case.n == 17
        ref = run(db, f"one wave and a window, the last one {m} pairs of '{p}'", case)
        assert [c for c, _, _ in ref] == want + [cls]


def test_a_single_target_of_any_length_stays_on_the_device(db):
    rng = np.random.default_rng(4)
    ref = run(db, "5 000 pairs of one target", Case([seg_one(rng, 5000), seg_one(rng, 1), seg_distinct(rng, 150)]))
    assert [c for c, _, _ in ref] == ["single", "single", "left"]


def test_verdicts(db):
    rng = np.random.default_rng(5)
    segs, verd = [], []
    for v in (DROP, HOST, KEEP):
        for pat in ("one", "aba", "distinct"):
            for m in (0, 1, 5, 65):
                segs.append(PATTERNS[pat](rng, m))
                verd.append(v)
    case = Case(segs, verdicts=verd)
    ref = run(db, "verdicts", case)
    lens = np.diff(case.offs.astype(np.int64))
    for r, (cls, _, _) in enumerate(ref):
        if verd[r] == DROP or lens[r] == 0:
            assert cls == "empty"
        elif verd[r] == HOST:
            assert cls == "left"


def test_printed_ties(db):
    """count / qkmers whose fifth decimal is a 5: 1/32 and 3/32 are exact ties (half to even on the digits), 341/400 and 343/400 lie
    beside one in binary; alone (single) and as the parts of a sum (wave)"""
    ties = [(32, 1), (32, 3), (400, 341), (400, 343)]
    segs, nk, counts = [], [], []
    for qk, c in ties:
        segs.append(np.array([3 * 7], dtype=np.uint32))
        nk.append(qk)
        counts.append(c)
    for qk, c in ties:
        segs.append(np.array([3 * 7, 3 * 8 + 1, 3 * 9 + 2], dtype=np.uint32))
        nk.append(qk)
        counts += [c, c, max(1, c - 1)]
    ref = run(db, "ties", Case(segs, nk=nk, counts=np.array(counts, dtype=np.uint32)))
    assert [s for _, _, s in ref[:4]] == [0.0312, 0.0938, 0.8525, 0.8575]


@pytest.mark.parametrize("n_windows", [1, 15, 16, 17, 63, 64, 65, 130])
def test_window_counts(db, n_windows):
    run(db, f"{n_windows} windows", mixed(n_windows, seed=n_windows))
    if n_windows in (1, 17):  # the last window has several targets, is LEFT, is empty
        rng = np.random.default_rng(8)
        run(db, f"{n_windows} windows, all by the wave", Case([seg_aba(rng, 40)] * n_windows))
        run(db, f"{n_windows} windows, all LEFT", Case([seg_distinct(rng, 70)] * n_windows))
        run(db, f"{n_windows} windows, all empty", Case([np.zeros(0, dtype=np.uint32)] * n_windows))


def test_the_stage_off_and_bad_arguments(db):
    import torch

    from kmcp_amd.lib import KmcpGpuError
    dev = torch.device("cuda", 0)
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    args = (z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 1, z.data_ptr())
    db.set_specific()
    try:
        st, launches = db.last_summary()
        assert launches == [] and not any(st.values())
        with pytest.raises(KmcpGpuError, match="stage is off"):
            db.summarize_device(*args)
    finally:
        db.set_specific(TARGET, None)
    with pytest.raises(KmcpGpuError, match="left_cap"):
        db.summarize_device(z.data_ptr(), z.data_ptr(), 4, z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 3, z.data_ptr())
