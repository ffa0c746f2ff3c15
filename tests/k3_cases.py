"""Crafted hit lists for K3 (kmcp_amd/csrc/k3_finalize.hip) and a plain numpy restatement of what K3 and the host half behind it make
of a hit list.  No GPU, numpy only: tests/test_k3_reference_cpu.py holds the restatement against the host half (kmcpg_finalize,
kmcpg_finalize_grouped), tests/test_gpu_k3_alone.py holds the kernels against the restatement.

The databases built here exist for their column sizes alone (a column is a list of random hashes): many columns of one size, sizes in
the ratios 1 : 2 : 3, the sizes 32 / 64 / 96 (scores of k/32), and sizes s = 21 c - 120 (equal jacc 1/20 for different counts c of a
read of 120 k-mers).  Every case builder takes the sizes as the opened database reports them (sizes_of), never as they were planned.

A case is (hits, n_hits_word, hit_cap, nk, n_reads): `hits` holds hit_cap entries of lib.HIT_DTYPE, the count word may be smaller
(the entries behind it are well-formed hits that must not be looked at) or larger (only hit_cap are looked at).  Inside a case (read,
column) is unique, 1 <= count <= min(nk[read], size[column]) and nk >= 1: every score is inside the contract of k3_keys.hpp and fixed4."""
from collections import namedtuple
from math import gcd

import numpy as np

from kmcp_amd.lib import HIT_DTYPE

Case = namedtuple("Case", "hits n_hits_word hit_cap nk n_reads")
Ref = namedtuple("Ref", "offs pairs bad classes mixed_runs reordered")

NONE = 0xFFFFFFFF                      # read == col == NONE: K2's tombstone
WAVE_CAP, WG_CAP = 512, 4096           # K3_WAVE_CAP, K3_WG_CAP
SCAN_TILE = 4096                       # counters per tile of the scan
NK = 120                               # NumKmers of most reads (few distinct values: the host keeps an FPR row per value)
JACC_SIZES = {10: 90, 11: 111, 12: 132, 20: 300}  # count -> size with count / (120 + size - count) == 1/20
MODES = dict(qcov=dict(sort_by=0), tcov=dict(sort_by=1), jacc=dict(sort_by=2), nosort=dict(do_not_sort=1))
EDGE_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 4095, 4096, 4097)


def params_for(mode, min_tcov=0.0):
    """only -T and the order act"""
    from kmcp_amd import default_params
    return default_params(min_qcov=0.0, min_matched=1, max_fpr=1.0, min_qlen=0, top_n_scores=0, min_tcov=float(min_tcov), **MODES[mode])


# ---- databases ----
def plan_sizes(n_cols, seed):
    """the sizes asked for: fixed families in proportion to n_cols, the rest random in 8 .. 400, in random order"""
    rng = np.random.default_rng(seed)
    u = n_cols // 42
    fam = [100] * (6 * u) + [200] * (3 * u) + [300] * (3 * u) + [32, 64, 96] * (3 * u // 2) + [90, 111, 132, 81] * u
    rest = rng.integers(8, 401, size=n_cols - len(fam)).tolist()
    return rng.permutation(np.array(fam + rest, dtype=np.int64))


def build_database(O, out_dir, n_cols, seed):
    """O = the oracle module; returns the database directory"""
    rng = np.random.default_rng(seed + 1)
    cols = []
    for i, n in enumerate(plan_sizes(n_cols, seed)):
        h = np.unique(rng.integers(1, 2**63, size=int(n), dtype=np.int64).astype(np.uint64))
        cols.append((f"s{seed}c{i:04d}", int(n), 0, 1, h))
    return O.build_db(str(out_dir), O.sketch_cfg(k=21), cols, num_hashes=1, fpr=0.3, threads=8, block_size=512)


def sizes_of(db):
    return np.array([db.col_info(c)[3] for c in range(int(db.info.n_cols))], dtype=np.uint64)


# ---- building blocks ----
def _pack(read, col, count):
    h = np.empty(len(read), dtype=HIT_DTYPE)
    h["read"], h["col"], h["count"] = read, col, count
    return h


def _counts(rng, read, col, sizes, nk):
    cmax = np.minimum(nk[read].astype(np.int64), sizes[col].astype(np.int64))
    return 1 + rng.integers(0, 1 << 30, size=len(read)) % cmax


def _fill(seg_lens, sizes, nk, rng, permute_above=3):
    """seg_lens[r] hits for read r, the reads' hits side by side in read order (as K2 emits them); distinct columns inside a read: a
    random draw for reads of more than permute_above hits, start + i * stride (stride coprime to the number of columns) for the others"""
    seg_lens = np.asarray(seg_lens, dtype=np.int64)
    n_reads, n_cols = len(seg_lens), len(sizes)
    assert seg_lens.max(initial=0) <= n_cols
    offs = np.concatenate([[0], np.cumsum(seg_lens)])
    read = np.repeat(np.arange(n_reads, dtype=np.int64), seg_lens)
    within = np.arange(int(offs[-1]), dtype=np.int64) - offs[read]
    strides = np.array([s for s in range(1, n_cols) if gcd(s, n_cols) == 1], dtype=np.int64)
    col = (rng.integers(0, n_cols, size=n_reads)[read] + within * rng.choice(strides, size=n_reads)[read]) % n_cols
    for r in np.flatnonzero(seg_lens > permute_above):
        col[offs[r]:offs[r + 1]] = rng.permutation(n_cols)[:seg_lens[r]]
    return _pack(read, col, _counts(rng, read, col, sizes, nk))


def reorder(hits, how, rng):
    """hits in runs by ascending read -> `how`: runs | shuffled | round_robin (every run one hit long, neighbours differ) | descending"""
    read = hits["read"].astype(np.int64)
    if how == "runs":
        return hits
    if how == "shuffled":
        return hits[rng.permutation(len(hits))]
    if how == "descending":
        return hits[np.argsort(-read, kind="stable")]
    assert how == "round_robin"
    within = np.arange(len(hits)) - np.searchsorted(read, read, side="left")
    return hits[np.lexsort((read, within))]


def _case(hits, nk, n_reads, slack=0, rng=None, sizes=None, word=None):
    """hit_cap = the hits + `slack` well-formed hits behind the count word that must not be looked at"""
    if slack:
        junk_read = rng.integers(0, n_reads, size=slack)
        junk_col = rng.integers(0, len(sizes), size=slack)
        hits = np.concatenate([hits, _pack(junk_read, junk_col, _counts(rng, junk_read, junk_col, sizes, nk))])
    n = len(hits) - slack
    return Case(np.ascontiguousarray(hits), n if word is None else word, len(hits), np.ascontiguousarray(nk, dtype=np.int32), int(n_reads))


def _nk(n_reads, rng):
    nk = np.full(n_reads, NK, dtype=np.int32)
    nk[rng.random(n_reads) < 0.1] = 77
    return nk


# ---- case 1: class edges ----
def class_edges(sizes, order="runs", last_empty=False, seed=1, k32=False, big_nk=False):
    """77 reads with every length of EDGE_LENGTHS (zeros between some of them) and short reads around them.  k32: counts on columns of
    32 / 64 / 96 k-mers give tcov 1/32 and 3/32; big_nk: one read of 30 000 k-mers, whose qcov differs beyond the fourth decimal"""
    rng = np.random.default_rng(seed)
    n_reads = 77
    lens = rng.integers(0, 6, size=n_reads)
    for i, m in enumerate(EDGE_LENGTHS):
        lens[3 * i + 1] = m
        if i % 2:
            lens[3 * i + 2] = 0
    lens[76], lens[75] = (0, 4) if last_empty else (7, 0)
    nk = _nk(n_reads, rng)
    if big_nk:
        nk[3 * EDGE_LENGTHS.index(257) + 1] = 30000
    hits = _fill(lens, sizes, nk, rng)
    if k32:
        s = sizes[hits["col"]].astype(np.int64)
        pick = np.isin(s, (32, 64, 96)) & (rng.random(len(hits)) < 0.7)
        hits["count"][pick] = (s[pick] // 32) * rng.choice([1, 3], size=int(pick.sum()))
        # reads of two or three matches whose scores all differ: no run of equal printed score
        small = np.flatnonzero(np.isin(lens[hits["read"]], (2, 3)))
        hits["count"][small] = 1 + (small - np.searchsorted(hits["read"], hits["read"][small], side="left")) * 3
        assert (hits["count"] <= np.minimum(nk[hits["read"]], sizes[hits["col"]].astype(np.int64))).all()
    return _case(reorder(hits, order, rng), nk, n_reads, slack=5, rng=rng, sizes=sizes)


# ---- case 2: runs and lanes ----
def runs_and_lanes(sizes, seed=2):
    """A hit list laid out by position (lane = position % 64): runs that fill a wave, cross into the next, start or end at lane 63, and runs
    broken by a tombstone, a hit of a read / column that does not exist, or a hit of the same read that fails -T — each in the middle
    of a wave, at lane 0 and at lane 63.  Returns (case, positions of the -T breakers)."""
    rng = np.random.default_rng(seed)
    n_cols = len(sizes)
    big = np.flatnonzero(sizes == 300)
    reads, kinds = [], []  # per position: the read, and what stands there ("hit" or a breaker)
    fresh = [0]

    def new_read():
        fresh[0] += 1
        return fresh[0] - 1

    def run(r, n, kind="hit"):
        reads.extend([r] * n)
        kinds.extend([kind] * n)

    def pad_to(lane):  # one-hit runs of new reads up to the lane
        while len(reads) % 64 != lane:
            run(new_read(), 1)

    run(new_read(), 64)                      # fills wave 0 exactly
    run(new_read(), 1)
    run(new_read(), 64)                      # lanes 1 .. 63 and lane 0 of the next wave
    run(new_read(), 65)
    run(new_read(), 130)
    pad_to(63)
    run(new_read(), 10)                      # the first hit at lane 63
    pad_to(50)
    run(new_read(), 14)                      # ends at lane 63
    pad_to(60)
    run(new_read(), 3)
    assert len(reads) % 64 == 63
    run(new_read(), 1)                       # one hit at lane 63 between two other reads
    run(new_read(), 5)
    for kind in ("tomb", "bad_read", "bad_col", "bad_read_max", "bad_col_max", "fails_T"):
        for lane in (20, 0, 63):
            pad_to((lane - 5) % 64)
            r = new_read()
            run(r, 5)
            assert len(reads) % 64 == lane
            run(r, 1, kind)
            run(r, 5)
    pad_to(37)                               # the last wave is partial
    n_reads = fresh[0] + 2                   # (the last two reads have no hit)
    read = np.array(reads, dtype=np.int64)
    kinds = np.array(kinds)
    nk = _nk(n_reads, rng)
    col = np.zeros(len(read), dtype=np.int64)
    for r in np.unique(read):                # distinct columns inside a read; the -T breaker on a column of 300 k-mers
        at = np.flatnonzero(read == r)
        col[at] = rng.permutation(n_cols)[:len(at)]
        for i in at[kinds[at] == "fails_T"]:
            col[i] = next(c for c in big if c not in col[at])
    count = _counts(rng, read, col, sizes, nk)
    count[kinds == "fails_T"] = 1            # 1 / 300: below every -T the case is run with
    hits = _pack(read, col, count)
    for kind, (r, c) in dict(tomb=(NONE, NONE), bad_read=(n_reads + 3, None), bad_col=(None, n_cols), bad_read_max=(NONE, None),
                             bad_col_max=(None, NONE)).items():
        if r is not None:
            hits["read"][kinds == kind] = r
        if c is not None:
            hits["col"][kinds == kind] = c
    return _case(hits, nk, n_reads), np.flatnonzero(kinds == "fails_T")


def prefixes(case):
    """the list cut to 1, 63, 64, 65 and 127 hits: by the count word (the hits behind it are not looked at) and by hit_cap (the word says more)"""
    out = {}
    for n in (1, 63, 64, 65, 127):
        out[f"word{n}"] = Case(case.hits, n, case.hit_cap, case.nk, case.n_reads)
        out[f"cap{n}"] = Case(np.ascontiguousarray(case.hits[:n]), n + 7, n, case.nk, case.n_reads)
    return out


def tcov_quantile(case, sizes, q):
    """the -T that drops about the fraction q of the well-formed hits"""
    h = case.hits[:min(case.n_hits_word, case.hit_cap)]
    ok = (h["read"] < case.n_reads) & (h["col"] < len(sizes))
    return float(np.quantile(h["count"][ok].astype(np.float64) / sizes[h["col"][ok]].astype(np.float64), q))


# ---- case 3: ties and the -T boundary ----
def _tie_counts(rng, col, sizes):
    """counts from a handful of values per column size: c / size in {1/32, 3/32, 1/20, 1/10, 1/4, 1/3}, the counts on either side of
    size / 3, the count that gives jacc 1/20 at 120 k-mers, and 4, 5, 10 whatever the size"""
    out = np.empty(len(col), dtype=np.int64)
    opts = {}
    for i, c in enumerate(col):
        s = int(sizes[c])
        if s not in opts:
            o = {4, 5, 10, s // 3 - 1, s // 3 + 1}
            o |= {num * s // den for num, den in ((1, 32), (3, 32), (1, 20), (1, 10), (1, 4), (1, 3)) if num * s % den == 0}
            o |= {c2 for c2, s2 in JACC_SIZES.items() if s2 == s}
            opts[s] = np.array(sorted(x for x in o if 1 <= x <= min(NK, s)), dtype=np.int64)
        out[i] = rng.choice(opts[s])
    return out


def ties(sizes, seed=3):
    """one read per tie family, segment lengths on both sides of 512; all reads have 120 k-mers"""
    rng = np.random.default_rng(seed)
    pool = lambda *ss: np.flatnonzero(np.isin(sizes, ss))  # noqa: E731
    fam = dict(tcov=pool(100, 200, 300), k32=pool(32, 64, 96), jacc=pool(90, 111, 132, 300), edge=pool(96, 300, 90, 111, 132, 100, 81, 200))
    fam["all"] = pool(100, 200, 300, 32, 64, 96, 90, 111, 132, 81)
    plan = [("tcov", 300), ("tcov", 700), ("k32", 300), ("jacc", 300), ("edge", 300), ("edge", 513), ("all", 511), ("all", 512), ("all", 513),
            ("all", 700), ("all", 2000), ("edge", 2)]
    read, col = [], []
    for r, (f, m) in enumerate(plan):
        assert len(fam[f]) >= m, (f, len(fam[f]), m)
        read.append(np.full(m, r))
        col.append(rng.permutation(fam[f])[:m])
    read, col = np.concatenate(read), np.concatenate(col)
    nk = np.full(len(plan), NK, dtype=np.int32)
    hits = _pack(read, col, _tie_counts(rng, col, sizes))
    return _case(reorder(hits, "shuffled", rng), nk, len(plan))


def _variety(group_keys, vary):
    """neighbours (once sorted) that agree in every group key and differ in `vary`: > 0 iff some group holds two values of it"""
    o = np.lexsort((vary,) + tuple(reversed(group_keys)))
    same = np.ones(max(len(o) - 1, 0), dtype=bool)
    for k in group_keys:
        same &= k[o][1:] == k[o][:-1]
    return int(np.count_nonzero(same & (vary[o][1:] != vary[o][:-1])))


def tie_census(case, sizes):
    """which kinds of ties a case holds (all hits well-formed)"""
    h = case.hits[:min(case.n_hits_word, case.hit_cap)]
    rd, cl, ct = h["read"].astype(np.int64), h["col"].astype(np.int64), h["count"].astype(np.int64)
    s = sizes[cl].astype(np.int64)
    c, sf, nh = ct.astype(np.float64), s.astype(np.float64), case.nk[rd].astype(np.float64)
    return dict(count_only=_variety((rd, ct), s), all_but_column=_variety((rd, ct, s), cl), tcov_other_count=_variety((rd, c / sf), ct),
                jacc_other_count=_variety((rd, c / (nh + sf - c)), ct), jacc_all_but_column=_variety((rd, c / (nh + sf - c), ct), cl))


# ---- case 4: many reads ----
def many_reads(sizes, n_reads, order="runs", seed=4):
    """sparse: one read in three has 1 to 3 hits; ~300 wave-class segments, more of them on either side of every tile edge of the scan;
    four workgroup-class segments and one above 4096 at the first and last tile edge, above read 524 288 and in the last window of 256"""
    rng = np.random.default_rng(seed + n_reads)
    lens = np.where(rng.random(n_reads) < 1 / 3, rng.integers(1, 4, size=n_reads), 0)
    lens[rng.integers(0, n_reads, size=300)] = rng.integers(2, 200, size=300)
    lens[rng.integers(0, n_reads, size=6)] = (509, 510, 511, 512, 512, 2)
    edges = np.arange(SCAN_TILE, n_reads, SCAN_TILE)
    for side in (edges - 1, edges, edges - 2):  # (counter n_reads is the bad-hit word's neighbour: tile edges are those of the reads)
        lens[side] = rng.integers(2, 40, size=len(side))
    cands = [SCAN_TILE - 1, SCAN_TILE, 524288 + 4097] + ([int(edges[-1]) - 1, int(edges[-1])] if len(edges) else [])
    cands += [n_reads - 3, n_reads - 100, n_reads // 2, n_reads // 3, n_reads // 5]
    spots = []
    for x in cands:
        if 0 <= x <= n_reads - 2 and x not in spots and len(spots) < 5:
            spots.append(x)
    large = [513, 4096, 2500, 4097, 1000]
    assert len(spots) == 5, spots
    lens[spots] = large
    lens[n_reads - 1] = 5
    nk = _nk(n_reads, rng)
    return _case(reorder(_fill(lens, sizes, nk, rng), order, rng), nk, n_reads, slack=3, rng=rng, sizes=sizes)


# ---- case 5: many hits ----
def many_hits(sizes, seed=5):
    """16384 x 256 + 3037 hits of 50 000 reads in runs by read: the count and scatter grids make a second trip whose last wave is partial"""
    rng = np.random.default_rng(seed)
    n_reads, total = 50000, 16384 * 256 + 3037
    lens = rng.integers(40, 128, size=n_reads)
    lens[rng.integers(0, n_reads, size=2000)] = 0
    some = rng.choice(n_reads, size=2000, replace=False)  # ... and these take what is missing
    lens[some] += (total - lens.sum()) // 2000
    lens[-1] += total - lens.sum()
    assert lens.min() >= 0 and lens.max() <= len(sizes) and lens.sum() == total and lens[-1] > 0 and total % 64
    nk = _nk(n_reads, rng)
    return _case(_fill(lens, sizes, nk, rng, permute_above=len(sizes)), nk, n_reads)


# ---- the plain restatement ----
def reference(hits, n, cap, nk, n_reads, sizes, params, bases=None):
    """What K3 + the host half make of a hit list -> Ref(offs[0 .. n_reads], pairs [m, 2] (column, count), bad, (segments of 2..512,
    513..4096, more), runs of equal printed score with several members in segments of at most 4096, segments of 2..4096 that the set
    order changes).  One lexsort over the batch, on the scores themselves."""
    sizes = np.asarray(sizes, dtype=np.uint64)
    n_cols = len(sizes)
    h = hits[:min(int(n), int(cap))]
    rd, cl, ct = h["read"].astype(np.int64), h["col"].astype(np.int64), h["count"].astype(np.int64)
    tomb = (rd == NONE) & (cl == NONE)
    wrong = ~tomb & ((rd >= n_reads) | (cl >= n_cols))
    bad = int(wrong.sum())
    keep = ~tomb & ~wrong
    rd, cl, ct = rd[keep], cl[keep], ct[keep]
    if params.min_tcov > 0:
        keep = ct.astype(np.float64) / sizes[cl].astype(np.float64) >= float(params.min_tcov)
        rd, cl, ct = rd[keep], cl[keep], ct[keep]
    c, s, nh = ct.astype(np.float64), sizes[cl].astype(np.float64), np.asarray(nk)[rd].astype(np.float64)
    mode = 3 if params.do_not_sort else int(params.sort_by)
    score = (c / nh, c / s, c / (nh + s - c), None)[mode]
    if mode == 3:
        o = np.lexsort((cl, rd))
    elif mode == 0:
        o = np.lexsort((cl, sizes[cl].astype(np.int64), -ct, rd))
    else:
        o = np.lexsort((cl, -ct, -score, rd))
    rd, cl, ct = rd[o], cl[o], ct[o]
    offs = np.concatenate([[0], np.cumsum(np.bincount(rd, minlength=n_reads))]).astype(np.uint64)
    lens = np.diff(offs.astype(np.int64))
    mixed = reordered = 0
    if bases is not None:
        score = score[o]
        u, inv = np.unique(score, return_inverse=True)
        printed = np.array([float("%.4f" % v) for v in u])[inv]
        member = np.searchsorted(np.asarray(bases, dtype=np.int64), cl, side="right") - 1
        o2 = np.lexsort((member, -printed, rd))  # stable: equal (read, printed score, member) keep the exact order
        short = lens[rd] <= WG_CAP
        reordered = len(np.unique(rd[(o2 != np.arange(len(o2))) & short]))
        rd, cl, ct, printed, member = rd[o2], cl[o2], ct[o2], printed[o2], member[o2]
        if len(rd):
            first = np.concatenate([[True], (rd[1:] != rd[:-1]) | (printed[1:] != printed[:-1])])
            start = np.flatnonzero(first)
            end = np.concatenate([start[1:], [len(rd)]]) - 1
            mixed = int(np.count_nonzero((member[start] != member[end]) & (lens[rd[start]] <= WG_CAP)))  # members ascend inside a run
    classes = (int(np.count_nonzero((lens >= 2) & (lens <= WAVE_CAP))), int(np.count_nonzero((lens > WAVE_CAP) & (lens <= WG_CAP))),
               int(np.count_nonzero(lens > WG_CAP)))
    return Ref(offs, np.stack([cl, ct], axis=1).astype(np.uint32), bad, classes, mixed, reordered)


def reference_of(case, sizes, params, bases=None):
    return reference(case.hits, case.n_hits_word, case.hit_cap, case.nk, case.n_reads, sizes, params, bases)


def well_formed(case, n_cols):
    """the hits K3 looks at without those that name no read or column (the host half refuses them; tombstones stay: it skips them)"""
    h = case.hits[:min(case.n_hits_word, case.hit_cap)]
    tomb = (h["read"] == NONE) & (h["col"] == NONE)
    return np.ascontiguousarray(h[tomb | ((h["read"] < case.n_reads) & (h["col"] < n_cols))])


def shuffled_segments(ref, rng):
    """the reference's grouping with the pairs of every segment in random order"""
    rd = np.repeat(np.arange(len(ref.offs) - 1), np.diff(ref.offs.astype(np.int64)))
    p = rng.permutation(len(rd))
    return np.ascontiguousarray(ref.pairs[p[np.argsort(rd[p], kind="stable")]])


def first_difference(name, got_offs, got_pairs, ref):
    """None, or a line naming the case, the read, the length of its segment and the first differing position.  Segments of more than
    4096 matches are compared as multisets (K3 leaves their order to the host)."""
    n_reads = len(ref.offs) - 1
    if not np.array_equal(got_offs[:n_reads + 1], ref.offs):
        r = int(np.flatnonzero(got_offs[:n_reads + 1] != ref.offs)[0])
        return f"{name}: offs[{r}] is {int(got_offs[r])} for {int(ref.offs[r])}"
    offs = ref.offs.astype(np.int64)
    lens = np.diff(offs)
    got, want = got_pairs[:int(offs[-1])].copy(), ref.pairs.copy()
    for r in np.flatnonzero(lens > WG_CAP):
        for x in (got, want):
            seg = x[offs[r]:offs[r + 1]]
            seg[:] = seg[np.lexsort((seg[:, 1], seg[:, 0]))]
    diff = np.flatnonzero((got != want).any(axis=1))
    if len(diff) == 0:
        return None
    i = int(diff[0])
    r = int(np.searchsorted(offs, i, side="right")) - 1
    return (f"{name}: read {r} ({int(lens[r])} matches{', as a multiset' if lens[r] > WG_CAP else ''}) differs at position {i - int(offs[r])}: "
            f"(column, count) {got[i].tolist()} for {want[i].tolist()}")
