"""Crafted hash lists for K1d, the dedup stage of the k-mer step (kmcp_amd/csrc/k1_dedup.hip, sort_huge.hip, query.cpp run_dedup), a plain
numpy reference of what the stage computes and a numpy restatement of how it routes a query.  No GPU, numpy only:
tests/test_dedup_cases_cpu.py checks this table against the restatement, tests/test_gpu_dedup_alone.py holds the kernels against the
reference and the launch witness against the declared sequences.

A case is one batch: queries (each a list of raw 64-bit keys, in the order the k-mer kernel would have left them) and the scalars of the
stage.  What a case is there for is DECLARED in the table as literals — the class every query lands in (`cls`), the largest bucket of
the queries that were built around one (`maxb`), the launch sequence (`seq`) and how many queries each distribution class sends to its
bitonic fallback (`fb`) — and computed a second time by the restatement (`route`, `largest_bucket`, `tokens`, `fallbacks`); the CPU
test holds the two against each other.

Classes (`cls`): "keep" n <= u (the list stays as it is); "wave" u < n <= 512 (k_dedup_wave); above that by the number m of elements
to sort (n, or what is left after adjacent repeats are dropped when `pre`): "b2048" / "b4096" / "b16384" (k_dedup_bucket, with
":buckets" or ":fallback" for the path inside the kernel), "wg:lds" / "wg:global" (k_dedup<1024, 16384>), and "huge" n > 65536 in a
batch whose max_n is above 65536 (sort_huge.hip).

Inside the contract only: max_n bounds every n, with key_shift no key is above maxHash, slots do not overlap."""
from collections import namedtuple

import numpy as np

Q = namedtuple("Q", "keys cls maxb")          # maxb: declared largest bucket, None where the query is not built around one
Case = namedtuple("Case", "id u mm pre pre_done key_shift big_bucket max_n paired queries seq fb")

U64 = np.uint64
ALL_ONES = U64(0xFFFFFFFFFFFFFFFF)
WAVE_CAP, HUGE_MIN, DB_MAXB, INT_MAX = 512, 65536, 24, 0x7FFFFFFF
KEYS_PER_WAVE = SCAN_TILE = 4096
# a FracMinHash database of scale 1000: maxHash = floor(2^64 / 1000) is no power of two, key_shift = its leading zeros
MAX_HASH = (1 << 64) // 1000
KEY_SHIFT = 64 - MAX_HASH.bit_length()
# (kernel, template parameters) of everything the stage can launch; the first two name the branch
BUCKETS = {"b2048": (2048, 1024, 256, 256 * 12), "b4096": (4096, 2048, 256, 256 * 6), "b16384": (16384, 2048, 1024, 256)}  # CAP, NB, NT, largest grid
HUGE_KERNELS = ("k_rs_hist", "k_scan_tile_sums", "k_scan_u32", "k_scan_tiles", "k_rs_scatter", "k_uq_count", "k_uq_scatter", "k_set_nk_huge")
ALL_KERNELS = sorted([("launch_dedup", 0, 0, 0), ("k_nk_simple", 0, 0, 0), ("k_dedup_wave", 0, 0, 0), ("k_adj_unique", 0, 0, 0), ("k_dedup", 1024, 16384, 0)] +
                     [("k_dedup_bucket",) + v[:3] for v in BUCKETS.values()] + [(k, 0, 0, 0) for k in HUGE_KERNELS])


def identity(rec):
    """what ALL_KERNELS holds of a witness record: the kernel and its template parameters (a radix pass's bit is none)"""
    return (rec[0],) + (tuple(rec[1:4]) if rec[0] in ("k_dedup_bucket", "k_dedup") else (0, 0, 0))


# ---- the reference ----
def adj_unique(keys):
    keep = np.ones(len(keys), dtype=bool)
    keep[1:] = keys[1:] != keys[:-1]
    return keys[keep]


def reference(case):
    """[(NumKmers, the list afterwards)] per query: np.unique above -u, else the keys as given; NumKmers 0 below -m (raw count)"""
    out = []
    for q in case.queries:
        n = len(q.keys)
        lst = np.unique(q.keys) if n > case.u else q.keys
        out.append((len(lst) if n >= case.mm else 0, lst))
    return out


def pre_done_state(case):
    """what the fused k-mer kernel (wg_reads_windows, k1_reads.hip) leaves for the stage when pre_done: per query (m, the list without
    adjacent repeats) — in scratch and nk_search — for raw counts in (max(u, 512), 65536], (None, None) for the others, whose raw lists
    stay in hashes"""
    out = []
    for q in case.queries:
        lst = adj_unique(q.keys) if max(case.u, WAVE_CAP) < len(q.keys) <= HUGE_MIN else None
        out.append((None if lst is None else len(lst), lst))
    return out


# ---- the restatement of the routing ----
def to_sort(case, q):
    """the elements the workgroup classes sort"""
    return adj_unique(q.keys) if case.pre else q.keys


def bucket_of(v, lz, nb):
    """k_dedup_bucket: (v << lz) >> (64 - 10 | 11)"""
    return (np.asarray(v, dtype=U64) << U64(lz)) >> U64(64 - (10 if nb == 1024 else 11))


def largest_bucket(case, q, nb):
    return int(np.bincount(bucket_of(to_sort(case, q), case.key_shift, nb).astype(np.int64), minlength=nb).max())


def route(case, q):
    n = len(q.keys)
    if n <= case.u:
        return "keep"
    if n <= WAVE_CAP:
        return "wave"
    if n > (HUGE_MIN if case.max_n > HUGE_MIN else INT_MAX):
        return "huge"
    m = len(to_sort(case, q))
    for name in ("b2048", "b4096") + (("b16384",) if case.big_bucket else ()):
        cap, nb = BUCKETS[name][:2]
        if m <= cap:
            return name + (":fallback" if largest_bucket(case, q, nb) > DB_MAXB else ":buckets")
    return "wg:lds" if m <= 16384 else "wg:global"


def fallbacks(case):
    r = [route(case, q) for q in case.queries]
    return tuple(r.count(b + ":fallback") for b in BUCKETS)


def tokens(case):
    """the launch sequence as a pure function of max_n, pre, pre_done, the knob and the huge queries (launch_dedup, run_dedup)"""
    if case.max_n <= case.u:
        return ["nk_simple"]
    t = ["dedup"]
    if not case.queries:
        return t
    t.append("wave")
    if case.max_n > WAVE_CAP:
        if case.pre and not case.pre_done:
            t.append("adj")
        t.append("b2048")
    if case.max_n > 2048:
        t.append("b4096")
    if case.max_n > 4096:
        if case.big_bucket:
            t.append("b16384")
            if case.max_n > 16384:
                t.append("wg>16384")
        else:
            t.append("wg>4096")
    if case.max_n > HUGE_MIN:
        t += [("huge", r, len(q.keys)) for r, q in enumerate(case.queries) if len(q.keys) > max(HUGE_MIN, case.u)]
    return t


def huge_records(r, n):
    """the 46 launches of huge_dedup for query r of n keys"""
    nw = -(-n // KEYS_PER_WAVE)
    blocks = -(-nw // 4)

    def scan(total):
        tiles = -(-total // SCAN_TILE)
        return [("k_scan_tile_sums", 0, 0, 0, tiles, 256, r, n), ("k_scan_u32", 0, 0, 0, 1, 1024, r, n), ("k_scan_tiles", 0, 0, 0, tiles, 256, r, n)]
    out = []
    for shift in range(0, 64, 8):
        out += [("k_rs_hist", shift, 0, 0, blocks, 256, r, n)] + scan(256 * nw) + [("k_rs_scatter", shift, 0, 0, blocks, 256, r, n)]
    return out + [("k_uq_count", 0, 0, 0, blocks, 256, r, n)] + scan(nw) + [("k_uq_scatter", 0, 0, 0, blocks, 256, r, n), ("k_set_nk_huge", 0, 0, 0, 1, 1, r, n)]


def expand(seq, n_reads, u, max_n, fb):
    """declared tokens -> the records Database.last_dedup_launches() returns: (kernel, p0, p1, p2, grid, block, lo, hi)"""
    grid = min(n_reads, 1 << 20)
    out = []
    for t in seq:
        if t == "nk_simple":
            out.append(("k_nk_simple", 0, 0, 0, 0, 0, 0, 0))
        elif t == "dedup":
            out.append(("launch_dedup",) + tuple(fb) + (0, 0, 0, 0))
        elif t == "wave":
            out.append(("k_dedup_wave", 0, 0, 0, (n_reads + 3) // 4, 256, u, WAVE_CAP))
        elif t == "adj":
            out.append(("k_adj_unique", 0, 0, 0, grid, 512, WAVE_CAP, HUGE_MIN if max_n > HUGE_MIN else INT_MAX))
        elif t in BUCKETS:
            cap, nb, nt, gmax = BUCKETS[t]
            out.append(("k_dedup_bucket", cap, nb, nt, min(grid, gmax), nt, {2048: 0, 4096: 2048, 16384: 4096}[cap], cap))
        elif t in ("wg>16384", "wg>4096"):
            out.append(("k_dedup", 1024, 16384, 0, min(grid, 1024), 1024, int(t[3:]), INT_MAX))
        else:
            assert t[0] == "huge", t
            out += huge_records(t[1], t[2])
    return out


def canonical(records):
    """which of several huge queries is sorted first is decided by an atomic on the device: their groups of records are put in the
    order of the queries (each group keeps its own order)"""
    head = [r for r in records if r[0] not in HUGE_KERNELS]
    tail = [r for r in records if r[0] in HUGE_KERNELS]
    return head + sorted(tail, key=lambda r: r[6])  # sorted() is stable


# ---- layout ----
def layout(case):
    """where every query's slot starts (koff), the split into offs + offs2 of a paired batch, and the words in all: a slot is longer than
    its list, by 1 .. 13 words, so that what lies behind a list is a guard in front of the next one"""
    n = np.array([len(q.keys) for q in case.queries], dtype=np.int64)
    slot = n + 1 + (np.arange(len(n)) * 7) % 13
    koff = np.concatenate([[0], np.cumsum(slot)[:-1]]).astype(np.int64) if len(n) else np.zeros(0, dtype=np.int64)
    offs2 = koff // 3 if case.paired else None
    offs = koff - offs2 if case.paired else koff
    return koff, offs, offs2, int(slot.sum())


# ---- key builders ----
def rnd(n, seed, hi=(1 << 64) - 1):
    """n keys in [1, hi), about one in twenty a repeat of another"""
    rng = np.random.default_rng(seed)
    k = rng.integers(1, hi, size=n, dtype=U64)
    if n >= 20:
        at = rng.choice(n, size=n // 20, replace=False)
        k[at] = k[rng.integers(0, n, size=len(at))]
    return k


def cat(*parts):
    """(every part made uint64 first: numpy would join uint64 and Python ints as float64)"""
    return np.concatenate([np.asarray(p, dtype=U64) for p in parts])


def shuffled(keys, seed):
    return np.random.default_rng(seed).permutation(keys)


def sorted_with_repeats_at(n, seams, seed):
    """n keys whose SORTED order has elements s - 1 and s equal for every seam s, in random order"""
    s = np.unique(np.random.default_rng(seed).integers(1, (1 << 64) - 1, size=n + 64, dtype=U64))[:n].copy()
    assert len(s) == n
    for x in seams:
        s[x] = s[x - 1]
    return shuffled(s, seed + 1)


def around_bucket(n, nb, count, bucket, seed, lz=0, used=None):
    """n elements of which exactly `count` fall into `bucket` of nb and every other bucket (of the first `used`: those below maxHash)
    holds far fewer; ten of them repeats"""
    bits = 10 if nb == 1024 else 11
    rng = np.random.default_rng(seed)
    others = np.array([b for b in range(used or nb) if b != bucket], dtype=U64)
    ids = np.concatenate([np.full(count, bucket, dtype=U64), others[np.arange(n - count - 10) % len(others)]])
    low = rng.integers(0, 1 << (64 - bits), size=len(ids), dtype=U64)
    keys = ((ids << U64(64 - bits)) | low) >> U64(lz)
    rest = keys[count:]
    keys = np.concatenate([keys, rest[rng.integers(0, len(rest), size=10)]])
    return shuffled(keys, seed + 1)


def in_bucket(n, nb, bucket, seed):
    """n keys that all fall into one bucket"""
    bits = 10 if nb == 1024 else 11
    low = np.random.default_rng(seed).integers(0, 1 << (64 - bits), size=n, dtype=U64)
    return (U64(bucket) << U64(64 - bits)) | low


def runs(n, m, seed, same=()):
    """n keys in m runs of equal keys (run lengths random, every run's key differs from its neighbours'); same = pairs of runs that
    share a key although they are not adjacent: only the sort removes that repeat"""
    rng = np.random.default_rng(seed)
    vals = np.unique(rng.integers(1, (1 << 64) - 1, size=m + 64, dtype=U64))
    vals = rng.permutation(vals)[:m].copy()
    for a, b in same:
        assert abs(a - b) > 1
        vals[b] = vals[a]
    cuts = np.sort(rng.choice(np.arange(1, n), size=m - 1, replace=False)) if m > 1 else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([[0], cuts, [n]]))
    return np.repeat(vals, lens)


def seams(n, seed):
    """random keys with runs of equal keys across the positions 63 | 64, 511 | 512 and 1023 | 1024 of the raw list (the lane, tile and
    second-tile seams of k_adj_unique), and one repeat far from its twin"""
    k = rnd(n, seed)
    for lo, hi in ((60, 68), (508, 516), (1020, 1030)):
        k[lo:hi] = k[lo]
    k[5] = k[n - 7]
    return k


def plane(n, b, seed):
    """keys that differ in byte b only"""
    base = U64(0x5AC3961E2D784B0F) & ~(U64(255) << U64(8 * b))
    return base | (np.random.default_rng(seed).integers(0, 256, size=n, dtype=U64) << U64(8 * b))


def asc(n, step=3):
    return (np.arange(1, n + 1, dtype=U64) * U64(step)) << U64(40)


# ---- the table ----
CASES = []


def case(id, queries, seq, u=4, mm=1, pre=0, pre_done=0, key_shift=0, big_bucket=True, max_n=None, paired=False, fb=(0, 0, 0)):
    queries = [q if isinstance(q, Q) else Q(np.ascontiguousarray(q[0], dtype=U64), q[1], q[2] if len(q) > 2 else None) for q in queries]
    CASES.append(Case(id, u, mm, pre, pre_done, key_shift, big_bucket, max(len(q.keys) for q in queries) if max_n is None else max_n, paired, queries, seq, fb))


ONE = np.array([77], dtype=U64)
WG_ALL = ["dedup", "wave", "b2048", "b4096", "b16384", "wg>16384"]

# -- the wave class: n = 5, 8, 9, 63, 64, 65, 511, 512 in batches of 1, 4 and 5 queries (a partial block of four waves)
# (three zeros sort in front: the pair of sorted_with_repeats_at lands on elements 255 | 256)
case("wave-1", [(cat(sorted_with_repeats_at(506, (253,), 10), [0, 0, 0], [ALL_ONES] * 3)[::-1], "wave")], ["dedup", "wave"])
case("wave-4", [(asc(5), "wave"), (asc(8)[::-1], "wave"), (np.full(9, 12345, dtype=U64), "wave"),
                (cat([ALL_ONES], rnd(61, 11), [0]), "wave")], ["dedup", "wave"])
case("wave-5", [(sorted_with_repeats_at(64, (8,), 12), "wave"), (cat([0, ALL_ONES] * 4, rnd(57, 13)), "wave"),
                (np.repeat(asc(256), 2)[::-1][:511], "wave"), (np.array([9, 3, 3, 1], dtype=U64), "keep"), (np.array([9, 3, 3, 1, 3], dtype=U64), "wave")],
     ["dedup", "wave"])
case("wave-edges", [(np.full(512, ALL_ONES, dtype=U64), "wave"), (np.zeros(512, dtype=U64), "wave"), (asc(512), "wave"), (asc(64)[::-1], "wave"),
                    (sorted_with_repeats_at(512, (8, 256, 511), 14), "wave"), (np.full(65, 0, dtype=U64), "wave")], ["dedup", "wave"])
case("wave-min-matched", [(rnd(9, 15), "wave"), (rnd(10, 16), "wave"), (np.array([5, 1, 5], dtype=U64), "keep")], ["dedup", "wave"], mm=10)

# -- the distribution classes at their bounds, uniform keys
case("bucket-uniform", [(rnd(n, 20 + i), c) for i, (n, c) in enumerate(((513, "b2048:buckets"), (2048, "b2048:buckets"), (2049, "b4096:buckets"),
                                                                        (4096, "b4096:buckets"), (4097, "b16384:buckets"), (16384, "b16384:buckets")))],
     ["dedup", "wave", "b2048", "b4096", "b16384"])
# exactly 24 keys in one bucket (the buckets), exactly 25 (the bitonic network), for each instantiation
case("bucket-24-25", [(around_bucket(1500, 1024, 24, 700, 30), "b2048:buckets", 24), (around_bucket(1500, 1024, 25, 700, 31), "b2048:fallback", 25),
                      (around_bucket(3500, 2048, 24, 1, 32), "b4096:buckets", 24), (around_bucket(3500, 2048, 25, 1, 33), "b4096:fallback", 25),
                      (around_bucket(12000, 2048, 24, 2046, 34), "b16384:buckets", 24), (around_bucket(12000, 2048, 25, 2046, 35), "b16384:fallback", 25)],
     ["dedup", "wave", "b2048", "b4096", "b16384"], fb=(1, 1, 1))
case("bucket-one-value-one-bucket",
     [(np.full(2048, 1 << 50, dtype=U64), "b2048:fallback", 2048), (np.full(4096, ALL_ONES, dtype=U64), "b4096:fallback", 4096),
      (np.zeros(16384, dtype=U64), "b16384:fallback", 16384),
      (in_bucket(600, 1024, 0, 40), "b2048:fallback", 600), (in_bucket(2500, 2048, 0, 41), "b4096:fallback", 2500), (in_bucket(5000, 2048, 0, 42), "b16384:fallback", 5000),
      (in_bucket(600, 1024, 1023, 43), "b2048:fallback", 600), (in_bucket(2500, 2048, 2047, 44), "b4096:fallback", 2500),
      (in_bucket(5000, 2048, 2047, 45), "b16384:fallback", 5000)],
     ["dedup", "wave", "b2048", "b4096", "b16384"], fb=(3, 3, 3))
# FracMinHash: keys in [0, maxHash], maxHash itself and 0 among them, each three times
_mh = lambda n, seed: shuffled(cat(rnd(n - 6, seed, hi=MAX_HASH), [MAX_HASH] * 3, [0] * 3), seed + 1)  # noqa: E731
case("bucket-key-shift", [(_mh(1500, 50), "b2048:buckets"), (_mh(3000, 52), "b4096:buckets"), (_mh(9000, 54), "b16384:buckets"),
                          (around_bucket(1500, 1024, 24, 523, 56, lz=KEY_SHIFT, used=524), "b2048:buckets", 24),  # (maxHash itself is in bucket 524)
                          (around_bucket(1500, 1024, 25, 0, 57, lz=KEY_SHIFT, used=524), "b2048:fallback", 25)],
     ["dedup", "wave", "b2048", "b4096", "b16384"], key_shift=KEY_SHIFT, fb=(1, 0, 0))
case("classes-min-matched", [(rnd(9, 60), "wave"), (rnd(1000, 61), "b2048:buckets"), (np.full(2999, 8, dtype=U64), "b4096:fallback", 2999),
                             (rnd(3000, 62), "b4096:buckets"), (rnd(20000, 63), "wg:global"), (rnd(20001, 64), "wg:global"), (np.array([4, 4], dtype=U64), "keep")],
     WG_ALL, mm=20001, fb=(0, 1, 0))


# -- one workgroup strides from query 0 to query `grid`: the fallback first and the buckets second, and the other way round
def _stride(id, grid, first, second, seq, fb, **kw):
    case(id, [first] + [(ONE, "keep")] * (grid - 1) + [second], seq, fb=fb, **kw)


for _name, _n, _seq in (("b2048", 1500, WG_ALL[:3]), ("b4096", 3500, WG_ALL[:4]), ("b16384", 12000, WG_ALL[:5])):
    _cap, _nb, _nt, _grid = BUCKETS[_name]
    _bad, _good = (around_bucket(_n, _nb, 25, 5, 70), _name + ":fallback", 25), (around_bucket(_n, _nb, 24, 5, 71), _name + ":buckets", 24)
    _fb = tuple(int(b == _name) for b in BUCKETS)
    _stride("stride-%s-fallback-first" % _name, _grid, _bad, _good, _seq, _fb)
    _stride("stride-%s-buckets-first" % _name, _grid, _good, _bad, _seq, _fb)
_stride("stride-wg-lds-first", 1024, (rnd(5000, 72), "wg:lds"), (rnd(17000, 73), "wg:global"), ["dedup", "wave", "b2048", "b4096", "wg>4096"], (0, 0, 0), big_bucket=False)
_stride("stride-wg-global-first", 1024, (rnd(17000, 73), "wg:global"), (rnd(5000, 72), "wg:lds"), ["dedup", "wave", "b2048", "b4096", "wg>4096"], (0, 0, 0), big_bucket=False)

# -- k_dedup<1024, 16384>: the network in global memory, and (KMCPG_DEDUP_BIG_BUCKET=0) in LDS
case("wg-global", [(rnd(16385, 80), "wg:global"), (rnd(20000, 81), "wg:global"), (rnd(65536, 82), "wg:global")], WG_ALL)
case("wg-lds", [(rnd(4097, 83), "wg:lds"), (rnd(10000, 84), "wg:lds"), (rnd(16384, 85), "wg:lds")], ["dedup", "wave", "b2048", "b4096", "wg>4096"], big_bucket=False)
# n_hi == HUGE_MIN: 65536 keys still belong to the workgroup class
case("wg-65536-beside-huge", [(rnd(65536, 86), "wg:global"), (rnd(65537, 87), "huge")], WG_ALL + [("huge", 1, 65537)])

# -- adjacent repeats first (window sketches): k_adj_unique, or what the fused k-mer kernel leaves
_PRE = [(seams(1500, 90), "b2048:buckets"), (runs(20000, 1500, 91, same=((10, 700),)), "b2048:buckets"), (runs(3000, 1, 92), "b2048:buckets"),
        (runs(5000, 2048, 93), "b2048:buckets"), (runs(5000, 2049, 94, same=((0, 2048),)), "b4096:buckets"), (runs(30000, 9000, 95), "b16384:buckets"),
        (runs(30000, 17000, 96, same=((1, 16999),)), "wg:global"), (seams(65536, 97), "wg:global"), (runs(300, 40, 98, same=((3, 30),)), "wave"),
        (np.array([6, 6, 2], dtype=U64), "keep")]
case("pre", _PRE, ["dedup", "wave", "adj", "b2048", "b4096", "b16384", "wg>16384"], pre=1)
case("pre-done", _PRE, WG_ALL, pre=1, pre_done=1)
case("pre-min-matched", _PRE[:3], ["dedup", "wave", "adj", "b2048", "b4096", "b16384", "wg>16384"], pre=1, mm=3001)

# -- the device-wide sort
case("huge-65537", [(rnd(65537, 100), "huge")], WG_ALL + [("huge", 0, 65537)])
case("huge-17-waves-all-equal", [(np.full(69632, 0x0123456789ABCDEF, dtype=U64), "huge")], WG_ALL + [("huge", 0, 69632)])
case("huge-descending", [(asc(69633, 5)[::-1], "huge")], WG_ALL + [("huge", 0, 69633)])
for _b in range(8):
    case("huge-byte-%d" % _b, [(plane(65537, _b, 110 + _b), "huge")], WG_ALL + [("huge", 0, 65537)])
case("huge-seams", [(sorted_with_repeats_at(69633, (64, 4096, 8192, 69632), 120), "huge")], WG_ALL + [("huge", 0, 69633)])
case("huge-zero-and-ones", [(shuffled(cat(rnd(65531, 121), [0] * 3, [ALL_ONES] * 3), 122), "huge")], WG_ALL + [("huge", 0, 65537)])
case("huge-two", [(rnd(70000, 123), "huge"), (rnd(9, 124), "wave"), (rnd(1000, 125), "b2048:buckets"), (np.array([3, 1, 3], dtype=U64), "keep"),
                  (rnd(66000, 126), "huge")], WG_ALL + [("huge", 0, 70000), ("huge", 4, 66000)])
case("huge-paired", [(rnd(65537, 127), "huge"), (rnd(100, 128), "wave"), (rnd(70001, 129), "huge")], WG_ALL + [("huge", 0, 65537), ("huge", 2, 70001)], paired=True)
case("huge-u-70000", [(rnd(69000, 130), "keep"), (rnd(70001, 131), "huge")], WG_ALL + [("huge", 1, 70001)], u=70000)
case("huge-min-matched", [(rnd(65537, 132), "huge"), (rnd(1000, 133), "b2048:buckets"), (np.array([2, 1], dtype=U64), "keep")],
     WG_ALL + [("huge", 0, 65537)], mm=100000)

# -- no query can be above -u: k_nk_simple alone
case("nk-simple", [(rnd(600, 140), "keep"), (rnd(299, 141), "keep"), (rnd(300, 142), "keep"), (ONE, "keep")], ["nk_simple"], u=1000, mm=300, max_n=600)

# -- one large query: k_scan_u32 with two elements per thread (more than 1024 scan tiles = more than 16384 waves of keys).  The keys are
# generated on the device: keys[i] = ((n - 1 - i) // 3) * LARGE_C, descending in triples, below 2^63, every byte plane varies
LARGE_N = 4096 * 16384 + 1
LARGE_C = (1 << 38) + 12345
LARGE_SEQ = WG_ALL + [("huge", 0, LARGE_N)]
