"""The K1 test plan: every kernel instantiation launch_k1 (kmcp_amd/csrc/k1_kmers.hip) can be asked for, with the smallest batches that reach
each edge of it, and the witness (`Database.last_k1_launches()` / `last_k1_plan()`) every case must produce.

A case is a database (open_synthetic: k, sketch mode, s or w, scale), a batch (single or paired reads, text or 2-bit codes), the knobs
KMCPG_K1_FLAGS and KMCPG_WR_WAVES, and -u / -m.  It DECLARES the form of the plan, wsz / waves / grid / dynamic LDS of its kernels (the
LDS limits as literals, the rest by the documented formula, _wr_lds) and — for the two list forms — exactly how many reads / segments
the first kernel leaves to the one behind it.
tests/test_k1_forms_plan_cpu.py checks the declarations without a GPU: against k1_plan() compiled for the host, and against the oracle
(the conditions that keep a GPU test from passing vacuously); tests/test_gpu_k1_forms.py runs the cases.

The reference is independent of the kernels: the oracle's generate_kmers per mate, mate 1's list followed by mate 2's, sort_unique above
-u; left_on_list from a numpy restatement of the documented leave rules (roll_left, seg_left).

k1_windows_roll<32, 4> is not in ALL_KERNELS: four rings of 32 x 64 k-mer hashes are 65 536 bytes by themselves, so with the 1 024
bytes of tables in front no read length fits and the plan always halves the waves (UNREACHABLE; the CPU test sweeps the lengths).
"""
import collections

import numpy as np

BIG = 1 << 30   # a -u no read reaches
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K1SEG = 65536
HUGE_MIN = 65536
WAVE_SORT_CAP = 512
WR_MIN_WINDOWS = 1024
MODES = {"plain": 0, "min": 1, "syn": 2}

Db = collections.namedtuple("Db", "k mode ws scale")   # mode: plain | min | syn; ws: w (min) or s (syn)


class Case:
    def __init__(self, id, db, reads, expect, reads2=None, flags=None, wr_waves=None, u=BIG, min_qlen=0, codes=False, left=None, roll_reads=(),
                 u_both=False, seam=None):
        self.id, self.db, self.reads, self.reads2 = id, db, list(reads), (None if reads2 is None else list(reads2))
        self.flags, self.wr_waves, self.u, self.min_qlen, self.codes = flags, wr_waves, u, min_qlen, codes
        self.expect = expect          # dict(form, kernels=[(name, p0, p1, grid, block, lds)], codes_direct, list_fallback, adj_done)
        self.left = left              # the two list forms: what the witness must report (exact); None elsewhere
        self.roll_reads = tuple(roll_reads)   # reads meant for k1_windows_roll
        self.u_both = u_both          # the batch has reads on both sides of -u
        self.seam = seam              # "read" / "mate": adjacent repeats across every wave / tile / lane seam of a read, or across the mates
        assert reads2 is None or len(self.reads2) == len(self.reads)

    @property
    def paired(self):
        return self.reads2 is not None

    @property
    def max_read_len(self):
        return max(len(r) for r in self.reads + (self.reads2 or []))

    @property
    def env(self):
        return {"KMCPG_K1_FLAGS": self.flags, "KMCPG_WR_WAVES": self.wr_waves}

    def shape_line(self):
        """the case's shape for tests/k1_forms_print.cpp"""
        n_exc = n_bases = 0
        if self.codes:
            n_bases = sum(len(r) for r in self.reads)
            n_exc = len(foreign_runs(b"".join(self.reads)))
        return "%s %d %d %d %d %d %d %d %d %d %d %d %d" % (self.id, MODES[self.db.mode], self.db.k, self.db.ws, int(self.paired), len(self.reads), self.max_read_len,
                                                        self.u, 3 if self.flags is None else int(self.flags), 2 if self.wr_waves is None else int(self.wr_waves),
                                                        int(self.codes), n_exc, n_bases)


# ---- sequences ------------------------------------------------------------------------------------------------------------------
def rnd(n, seed):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def put(seq, pos, what):
    b = bytearray(seq)
    b[pos:pos + len(what)] = what
    return bytes(b)


LOWC = b"ACGTTGCAAT"


def is_acgt(seq):
    a = np.frombuffer(seq, dtype=np.uint8) & 0xDF
    return np.isin(a, ACGT)


def foreign_runs(seq):
    """runs of equal bytes other than A/C/G/T in either case, as the packer of 2-bit codes notes them (no U in this plan's reads)"""
    a = np.frombuffer(seq, dtype=np.uint8)
    bad = ~is_acgt(seq)
    idx = np.nonzero(bad)[0]
    runs = []
    for p in idx:
        if runs and runs[-1][0] + runs[-1][1] == p and a[p] == runs[-1][2]:
            runs[-1][1] += 1
        else:
            runs.append([int(p), 1, int(a[p])])
    return runs


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def sketch_cfg(O, db):
    return O.sketch_cfg(k=db.k, scale=db.scale, minimizer_w=db.ws if db.mode == "min" else 0, syncmer_s=db.ws if db.mode == "syn" else 0)


def reference(case, O):
    """per query: (raw emissions of mate 1, of mate 2, the list the k-mer stage must leave, nk1); a query shorter than -m in mate 1 whose
    mate 2 does not reach -m either has no k-mers (handleQuery); otherwise both mates are sketched whatever their lengths"""
    cfg = sketch_cfg(O, case.db)
    out = []
    for i, r1 in enumerate(case.reads):
        r2 = case.reads2[i] if case.paired else None
        skip = len(r1) < case.min_qlen and not (r2 is not None and len(r2) >= case.min_qlen)
        e = np.zeros(0, dtype=np.uint64)
        raw1 = e if skip else O.generate_kmers(r1, cfg)
        raw2 = e if (skip or r2 is None) else O.generate_kmers(r2, cfg)
        raw = np.concatenate([raw1, raw2])
        want = O.sort_unique(raw) if len(raw) > case.u else raw
        out.append((raw1, raw2, want, len(raw1)))
    return out


def roll_left(case, ref):
    """how many reads k1_windows_roll leaves to k1_windows_wave: a byte other than A/C/G/T in either case, fewer than 1024 windows,
    len <= max(-u, 512), or an emission count outside (max(-u, 512), 65 536]"""
    k, s = case.db.k, case.db.ws
    lw = 2 * k - s - 1
    bound = max(case.u, WAVE_SORT_CAP)
    left = []
    for i, r in enumerate(case.reads):
        n_emit = len(ref[i][0])
        if (not is_acgt(r).all() or len(r) - lw + 1 < WR_MIN_WINDOWS or len(r) <= bound or len(r) < case.min_qlen or not (bound < n_emit <= HUGE_MIN)):
            left.append(i)
    return left


def seg_left(case):
    """how many (read, segment) pairs k1_seg_roll2 leaves to k1_seg_roll: segments with a foreign byte among the bases their k-mers cover
    (segment g owns the k-mer positions [g 65536, (g + 1) 65536): the bases up to k - 1 further)"""
    k = case.db.k
    n = 0
    for r in case.reads:
        npos = len(r) - k + 1
        if len(r) < case.min_qlen or npos <= 0:
            continue
        ok = is_acgt(r)
        for g in range((npos + K1SEG - 1) // K1SEG):
            lo, hi = g * K1SEG, min((g + 1) * K1SEG, npos) + k - 1
            n += int(not ok[lo:hi].all())
    return n


# ---- the witness a form leaves ------------------------------------------------------------------------------------------------------
def _exp(form, kernels, codes_direct=False, list_fallback=False, adj_done=False, wsz=0, waves=0, lds=0):
    return dict(form=form, kernels=kernels, codes_direct=codes_direct, list_fallback=list_fallback, adj_done=adj_done, wsz=wsz, waves=waves, lds=lds,
                grid=kernels[0][3] if kernels else 0)


def x_short(mode, grid):
    return _exp("Short", [("k1_kmers", mode, 0, grid, 256, 0)])


def x_wg(mode, grid, adj):
    return _exp("Wg", [("k1_kmers_wg", mode, 0, grid, 1024, 0)], adj_done=adj)


def x_wg_global(grid):
    return _exp("WgGlobal", [("k1_kmers_wg_global", 0, 0, grid, 1024, 0)])


def x_wave(mode, grid):
    return _exp("WindowsWave", [("k1_windows_wave", mode, 0, grid, 512, 0)], adj_done=True)


def x_roll(wsz, waves, grid, lds, grid2):
    return _exp("WindowsRoll", [("k1_windows_roll", wsz, waves, grid, 64 * waves, lds), ("k1_windows_wave", 2, 0, grid2, 512, 0)], list_fallback=True,
                adj_done=True, wsz=wsz, waves=waves, lds=lds)


def x_seg_roll2(grid, grid2, codes=False, n_exc_grid=0):
    if not codes:
        ks = [("k1_seg_roll2", 0, 0, grid, 256, 0), ("k1_seg_roll", 0, 0, grid2, 512, 0), ("k1_seg_pack", 0, 0, grid, 256, 0)]
        return _exp("SegRoll2", ks, list_fallback=True)
    if not n_exc_grid:  # codes without a foreign byte: nothing gets on the list, no fallback kernel is launched
        return _exp("SegRoll2", [("k1_seg_roll2", 0, 0, grid, 256, 0), ("k1_seg_pack", 0, 0, grid, 256, 0)], codes_direct=True)
    ks = [("k_mark_exc", 0, 0, n_exc_grid, 256, 0), ("k1_seg_roll2", 0, 0, grid, 256, 0), ("k_unpack2_list", 0, 0, grid2, 256, 0),
          ("k1_seg_roll", 0, 0, grid2, 512, 0), ("k1_seg_pack", 0, 0, grid, 256, 0)]
    e = _exp("SegRoll2", ks, codes_direct=True, list_fallback=True)
    e["grid"] = grid
    return e


def x_seg_roll(grid):
    return _exp("SegRoll", [("k1_seg_roll", 0, 0, grid, 512, 0), ("k1_seg_pack", 0, 0, grid, 256, 0)])


def x_seg_hash(grid):
    return _exp("SegHash", [("k1_seg_hash", 0, 0, grid, 1024, 0), ("k1_seg_pack", 0, 0, grid, 256, 0)])


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)


def _tag(db):
    return "k%d-%s%s%s" % (db.k, db.mode, db.ws or "", "-x%d" % db.scale if db.scale > 1 else "")


# -- Short: k1_kmers<0|1|2>, four reads per workgroup; k <= 65 the prefix-XOR scan, above it the closed form
def _short():
    for n, db in enumerate((Db(21, "plain", 0, 1), Db(21, "plain", 0, 5), Db(21, "min", 5, 1), Db(21, "syn", 11, 1), Db(65, "plain", 0, 1), Db(65, "syn", 33, 1),
                            Db(66, "plain", 0, 1), Db(66, "min", 5, 1))):
        k, m = db.k, MODES[db.mode]
        g, h = rnd(2048, 100 + n), rnd(2048, 200 + n)
        lens = [k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 2048]
        single = [g[:L] for L in lens] + [put(g[300:450], 40, b"N"), g[500:650].lower()]          # 12 reads: 3 workgroups
        add("short-%s" % _tag(db), db, single, x_short(m, 3))
        # mate 2 empty / shorter than k / shorter than -m (30) while mate 1 passes / the other way round / both too short / mate 1 empty
        pairs = [(2048, 0), (150, k - 1), (150, 25), (25, 150), (25, 25), (k, k + 1), (63, 129), (128, 64), (2048, 2048), (0, 150), (129, 127)]
        r1 = [g[:a] for a, b in pairs] + [g[100:250]]
        r2 = [h[:b] for a, b in pairs] + [g[100:250]]                                               # ... and a pair of equal mates
        add("short-pe-%s" % _tag(db), db, r1, x_short(m, 3), reads2=r2, min_qlen=30)
        if db in (Db(21, "plain", 0, 1), Db(21, "syn", 11, 1), Db(66, "plain", 0, 1)):
            add("short-u100-%s" % _tag(db), db, single, x_short(m, 3), u=100, u_both=True)
            add("short-pe-u140-%s" % _tag(db), db, r1, x_short(m, 3), reads2=r2, min_qlen=30, u=140, u_both=True)


# -- Wg: k1_kmers_wg<0|1|2>, one workgroup per read, tiles of T positions / windows (T = 1024 - halo; 1024 with a halo above 512)
def _wg():
    # plain k-mers: halo k - 1
    for n, (db, T) in enumerate(((Db(21, "plain", 0, 1), 1004), (Db(66, "plain", 0, 1), 959), (Db(21, "plain", 0, 5), 1004))):
        k = db.k
        g, h = rnd(4000, 300 + n), rnd(4000, 320 + n)
        lens = [T + k - 1, T + k, 2 * T + k - 1, 2 * T + k, 2049, 3000, 100, 276, 277]              # positions T, T + 1, 2T, 2T + 1; -u 256 at 256 / 257
        reads = [g[:L] for L in lens] + [put(g[:2500], 1200, b"NN")]
        add("wg-%s" % _tag(db), db, reads, x_wg(0, 10, False))
        add("wg-u256-%s" % _tag(db), db, reads, x_wg(0, 10, False), u=256, u_both=True)
        pairs = [(3000, 2500), (2100, 0), (0, 2100), (T + k - 1, T + k), (2 * T + k, 20), (2049, 2049), (100, 120)]
        add("wg-pe-%s" % _tag(db), db, [g[:a] for a, b in pairs], x_wg(0, 7, False), reads2=[h[:b] for a, b in pairs], u=256, u_both=True)

    def windows(db, T, extra, flags_list, pe=True, tag=""):
        """reads of T, T + 1, 2T, 2T + 1 windows, `extra` bases of random sequence (enough emissions for the fused path), a homopolymer
        (every window emits the same value: an adjacent repeat across every tile seam), low-complexity sequence, a short read"""
        k, m = db.k, MODES[db.mode]
        base = (k + db.ws - 2) if db.mode == "min" else (2 * k - db.ws - 2)     # len = windows + base
        g = rnd(extra + 100, 400 + T + db.ws)
        reads = [g[:w + base] for w in (T, T + 1, 2 * T, 2 * T + 1)] + [g[:extra], b"A" * 3100, (LOWC * 400)[:3777], g[5:205]]
        for flags in flags_list:
            adj = flags is None or bool(int(flags) & 2)
            f = "" if flags is None else "-f%s" % flags
            add("wg-%s%s%s" % (_tag(db), tag, f), db, reads, x_wg(m, 8, adj), flags=flags, u=256, u_both=True, seam="read" if adj and db.scale == 1 else None)
            add("wg-uBIG-%s%s%s" % (_tag(db), tag, f), db, reads, x_wg(m, 8, adj), flags=flags)
        if pe:  # equal emissions on both sides of the mate boundary: the same sequence as both mates, and a homopolymer
            r1 = [g[:extra], b"A" * 2600, g[:2 * T + base], g[:2100], b"", g[:150]]
            r2 = [g[:extra], b"A" * 2600, g[7:T + base + 8], b"", g[:2100], g[300:400]]
            for flags in flags_list[:1]:
                adj = flags is None or bool(int(flags) & 2)
                f = "" if flags is None else "-f%s" % flags
                add("wg-pe-%s%s%s" % (_tag(db), tag, f), db, r1, x_wg(m, 6, adj), reads2=r2, flags=flags, u=256, u_both=True, seam="mate" if adj else None)

    windows(Db(21, "min", 61, 1), 942, 20000, [None])                   # w = 61: the first width k1_windows_wave does not take
    windows(Db(21, "min", 491, 1), 512, 4000, [None])                   # w + k = 512: the last halo with tiles of 1024 - halo
    windows(Db(21, "min", 492, 1), 1024, 5000, [None, "1", "0"])        # w + k = 513: tiles of 1024 windows, wg_prefix in two rounds
    windows(Db(21, "min", 510, 1), 1024, 5000, [None])                  # w = 510: the last width of the LDS tile form
    windows(Db(63, "syn", 32, 1), 931, 3000, [None])                    # 2 (k - s) = 62: the first window k1_windows_wave does not take
    windows(Db(21, "min", 7, 1), 996, 5000, ["7", "4", "5"])            # KMCPG_K1_FLAGS bit 2: the tile form where the wave form would do
    windows(Db(21, "syn", 11, 1), 994, 5000, ["7", "4", "5"])
    windows(Db(21, "syn", 11, 3), 994, 9000, ["7"], pe=False)


# -- WgGlobal: halo too large for the LDS tiles
def _wg_global():
    db = Db(21, "min", 511, 1)
    g, h = rnd(4000, 500), rnd(4000, 501)
    add("wgglobal-%s" % _tag(db), db, [g[:2049], g[:3000], b"A" * 2600, g[:600], g[:531], g[:530]], x_wg_global(6))
    add("wgglobal-u256-%s" % _tag(db), db, [g[:2049], g[:3000], b"A" * 2600, g[:600]], x_wg_global(4), u=256, u_both=True)
    pairs = [(3000, 2500), (2100, 0), (0, 2100), (2600, 2600)]
    add("wgglobal-pe-%s" % _tag(db), db, [g[:a] for a, b in pairs[:3]] + [b"A" * 2600], x_wg_global(4), reads2=[h[:b] for a, b in pairs[:3]] + [b"A" * 2600], u=256,
        u_both=True)


# -- WindowsWave: k1_windows_wave<1|2>, a wave per read segment: eight waves, segments of ceil(windows / 512) * 64 windows
def _wave():
    for n, db in enumerate((Db(21, "min", 60, 1), Db(61, "syn", 31, 1), Db(21, "min", 7, 2))):   # w = 60 and 2 (k - s) = 60: the last the wave form takes
        k, m = db.k, MODES[db.mode]
        base = (k + db.ws - 2) if db.mode == "min" else (2 * k - db.ws - 2)
        g, h = rnd(9000, 600 + n), rnd(9000, 610 + n)
        reads = [g[:w + base] for w in (2560, 2561, 3072, 3073)] + [g[:9000], b"A" * 3000, (LOWC * 300)[:2999], g[9:309], put(g[:4000], 2000, b"N" * 70)]
        add("wave-%s" % _tag(db), db, reads, x_wave(m, 9), u=256, u_both=True, seam="read" if db.scale == 1 else None)
        add("wave-uBIG-%s" % _tag(db), db, reads, x_wave(m, 9))
        r1 = [g[:9000], b"A" * 3000, g[:2560 + base], g[:3000], g[:3000], b"", g[:200]]
        r2 = [g[:9000], b"A" * 3000, h[:2561 + base], h[:20], b"", h[:3000], h[:160]]                      # ... a short and an empty mate 2
        add("wave-pe-%s" % _tag(db), db, r1, x_wave(m, 7), reads2=r2, u=256, u_both=True, seam="mate" if db.scale == 1 else None)
    # closed syncmers the rolling kernel would take, but paired: the wave form alone
    db = Db(21, "syn", 11, 1)
    g, h = rnd(6000, 620), rnd(6000, 621)
    add("wave-pe-%s" % _tag(db), db, [g[:6000], b"A" * 3000, g[:3000], g[:2100], g[:150]], x_wave(2, 5), reads2=[g[:6000], b"A" * 3000, h[:25], b"", h[:100]], u=256, u_both=True,
        seam="mate")
    add("wave-f35-%s" % _tag(db), db, [g[:6000], b"A" * 3000, g[:3000], g[:200]], x_wave(2, 4), flags="35", u=256, u_both=True, seam="read")


# -- WindowsRoll: k1_windows_roll<WSZ, WAVES> with k1_windows_wave<2> behind it for the reads on its list
ROLL_KS = ((21, 15, 12), (21, 13, 16), (21, 11, 20), (31, 19, 24), (31, 15, 32))   # k, s, WSZ = 2 (k - s)
UNREACHABLE = (("k1_windows_roll", 32, 4),)


def _wr_lds(wsz, max_len, waves):
    """1 KiB of tables, then per wave a ring of 16 (WSZ <= 30) or 32 x 64 k-mer hashes and the longest read's 2-bit codes (+ 1280 bases of
    zeros the last steps may read, + 4 words)"""
    words = (max_len + 1280 + 15) // 16 + 4
    return 1024 + waves * ((16 if wsz <= 30 else 32) * 64 * 8 + words * 4)


def _roll():
    for n, (k, s, wsz) in enumerate(ROLL_KS):
        db = Db(k, "syn", s, 1)
        lw = 2 * k - s - 1
        g = rnd(9000, 700 + n)
        # 1024 windows (the fewest the kernel takes) and one more, ~5000 bases; left on the list: an N, a short read, 1023 windows
        few = [g[:lw + 1023], g[:lw + 1024], g[:5000], put(g[1000:4000], 1500, b"N"), g[:400], g[:lw + 1022]]
        for waves in (1, 2, 4):
            if (("k1_windows_roll", wsz, waves)) in UNREACHABLE:
                continue
            reads = list(few)
            if waves == 2:  # soft-masked, low-complexity (runs of equal emissions across the lanes' runs), a homopolymer
                reads += [g[2000:8000].lower(), (LOWC * 700)[:6500] + g[:3000], b"A" * 5000]
            nr = len(reads)
            lds = _wr_lds(wsz, max(len(r) for r in reads), waves)
            add("roll-%d-w%d" % (wsz, waves), db, reads, x_roll(wsz, waves, (nr + waves - 1) // waves, lds, nr), wr_waves=str(waves), u=256, left=3,
                roll_reads=[0, 1, 2] + list(range(6, nr)), seam="read" if waves == 2 else None)
    # -u above some of the reads the kernel could take: they stay with the wave kernel
    db = Db(21, "syn", 11, 1)
    g = rnd(9000, 702)
    reads = [g[:3001], g[:3000], g[:5000], g[:9000], g[:400]]
    add("roll-20-u3000", db, reads, x_roll(20, 2, 3, _wr_lds(20, 9000, 2), 5), u=3000, left=3, roll_reads=[2, 3], u_both=True)
    # FracMinHash, scale 3 (five canonical k-mers in nine are kept)
    db = Db(31, "syn", 15, 3)
    g = rnd(9000, 704)
    reads = [g[:9000], g[:3000], g[2000:3100], put(g[:5000], 4999, b"N"), put(g[:5000], 0, b"n")]   # 1100 bases: enough windows, 498 emissions
    add("roll-32-x3", db, reads, x_roll(32, 2, 3, _wr_lds(32, 9000, 2), 5), u=256, left=3, roll_reads=[0, 1])
    # the LDS limits (tests/k1_plan_check.cpp): the longest read two waves hold, one base more (one wave), the longest read one wave holds
    # (65 536 bytes of dynamic LDS), one base more (no rolling kernel).  FracMinHash keeps the emissions within (512, 65 536].
    db = Db(21, "syn", 11, 8)
    g = rnd(223937, 710)
    add("roll-20-lds-94912", db, [g[:94912]], x_roll(20, 2, 1, 65536, 1), u=256, left=0, roll_reads=[0])
    add("roll-20-lds-94913", db, [g[:94913]], x_roll(20, 1, 1, 33284, 1), u=256, left=0, roll_reads=[0])
    add("roll-20-lds-223936", db, [g[:223936]], x_roll(20, 1, 1, 65536, 1), u=256, left=0, roll_reads=[0])
    add("roll-20-lds-223937", db, [g[:223937]], x_wave(2, 1), u=256)
    db = Db(31, "syn", 15, 1)
    g = rnd(62145, 711)
    add("roll-32-lds-62144", db, [g[:62144]], x_roll(32, 2, 1, 65536, 1), u=256, left=0, roll_reads=[0])
    add("roll-32-lds-62145", db, [g[:62145]], x_roll(32, 1, 1, 33284, 1), u=256, left=0, roll_reads=[0])


# -- whole genomes: one workgroup per 65 536-position segment, then an ordered pack
def _seg():
    g = rnd(200000, 800)
    clean = [g[:140000], g[:200000], g[3:70003].lower(), g[:3000]]                              # 4 reads x 4 segments
    # an N inside the second segment only; a run across the boundary of segments 0 and 1 (both); the last base segment 0's k-mers cover
    # (k = 21: base 65 555) and, in another read, the first one they do not (segment 1 alone)
    dirty = [g[:140000], put(g[:200000], 65536 + 1000, b"N"), put(g[3:70003], 65530, b"N" * 10), g[:3000], put(g[:140000], 65555, b"R"),
             put(g[:140000], 65556, b"n")]                                                          # 6 reads x 4 segments, 1 + 2 + 2 + 1 left
    for db in (Db(21, "plain", 0, 1), Db(21, "plain", 0, 7)):
        t = _tag(db)
        add("seg-roll2-%s" % t, db, dirty, x_seg_roll2(24, 24), left=6)
        add("seg-roll2-clean-%s" % t, db, clean, x_seg_roll2(16, 16), left=0)
        add("seg-roll2-codes-%s" % t, db, dirty, x_seg_roll2(24, 24, codes=True, n_exc_grid=1), codes=True, left=6)
        add("seg-roll2-codes-clean-%s" % t, db, clean, x_seg_roll2(16, 16, codes=True), codes=True, left=0)
    db = Db(21, "plain", 0, 1)
    add("seg-roll-f19", db, dirty, x_seg_roll(24), flags="19")
    add("seg-roll-f19-codes", db, dirty, x_seg_roll(24), flags="19", codes=True)                # expanded whole first: the byte kernel reads text
    add("seg-hash-f11", db, dirty, x_seg_hash(24), flags="11")
    add("seg-roll2-u256-x7", Db(21, "plain", 0, 7), clean + [g[:600]], x_seg_roll2(20, 20), left=0, u=256, u_both=True)
    g8 = rnd(150000, 801)
    big = [g8[:140000], put(g8[:150000], 65536 + 127, b"N"), g8[:65536 + 127], g8[:65536 + 128]]  # 3 segments; k = 128: base 65 663 is the first that segment 0's k-mers do not cover
    add("seg-roll2-k128", Db(128, "plain", 0, 1), big, x_seg_roll2(12, 12), left=1)
    add("seg-hash-k128-f11", Db(128, "plain", 0, 1), big, x_seg_hash(12), flags="11")
    add("seg-hash-k129", Db(129, "plain", 0, 1), big, x_seg_hash(12))
    add("seg-hash-k129-f19", Db(129, "plain", 0, 1), big, x_seg_hash(12), flags="19")             # the byte kernel's halo ends at k = 128


_short()
_wg()
_wg_global()
_wave()
_roll()
_seg()

# the hash-once window kernels (witness only here; every hash, count and qlen they leave is compared with the oracle in
# tests/test_gpu_win_forms.py, case plan tests/win_cases.py)
WIN_ONCE = [("k1_win_hash", 0, 0), ("k1_win_scan", 0, 0), ("k1_win_rank", 0, 0), ("k1_win_gather", 0, 0)]

# every instantiation launch_k1 can be asked for: (kernel, p0, p1)
ALL_KERNELS = sorted(
    [("k1_kmers", m, 0) for m in (0, 1, 2)] + [("k1_kmers_wg", m, 0) for m in (0, 1, 2)] + [("k1_kmers_wg_global", 0, 0)] +
    [("k1_windows_wave", m, 0) for m in (1, 2)] +
    [("k1_windows_roll", wsz, waves) for _, _, wsz in ROLL_KS for waves in (1, 2, 4) if ("k1_windows_roll", wsz, waves) not in UNREACHABLE] +
    [("k1_seg_roll2", 0, 0), ("k1_seg_roll", 0, 0), ("k1_seg_hash", 0, 0), ("k1_seg_pack", 0, 0), ("k_mark_exc", 0, 0), ("k_unpack2_list", 0, 0)] + WIN_ONCE)


def planned_kernels():
    s = set(WIN_ONCE)
    for c in CASES:
        s |= {w[:3] for w in c.expect["kernels"]}
    return sorted(s)
