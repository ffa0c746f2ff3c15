"""The sliding-window test plan of the k-mer stage: the hash-once kernels k1_win_hash / k1_win_scan / k1_win_rank / k1_win_gather (form WinOnce
of kmcp_amd/csrc/k1_win_once.hip), k_window_desc (windows.hip) and the window view (K1Args::src, k1_bases) through which every other K1 form reads
a window's bases in place — with the smallest batches that reach each edge of them, and the witness every case must produce.

A case is a database (open_synthetic: k, sketch mode, w or s, scale), reads with (step, window, greedy), an optional explicit cut of its
windows into pieces — one call of kmcpg_kmers_device_windows each —, -u / -m, and the DECLARED witness: the plan's form and the kernels in
launch order with their template parameters, grids and block sizes.

The staging is stated here in plain Python, from the enumeration rule (windows of a read of L bases start at 0, S, 2S, ... and end at
min(i + W, L); without greedy only windows with i + W <= L exist, with greedy every i < L does) and the documented chunk rule (a staged slice
of n >= k bases holds ceil((n - k + 1) / 1024) chunks of k-mer positions, a shorter one none).  A slice is a run of windows of one read —
the bases from its first window's start to its last window's end — or, where windows do not overlap (S >= W), each window on its own.
Nothing here is read from the library; tests/test_win_cases_cpu.py holds it against window_plan.hpp compiled alone.

The reference is independent of the kernels: per window the oracle's generate_kmers on the window's text read[i:e], sort_unique when the
count exceeds -u; a window shorter than -m has an empty list; qlen = e - i.
tests/test_win_cases_cpu.py checks the plan without a GPU (the conditions that keep a GPU test from passing vacuously);
tests/test_gpu_win_forms.py runs the cases.
"""
import ctypes as C

import numpy as np

from tests.k1_forms_plan import BIG, Db, K1SEG, _wr_lds, is_acgt, put, rnd, roll_left, seg_left, sketch_cfg, x_roll, x_seg_roll2, x_short, x_wave, x_wg, x_wg_global

CHUNK = 1024          # k-mer positions of a slice one wave hashes
SCAN_MAX_K = 65       # the last k of the hash-once form
GATHER_GRID = 65536   # workgroups of four windows: above 262 144 windows k1_win_gather strides
WIN_ONCE = ("k1_win_hash", "k1_win_scan", "k1_win_rank", "k1_win_gather")
NO_LIST = dict(codes_direct=False, list_fallback=False, adj_done=False)


# ---- the enumeration and the staging ------------------------------------------------------------------------------------------------
def windows_of(L, step, window, greedy):
    out, i = [], 0
    while True:
        e = i + window
        if e > L:
            if not greedy or i >= L:
                break
            e = L
        out.append((i, e))
        i += step
    return out


class Staged:
    """what one piece stages: text, the four prefix arrays, and per window (read, i, e), src and koff"""


def stage(reads, step, window, greedy, k, piece):
    """piece: [(read, j0, j1)] — windows [j0, j1) of that read, reads ascending"""
    st = Staged()
    text, soffs, wpre, vpre, cpre, wins, src, koff = [], [0], [0], [0], [0], [], [], [0]

    def slice_(r, ws):
        read = reads[r]
        a0, a1 = ws[0][0], ws[-1][1]
        text.append(read[a0:a1])
        n = a1 - a0
        for i, e in ws:
            wins.append((r, i, e))
            src.append(soffs[-1] + (i - a0))
            koff.append(koff[-1] + (e - i))
        soffs.append(soffs[-1] + n)
        wpre.append(wpre[-1] + len(ws))
        vpre.append(vpre[-1] + sum(e - i for i, e in ws))
        cpre.append(cpre[-1] + (-(-(n - k + 1) // CHUNK) if n >= k else 0))

    for r, j0, j1 in piece:
        ws = windows_of(len(reads[r]), step, window, greedy)[j0:j1]
        assert len(ws) == j1 - j0 > 0
        if step >= window:
            for w in ws:
                slice_(r, [w])
        else:
            slice_(r, ws)
    st.text = b"".join(text)
    st.soffs, st.wpre, st.vpre, st.cpre = (np.array(a, dtype=np.uint64) for a in (soffs, wpre, vpre, cpre))
    st.wins, st.src, st.koff = wins, np.array(src, dtype=np.uint64), np.array(koff, dtype=np.uint64)
    st.n_slices, st.n_win, st.bases, st.n_chunks, st.sb = len(soffs) - 1, len(wins), koff[-1], cpre[-1], soffs[-1]
    st.wmax = max([e - i for _, i, e in wins], default=0)
    st.piece = list(piece)
    return st


# ---- the witness --------------------------------------------------------------------------------------------------------------------
def x_win_once(st):
    """exactly, in order: k1_win_hash (grid ceil(n_chunks / 4), block 256), k1_win_scan (1, 1024), k1_win_rank (as k1_win_hash), k1_win_gather
    (grid ceil(n_windows / 4), 256); without a chunk the gather alone; grids end at 65 536 workgroups"""
    g = min(-(-st.n_chunks // 4), 65536)
    ks = [("k1_win_hash", 0, 0, g, 256, 0), ("k1_win_scan", 0, 0, 1, 1024, 0), ("k1_win_rank", 0, 0, g, 256, 0)] if st.n_chunks else []
    return dict(NO_LIST, form="WinOnce", kernels=ks + [("k1_win_gather", 0, 0, min(-(-st.n_win // 4), GATHER_GRID), 256, 0)])


X_NONE = dict(NO_LIST, form="None", kernels=[])


class Case:
    def __init__(self, id, group, db, reads, step, window, greedy, expect=None, cuts=None, u=BIG, min_qlen=0, whole_read=False, left=None):
        self.id, self.group, self.db, self.reads = id, group, db, list(reads)
        self.step, self.window, self.greedy, self.u, self.min_qlen = step, window, greedy, u, min_qlen
        self.cuts = cuts              # [(w0, w1)]: windows of the batch, one call each; None: all of them in one call
        self.expect = expect          # None: WinOnce (x_win_once of each piece); else a function of the piece's staging
        self.whole_read = whole_read  # the reference is the oracle's list for the whole read, sliced (S = 1, W = k, A/C/G/T only)
        self.left = left              # the list forms: what the first kernel must leave (a function of the piece's windows' texts)
        self._pieces = None

    def pieces(self):
        """the staging of every call"""
        if self._pieces is None:
            per_read = [len(windows_of(len(r), self.step, self.window, self.greedy)) for r in self.reads]
            total = sum(per_read)
            cuts = self.cuts if self.cuts is not None else [(0, total)]
            assert [a for a, _ in cuts] == [0] + [b for _, b in cuts[:-1]] and cuts[-1][1] == total, self.id
            out = []
            for w0, w1 in cuts:
                piece, at = [], 0
                for r, c in enumerate(per_read):
                    lo, hi = max(w0, at), min(w1, at + c)
                    if lo < hi:
                        piece.append((r, lo - at, hi - at))
                    at += c
                out.append(stage(self.reads, self.step, self.window, self.greedy, self.db.k, piece))
            self._pieces = out
        return self._pieces

    def expected(self, st):
        if st.n_win == 0:
            return X_NONE
        return x_win_once(st) if self.expect is None else self.expect(st)

    def win_once(self):
        return self.expect is None


class _Texts:
    """the windows of a piece as the reads of a k1_forms_plan case: what roll_left / seg_left are asked about"""

    def __init__(self, case, st):
        self.db, self.u, self.min_qlen = case.db, case.u, case.min_qlen
        self.reads = [case.reads[r][i:e] for r, i, e in st.wins]


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def reference(case, st, O):
    """per window of the piece (raw count, the list the k-mer stage must leave); qlen is e - i"""
    cfg = sketch_cfg(O, case.db)
    k = case.db.k
    out = []
    if case.whole_read:
        assert case.step == 1 and case.window == k and case.u >= 1 and case.min_qlen <= k
        whole = {}
        for r, i, e in st.wins:
            if r not in whole:
                assert is_acgt(case.reads[r]).all()
                whole[r] = O.generate_kmers(case.reads[r], cfg)
                assert len(whole[r]) == len(case.reads[r]) - k + 1   # one k-mer per position: the list can be sliced by position
            out.append((1, whole[r][i:i + 1]) if e - i == k else (0, whole[r][:0]))
        return out
    L = O.lib()
    buf = np.zeros(max(st.wmax, 1), dtype=np.uint64)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    for r, i, e in st.wins:
        if e - i < case.min_qlen:
            out.append((0, buf[:0].copy()))
            continue
        w = case.reads[r][i:e]
        n = L.ko_generate_kmers(w, len(w), C.byref(cfg), p)
        raw = buf[:n].copy()
        out.append((n, O.sort_unique(raw) if n > case.u else raw))
    return out


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
FILL = -7                                                   # what every output array holds before the call
FILL64 = np.array([FILL], dtype=np.int64).view(np.uint64)[0]
PAD_H = 8                                                   # words behind the hashes, one behind every other array


def compare(st, ref, h, koff, src, nk, ql):
    """what the device left — h uint64[bases + PAD_H], koff uint64[n_win + 1], src uint64 / nk int32 / ql int32 [n_win + 1], all FILL before
    the call — against the staging and the reference: a list of disagreements, empty when every number is right.  No tolerance anywhere."""
    problems = []
    nw = st.n_win
    if nw and not np.array_equal(koff[:nw + 1], st.koff):
        d = int(np.nonzero(koff[:nw + 1] != st.koff)[0][0])
        problems.append("koff[%d] is %d, the staging has %d" % (d, int(koff[d]), int(st.koff[d])))
    if not np.array_equal(src[:nw], st.src):
        d = int(np.nonzero(src[:nw] != st.src)[0][0])
        problems.append("src[%d] is %d, the staging has %d" % (d, int(src[d]), int(st.src[d])))
    if src[nw] != FILL64 or nk[nw] != FILL or ql[nw] != FILL or (nw == 0 and koff[0] != FILL64) or not (h[st.bases:] == FILL64).all():
        problems.append("a word behind the end of an output array was written")
    want_ql = np.array([j - i for _, i, j in st.wins], dtype=np.int32)
    if not np.array_equal(ql[:nw], want_ql):
        d = int(np.nonzero(ql[:nw] != want_ql)[0][0])
        problems.append("window %d %s: qlen %d" % (d, st.wins[d], int(ql[d])))
    want_nk = np.array([len(lst) for _, lst in ref], dtype=np.int32)
    if not np.array_equal(nk[:nw], want_nk):
        d = int(np.nonzero(nk[:nw] != want_nk)[0][0])
        problems.append("window %d %s: NumKmers %d, the oracle has %d (%d raw)" % (d, st.wins[d], int(nk[d]), int(want_nk[d]), ref[d][0]))
    elif nw and want_nk.sum():
        # every list in one comparison: window w's list is h[koff[w] .. koff[w] + nk[w]), with the staging's koff
        want = np.concatenate([lst for _, lst in ref])
        owner = np.repeat(np.arange(nw), want_nk)
        first = np.cumsum(want_nk) - want_nk
        got = h[st.koff[:nw].astype(np.int64)[owner] + (np.arange(len(want)) - first[owner])]
        if not np.array_equal(got, want):
            d = int(np.nonzero(got != want)[0][0])
            w = int(owner[d])
            problems.append("window %d %s: hash %d of %d is %#x, the oracle has %#x (%d lists differ)" %
                            (w, st.wins[w], d - int(first[w]), int(want_nk[w]), int(got[d]), int(want[d]), len(set(owner[got != want].tolist()))))
    return problems


def right_output(st, ref):
    """the arrays compare() finds nothing wrong with (the CPU test perturbs them one number at a time)"""
    nw = st.n_win
    h = np.full(st.bases + PAD_H, FILL64, dtype=np.uint64)
    for w, (_, lst) in enumerate(ref):
        h[int(st.koff[w]):int(st.koff[w]) + len(lst)] = lst
    koff = np.full(nw + 1, FILL64, dtype=np.uint64)
    if nw:
        koff[:] = st.koff
    src = np.append(st.src, FILL64).astype(np.uint64)
    nk = np.array([len(lst) for _, lst in ref] + [FILL], dtype=np.int32)
    ql = np.array([j - i for _, i, j in st.wins] + [FILL], dtype=np.int32)
    return h, koff, src, nk, ql


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
CASES = []
PLAIN = Db(21, "plain", 0, 1)


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)


def chunk_reads(k, seed):
    """2100 k-mer positions (chunks of 1024, 1024, 52) and two more: with S = 7, W = k + 1023 the first has (L - W) % S = 5, the second 0"""
    g = rnd(2102 + k - 1, seed)
    return [g[:2100 + k - 1], g[:2102 + k - 1]]


def _chunk():
    k = 21
    reads = chunk_reads(k, 1000)
    add("chunk-s1-wk", "chunk", PLAIN, reads, 1, k, False)                 # 2100 + 2102 windows of one k-mer
    add("chunk-s1-wk1-g", "chunk", PLAIN, reads, 1, k + 1, True)           # ... of two, and greedy tails down to one base
    add("chunk-s7-w1044", "chunk", PLAIN, reads, 7, k + 1023, False)       # 1024 positions a window


TILE_POS = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 2049)


def _tile():
    k = 21
    g = rnd(2049 + k - 1, 1010)
    add("tile", "tile", PLAIN, [g[:n + k - 1] for n in TILE_POS], 3, k + 5, True)


SCAN_CHUNKS = (1023, 1024, 1025, 2049, 3000)


def scan_reads(n_chunks, seed, k=21):
    """reads of k .. k + 9 bases (one chunk each), every 50th shorter than k (none), until the batch holds n_chunks"""
    rng = np.random.default_rng(seed)
    g = rnd(40000, seed + 1)
    reads = []
    while n_chunks:
        short = len(reads) % 50 == 49
        L = int(rng.integers(5, k)) if short else int(rng.integers(k, k + 10))
        at = int(rng.integers(0, len(g) - 40))
        reads.append(g[at:at + L])
        n_chunks -= 0 if short else 1
    return reads


def _scan():
    db = Db(21, "plain", 0, 3)
    for n in SCAN_CHUNKS:
        add("scan-%d" % n, "scan", db, scan_reads(n, 1100 + n), 2, 23, True)


def _none():
    g = rnd(400, 1020)
    short = [g[7 * L:7 * L + L] for L in range(1, 21)]
    add("none-greedy", "none", PLAIN, short, 3, 26, True)                    # windows, but no k-mer position anywhere
    add("none-no-window", "none", PLAIN, short, 3, 26, False)                # no window at all


def _k():
    for k in (31, 64, 65):
        add("k%d" % k, "k", Db(k, "plain", 0, 1), chunk_reads(k, 1030 + k), 7, k + 1023, True)
    db = Db(66, "plain", 0, 1)
    reads = chunk_reads(66, 1036)
    add("k66-w150", "k", db, reads, 50, 150, True, expect=lambda st: x_short(0, -(-st.n_win // 4)))
    add("k66-w3000", "k", db, [rnd(7000, 1037)], 1000, 3000, True, expect=lambda st: x_wg(0, st.n_win, False))


def _frac():
    for scale in (5, 1000):
        db = Db(21, "plain", 0, scale)
        reads = chunk_reads(21, 1040)
        add("frac-x%d-s1-wk" % scale, "frac", db, reads, 1, 21, False)
        add("frac-x%d-s7-w1044-g" % scale, "frac", db, reads, 7, 1044, True)


def _u_m():
    g = rnd(3000, 1050)
    reads = [g[:1000], put(g[1000:2000], 500, b"N"), g[2000:3000]]             # 130 k-mers a window; the greedy tails have 80 and 30
    for u in (64, 129, 130):
        add("u%d" % u, "u-m", PLAIN, reads, 50, 150, True, u=u)
    add("m100-g", "u-m", PLAIN, reads, 50, 150, True, min_qlen=100)            # the tails of 100 and 50 bases: at -m, and k <= len < -m
    add("m100-g-u90", "u-m", PLAIN, reads, 50, 150, True, min_qlen=100, u=90)


def _pieces():
    add("pieces", "pieces", PLAIN, [rnd(5000, 1060)], 100, 300, False, cuts=[(0, 17), (17, 18), (18, 48)])


GATHER_WINDOWS = 262145


def _gather_loop():
    add("gather-loop", "gather-loop", PLAIN, [rnd(GATHER_WINDOWS + 20, 1070)], 1, 21, False, whole_read=True)


# -- the window view in the other forms: each read has one N run and one lower-case stretch
def view_read(n, seed, n_at, n_len, low_at, low_len=300):
    g = rnd(n, seed)
    g = put(g, n_at, b"N" * n_len)
    return put(g, low_at, g[low_at:low_at + low_len].lower())


def _view():
    r1 = view_read(1000, 1080, 400, 3, 600, 120)
    for db, mode in ((Db(21, "min", 5, 1), 1), (Db(21, "syn", 11, 1), 2)):
        for step in (50, 150, 170):                                                                # S < W, S = W, S > W
            add("view-short-%s%d-s%d" % (db.mode, db.ws, step), "view", db, [r1, r1[:333]], step, 150, True,
                expect=lambda st, mode=mode: x_short(mode, -(-st.n_win // 4)))
    r2 = view_read(10000, 1081, 4000, 5, 7000)
    add("view-wg-plain", "view", PLAIN, [r2], 3000, 3000, True, expect=lambda st: x_wg(0, st.n_win, False))
    add("view-wg-min61", "view", Db(21, "min", 61, 1), [r2], 1000, 2500, True, expect=lambda st: x_wg(1, st.n_win, True), u=256)
    add("view-wave-min7", "view", Db(21, "min", 7, 1), [r2], 1000, 3000, True, expect=lambda st: x_wave(1, st.n_win), u=256)
    r3 = view_read(12000, 1082, 6000, 4, 300)
    add("view-roll-syn11", "view", Db(21, "syn", 11, 1), [r3], 500, 5000, False, u=256,
        expect=lambda st: x_roll(20, 2, (st.n_win + 1) // 2, _wr_lds(20, 5000, 2), min(st.n_win, 1024)),
        left=lambda case, st, ref: len(roll_left(_Texts(case, st), [(np.zeros(n),) for n, _ in ref])))   # (roll_left asks for the raw counts only)
    add("view-wgglobal-min511", "view", Db(21, "min", 511, 1), [r2], 1500, 3000, True, expect=lambda st: x_wg_global(st.n_win), u=256)
    # an N run across position 65 536 of the second window (read position 70 000 + 65 536), lower case in the first
    r4 = view_read(150000, 1083, 70000 + K1SEG - 6, 16, 30000, 2000)
    add("view-seg-roll2", "view", PLAIN, [r4], 70000, 70000, True, expect=lambda st: x_seg_roll2(2 * st.n_win, 2 * st.n_win),
        left=lambda case, st, ref: seg_left(_Texts(case, st)))


VIEW_FORMS = ("Short", "Wg", "WindowsWave", "WindowsRoll", "WgGlobal", "SegRoll2")

_chunk()
_tile()
_scan()
_none()
_k()
_frac()
_u_m()
_pieces()
_gather_loop()
_view()

GROUPS = ("chunk", "tile", "scan", "none", "k", "frac", "u-m", "pieces", "gather-loop", "view")
assert {c.group for c in CASES} == set(GROUPS)
