"""The sliding-window test plan (tests/win_cases.py) checked without a GPU, so that tests/test_gpu_win_forms.py cannot pass vacuously:

  * from the oracle and the plan's own staging alone: the positions, lane counts and chunk counts each group names really occur; each -u
    case has windows on the side it names (and sorting changes their lists); the scale-1000 case has empty and non-empty windows and chunks
    with nothing kept; the scan cases have unequal chunk counts; every view case has a window over its N run and one over its lower-case
    stretch, and the list forms leave some but not all; no case other than the group `none` has nothing but empty lists;
  * the Python staging of every piece equals the header's: kmcp_amd/csrc/window_plan.hpp compiled alone (tests/win_cases_print.cpp, g++ with
    ASan/UBSan) prints stage_windows and window_desc_at for the case's piece cuts; text, soffs, wpre, vpre, cpre, src, koff, the longest
    window and the totals are compared number for number."""
import os
import subprocess

import numpy as np
import pytest

from tests import win_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMS = {1023, 1024, 1025, 2047, 2048, 2049}


def group(name):
    cs = [c for c in P.CASES if c.group == name]
    assert cs, name
    return cs


@pytest.fixture(scope="module")
def refs(oracle_lib):
    cache = {}

    def get(c):
        if c.id not in cache:
            cache[c.id] = [P.reference(c, st, oracle_lib) for st in c.pieces()]
        return cache[c.id]
    return get


def positions(c):
    """per window of every piece: (first k-mer position in its slice, one past its last, positions of the slice); np <= 0: (p, p, npos)"""
    out = []
    for st in c.pieces():
        q = np.searchsorted(st.wpre, np.arange(st.n_win), side="right") - 1
        for w, (r, i, e) in enumerate(st.wins):
            p = int(st.src[w] - st.soffs[q[w]])
            npos = int(st.soffs[q[w] + 1] - st.soffs[q[w]]) - c.db.k + 1
            out.append((p, p + max(e - i - c.db.k + 1, 0), npos))
    return out


def test_ids_and_forms():
    assert len({c.id for c in P.CASES}) == len(P.CASES)
    for c in P.CASES:
        once = c.db.mode == "plain" and c.db.k <= P.SCAN_MAX_K and c.step < c.window
        assert c.win_once() == once, c.id
        for st in c.pieces():
            assert (c.expected(st)["form"] == "WinOnce") == (once and st.n_win > 0), c.id
    assert {c.group for c in P.CASES if not c.win_once()} == {"k", "view"}


def test_chunk_group_reaches_the_seams():
    first, last, exact, one_before, tails = set(), set(), 0, 0, 0
    for c in group("chunk"):
        assert [int(x) for x in np.diff(c.pieces()[0].cpre)] == [3, 3] and len(c.reads[0]) - c.db.k + 1 == 2100
        for p, e, npos in positions(c):
            first.add(p)
            last.add(e)
            exact += e == npos and e > p
            one_before += e == npos - 1 and e > p
            tails += e == p
    assert SEAMS <= first and SEAMS <= last and exact and one_before and tails
    c = [c for c in group("chunk") if c.step == 7][0]
    assert sorted((len(r) - c.window) % c.step == 0 for r in c.reads) == [False, True]
    assert {e == npos for p, e, npos in positions(c)} == {False, True}


def test_tile_group_lane_counts():
    (c,) = group("tile")
    st = c.pieces()[0]
    npos = [int(x) - c.db.k + 1 for x in np.diff(st.soffs)]
    assert tuple(npos) == P.TILE_POS
    assert {1, 2, 63, 0, 65 % 64} <= {n % 64 for n in npos}
    assert [n for n in npos if n > P.CHUNK and (n - 1) % P.CHUNK == 0] == [1025, 2049]   # a last chunk of one position
    assert [int(x) for x in np.diff(st.cpre)] == [-(-n // P.CHUNK) for n in npos]


def test_scan_group(oracle_lib):
    pers = set()
    idle = partial = False
    for c, want in zip(group("scan"), P.SCAN_CHUNKS):
        (st,) = c.pieces()
        n = st.n_chunks
        assert n == want and st.n_win > 256 and c.db.scale == 3
        per = -(-n // 1024)
        pers.add(per)
        idle |= 1023 * per >= n           # the last thread (and more) with lo == hi == n
        partial |= n % per != 0           # a thread that holds fewer than `per`
        d = np.diff(st.cpre)
        assert set(d.tolist()) == {0, 1} and (d[:-1] == 0).sum() >= n // 50 - 1 and d[-1] == 1   # zero-chunk slices inside cpre
        cfg = P.sketch_cfg(oracle_lib, c.db)
        kept = [len(oracle_lib.generate_kmers(r, cfg)) for r in c.reads if len(r) >= c.db.k]
        assert len(kept) == n and len(set(kept)) > 2 and 0 in kept, c.id   # unequal chunk counts, some chunks with nothing kept
    assert pers == {1, 2, 3} and idle and partial


def test_none_group(refs):
    a, b = group("none")
    (st,) = a.pieces()
    assert st.n_win > 4 and st.n_chunks == 0 and a.greedy and all(len(r) < a.db.k for r in a.reads)
    assert all(len(lst) == 0 for _, lst in refs(a)[0])
    assert a.expected(st)["kernels"] == [("k1_win_gather", 0, 0, -(-st.n_win // 4), 256, 0)]
    (st,) = b.pieces()
    assert st.n_win == 0 and st.n_slices == 0 and b.expected(st) == P.X_NONE


def test_k_group():
    ks = sorted(c.db.k for c in group("k"))
    assert ks == [31, 64, 65, 66, 66] and P.SCAN_MAX_K == 65
    for c in group("k"):
        assert c.step < c.window, c.id
        if c.db.k == 66:
            assert {c.expected(st)["form"] for st in c.pieces()} <= {"Short", "Wg"}
    assert {c.expected(c.pieces()[0])["form"] for c in group("k") if c.db.k == 66} == {"Short", "Wg"}
    assert {c.window for c in group("k") if c.db.k == 66} == {150, 3000}


def test_frac_group(refs, oracle_lib):
    for c in group("frac"):
        (ref,) = refs(c)
        n = np.array([len(lst) for _, lst in ref])
        assert (n > 0).any(), c.id
        plain = P.sketch_cfg(oracle_lib, P.PLAIN)
        cfg = P.sketch_cfg(oracle_lib, c.db)
        all_, kept = oracle_lib.generate_kmers(c.reads[0], plain), oracle_lib.generate_kmers(c.reads[0], cfg)
        assert 0 < len(kept) < len(all_), c.id                                  # the filter keeps some and drops some
        if c.db.scale == 1000:
            assert (n == 0).any() and (n > 0).any(), c.id
            per_chunk = [np.isin(all_[a:a + P.CHUNK], kept).sum() for a in range(0, len(all_), P.CHUNK)]
            assert 0 in per_chunk, (c.id, per_chunk)                            # a chunk with nothing kept


def test_u_and_m_cases_have_windows_on_the_side_they_name(refs, oracle_lib):
    seen = set()
    for c in group("u-m"):
        (st,), (ref,) = c.pieces(), refs(c)
        raw = np.array([n for n, _ in ref])
        lens = np.array([e - i for _, i, e in st.wins])
        assert raw.max() == 130, c.id
        if c.u < P.BIG:
            above = raw > c.u
            assert above.any() == (c.u < 130) and (raw == 130).any(), c.id        # strictly above -u only
            assert (~above & (raw > 0)).any(), c.id                                # ... and lists that stay as they are
            for w in np.nonzero(above)[0][:3]:                                    # sorting is visible: the raw list is not in order
                r, i, e = st.wins[w]
                assert not np.array_equal(ref[w][1], oracle_lib.generate_kmers(c.reads[r][i:e], P.sketch_cfg(oracle_lib, c.db))), c.id
            seen.add(c.u)
        if c.min_qlen:
            assert c.greedy and c.min_qlen == 100
            cut = (lens >= c.db.k) & (lens < c.min_qlen)
            assert cut.any() and (raw[cut] == 0).all() and (lens == c.min_qlen).any() and (raw[lens == c.min_qlen] > 0).all(), c.id
            seen.add("m")
    assert seen == {64, 90, 129, 130, "m"}


def test_pieces_and_gather_loop_shapes():
    (c,) = group("pieces")
    sts = c.pieces()
    assert [st.piece for st in sts] == [[(0, 0, 17)], [(0, 17, 18)], [(0, 18, 48)]] and c.win_once()
    assert [int(st.soffs[1]) for st in sts] == [16 * 100 + 300, 300, 29 * 100 + 300]
    (c,) = group("gather-loop")
    (st,) = c.pieces()
    assert st.n_win == P.GATHER_WINDOWS > 4 * P.GATHER_GRID and c.expected(st)["kernels"][3][3] == P.GATHER_GRID
    assert st.n_chunks < 262144   # (the chunk passes do not stride: see the GPU test's docstring)


def test_view_group(refs):
    forms = set()
    for c in group("view"):
        (st,), (ref,) = c.pieces(), refs(c)
        e = c.expected(st)
        forms.add(e["form"])
        texts = [c.reads[r][i:j] for r, i, j in st.wins]
        assert any(b"N" in t for t in texts) and any(t != t.upper() for t in texts) and any(b"N" not in t for t in texts), c.id
        assert (c.left is not None) == (e["form"] in ("WindowsRoll", "SegRoll2")), c.id
        if c.left is not None:
            n_units = st.n_win if e["form"] == "WindowsRoll" else e["kernels"][0][3]
            assert 0 < c.left(c, st, ref) < n_units, (c.id, c.left(c, st, ref))
    assert forms == set(P.VIEW_FORMS)
    short = [c for c in group("view") if c.expected(c.pieces()[0])["form"] == "Short"]
    assert {(c.db.mode, c.step < c.window) for c in short} == {("min", True), ("min", False), ("syn", True), ("syn", False)}
    seg = [c for c in group("view") if c.expected(c.pieces()[0])["form"] == "SegRoll2"][0]
    r, i, e = seg.pieces()[0].wins[1]
    assert b"N" in seg.reads[r][i + 65530:i + 65536] and b"N" in seg.reads[r][i + 65536:i + 65546]   # an N run across position 65 536 of a window


def test_no_case_compares_empty_lists_only(refs):
    """a cap, not a measurement: outside the group `none` every case (and every call of it) has a window with k-mers"""
    for c in P.CASES:
        for st, ref in zip(c.pieces(), refs(c)):
            if c.group != "none":
                assert any(len(lst) for _, lst in ref), c.id
            assert len(ref) == st.n_win


def test_the_comparison_sees_one_wrong_number(refs):
    """compare() (what the GPU test asserts with) on outputs built from the reference: nothing to report; then one number changed at a time —
    the low bit of the hash at a chunk's last position in a window, two neighbours of a list swapped, a count, a qlen, a src, a koff, a word
    behind an array's end — each is reported"""
    by_id = {c.id: c for c in P.CASES}
    for c in P.CASES:
        for st, ref in zip(c.pieces(), refs(c)):
            assert P.compare(st, ref, *P.right_output(st, ref)) == [], c.id
    c = by_id["chunk-s7-w1044"]
    (st,), (ref,) = c.pieces(), refs(c)
    w = [w for w, (p, e, npos) in enumerate(positions(c)) if p <= 1023 < e][-1]     # a window over position 1023 of its slice
    at = int(st.koff[w]) + (1023 - positions(c)[w][0])

    def wrong(edit):
        out = [a.copy() for a in P.right_output(st, ref)]
        edit(*out)
        return P.compare(st, ref, *out)

    def flip(h, *_):
        h[at] ^= np.uint64(1)

    def swap(h, *_):
        h[at - 1], h[at] = h[at], h[at - 1]

    def beyond(h, *_):
        h[st.bases] = 0
    assert len(wrong(flip)) == 1 and "window %d " % w in wrong(flip)[0]
    assert len(wrong(swap)) == 1 and len(wrong(beyond)) == 1
    for i, name in ((1, "koff"), (2, "src"), (3, "NumKmers"), (4, "qlen")):
        def one(*out, i=i):
            out[i][w] += 1
        got = wrong(one)
        assert len(got) == 1 and name in got[0], (name, got)

        def end(*out, i=i):   # koff's last word is offs[n_win]; the others' is the word behind their end
            out[i][-1] = 0
        assert len(wrong(end)) == 1, name


# ---- the plan's staging against window_plan.hpp ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_staging(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("win_cases") / "win_cases_print")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "win_cases_print.cpp")], check=True)
    lines, ids = [], []
    for c in P.CASES:
        for n, st in enumerate(c.pieces()):
            ids.append("%s/%d" % (c.id, n))
            f = [ids[-1], c.db.k, c.step, c.window, int(c.greedy), len(c.reads)] + [len(r) for r in c.reads] + [len(st.piece)] + [x for sl in st.piece for x in sl]
            lines.append(" ".join(str(x) for x in f))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = {}
    for ln in r.stdout.splitlines():
        key, _, rest = ln.partition(" ")
        if key == "piece":
            f = rest.split()
            cur = out[f[0]] = dict(n_win=int(f[1]), bases=int(f[2]), wmax=int(f[3]))
        elif key == "copies":
            cur[key] = [tuple(int(v) for v in x.split(":")) for x in rest.split()]
        else:
            cur[key] = np.array(rest.split(), dtype=np.uint64)
    assert sorted(out) == sorted(ids)
    return out


def test_python_staging_equals_the_headers(header_staging):
    n_pieces = 0
    for c in P.CASES:
        batch = b"".join(c.reads)
        for n, st in enumerate(c.pieces()):
            h = header_staging["%s/%d" % (c.id, n)]
            what = (c.id, n)
            assert (h["n_win"], h["bases"], h["wmax"]) == (st.n_win, st.bases, st.wmax), what
            assert b"".join(batch[a:a + ln] for a, ln in h["copies"]) == st.text and len(h["copies"]) == st.n_slices, what
            for key in ("soffs", "wpre", "vpre", "cpre", "src", "koff"):
                assert np.array_equal(h[key], getattr(st, key)), (what, key)
            assert (int(st.soffs[-1]), int(st.wpre[-1]), int(st.vpre[-1]), int(st.cpre[-1])) == (st.sb, st.n_win, st.bases, st.n_chunks), what
            n_pieces += 1
    assert n_pieces == len(P.CASES) + 2
