"""Sliding windows of long queries on the GPU (kmcpg_submit_windows / kmcpg_submit_packed_windows, kmcp-search --sliding-*): every window
is an ordinary query, so the result must be, bit for bit, what kmcpg_submit gives on the same windows cut into text on the host — qlen,
qkmers, ksize, the CSR offsets and every Match field — in plain, FracMinHash, Closed Syncmer, Minimizer and multi-k databases, over reads
with N runs and IUPAC bytes, windows at every boundary case (shorter than W, cut at the end with greedy, S < W, S = W, S > W), windows
above -u (dedup), windows above 2048 bases (the long-query k-mer kernels) and above one 65 536-position segment (whole-genome kernels).
A sample of windows is checked against the oracle; the CLI output equals kmcp-search on a FASTA of the windows byte for byte."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")


def windows_of(L, step, window, greedy):
    out = []
    i = 0
    while True:
        e = i + window
        if e > L:
            if not greedy or i >= L:
                break
            e = L
        out.append((i, e))
        i += step
    return out


def materialize(reads, step, window, greedy):
    return [r[i:e] for r in reads for (i, e) in windows_of(len(r), step, window, greedy)]


def _reads(genomes, seed, long_len=3000):
    rng = np.random.default_rng(seed)
    base = synth.sample_reads(genomes, 10, long_len, sub_rate=0.005, seed=seed, frac_random=0.1)
    base += synth.sample_reads(genomes, 6, 300, sub_rate=0.005, seed=seed + 1, frac_random=0.0)   # = W of -W 300
    base += [genomes[0][100:399], genomes[1][500:801], genomes[2][7:157], genomes[3][9:221], genomes[4][3:14]]  # W - 1, W + 1, ...
    base.append(genomes[5][1000:21000])                                                           # one 20-kb read
    out = []
    for i, r in enumerate(base):
        b = bytearray(r)
        if i % 4 == 1 and len(b) > 200:
            for _ in range(3):  # N runs
                p = int(rng.integers(0, len(b) - 60))
                ln = int(rng.integers(1, 50))
                b[p:p + ln] = b"N" * ln
        elif i % 4 == 2:
            for p in rng.integers(0, len(b), size=max(1, len(b) // 150)):  # IUPAC codes, lower case
                b[int(p)] = int(rng.choice(list(b"RYKMSWBDHVnacgt")))
        out.append(bytes(b))
    return out


SPECS = [(100, 300, False), (100, 300, True), (1000, 212, True), (4, 150, False), (300, 300, False), (500, 200, True), (700, 3000, True)]


def _same(a, b, what):
    assert len(a.qlen) == len(b.qlen), what
    assert np.array_equal(a.qlen, b.qlen), what
    assert np.array_equal(a.qkmers, b.qkmers), what
    assert np.array_equal(a.ksize, b.ksize), what
    assert np.array_equal(a.offs, b.offs), what
    if hasattr(a, "matches"):
        assert a.matches.tobytes() == b.matches.tobytes(), what
    else:
        assert a.pairs.tobytes() == b.pairs.tobytes(), what


def _check_db(db, reads, specs, params, tag):
    from kmcp_amd import lib
    seqs, offs = lib.pack_reads(reads)
    codes, exc, _ = lib.pack2(reads)
    n_rows = 0
    for (S, W, g) in specs:
        wins = materialize(reads, S, W, g)
        ws, wo = lib.pack_reads(wins)
        want = db.wait(db.submit(ws, wo, params=params))
        got = db.wait(db.submit_windows(seqs, offs, S, W, g, params))
        _same(got, want, f"{tag} text -s {S} -W {W} g={g}")
        got_p = db.wait(db.submit_packed_windows(codes, offs, exc, S, W, g, params))
        _same(got_p, want, f"{tag} packed -s {S} -W {W} g={g}")
        want_pairs = db.wait_pairs(db.submit(ws, wo, params=params))
        got_pairs = db.wait_pairs(db.submit_windows(seqs, offs, S, W, g, params))
        _same(got_pairs, want_pairs, f"{tag} pairs -s {S} -W {W} g={g}")
        rd, st = lib.window_locate(offs, S, W, g)
        assert len(rd) == len(wins) == len(got.qlen)
        for q in range(0, len(wins), max(1, len(wins) // 13)):
            assert reads[rd[q]][st[q]:st[q] + len(wins[q])] == wins[q]
        n_rows += len(wins)
    return n_rows


@pytest.fixture(scope="module")
def genomes():
    return synth.random_genomes(6, 30000, seed=41)


@pytest.mark.parametrize("mode", ["plain", "frac", "syncmer", "minimizer"])
def test_windows_equal_materialized_windows(oracle_lib, tmp_path, genomes, mode):
    from kmcp_amd import Database, default_params
    kw = {"plain": {}, "frac": {"scale": 4}, "syncmer": {"syncmer_s": 11}, "minimizer": {"minimizer_w": 10}}[mode]
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=3, overlap=150, threads=3, **kw)
    reads = _reads(genomes, 3)
    odb = oracle_lib.OracleDB(db_dir)
    with Database.open(db_dir) as db:
        n = _check_db(db, reads, SPECS, default_params(), mode)
        assert n > 1000
        # -u below the windows' k-mer counts (every window through the dedup kernels), -n, -S, -s tcov
        _check_db(db, reads, [(100, 300, True), (50, 3000, False)], default_params(dedup_threshold=64, top_n_scores=2), mode + " -u 64 -n 2")
        _check_db(db, reads, [(100, 300, False)], default_params(do_not_sort=1), mode + " -S")
        _check_db(db, reads, [(100, 300, False)], default_params(sort_by=1, min_qcov=0.3), mode + " -s tcov -t 0.3")
        # a sample of windows against the oracle
        from kmcp_amd import lib
        seqs, offs = lib.pack_reads(reads)
        for (S, W, g) in [(100, 300, True), (4, 150, False)]:
            wins = materialize(reads, S, W, g)
            got = db.wait(db.submit_windows(seqs, offs, S, W, g, default_params()))
            hits = 0
            for q in range(0, len(wins), max(1, len(wins) // 40)):
                want = synth.oracle_tuples(odb, wins[q])
                have = synth.gpu_tuples(got, q)
                assert have[:3] == want[:3], f"{mode} window {q}"
                assert have[4] == want[4]
                hits += len(want[2])
            assert hits > 0
        # the witness (Database.last_k1_launches): overlapping windows of plain / FracMinHash k-mers ran the four hash-once kernels and
        # nothing else of K1; windows that do not overlap (step >= window), and the window sketches, did not run them
        db.set_profiling(1)
        try:
            win_once = ["k1_win_hash", "k1_win_scan", "k1_win_rank", "k1_win_gather"]
            for (S, W, g) in [(100, 300, True), (300, 300, False), (500, 200, True)]:
                db.wait(db.submit_windows(seqs, offs, S, W, g, default_params()))
                ran = [w[0] for w in db.last_k1_launches()]
                plan = db.last_k1_plan()
                assert plan["left_on_list"] is None, plan  # nothing is read back on the asynchronous path
                if mode in ("plain", "frac") and S < W:
                    assert plan["form"] == "WinOnce" and ran == win_once, (mode, S, W, plan, ran)
                else:
                    assert plan["form"] != "WinOnce" and ran and not set(ran) & set(win_once), (mode, S, W, plan, ran)
        finally:
            db.set_profiling(0)
        assert db.last_k1_launches() == [] and db.last_k1_plan() is None
    odb.close()


def test_windows_above_one_segment(oracle_lib, tmp_path):
    """windows longer than 65 536 k-mer positions: plain k-mers go through the whole-genome segment kernels, read in place"""
    from kmcp_amd import Database, default_params
    gs = synth.random_genomes(4, 200000, seed=5)
    db_dir = synth.make_db(tmp_path / "db", gs, k=21, n_chunks=2, overlap=150, threads=2)
    reads = [gs[0][:150000], gs[1][1000:190000] + b"N" * 40 + gs[2][:30000]]
    with Database.open(db_dir) as db:
        _check_db(db, reads, [(30000, 70000, True), (50000, 100000, False)], default_params(), "segments")


def test_multi_k_database(oracle_lib, tmp_path, genomes):
    """several k-mer sizes: the windows without a match are searched again with the smaller k (host-cut text), an explicit k reads in place"""
    import re
    from kmcp_amd import Database, default_params
    O = oracle_lib
    cols = []
    for gi, g in enumerate(genomes):
        h = np.concatenate([O.generate_kmers(g, O.sketch_cfg(k=k)) for k in (21, 31)])
        cols.append((f"g{gi}", len(g), 0, 1, O.sort_unique(h)))
    db_dir = O.build_db(str(tmp_path), O.sketch_cfg(k=31), cols, num_hashes=1, fpr=0.3, threads=2)
    yml = open(db_dir + "/__db.yml").read()
    open(db_dir + "/__db.yml", "w").write(re.sub(r"ks:\n- 31\n", "ks:\n- 21\n- 31\n", yml))
    reads = _reads(genomes, 9)
    rng = np.random.default_rng(1)
    for i in (0, 3, 5):  # a substitution every 24 bases: no intact 31-mer, the 21-mers answer
        b = bytearray(reads[i])
        for j in range(int(rng.integers(0, 24)), len(b), 24):
            b[j] = ord("A") if b[j] != ord("A") else ord("C")
        reads[i] = bytes(b)
    with Database.open(db_dir) as db:
        _check_db(db, reads, [(100, 300, True), (4, 150, False)], default_params(), "multi-k")
        _check_db(db, reads, [(100, 300, False)], default_params(k=21), "multi-k k=21")


def test_windows_over_several_pieces(oracle_lib, tmp_path, genomes):
    """one read whose windows exceed what a batch may hold (KMCPG_TEST_MAX_BASES: the fake ENOMEM of the test hooks) is cut into pieces by
    the library — more pieces than the handle has lanes — and answered as when it fits"""
    from kmcp_amd import Database, default_params, lib
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=3, overlap=150, threads=3, syncmer_s=11)
    reads = _reads(genomes, 4)
    seqs, offs = lib.pack_reads(reads)
    with Database.open(db_dir) as db:
        full = db.wait(db.submit_windows(seqs, offs, 4, 150, False, default_params()))
        full_p = db.wait_pairs(db.submit_windows(seqs, offs, 4, 150, False, default_params()))
        os.environ["KMCPG_TEST_MAX_BASES"] = "60000"
        try:
            cut = db.wait(db.submit_windows(seqs, offs, 4, 150, False, default_params()))
            cut_p = db.wait_pairs(db.submit_windows(seqs, offs, 4, 150, False, default_params()))
            t1 = db.submit_windows(seqs, offs, 100, 300, True, default_params())  # a second ticket in flight beside a cut one
            cut2 = db.wait(db.submit_windows(seqs, offs, 4, 150, False, default_params()))
            w1 = db.wait(t1)
        finally:
            del os.environ["KMCPG_TEST_MAX_BASES"]
        _same(cut, full, "pieces")
        _same(cut_p, full_p, "pieces, pairs")
        _same(cut2, full, "pieces beside another ticket")
        _same(w1, db.wait(db.submit_windows(seqs, offs, 100, 300, True, default_params())), "the other ticket")
    n, b = lib.window_count(offs, 4, 150, False)
    assert b > 10 * 60000 and len(full.qlen) == n


def test_paged_and_device_list_handles(oracle_lib, tmp_path, genomes):
    from kmcp_amd import Database, default_params, lib
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=3, overlap=150, threads=3)
    reads = _reads(genomes, 6)
    seqs, offs = lib.pack_reads(reads)
    codes, exc, _ = lib.pack2(reads)
    with Database.open(db_dir) as db:
        want = {s: db.wait(db.submit_windows(seqs, offs, *s, default_params())) for s in [(100, 300, True), (4, 150, False)]}
    for opener in (lambda: Database.open_paged(db_dir, device=0, passes=2), lambda: Database.open_devices(db_dir, [0])):
        with opener() as db:
            for s, w in want.items():
                _same(db.wait(db.submit_windows(seqs, offs, *s, default_params())), w, f"handle {s}")
                _same(db.wait(db.submit_packed_windows(codes, offs, exc, *s, default_params())), w, f"handle packed {s}")


def _run(args):
    r = subprocess.run([CLI] + args, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r


@pytest.mark.parametrize("gz", [False, True])
def test_cli_equals_search_of_the_window_fasta(oracle_lib, tmp_path, genomes, gz):
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=3, overlap=150, threads=3)
    reads = _reads(genomes, 8)
    ids = [f"r{i}" for i in range(len(reads))]
    with open(tmp_path / "reads.fa", "w") as fh:
        for i, r in zip(ids, reads):
            fh.write(f">{i} some description\n{r.decode()}\n")
    ext = ".tsv.gz" if gz else ".tsv"
    for (S, W, g) in [(100, 300, False), (100, 300, True), (1000, 212, True), (4, 150, False)]:
        with open(tmp_path / "win.fa", "w") as fh:
            for i, r in zip(ids, reads):
                for (a, e) in windows_of(len(r), S, W, g):
                    fh.write(f">{i}_sliding:{a + 1}-{e}\n{r[a:e].decode()}\n")
        for extra in ([], ["-K", "-n", "2"]):
            common = ["-d", str(tmp_path / "db"), "-q", "-j", "4", "--gpu-batch", "1000000"] + extra
            flags = ["--sliding-step", str(S), "--sliding-window", str(W)] + (["--sliding-greedy"] if g else [])
            _run(common + flags + [str(tmp_path / "reads.fa"), "-o", str(tmp_path / ("a" + ext))])
            _run(common + [str(tmp_path / "win.fa"), "-o", str(tmp_path / ("b" + ext))])
            a = open(tmp_path / ("a" + ext), "rb").read()
            b = open(tmp_path / ("b" + ext), "rb").read()
            assert a == b, f"-s {S} -W {W} g={g} {extra}"
            text = (gzip.decompress(a) if gz else a).decode()
            assert f"# input queries: {sum(len(windows_of(len(r), S, W, g)) for r in reads)}\n" in text
            assert "_sliding:" in text
    # batches of a few windows: queryIdx and the trailer still count windows across batches
    flags = ["--sliding-step", "100", "--sliding-window", "300"]
    with open(tmp_path / "win.fa", "w") as fh:
        for i, r in zip(ids, reads):
            for (a, e) in windows_of(len(r), 100, 300, False):
                fh.write(f">{i}_sliding:{a + 1}-{e}\n{r[a:e].decode()}\n")
    _run(["-d", str(tmp_path / "db"), "-q", "-K", "--gpu-batch", "7"] + flags + [str(tmp_path / "reads.fa"), "-o", str(tmp_path / "c.tsv")])
    _run(["-d", str(tmp_path / "db"), "-q", "-K", "--gpu-batch", "1000000", str(tmp_path / "win.fa"), "-o", str(tmp_path / "d.tsv")])
    assert open(tmp_path / "c.tsv").read() == open(tmp_path / "d.tsv").read()
