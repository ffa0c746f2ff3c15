"""Specific regions end to end: `kmcp-search --regions-bed` (K5 behind K4 behind K3) and the library's kmcpg_submit_windows_summary, on a
synthetic mosaic (tests/synth.py: k = 21, random genomes of 30 kb, 3 chunks each):
  Q   the query genome itself                                   species A
  S1  Q on [0, 12 k) with about 3 % substitutions, else random  species A: its qCov straddles 0.55, so the type flips between windows
  X   Q on [8 k, 20 k) exactly, else random                     species B: windows there name two species and are dropped
  U1, U2  unrelated                                             species C, D
Windows are -s 50 -W 150; regions with --regions-min-overlap 20.

The contract: the BED is byte for byte what kmcp-regions -f 1 -t 0 makes of what kmcp-filter -f 1 -t 0 makes of the TSV of the same
kmcp-search command without --specific-level / --regions-* (tests/test_regions_cpu.py and tests/test_filter_cpu.py hold those two
against the restatements of the reference)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import regions_reference as RR
from tests import synth
from tests.test_gpu_cli import CLI, oracle_tsv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER = os.path.join(ROOT, "kmcp_amd", "kmcp-filter")
REGIONS = os.path.join(ROOT, "kmcp_amd", "kmcp-regions")
STEP, WINDOW, OVERLAP = 50, 150, 20
SLIDING = ["--sliding-step", str(STEP), "--sliding-window", str(WINDOW)]
NAMES = ["Q", "S1", "X", "U1", "U2"]
SPECIES = {"Q": 2000, "S1": 2000, "X": 2001, "U1": 2002, "U2": 2003}


def run(cmd, env=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=120, env=None if env is None else dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def windows_of(seq):
    return [(a, a + WINDOW) for a in range(0, len(seq) - WINDOW + 1, STEP)]


@pytest.fixture(scope="module")
def mosaic(oracle_lib, tmp_path_factory):
    O = oracle_lib
    tmp = tmp_path_factory.mktemp("regions")
    rng = np.random.default_rng(2024)
    q, s1, x, u1, u2 = [np.frombuffer(g, dtype=np.uint8).copy() for g in synth.random_genomes(5, 30000, seed=31)]
    s1[:12000] = q[:12000]
    flip = np.flatnonzero(rng.random(12000) < 0.03)
    s1[flip] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), s1[flip]) + rng.integers(1, 4, size=len(flip))) % 4]
    x[8000:20000] = q[8000:20000]
    genomes = [g.tobytes() for g in (q, s1, x, u1, u2)]
    db_dir = synth.make_db(tmp / "db", genomes, k=21, n_chunks=3, overlap=150, threads=2, names=NAMES)
    # the taxonomy: four species of one genus, the targets as strains
    dump = tmp / "tax"
    os.makedirs(dump)
    nodes = [(1, 1, "no rank"), (10, 1, "family"), (1000, 10, "genus")] + [(s, 1000, "species") for s in sorted(set(SPECIES.values()))]
    nodes += [(100000 + i, SPECIES[n], "strain") for i, n in enumerate(NAMES)]
    (dump / "nodes.dmp").write_text("".join(f"{t}\t|\t{p}\t|\t{r}\t|\t\t|\n" for t, p, r in nodes))
    tmap = tmp / "map.tsv"
    tmap.write_text("".join(f"{n}\t{100000 + i}\n" for i, n in enumerate(NAMES)))
    fa = tmp / "q.fa"
    fa.write_text(">chrQ\n" + genomes[0].decode() + "\n")
    twice = tmp / "twice.fa"  # a second record with the same ID right behind the first
    twice.write_text(">chrQ\n" + genomes[0][:9000].decode() + "\n>chrQ\n" + genomes[0][4000:16000].decode() + "\n")
    # the oracle's TSV of the windows as text
    odb = O.OracleDB(db_dir)
    try:
        wins = windows_of(genomes[0])
        rows, _ = oracle_tsv(O, odb, [f"chrQ_sliding:{a + 1}-{e}" for a, e in wins], [genomes[0][a:e] for a, e in wins])
    finally:
        odb.close()
    (tmp / "oracle.tsv").write_text("".join(r + "\n" for r in rows))
    return dict(tmp=tmp, db_dir=db_dir, root=os.path.dirname(db_dir), q=genomes[0], fa=fa, twice=twice, dump=dump, tmap=tmap, oracle=tmp / "oracle.tsv")


def tax_flags(m, level, short=False):
    if level != "species":
        return []
    return ["-T", m["tmap"], "-X", m["dump"]] if short else ["--taxid-map", m["tmap"], "--taxdump", m["dump"]]


def test_the_mosaic_has_every_kind_of_region(mosaic):
    """a CPU-side precondition, from the oracle's TSV through kmcp-filter and the restatement"""
    m = mosaic
    kept = run([FILTER, "-f", 1, "-t", 0, "--level", "species"] + tax_flags(m, "species", True) + [m["oracle"]]).stdout.splitlines(True)
    bed = RR.merge_file(kept, max_fpr=1, min_qcov=0, min_overlap=OVERLAP, garbage_line=False)
    regions = [l.split("\t") for l in bed.splitlines()]
    by_name = {n: sum(1 for r in regions if r[3] == n) for n in ("species-specific", "assembly-specific")}
    print(by_name, len(regions))
    assert min(by_name.values()) >= 5, by_name
    assert any(int(r[2]) - int(r[1]) >= WINDOW + 2 * STEP for r in regions)  # merged from three windows or more
    begins = sorted({int(l.split("\t", 1)[0].rsplit(":", 1)[1].split("-")[0]) for l in kept if l[0] != "#"})
    n_windows = len(windows_of(m["q"]))
    ended_by_drop = ended_by_type = 0
    for r in regions:
        nxt = int(r[2]) - WINDOW + 1 + STEP  # the begin of the window after the region's last one
        if nxt > (n_windows - 1) * STEP + 1:
            continue
        if nxt in begins:
            ended_by_type += 1
        else:
            ended_by_drop += 1
    assert ended_by_drop >= 1 and ended_by_type >= 1, (ended_by_drop, ended_by_type)
    fewer = RR.merge_file(kept, max_fpr=1, min_qcov=0, min_overlap=OVERLAP, garbage_line=False, ignore_type=True)
    assert 0 < fewer.count("\n") < len(regions)


@pytest.fixture(scope="module")
def plain_tsv(mosaic):
    """the TSV of the same kmcp-search command without --specific-level / --regions-*, for both inputs"""
    out = {}
    for key in ("fa", "twice"):
        p = mosaic["tmp"] / f"plain_{key}.tsv"
        run([CLI, "-d", mosaic["root"], mosaic[key], "-o", p, "-q"] + SLIDING)
        out[key] = p
    return out


def three_commands(m, plain, level, region_flags):
    kept = run([FILTER, "-f", 1, "-t", 0, "--level", level] + tax_flags(m, level, True) + [plain]).stdout
    r = subprocess.run([REGIONS, "-f", "1", "-t", "0"] + [str(f) for f in region_flags], input=kept, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def one_pass(m, inp, level, search_flags, env=None, name="out.bed"):
    bed = m["tmp"] / name
    if bed.exists():
        bed.unlink()
    r = run([CLI, "-d", m["root"], m[inp], "--specific-level", level, "--regions-bed", bed] + tax_flags(m, level) + SLIDING + search_flags, env=env)
    assert r.stdout == ""
    return (gzip.open(bed, "rt") if name.endswith(".gz") else open(bed)).read(), r.stderr


CONTRACT = [
    ("species", "fa", "species", ["--regions-min-overlap", OVERLAP], ["-l", OVERLAP], "out.bed"),
    ("strain", "fa", "strain", ["--regions-min-overlap", OVERLAP], ["-l", OVERLAP], "out.bed"),
    ("ignore type", "fa", "species", ["--regions-min-overlap", OVERLAP, "--regions-ignore-type"], ["-l", OVERLAP, "-I"], "out.bed"),
    ("max gap 60", "fa", "species", ["--regions-min-overlap", OVERLAP, "--regions-max-gap", 60], ["-l", OVERLAP, "-g", 60], "out.bed"),
    ("default overlap", "fa", "species", [], [], "out.bed"),
    ("custom names", "fa", "species", ["--regions-min-overlap", OVERLAP, "--regions-name-species", "sp", "--regions-name-assembly", "asm x"],
     ["-l", OVERLAP, "-s", "sp", "-a", "asm x"], "out.bed"),
    ("gz", "fa", "species", ["--regions-min-overlap", OVERLAP], ["-l", OVERLAP], "out.bed.gz"),
    ("the same ID twice", "twice", "species", ["--regions-min-overlap", OVERLAP], ["-l", OVERLAP], "out.bed"),
]


@pytest.mark.parametrize("case", CONTRACT, ids=[c[0] for c in CONTRACT])
def test_the_contract(mosaic, plain_tsv, case):
    _, inp, level, search_flags, region_flags, name = case
    want = three_commands(mosaic, plain_tsv[inp], level, region_flags)
    got, err = one_pass(mosaic, inp, level, search_flags + ["-q"], name=name)
    assert got == want
    assert want.count("\n") >= 2  # (with --regions-ignore-type the mosaic comes to two regions)


def test_the_stderr_line(mosaic, plain_tsv):
    want = three_commands(mosaic, plain_tsv["fa"], "species", ["-l", OVERLAP])
    got, err = one_pass(mosaic, "fa", "species", ["--regions-min-overlap", OVERLAP])
    assert got == want
    line = [l for l in err.splitlines() if "specific regions:" in l]
    assert len(line) == 1 and f"{len(windows_of(mosaic['q']))} windows" in line[0] and f"{want.count(chr(10))} regions" in line[0], err


ENVS = [
    ("pieces", "fa", dict(KMCPG_TEST_HOOKS="1", KMCPG_TEST_MAX_BASES=str(WINDOW * 150)), []),  # 597 windows in pieces of 150: the record spans four
    ("tiny batches", "twice", None, ["--gpu-batch", "1"]),  # a batch per record: the merger's state crosses batches
    ("window text", "fa", dict(KMCPG_WINDOWS_HOST="1"), []),
    ("window text in pieces", "fa", dict(KMCPG_WINDOWS_HOST="1", KMCPG_TEST_HOOKS="1", KMCPG_TEST_MAX_BASES=str(WINDOW * 150)), []),
    ("every window LEFT", "fa", dict(KMCPG_SPECIFIC_DEVICE="0"), []),
    ("no K3", "fa", dict(KMCPG_DEVICE_FINALIZE="0"), []),
]


@pytest.mark.parametrize("case", ENVS, ids=[c[0] for c in ENVS])
def test_pieces_and_switches(mosaic, plain_tsv, case):
    _, inp, env, flags = case
    want = three_commands(mosaic, plain_tsv[inp], "species", ["-l", OVERLAP])
    got, _ = one_pass(mosaic, inp, "species", ["--regions-min-overlap", OVERLAP, "-q"] + flags, env=env)
    assert got == want


def tables(db, level):
    names = [db.col_info(c)[0] for c in range(int(db.info.n_cols))]
    ids = {}
    target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
    return names, target, np.array([SPECIES[x] for x in names], dtype=np.uint32) if level == "species" else None


def want_summaries(plain, names, level):
    """the restatement's summary of every window of a plain windows result that the filter's rule keeps"""
    out = []
    for i in range(len(plain)):
        ms = plain.read(i)
        targets = [names[c] for c in ms["col"]]
        keep = len(set(targets)) == 1 or (level == "species" and len({SPECIES[t] for t in targets}) == 1)
        if not len(ms) or not keep:
            out.append((0, 0.0))
        else:
            out.append(RR.window_summary([(t, float("%.4f" % q)) for t, q in zip(targets, ms["qcov"])]))
    return out


def check_summaries(got, want, tag):
    s, qlen, qkmers = got
    assert len(s) == len(want), tag
    assert not s["flags"].any(), tag
    for i, (n, score) in enumerate(want):
        assert int(s["n_targets"][i]) == n and np.float64(s["score"][i]).view(np.uint64) == np.float64(score).view(np.uint64), (tag, i, s[i], n, score)


@pytest.mark.parametrize("level", ["species", "strain"])
def test_library(mosaic, level, monkeypatch):
    from kmcp_amd import Database
    from kmcp_amd.lib import KmcpGpuError, pack_reads
    seqs, offs = pack_reads([mosaic["q"]])
    n = len(windows_of(mosaic["q"]))
    with Database.open(mosaic["db_dir"], device=0) as db:
        db.set_profiling(1)
        names, target, species = tables(db, level)
        with pytest.raises(KmcpGpuError, match="stage is off"):
            db.submit_windows_summary(seqs, offs, STEP, WINDOW)
        plain = db.wait(db.submit_windows(seqs, offs, STEP, WINDOW))
        assert len(plain) == n
        want = want_summaries(plain, names, level)
        assert sum(1 for w in want if w[0] == 1) > 50 and (level != "species" or sum(1 for w in want if w[0] > 1) > 20)
        db.set_specific(target, species)
        t = db.submit_windows_summary(seqs, offs, STEP, WINDOW)
        for wrong in (db.wait, db.wait_pairs):
            with pytest.raises(KmcpGpuError, match="kmcpg_wait_summaries"):
                wrong(t)
        got = db.wait_summaries(t)
        check_summaries(got, want, "default")
        assert np.array_equal(got[1], plain.qlen) and np.array_equal(got[2], plain.qkmers)
        st, launches = db.last_summary()
        empty = sum(1 for w in want if w[0] == 0)
        assert (st["single"], st["wave"], st["left"], st["empty"]) == (sum(1 for w in want if w[0] == 1), sum(1 for w in want if w[0] > 1), 0, empty), st
        # 16 bytes per window, its qlen and qkmers, and four counter words: no pairs, no offsets, no verdicts
        assert st["left_pairs"] == 0 and st["bytes_d2h"] == 16 * n + 8 * n + 32, st
        assert [l.kernel for l in launches][0] == 16 and len(launches) == 5
        # a ticket of submit_windows is refused by wait_summaries, and still good for wait
        db.set_specific()
        t2 = db.submit_windows(seqs, offs, STEP, WINDOW)
        with pytest.raises(KmcpGpuError, match="not one of kmcpg_submit_windows_summary"):
            db.wait_summaries(t2)
        assert len(db.wait(t2)) == n
        db.set_specific(target, species)
        # every window LEFT (pieces and window text: test_pieces_and_switches — the library reads those switches once per process)
        monkeypatch.setenv("KMCPG_SPECIFIC_DEVICE", "0")
        check_summaries(db.wait_summaries(db.submit_windows_summary(seqs, offs, STEP, WINDOW)), want, "LEFT")
        st = db.last_summary()[0]
        assert (st["single"], st["wave"], st["left"]) == (0, 0, n - sum(1 for i in range(n) if len(plain.read(i)) == 0)), st
        assert st["left_pairs"] == len(plain.matches) and st["bytes_d2h"] == 24 * n + 32 + 8 * len(plain.matches)
        monkeypatch.delenv("KMCPG_SPECIFIC_DEVICE")
