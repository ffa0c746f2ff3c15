"""Species-specific queries end to end: K4 behind K3 inside the library's pipelines (kmcpg_set_specific) and
`kmcp-search --specific-level`, on the reduced real-genome family database (tools/family_db.py: 16 base genomes, 6 + 15 x 3 strains,
10 chunks each) under two taxonomies the test writes:
  A  one species per base genome, its strains as children;
  B  the strains of each base genome alternately in two species of one genus.
The yardstick is `kmcp-filter` over the plain run's TSV (tests/test_filter_cpu.py holds it against the restatement of filter.go) and,
for the library, the restatement's literal rule (tests/filter_reference.py) on the plain result.

The searches run with -t 0.75 (MIN_QCOV): at the default 0.55 a read of this database matches nearly every strain of its base genome,
and only 1.5 % of the matched reads name one target.  From the oracle's TSV (2649 matched reads at 0.55), under taxonomy B:
    -t     one target   several targets of one species   several species
    0.55   0.015        0.061                            0.924
    0.65   0.054        0.077                            0.869
    0.75   0.140        0.078                            0.782     (2479 matched reads)
test_the_sample_is_not_one_sided asserts the 5 % per class for the value used; one command run keeps the default."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import filter_reference as FR
from tests.test_gpu_cli import CLI, HEADER, oracle_tsv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FILTER = os.path.join(ROOT, "kmcp_amd", "kmcp-filter")
MIN_QCOV = 0.75


def strain_of(name, accs):
    acc, s = name.rsplit(".s", 1)
    return accs.index(acc), int(s)


def write_taxonomy(d, names, accs, split):
    """nodes.dmp + a TaxId map for the targets `names`; split: the strains of a base genome in one species (A) or alternately in two (B)"""
    os.makedirs(d, exist_ok=True)
    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom"), (10, 2, "family")]
    ids = {}
    for gi in range(len(accs)):
        nodes.append((1000 + gi, 10, "genus"))
        for half in range(2 if split else 1):
            nodes.append((2000 + 2 * gi + half, 1000 + gi, "species"))
    for n in sorted(set(names)):
        gi, si = strain_of(n, accs)
        ids[n] = 100000 + 100 * gi + si
        nodes.append((ids[n], 2000 + 2 * gi + (si % 2 if split else 0), "strain"))
    with open(os.path.join(d, "nodes.dmp"), "w") as fh:
        for t, p, r in nodes:
            fh.write(f"{t}\t|\t{p}\t|\t{r}\t|\t\t|\n")
    with open(os.path.join(d, "map.tsv"), "w") as fh:
        for n, t in ids.items():
            fh.write(f"{n}\t{t}\n")
    return str(d), os.path.join(d, "map.tsv")


@pytest.fixture(scope="module")
def family(oracle_lib, tmp_path_factory):
    import family_db
    from kmcp_amd import lib
    O = oracle_lib
    tmp = tmp_path_factory.mktemp("specific")
    cols, reads, info = family_db.generate(ecoli_strains=6, small_strains=3, n_reads=3000)
    whole = lib.build_db(str(tmp / "db"), cols, k=family_db.K, threads=8, alias="family-db")
    accs = [a for a, _ in family_db.base_genomes()]
    names = [c[0] for c in cols]
    # the database split in two by base genome (a target's chunks stay together), for --also-db
    first = [c for c in cols if strain_of(c[0], accs)[0] % 2 == 0]
    second = [c for c in cols if strain_of(c[0], accs)[0] % 2 == 1]
    halves = [lib.build_db(str(tmp / "h0"), first, k=family_db.K, threads=8, alias="family-h0"), lib.build_db(str(tmp / "h1"), second, k=family_db.K, threads=8, alias="family-h1")]
    rl = [reads[i].tobytes() for i in range(reads.shape[0])]
    fq = str(tmp / "r.fq")
    family_db.write_fastq(fq, reads)
    tax = {"A": write_taxonomy(str(tmp / "taxA"), names, accs, False), "B": write_taxonomy(str(tmp / "taxB"), names, accs, True)}
    odb = O.OracleDB(whole)
    try:
        rows, _ = oracle_tsv(O, odb, [f"r{i}" for i in range(len(rl))], rl, params=O.default_params(min_qcov=MIN_QCOV))
    finally:
        odb.close()
    long_query = family_db.base_genomes()[1][1][:3000]
    return dict(tmp=tmp, db_dir=whole, root=os.path.dirname(whole), halves=[os.path.dirname(h) for h in halves], reads=rl, fq=fq, tax=tax, oracle_rows=rows,
                long_query=long_query)


def run(cmd, env=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    return r


def trailer(text, total):
    queries = {l.split("\t", 1)[0] + "\t" + l.rsplit("\t", 1)[1] for l in text.splitlines() if l and l[0] != "#"}
    return f"# input queries: {total}\n# matched queries: {len(queries)}\n" + "# matched percentage: %.4f%%\n" % (len(queries) / total * 100)


def test_the_sample_is_not_one_sided(family):
    """from the ORACLE's TSV, by the restatement under taxonomy B: reads with one target, with several targets of one species, with several
    species — at least 5 % of the matched reads each"""
    dump, tmap = family["tax"]["B"]
    verdicts = []
    FR.filter_files([[r + "\n" for r in family["oracle_rows"]]], max_fpr=1, min_qcov=0, taxid_map=FR.read_taxid_maps([tmap]), tax=FR.Taxonomy(dump), verdicts=verdicts)
    n = len(verdicts)
    one = sum(1 for _, t, k in verdicts if t == 1)
    same = sum(1 for _, t, k in verdicts if t > 1 and k)
    several = sum(1 for _, t, k in verdicts if not k)
    print(f"matched reads {n}: one target {one} ({one / n:.3f}), several targets of one species {same} ({same / n:.3f}), several species {several} ({several / n:.3f})")
    assert n > 2000 and min(one, same, several) >= 0.05 * n, (n, one, same, several)


def cli_contract(family, tmp, db_args, levels):
    plain = str(tmp / "plain.tsv")
    run([CLI] + db_args + [family["fq"], "-o", plain, "-q"])
    n_plain = open(plain).read().count("\n")
    n_reads = len(family["reads"])
    seen = set()
    for tag, level in levels:
        tx = []
        if tag:
            dump, tmap = family["tax"][tag]
            tx = ["--taxid-map", tmap, "--taxdump", dump]
        ftx = ["-T", tx[1], "-X", tx[3]] if tx else []
        want = run([FILTER, "-f", "1", "-t", "0", "--level", level] + ftx + [plain]).stdout
        out = str(tmp / f"specific_{tag}_{level}.tsv")
        run([CLI] + db_args + [family["fq"], "-o", out, "-q", "--specific-level", level] + tx)
        got = open(out).read()
        assert got == want + trailer(want, n_reads), (tag, level)
        assert want.startswith(HEADER + "\n") and 20 < want.count("\n") < n_plain - 100
        seen.add(want)
    return seen


def test_cli_equals_kmcp_filter_over_the_plain_run(family, tmp_path):
    seen = cli_contract(family, tmp_path, ["-d", family["root"], "-t", MIN_QCOV], [("A", "species"), ("B", "species"), (None, "strain"), ("A", "assembly")])
    assert len(seen) == 3  # A, B and strain level keep different reads; assembly is strain


def test_cli_with_also_db(family, tmp_path):
    cli_contract(family, tmp_path, ["-d", family["halves"][0], "--also-db", family["halves"][1]], [("B", "species"), (None, "strain")])


def test_cli_gz_paired_and_sort_modes(family, tmp_path):
    """-s tcov / -S change the order of a query's rows, not the verdict; paired input (the reads as their own mates) and -o .gz"""
    import gzip
    dump, tmap = family["tax"]["B"]
    tx = ["--taxid-map", tmap, "--taxdump", dump]
    for extra in (["-s", "tcov", "-t", MIN_QCOV], ["-S", "-t", MIN_QCOV], ["-1", family["fq"], "-2", family["fq"]]):
        files = [] if "-1" in extra else [family["fq"]]
        plain, out = str(tmp_path / "p.tsv"), str(tmp_path / "s.tsv.gz")
        run([CLI, "-d", family["root"], "-o", plain, "-q"] + extra + files)
        run([CLI, "-d", family["root"], "-o", out, "-q", "--specific-level", "species"] + tx + extra + files)
        want = run([FILTER, "-f", "1", "-t", "0", "-T", tmap, "-X", dump, plain]).stdout
        assert gzip.open(out, "rt").read() == want + trailer(want, len(family["reads"])), extra


def test_cli_needs_a_taxid_for_every_target(family, tmp_path):
    dump, tmap = family["tax"]["A"]
    short = tmp_path / "short_map.tsv"
    lines = open(tmap).read().splitlines()
    short.write_text("\n".join(lines[:-1]) + "\n")
    out = tmp_path / "o.tsv"
    r = subprocess.run([CLI, "-d", family["root"], family["fq"], "-o", str(out), "-q", "--specific-level", "species", "--taxid-map", str(short), "--taxdump", dump],
                       capture_output=True, text=True, timeout=300)
    missing = lines[-1].split("\t")[0]
    assert r.returncode == 255 and f"unknown taxid for {missing}, please check taxid mapping file(s)" in r.stderr and not out.exists()


# ---- the library ----
def tables(db, family, tag):
    n = int(db.info.n_cols)
    names = [db.col_info(c)[0] for c in range(n)]
    ids = {}
    target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
    if tag is None:
        return names, target, None, None, None
    dump, tmap = family["tax"][tag]
    taxo, tmap_ids = FR.Taxonomy(dump), FR.read_taxid_maps([tmap])

    def species_of(t):
        return next((x for x in taxo.lineage(t) if taxo.rank[x] == "species"), 0)
    return names, target, np.array([species_of(tmap_ids[x]) for x in names], dtype=np.uint32), taxo, tmap_ids


def judged(plain_offs, cols_of, names, level_species, tmap_ids, taxo):
    """the restatement's literal rule on every read of a plain result -> keep[r] (True for reads without matches)"""
    keep = np.ones(len(plain_offs) - 1, dtype=bool)
    for r in range(len(keep)):
        cols = cols_of(r)
        if len(cols):
            targets = list(dict.fromkeys(names[c] for c in cols))
            keep[r] = FR.judge(targets, level_species, tmap_ids, taxo)
    return keep


def emptied(res, keep, field):
    lens = np.diff(res.offs.astype(np.int64))
    offs = np.concatenate([[0], np.cumsum(np.where(keep, lens, 0))]).astype(np.uint64)
    return offs, getattr(res, field)[np.repeat(keep, lens)]


@pytest.mark.parametrize("tag", ["A", "B", None])
def test_library_equals_the_plain_result_with_the_dropped_reads_emptied(family, tag, monkeypatch):
    from kmcp_amd import Database, default_params
    reads = family["reads"]
    with Database.open(family["db_dir"], device=0) as db:
        db.set_profiling(1)
        names, target, species, taxo, tmap_ids = tables(db, family, tag)
        plain, plain_p = db.search(reads, params=default_params(min_qcov=MIN_QCOV)), db.search_pairs(reads, params=default_params(min_qcov=MIN_QCOV))
        st, launches = db.last_specific()
        assert launches == [] and not any(st.values())  # the stage is off: nothing launched
        keep = judged(plain.offs, lambda r: plain.read(r)["col"], names, tag is not None, tmap_ids, taxo)
        assert keep.sum() > 300 and (~keep).sum() > 50  # (under A few reads are dropped: a read rarely matches two base genomes)
        want_offs, want_m = emptied(plain, keep, "matches")
        _, want_p = emptied(plain_p, keep, "pairs")
        db.set_specific(target, species)
        for env in (None, "0"):
            if env is not None:
                monkeypatch.setenv("KMCPG_SPECIFIC_DEVICE", env)
            got = db.search(reads, params=default_params(min_qcov=MIN_QCOV))
            st, launches = db.last_specific()
            assert np.array_equal(got.offs, want_offs) and got.matches.tobytes() == want_m.tobytes(), (tag, env)
            assert np.array_equal(got.qkmers, plain.qkmers) and np.array_equal(got.qlen, plain.qlen)
            assert len(launches) == 5 and st["bad_segments"] == 0
            matched = int((np.diff(plain.offs.astype(np.int64)) > 0).sum())
            if env is None:  # 150-base reads: every verdict on the device
                assert st["host"] == 0 and st["kept"] + st["dropped"] == matched and st["dropped"] == int((~keep).sum())
                assert st["pairs_in"] == int(plain.offs[-1]) and st["pairs_out"] == int(want_offs[-1])
            else:            # every read left to the host: the same result, no device verdict
                assert st["kept"] == 0 and st["dropped"] == 0 and st["host"] == matched and st["pairs_out"] == st["pairs_in"]
            got_p = db.search_pairs(reads, params=default_params(min_qcov=MIN_QCOV))
            assert np.array_equal(got_p.offs, want_offs) and np.array_equal(got_p.pairs, want_p), (tag, env)
            # submit / wait, records and pairs
            from kmcp_amd.lib import pack_reads
            seqs, offs = pack_reads(reads)
            got_w = db.wait(db.submit(seqs, offs, params=default_params(min_qcov=MIN_QCOV)))
            assert np.array_equal(got_w.offs, want_offs) and got_w.matches.tobytes() == want_m.tobytes()
            got_wp = db.wait_pairs(db.submit(seqs, offs, params=default_params(min_qcov=MIN_QCOV)))
            assert np.array_equal(got_wp.offs, want_offs) and np.array_equal(got_wp.pairs, want_p)
        monkeypatch.delenv("KMCPG_SPECIFIC_DEVICE")
        # K3 off (the hits go through kmcpg_finalize): the rule on the finished records
        monkeypatch.setenv("KMCPG_DEVICE_FINALIZE", "0")
        with Database.open(family["db_dir"], device=0) as db2:
            db2.set_specific(target, species)
            got = db2.search(reads, params=default_params(min_qcov=MIN_QCOV))
            assert np.array_equal(got.offs, want_offs) and got.matches.tobytes() == want_m.tobytes()
        monkeypatch.delenv("KMCPG_DEVICE_FINALIZE")
        # off again: the plain result, nothing launched
        db.set_specific()
        again = db.search(reads, params=default_params(min_qcov=MIN_QCOV))
        assert np.array_equal(again.offs, plain.offs) and again.matches.tobytes() == plain.matches.tobytes()
        assert db.last_specific()[1] == []


def test_pieces_of_a_large_batch(family, monkeypatch):
    """kmcpg_search_batch cuts large batches into pieces that land in one result (host.cpp search_batch_pieces): the verdicts go with them"""
    from kmcp_amd import Database, default_params
    reads = family["reads"]
    monkeypatch.setenv("KMCPG_PIECE_MIN", "500")
    with Database.open(family["db_dir"], device=0) as db:
        names, target, species, taxo, tmap_ids = tables(db, family, "B")
        db.search(reads, params=default_params(min_qcov=MIN_QCOV))  # (the first large batch of a handle goes through whole)
        plain = db.search_pairs(reads, params=default_params(min_qcov=MIN_QCOV))
        keep = judged(plain.offs, lambda r: plain.read(r)[:, 0], names, True, tmap_ids, taxo)
        want_offs, want_p = emptied(plain, keep, "pairs")
        db.set_specific(target, species)
        for env in (None, "0"):
            if env is not None:
                monkeypatch.setenv("KMCPG_SPECIFIC_DEVICE", env)
            got = db.search_pairs(reads, params=default_params(min_qcov=MIN_QCOV))
            assert np.array_equal(got.offs, want_offs) and np.array_equal(got.pairs, want_p), env
            st = db.last_specific()[0]
            assert st["pairs_in"] < int(plain.offs[-1])  # the last launch saw a piece, not the batch


def test_a_long_query_is_judged_on_the_host(family, tmp_path):
    """more than 1024 k-mers: the -f test is the host's, so K4 leaves the read to it (HOST) and the host applies the rule afterwards"""
    from kmcp_amd import Database, default_params
    q = family["long_query"]
    with Database.open(family["db_dir"], device=0) as db:
        plain = db.search([q], params=default_params(min_qcov=MIN_QCOV))
        assert plain.qkmers[0] > 1024 and len(plain.matches) >= 2
        for tag in ("A", "B", None):
            names, target, species, taxo, tmap_ids = tables(db, family, tag)
            keep = judged(plain.offs, lambda r: plain.read(r)["col"], names, tag is not None, tmap_ids, taxo)
            db.set_specific(target, species)
            got = db.search([q], params=default_params(min_qcov=MIN_QCOV))
            st = db.last_specific()[0]
            assert (st["kept"], st["dropped"], st["host"]) == (0, 0, 1), st
            assert len(got.matches) == (len(plain.matches) if keep[0] else 0), tag
            if keep[0]:
                assert got.matches.tobytes() == plain.matches.tobytes()
        # the same through the command: -g, against kmcp-filter
        fa = tmp_path / "long.fa"
        fa.write_text(">long\n" + q.decode() + "\n")
        plain_tsv, out = str(tmp_path / "p.tsv"), str(tmp_path / "s.tsv")
        run([CLI, "-d", family["root"], "-g", str(fa), "-o", plain_tsv, "-q"])
        for tag in ("A", "B"):
            dump, tmap = family["tax"][tag]
            run([CLI, "-d", family["root"], "-g", str(fa), "-o", out, "-q", "--specific-level", "species", "--taxid-map", tmap, "--taxdump", dump])
            want = run([FILTER, "-f", "1", "-t", "0", "-T", tmap, "-X", dump, plain_tsv]).stdout
            assert open(out).read() == want + trailer(want, 1), tag


def test_library_refusals(family):
    from kmcp_amd import Database, default_params
    from kmcp_amd.lib import KmcpGpuError, pack_reads
    reads = family["reads"][:64]
    seqs, offs = pack_reads(reads)
    with Database.open(family["db_dir"], device=0) as db:
        target = tables(db, family, None)[1]
        db.set_specific(target)
        for kw, word in ((dict(try_se=1), "try_se"), (dict(top_n_scores=2), "top_n_scores")):
            for call in (lambda p: db.search(reads, params=p), lambda p: db.submit(seqs, offs, params=p)):
                with pytest.raises(KmcpGpuError, match=word) as e:
                    call(default_params(**kw))
                assert e.value.code == -6
        with pytest.raises(KmcpGpuError, match="kmcpg_submit_windows"):
            db.submit_windows(seqs, offs, 100, 150)
        db.set_specific()
        assert len(db.search(reads, params=default_params(top_n_scores=2))) == 64
    with Database.open_paged(family["db_dir"], device=0, passes=2) as paged:
        with pytest.raises(KmcpGpuError, match="paged handle"):
            paged.set_specific(target)
    with Database.open(family["db_dir"], device=0, shard_rank=0, shard_count=2) as shard:
        with pytest.raises(KmcpGpuError, match="shard_count"):
            shard.set_specific(target)
    with Database.open_devices(family["db_dir"], [0, 0]) as multi:
        with pytest.raises(KmcpGpuError, match="multi-device"):
            multi.set_specific(target)
