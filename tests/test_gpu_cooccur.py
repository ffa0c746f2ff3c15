"""Shared reads of reference pairs end to end: K7 behind K3 inside the library's pipelines (kmcpg_set_cooccur) and `kmcp-search
--ref-stats R --ref-stats-cooccur C`, on the family database, reads and taxonomies of tests/test_gpu_refstats.py (its helpers are
imported, the file is not touched).  Three things must agree: C, what `kmcp-refstats -f 1 -t 0 ... --cooccur` makes of the same run's
TSV, and the plain restatement of profile.go:1117-1279 (tests/cooccur_reference.py) on that TSV.  For the library the brute force runs on
the result's own records: for every read the set of its matches' targets, one read for every unordered pair of them."""
import os
import re
from collections import Counter
from itertools import combinations

import numpy as np
import pytest

from tests import cooccur_reference as CR
from tests import filter_reference as FR
from tests import synth
from tests.test_gpu_cli import CLI
from tests.test_gpu_refstats import MIN_QCOV, TOOL, family, flags, run, tables  # noqa: F401 (family: the fixture)

pytestmark = pytest.mark.gpu

# (taxonomy, level, mode, H, p): one at level species, one at level strain (tests/test_gpu_refstats.py CONFIGS)
CONFIGS = [("B", "species", 5, None, None), (None, "strain", 3, 0.9, None)]


def restated(family, text, tag, level, mode, H, p):
    kw = {}
    if tag:
        dump, tmap = family["tax"][tag]
        kw = dict(taxid_map=FR.read_taxid_maps([tmap]), tax=FR.Taxonomy(dump))
    return CR.cooccur([text], max_fpr=1, min_qcov=0, level=level, mode=mode, min_hic_ureads_qcov=H, min_chunks_fraction=p, **kw)


def search(family, tmp_path, name, extra=(), env=None):
    """one kmcp-search run -> (the TSV, the statistics or None, the pairs or None, stderr)"""
    out, files = str(tmp_path / f"{name}.tsv"), {}
    cmd = [CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", out] + list(extra)
    for flag in ("--ref-stats", "--ref-stats-cooccur"):
        if flag in cmd:
            files[flag] = cmd[cmd.index(flag) + 1]
    r = run(cmd, env=env)
    return open(out).read(), *(open(files[f]).read() if f in files else None for f in ("--ref-stats", "--ref-stats-cooccur")), r.stderr


@pytest.mark.parametrize("config", CONFIGS, ids=["species", "strain"])
def test_cli_equals_kmcp_refstats_and_the_restatement(family, tmp_path, config):
    s, t = flags(family, *config)
    R, C = str(tmp_path / "R.tsv"), str(tmp_path / "C.tsv")
    plain, _, _, _ = search(family, tmp_path, "plain", ["-q"])
    _, stats, _, _ = search(family, tmp_path, "stats", ["-q", "--ref-stats", R] + s)
    want = restated(family, plain, *config)
    pairs = CR.pairs_of(want)
    print(f"{config}: {len(pairs)} pairs, the largest count {max(pairs.values())}")
    assert len(pairs) >= 2 and max(pairs.values()) > 1, "the expected file must not be (nearly) empty"
    open(tmp_path / "plain.tsv", "w").write(plain)
    tool_stats = run([TOOL] + t + ["--cooccur", tmp_path / "tool.tsv", tmp_path / "plain.tsv"]).stdout
    assert open(tmp_path / "tool.tsv").read() == want and tool_stats == stats

    def check(name, extra=(), env=None, tsv=plain):
        got_tsv, got_stats, got_pairs, err = search(family, tmp_path, name, ["--ref-stats", R, "--ref-stats-cooccur", C] + s + list(extra), env=env)
        assert got_tsv == tsv, f"{name}: the search result is what it is without the new flag"
        assert got_stats == stats, f"{name}: the statistics are what they are without the new flag"
        assert got_pairs == want, name
        return err

    err = check("one batch")
    m = re.search(r"(\d+) reads with several targets, (\d+) of them counted on the host, (\d+) for want of room", err)
    assert m and int(m.group(1)) > 100 and int(m.group(3)) == 0, err
    check("batches and threads", ["-q", "-j", "4", "--gpu-batch", "300"])
    if config[0]:  # --specific-level beside it: the TSV is the filtered one, statistics and pairs are those of the unfiltered run
        dump, tmap = family["tax"][config[0]]
        filtered, _, _, _ = search(family, tmp_path, "filtered", ["-q", "--specific-level", "species", "--taxid-map", tmap, "--taxdump", dump])
        assert 50 < filtered.count("\n") < plain.count("\n") - 50
        check("with K4", ["-q", "--gpu-batch", "300", "--specific-level", "species"], tsv=filtered)
    # every read to the host half, no K3 at all, and a table with room for 8 pairs: the same file
    for knob in ("KMCPG_COOCCUR_DEVICE", "KMCPG_DEVICE_FINALIZE"):
        err = check(knob, env=dict(os.environ, **{knob: "0"}))
        m = re.search(r"(\d+) reads with several targets, (\d+) of them counted on the host", err)
        assert m and m.group(1) == m.group(2), err
    err = check("8 slots", ["--ref-stats-cooccur-slots", "8"])
    assert int(re.search(r"(\d+) for want of room", err).group(1)) > 0, err
    # .gz is honoured
    import gzip
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", tmp_path / "gz.tsv", "-q", "--ref-stats", R, "--ref-stats-cooccur", C + ".gz"] + s)
    assert gzip.open(C + ".gz", "rt").read() == want


# ---- the library ----
def brute(target, res):
    """(pair -> reads, reads with several targets, pair adds) over a result of records"""
    c, multi = Counter(), 0
    for r in range(len(res.offs) - 1):
        ts = sorted({int(target[int(m["col"])]) for m in res.read(r)})
        multi += len(ts) > 1
        c.update(combinations(ts, 2))
    return dict(c), multi, sum(c.values())


def table(db):
    got, tot = db.cooccur_read()
    keys = list(zip(got["class_a"].tolist(), got["class_b"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and all(a < b for a, b in keys)
    return dict(zip(keys, got["reads"].tolist())), tot


def test_library_counts_what_the_brute_force_counts_and_changes_no_result(family, monkeypatch):
    from kmcp_amd import Database, default_params, lib
    reads = family["reads"] + [family["long_query"]]  # ... and one query above the device's -f bound: the host half counts it
    p = default_params(min_qcov=MIN_QCOV)
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        plain, plain_p = db.search(reads, params=p), db.search_pairs(reads, params=p)
        want, multi, adds = brute(target, plain)
        assert multi > 100 and len(want) >= 2 and max(want.values()) > 1
        long_multi = len({int(target[int(m["col"])]) for m in plain.read(len(reads) - 1)}) > 1
        db.set_cooccur(target)
        for form in ("records", "pairs", "tickets", "with K4", "host only", "8 slots", "with K6"):
            db.cooccur_reset()
            if form == "records":
                res = db.search(reads, params=p)
                assert all(np.array_equal(getattr(res, f), getattr(plain, f)) for f in ("qlen", "qkmers", "offs", "matches")), "the result changed"
            elif form == "pairs":
                res = db.search_pairs(reads, params=p)
                assert all(np.array_equal(getattr(res, f), getattr(plain_p, f)) for f in ("qlen", "qkmers", "offs", "pairs")), "the result changed"
            elif form == "tickets":  # three batches in flight
                cuts = [0, 300, 600, len(reads)]
                tickets = [db.submit(*lib.pack_reads(reads[a:b]), params=p) for a, b in zip(cuts, cuts[1:])]
                parts = [db.wait(t) for t in tickets]
                assert sum(len(x.matches) for x in parts) == len(plain.matches)
            elif form == "with K4":
                db.set_specific(target, species)
                res = db.search(reads, params=p)
                db.set_specific()
                assert 0 < len(res.matches) < len(plain.matches)
            elif form == "host only":
                monkeypatch.setenv("KMCPG_COOCCUR_DEVICE", "0")
                res = db.search(reads, params=p)
                monkeypatch.delenv("KMCPG_COOCCUR_DEVICE")
                assert np.array_equal(res.matches, plain.matches)
            elif form == "8 slots":  # the table does not grow: the reads that find no room are LEFT whole, and the host half counts them
                db.set_cooccur(target, table_slots=8)
                res = db.search(reads, params=p)
                assert np.array_equal(res.matches, plain.matches)
            else:  # K6 and K7 together: each counts what it counts alone
                db.set_refstats(target, species, hic_min_qcov=0.8)
                res = db.search(reads, params=p)
                both_on, _ = db.refstats_read(n)
                db.set_cooccur()
                db.refstats_reset()
                res2 = db.search(reads, params=p)
                k6_alone, _ = db.refstats_read(n)
                db.set_refstats()
                assert both_on.tobytes() == k6_alone.tobytes() and both_on.view(np.uint64).any()
                assert np.array_equal(res.matches, plain.matches) and np.array_equal(res2.matches, plain.matches)
                db.set_cooccur(target)  # (the comparison below then sees an empty table)
                db.search(reads, params=p)
            got, tot = table(db)
            assert got == want, f"{form}: {len(got)} pairs, expected {len(want)}"
            assert tot["multi_reads"] == multi and tot["device_adds"] + tot["host_adds"] == adds and tot["rebuilds"] == 0, (form, tot)
            assert tot["host_reads"] >= int(long_multi), (form, tot)
            if form == "host only":
                assert tot["device_adds"] == 0 and tot["host_reads"] == multi and tot["keys"] == 0, tot
            elif form == "8 slots":
                assert tot["left_full"] > 0 and tot["table_slots"] == 8 and tot["keys"] <= 8 and tot["host_adds"] > 0, tot
                db.set_cooccur(target)
            else:
                assert tot["left_full"] == 0 and tot["device_adds"] > 0 and tot["table_slots"] == 1 << 21, (form, tot)
        st, _ = db.last_cooccur()
        assert st["bad_segments"] == 0 and st["skipped"] == 0
        # reset zeroes; switching the stage off and on leaves no counts behind
        db.cooccur_reset()
        got, tot = table(db)
        assert got == {} and not any(v for k, v in tot.items() if k != "table_slots")
        db.search(reads[:300], params=p)
        assert table(db)[0]
        db.set_cooccur()
        db.set_cooccur(target)
        assert table(db)[0] == {}
        # what the stage refuses while it is on
        from kmcp_amd.lib import KmcpGpuError
        for kw in (dict(try_se=1), dict(top_n_scores=1)):
            with pytest.raises(KmcpGpuError, match="kmcpg_set_cooccur"):
                db.search(reads[:10], params=default_params(**kw))
        seqs, offs = np.frombuffer(family["long_query"], dtype=np.uint8).copy(), np.array([0, 3000], dtype=np.uint64)
        with pytest.raises(KmcpGpuError, match="kmcpg_set_cooccur"):
            db.submit_windows(seqs, offs, 100, 300)
        db.set_cooccur()
        again = db.search(reads, params=p)
        assert np.array_equal(again.matches, plain.matches)


def test_a_batch_that_is_run_again_is_counted_once(oracle_lib, tmp_path):
    """40 close relatives (the database of the same test of tests/test_gpu_refstats.py): every read matches ~35 columns, more than the 8
    per read a fresh lane has room for — the first attempt overflows its hit buffer and collect() runs the batch again.  The witness is
    the handle's count of K7 launches that left the counting to the rerun."""
    from kmcp_amd import Database, default_params
    rng = np.random.default_rng(91)
    base = synth.random_genomes(1, 6000, seed=90)[0]
    genomes = []
    for i in range(40):
        g = np.frombuffer(base, dtype=np.uint8).copy()
        m = rng.random(len(g)) < 0.004
        g[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(m.sum()))
        genomes.append(g.tobytes())
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=2, overlap=150, threads=1)
    reads = synth.sample_reads([base], 1500, 150, sub_rate=0.0, seed=200, frac_random=0.1)
    with Database.open(db_dir, device=0) as db:
        n = int(db.info.n_cols)
        names = [db.col_info(c)[0] for c in range(n)]
        ids = {}
        target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
        db.set_cooccur(target)
        res = db.search(reads, params=default_params())
        assert len(res.matches) > 8 * len(reads) + 1024, "more matches than the first attempt's hit buffer holds"
        want, multi, adds = brute(target, res)
        got, tot = table(db)
        assert got == want and multi > 1000 and max(want.values()) > 1000
        assert tot["multi_reads"] == multi and tot["device_adds"] + tot["host_adds"] == adds and tot["skipped_launches"] == 1, tot
        # a hot table: 780 pairs share 1 500 reads — the workgroups' LDS tables take the adds (the witness is of the rerun, the last launch)
        st, _ = db.last_cooccur()
        assert st["skipped"] == 0 and st["lds_adds"] + st["spilled_adds"] == st["pairs"] > 0 and st["global_adds"] < st["pairs"] // 4, st
