"""Recount with ambiguity correction end to end: K8 inside the library's pipelines (kmcpg_set_recount: the log kernel behind K3, the replay
after the last batch) and `kmcp-search --ref-stats R --ref-stats-cooccur C --ref-stats-recount FILE`, on the family database, reads and
taxonomies of tests/test_gpu_refstats.py (its helpers are imported, the file is not touched).  Three things must agree: FILE, what
`kmcp-refstats -f 1 -t 0 ... --recount` makes of the same run's TSV — byte for byte — and the plain restatement of profile.go:1282-1888
(tests/recount_reference.py) on that TSV, within the derived tolerance of tests/test_recount_cpu.py (`compare`).

The configurations are the species one (taxonomy B) and the strain one of tests/test_gpu_refstats.py, and the species one at mode 1 for
the verdicts.  With the defaults D = R = 0.05 the 800 reads have nothing to correct (no reference has 20 times the unique reads of one it
shares reads with), so the searches run with --ref-stats-max-mismatch-err 0.9 (D stays 0.05).  From the oracle's TSV, by the restatement:
    taxonomy, level, mode    recounted   unique   corrected   unique without the correction   verdicts
    B  species  5            519         511      264         254                             few-unique 23
    -  strain   3, H = 0.9   421         416       62         359                             low-chunks-fraction 12, few-unique 3
    B  species  1            660         626      508         145                             low-chunks-fraction 32, few-unique 11, ok 1
(modes 5 and 3 ask 50 and 20 unique reads of a reference; 800 reads over 51 references cannot say more than that — mode 1 can.)
test_the_sample_has_something_to_correct asserts the table's shape on the oracle's TSV."""
import gzip
import os
import re

import numpy as np
import pytest

from tests import filter_reference as FR
from tests import recount_reference as R3
from tests import synth
from tests.test_gpu_cli import CLI
from tests.test_gpu_refstats import MIN_QCOV, TOOL, family, flags, run, tables  # noqa: F401 (family: the fixture)
from tests.test_recount_cpu import compare

pytestmark = pytest.mark.gpu

# (taxonomy, level, mode, H, p)
CONFIGS = [("B", "species", 5, None, None), (None, "strain", 3, 0.9, None), ("B", "species", 1, None, None)]
IDS = ["species", "strain", "species mode 1"]
D, R = 0.05, 0.9
S_FLAGS = ["--ref-stats-max-mismatch-err", R, "--ref-stats-min-dreads-prop", D]
T_FLAGS = ["-R", R, "-D", D]


def restated(family, text, tag, level, mode, H, p, **kw):
    if tag:
        dump, tmap = family["tax"][tag]
        kw.update(taxid_map=FR.read_taxid_maps([tmap]), tax=FR.Taxonomy(dump))
    return R3.recount([text], max_fpr=1, min_qcov=0, level=level, mode=mode, min_hic_ureads_qcov=H, min_chunks_fraction=p, min_dreads_prop=D, max_mismatch_err=R, **kw)


def test_the_sample_has_something_to_correct(family):
    """from the ORACLE's TSV, by the restatement: in every configuration at least 50 reads lose a target to the correction, at least 5 of
    them end unique, and the file differs from the one without the correction; at least three different stage-3 verdicts occur"""
    text = "\n".join(family["oracle_rows"]) + "\n"
    seen = set()
    for config in CONFIGS:
        with_corr, without = restated(family, text, *config), restated(family, text, *config, no_amb_corr=True)
        (n, uniq, corrected), refs = R3.parse(with_corr)
        (n0, uniq0, corrected0), _ = R3.parse(without)
        verdicts = [v["verdict"] for v in refs.values()]
        print(f"{config}: recounted {n}, unique {uniq}, corrected {corrected}, unique without the correction {uniq0}; " +
              ", ".join(f"{x} {verdicts.count(x)}" for x in sorted(set(verdicts))))
        assert n == n0 and corrected0 == 0 and corrected >= 50 and uniq - uniq0 >= 5 and with_corr != without, config
        seen |= set(verdicts)
    assert len(seen) >= 3 and len(set(verdicts)) >= 3, seen  # ... three of them in the last configuration alone


def search(family, tmp_path, name, extra=(), env=None):
    """one kmcp-search run -> (the TSV, {flag: its file's text}, stderr)"""
    out, files = str(tmp_path / f"{name}.tsv"), {}
    cmd = [CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", out] + list(extra)
    for flag in ("--ref-stats", "--ref-stats-cooccur", "--ref-stats-recount"):
        if flag in cmd:
            files[flag] = cmd[cmd.index(flag) + 1]
    r = run(cmd, env=env)
    return open(out).read(), {f: open(p).read() for f, p in files.items()}, r.stderr


@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_cli_equals_kmcp_refstats_and_the_restatement(family, tmp_path, config):
    s, t = flags(family, *config)
    Rf, Cf, Ff = str(tmp_path / "R.tsv"), str(tmp_path / "C.tsv"), str(tmp_path / "F.tsv")
    plain, _, _ = search(family, tmp_path, "plain", ["-q"])
    _, before, _ = search(family, tmp_path, "before", ["-q", "--ref-stats", Rf, "--ref-stats-cooccur", Cf] + s)
    open(tmp_path / "plain.tsv", "w").write(plain)
    run([TOOL] + t + T_FLAGS + ["--recount", tmp_path / "tool.tsv", tmp_path / "plain.tsv"])
    want = open(tmp_path / "tool.tsv").read()
    run([TOOL] + t + T_FLAGS + ["--no-amb-corr", "--recount", tmp_path / "tool0.tsv", tmp_path / "plain.tsv"])
    want0 = open(tmp_path / "tool0.tsv").read()
    (n, uniq, corrected), refs = R3.parse(want)
    assert n > 400 and corrected >= 50 and len(refs) >= 15 and want != want0, "the expected file must have something in it"
    compare(want, restated(family, plain, *config), plain.count("\n"))
    compare(want0, restated(family, plain, *config, no_amb_corr=True), plain.count("\n"))

    def check(name, extra=(), env=None, tsv=plain, expect=want):
        got_tsv, files, err = search(family, tmp_path, name, ["--ref-stats", Rf, "--ref-stats-cooccur", Cf, "--ref-stats-recount", Ff] + s + S_FLAGS + list(extra), env=env)
        assert got_tsv == tsv, f"{name}: the search result is what it is without the new flag"
        assert files["--ref-stats"] == before["--ref-stats"] and files["--ref-stats-cooccur"] == before["--ref-stats-cooccur"], f"{name}: R and C are what they are without it"
        assert files["--ref-stats-recount"] == expect, name
        m = re.search(r"(\d+) reads recounted, (\d+) of them replayed \((\d+) on the host, (\d+) for want of log room\), (\d+) corrected", err)
        assert m, err
        return [int(x) for x in m.groups()]

    recounted, replayed, host, full, corr = check("one batch")
    assert (recounted, corr) == (n, corrected) and 0 < replayed < recounted and full == 0 and host < replayed
    check("no-amb-corr", ["-q", "--ref-stats-no-amb-corr"], expect=want0)
    if config is not CONFIGS[0]:
        return
    check("batches and threads", ["-q", "-j", "4", "--gpu-batch", "300"])
    dump, tmap = family["tax"][config[0]]  # --specific-level beside it: the TSV is the filtered one, the three files are those of the unfiltered run
    filtered, _, _ = search(family, tmp_path, "filtered", ["-q", "--specific-level", "species", "--taxid-map", tmap, "--taxdump", dump])
    assert 50 < filtered.count("\n") < plain.count("\n") - 50
    check("with K4", ["-q", "--gpu-batch", "300", "--specific-level", "species"], tsv=filtered)
    # every read to the host half, no K3 at all, and a log of a few KiB: the same file
    for knob in ("KMCPG_RECOUNT_DEVICE", "KMCPG_DEVICE_FINALIZE"):
        recounted, replayed, host, full, corr = check(knob, env=dict(os.environ, **{knob: "0"}))
        assert host >= recounted == n and full == 0
    _, _, host, full, _ = check("a log of 4 KiB", env=dict(os.environ, KMCPG_RECOUNT_LOG_BYTES="4096"))
    assert full > 0 and host >= full
    check("the smallest --ref-stats-recount-log-mb", ["-q", "--ref-stats-recount-log-mb", "1"])
    # .gz is honoured
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", tmp_path / "gz.tsv", "-q", "--ref-stats", Rf, "--ref-stats-cooccur", Cf, "--ref-stats-recount", Ff + ".gz"] + s + S_FLAGS)
    assert gzip.open(Ff + ".gz", "rt").read() == want


# ---- the library ----
def stage12(db, family, names, target, n, p_min):
    """stages 1 and 2 as the library counted them -> (classes RECOUNT_CLASS_DTYPE, pairs COOCCUR_DTYPE)"""
    from kmcp_amd import lib
    cols, _ = db.refstats_read(n)
    g = cols.view(np.uint64).reshape(n, 4)
    classes = np.zeros(int(target.max()) + 1, dtype=lib.RECOUNT_CLASS_DTYPE)
    for t in range(len(classes)):
        mine = np.flatnonzero(target == t)
        chunks = db.col_info(int(mine[0]))[1] >> 16
        reads, ureads, hic = int(g[mine, 1].sum()), int(g[mine, 2].sum()), int(g[mine, 3].sum())
        classes[t] = (int(ureads >= 1 and hic >= 1 and float((g[mine, 0] > 0).sum()) / float(chunks) >= p_min), 0, reads, ureads)
    pairs, _ = db.cooccur_read()
    return classes, pairs


def test_library_replays_what_the_host_half_replays_and_changes_no_result(family, monkeypatch):
    """every form — records, pairs, three tickets in flight, with K4, K6 + K7 + K8 together and K8 alone — gives the bytes of the host-only
    form, whose replay is recount_rule.hpp's generic code and not the kernel's; the long query above the -f bound is logged by the host half"""
    from kmcp_amd import Database, default_params, lib
    reads = family["reads"] + [family["long_query"]]
    p = default_params(min_qcov=MIN_QCOV)
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        plain, plain_p = db.search(reads, params=p), db.search_pairs(reads, params=p)
        assert plain.qkmers[-1] > 512 and len(plain.read(len(reads) - 1)) > 0
        db.set_refstats(target, species, hic_min_qcov=0.8)
        db.set_cooccur(target)
        db.set_recount(target, species, hic_min_qcov=0.8)
        res = db.search(reads, params=p)
        assert all(np.array_equal(getattr(res, f), getattr(plain, f)) for f in ("qlen", "qkmers", "offs", "matches")), "the result changed"
        classes, pairs = stage12(db, family, names, target, n, 1.0)
        assert 5 < int(classes["kept"].sum()) < len(classes) and len(pairs) > 10
        kw = dict(min_dreads_prop=D, max_mismatch_err=R)
        db.recount_run(classes, pairs, **kw)
        together, tot_together = db.recount_read()
        k6, _ = db.refstats_read(n)
        k7, _ = db.cooccur_read()
        assert tot_together["corrected_reads"] >= 50 and tot_together["host_reads"] >= 1 and tot_together["left_full"] == 0 and tot_together["logged_reads"] > 100
        # K6 and K7 alone count what they counted beside K8
        db.set_recount()
        db.refstats_reset()
        db.cooccur_reset()
        db.search(reads, params=p)
        assert db.refstats_read(n)[0].tobytes() == k6.tobytes() and db.cooccur_read()[0].tobytes() == k7.tobytes()
        db.set_refstats()
        db.set_cooccur()
        db.set_recount(target, species, hic_min_qcov=0.8)
        for form in ("records", "pairs", "tickets", "with K4", "host only", "no K3", "a log of 4 KiB"):
            db.recount_reset()
            if form == "records":
                res = db.search(reads, params=p)
                assert np.array_equal(res.matches, plain.matches)
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
                monkeypatch.setenv("KMCPG_RECOUNT_DEVICE", "0")
                res = db.search(reads, params=p)
                monkeypatch.delenv("KMCPG_RECOUNT_DEVICE")
                assert np.array_equal(res.matches, plain.matches)
            elif form == "no K3":
                monkeypatch.setenv("KMCPG_DEVICE_FINALIZE", "0")
                with Database.open(family["db_dir"], device=0) as db2:
                    db2.set_recount(target, species, hic_min_qcov=0.8)
                    res = db2.search(reads, params=p)
                    db2.recount_run(classes, pairs, **kw)
                    got, tot = db2.recount_read()
                monkeypatch.delenv("KMCPG_DEVICE_FINALIZE")
                assert np.array_equal(res.matches, plain.matches) and tot["logged_reads"] == 0 and tot["single_reads"] == 0
            else:
                db.set_recount(target, species, hic_min_qcov=0.8, log_bytes=4096)
                res = db.search(reads, params=p)
                assert np.array_equal(res.matches, plain.matches)
            if form != "no K3":
                db.recount_run(classes, pairs, **kw)
                got, tot = db.recount_read()
            assert got.tobytes() == together.tobytes(), form
            assert {k: tot[k] for k in ("recounted_reads", "unique_reads", "corrected_reads")} == {k: tot_together[k] for k in ("recounted_reads", "unique_reads", "corrected_reads")}, (form, tot)
            if form in ("host only", "no K3"):
                assert tot["host_reads"] == tot["replayed_reads"] >= tot["recounted_reads"] and tot["logged_reads"] == 0, (form, tot)
            elif form == "a log of 4 KiB":
                assert tot["left_full"] > 0 and tot["log_bytes"] == 4096 and tot["log_bytes_used"] <= 4096 and tot["host_reads"] > tot["left_full"], tot
                db.set_recount(target, species, hic_min_qcov=0.8)
            else:
                assert tot["left_full"] == 0 and tot["host_reads"] >= 1 and tot["logged_reads"] == tot_together["logged_reads"], (form, tot)
        st, _ = db.last_recount()
        assert st["bad_segments"] == 0 and st["skipped"] == 0
        # other parameters need no new search; without the correction nothing is corrected
        db.search(reads, params=p)  # (the last form set the stage anew: its logs were empty)
        db.recount_run(classes, pairs, no_amb_corr=True)
        other, tot = db.recount_read()
        assert tot["corrected_reads"] == 0 and other.tobytes() != together.tobytes() and int(other["match"].sum()) > int(together["match"].sum())
        db.recount_run(classes, pairs, **kw)
        assert db.recount_read()[0].tobytes() == together.tobytes()
        # what the stage refuses while it is on
        from kmcp_amd.lib import KmcpGpuError
        for bad in (dict(try_se=1), dict(top_n_scores=1)):
            with pytest.raises(KmcpGpuError, match="kmcpg_set_recount"):
                db.search(reads[:10], params=default_params(**bad))
        db.set_recount()
        again = db.search(reads, params=p)
        assert np.array_equal(again.matches, plain.matches)


def test_a_batch_that_is_run_again_is_logged_once(oracle_lib, tmp_path):
    """40 close relatives (the database of the same test of tests/test_gpu_refstats.py): the first attempt overflows its hit buffer and
    collect() runs the batch again — the log holds every read once, and the handle counts one launch that left the work to the rerun"""
    from kmcp_amd import Database, default_params, lib
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
        classes = np.zeros(40, dtype=lib.RECOUNT_CLASS_DTYPE)
        classes["kept"], classes["reads"], classes["ureads"] = 1, 1400, np.arange(40) * 30
        none = np.zeros(0, dtype=lib.COOCCUR_DTYPE)
        db.set_recount(target, None, hic_min_qcov=0.75)
        res = db.search(reads, params=default_params())
        assert len(res.matches) > 8 * len(reads) + 1024, "more matches than the first attempt's hit buffer holds"
        matched = int((np.diff(res.offs) > 0).sum())
        db.recount_run(classes, none, level_species=False)
        got, tot = db.recount_read()
        assert tot["skipped_launches"] == 1 and tot["recounted_reads"] == matched and tot["logged_reads"] + tot["single_reads"] + tot["host_reads"] == matched, tot
        assert tot["corrected_reads"] > 1000 and tot["left_full"] == 0
        st, _ = db.last_recount()
        assert st["skipped"] == 0 and st["logged"] == tot["logged_reads"]  # (the witness is of the rerun, the last launch)
        # ... and the host half replays the same reads to the same counters
        os.environ["KMCPG_RECOUNT_DEVICE"] = "0"
        try:
            db.recount_reset()
            db.search(reads, params=default_params())
        finally:
            os.environ.pop("KMCPG_RECOUNT_DEVICE")
        db.recount_run(classes, none, level_species=False)
        host, tot_h = db.recount_read()
        assert host.tobytes() == got.tobytes() and tot_h["host_reads"] == matched and tot_h["corrected_reads"] == tot["corrected_reads"]
