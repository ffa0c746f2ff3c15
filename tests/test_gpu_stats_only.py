"""Statistics-only search end to end: kmcpg_submit_stats / kmcpg_wait_stats (K10 behind the counting stages, kmcp_amd/csrc/k10_left.hip)
and `kmcp-search --ref-stats ... --ref-stats-only`, on the family database, reads and taxonomy of tests/test_gpu_recount.py /
test_gpu_profile.py (their helpers are imported, the files are not touched).

The contract: whatever the counting stages report after a statistics-only search — refstats_read, cooccur_read, recount_read after the same
recount_run, em_read after the same em_pass — is byte for byte what they report on a fresh handle after the same reads went through
search (pairs and all); the CLI's R, C, F and P are the bytes of the run without the flag, and no other file appears.  What left the GPU is
bounded: bytes_d2h <= 9 n + 256 without a LEFT read, <= 17 n + 256 + 8 left_pairs with one (include/kmcp_gpu.h)."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_cli import CLI
from tests.test_gpu_recount import D, R, S_FLAGS, stage12
from tests.test_gpu_refstats import MIN_QCOV, family, flags, run, tables  # noqa: F401 (family: the fixture)

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6
CONFIG = ("B", "species", 1, None, 0.0)  # tests/test_gpu_profile.py: the configuration that leaves the EM several references
KNOBS = ("KMCPG_REFSTATS_DEVICE", "KMCPG_COOCCUR_DEVICE", "KMCPG_RECOUNT_DEVICE")


def bound(st):
    return 9 * st["n_reads"] + 256 if st["left_reads"] == 0 else 17 * st["n_reads"] + 256 + 8 * st["left_pairs"]


def stages_on(db, target, species, stages="678", log_bytes=0):
    if "6" in stages:
        db.set_refstats(target, species, hic_min_qcov=0.7)
    if "7" in stages:
        db.set_cooccur(target)
    if "8" in stages:
        db.set_recount(target, species, hic_min_qcov=0.7, log_bytes=log_bytes)


def counted(db, family, names, target, n):
    """everything the four stages report, after the same recount_run and the same em_pass"""
    from kmcp_amd import lib
    k6, t6 = db.refstats_read(n)
    k7, t7 = db.cooccur_read()
    classes, pairs = stage12(db, family, names, target, n, 0.0)
    db.recount_run(classes, pairs, min_dreads_prop=D, max_mismatch_err=R)
    k8, t8 = db.recount_read()
    c = np.zeros(len(classes), dtype=lib.EM_CLASS_DTYPE)
    c["est"], c["coverage"] = classes["kept"], 1.0 + np.arange(len(classes)) % 7
    db.em_pass(c, level_species=True)
    k9, t9 = db.em_read()
    return dict(k6=k6.tobytes(), k7=k7.tobytes(), k8=k8.tobytes(), k9=k9.tobytes(), t6=t6, t7=t7, t8=t8, t9=t9)


def both_routes(family, reads, cuts=None, reads2=None, log_bytes=0):
    """two fresh handles with the three stages on: the reads through search (pairs and all) and through submit_stats / wait_stats (in
    tickets of reads[a:b] for consecutive cuts, two in flight) -> (what the first counted, what the second counted, the tickets' results,
    the pairs result, the second handle's three witnesses of the last batch)"""
    from kmcp_amd import Database, default_params, lib
    p = default_params(min_qcov=MIN_QCOV)
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        stages_on(db, target, species, log_bytes=log_bytes)
        res = db.search_pairs(reads, reads2, params=p)
        want = counted(db, family, names, target, n)
    with Database.open(family["db_dir"], device=0) as db:
        stages_on(db, target, species, log_bytes=log_bytes)
        cuts = cuts or [0, len(reads)]
        out, fl = [], []
        for a, b in zip(cuts, cuts[1:]):
            s, o = lib.pack_reads(reads[a:b])
            s2, o2 = lib.pack_reads(reads2[a:b]) if reads2 is not None else (None, None)
            fl.append(db.submit_stats(s, o, s2, o2, params=p))
            if len(fl) == 2:
                out.append(db.wait_stats(fl.pop(0)))
        out += [db.wait_stats(t) for t in fl]
        ticket, _ = db.last_stats()
        wit = (db.last_refstats()[0], db.last_cooccur()[0], db.last_recount()[0])
        got = counted(db, family, names, target, n)
    assert {k: ticket[k] for k in out[-1]} == out[-1] and ticket["bad_segments"] == 0 and ticket["skipped"] == 0, (ticket, out[-1])
    return want, got, out, res, wit


def flagged(family, reads, p):
    """which reads do the stages flag?  On a handle of its own the batch goes through the GPU half, K3 and the three stages' own device
    entries (what the lane enqueues, each writing its byte per read) -> (every read's length in K3's output, the reads a stage LEFT)"""
    import torch

    from kmcp_amd import Database, lib
    dev = torch.device("cuda", 0)
    seqs, offs = lib.pack_reads(reads)
    n, cap = len(reads), 64 * len(reads) + 4096
    with Database.open(family["db_dir"], device=0) as db:
        names, target, species = tables(db, family, "B")
        stages_on(db, target, species)
        t_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(16, dtype=np.uint8)])).to(dev)
        t_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_hits, d_pairs = torch.empty((cap, 3), dtype=torch.int32, device=dev), torch.empty((cap, 2), dtype=torch.int32, device=dev)
        d_cnt, d_roffs = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(n + 2, dtype=torch.int64, device=dev)
        d_qk, d_ql = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        left = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(3)]
        db.query_device(t_seqs.data_ptr(), t_offs.data_ptr(), n, int(offs[-1]), int(np.diff(offs.astype(np.int64)).max()), d_hits.data_ptr(), cap, d_cnt.data_ptr(),
                        d_qk.data_ptr(), d_ql.data_ptr(), params=p)
        db.group_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_qk.data_ptr(), n, d_pairs.data_ptr(), d_roffs.data_ptr(), params=p)
        kw = dict(d_n_hits=d_cnt.data_ptr(), hit_cap=cap)
        db.refstats_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), n, 512, left[0].data_ptr(), **kw)
        db.cooccur_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), n, 512, left[1].data_ptr(), **kw)
        db.recount_log_device(d_pairs.data_ptr(), d_roffs.data_ptr(), cap, d_qk.data_ptr(), d_ql.data_ptr(), n, 512, left[2].data_ptr(), **kw)
        torch.cuda.synchronize()
        assert int(d_cnt[0]) <= cap
        lens = np.diff(d_roffs.cpu().numpy()[:n + 1])
        any_left = np.zeros(n, dtype=bool)
        for l in left:
            any_left |= l.cpu().numpy() != 0
    return lens, any_left


# which reads find room in a log of a few KiB is decided by the order the waves arrive in: with such a log the totals that say WHERE a
# read was replayed differ from run to run (on either route); every counter that says WHAT was counted does not
WHERE = ("host_reads", "left_full", "log_bytes_used", "logged_reads")


def same(want, got, name, tiny_log=False):
    for k in want:
        w, g = want[k], got[k]
        if tiny_log and k[0] == "t":
            w, g = ({f: v for f, v in x.items() if f not in WHERE} for x in (w, g))
        if tiny_log and k == "t8":  # ... and what the two places hold together does not vary either
            for x in (want[k], got[k]):
                assert x["logged_reads"] + x["host_reads"] == x["replayed_reads"] and x["host_reads"] >= x["left_full"], x
            assert want[k]["host_reads"] - want[k]["left_full"] == got[k]["host_reads"] - got[k]["left_full"], (want[k], got[k])
        assert w == g, f"{name}: {k} differs between the pairs route and the statistics-only route: {w if k[0] == 't' else ''} {g if k[0] == 't' else ''}"


def check_tickets(out, res, name):
    for st in out:
        print(name, st, "bound", bound(st))
        assert st["bytes_d2h"] <= bound(st), (name, st)
        assert st["left_pairs"] <= st["kept_pairs"] and st["left_reads"] <= st["matched_reads"] <= st["n_reads"], (name, st)
    assert sum(st["n_reads"] for st in out) == len(res.offs) - 1


def test_library_counts_what_the_pairs_route_counts(family):
    from kmcp_amd import default_params
    reads = family["reads"] + [family["long_query"]]  # ... and one query above the device's -f bound: the host half counts it
    want, got, out, res, wit = both_routes(family, reads)
    same(want, got, "one ticket")
    check_tickets(out, res, "one ticket")
    (st,) = out
    assert want["t8"]["corrected_reads"] >= 50 and want["t9"]["assigned_reads"] > 300, "the expected state must have something in it"
    assert sum(s["matched_reads"] for s in out) == got["t6"]["matched_reads"]
    # the LEFT reads are exactly those a stage flagged, and their pairs — to the pair — are what came down
    lens, any_left = flagged(family, reads, default_params(min_qcov=MIN_QCOV))
    assert np.array_equal(lens[:-1], np.diff(res.offs.astype(np.int64))[:-1]), "below the -f bound K3's segments are the final rows"
    assert (st["matched_reads"], st["kept_pairs"]) == (int((lens > 0).sum()), int(lens.sum())), (st, int(lens.sum()))
    assert (st["left_reads"], st["left_pairs"]) == (int(any_left.sum()), int(lens[any_left].sum())), (st, int(any_left.sum()), int(lens[any_left].sum()))
    assert any_left[-1], "the long query is above the device's -f bound: every stage leaves it"
    # (one batch in flight: the witnesses are this batch's)
    k6, k7, k8 = wit
    assert max(k6["left"], k7["left"], k8["left"]) <= st["left_reads"] <= k6["left"] + k7["left"] + k8["left"], (st, wit)
    assert 1 <= st["left_reads"] < st["matched_reads"] and 0 < st["left_pairs"] < st["kept_pairs"], st
    assert st["kept_pairs"] >= int(res.offs[-1])  # (K3's total: the host's -f test may still thin out the long query)
    # several tickets, two in flight: the same state, the same sums
    want2, got2, out2, _, _ = both_routes(family, reads, cuts=[0, 300, 301, 600, len(reads)])
    same(want, want2, "the pairs route twice")
    same(want, got2, "four tickets")
    check_tickets(out2, res, "four tickets")
    for k in ("n_reads", "matched_reads", "kept_pairs", "left_reads", "left_pairs"):
        assert sum(s[k] for s in out2) == st[k], k
    assert sum(s["matched_reads"] for s in out2) == got2["t6"]["matched_reads"]


def test_paired_reads(family):
    reads = family["reads"][:400]
    mates = family["reads"][400:800]
    want, got, out, res, _ = both_routes(family, reads, reads2=mates, cuts=[0, 150, 400])
    same(want, got, "pairs of reads")
    check_tickets(out, res, "pairs of reads")


@pytest.mark.parametrize("knobs", [("KMCPG_RECOUNT_DEVICE",), KNOBS, ()], ids=["K8 to the host", "all to the host", "a log of 4 KiB"])
def test_forced_left_paths(family, monkeypatch, knobs):
    reads = family["reads"] + [family["long_query"]]
    for k in knobs:
        monkeypatch.setenv(k, "0")
    log_bytes = 0
    if not knobs:
        monkeypatch.setenv("KMCPG_RECOUNT_LOG_BYTES", "4096")
        log_bytes = 4096
    want, got, out, res, wit = both_routes(family, reads, log_bytes=log_bytes)
    same(want, got, str(knobs), tiny_log=not knobs)
    check_tickets(out, res, str(knobs))
    (st,) = out
    if knobs == ("KMCPG_RECOUNT_DEVICE",):  # every matched read is LEFT for K8, and almost none for another stage: the third mask bit alone
        assert st["left_reads"] == st["matched_reads"] == wit[2]["left"] and st["left_pairs"] == st["kept_pairs"], st
        assert wit[0]["left"] < st["left_reads"] and got["t8"]["host_reads"] >= got["t8"]["recounted_reads"] > 0
    elif knobs == KNOBS:  # all pairs come down
        assert st["left_pairs"] == st["kept_pairs"] and st["left_reads"] == st["matched_reads"], st
        assert got["t6"]["host_reads"] == st["matched_reads"]
    else:
        assert got["t8"]["left_full"] > 0 and wit[2]["left_full"] > 0 and st["left_reads"] >= wit[2]["left_full"], (st, got["t8"])


def relatives(tmp_path):
    """40 close relatives in two chunks each (the database of the rerun tests of tests/test_gpu_cooccur.py / test_gpu_recount.py): every
    read matches dozens of columns of several targets, the reads over the chunks' overlap more than 64; a fresh lane's hit buffer (8 per
    read) overflows on the first attempt"""
    rng = np.random.default_rng(91)
    base = synth.random_genomes(1, 6000, seed=90)[0]
    genomes = []
    for i in range(40):
        g = np.frombuffer(base, dtype=np.uint8).copy()
        m = rng.random(len(g)) < 0.004
        g[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(m.sum()))
        genomes.append(g.tobytes())
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=2, overlap=150, threads=1)
    return db_dir, synth.sample_reads([base], 1500, 150, sub_rate=0.0, seed=200, frac_random=0.1)


def test_a_batch_that_is_run_again_is_counted_once_and_long_segments_of_several_targets(oracle_lib, tmp_path):
    from kmcp_amd import Database, default_params, lib
    db_dir, reads = relatives(tmp_path)
    p = default_params()
    state = []
    for route in ("pairs", "stats"):
        with Database.open(db_dir, device=0) as db:
            n = int(db.info.n_cols)
            names = [db.col_info(c)[0] for c in range(n)]
            ids = {}
            target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
            stages_on(db, target, None)
            if route == "pairs":
                res = db.search_pairs(reads, params=p)
                lens = np.diff(res.offs.astype(np.int64))
                assert int(res.offs[-1]) > 8 * len(reads) + 1024, "more matches than the first attempt's hit buffer holds"
                assert (lens > 64).sum() >= 1, "reads with several targets among more than 64 matches"
            else:
                st = db.wait_stats(db.submit_stats(*lib.pack_reads(reads), params=p))
                print(st, bound(st))
                assert st["bytes_d2h"] <= bound(st) and st["kept_pairs"] == int(res.offs[-1]) and st["matched_reads"] == int((lens > 0).sum()), st
                assert st["left_reads"] >= int((lens > 64).sum()) and st["left_pairs"] >= int(lens[lens > 64].sum()), st
                ticket, _ = db.last_stats()
                assert ticket["skipped"] == 0 and ticket["bad_segments"] == 0  # (the witness is of the rerun)
            k6, t6 = db.refstats_read(n)
            k7, t7 = db.cooccur_read()
            classes = np.zeros(40, dtype=lib.RECOUNT_CLASS_DTYPE)
            classes["kept"], classes["reads"], classes["ureads"] = 1, 1400, np.arange(40) * 30
            db.recount_run(classes, k7, level_species=False)
            k8, t8 = db.recount_read()
            assert t6["skipped_launches"] == 1 and t7["skipped_launches"] == 1 and t8["skipped_launches"] == 1, "the first attempt overflowed and counted nothing"
            state.append(dict(k6=k6.tobytes(), k7=k7.tobytes(), k8=k8.tobytes(), t6=t6, t7=t7, t8=t8))
    same(state[0], state[1], "the rerun")
    assert state[1]["t6"]["matched_reads"] == int((lens > 0).sum())


def test_ticket_refusals(family):
    from kmcp_amd import Database, default_params, lib
    reads = family["reads"][:64]
    p = default_params(min_qcov=MIN_QCOV)
    s, o = lib.pack_reads(reads)
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        with pytest.raises(lib.KmcpGpuError, match="no counting stage") as e:
            db.submit_stats(s, o, params=p)
        assert e.value.code == EINVAL
        assert db.last_stats()[0]["n_reads"] == 0, "nothing ran"
        stages_on(db, target, species, "6")
        t = db.submit_stats(s, o, params=p)
        for wrong in (db.wait, db.wait_pairs, db.wait_summaries):
            with pytest.raises(lib.KmcpGpuError, match="kmcpg_wait_stats") as e:
                wrong(t)
            assert e.value.code == EINVAL
        st = db.wait_stats(t)  # the ticket stayed valid
        assert st["n_reads"] == 64 and st["bytes_d2h"] <= bound(st)
        k6, _ = db.refstats_read(n)
        t = db.submit(s, o, params=p)
        with pytest.raises(lib.KmcpGpuError, match="not one of kmcpg_submit_stats") as e:
            db.wait_stats(t)
        assert e.value.code == EINVAL
        db.wait_pairs(t)
        again, _ = db.refstats_read(n)
        assert again.tobytes() == (2 * k6.view(np.uint64)).tobytes(), "both tickets counted the same reads once each"
        # a K6-only handle: the LEFT reads are exactly the ones K6 flagged
        assert st["left_reads"] == db.last_refstats()[0]["left"]
        db.set_specific(target, species)
        with pytest.raises(lib.KmcpGpuError, match="kmcpg_set_specific") as e:
            db.submit_stats(s, o, params=p)
        assert e.value.code == EINVAL
        db.set_specific()
        for kw in (dict(try_se=1), dict(top_n_scores=1)):
            with pytest.raises(lib.KmcpGpuError, match="kmcpg_set_refstats") as e:
                db.submit_stats(s, o, params=default_params(**kw))
            assert e.value.code == EUNSUPPORTED


def test_needs_k3_on_the_device(family, monkeypatch):
    from kmcp_amd import Database, default_params, lib
    monkeypatch.setenv("KMCPG_DEVICE_FINALIZE", "0")
    with Database.open(family["db_dir"], device=0) as db:
        names, target, species = tables(db, family, "B")
        stages_on(db, target, species, "6")
        with pytest.raises(lib.KmcpGpuError, match="KMCPG_DEVICE_FINALIZE") as e:
            db.submit_stats(*lib.pack_reads(family["reads"][:8]), params=default_params(min_qcov=MIN_QCOV))
        assert e.value.code == EUNSUPPORTED


# ---- the CLI ----
LINE = re.compile(r"^(\d+) reads searched, (\d+) matched; (\d+) reads \((\d+) pairs\) left to the host, (\d+) bytes from the device$", re.M)


def cli(family, d, only, extra=(), gz="", inputs=None):
    """one run in directory d -> ({R, C, F, P: bytes}, the files of d, stderr)"""
    os.makedirs(d, exist_ok=True)
    s, _ = flags(family, *CONFIG)
    files = {x: os.path.join(d, f"{x}.tsv{gz}") for x in "RCFP"}
    cmd = [CLI, "-d", family["root"], "-t", MIN_QCOV] + (inputs or [family["fq"]]) + ["--ref-stats", files["R"], "--ref-stats-cooccur", files["C"], "--ref-stats-recount", files["F"],
                                                                                     "--ref-stats-profile", files["P"]] + s + S_FLAGS + list(extra)
    cmd += ["--ref-stats-only"] if only else ["-o", os.path.join(d, "out.tsv")]
    r = run(cmd)
    return {x: (gzip.open(f).read() if gz else open(f, "rb").read()) for x, f in files.items()}, sorted(os.listdir(d)), r.stderr


@pytest.mark.parametrize("form", ["defaults", "batches and threads", "paired", "gz"])
def test_cli_writes_the_files_of_the_run_without_the_flag(family, tmp_path, form):
    from kmcp_amd import Database, default_params
    extra = ["-q"] if form != "defaults" else []
    gz, inputs = "", None
    if form == "batches and threads":
        extra += ["-j", "4", "--gpu-batch", "300"]
    elif form == "paired":
        inputs = ["-1", family["fq"], "-2", family["fq"]]
    elif form == "gz":
        gz = ".gz"
    want, _, err0 = cli(family, str(tmp_path / "with"), False, extra, gz, inputs)
    got, listing, err = cli(family, str(tmp_path / "only"), True, extra, gz, inputs)
    for x in "RCFP":
        assert got[x] == want[x], f"{form}: {x} differs from the run without --ref-stats-only"
    assert len(want["P"].splitlines()) > 6 and len(want["C"].splitlines()) > 3, "the expected files must have something in them"
    assert listing == sorted(f"{x}.tsv{gz}" for x in "RCFP"), f"{form}: {listing}"
    for stage_line in (r"\d+ reads recounted, \d+ of them replayed", r"\d+ EM passes"):
        assert re.search(stage_line, err) and re.search(stage_line, err).group(0) == re.search(stage_line, err0).group(0), err
    m = LINE.search(err)
    assert m, err
    n, matched, left, left_pairs, nbytes = (int(x) for x in m.groups())
    # the same reads through the library in one ticket: the same counts (the bytes depend on how the reads were cut into batches)
    p = default_params(min_qcov=MIN_QCOV)
    p.fpr_buf_size = 499 if inputs else 249
    with Database.open(family["db_dir"], device=0) as db:
        names, target, species = tables(db, family, "B")
        stages_on(db, target, species)
        st = db.search_stats(family["reads"], family["reads"] if inputs else None, params=p)
        assert db.last_stats()[0]["left_pairs"] == st["left_pairs"]
    assert (n, matched, left, left_pairs) == (st["n_reads"], st["matched_reads"], st["left_reads"], st["left_pairs"]), (m.group(0), st)
    batches = -(-n // 300) if form == "batches and threads" else 8  # (at most: the reader may cut a file into a few batches)
    assert 9 * n < nbytes <= 17 * n + 256 * batches + 8 * left_pairs, (m.group(0), st)


def test_cli_refuses_on_the_gpu_machine_too(family, tmp_path):
    r = subprocess.run([CLI, "-d", family["root"], family["fq"], "--ref-stats", str(tmp_path / "R.tsv"), "--ref-stats-only", "-o", str(tmp_path / "o.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "--ref-stats-only" in r.stderr and os.listdir(tmp_path) == []
