"""Abundance estimation end to end: K9 inside `kmcp-search --ref-stats R --ref-stats-cooccur C --ref-stats-recount F --ref-stats-profile P`
and the library loop over kmcpg_em_pass, on the family database, reads and taxonomy of tests/test_gpu_recount.py (its helpers are
imported, the file is not touched), with the R = 0.9 that makes stage 3's correction act.  P must be, byte for byte, what
`kmcp-refstats ... --profile` writes from the same command's TSV; the TSV, R, C and F are what they are without the flag; and the loop
written in Python over Database.em_pass / em_read (tests/em_reference.py: run, finish, table) gives the same table.

800 reads over 51 references support few references at the presets' thresholds: the configuration is species level at mode 1 with
--ref-stats-min-chunks-fraction 0, which leaves the loop several references to share the reads among."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import em_reference as E
from tests.test_gpu_cli import CLI
from tests.test_gpu_recount import D, R, S_FLAGS, T_FLAGS, search as search8, stage12
from tests.test_gpu_refstats import MIN_QCOV, TOOL, family, flags, run, tables  # noqa: F401 (family: the fixture)

pytestmark = pytest.mark.gpu

CONFIG = ("B", "species", 1, None, 0.0)
MODE1 = dict(r=5, u=2, U=1, P=0.1, p=0.0, d=2.0, norm="mean")  # refstats_rule.hpp: the preset of mode 1 (H = 0.7), with p = 0


def head(text):
    lines = text.splitlines()
    return int(lines[0].split(": ")[1]), int(lines[1].split(": ")[1]), lines[2].split(": ")[1], [l.split("\t")[0] for l in lines[4:]]


def test_cli_equals_kmcp_refstats_and_leaves_the_other_files_alone(family, tmp_path):
    s, t = flags(family, *CONFIG)
    Rf, Cf, Ff, Pf = (str(tmp_path / f"{x}.tsv") for x in "RCFP")
    base = ["--ref-stats", Rf, "--ref-stats-cooccur", Cf, "--ref-stats-recount", Ff] + s + S_FLAGS
    plain, before, _ = search8(family, tmp_path, "before", ["-q"] + base)
    open(tmp_path / "plain.tsv", "w").write(plain)

    def check(name, extra=(), tool_extra=(), env=None):
        tsv, files, err = search8(family, tmp_path, name, base + ["--ref-stats-profile", Pf] + list(extra), env=env)
        assert tsv == plain and files == before, f"{name}: the TSV, R, C and F are what they are without the flag"
        run([TOOL] + t + T_FLAGS + list(tool_extra) + ["-o", tmp_path / "s1.tsv", "--profile", tmp_path / "tool.tsv", tmp_path / "plain.tsv"])
        want = open(tmp_path / "tool.tsv").read()
        assert open(Pf).read() == want, name
        m = re.search(r"(\d+) EM passes \((converged|not converged)\), (\d+) reads assigned in the last, (\d+) of them split \((\d+) from the host log\)", err)
        assert m, err
        assigned, passes, converged, names = head(want)
        assert (int(m.group(1)), m.group(2) == "converged", int(m.group(3))) == (passes, converged == "yes", assigned)
        return want, int(m.group(4)), int(m.group(5))

    want, split, host = check("defaults")
    assigned, passes, converged, names = head(want)
    print(want)
    assert len(names) >= 3 and passes >= 2 and assigned > 300 and split > 50, "the expected table must have something in it"
    pct = [float(l.split("\t")[1]) for l in want.splitlines()[4:]]
    assert abs(sum(pct) - 100) < 1e-3 and pct == sorted(pct, reverse=True)
    one, _, _ = check("one iteration, a filter", ["-q", "--ref-stats-abund-max-iters", 1, "--ref-stats-filter-low-pct", 5], ["-I", 1, "-F", 5])
    assert head(one)[1] == 2 and len(head(one)[3]) < len(names)
    check("a threshold nothing gets under", ["-q", "--ref-stats-abund-pct-threshold", 1e-13, "-j", "4", "--gpu-batch", "300"], ["--abund-pct-threshold", 1e-13])
    # every read to the host half, a log of a few KiB, an LDS table: the same file
    _, split_h, host_h = check("host only", env=dict(os.environ, KMCPG_RECOUNT_DEVICE="0"))
    assert host_h >= split_h == split
    _, _, host_s = check("a log of 4 KiB", env=dict(os.environ, KMCPG_RECOUNT_LOG_BYTES="4096"))
    assert host_s > host
    check("an LDS table", env=dict(os.environ, KMCPG_EM_SLOTS="1024"))
    check("plain atomics", env=dict(os.environ, KMCPG_EM_SLOTS="0"))


def test_the_library_loop_in_python_gives_the_same_table(family, tmp_path):
    from kmcp_amd import Database, default_params, lib
    s, t = flags(family, *CONFIG)
    reads = family["reads"]
    p = default_params(min_qcov=MIN_QCOV)
    th = MODE1
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        H = 0.7  # mode 1
        db.set_refstats(target, species, hic_min_qcov=H)
        db.set_cooccur(target)
        db.set_recount(target, species, hic_min_qcov=H)
        res = db.search(reads, params=p)
        classes3, pairs = stage12(db, family, names, target, n, th["p"])
        db.recount_run(classes3, pairs, min_dreads_prop=D, max_mismatch_err=R)
        cols3, _ = db.recount_read()
        info = [db.col_info(c) for c in range(n)]
        # the search result as a TSV, for the tool
        lines = []
        for r in range(len(res.offs) - 1):
            for m in res.read(r):
                name, tidx, gsize, _ = info[int(m["col"])]
                lines.append("\t".join([f"q{r}", str(res.qlen[r]), str(res.qkmers[r]), "0", "1", name, str(tidx & 0xffff), str(tidx >> 16), str(gsize), "21",
                                        str(int(m["mkmers"])), "%.4f" % (int(m["mkmers"]) / int(res.qkmers[r])), "0", "0", str(r)]))
        (tmp_path / "lib.tsv").write_text("\n".join(lines) + "\n")
        run([TOOL] + t + T_FLAGS + ["-o", tmp_path / "s1.tsv", "--profile", tmp_path / "tool.tsv", tmp_path / "lib.tsv"])
        want = open(tmp_path / "tool.tsv").read()
        # stage 3's references -> the loop's classes: a chunk table, a reference's chunks side by side
        n_classes = int(target.max()) + 1
        classes, est, cov, chunk_of, n_chunks = [], [], [], {}, 0
        for k in range(n_classes):
            mine = [int(c) for c in np.flatnonzero(target == k)]
            chunks, tlen = info[mine[0]][1] >> 16, info[mine[0]][2]
            w = [[0] * 4 for _ in range(chunks)]
            for c in mine:
                for j, f in enumerate(("match", "uniq", "hic", "bases")):
                    w[info[c][1] & 0xffff][j] += int(cols3[c][f])
                chunk_of[c] = n_chunks + (info[c][1] & 0xffff)
            from tests.test_em_cpu import rollup3
            ok, cv = rollup3(w, tlen, th)
            classes.append(dict(columns=list(range(n_chunks, n_chunks + chunks)), tlen=tlen, name=names[mine[0]]))
            est.append(int(ok))
            cov.append(cv)
            n_chunks += chunks

        def do_pass(e, cv):
            c = np.zeros(n_classes, dtype=lib.EM_CLASS_DTYPE)
            c["est"], c["coverage"] = e, cv
            db.em_pass(c, level_species=True)
            got, tot = db.em_read()
            table = [[0] * 6 for _ in range(n_chunks)]
            for col in range(n):
                for j, f in enumerate(("match", "uniq", "hic", "single_bases", "bases_lo", "bases_hi")):
                    table[chunk_of[col]][j] += int(got[col][f])
            assert int(got["match"].sum()) == tot["assigned_reads"] * E.EM_UNIT  # the conservation law
            return table, tot["assigned_reads"]
        out = E.run(classes, est, cov, th, do_pass)
        assert E.table(classes, out, E.finish(classes, out)) == want
        assert len(head(want)[3]) >= 3 and out["passes"] >= 2


def test_refusals(family, tmp_path):
    s, _ = flags(family, *CONFIG)
    Rf, Cf, Ff, Pf, out = (str(tmp_path / f"{x}.tsv") for x in "RCFPo")
    front = [CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", out]
    three = ["--ref-stats", Rf, "--ref-stats-cooccur", Cf, "--ref-stats-recount", Ff]
    for args, word in ((["--ref-stats", Rf, "--ref-stats-cooccur", Cf, "--ref-stats-profile", Pf], "--ref-stats-recount"), (["--ref-stats", Rf, "--ref-stats-profile", Pf], "--ref-stats-recount"),
                       (three + ["--ref-stats-abund-max-iters", 3], "--ref-stats-profile"), (three + ["--ref-stats-filter-low-pct", 3], "--ref-stats-profile"),
                       (three + ["--ref-stats-profile", Ff], "recount's file"), (three + ["--ref-stats-profile", out], "search result"),
                       (three + ["--ref-stats-profile", Rf], "statistics file"), (three + ["--ref-stats-profile", Cf], "pairs' file"),
                       (three + ["--ref-stats-profile", Pf, "--ref-stats-abund-max-iters", 0], "abund-max-iters"),
                       (three + ["--ref-stats-profile", Pf, "--ref-stats-abund-pct-threshold", 0], "abund-pct-threshold"),
                       (three + ["--ref-stats-profile", Pf, "--ref-stats-filter-low-pct", 100], "filter-low-pct")):
        r = subprocess.run([str(x) for x in front + s + args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 255 and word in r.stderr, (args, r.returncode, r.stderr)
        assert not any(os.path.exists(f) for f in (Rf, Cf, Ff, Pf, out)), "refused before a file is touched"
