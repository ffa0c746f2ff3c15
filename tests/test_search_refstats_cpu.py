"""kmcp-search --ref-stats: what is refused is refused before a file is opened or a GPU touched — status 255, the flag named, no output
file and no statistics file.  (None of these runs gets as far as a database: the -d directory and the input do not exist.)"""
import os
import subprocess

import pytest

from tests import filter_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")


@pytest.fixture(scope="module")
def tax(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxdump")
    return FC.write_taxdump(d / "dump"), FC.write_map(d / "map.tsv")


def run(tmp_path, args):
    if not os.path.exists(CLI):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # a GPU, were it asked for, would not be there
    return subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq"), "-o", str(tmp_path / "out.tsv")] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=60, env=env)


def refused(tmp_path, args, *words):
    stats = tmp_path / "stats.tsv"
    r = run(tmp_path, [("--ref-stats=" + str(stats)) if a == "--ref-stats=FILE" else a for a in args])
    assert r.returncode == 255, (r.returncode, r.stderr)
    last = r.stderr.strip().splitlines()[-1]
    for w in words:
        assert w in last, (w, r.stderr)
    assert "no-such" not in r.stderr, r.stderr  # neither the database nor the input was looked at
    assert r.stdout == "" and not (tmp_path / "out.tsv").exists() and not stats.exists()


ON = ["--ref-stats=FILE"]
CASES = [
    (["-K"], "-K/--keep-unmatched"),
    (["--try-se"], "--try-se"),
    (["-n", "2"], "-n/--keep-top-scores"),
    (["--sliding-step", "100", "--sliding-window", "300"], "--sliding-"),
    (["--sliding-greedy"], "--sliding-"),
    (["--gpus", "2"], "--gpus/--gpu-ids"),
    (["--gpu-ids", "0,1"], "--gpus/--gpu-ids"),
    (["--gpu-passes", "2"], "--gpu-passes"),
]


@pytest.mark.parametrize("extra,word", CASES, ids=[" ".join(c[0]) for c in CASES])
def test_flags_that_cannot_be_combined(tax, tmp_path, extra, word):
    dump, tmap = tax
    refused(tmp_path, ON + extra, word, "--ref-stats")
    refused(tmp_path, ON + ["--taxid-map", tmap, "--taxdump", dump] + extra, word, "--ref-stats")


def test_modes_and_thresholds(tmp_path):
    refused(tmp_path, ON + ["--ref-stats-mode", "0"], "--ref-stats-mode 0", "kmcp-refstats")
    refused(tmp_path, ON + ["--ref-stats-mode", "6"], "invalid profiling mode: 6")
    refused(tmp_path, ON + ["--ref-stats-mode", "-1"], "invalid profiling mode")
    refused(tmp_path, ON + ["--ref-stats-mode", "x"], "invalid argument", "ref-stats-mode")
    refused(tmp_path, ON + ["--ref-stats-min-chunks-fraction", "1.1"], "--ref-stats-min-chunks-fraction")
    refused(tmp_path, ON + ["--ref-stats-min-chunks-fraction", "-0.1"], "--ref-stats-min-chunks-fraction")
    refused(tmp_path, ON + ["--ref-stats-min-hic-ureads-qcov", "0"], "--ref-stats-min-hic-ureads-qcov")
    refused(tmp_path, ON + ["--ref-stats-min-hic-ureads-qcov", "1.01"], "--ref-stats-min-hic-ureads-qcov")
    # the other flags of the family mean nothing without the file
    for flag in (["--ref-stats-mode", "2"], ["--ref-stats-min-chunks-fraction", "0.5"], ["--ref-stats-min-hic-ureads-qcov", "0.8"], ["--ref-stats-level", "strain"]):
        refused(tmp_path, flag, flag[0], "only used with --ref-stats")
    # the statistics do not go where the result goes
    r = run(tmp_path, ["--ref-stats", str(tmp_path / "out.tsv")])
    assert r.returncode == 255 and "must not be the search result's file" in r.stderr and "no-such" not in r.stderr


def test_level_and_taxonomy_flags(tax, tmp_path):
    dump, tmap = tax
    refused(tmp_path, ON + ["--ref-stats-level", "genus"], "invalid value for --ref-stats-level")
    refused(tmp_path, ON + ["--ref-stats-level", "species"], "--taxid-map", "--taxdump", "are needed for --ref-stats-level species")
    refused(tmp_path, ON + ["--taxid-map", tmap], "--taxdump is needed when --taxid-map given")
    refused(tmp_path, ON + ["--taxdump", dump], "--taxid-map is needed when --taxdump given")
    # what --specific-level refuses stays refused, and is named first
    refused(tmp_path, ON + ["--specific-level", "strain", "-K"], "-K/--keep-unmatched", "--specific-level")
    refused(tmp_path, ["--taxid-map", tmap, "--taxdump", dump], "only used with --specific-level")


@pytest.mark.parametrize("extra", [[], ["--ref-stats-level", "Strain"], ["--ref-stats-mode", "5", "--ref-stats-min-chunks-fraction", "0.3", "--ref-stats-min-hic-ureads-qcov", "1"],
                                   ["--specific-level", "assembly"]], ids=["plain", "level", "thresholds", "with --specific-level"])
def test_the_accepted_forms_get_as_far_as_the_input(tmp_path, extra):
    """not refused by the flag checks: they fail later, on the input file that does not exist"""
    r = run(tmp_path, ["--ref-stats", str(tmp_path / "stats.tsv")] + extra)
    assert r.returncode == 255 and "no-such-reads.fq" in r.stderr and not (tmp_path / "out.tsv").exists() and not (tmp_path / "stats.tsv").exists()


def test_accepted_with_a_taxonomy(tax, tmp_path):
    dump, tmap = tax
    r = run(tmp_path, ["--ref-stats", str(tmp_path / "stats.tsv"), "--taxid-map", tmap, "--taxdump", dump])
    assert r.returncode == 255 and "no-such-reads.fq" in r.stderr
