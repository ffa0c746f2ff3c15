"""kmcp-search --ref-stats-recount: what is refused is refused before a file is opened or a GPU touched — status 255, the flag named, and
none of the four files written.  (None of these runs gets as far as a database: the -d directory and the input do not exist.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
FILES = ("out.tsv", "stats.tsv", "pairs.tsv", "recount.tsv")


def run(tmp_path, args):
    if not os.path.exists(CLI):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # a GPU, were it asked for, would not be there
    return subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq"), "-o", str(tmp_path / "out.tsv")] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=60, env=env)


def refused(tmp_path, args, *words):
    r = run(tmp_path, args)
    assert r.returncode == 255, (r.returncode, r.stderr)
    last = r.stderr.strip().splitlines()[-1]
    for w in words:
        assert w in last, (w, r.stderr)
    assert "no-such" not in r.stderr, r.stderr  # neither the database nor the input was looked at
    assert r.stdout == "" and not [f for f in FILES if (tmp_path / f).exists()]


def test_refusals(tmp_path):
    out, stats, pairs, rec = (tmp_path / f for f in FILES)
    on = ["--ref-stats", stats, "--ref-stats-cooccur", pairs, "--ref-stats-recount", rec]
    # the optional flags without --ref-stats-recount
    for flag in (["--ref-stats-no-amb-corr"], ["--ref-stats-min-dreads-prop", "0.1"], ["--ref-stats-max-mismatch-err", "0.1"], ["--ref-stats-recount-log-mb", "16"]):
        refused(tmp_path, flag, flag[0], "only used with --ref-stats-recount")
        refused(tmp_path, ["--ref-stats", stats, "--ref-stats-cooccur", pairs] + flag, flag[0], "only used with --ref-stats-recount")
    # --ref-stats-recount without the two stages it starts from
    refused(tmp_path, ["--ref-stats-recount", rec], "--ref-stats-recount", "only used with --ref-stats and --ref-stats-cooccur")
    refused(tmp_path, ["--ref-stats", stats, "--ref-stats-recount", rec], "--ref-stats-recount", "only used with --ref-stats and --ref-stats-cooccur")
    refused(tmp_path, ["--ref-stats-cooccur", pairs, "--ref-stats-recount", rec], "--ref-stats-recount", "only used with --ref-stats and --ref-stats-cooccur")
    # the file is none of the other three
    refused(tmp_path, ["--ref-stats", stats, "--ref-stats-cooccur", pairs, "--ref-stats-recount", out], "--ref-stats-recount", "must not be the search result's file")
    refused(tmp_path, ["--ref-stats", stats, "--ref-stats-cooccur", pairs, "--ref-stats-recount", stats], "--ref-stats-recount", "must not be the statistics file")
    refused(tmp_path, ["--ref-stats", stats, "--ref-stats-cooccur", pairs, "--ref-stats-recount", pairs], "--ref-stats-recount", "must not be the pairs' file")
    # a log size of 0, below it, too large or not a number
    for bad in ("0", "-3", "4097"):
        refused(tmp_path, on + ["--ref-stats-recount-log-mb", bad], "--ref-stats-recount-log-mb", "[1, 4096]")
    refused(tmp_path, on + ["--ref-stats-recount-log-mb", "x"], "invalid argument", "ref-stats-recount-log-mb")
    refused(tmp_path, on + ["--ref-stats-recount-log-mb", "1.5"], "invalid argument", "ref-stats-recount-log-mb")
    # D in (0, 1], R in (0, 1), as kmcp profile has them
    for bad in ("0", "-0.1", "1.01"):
        refused(tmp_path, on + ["--ref-stats-min-dreads-prop", bad], "--ref-stats-min-dreads-prop", "(0, 1]")
    for bad in ("0", "1", "2"):
        refused(tmp_path, on + ["--ref-stats-max-mismatch-err", bad], "--ref-stats-max-mismatch-err", "(0, 1)")
    refused(tmp_path, on + ["--ref-stats-max-mismatch-err", "x"], "invalid argument", "ref-stats-max-mismatch-err")
    # everything --ref-stats refuses
    for extra, word in ((["-K"], "-K/--keep-unmatched"), (["--try-se"], "--try-se"), (["-n", "2"], "-n/--keep-top-scores"),
                        (["--sliding-step", "100", "--sliding-window", "300"], "--sliding-"), (["--gpus", "2"], "--gpus/--gpu-ids"), (["--gpu-passes", "2"], "--gpu-passes")):
        refused(tmp_path, on + extra, word, "--ref-stats")
    refused(tmp_path, on + ["--ref-stats-mode", "0"], "--ref-stats-mode 0", "kmcp-refstats")


@pytest.mark.parametrize("extra", [[], ["--ref-stats-no-amb-corr"], ["--ref-stats-min-dreads-prop", "1", "--ref-stats-max-mismatch-err", "0.99", "--ref-stats-recount-log-mb", "1"],
                                   ["--ref-stats-recount-log-mb", "4096", "--ref-stats-level", "strain", "--ref-stats-mode", "1"]], ids=["plain", "no-amb-corr", "D R log", "largest log"])
def test_the_accepted_forms_get_as_far_as_the_input(tmp_path, extra):
    """not refused by the flag checks: they fail later, on the input file that does not exist"""
    r = run(tmp_path, ["--ref-stats", tmp_path / "stats.tsv", "--ref-stats-cooccur", tmp_path / "pairs.tsv", "--ref-stats-recount", tmp_path / "recount.tsv"] + extra)
    assert r.returncode == 255 and "no-such-reads.fq" in r.stderr and not [f for f in FILES if (tmp_path / f).exists()]


def test_the_help_names_the_flags(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    for flag in ("--ref-stats-recount", "--ref-stats-no-amb-corr", "--ref-stats-min-dreads-prop", "--ref-stats-max-mismatch-err", "--ref-stats-recount-log-mb"):
        assert flag in r.stdout + r.stderr
