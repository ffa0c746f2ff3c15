"""kmcp-search --ref-stats-only: what is refused is refused before a file is opened or a GPU touched — status 255, the flag named, and
nothing created on disk.  (None of these runs gets as far as a database: the -d directory and the input do not exist.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")


def run(tmp_path, args):
    if not os.path.exists(CLI):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # a GPU, were it asked for, would not be there
    return subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq")] + [str(a) for a in args], capture_output=True, text=True, timeout=60, env=env)


def refused(tmp_path, args, *words):
    r = run(tmp_path, args)
    assert r.returncode == 255, (r.returncode, r.stderr)
    last = r.stderr.strip().splitlines()[-1]
    for w in words:
        assert w in last, (w, r.stderr)
    assert "no-such" not in r.stderr, r.stderr  # neither the database nor the input was looked at
    assert r.stdout == "" and os.listdir(tmp_path) == [], os.listdir(tmp_path)


def test_refusals(tmp_path):
    R, C, F, P = (tmp_path / f"{x}.tsv" for x in "RCFP")
    on = ["--ref-stats", R, "--ref-stats-only"]
    four = on + ["--ref-stats-cooccur", C, "--ref-stats-recount", F, "--ref-stats-profile", P]
    # without --ref-stats: nothing to count
    refused(tmp_path, ["--ref-stats-only"], "--ref-stats-only", "only used with --ref-stats")
    refused(tmp_path, ["--ref-stats-only", "-o", tmp_path / "out.tsv"], "--ref-stats-only", "only used with --ref-stats")
    for base in (on, four):
        # no search result is written: nothing that names one, filters one, cuts one into regions, merges several, or reads whole files
        refused(tmp_path, base + ["-o", tmp_path / "out.tsv"], "-o/--out-file", "--ref-stats-only", "no search result is written")
        refused(tmp_path, base + ["--out-file", tmp_path / "out.tsv.gz"], "-o/--out-file", "--ref-stats-only")
        refused(tmp_path, base + ["--specific-level", "strain"], "--specific-level", "--ref-stats-only")
        refused(tmp_path, base + ["--regions-bed", tmp_path / "r.bed"], "--regions-bed", "--ref-stats-only")
        refused(tmp_path, base + ["--also-db", tmp_path / "other-db"], "--also-db", "--ref-stats-only")
        refused(tmp_path, base + ["-g"], "-g/--query-whole-file", "--ref-stats-only")
        # everything --ref-stats refuses
        for extra, word in ((["-K"], "-K/--keep-unmatched"), (["--try-se"], "--try-se"), (["-n", "2"], "-n/--keep-top-scores"),
                            (["--sliding-step", "100", "--sliding-window", "300"], "--sliding-"), (["--gpus", "2"], "--gpus/--gpu-ids"), (["--gpu-passes", "2"], "--gpu-passes")):
            refused(tmp_path, base + extra, word, "--ref-stats")
        refused(tmp_path, base + ["--ref-stats-mode", "0"], "--ref-stats-mode 0", "kmcp-refstats")
    # ... and what the later stages' flags refuse
    refused(tmp_path, on + ["--ref-stats-recount", F], "--ref-stats-recount", "only used with --ref-stats and --ref-stats-cooccur")
    refused(tmp_path, on + ["--ref-stats-cooccur", C, "--ref-stats-profile", P], "--ref-stats-profile", "only used with --ref-stats-recount")
    refused(tmp_path, on + ["--ref-stats-cooccur", R], "--ref-stats-cooccur", "must not be the statistics file")


def test_the_accepted_forms_get_as_far_as_the_input(tmp_path):
    """not refused by the flag checks: they fail later, on the input file that does not exist — and still nothing is created"""
    R, C, F, P = (tmp_path / f"{x}.tsv" for x in "RCFP")
    for args in (["--ref-stats", R, "--ref-stats-only"], ["--ref-stats", R, "--ref-stats-cooccur", C, "--ref-stats-recount", F, "--ref-stats-profile", P, "--ref-stats-only", "-j", "4"]):
        r = run(tmp_path, args)
        assert r.returncode == 255 and "no-such-reads.fq" in r.stderr and os.listdir(tmp_path) == [], (r.stderr, os.listdir(tmp_path))


def test_the_help_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--ref-stats-only" in r.stdout + r.stderr
