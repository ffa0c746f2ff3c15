"""kmcp-search --regions-bed: what is refused is refused before a file is opened or a GPU touched — status 255, the flag named, no output
file.  (None of these runs gets as far as a database: the -d directory and the input do not exist.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
SLIDING = ["--sliding-step", "10", "--sliding-window", "100"]
LEVEL = ["--specific-level", "strain"]


def run(tmp_path, args):
    if not os.path.exists(CLI):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # a GPU, were it asked for, would not be there
    return subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq")] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=60, env=env)


def refused(tmp_path, args, *words):
    bed = tmp_path / "out.bed"
    r = run(tmp_path, [a if a != "BED" else bed for a in args])
    assert r.returncode == 255, (r.returncode, r.stderr)
    last = r.stderr.strip().splitlines()[-1]
    for w in words:
        assert w in last, (w, r.stderr)
    assert "no-such" not in r.stderr, r.stderr  # neither the database nor the input was looked at
    assert r.stdout == "" and not bed.exists() and not (tmp_path / "out.tsv").exists()


def test_what_regions_bed_needs(tmp_path):
    refused(tmp_path, ["--regions-bed", "BED"] + SLIDING, "--regions-bed", "--specific-level")
    refused(tmp_path, ["--regions-bed", "BED"] + LEVEL, "--regions-bed", "--sliding-step", "--sliding-window")
    refused(tmp_path, ["--regions-bed", "BED"], "--regions-bed", "--specific-level")
    refused(tmp_path, ["--regions-bed", "BED", "--sliding-step", "10"] + LEVEL, "--sliding-step and --sliding-window are needed together")
    refused(tmp_path, ["--regions-bed", "BED", "-o", tmp_path / "out.tsv"] + LEVEL + SLIDING, "-o/--out-file", "--regions-bed")
    refused(tmp_path, ["--regions-bed", "BED", "--out-file", "-"] + LEVEL + SLIDING, "-o/--out-file", "--regions-bed")


REGION_FLAGS = [["--regions-min-overlap", "20"], ["--regions-max-gap", "5"], ["--regions-ignore-type"], ["--regions-name-species", "s"], ["--regions-name-assembly", "a"]]


@pytest.mark.parametrize("flag", REGION_FLAGS, ids=[f[0] for f in REGION_FLAGS])
def test_region_flags_alone(tmp_path, flag):
    refused(tmp_path, flag, flag[0], "only used with --regions-bed")
    refused(tmp_path, flag + LEVEL, flag[0], "only used with --regions-bed")


def test_values(tmp_path):
    ok = ["--regions-bed", "BED"] + LEVEL + SLIDING
    refused(tmp_path, ok + ["--regions-min-overlap", "0"], "--regions-min-overlap", "positive")
    refused(tmp_path, ok + ["--regions-min-overlap", "-3"], "--regions-min-overlap", "positive")
    refused(tmp_path, ok + ["--regions-max-gap", "-1"], "--regions-max-gap", "negative")
    refused(tmp_path, ok + ["--regions-min-overlap", "x"], "invalid argument", "regions-min-overlap")


def test_specific_level_with_windows_stays_refused_without_regions_bed(tmp_path):
    refused(tmp_path, LEVEL + SLIDING, "--sliding-", "--specific-level")
    refused(tmp_path, LEVEL + SLIDING + ["--regions-ignore-type"], "--sliding-", "--specific-level")  # the existing check comes first


# every flag --specific-level and --sliding-* refuse: unchanged with --regions-bed
CLASHES = [
    (["-K"], ("-K/--keep-unmatched", "--specific-level")),
    (["--try-se"], ("--try-se", "--specific-level")),
    (["-n", "2"], ("-n/--keep-top-scores", "--specific-level")),
    (["--gpus", "2"], ("--gpus/--gpu-ids", "--specific-level")),
    (["--gpu-ids", "0,1"], ("--gpus/--gpu-ids", "--specific-level")),
    (["--gpu-passes", "2"], ("--gpu-passes", "--specific-level")),
    (["-1", "a.fq", "-2", "b.fq"], ("--sliding-step/--sliding-window", "paired-end")),
    (["-g"], ("--sliding-step/--sliding-window", "-g/--query-whole-file")),
    (["-G"], ("--sliding-step/--sliding-window", "-G/--use-filename")),
    (["--query-id", "x"], ("--sliding-step/--sliding-window", "--query-id")),
    (["--also-db", "other-db"], ("--sliding-", "--also-db")),
]


@pytest.mark.parametrize("extra,words", CLASHES, ids=[" ".join(c[0]) for c in CLASHES])
def test_flags_that_cannot_be_combined(tmp_path, extra, words):
    refused(tmp_path, ["--regions-bed", "BED", "--regions-min-overlap", "20"] + LEVEL + SLIDING + extra, *words)


def test_the_accepted_form_gets_as_far_as_the_input(tmp_path):
    """not refused by the flag checks: it fails later, on the input file that does not exist, and leaves no BED behind"""
    bed = tmp_path / "o.bed"
    r = run(tmp_path, ["--regions-bed", bed, "--regions-min-overlap", 20, "--regions-max-gap", 0, "--regions-ignore-type", "--regions-name-species", "S",
                       "--regions-name-assembly", "A"] + LEVEL + SLIDING)
    assert r.returncode == 255 and "no-such-reads.fq" in r.stderr and not bed.exists()
